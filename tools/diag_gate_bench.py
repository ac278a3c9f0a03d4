import os as _os, sys as _sys
_r = _os.path.dirname(_os.path.abspath(__file__))
while not _os.path.exists(_os.path.join(_r, "_gfbe_import.py")):
    _r = _os.path.dirname(_r)
_sys.path[:0] = [_r, _os.path.join(_r, "tests")]   # (measurement scripts: the package root and the test helpers they share)
"""Timing of gfbe_gate_frame (include/gfbe_gate.h) for B = 1, 64 and 1024 robots with 300-feature tables, 20 IMU and 5 wheel samples and 12
frames a robot, against what it replaces: gfbe_ftab_download of every table plus the host build of the same header (tests/gate_host_shim.cpp,
one thread) looped over the robots. Host-call wall time, the wait included; the median of REPS calls after a warm-up. The results of the two
paths are compared byte for byte before anything is timed. Output goes to profiles/gate_bench.txt."""
import os, time
import numpy as np
import gate_cases as gc
import gate_np as m
from _gfbe_import import gf
abi = gf.abi

REPS = int(os.environ.get("REPS", "30"))
be = gf.Backend(device=0)
shim = gc.load_shim()
o = m.options()
rng = np.random.default_rng(3)
tracks = gc.random_tracks(rng, 300, depth=(0.5, 8.0))
kinds = ["moving", "slip", "rest", "turning"]
print("gfbe_gate_frame: 300-feature tables, 20 IMU + 5 wheel samples, 12 frames a robot; median of %d calls, ms" % REPS)
print("%8s %14s %18s %16s %14s %8s" % ("robots", "gate_frame", "download (all)", "host header", "host path", "ratio"))
for B in (1, 64, 1024):
    ft = abi.FeatureTables(be.lib, "gfbe_", be.ctx, B, 512)
    gc.run_script_device(gc.script_of([tracks] * B), ft)
    robots = [gc.robot(rng, 20, 5, 12, kind=kinds[b % 4]) for b in range(B)]
    g = be.sensor_gate(B)
    args = gc.frame_args(robots)

    def device():
        return g.frame(ft, *args)

    def download():
        return [ft.download(w) for w in range(B)]

    def host(packed):
        return gc.shim_frame(shim, o, None, robots, packed)
    got, tabs = device(), download()
    packed = (gc.pack_tables(tabs), gc.pack_robots(robots))
    gc.assert_same(host(packed), got, "device against the host build")
    t = {}
    for name, fn in (("device", device), ("download", download), ("host", lambda: host(packed))):
        fn()
        s = []
        for _ in range(REPS if B < 1024 or name == "device" else max(3, REPS // 10)):
            t0 = time.perf_counter()
            fn()
            s.append(time.perf_counter() - t0)
        t[name] = float(np.median(s)) * 1e3
    print("%8d %14.3f %18.3f %16.3f %14.3f %8.1f" % (B, t["device"], t["download"], t["host"], t["download"] + t["host"], (t["download"] + t["host"]) / t["device"]))
    g.close()
    ft.close()
print("(the device column includes the Python packing of the intervals; the host header column runs on arguments packed beforehand)")
