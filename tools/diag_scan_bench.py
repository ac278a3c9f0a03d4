#!/usr/bin/env python3
"""Times one LiDAR frame through the device-resident scan handle (gfbe_scan_* + gfbe_vmap_register_scan + gfbe_vmap_add_scan_handle)
against the same frame prepared on the host and uploaded twice (the keypoints for gfbe_vmap_register, the surface set for
gfbe_vmap_add_scan): a 24 000-point scan of the room scene, sub-sampling at 0.05 m, 21 nominal states, keypoints at 0.2 m. The host
preparation is a single-thread C++ restatement (tests/scan_host_shim.cpp: std::unordered_map, the per-point functions of gfbe_scan.h
compiled for the host) with numpy gathers between its steps. Host clock, the two legs alternating on two maps seeded alike, warm,
median and max - min of the repetitions. The handle's stages are timed in a pass of their own with a synchronising gfbe_scan_size
behind each (the frame itself never waits there). Writes profiles/scan_bench.txt.

    python tools/diag_scan_bench.py [--points 24000] [--reps 20] [--out profiles/scan_bench.txt]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _gfbe_import import gf      # noqa: E402
import scan_cases as sc      # noqa: E402

PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int)
SUB, KP = 0.05, 0.2


def _p(a):
    return a.ctypes.data_as(PD)


def build_shim():
    so = os.path.join(ROOT, "tests", "_build", "libscan_host_shim_o3.so")
    src = os.path.join(ROOT, "tests", "scan_host_shim.cpp")
    deps = [src] + [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_scan.h", "gfbe_lio_pose.h", "gfbe_vmap.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-ffp-contract=off", "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.hscan_subsample.argtypes = [C.c_int, PD, C.c_double, PI, PI]
    return lib


def clock():
    return time.perf_counter() * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=24000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_bench.txt"))
    a = ap.parse_args()
    shim = build_shim()
    be = gf.Backend(device=0)
    room = gf.synth_scan.Room(seed=31)
    poses = room.trajectory(2)
    pb, pe = poses[0], poses[1]
    frame = room.scan(pb, pe, a.points, 0.05)
    raw, alpha = np.ascontiguousarray(frame["raw"]), np.ascontiguousarray(frame["alpha"])
    t, P = sc.states(70, 21, t0=10.0, dt=0.005, rot=(1.1e-3, 2e-3))
    P[:, :3] *= 0.02
    ts = np.ascontiguousarray(t[0] + alpha * (t[-1] - t[0]))
    first = room.surface(60000, 0.05)
    va, vb = be.voxel_map(1 << 16), be.voxel_map(1 << 16)
    va.add_points(first)
    vb.add_points(first)
    s = be.scan(a.points)
    o = dict(min_num_residuals=50)
    n = len(raw)
    kept, kept2 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    und, world = np.zeros((n, 3)), np.zeros((n, 3))
    seg, skipped = np.zeros(n, np.int32), C.c_int(0)
    info = {}

    def handle():
        s.upload(raw, alpha, ts)
        s.subsample(SUB)
        s.undistort(t, P)
        info["nkp_dev"] = s.keypoints(1, pb, pe, KP)
        ob, oe, sm = va.register_scan(1, s, pb, pe, pb[:3], pb[3:], False, **o)
        va.add_scan_handle(1, s, ob, oe)
        va.size()      # (the map update does not wait: the size call synchronises, in both legs)
        info["dev"] = (ob, oe, sm)

    def host():
        x = [clock()]
        m = shim.hscan_subsample(n, _p(raw), SUB, kept.ctypes.data_as(PI), C.byref(skipped))
        k = kept[:m]
        p1, a1, t1 = np.ascontiguousarray(raw[k]), np.ascontiguousarray(alpha[k]), np.ascontiguousarray(ts[k])
        shim.shim_scan_undistort(len(t), _p(t), _p(np.ascontiguousarray(P)), m, _p(p1), _p(t1), _p(und), seg.ctypes.data_as(PI))
        p1 = und[:m]
        shim.hscan_world(1, m, _p(p1), _p(a1), _p(pb), _p(pe), _p(world))
        mk = shim.hscan_subsample(m, _p(world), KP, kept2.ctypes.data_as(PI), C.byref(skipped))
        kk = kept2[:mk]
        kp_pts, kp_al = np.ascontiguousarray(p1[kk]), np.ascontiguousarray(a1[kk])
        x.append(clock())
        ob, oe, sm = vb.register(1, kp_pts, kp_al, pb, pe, pb[:3], pb[3:], False, **o)
        x.append(clock())
        vb.add_scan(1, p1, a1, ob, oe)
        vb.size()
        x.append(clock())
        info["host"], info["n_sub"], info["nkp_host"], info["host_parts"] = (ob, oe, sm), m, mk, np.diff(x)

    td, th, parts = [], [], []
    for i in range(a.reps + 2):      # two warm-up rounds
        x0 = clock(); handle(); x1 = clock(); host(); x2 = clock()
        assert info["nkp_dev"] == info["nkp_host"]      # (the host's undistorted points differ from the device's in rounding only)
        assert np.abs(info["dev"][0] - info["host"][0]).max() < 1e-6 and np.abs(info["dev"][1] - info["host"][1]).max() < 1e-6, "the two legs must register alike"
        if i >= 2:
            td.append(x1 - x0); th.append(x2 - x1); parts.append(info["host_parts"])
    # the handle's stages, each with a synchronising size() behind it
    names = ("upload", "subsample", "undistort", "keypoints", "register_scan", "add_scan_handle")
    stage = {k: [] for k in names}
    for i in range(a.reps + 2):
        steps = ((lambda: (s.upload(raw, alpha, ts), s.size())), (lambda: (s.subsample(SUB), s.size())), (lambda: (s.undistort(t, P), s.size())),
                 (lambda: s.keypoints(1, pb, pe, KP)), (lambda: info.__setitem__("r", va.register_scan(1, s, pb, pe, pb[:3], pb[3:], False, **o))),
                 (lambda: (va.add_scan_handle(1, s, info["r"][0], info["r"][1]), va.size())))
        for k, f in zip(names, steps):
            x0 = clock(); f(); x1 = clock()
            if i >= 2:
                stage[k].append(x1 - x0)
    med = lambda v: float(np.median(v))
    spread = lambda v: float(max(v) - min(v))
    parts = np.array(parts)
    sm = info["dev"][2]
    lines = ["one LiDAR frame: %d points, sub-sampling %.2f m -> %d, 21 states, keypoints %.1f m -> %d; %d outer iterations, n_res %d; ms" %
             (n, SUB, info["n_sub"], KP, info["nkp_dev"], sm["outer_iterations"], sm["n_res"][0]),
             "median [max - min] of %d alternating repetitions after two warm-up rounds; host clock" % a.reps, "",
             "handle, end to end (upload .. add_scan_handle, two host waits + the closing size)   %8.3f [%6.3f]" % (med(td), spread(td)),
             "host preparation + register + add_scan (two uploads), end to end                   %8.3f [%6.3f]" % (med(th), spread(th)),
             "  of which: host preparation %.3f, register (keypoints uploaded) %.3f, add_scan (surface set uploaded) %.3f" %
             tuple(float(np.median(parts[:, k])) for k in range(3)), "",
             "handle, stage by stage (each followed by a synchronising gfbe_scan_size / gfbe_vmap_size):"]
    for k in names:
        lines.append("  %-16s %8.3f [%6.3f]" % (k, med(stage[k]), spread(stage[k])))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    s.close(); va.close(); vb.close(); be.close()


if __name__ == "__main__":
    main()
