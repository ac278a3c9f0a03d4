#!/usr/bin/env python3
"""Times the second half of a frame host to host for 1, 64 and 1024 cameras of 640 x 480 with 150 held points a camera and a uint16
depth image a camera, two ways in the same build:

  (a) the path a caller had before gfbe_obs_*: the lists gfbe_det_detect returned are on the host; O3 .. O6 by the host build of
      csrc/gfbe_obs.h on one thread (tests/obs_host_shim.cpp, g++ -O2); gfbe_ftab_add_frame with the rows;
  (b) gfbe_obs_observe with NULL outputs (the depth images are uploaded, nothing but the counters comes back), then gfbe_obs_add_frame;

and both once more with depth_cam == 0 (no depth images, every depth -2.4), which shows what the upload of the depth images costs (b).

Both feed tables of their own with the same frames: repetition r adds frame r of the same ids, so a repetition does the same work on
both sides (the first adds 150 features a table, the later ones 150 observations). After one warm-up frame the two paths and the
three shapes run alternately `--reps` times (at most 9: a feature holds 11 observations); median and max - min of the repetitions.
The calls are made on preallocated arrays through the C ABI, without the binding's per-camera lists. No time is asserted anywhere.
First numbers; nothing is tuned to them. Writes profiles/obs_bench.txt.

    python tools/diag_obs_bench.py [--reps 9] [--out profiles/obs_bench.txt]
"""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _gfbe_import import gf      # noqa: E402

ROWS, COLS, HELD = 480, 640, 150
CAMERA = [605.687407, 607.16452123, 323.35155412, 236.66167004, 0.15860811, -0.34018021, -0.00180768, 0.00032313]      # a distorted PINHOLE model: the lift iterates
PF, PI, PD, PU16 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint16)


def host_shim():
    out = os.path.join(ROOT, "tests", "_build", "obs_host_shim.so")
    src = os.path.join(ROOT, "tests", "obs_host_shim.cpp")
    hdrs = [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_obs.h", "gfbe_klt.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + hdrs):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([os.environ.get("CXX") or shutil.which("g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.shim_obs_observe_all.argtypes = [C.c_int, PD, PI, PF, PI, PI, PI, PF, PD, PU16, C.c_int, C.c_int, PI, PD, PF, PI]
    return lib


class Shape:
    def __init__(self, be, n, shim):
        abi = gf.abi
        self.be, self.n, self.shim = be, n, shim
        rng = np.random.default_rng(n)
        self.t = be.tracker(n, ROWS, COLS, HELD)
        self.t.push_image(np.zeros((n, ROWS, COLS), np.uint8))
        self.cams = np.ascontiguousarray(np.tile(np.array(CAMERA), (n, 1)))
        self.o, self.o0 = be.observer(self.t, self.cams), be.observer(self.t, self.cams, depth_cam=0)
        self.A, self.B, self.A0, self.B0 = [abi.FeatureTables(be.lib, "gfbe_", be.ctx, n, 256) for _ in range(4)]
        self.base = np.stack([rng.uniform(30, COLS - 31, (n, HELD)), rng.uniform(30, ROWS - 31, (n, HELD))], 2).astype(np.float32)
        self.ids = np.ascontiguousarray(np.stack([rng.permutation(HELD) * 3 + 7 for _ in range(n)]).astype(np.int32).ravel())
        self.cnt = np.ones(n * HELD, np.int32)
        self.off = (np.arange(n + 1) * HELD).astype(np.int32)
        self.depth = rng.integers(300, 6000, (n, ROWS, COLS)).astype(np.uint16)
        # outputs and the host path's own previous list
        m = n * HELD
        self.ids_out, self.obs8, self.un = np.zeros(m, np.int32), np.zeros((m, 8)), np.zeros((m, 2), np.float32)
        self.prev = {d: [np.zeros(m, np.int32), np.zeros((m, 2), np.float32), np.zeros(n + 1, np.int32)] for d in (0, 1)}
        self.cn4 = np.zeros((n, 4), np.int32)
        self.kf, self.cn3, self.avg = np.zeros(n, np.int32), np.zeros((n, 3), np.int32), np.zeros(n)
        self.td = np.zeros(n)
        self.times = dict(a=[], b=[], a0=[], b0=[])
        self.frame = 0

    def step(self, record):
        f, n = self.frame, self.n
        pts = np.ascontiguousarray(self.base + np.float32(f))      # the scene moves by one pixel a frame
        self.t.set_points(list(pts), list(self.ids.reshape(n, HELD)), list(self.cnt.reshape(n, HELD)))
        fc = np.full(n, f, np.int32)
        tm, dt = np.full(n, 0.1 * f + 1.0), np.full(n, 0.1 if f else 1.0)
        lib, ctx = self.be.lib, self.be.ctx
        p = lambda a, ty: a.ctypes.data_as(ty)
        for with_depth, tab_a, tab_b, obs, ka, kb in ((1, self.A, self.B, self.o, "a", "b"), (0, self.A0, self.B0, self.o0, "a0", "b0")):
            prev_ids, prev_un, prev_off = self.prev[with_depth]
            dp = p(self.depth, PU16) if with_depth else None
            t0 = time.perf_counter()      # (a)
            self.shim.shim_obs_observe_all(n, p(self.cams, PD), p(self.off, PI), p(pts, PF), p(self.ids, PI), p(prev_off, PI), p(prev_ids, PI), p(prev_un, PF), p(dt, PD),
                                           dp, COLS, ROWS, p(self.ids_out, PI), p(self.obs8, PD), p(self.un, PF), p(self.cn4, PI))
            rc = lib.gfbe_ftab_add_frame(ctx, tab_a.h, p(fc, PI), p(self.off, PI), p(self.ids_out, PI), p(self.obs8, PD), p(self.td, PD), p(self.kf, PI), p(self.cn3, PI), p(self.avg, PD))
            t1 = time.perf_counter()
            assert rc == 0, rc
            host_counts, host_kf = self.cn4.copy(), (self.kf.copy(), self.cn3.copy(), self.avg.copy())
            prev_ids[:], prev_un[:], prev_off[:] = self.ids_out, self.un, self.off
            t2 = time.perf_counter()      # (b)
            rc1 = lib.gfbe_obs_observe(ctx, obs.h, p(tm, PD), dp, None, None, None, p(self.cn4, PI))
            rc2 = lib.gfbe_obs_add_frame(ctx, obs.h, tab_b.h, p(fc, PI), p(self.td, PD), p(self.kf, PI), p(self.cn3, PI), p(self.avg, PD))
            t3 = time.perf_counter()
            assert rc1 == 0 and rc2 == 0, (rc1, rc2)
            assert np.array_equal(host_counts, self.cn4) and all(np.array_equal(x, y) for x, y in zip(host_kf, (self.kf, self.cn3, self.avg))), "the two paths disagree"
            if record:
                self.times[ka].append((t1 - t0) * 1e3)
                self.times[kb].append((t3 - t2) * 1e3)
        self.frame += 1

    def close(self):
        for h in (self.o, self.o0, self.A, self.B, self.A0, self.B0, self.t):
            h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_bench.txt"))
    a = ap.parse_args()
    assert 1 <= a.reps <= 9
    be = gf.Backend(device=0)
    shim = host_shim()
    shapes = (1, 64, 1024)
    runs = {n: Shape(be, n, shim) for n in shapes}
    for n in shapes:
        runs[n].step(False)
    for _ in range(a.reps):
        for n in shapes:
            runs[n].step(True)
    lines = ["the second half of a frame host to host, 640 x 480, %d points and one uint16 depth image a camera, %d alternating repetitions after a warm-up (ms: median, max - min)"
             % (HELD, a.reps),
             "%58s %8s %12s %10s %14s" % ("path", "cameras", "median ms", "spread ms", "ms per camera")]
    for n in shapes:
        for key, label in (("a", "(a) host O3 .. O6 on one thread + gfbe_ftab_add_frame"), ("b", "(b) gfbe_obs_observe (NULL outputs) + gfbe_obs_add_frame"),
                           ("a0", "(a) with depth_cam 0"), ("b0", "(b) with depth_cam 0")):
            ts = runs[n].times[key]
            med = float(np.median(ts))
            lines.append("%58s %8d %12.3f %10.3f %14.4f" % (label, n, med, max(ts) - min(ts), med / n))
    lines.append("(b) uploads the depth images (%d KiB a camera) every frame, the one input of the second half that is not on the device; (a) reads them" % (ROWS * COLS * 2 // 1024))
    lines.append("where they are. Both paths gave the same counters, keyframe decisions and parallax in every repetition. The host build of gfbe_obs.h is")
    lines.append("g++ -O2 on one thread. First numbers, nothing is tuned to them.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    for r in runs.values():
        r.close()
    be.close()


if __name__ == "__main__":
    main()
