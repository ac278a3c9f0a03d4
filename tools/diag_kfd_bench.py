#!/usr/bin/env python3
"""Times the descriptors of a keyframe host to host for 1, 64 and 1024 cameras of 640 x 480 (synth.klt_texture, 344 kept
corners a camera), two ways in the same build:

  (a) the path a caller had before gfbe_kfd_*: the keyframe images are on the host; K1 .. K5 by the host build of csrc/gfbe_kfd.h on
      one thread (tests/kfd_host_shim.cpp, g++ -O2), camera after camera; gfbe_ldb_add_keyframe (detecting) with camera 0's lists;
  (b) gfbe_kfd_capture from a tracker that holds the images, gfbe_kfd_extract with NULL outputs (nothing but the counters comes back),
      gfbe_kfd_add_keyframe (detecting) of camera 0.

Both feed a loop database of their own, so a repetition does the same work on both sides. After one warm-up keyframe the two paths and
the three shapes run alternately `--reps` times; median and max - min of the repetitions. The calls are made on preallocated arrays
through the C ABI. No time is asserted anywhere. First numbers; nothing is tuned to them. Writes profiles/kfd_bench.txt.

    python tools/diag_kfd_bench.py [--reps 9] [--out profiles/kfd_bench.txt]
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _gfbe_import import gf      # noqa: E402
import ldb_cases                 # noqa: E402  (the synthetic vocabulary of the loop-database tests)

ROWS, COLS, CAP = 480, 640, 4096
CAMERA = [605.687407, 607.16452123, 323.35155412, 236.66167004, 0.15860811, -0.34018021, -0.00180768, 0.00032313]      # a distorted PINHOLE model: the lift iterates
PF, PI, PD, PU8, PU64 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)


def host_shim():
    out = os.path.join(ROOT, "tests", "_build", "kfd_host_shim.so")
    src = os.path.join(ROOT, "tests", "kfd_host_shim.cpp")
    hdrs = [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_kfd.h", "gfbe_obs.h", "gfbe_klt.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + hdrs):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([os.environ.get("CXX") or shutil.which("g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.shim_kfd_keyframe.argtypes = [PU8, C.c_int, C.c_int, PI, PD, C.c_int, C.c_int, PU8, PU8, PF, PI, PF, PU64, PI]
    return lib


class Shape:
    def __init__(self, be, n, shim, pattern, voc):
        self.be, self.n, self.shim, self.pattern = be, n, shim, pattern
        base = gf.synth.klt_texture(ROWS, COLS, seed=0)
        self.images = np.ascontiguousarray(np.stack([np.roll(base, 3 * k, axis=1) for k in range(n)]))
        self.cams = np.ascontiguousarray(np.tile(np.array(CAMERA), (n, 1)))
        self.t = be.tracker(n, ROWS, COLS, 8)
        self.t.push_image(self.images)
        self.d = be.describer(n, ROWS, COLS, pattern, self.cams, ring_slots=1, keypoint_capacity=CAP)
        self.A, self.B = be.loop_database(voc, 64, 1 << 18), be.loop_database(voc, 64, 1 << 18)
        px = ROWS * COLS
        self.blur, self.plane = np.zeros(px, np.uint8), np.zeros(px, np.uint8)
        self.pts, self.ptsn, self.score, self.desc = np.zeros((CAP, 2), np.float32), np.zeros((CAP, 2), np.float32), np.zeros(CAP, np.int32), np.zeros((CAP, 4), np.uint64)
        self.first = [a.copy() for a in (self.pts, self.ptsn, self.desc)]
        self.cn, self.cn_all = np.zeros(4, np.int32), np.zeros((n, 4), np.int32)
        self.res = [np.zeros(1, np.int32) for _ in range(3)] + [np.zeros(16, np.int32), np.zeros(16)]
        self.times = dict(a=[], b=[])

    def step(self, record):
        lib, ctx, n = self.be.lib, self.be.ctx, self.n
        p = lambda a, ty: a.ctypes.data_as(ty)
        out = lambda: (p(self.res[0], PI), p(self.res[1], PI), p(self.res[2], PI), p(self.res[3], PI), p(self.res[4], PD))
        t0 = time.perf_counter()      # (a)
        n0 = 0
        for k in range(n):
            m = self.shim.shim_kfd_keyframe(p(self.images[k], PU8), ROWS, COLS, p(self.pattern, PI), p(self.cams[k], PD), 20, CAP, p(self.blur, PU8), p(self.plane, PU8),
                                            p(self.pts, PF), p(self.score, PI), p(self.ptsn, PF), p(self.desc, PU64), p(self.cn, PI))
            if k == 0:
                n0 = m
                for dst, src in zip(self.first, (self.pts, self.ptsn, self.desc)):
                    dst[:] = src
        rc = lib.gfbe_ldb_add_keyframe(ctx, self.A.h, n0, p(self.first[2], PU64), p(self.first[0], PF), p(self.first[1], PF), 1, *out())
        t1 = time.perf_counter()
        assert rc == 0, rc
        host = [r.copy() for r in self.res]
        t2 = time.perf_counter()      # (b)
        rc1 = lib.gfbe_kfd_capture(ctx, self.d.h, self.t.h, 0)
        rc2 = lib.gfbe_kfd_extract(ctx, self.d.h, 0, None, None, None, None, None, p(self.cn_all, PI))
        rc3 = lib.gfbe_kfd_add_keyframe(ctx, self.d.h, 0, self.B.h, 1, *out())
        t3 = time.perf_counter()
        assert (rc1, rc2, rc3) == (0, 0, 0), (rc1, rc2, rc3)
        assert self.cn_all[0, 2] == n0 and all(np.array_equal(x, y) for x, y in zip(host, self.res)), "the two paths disagree"
        if record:
            self.times["a"].append((t1 - t0) * 1e3)
            self.times["b"].append((t3 - t2) * 1e3)

    def close(self):
        for h in (self.d, self.A, self.B, self.t):
            h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="1,64,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfd_bench.txt"))
    a = ap.parse_args()
    be = gf.Backend(device=0)
    shim = host_shim()
    pat = json.load(open(os.path.join(ROOT, "tests", "golden", "brief_pattern.json")))
    pattern = np.ascontiguousarray(np.array([pat[k] for k in ("x1", "y1", "x2", "y2")], np.int32))
    voc = ldb_cases.trees()["k10L3"]
    shapes = tuple(int(s) for s in a.shapes.split(","))
    runs = {n: Shape(be, n, shim, pattern, voc) for n in shapes}
    for n in shapes:
        runs[n].step(False)
    for r in range(a.reps):
        for n in shapes:
            runs[n].step(True)
        print("repetition %d of %d" % (r + 1, a.reps), file=sys.stderr, flush=True)
    lines = ["the descriptors of a keyframe host to host, 640 x 480, about %d listed corners a camera, %d alternating repetitions after a warm-up (ms: median, max - min)"
             % (int(runs[shapes[0]].cn_all[0, 2]), a.reps),
             "%66s %8s %12s %10s %14s" % ("path", "cameras", "median ms", "spread ms", "ms per camera")]
    for n in shapes:
        for key, label in (("a", "(a) host K1 .. K5 on one thread + gfbe_ldb_add_keyframe (camera 0)"), ("b", "(b) capture + extract (NULL outputs) + gfbe_kfd_add_keyframe (camera 0)")):
            ts = runs[n].times[key]
            med = float(np.median(ts))
            lines.append("%66s %8d %12.3f %10.3f %14.4f" % (label, n, med, max(ts) - min(ts), med / n))
    lines.append("(a) has the images on the host already; (b) has them in the tracker. Both paths gave the same corner count, keyframe index, loop_index and results")
    lines.append("in every repetition. The host build of gfbe_kfd.h is g++ -O2 on one thread. First numbers, nothing is tuned to them.")
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
