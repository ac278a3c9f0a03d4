#!/usr/bin/env python3
"""Times a push of equalised images for 1, 64 and 1024 cameras of 752 x 480 (synth.klt_texture, rolled from camera to camera),
three ways in the same build and on the same tracker:

  (p) gfbe_klt_push_image alone: the frame loop without `equalize: 1` (this route does not touch the new code);
  (e) gfbe_eq_push_klt: upload, k_eq_lut and k_eq_apply on the raw images, the same pyramid build;
  (h) the route a caller had before gfbe_eq_*: E1 .. E6 by the host build of csrc/gfbe_eq.h on one thread (tests/eq_host_shim.cpp,
      g++ -O2), camera after camera, then gfbe_klt_push_image of the equalised images.

A push returns without waiting, so every figure is the call plus a gfbe_klt_download_level with NULL outputs, which only waits for the
stream: a host clock around work that ends in a device synchronise. After one warm-up of every route and shape, the routes and the
shapes run alternately `--reps` times; median and max - min of the repetitions. (e) and (h) must leave the same level-0 image of the
first and the last camera, or the tool fails. The calls are made on preallocated arrays through the C ABI. No time is asserted
anywhere. Writes profiles/eq_bench.txt.

    python tools/diag_eq_bench.py [--reps 9] [--out profiles/eq_bench.txt]
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

ROWS, COLS, TILES, CLIP = 480, 752, 8, 40.0
PU8 = C.POINTER(C.c_uint8)


def host_shim():
    out = os.path.join(ROOT, "tests", "_build", "eq_host_shim.so")
    src = os.path.join(ROOT, "tests", "eq_host_shim.cpp")
    hdrs = [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_eq.h", "gfbe_klt.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + hdrs):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([os.environ.get("CXX") or shutil.which("g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.shim_eq.argtypes = [PU8] + [C.c_int] * 4 + [C.c_double, PU8, PU8]
    return lib


class Shape:
    def __init__(self, be, n, shim):
        self.be, self.n, self.shim = be, n, shim
        base = gf.synth.klt_texture(ROWS, COLS, seed=0)
        self.images = np.ascontiguousarray(np.stack([np.roll(base, 3 * k, axis=1) for k in range(n)]))
        self.equalised = np.zeros_like(self.images)
        self.lut = np.zeros((TILES, TILES, 256), np.uint8)
        self.t = be.tracker(n, ROWS, COLS, 8)
        self.e = be.equalizer(n, ROWS, COLS, tiles_x=TILES, tiles_y=TILES, clip_limit=CLIP)
        self.times = dict(p=[], e=[], h=[])

    def _wait(self):
        lib, ctx = self.be.lib, self.be.ctx
        rc = lib.gfbe_klt_download_level(ctx, self.t.h, 1, 0, 0, None, None, None)      # (NULL outputs: the stream synchronise alone)
        assert rc == 0, rc

    def step(self, record):
        lib, ctx, n = self.be.lib, self.be.ctx, self.n
        p = lambda a: a.ctypes.data_as(PU8)
        t0 = time.perf_counter()      # (p)
        rc = lib.gfbe_klt_push_image(ctx, self.t.h, p(self.images))
        self._wait()
        t1 = time.perf_counter()
        assert rc == 0, rc
        t2 = time.perf_counter()      # (e)
        rc = lib.gfbe_eq_push_klt(ctx, self.e.h, self.t.h, p(self.images))
        self._wait()
        t3 = time.perf_counter()
        assert rc == 0, rc
        dev = [self.t.level(1, k, 0)["image"] for k in (0, n - 1)]
        t4 = time.perf_counter()      # (h)
        for k in range(n):
            self.shim.shim_eq(p(self.images[k]), ROWS, COLS, TILES, TILES, CLIP, p(self.lut), p(self.equalised[k]))
        rc = lib.gfbe_klt_push_image(ctx, self.t.h, p(self.equalised))
        self._wait()
        t5 = time.perf_counter()
        assert rc == 0, rc
        host = [self.t.level(1, k, 0)["image"] for k in (0, n - 1)]
        assert all(np.array_equal(a, b) for a, b in zip(dev, host)), "the two routes disagree"
        if record:
            for key, dt in (("p", t1 - t0), ("e", t3 - t2), ("h", t5 - t4)):
                self.times[key].append(dt * 1e3)

    def close(self):
        self.e.close()
        self.t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="1,64,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eq_bench.txt"))
    a = ap.parse_args()
    be = gf.Backend(device=0)
    shim = host_shim()
    shapes = tuple(int(s) for s in a.shapes.split(","))
    runs = {n: Shape(be, n, shim) for n in shapes}
    for n in shapes:
        runs[n].step(False)
    for r in range(a.reps):
        for n in shapes:
            runs[n].step(True)
        print("repetition %d of %d" % (r + 1, a.reps), file=sys.stderr, flush=True)
    labels = (("p", "(p) gfbe_klt_push_image + wait"), ("e", "(e) gfbe_eq_push_klt + wait"), ("h", "(h) host E1 .. E6 on one thread + gfbe_klt_push_image + wait"))
    lines = ["a push of %d x %d images, CLAHE %d x %d tiles, clip_limit %g, %d alternating repetitions after a warm-up (ms: median, max - min)" % (COLS, ROWS, TILES, TILES, CLIP, a.reps),
             "%62s %8s %12s %10s %14s %16s" % ("route", "cameras", "median ms", "spread ms", "ms per camera", "over (p), ms")]
    for n in shapes:
        base = float(np.median(runs[n].times["p"]))
        for key, label in labels:
            ts = runs[n].times[key]
            med = float(np.median(ts))
            lines.append("%62s %8d %12.3f %10.3f %14.4f %16s" % (label, n, med, max(ts) - min(ts), med / n, "" if key == "p" else "%.3f" % (med - base)))
    lines.append("(e) and (h) left the same level-0 image of the first and the last camera in every repetition. Every push copies the images into a pinned mirror")
    lines.append("before it returns; that copy is inside every figure. The host side of (h) is this project's restatement of CLAHE, the host build of gfbe_eq.h")
    lines.append("(g++ -O2) on one thread. It is not OpenCV, which is not part of the reference tree: cv::CLAHE is vectorised and threaded. First numbers, nothing is tuned to them.")
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
