#!/usr/bin/env python3
"""Times gfbe_klt_push_image and gfbe_klt_track host to host for 1, 64 and 1024 cameras of 640 x 480 with 150 points each (numpy
arrays in, numpy arrays out). push_image returns without waiting, so its figure is the call plus the download of the smallest
level, which waits for the pyramid; track has its one wait inside. After a warm-up the shapes run alternately `--reps` times each;
median and max - min of the repetitions. Beside them the one-thread host build of the same header (tests/klt_host_shim.cpp, g++ -O2)
on one camera: pyramid and derivative of one image, and the tracking half on the same 150 points. That says nothing about OpenCV,
which is not part of the reference tree: OpenCV's tracker is vectorised and runs on several threads. No time is asserted anywhere. First
numbers; nothing is tuned to them. Writes profiles/klt_bench.txt.

    python tools/diag_klt_bench.py [--reps 15] [--out profiles/klt_bench.txt]
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

ROWS, COLS, NPTS, SHIFT = 480, 640, 150, (2.6, -1.3)
PF, PI, PU8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def host_shim():
    out = os.path.join(ROOT, "tests", "_build", "klt_host_shim.so")
    src = os.path.join(ROOT, "tests", "klt_host_shim.cpp")
    hdr = os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_klt.h")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, hdr)):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([os.environ.get("CXX") or shutil.which("g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.shim_klt_build.restype = C.c_void_p
    lib.shim_klt_build.argtypes = [PU8, C.c_int, C.c_int, C.c_int]
    lib.shim_klt_free.argtypes = [C.c_void_p]
    lib.shim_klt_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int, PF, PI, PI, C.c_int, PF, PI, C.POINTER(C.c_double), PF, PF, PI, PI, PI]
    return lib


def host_times(a, b, pts, reps=3):
    lib = host_shim()
    ids, cnt = np.arange(NPTS, dtype=np.int32), np.ones(NPTS, np.int32)
    iopt, dopt = np.array([3, 1, 1, 250, 10, 30], np.int32), np.array([0.5, 0.01, 1e-4])
    po, co, io, no, cn = np.zeros((NPTS, 2), np.float32), np.zeros((NPTS, 2), np.float32), np.zeros(NPTS, np.int32), np.zeros(NPTS, np.int32), np.zeros(4, np.int32)
    tb, tt, kept = [], [], 0
    for _ in range(reps):
        pa = lib.shim_klt_build(a.ctypes.data_as(PU8), COLS, ROWS, 3)
        t0 = time.perf_counter()
        pb = lib.shim_klt_build(b.ctypes.data_as(PU8), COLS, ROWS, 3)
        t1 = time.perf_counter()
        kept = lib.shim_klt_track(pa, pb, NPTS, pts.ctypes.data_as(PF), ids.ctypes.data_as(PI), cnt.ctypes.data_as(PI), 0, pts.ctypes.data_as(PF), iopt.ctypes.data_as(PI),
                                  dopt.ctypes.data_as(C.POINTER(C.c_double)), po.ctypes.data_as(PF), co.ctypes.data_as(PF), io.ctypes.data_as(PI), no.ctypes.data_as(PI),
                                  cn.ctypes.data_as(PI))
        t2 = time.perf_counter()
        lib.shim_klt_free(pa)
        lib.shim_klt_free(pb)
        tb.append((t1 - t0) * 1e3)
        tt.append((t2 - t1) * 1e3)
    return float(np.median(tb)), float(np.median(tt)), kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_bench.txt"))
    a = ap.parse_args()
    be = gf.Backend(device=0)
    base = [gf.synth.klt_image_pair(ROWS, COLS, seed, SHIFT) for seed in range(8)]      # (eight scenes, repeated over the cameras)
    pts = [gf.synth.klt_grid_points(ROWS, COLS, NPTS, seed=s, margin=30.0) for s in range(8)]
    shapes = (1, 64, 1024)
    runs = {}
    for n in shapes:
        A, B = np.stack([base[k % 8][0] for k in range(n)]), np.stack([base[k % 8][1] for k in range(n)])
        t = be.tracker(n, ROWS, COLS, NPTS)
        P = [pts[k % 8] for k in range(n)]
        ids, cnt = [np.arange(NPTS, dtype=np.int32)] * n, [np.ones(NPTS, np.int32)] * n
        top = t.opt.max_level
        runs[n] = dict(t=t, A=A, B=B, P=P, ids=ids, cnt=cnt, top=top, push=[], track=[], kept=0)

    def once(r, record):
        t = r["t"]
        t.push_image(r["A"])
        t.set_points(r["P"], r["ids"], r["cnt"])
        t0 = time.perf_counter()
        t.push_image(r["B"])
        t.level(1, 0, r["top"])
        t1 = time.perf_counter()
        out = t.track()
        t2 = time.perf_counter()
        r["kept"] = sum(len(o["ids"]) for o in out)
        if record:
            r["push"].append((t1 - t0) * 1e3)
            r["track"].append((t2 - t1) * 1e3)
    for n in shapes:
        once(runs[n], False)
    for _ in range(a.reps):
        for n in shapes:
            once(runs[n], True)
    hb, ht, hk = host_times(base[0][0], base[0][1], pts[0])
    lines = ["gfbe_klt_* host to host, 640 x 480, 150 points a camera, max_level 3, flow_back on, %d alternating repetitions after a warm-up (ms: median, max - min)" % a.reps,
             "%22s %8s %12s %10s %14s  %s" % ("call", "cameras", "median ms", "spread ms", "ms per camera", "note")]
    for n in shapes:
        r = runs[n]
        for key, label in (("push", "push_image + wait"), ("track", "track")):
            med = float(np.median(r[key]))
            lines.append("%22s %8d %12.3f %10.3f %14.4f  %s" % (label, n, med, max(r[key]) - min(r[key]), med / n, "kept %d of %d" % (r["kept"], n * NPTS) if key == "track" else ""))
    lines.append("one thread host, one camera: pyramid + derivative of one image %.3f ms, tracking half on 150 points %.3f ms (kept %d); the host build of" % (hb, ht, hk))
    lines.append("gfbe_klt.h (g++ -O2), median of 3. It is not OpenCV, which is not part of the reference tree: cv::calcOpticalFlowPyrLK is vectorised and threaded.")
    lines.append("push_image copies the images into a pinned mirror before it returns; that copy is inside its figure. First numbers, nothing is tuned to them.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    for r in runs.values():
        r["t"].close()


if __name__ == "__main__":
    main()
