#!/usr/bin/env python3
"""Times gfbe_det_detect host to host for 1, 64 and 1024 cameras of 640 x 480 with max_cnt 150, min_dist 30 and 100 held points a
camera (numpy arrays in, numpy arrays out), and beside it gfbe_klt_set_points with the lists detect returned: the upload a frame
needed while the caller ran setMask / goodFeaturesToTrack / addPoints itself, which detect replaces. Every repetition first restores
the held points, so each detect does the same work. After a warm-up the shapes run alternately `--reps` times each; median and
max - min of the repetitions. Beside them the one-thread host build of the same header (tests/det_host_shim.cpp, g++ -O2) on one
camera with the same inputs. That says nothing about OpenCV, which is not part of the reference tree: cv::goodFeaturesToTrack is
vectorised and threaded. No time is asserted anywhere. First numbers; nothing is tuned to them. Writes profiles/det_bench.txt.

    python tools/diag_det_bench.py [--reps 15] [--out profiles/det_bench.txt]
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

ROWS, COLS, MAX_CNT, MIN_DIST, HELD, QUALITY, CAND = 480, 640, 150, 30, 100, 0.01, 1 << 15
PF, PI, PU8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def host_time(im, pts, ids, cnt, reps=3):
    out = os.path.join(ROOT, "tests", "_build", "det_host_shim.so")
    src = os.path.join(ROOT, "tests", "det_host_shim.cpp")
    hdrs = [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_det.h", "gfbe_klt.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + hdrs):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([os.environ.get("CXX") or shutil.which("g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.shim_det_detect.argtypes = [PU8, C.c_int, C.c_int, C.c_int, PF, PI, PI, C.c_int, C.c_int, C.c_double, C.c_int, PI, PF, PI, PI, PI]
    po, io, no, cn = np.zeros((MAX_CNT, 2), np.float32), np.zeros(MAX_CNT, np.int32), np.zeros(MAX_CNT, np.int32), np.zeros(6, np.int32)
    ts = []
    for _ in range(reps):
        nid = np.zeros(1, np.int32)
        t0 = time.perf_counter()
        lib.shim_det_detect(im.ctypes.data_as(PU8), COLS, ROWS, len(pts), pts.ctypes.data_as(PF), ids.ctypes.data_as(PI), cnt.ctypes.data_as(PI), MAX_CNT, MIN_DIST, QUALITY, 0,
                            nid.ctypes.data_as(PI), po.ctypes.data_as(PF), io.ctypes.data_as(PI), no.ctypes.data_as(PI), cn.ctypes.data_as(PI))
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), cn.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_bench.txt"))
    a = ap.parse_args()
    be = gf.Backend(device=0)
    base = [gf.synth.klt_texture(ROWS, COLS, seed) for seed in range(8)]      # (eight scenes, repeated over the cameras)
    rng = np.random.default_rng(0)
    pts = [np.stack([rng.uniform(1, COLS - 2, HELD), rng.uniform(1, ROWS - 2, HELD)], 1).astype(np.float32) for _ in range(8)]
    ids, cnt = np.arange(HELD, dtype=np.int32), (np.arange(HELD, dtype=np.int32) % 7 + 1).astype(np.int32)
    shapes = (1, 64, 1024)
    runs = {}
    for n in shapes:
        t = be.tracker(n, ROWS, COLS, MAX_CNT)
        t.push_image(np.stack([base[k % 8] for k in range(n)]))
        d = be.detector(t, max_cnt=MAX_CNT, min_dist=MIN_DIST, quality=QUALITY, candidate_capacity=CAND)
        runs[n] = dict(t=t, d=d, P=[pts[k % 8] for k in range(n)], ids=[ids] * n, cnt=[cnt] * n, detect=[], set_points=[], out=None)

    def once(r, record):
        r["t"].set_points(r["P"], r["ids"], r["cnt"])
        t0 = time.perf_counter()
        out = r["d"].detect()
        t1 = time.perf_counter()
        r["t"].set_points([o["pts"] for o in out], [o["ids"] for o in out], [o["track_cnt"] for o in out])
        t2 = time.perf_counter()
        r["out"] = out
        if record:
            r["detect"].append((t1 - t0) * 1e3)
            r["set_points"].append((t2 - t1) * 1e3)
    for n in shapes:
        once(runs[n], False)
    for _ in range(a.reps):
        for n in shapes:
            once(runs[n], True)
    hm, hc = host_time(base[0], pts[0], ids, cnt)
    lines = ["gfbe_det_detect host to host, 640 x 480, max_cnt %d, min_dist %d, quality %g, %d held points a camera, %d alternating repetitions after a warm-up (ms: median, max - min)"
             % (MAX_CNT, MIN_DIST, QUALITY, HELD, a.reps),
             "%34s %8s %12s %10s %14s  %s" % ("call", "cameras", "median ms", "spread ms", "ms per camera", "note")]
    for n in shapes:
        r = runs[n]
        c = np.array([list(o["counters"].values()) for o in r["out"]])
        note = "kept %d, candidates %d (most of a camera %d), added %d, overflow %d" % (c[:, 1].sum(), c[:, 2].sum(), c[:, 2].max(), c[:, 3].sum(), c[:, 5].sum())
        for key, label in (("detect", "detect"), ("set_points", "set_points of detect's lists")):
            med = float(np.median(r[key]))
            lines.append("%34s %8d %12.3f %10.3f %14.4f  %s" % (label, n, med, max(r[key]) - min(r[key]), med / n, note if key == "detect" else "the upload detect replaces"))
    lines.append("one thread host, one camera: G1 .. G5 on the same inputs %.3f ms (kept %d, candidates %d, added %d); the host build of gfbe_det.h (g++ -O2), median" % (hm, hc[1], hc[2], hc[3]))
    lines.append("of 3. It is not OpenCV, which is not part of the reference tree: cv::goodFeaturesToTrack is vectorised and threaded. The figures include the")
    lines.append("binding's numpy work on both sides of a call. First numbers, nothing is tuned to them.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    for r in runs.values():
        r["d"].close()
        r["t"].close()


if __name__ == "__main__":
    main()
