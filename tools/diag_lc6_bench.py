#!/usr/bin/env python3
"""Times gfbe_lc6_solve host to host (numpy arrays in, numpy arrays out, one device wait inside) on figure-of-eight graphs of n = 1000
and 5000 keyframes with 16, 64 and 128 loop edges, and beside each the 4-DoF solve on the graph of the same size (gfbe_lc4_solve up to
64 loop edges, gfbe_lc4_solve_long at 128). After a warm-up the twelve calls run alternately `--reps` times each; median and max - min
of the repetitions. No split by kernel: every kernel of a solve is enqueued blindly and the host waits once, a device-clock split needs
the profiler. No time is asserted anywhere. Writes profiles/lc6_bench.txt.

    python tools/diag_lc6_bench.py [--reps 15] [--out profiles/lc6_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _gfbe_import import gf      # noqa: E402

KEYS4 = ("t", "ypr", "sequence", "fixed", "loop_i", "loop_c", "loop_meas")
KEYS6 = ("t", "q", "sequence", "fixed", "loop_i", "loop_c", "loop_meas")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lc6_bench.txt"))
    a = ap.parse_args()
    be = gf.Backend(device=0)
    lg4, lg6 = gf.abi.LoopGraph(be.lib, "gfbe_", be.ctx), be.loop_graph6()
    shapes = [(n, L) for n in (1000, 5000) for L in (16, 64, 128)]
    calls = {}
    for n, L in shapes:
        kw = dict(n=n, n_loop=L, seed=n + L, laps=4, yaw_bias=0.05, scale_err=0.02)
        g6, g4 = gf.synth.loop_graph6(**kw), gf.synth.loop_graph(**kw)
        calls[("gfbe_lc6_solve", n, L)] = (lg6.solve, [g6[k] for k in KEYS6])
        name4 = "gfbe_lc4_solve" if L <= gf.abi.LC4_MAX_LOOPS else "gfbe_lc4_solve_long"
        calls[(name4, n, L)] = (lg4.solve if L <= gf.abi.LC4_MAX_LOOPS else lg4.solve_long, [g4[k] for k in KEYS4])
    times = {k: [] for k in calls}
    outs = {}
    for k, (fn, args) in calls.items():      # warm-up: the scratch grows to the largest graph
        outs[k] = fn(*args)
    for _ in range(a.reps):
        for k, (fn, args) in calls.items():
            t0 = time.perf_counter()
            fn(*args)
            times[k].append((time.perf_counter() - t0) * 1e3)
    lines = ["gfbe_lc6_solve beside the 4-DoF solve of the same size, host to host, %d alternating repetitions after a warm-up (ms: median, max - min); 5 iterations enqueued" % a.reps,
             "%20s %6s %6s %12s %10s %6s %6s" % ("call", "n", "loops", "median ms", "spread ms", "iters", "acc")]
    for k in calls:
        sm = outs[k]["summary"]
        lines.append("%20s %6d %6d %12.3f %10.3f %6d %6d" % (k[0], k[1], k[2], float(np.median(times[k])), max(times[k]) - min(times[k]), sm["iterations"], sm["num_successful"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
