#!/usr/bin/env python3
"""Times gfbe_lc4_solve and gfbe_lc4_solve_long host to host (numpy arrays in, numpy arrays out, one device wait inside) on
figure-of-eight graphs of n = 1000 and 5000 keyframes: gfbe_lc4_solve with 16 and 64 loop edges, gfbe_lc4_solve_long with 65, 128, 256
and 512 (the capacitance system blocked across workgroups). After a warm-up the twelve graphs are solved alternately `--reps` times
each, median and max - min of the repetitions. Beside the four short rows the time of the numpy model of the tests (tests/lc4_np.py,
FP64, band path, one core) on the same graph, once (beyond 64 loop edges the model takes minutes and is not run). That comparison says how far the test model is from the device, nothing more: the model is written
to follow the device phase by phase in numpy calls and Python loops, and says nothing about what Ceres with SPARSE_NORMAL_CHOLESKY
takes for the same graph — no such build exists here. No split by kernel: every kernel of a solve is enqueued blindly and the host
waits once, a device-clock split needs the profiler. Writes profiles/lc4_long_bench.txt (profiles/lc4_bench.txt is the record of the
four short rows before gfbe_lc4_solve_long existed).

    python tools/diag_lc4_bench.py [--reps 15] [--no-model] [--out profiles/lc4_long_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _gfbe_import import gf      # noqa: E402
import lc4_np as m      # noqa: E402

KEYS = ("t", "ypr", "sequence", "fixed", "loop_i", "loop_c", "loop_meas")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lc4_long_bench.txt"))
    a = ap.parse_args()
    be = gf.Backend(device=0)
    lg = gf.abi.LoopGraph(be.lib, "gfbe_", be.ctx)
    shapes = [(1000, 16), (1000, 64), (5000, 16), (5000, 64)] + [(n, L) for n in (1000, 5000) for L in (65, 128, 256, 512)]
    call = {s: (lg.solve if s[1] <= gf.abi.LC4_MAX_LOOPS else lg.solve_long) for s in shapes}
    graphs = {}
    for n, L in shapes:
        g = gf.synth.loop_graph(n=n, n_loop=L, seed=n + L, laps=4, yaw_bias=0.05, scale_err=0.02)
        graphs[(n, L)] = [g[k] for k in KEYS]
    times = {s: [] for s in shapes}
    outs = {}
    for s in shapes:      # warm-up: the scratch grows to the largest graph
        outs[s] = call[s](*graphs[s])
    for _ in range(a.reps):
        for s in shapes:
            t0 = time.perf_counter()
            call[s](*graphs[s])
            times[s].append((time.perf_counter() - t0) * 1e3)
    lines = ["gfbe_lc4_solve (up to 64 loops) / gfbe_lc4_solve_long, host to host, %d alternating repetitions after a warm-up (ms: median, max - min); 5 iterations enqueued" % a.reps,
             "%20s %6s %6s %12s %10s %6s %6s %14s" % ("call", "n", "loops", "median ms", "spread ms", "iters", "acc", "numpy model ms")]
    for s in shapes:
        sm = outs[s]["summary"]
        model = float("nan")
        if not a.no_model and s[1] <= gf.abi.LC4_MAX_LOOPS:
            t0 = time.perf_counter()
            m.solve(*graphs[s], dt=np.float64, path="band")
            model = (time.perf_counter() - t0) * 1e3
        lines.append("%20s %6d %6d %12.3f %10.3f %6d %6d %14.0f" % ("gfbe_lc4_solve" if s[1] <= gf.abi.LC4_MAX_LOOPS else "gfbe_lc4_solve_long", s[0], s[1], float(np.median(times[s])),
                                                                   max(times[s]) - min(times[s]), sm["iterations"], sm["num_successful"], model))
    lines.append("numpy model: tests/lc4_np.py in FP64 on one core, once per graph, including its kappa estimate; a test model in Python, not a baseline.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
