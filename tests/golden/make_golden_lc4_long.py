#!/usr/bin/env python3
"""Records the reference of the 512-loop case of tests/lc4_long_cases.py: the model (tests/lc4_np.py, band path) solves the graph once in
longdouble and once in FP64 (two processes, minutes each on one core) and tests/golden/lc4_long_cap.npz receives what the tests compare
against: t / yaw / drift / cost history of the longdouble solve as float64 high / low pairs, the absolute sums behind them (A_cost, g_l1,
A_pose), the decisions of both precisions, the smallest decision margin in units of u A, r_cpu (FP64 against longdouble) and a SHA-256
of the input arrays, which tests/test_lc4_long_host.py holds against synth.loop_graph's arrays of the day.

    python tests/golden/make_golden_lc4_long.py
"""
import concurrent.futures
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def _solve(dtype):
    import lc4_long_cases as ll
    import lc4_np as m
    c = ll.cap_case()
    return m.solve(*c["args"], opt=c["opt"], dt=m.LD if dtype == "ld" else np.float64, path="band")


def main():
    import lc4_cases as lc
    import lc4_long_cases as ll
    with concurrent.futures.ProcessPoolExecutor(2) as ex:
        ld, f64 = ex.map(_solve, ("ld", "f64"))
    c = ll.cap_case()
    rr = lc.solve_ratios(f64, ld)
    margin = min(lc.margin_ratio(ld), lc.margin_ratio(f64))
    print("decisions", lc.decisions(ld), lc.decisions(f64), "margin %.3g" % margin, "r_cpu", rr)
    if lc.decisions(ld) != lc.decisions(f64) or margin < 1e3:
        sys.exit("the seed does not satisfy the rule of lc4_cases.py: replace it")
    out = {}
    for k, v in (("t", ld["t"]), ("yaw", ld["yaw"]), ("drift", ld["drift"]), ("cost", np.array(ld["cost_history"], ll.m.LD))):
        out[k + "_hi"], out[k + "_lo"] = ll.split(v)
    dec = lambda r: np.array([r["iterations"], r["termination"], r["status"], r["num_successful"]], np.int64)
    out.update(A_cost=np.array(ld["A_cost"], np.float64), g_l1=np.array(ld["g_l1"], np.float64), A_pose=np.float64(ld["A_pose"]),
               decisions_ld=dec(ld), decisions_f64=dec(f64), accepted_ld=np.array(ld["accepted"], np.int64), accepted_f64=np.array(f64["accepted"], np.int64),
               margin=np.float64(margin), r_cpu_pose=np.float64(rr["pose"]), r_cpu_cost=np.float64(rr["cost"]), digest=np.array(ll.input_digest(c)))
    np.savez_compressed(ll.GOLDEN, **out)
    print("wrote", ll.GOLDEN, os.path.getsize(ll.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
