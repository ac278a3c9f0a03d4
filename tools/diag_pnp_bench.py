#!/usr/bin/env python3
"""Times the loop verification host to host on preallocated arrays through the C ABI, in the same build:

  verify            gfbe_pnp_verify of B = 1 and 64 problems of 150 and 1 000 matches (planted poses, inlier share 0.6), against the host
                    build of csrc/gfbe_pnp.h on one thread (tests/pnp_host_shim.cpp, g++ -O2), which runs the same rules V1 .. V8 problem
                    after problem. The host column is this library's own arithmetic on a CPU; it is NOT cv::solvePnPRansac, which stops
                    early and uses another minimal solver, so it says nothing about OpenCV's time.
  find_connection   gfbe_pnp_find_connection_kfd (one wait) against gfbe_kfd_match + a host gather + gfbe_pnp_verify (two waits) on the
                    window descriptors a describer holds: a 240 x 320 keyframe matched against itself.

After one warm-up the paths and shapes run alternately `--reps` times; median and max - min of the repetitions. The two sides of a row
gave the same results in every repetition (asserted). No time is asserted anywhere. First numbers; nothing is tuned to them. Writes
profiles/pnp_bench.txt.

    python tools/diag_pnp_bench.py [--reps 9] [--out profiles/pnp_bench.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _gfbe_import import gf      # noqa: E402
import kfd_cases                 # noqa: E402
import ldb_cases                 # noqa: E402  (the synthetic vocabulary of the loop-database tests)
import pnp_cases                 # noqa: E402
import pnp_np                    # noqa: E402
import pnp_host                  # noqa: E402  (the build of the host shim)

PF, PI, PD, PU8, PU64 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
p = lambda a, ty: a.ctypes.data_as(ty)


class Verify:
    def __init__(self, be, shim, B, n):
        self.be, self.shim, self.B, self.n = be, shim, B, n
        self.o = pnp_np.options()
        problems = [pnp_cases.planted(1000 + 7 * b + n, int(0.6 * n), n - int(0.6 * n)) for b in range(B)]
        self.off, self.p3, self.pn, self.pc, self.tq = [np.ascontiguousarray(a) for a in pnp_cases.pack(problems)]
        self.v = be.loop_verifier(max_problems=B)
        mk = lambda: [np.zeros(B * n, np.uint8), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, 8)), np.zeros((B, 12)), np.zeros((B, 2), np.int32), np.zeros(B, np.int32)]
        self.dev, self.host = mk(), mk()
        self.times = dict(host=[], dev=[])

    @staticmethod
    def _outs(r):
        return [p(r[0], PU8), p(r[1], PI), p(r[2], PI), p(r[3], PD), p(r[4], PD), p(r[5], PI), p(r[6], PI)]

    def step(self, record):
        o = self.o
        ins = [p(self.off, PI), p(self.p3, PF), p(self.pn, PF), p(self.pc, PD), p(self.tq, PD)]
        t0 = time.perf_counter()
        self.shim.shim_pnp_verify(self.B, *ins, o["iterations"], o["refine_iterations"], o["min_loop_num"], o["seed"], o["reproj_threshold"], o["max_yaw_deg"], o["max_translation"],
                                  *self._outs(self.host), None, None, None, None)
        t1 = time.perf_counter()
        rc = self.be.lib.gfbe_pnp_verify(self.be.ctx, self.v.h, self.B, *ins, *self._outs(self.dev), None, None, None, None)
        t2 = time.perf_counter()
        assert rc == 0, rc
        for k, (a, b) in enumerate(zip(self.host, self.dev)):
            assert np.array_equal(a, b) if k != 3 else (np.array_equal(a[:, :7], b[:, :7]) and np.abs(a[:, 7] - b[:, 7]).max() <= pnp_cases.YAW_ATOL), "host and device disagree"
        assert int(self.dev[2].sum()) == self.B
        if record:
            self.times["host"].append((t1 - t0) * 1e3)
            self.times["dev"].append((t2 - t1) * 1e3)


class Connect:
    def __init__(self, be):
        rows, cols = 240, 320
        self.be = be
        img = kfd_cases.texture(rows, cols, 1)
        self.d = be.describer(1, rows, cols, kfd_cases.pattern(), [kfd_cases.CAMERAS["plain"]], window_capacity=2048)
        self.db = be.loop_database(ldb_cases.trees()["k10L3"], 4, 8192)
        self.d.push_image(0, img[None])
        lists = self.d.extract(0)[0]
        assert self.d.add_keyframe(0, self.db, False)["index"] == 0
        rng = np.random.default_rng(5)
        f = pnp_cases.frame(rng)
        self.W = W = len(lists["pts"])
        self.d.describe(0, [lists["pts"]])
        depth = rng.uniform(2.0, 8.0, W)
        Xc = np.concatenate([lists["pts_norm"].astype(np.float64) * depth[:, None], depth[:, None]], 1)
        self.p3 = np.ascontiguousarray((Xc @ f["R_wc"].T + f["t_wc"]).astype(np.float32))
        self.pc, self.tq = np.ascontiguousarray(f["pose_cur"]), np.ascontiguousarray(f["tic_qic"])
        self.v = be.loop_verifier(max_problems=1)
        mk = lambda: [np.zeros(1, np.int32), np.zeros(W, np.int32), np.zeros((W, 2), np.float32), np.zeros((W, 2), np.float32), np.zeros(W, np.uint8), np.zeros(1, np.int32),
                      np.zeros(1, np.int32), np.zeros(8), np.zeros(12), np.zeros(2, np.int32), np.zeros(1, np.int32)]
        self.one, self.two = mk(), mk()
        self.gather, self.off = np.zeros((W, 3), np.float32), np.zeros(2, np.int32)
        self.times = dict(one=[], two=[])

    def step(self, record):
        lib, ctx = self.be.lib, self.be.ctx
        a, b = self.one, self.two
        t0 = time.perf_counter()
        rc = lib.gfbe_pnp_find_connection_kfd(ctx, self.v.h, self.d.h, 0, self.db.h, 0, p(self.p3, PF), p(self.pc, PD), p(self.tq, PD), p(a[0], PI), p(a[1], PI), p(a[2], PF), p(a[3], PF),
                                              p(a[4], PU8), p(a[5], PI), p(a[6], PI), p(a[7], PD), p(a[8], PD), p(a[9], PI), p(a[10], PI))
        t1 = time.perf_counter()
        rc1 = lib.gfbe_kfd_match(ctx, self.d.h, 0, self.db.h, 0, None, None, None, p(b[0], PI), p(b[1], PI), p(b[2], PF), p(b[3], PF))
        nm = int(b[0][0])
        self.gather[:nm] = self.p3[b[1][:nm]]
        self.off[1] = nm
        rc2 = lib.gfbe_pnp_verify(ctx, self.v.h, 1, p(self.off, PI), p(self.gather, PF), p(b[3], PF), p(self.pc, PD), p(self.tq, PD), p(b[4], PU8), p(b[5], PI), p(b[6], PI), p(b[7], PD),
                                  p(b[8], PD), p(b[9], PI), p(b[10], PI), None, None, None, None)
        t2 = time.perf_counter()
        assert (rc, rc1, rc2) == (0, 0, 0), (rc, rc1, rc2)
        assert all(np.array_equal(x[:nm] if len(x) == self.W else x, y[:nm] if len(y) == self.W else y) for x, y in zip(a, b)) and a[6][0] == 1, "the two paths disagree"
        self.nm = nm
        if record:
            self.times["one"].append((t1 - t0) * 1e3)
            self.times["two"].append((t2 - t1) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_bench.txt"))
    a = ap.parse_args()
    be = gf.Backend(device=0)
    shim = pnp_host.load_shim()
    runs = [Verify(be, shim, B, n) for B in (1, 64) for n in (150, 1000)]
    con = Connect(be)
    for r in runs + [con]:
        r.step(False)
    for k in range(a.reps):
        for r in runs + [con]:
            r.step(True)
        print("repetition %d of %d" % (k + 1, a.reps), file=sys.stderr, flush=True)
    stat = lambda ts: (float(np.median(ts)), max(ts) - min(ts))
    lines = ["the loop verification host to host, 100 hypotheses and 5 refinement steps a problem, inlier share 0.6, %d alternating repetitions after a warm-up (ms: median, max - min)"
             % a.reps, "%58s %9s %8s %12s %10s %15s" % ("path", "problems", "matches", "median ms", "spread ms", "ms per problem")]
    for r in runs:
        for key, label in (("host", "host build of csrc/gfbe_pnp.h, one thread (not OpenCV)"), ("dev", "gfbe_pnp_verify")):
            med, spread = stat(r.times[key])
            lines.append("%58s %9d %8d %12.3f %10.3f %15.4f" % (label, r.B, r.n, med, spread, med / r.B))
    for key, label in (("two", "gfbe_kfd_match + host gather + gfbe_pnp_verify (two waits)"), ("one", "gfbe_pnp_find_connection_kfd (one wait)")):
        med, spread = stat(con.times[key])
        lines.append("%58s %9d %8d %12.3f %10.3f %15.4f" % (label, 1, con.nm, med, spread, med))
    lines.append("The host column is the same rules V1 .. V8 compiled with g++ -O2 on one thread, problem after problem: it scores all 100 hypotheses as the device does.")
    lines.append("It is not cv::solvePnPRansac. Both sides of a row gave the same results in every repetition. First numbers, nothing is tuned to them.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    be.close()


if __name__ == "__main__":
    main()
