import os as _os, sys as _sys
_r = _os.path.dirname(_os.path.abspath(__file__))
while not _os.path.exists(_os.path.join(_r, "_gfbe_import.py")):
    _r = _os.path.dirname(_r)
_sys.path[:0] = [_r, _os.path.join(_r, "tests")]   # (measurement scripts: the package root and the test helpers they share)
"""Timing of the line-only refinement (onlyLineOpt + removeLineOutlier on the device), host-fed against table-fed, on the same seeded
windows: 150 eligible lines with 5-11 observations each (NUM_ITERATIONS = 8), for 1 / 256 / 1024 / 4096 windows.
  host-fed   gfbe_line_refine: the whole list packed on the host and copied up on every call, lines and keep flags copied back
  table-fed  gfbe_ltab_refine on device-resident line tables that already hold the same lines (re-seeded by upload outside the timed
             region, since the refine edits the tables): only the poses go up and the summaries come down
Both legs: the host's clock around the call, which ends synchronised; the legs alternate, REPS repetitions each after one warm-up of
each; median and spread (max - min). kernel: the longest time one window spent in the kernel (gfbe_summary.ms_solve, device clock).
The two legs' results are compared bit for bit once per size. Output: stdout, and the same lines into the file given with --out.

--reduce: the same measurement for the reduced normal equations of the line factors (gfbe_line_reduce host-fed against gfbe_ltab_reduce
table-fed, solve mode, HuberLoss(1.0), mu = 0; outputs asked for: H, g, cost, the counts and ms_kernel — what the join into the window
solve takes; the per-line records stay on the device side of this measurement). The tables are not edited by the call, so they are
seeded once. kernel / mfma: the longest time one window spent in the kernel and in its matrix-core contraction loop (ms_kernel, device
clock); the sum over the windows divided by the 256 workgroups in flight estimates the kernel's own duration for the large batches.

--step: the same measurement for the step half of a joint iteration (gfbe_line_step host-fed against gfbe_ltab_step table-fed on the
records a solve-mode gfbe_ltab_reduce kept on the handle; outputs asked for: total, coef, invalid, cost_cand, ms_kernel - what the
caller's accept test takes; the candidates stay on the device). y_p, v_p, rest: seeded, the radius large (the Gauss-Newton branch).
gfbe_ltab_reduce on the same tables is timed in the same repetitions, for scale. kernel: the sum of the windows' times in k_line_step
divided by the workgroups in flight (device clock), and the bytes of the records it streams (2544 per entering line: W, Vinv, bl, V)
over that time as a fraction of the 8 TB/s HBM peak."""
import argparse
import time

import numpy as np
import torch  # noqa: F401  (one ROCm runtime per process: torch's goes first)

from _gfbe_import import gf
import line_np as ln

abi, synth_line = gf.abi, gf.synth_line
REPS = 7


def _table_of(lw, base_id=0):
    n = len(lw["start_frame"])
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])]).astype(int)
    obs4 = np.zeros((n, abi.NFRAMES, 4))
    for i in range(n):
        obs4[i, :lw["n_obs"][i]] = lw["obs"][off[i]:off[i + 1]]
    return dict(line_id=np.arange(n, dtype=np.int32) + base_id, start_frame=lw["start_frame"], n_obs=lw["n_obs"], obs4=obs4,
                is_triangulation=lw["is_triangulation"], line_plucker=lw["line_plucker"])


def reduce_leg(be, base, holders, seeds, sizes, say):
    import line_reduce_np as lrn
    want = ("H", "g", "cost", "n_eligible", "n_failed", "ms_kernel")
    for nw in sizes:
        hs = [holders[k % len(holders)] for k in range(nw)]
        tabs = be.line_tables(nw, 160)
        for w in range(nw):
            tabs.upload(w, seeds[w % len(seeds)])
        pose7 = np.ascontiguousarray([base[k % len(base)]["pose"] for k in range(nw)])
        ex = np.ascontiguousarray([base[k % len(base)]["ex_cam"] for k in range(nw)])
        bh, bt = abi.line_reduced_buffers(nw, 1, want), abi.line_reduced_buffers(nw, 1, want)
        rh, rt = abi.line_reduced_struct(bh), abi.line_reduced_struct(bt)
        t_host, t_tab = [], []
        for rep in range(REPS + 1):          # (rep 0: warm-up of both legs)
            t0 = time.perf_counter()
            rc = abi.line_reduce_raw(be.lib, "gfbe_", be.ctx, hs, 0, 400.0, 1.0, 0.0, rh)
            t1 = time.perf_counter()
            rc_t = tabs.reduce_raw(pose7, ex, 0, 400.0, 1.0, 0.0, rt)
            t2 = time.perf_counter()
            assert rc == abi.OK and rc_t == abi.OK, (rc, rc_t)
            if rep:
                t_host.append((t1 - t0) * 1e3)
                t_tab.append((t2 - t1) * 1e3)
        for k in ("H", "g", "cost", "n_eligible", "n_failed"):
            assert bh[k].tobytes() == bt[k].tobytes(), "table-fed != host-fed: " + k
        assert not bt["n_failed"].any()
        tabs.close()

        def stat(t):
            return float(np.median(t)), float(max(t) - min(t))
        (mh, sh), (mt, st) = stat(t_host), stat(t_tab)
        ms = bt["ms_kernel"]
        say("%5d windows: host-fed %8.3f ms (spread %6.3f) | table-fed %8.3f ms (spread %6.3f) | table-fed / host-fed %.3f, "
            "%7.2f -> %7.2f us / window | in the kernel per window: max %.3f ms, mean %.3f ms, matrix-core loop %.1f %% of it; "
            "sum / 256 workgroups %.3f ms | eligible lines %d" %
            (nw, mh, sh, mt, st, mt / mh, 1e3 * mh / nw, 1e3 * mt / nw, ms[:, 0].max(), ms[:, 0].mean(),
             100.0 * ms[:, 1].sum() / ms[:, 0].sum(), ms[:, 0].sum() / min(nw, 256), int(bt["n_eligible"][0])))
        say("              host-fed  [%s]" % " ".join("%.3f" % t for t in t_host))
        say("              table-fed [%s]" % " ".join("%.3f" % t for t in t_tab))
    t0 = time.perf_counter()
    for w in base[:2]:
        lrn.reduce(w)
    say("numpy checker (FP64): %.1f ms / window" % ((time.perf_counter() - t0) / 2 * 1e3))


def step_leg(be, base, holders, seeds, sizes, say):
    want_r = ("H", "g", "cost", "n_eligible", "n_failed", "ms_kernel")
    want_s = ("total", "coef", "invalid", "cost_cand", "ms_kernel")
    rng = np.random.default_rng(5)
    for nw in sizes:
        hs = [holders[k % len(holders)] for k in range(nw)]
        tabs = be.line_tables(nw, 160)
        for w in range(nw):
            tabs.upload(w, seeds[w % len(seeds)])
        tabs.keep_records(True)
        pose7 = np.ascontiguousarray([base[k % len(base)]["pose"] for k in range(nw)])
        ex = np.ascontiguousarray([base[k % len(base)]["ex_cam"] for k in range(nw)])
        # the records for the host-fed leg, once (not timed)
        recs = be.line_reduce_v(hs, 0, 400.0, 1.0, 0.0, ("n_eligible",) + abi.LINE_RECORD_KEYS)
        rb, ne = abi.line_records_pack(recs)
        red_h = abi.line_reduced_struct_v(rb)
        y, v = rng.normal(0, 1e-3, (nw, 72)), rng.normal(0, 1e-3, (nw, 72))
        rest = np.abs(rng.normal(1, 0.1, (nw, 8))) * np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
        radius = np.full(nw, 1e4)
        br = abi.line_reduced_buffers(nw, 1, want_r)
        rr = abi.line_reduced_struct(br)
        bh, bt = abi.line_stepped_buffers(nw, 1, want_s), abi.line_stepped_buffers(nw, 1, want_s)
        sh_, st_ = abi.line_stepped_struct(bh), abi.line_stepped_struct(bt)
        t_host, t_tab, t_red = [], [], []
        for rep in range(REPS + 1):          # (rep 0: warm-up of every leg)
            t0 = time.perf_counter()
            rc_r = tabs.reduce_raw(pose7, ex, 0, 400.0, 1.0, 0.0, rr)
            t1 = time.perf_counter()
            rc_t = tabs.step_raw(pose7, ex, 400.0, 1.0, y, v, rest, radius, st_)
            t2 = time.perf_counter()
            rc_h = abi.line_step_raw(be.lib, "gfbe_", be.ctx, hs, red_h, 400.0, 1.0, 0.0, y, v, rest, radius, sh_)
            t3 = time.perf_counter()
            assert rc_r == abi.OK and rc_t == abi.OK and rc_h == abi.OK, (rc_r, rc_t, rc_h)
            if rep:
                t_red.append((t1 - t0) * 1e3)
                t_tab.append((t2 - t1) * 1e3)
                t_host.append((t3 - t2) * 1e3)
        for k in ("total", "coef", "invalid", "cost_cand"):
            assert bh[k].tobytes() == bt[k].tobytes(), "table-fed != host-fed: " + k
        tabs.close()

        def stat(t):
            return float(np.median(t)), float(max(t) - min(t))
        (mh, sh), (mt, st), (mr, sr) = stat(t_host), stat(t_tab), stat(t_red)
        ms = bt["ms_kernel"]
        kern = ms.sum() / min(nw, 256)
        nbytes = 2544.0 * float(ne.sum())
        say("%5d windows: step host-fed %8.3f ms (spread %6.3f) | step table-fed %8.3f ms (spread %6.3f), %7.2f us / window | "
            "gfbe_ltab_reduce, records kept %8.3f ms (spread %6.3f) | k_line_step per window: max %.4f ms, mean %.4f ms; sum / %d workgroups "
            "%.4f ms = %.1f GB/s over the records' %.1f MB, %.2f %% of 8 TB/s | entering lines %d, invalid %d" %
            (nw, mh, sh, mt, st, 1e3 * mt / nw, mr, sr, ms.max(), ms.mean(), min(nw, 256), kern, nbytes / kern * 1e-6, nbytes * 1e-6,
             100.0 * nbytes / kern * 1e-6 / 8000.0, int(ne[0]), int(bt["invalid"].sum())))
        say("              step host-fed  [%s]" % " ".join("%.3f" % t for t in t_host))
        say("              step table-fed [%s]" % " ".join("%.3f" % t for t in t_tab))
        say("              ltab_reduce    [%s]" % " ".join("%.3f" % t for t in t_red))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1,256,1024,4096")
    ap.add_argument("--reduce", action="store_true", help="time gfbe_line_reduce / gfbe_ltab_reduce instead of the refinement")
    ap.add_argument("--step", action="store_true", help="time gfbe_line_step / gfbe_ltab_step (and gfbe_ltab_reduce on the same tables)")
    args = ap.parse_args()
    lines = []

    def say(msg):
        print(msg, flush=True)
        lines.append(msg)
    be = gf.Backend(0)
    base = [synth_line.line_window(seed=900 + k, n_ok=150, n_short=0, n_late=0, n_untri=0, n_behind=0, n_long=0, n_outlier=0)
            for k in range(32)]
    holders = [abi.LineWindowHolder(w) for w in base]
    seeds = [_table_of(w) for w in base]
    say("lines per window %d, observations per window %.0f (mean); %d repetitions per leg, alternating" %
        (holders[0].n, np.mean([len(h.obs) for h in holders]), REPS))
    if args.reduce or args.step:
        (step_leg if args.step else reduce_leg)(be, base, holders, seeds, [int(x) for x in args.sizes.split(",")], say)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    for nw in [int(x) for x in args.sizes.split(",")]:
        hs = [holders[k % len(holders)] for k in range(nw)]
        n_lines = sum(h.n for h in hs)
        plk, keep, sums_h = np.zeros((n_lines, 6)), np.zeros(n_lines, np.uint8), (abi.Summary * nw)()
        tabs = be.line_tables(nw, 160)
        pose7 = np.ascontiguousarray([base[k % len(base)]["pose"] for k in range(nw)])
        ex = np.ascontiguousarray([base[k % len(base)]["ex_cam"] for k in range(nw)])
        sums_t = (abi.Summary * nw)()

        def reseed():
            for w in range(nw):
                tabs.upload(w, seeds[w % len(seeds)])
        t_host, t_tab, k_host, k_tab = [], [], 0.0, 0.0
        for rep in range(REPS + 1):          # (rep 0: warm-up of both legs — module load, first allocations, staging growth)
            reseed()
            t0 = time.perf_counter()
            rc = abi.line_refine_raw(be.lib, "gfbe_", be.ctx, hs, plucker_out=plk, keep_out=keep, summary=sums_h)[0]
            t1 = time.perf_counter()
            rc_t = tabs.refine_raw(pose7, ex, sums=sums_t)[0]
            t2 = time.perf_counter()
            assert rc == rc_t and rc in (abi.OK, abi.NO_CONVERGENCE), (rc, rc_t)
            if rep:
                t_host.append((t1 - t0) * 1e3)
                t_tab.append((t2 - t1) * 1e3)
                k_host = max(k_host, max(sums_h[w].ms_solve for w in range(nw)))
                k_tab = max(k_tab, max(sums_t[w].ms_solve for w in range(nw)))
        # the two legs computed the same thing (a few tables; tests/test_gpu_ltab.py compares all of them)
        o = 0
        for w in range(min(nw, 3)):
            got = tabs.download(w)
            k = keep[o:o + hs[w].n] != 0
            assert got["line_plucker"].tobytes() == np.ascontiguousarray(plk[o:o + hs[w].n][k]).tobytes(), "table-fed != host-fed"
            o += hs[w].n
        tabs.close()

        def stat(t):
            return float(np.median(t)), float(max(t) - min(t))
        (mh, sh), (mt, st) = stat(t_host), stat(t_tab)
        say("%5d windows: host-fed %8.3f ms (spread %6.3f, kernel %6.3f) | table-fed %8.3f ms (spread %6.3f, kernel %6.3f) | "
            "table-fed / host-fed %.3f, %7.2f -> %7.2f us / window, iterations %d" %
            (nw, mh, sh, k_host, mt, st, k_tab, mt / mh, 1e3 * mh / nw, 1e3 * mt / nw, sums_t[0].iterations))
        say("              host-fed  [%s]" % " ".join("%.3f" % t for t in t_host))
        say("              table-fed [%s]" % " ".join("%.3f" % t for t in t_tab))
    t0 = time.perf_counter()
    for w in base[:4]:
        ln.refine(w)
    say("numpy checker: %.1f ms / window" % ((time.perf_counter() - t0) / 4 * 1e3))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
