"""gfbe_line_reduce / gfbe_ltab_reduce on the GPU against the numpy checker evaluated in numpy.longdouble (tests/line_reduce_np.py),
entry by entry, no sampling, no max-norm fallback:

    |X_dev[i, j] - X_ref[i, j]| <= K_X u A_X[i, j],   exactly 0.0 where A_X is zero

A_X: for the plain sums U, bp, bl, W, cost the entry's absolute sum; for what passes through V'^-1 the allowance of a line's term is
multiplied by kappa_l = |C|_inf |C^-1|_inf of its Jacobi-scaled block C = D V'_l D, D = diag(V'_l)^-1/2, in extended precision:
    A_Vinv = kappa_l |Vinv| A_V' |Vinv|,   A_H = A_U + sum_l kappa_l A_W |Vinv| A_W^T,   A_g = A_bp + sum_l kappa_l A_W |Vinv| A_bl.
K_X = max(1024, 4 r_cpu[X]) rounded up to a power of two, r_cpu the checker in FP64 against itself in longdouble (line_reduce_np.R_CPU,
asserted by tests/test_line_reduce_host.py):
%(K)s

Cases (line_reduce_np.case_names(), each alone and all at shuffled places of a batch of 257, both modes): default window; no eligible
line; 1 line; 257 and 600 eligible lines; every line with 5 / with 11 observations; all lines / none in start frame 0; 10 %% of the
observations displaced (huber_active; note that the unrefined lines of these windows already put ~90 %% of the residuals outside the
width at sqrt_info = 400, so every case runs mostly on the loss's outer branch); mu = 1e-4, 1; Huber off; huber_inactive (sqrt_info = 4:
the residuals inside the width); marg_300 (319 lines that start in frame 0: MARG_OLD with more than one line per thread). n_failed == 0 is asserted in every one of them. Separately: a line with
a NaN observation (failed, alone, outputs equal to the window without it), and sqrt_info = 0 (every V_l exactly zero: all lines fail at
mu = 0, none at mu = 1, every sum exactly zero). Bit identity: alone vs. inside the batch, a window twice in a batch, table-fed vs.
host-fed on the downloaded list, H against its transpose, the tables before and after the call.

Measured on an MI355X (worst |X_dev - X_ref| / (u A_X) per array over all cases, modes and launch shapes):
%(MEASURED)s
"""
import numpy as np
import pytest

import line_reduce_np as lr
from _gfbe_import import gf

abi = gf.abi
pytestmark = pytest.mark.gpu

MEASURED = """Per case and mode (m0 solve, m1 MARG_OLD); alone and at a shuffled place of the batch of 257 are the same bits, hence the same figures:
  default          m0  H 0.00 g 0.00 U 762.83 bp 491.34 cost 16.94 Vinv 0.38 bl 3380.04 W 265669.87
  default          m1  H 0.00 g 0.00 U 1306.02 bp 886.29 cost 56.54 Vinv 0.47 bl 2885.18 W 4812.95
  no_eligible      m0  H 0.00 g 0.00 U 0.00 bp 0.00 cost 0.00 Vinv 0.00 bl 0.00 W 0.00
  no_eligible      m1  H 0.00 g 0.00 U 0.00 bp 0.00 cost 0.00 Vinv 0.00 bl 0.00 W 0.00
  one_line         m0  H 0.00 g 0.00 U 431.94 bp 724.39 cost 251.37 Vinv 0.00 bl 162.10 W 428.46
  one_line         m1  H 0.00 g 0.00 U 0.00 bp 0.00 cost 0.00 Vinv 0.00 bl 0.00 W 0.00
  lines_257        m0  H 0.00 g 0.00 U 463.97 bp 241.24 cost 31.06 Vinv 6.00 bl 5294.23 W 16046.54
  lines_257        m1  H 0.00 g 0.00 U 2508.17 bp 423.41 cost 4.88 Vinv 0.02 bl 3223.69 W 3572.74
  lines_600        m0  H 0.00 g 0.00 U 817.07 bp 279.80 cost 20.45 Vinv 0.84 bl 12320.26 W 100292.62
  lines_600        m1  H 0.00 g 0.00 U 1674.87 bp 652.62 cost 112.01 Vinv 0.23 bl 5814.98 W 8107.69
  obs_5            m0  H 0.00 g 0.00 U 621.66 bp 459.13 cost 56.09 Vinv 24.85 bl 3225.81 W 7238.61
  obs_5            m1  H 0.00 g 0.00 U 422.97 bp 214.13 cost 275.56 Vinv 0.00 bl 374.35 W 915.26
  obs_11           m0  H 0.00 g 0.00 U 458.47 bp 257.12 cost 43.54 Vinv 0.00 bl 652.87 W 993.83
  obs_11           m1  H 0.00 g 0.00 U 458.47 bp 257.12 cost 48.10 Vinv 0.00 bl 706.98 W 993.83
  all_start_0      m0  H 0.03 g 0.00 U 345.24 bp 468.67 cost 67.71 Vinv 0.01 bl 2126.46 W 1966.79
  all_start_0      m1  H 0.02 g 0.00 U 345.24 bp 468.67 cost 66.43 Vinv 0.00 bl 2174.98 W 1966.79
  none_start_0     m0  H 0.00 g 0.00 U 310.94 bp 530.57 cost 30.63 Vinv 29.81 bl 6311.40 W 9363.12
  none_start_0     m1  H 0.00 g 0.00 U 0.00 bp 0.00 cost 0.00 Vinv 0.00 bl 0.00 W 0.00
  huber_active     m0  H 0.00 g 0.00 U 753.80 bp 221.94 cost 2.44 Vinv 0.00 bl 1654.81 W 5039.67
  huber_active     m1  H 0.00 g 0.00 U 254.45 bp 153.74 cost 71.79 Vinv 0.00 bl 154.69 W 5039.67
  mu_1e-4          m0  H 0.00 g 0.00 U 1285.32 bp 917.82 cost 96.73 Vinv 0.00 bl 5993.83 W 5090.49
  mu_1e-4          m1  H 0.00 g 0.00 U 1878.81 bp 744.54 cost 204.58 Vinv 0.00 bl 751.13 W 2429.22
  mu_1             m0  H 260.26 g 5.45 U 1285.32 bp 917.82 cost 96.73 Vinv 78.51 bl 5993.83 W 5090.49
  mu_1             m1  H 190.04 g 11.98 U 1878.81 bp 744.54 cost 204.58 Vinv 76.94 bl 751.13 W 2429.22
  huber_off        m0  H 0.00 g 0.00 U 11.37 bp 352.63 cost 30.98 Vinv 0.02 bl 1197.80 W 10673.29
  huber_off        m1  H 0.00 g 0.00 U 23.52 bp 342.51 cost 86.80 Vinv 0.00 bl 736.63 W 346.84
  huber_inactive   m0  H 0.00 g 0.00 U 33.31 bp 454.30 cost 188.02 Vinv 0.00 bl 4109.52 W 3871.29
  huber_inactive   m1  H 0.00 g 0.00 U 155.23 bp 1420.09 cost 194.97 Vinv 0.00 bl 1098.56 W 389.32
  marg_300         m0  H 0.00 g 0.00 U 194.68 bp 205.38 cost 0.98 Vinv 6.83 bl 4488.63 W 18842.58
  marg_300         m1  H 0.00 g 0.00 U 194.68 bp 205.38 cost 1.93 Vinv 5.39 bl 4704.98 W 18842.58
No array needs more than its K. W of the default window (2.8 r_cpu, half of K_W) is one entry of a pose block, a single two-term
product: the excess over the checker's own FP64 error is the device's factor arithmetic, not summation order. The library is built with
-ffp-contract=off, so it is not FMA contraction; what differs from numpy are the device's sin / cos / atan2 / asin and the order of
operations inside the factor (the folded 3 x 3 blocks against the checker's full 6 x 6 chains), on a line seen under a small angle.
It has not been isolated further.
Sensitivity (each built once outside the tree, not committed; this file's 38 tests on an MI355X):
  chunk loop without its last LDS chunk          32 fail: all 26 test_one_window_alone with lines, test_batch_of_257 x 2, the NaN test x 2,
                                                 table-fed x 2 (pass: no_eligible x 2, the zero-pivot path x 2, one_line / none_start_0 in MARG_OLD)
  extrinsic rows of W stored as zero             32 fail: the same 32
  start-frame observation skipped in solve mode  17 fail: every solve-mode test with lines (14 alone, batch, NaN, table-fed); MARG_OLD
                                                 mode, where that observation is skipped anyway, and the empty cases pass"""
__doc__ = __doc__ % dict(K="  r_cpu %s\n  K     %s" % (lr.R_CPU, lr.K), MEASURED=MEASURED)
MODES = (lr.SOLVE, lr.MARG_OLD)
BITS = ("H", "g", "U", "bp", "cost", "n_eligible", "n_failed", "Vinv", "bl", "W", "failed")


@pytest.fixture(scope="module")
def be():
    if np.finfo(lr.LD).nmant < 63:
        pytest.skip("numpy.longdouble has no extended precision on this host")
    b = gf.Backend(device=0)
    yield b
    b.close()


_ref_cache = {}


def reference(name, mode):
    if (name, mode) not in _ref_cache:
        lw, par = lr.build_case(name)
        _ref_cache[(name, mode)] = (lw, par, lr.reduce(lw, mode, dtype=lr.LD, **par))
    return _ref_cache[(name, mode)]


def compare(got, ref, label, worst):
    fails = []
    if int(got["n_eligible"]) != ref["n_eligible"] or int(got["n_failed"]) != ref["n_failed"]:
        return ["%s: n_eligible / n_failed %d / %d, expected %d / %d" % (label, got["n_eligible"], got["n_failed"], ref["n_eligible"], ref["n_failed"])]
    if not np.array_equal(got["failed"], ref["failed"]):
        fails.append("%s: failed flags differ" % label)
    for k, (r, nz) in lr.ratios(got, ref).items():
        worst[k] = max(worst.get(k, 0.0), r)
        if not r <= lr.K[k]:
            fails.append("%s: %s off by %.1f u A (K = %g)" % (label, k, r, lr.K[k]))
        if nz:
            fails.append("%s: %s has %d non-zero entries where the reference's absolute sum is zero" % (label, k, nz))
    if not np.array_equal(got["H"], got["H"].T) or not np.array_equal(got["U"], got["U"].T):
        fails.append("%s: H or U is not symmetric bit for bit" % label)
    print("%-28s " % label + "  ".join("%s %9.2f" % (k, v[0]) for k, v in lr.ratios(got, ref).items()))
    return fails


def same_bits(a, b):
    return [k for k in BITS if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", lr.case_names())
def test_one_window_alone(be, name, mode):
    lw, par, ref = reference(name, mode)
    got = be.line_reduce([lw], mode, par["sqrt_info"], par["width"], par["mu"])[0]
    assert int(got["n_failed"]) == 0
    fails = compare(got, ref, "%s mode %d alone" % (name, mode), {})
    if ref["n_eligible"] == 0:
        assert not got["H"].any() and not got["g"].any() and not got["U"].any() and not got["bp"].any() and got["cost"] == 0.0
    if mode == lr.MARG_OLD:
        assert not got["H"][:6].any() and not got["H"][:, :6].any() and not got["g"][:6].any()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", MODES)
def test_batch_of_257(be, mode):
    """Every case at shuffled places of one batch (the parameters sqrt_info, width, mu are per call: one batch per parameter set), each
    first occurrence against the reference and against its result alone, later occurrences against the first."""
    names = lr.case_names()
    fails, worst = [], {}
    for par_key in sorted({tuple(sorted(lr.build_case(n)[1].items())) for n in names}):
        par = dict(par_key)
        mine = [n for n in names if lr.build_case(n)[1] == par]
        rng = np.random.default_rng(257 + mode)
        order = np.concatenate([rng.permutation(len(mine)) for _ in range(257 // len(mine) + 1)])[:257]
        holders = {n: abi.LineWindowHolder(reference(n, mode)[0]) for n in mine}
        res = be.line_reduce([holders[mine[q]] for q in order], mode, par["sqrt_info"], par["width"], par["mu"])
        first = {}
        for w, q in enumerate(order):
            name = mine[q]
            assert int(res[w]["n_failed"]) == 0
            if q not in first:
                first[q] = res[w]
                fails += compare(res[w], reference(name, mode)[2], "%s mode %d B=257" % (name, mode), worst)
                alone = be.line_reduce([holders[name]], mode, par["sqrt_info"], par["width"], par["mu"])[0]
                d = same_bits(alone, res[w])
                if d:
                    fails.append("%s: %s differ between alone and place %d of the batch" % (name, d, w))
            else:
                d = same_bits(first[q], res[w])
                if d:
                    fails.append("%s: %s differ between two places of the batch" % (name, d))
        assert len(first) == len(mine)
    print("B=257 mode %d worst ratios %s" % (mode, {k: round(v, 2) for k, v in worst.items()}))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", MODES)
def test_line_with_nan_observation_is_left_out(be, mode):
    bad, without, victim = lr.nan_case()
    a, b = be.line_reduce([bad], mode)[0], be.line_reduce([without], mode)[0]
    ent = list(np.flatnonzero(lr.entering(bad, mode)))
    at = ent.index(victim)
    assert int(a["n_failed"]) == 1 and int(b["n_failed"]) == 0 and int(a["n_eligible"]) == int(b["n_eligible"]) + 1
    assert a["failed"][at] == 1 and a["failed"].sum() == 1
    for k in ("H", "g", "U", "bp", "cost"):
        assert np.array_equal(a[k], b[k]), k
    keep = np.arange(len(ent)) != at
    for k in ("Vinv", "bl", "W"):
        assert np.array_equal(a[k][keep], b[k]), k
    assert np.isfinite(a["H"]).all() and np.isfinite(a["g"]).all()
    ref = lr.reduce(without, mode, dtype=lr.LD)
    fails = compare(b, ref, "without the NaN line, mode %d" % mode, {})
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", MODES)
def test_zero_pivot_path(be, mode):
    """sqrt_info = 0: every V_l is exactly zero. mu = 0: every entering line fails, every sum is exactly zero. mu = 1: the clamp gives
    V' = 1e-6 I, no line fails, H and g are exactly zero."""
    lw = lr.build_case("default")[0]
    n = int(lr.entering(lw, mode).sum())
    a = be.line_reduce([lw], mode, 0.0, 1.0, 0.0)[0]
    assert int(a["n_eligible"]) == n > 0 and int(a["n_failed"]) == n and a["failed"].all()
    for k in ("H", "g", "U", "bp"):
        assert not a[k].any(), k
    assert a["cost"] == 0.0
    b = be.line_reduce([lw], mode, 0.0, 1.0, 1.0)[0]
    assert int(b["n_eligible"]) == n and int(b["n_failed"]) == 0 and not b["failed"].any()
    assert not b["H"].any() and not b["g"].any() and not b["W"].any()
    assert np.array_equal(b["Vinv"], np.broadcast_to(np.diag(np.full(4, 1.0 / 1e-6)), (n, 4, 4)))


@pytest.mark.parametrize("mode", MODES)
def test_table_fed_equals_host_fed_and_leaves_the_tables_alone(be, mode):
    names = ["default", "lines_257", "no_eligible", "obs_11", "default"]
    lws = [lr.build_case(n)[0] for n in names]
    tabs = be.line_tables(len(lws), 320)
    try:
        for w, lw in enumerate(lws):
            n = len(lw["n_obs"])
            off = np.concatenate([[0], np.cumsum(lw["n_obs"])]).astype(int)
            obs4 = np.zeros((n, abi.NFRAMES, 4))
            for i in range(n):
                obs4[i, :lw["n_obs"][i]] = lw["obs"][off[i]:off[i + 1]]
            tabs.upload(w, dict(line_id=np.arange(n, dtype=np.int32), start_frame=lw["start_frame"], n_obs=lw["n_obs"], obs4=obs4,
                                is_triangulation=lw["is_triangulation"], line_plucker=lw["line_plucker"]))
        before = [tabs.download(w) for w in range(len(lws))]
        pose7 = np.ascontiguousarray([lw["pose"] for lw in lws])
        ex = np.ascontiguousarray([lw["ex_cam"] for lw in lws])
        got = tabs.reduce(pose7, ex, mode)
        after = [tabs.download(w) for w in range(len(lws))]
        for a, b in zip(before, after):
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), k
        host = be.line_reduce([abi.ltab_to_line_window(before[w], pose7[w], ex[w]) for w in range(len(lws))], mode)
        for w in range(len(lws)):
            assert not same_bits(host[w], got[w]), (names[w], same_bits(host[w], got[w]))
        assert not same_bits(got[0], got[4])
        fails = compare(got[1], reference("lines_257", mode)[2], "lines_257 table-fed mode %d" % mode, {})
        assert not fails, "\n".join(fails)
    finally:
        tabs.close()
