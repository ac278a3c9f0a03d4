"""The linear solve of one iteration (csrc/gfbe_solve.hip) pinned by its BACKWARD error, on every kernel and launch shape: the step y,
the Jacobi scaling s, the Cauchy direction v and the dense shares of the dogleg scalars, read through gfbe_debug_vector (which = 0,
2, 1 and 4) after ONE iteration, against the reduced system the device itself assembled (which = 1000 + r, 2000 + r, 3) restated in
numpy.longdouble (tests/solve_step_np.py). No forward comparison of y: its tolerance would depend on each window's conditioning; the
backward error of a correct Cholesky solve is a small multiple of u whatever the conditioning, and a dropped tile product, a wrong chain
block or a stale right-hand-side row breaks it by orders of magnitude. For accuracy this test replaces the kernel-against-kernel
comparison of tests/test_gpu_solve_kernels.py, which a defect shared by the kernels passes.

    eta = |S y - rhs|_inf / ( | |Ht| + mu D2 + |Et| |_inf |y|_inf + | |s g| + |s eg| |_inf )  <=  K_Y u            K_Y = %(K_Y)g
    s, v: relative error <= 4 u, 8 u     G2, N2, gy: within (ND + 3) u sum |term|     vHv, vHy, yHy: within K_S u A_X + B_X     K_S = %(K_S)g

K_Y = 16 eta_cpu and K_S = max(16 x the worst CPU scalar ratio, ND + 3), both rounded up to a power of two before the floor, with
eta_cpu = %(ETA_CPU)g u and the scalar ratio %(S_CPU)g (plain FP64 numpy: tests/test_solve_step_reference.py measures and asserts them).
mu is known a priori (GF_MIN_MU x 10^retries) and the device's reported mu must equal it bit for bit; grad_max must equal max |g|.

Windows (tests/solve_step_cases.py): the five of test_gpu_solve_kernels.py; n mod 16 = 15, 0, 1 (the right-hand side last in a full
tile, alone in a new tile row — the zlast path —, second in a tile); nd + 1 at a multiple of 16 and one above for the classic, two-ended
and nine-column chain kernels; a constant speed-bias block inside the chain; speed-bias blocks absent at the tail; the SpeedBias[2]
prior (monolithic fallback); six GNSS windows; robust; soak_349. Launch shapes: every window alone with solve_kernel 1, 2, 3, 0 (GNSS: 0
and 4); the non-GNSS windows at shuffled places of a batch of 33 (k_solve_chain, two workgroups per CU), the same batch with the
SpeedBias[2] prior in it (all 33 monolithic at full LDS), a batch of 36 mixing the GNSS windows with a plain one (the plain window runs
through k_solve_chain_wide); a window that occurs twice in a batch gives the same bits. Retries: gfbe_options.test_fail_chol_iter = 1
with test_fail_chol_count 1 and 2 — the same bounds at mu = 10 mu0 and 100 mu0 on the E that rebuild_E left, and that E against the
extended-precision E of normal_equations_np at the larger mu under that test's K.

Requested kernel -> kernel that runs: 1 k_solve; 2 k_solve_chain; 3 k_solve_chain_tw (k_solve_chain when the dense part has six tile
columns: all_free, nd80); 0 = 3 below 32 windows and 2 from there; GNSS batches: 0 k_solve_chain_wide, 4 k_solve_big; a prior with
another speed-bias block than SpeedBias[0]: k_solve whatever was asked.

Measured on an MI355X (worst over the windows; eta in u, the scalars as error / bound):
%(MEASURED)s
"""
import time

import numpy as np
import pytest

import normal_equations_np as ne
import solve_step_cases as sc
import solve_step_np as ss
from _gfbe_import import gf

abi = gf.abi
pytestmark = pytest.mark.gpu

MEASURED = """  launch shape (kernel that runs)                       eta/u     s/4u   v/8u      G2     N2     gy     vHv    vHy    yHy    worst eta
  alone, solve_kernel 1 (k_solve)                        4.96     0.36   0.32   0.006  0.007  0.006   0.005  0.004  0.005    all_free
  alone, solve_kernel 2 (k_solve_chain)                  1.72     0.36   0.32   0.006  0.008  0.012   0.005  0.004  0.004    prior
  alone, solve_kernel 3 and 0 (k_solve_chain_tw)         1.63     0.36   0.32   0.006  0.009  0.012   0.007  0.004  0.004    edge15
  alone, GNSS, solve_kernel 0 (k_solve_chain_wide)       1.21     0.36   0.30   0.005  0.004  0.008   0.007  0.003  0.001    gnss_a
  alone, GNSS, solve_kernel 4 (k_solve_big)              2.48     0.36   0.30   0.005  0.011  0.008   0.007  0.003  0.005    gnss_b
  retries 1 and 2, k_solve                               8.09     0.34   0.28   0.004  0.010  0.009   0.006  0.004  0.005    all_free
  retries 1 and 2, k_solve_chain / k_solve_chain_tw      3.19     0.34   0.28   0.004  0.010  0.010   0.006  0.006  0.005    all_free
  retries 1 and 2, k_solve_chain_wide / k_solve_big      1.92     0.36   0.27   0.000  0.003  0.007   0.004  0.003  0.004    gnss_a
  B = 33, k_solve_chain                                  2.21     0.36   0.32   0.009  0.006  0.008   0.007  0.004  0.004    partial
  B = 33 with the SpeedBias[2] prior, k_solve           10.97     0.36   0.32   0.009  0.007  0.010   0.010  0.003  0.005    all_free
  B = 36 with GNSS windows, k_solve_chain_wide           1.04     0.36   0.34   0.006  0.007  0.004   0.008  0.002  0.003    gnss_a
(eta/u against K_Y = 32; every other column is error / bound, 1.0 = at the bound. CPU, plain FP64 numpy: eta_cpu 1.71 u, vHv 3.06 u A.)
The subtracted scalars use a hundredth of their bound: B_X, the allowance for an inexact y at the full K_Y, is most of it — without it
vHv, the one scalar that has none, sits at 2.4 u A_X at most (CPU 3.06). The monolithic kernel on the window with every block free
(twelve tile steps, each through an explicitly inverted 16 x 16 diagonal tile) has the largest backward error, 5 to 11 u; every chain
kernel stays below 3.2 u. The rebuilt E of the retry cases is 139 to 230 u A_E from the extended-precision E at 10 mu0 and 100 mu0
(eg 18 to 88; K = 1024), the same as at mu0. Nothing exceeded a bound.
What the first run of this test did expose: gfbe_debug_vector handed out the 59 GNSS dims of a batch WITHOUT GNSS windows as they lay in
memory. No kernel of such a batch reads or writes them (BatchDev::nu = 187: upload plan, every loop of k_solve), so s came back as 0.0 or
as what an earlier batch of the context had left there, and H with stale diagonal entries — harmless to the solve, wrong for anyone who
reads the vectors. The call now reports those dims like inactive ones (0.0; s 1.0), on the host, after the copy.
Sensitivity (each built once, not committed; the 33 tests of this module / the 8 of test_gpu_solve_kernels.py that fail):
  chol_factor_all without the trailing product of tile (3, 2) at panel 1            33 / 7   (some windows lose positive definiteness)
  rsqrt_refined and rsq_stage without their two Newton steps (eta 3e6 to 6e7 u)     33 / 7   (the kernels amplify it differently)
  yHy without yEy in the chain kernels                                              31 / 1   (the two k_solve-only shapes pass, rightly;
                                                                                             of the old module only the whole solve of `prior`
                                                                                             fails, its step comparison does not read the scalars)"""
__doc__ = __doc__ % dict(K_Y=ss.K_Y, K_S=ss.K_S, ETA_CPU=ss.ETA_CPU, S_CPU=max(ss.S_CPU.values()), MEASURED=MEASURED)

SCALARS = ("G2", "N2", "gy", "vHv", "vHy", "yHy")
KERNELS_PLAIN, KERNELS_GNSS = (1, 2, 3, 0), (0, 4)


@pytest.fixture(scope="module")
def backends():
    ne.require_extended_precision()
    made = {}

    def get(kernel=0, fail_count=0):
        if (kernel, fail_count) not in made:
            o = abi.default_options()
            o.max_num_iterations, o.solve_kernel = 1, kernel
            if fail_count:
                o.test_fail_chol_iter, o.test_fail_chol_count = 1, fail_count
            made[(kernel, fail_count)] = gf.Backend(device=0, options=o)
        return made[(kernel, fail_count)]
    yield get
    for b in made.values():
        b.close()


def read_system(batch, w):
    got = ne.device_system(batch, w)
    got["Hs"] = ss.symmetrise(got["H"])
    return got


def read_step(batch, w):
    sc8 = batch.debug_vector(4, w)
    assert not sc8[8:].any()
    return dict(y=batch.debug_vector(0, w), v=batch.debug_vector(1, w), s=batch.debug_vector(2, w), scal=sc8[:8].copy())


def judge(name, sysd, step, retries, label, worst):
    """Every check of solve_step_np on one window; returns the list of failures and folds the ratios into `worst`."""
    fails = []
    H = sysd["Hs"]
    n_nd = sc.counts_of(ss.active_mask(H))
    if n_nd != sc.EXPECTED_N[name]:
        fails.append("%s %s: (n, nd) = %s, expected %s" % (name, label, n_nd, sc.EXPECTED_N[name]))
    mu = ss.mu_of(retries)
    scal = dict(zip(("mu",) + SCALARS + ("grad_max",), step["scal"].tolist()))
    if scal["mu"] != mu:
        fails.append("%s %s: the factorisation's mu is %.17g, expected %.17g" % (name, label, scal["mu"], mu))
    gmax = np.abs(sysd["g"][ss.active_mask(H)]).max()
    if scal["grad_max"] != gmax:
        fails.append("%s %s: grad_max %.17g is not max |g| = %.17g" % (name, label, scal["grad_max"], gmax))
    ratios, raw, exact = ss.check_all(H, sysd["g"], sysd["E"], sysd["eg"], step["s"], step["v"], step["y"], scal, mu)
    fails += ["%s %s: %s" % (name, label, e) for e in exact]
    shown = dict(ratios, eta_u=ratios["y"] * ss.K_Y)
    for k, r in shown.items():
        worst[k] = max(worst.get(k, 0.0), r)
    print("%-11s %-24s eta/u %6.2f  s %.2f v %.2f  " % (name, label, shown["eta_u"], ratios["s"], ratios["v"]) +
          "  ".join("%s %.3f" % (k, ratios[k]) for k in SCALARS) + "   raw vHv %.2f vHy %.2f yHy %.2f" % (raw["vHv"], raw["vHy"], raw["yHy"]))
    for k, r in ratios.items():
        if not r <= 1.0:
            fails.append("%s %s: %s is at %.3g x its bound%s" % (name, label, k, r, " (eta = %.3g u > K_Y = %g u)" % (shown["eta_u"], ss.K_Y) if k == "y" else ""))
    return fails


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("y", "v", "s", "scal"))


def run_alone(backends, snap, kernel, fail_count=0):
    b = backends(kernel, fail_count).batch_upload([snap])
    try:
        b.solve(abi.MARGIN_NONE)
        assert b.download()[0]["summary"]["iterations"] == 1
        return b, read_step(b, 0)
    except BaseException:
        b.free()
        raise


@pytest.mark.parametrize("name", list(sc.EXPECTED_N))
def test_one_window_alone(backends, oracle, name):
    """B = 1 with every solve kernel that can be asked for. H, E, eg are read once (the linearisation does not depend on the solve
    kernel: g must come back with the same bits)."""
    snap = sc.build(name, oracle)
    fails, sysd = [], None
    for kernel in (KERNELS_GNSS if name in sc.GNSS else KERNELS_PLAIN):
        b, step = run_alone(backends, snap, kernel)
        try:
            if sysd is None:
                sysd = read_system(b, 0)
            else:
                assert np.array_equal(b.debug_vector(3, 0), sysd["g"]), (name, kernel)
        finally:
            b.free()
        fails += judge(name, sysd, step, 0, "alone kernel=%d" % kernel, {})
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", ["prior", "all_free", "edge0", "gnss_a"])
@pytest.mark.parametrize("count", [1, 2])
def test_injected_retries_alone(backends, oracle, name, count):
    """The first `count` factorisations of the iteration report a bad pivot (in software): the step that comes out belongs to
    mu = 10^count mu0 and to the E rebuild_E formed for it — read back after the solve and held against the extended-precision E at that mu
    (the windows without GNSS factors, which that reference covers)."""
    snap = sc.build(name, oracle)
    mu = ss.mu_of(count)
    fails = []
    ref = None if name in sc.GNSS else ne.reference_system(snap, oracle.eval_factors(snap, robustify=True), mu=mu)
    for kernel in (KERNELS_GNSS if name in sc.GNSS else KERNELS_PLAIN[:3]):
        b, step = run_alone(backends, snap, kernel, count)
        try:
            sysd = read_system(b, 0)
        finally:
            b.free()
        fails += judge(name, sysd, step, count, "retries=%d kernel=%d" % (count, kernel), {})
        if ref is not None:
            ratios, f = ne.compare_system(sysd, ref, ne.K, "%s retries=%d kernel=%d:" % (name, count, kernel))
            print("%-11s rebuilt E against the reference at mu = %.0e: " % (name, mu) + "  ".join("%s %.1f" % kv for kv in ratios.items()))
            fails += f
    assert not fails, "\n".join(fails)


def check_batch(backends, oracle, names, order, label):
    snaps = [sc.build(names[q], oracle) for q in order]
    t0 = time.time()
    b = backends(0).batch_upload(snaps)
    fails, worst, first = [], {}, {}
    try:
        b.solve(abi.MARGIN_NONE)
        res = b.download()
        for w, q in enumerate(order):
            assert res[w]["summary"]["iterations"] == 1
            if q not in first:
                step = read_step(b, w)
                fails += judge(names[q], read_system(b, w), step, 0, label, worst)
                first[q] = (w, step)
            elif sum(1 for p in order[:w] if p == q) == 1:      # the second occurrence: the same bits at another place
                if not same_bits(read_step(b, w), first[q][1]):
                    fails.append("%s: y, v, s or the scalars differ between places %d and %d of the batch" % (names[q], first[q][0], w))
    finally:
        b.free()
    print("%s: worst %s  (%.1f s)" % (label, {k: round(v, 3) for k, v in worst.items()}, time.time() - t0))
    assert len(first) == len(names)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mix", ["chain", "mono"])
def test_batch_of_33(backends, oracle, mix):
    """Every non-GNSS window at shuffled places of a batch of 33 with solve_kernel = 0: the one-ended chain, two workgroups per CU.
    `mono`: with the SpeedBias[2] prior in it the whole batch takes k_solve, 33 workgroups at full LDS."""
    names = [n for n in sc.PLAIN if mix == "mono" or n != "sb2_prior"]
    rng = np.random.default_rng(33 + len(names))
    order = np.concatenate([rng.permutation(len(names)) for _ in range(33 // len(names) + 1)])[:33]
    check_batch(backends, oracle, names, order, "B=33 %s" % mix)


def test_batch_of_36_with_gnss_windows(backends, oracle):
    """The GNSS windows and a plain one in a batch of 36: every window, the plain one included, runs through k_solve_chain_wide."""
    names = sc.GNSS + ["first"]
    order = [len(sc.GNSS) if i % 4 == 0 else (i - i // 4 - 1) % len(sc.GNSS) for i in range(36)]
    check_batch(backends, oracle, names, np.array(order), "B=36 gnss")
