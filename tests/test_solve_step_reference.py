"""CPU half of the backward-error check of the reduced-system solve (tests/solve_step_np.py; the device half is
tests/test_gpu_solve_step.py): on every window of tests/solve_step_cases.py a plain FP64 solve — numpy.linalg.cholesky and two
triangular solves of S formed in FP64, the dogleg scalars restated in the device's term grouping — is judged by the checker's
longdouble residual. That is the measurement behind K_Y and K_S (asserted, so that the constants cannot drift), and the place where
the checker is shown to see what it is for: six defects injected into the FP64 solve each leave their bound by at least 100 x.

H, g, E, eg: the extended-precision reference of normal_equations_np rounded to FP64. That reference does not know the GNSS factors, so
the GNSS windows take the oracle's FP64 linearisation and an FP64 contraction of E (normal_equations_np.fp64_system) instead.

Measured over the 22 windows at mu0 and 100 mu0: eta_cpu 1.71 u (prior at 100 mu0), vHv 3.06 u A (gnss_nd127); vHy and yHy stay inside B_X.
The defects leave their bounds by 1e6 (mu a decade too large) to 1e13 (the stale right-hand side row). The module's 98 tests take 12 s."""
import numpy as np
import pytest

import normal_equations_np as ne
import solve_step_cases as sc
import solve_step_np as ss
from _gfbe_import import gf

abi = gf.abi
_sys = {}


@pytest.fixture(autouse=True)
def _extended_precision():
    ne.require_extended_precision()


def fp64_inputs(name, oracle):
    if name not in _sys:
        snap = sc.build(name, oracle)
        if name in sc.GNSS:
            lin = ne.fp64_system(oracle, snap)
            H, g, E, eg = lin["H"], lin["g"], lin["E"], lin["eg"]
        else:
            ref = ne.reference_system(snap, oracle.eval_factors(snap, robustify=True))
            H, g, E, eg = (np.asarray(ref[k], float) for k in ("H", "g", "E", "eg"))
        _sys[name] = (ss.symmetrise(H), np.asarray(g, float), np.asarray(E, float)[:ne.NV, :ne.NV], np.asarray(eg, float)[:ne.NV])
    return _sys[name]


def test_constants_follow_from_the_measurement():
    assert ss.K_MARGIN == 16.0
    assert ss.K_Y == 2.0 ** np.ceil(np.log2(16.0 * ss.ETA_CPU))
    assert ss.K_S == max(2.0 ** np.ceil(np.log2(16.0 * max(ss.S_CPU.values()))), ne.ND + 3)
    assert (ss.GF_MIN_MU, ss.GF_MU_INC, ss.GF_MIN_DIAG, ss.GF_MAX_DIAG) == (1e-8, 10.0, 1e-6, 1e32)
    assert ss.mu_of(0) == 1e-8 and abs(ss.mu_of(2) - 1e-6) < 1e-20


@pytest.mark.parametrize("name", list(sc.EXPECTED_N))
def test_case_has_the_expected_active_dims(oracle, name):
    H = fp64_inputs(name, oracle)[0]
    n, nd = sc.counts_of(ss.active_mask(H))
    print("%s: n = %d (n mod 16 = %d), nd = %d" % (name, n, n % 16, nd))
    assert sc.EXPECTED_N[name] == (n, nd)


def test_tile_and_column_edges_are_reached():
    N = sc.EXPECTED_N
    assert [N[k][0] % 16 for k in ("edge15", "edge0", "edge1")] == [15, 0, 1]
    assert [(N[k][1] + 1) % 16 for k in ("nd63", "nd64", "nd79", "nd80", "gnss_nd127", "gnss_nd128")] == [0, 1, 0, 1, 0, 1]
    assert N["gnss_nd141"][1] == 141 and N["all_free"][1] + 1 > 5 * 16


@pytest.mark.parametrize("name", list(sc.EXPECTED_N))
@pytest.mark.parametrize("retries", [0, 2])
def test_fp64_solve_is_within_the_measured_ratios(oracle, name, retries):
    """eta / u <= ETA_CPU and the raw scalar ratios <= S_CPU for the plain FP64 solve (the measurement of K_Y, K_S); every check of
    the checker passes on it. retries = 2: at mu = 100 mu0 (E of the first linearisation: only the solve is under test here)."""
    H, g, E, eg = fp64_inputs(name, oracle)
    mu = ss.mu_of(retries)
    out = ss.fp64_solve(H, g, E, eg, mu)
    ratios, raw, exact = ss.check_all(H, g, E, eg, out["s"], out["v"], out["y"], out, mu)
    print("%-12s mu %.0e  eta/u %.3f  s %.2f  v %.2f  sums %s  raw %s" % (
        name, mu, ratios["y"] * ss.K_Y, ratios["s"] * ss.S_TOL, ratios["v"] * ss.V_TOL,
        {k: round(ratios[k] * ss.SUM_TOL, 2) for k in ("G2", "N2", "gy")}, {k: round(raw[k], 3) for k in ("vHv", "vHy", "yHy")}))
    assert not exact, exact
    assert ratios["y"] * ss.K_Y <= ss.ETA_CPU
    for k in ("vHv", "vHy", "yHy"):
        assert raw[k] <= ss.S_CPU[k], (k, raw[k])
    assert all(r <= 1.0 for r in ratios.values()), ratios


MUTATIONS = {"tile_product": "y", "rhs_row": "y", "mu_decade": "y", "E_row": "y", "sb_coupling": "y", "no_yEy": "yHy"}


@pytest.mark.parametrize("name", ["prior", "all_free", "edge0", "partial", "gnss_a"])
@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_checker_sees_the_defect(oracle, name, mutation):
    """One 16-row block of the substitution without one off-diagonal tile, the right-hand side row read a tile row too early, mu a decade
    too large, E with one row and column zeroed, a speed-bias block without its coupling to the next one: eta leaves K_Y u by >= 100 x.
    yHy without yEy: leaves its bound by >= 100 x."""
    H, g, E, eg = fp64_inputs(name, oracle)
    mu = ss.mu_of(0)
    out = ss.fp64_solve(H, g, E, eg, mu, mutate=mutation)
    ratios, raw, exact = ss.check_all(H, g, E, eg, out["s"], out["v"], out["y"], out, mu)
    key = MUTATIONS[mutation]
    print("%s %s: %s ratio %.3g" % (name, mutation, key, ratios[key]))
    assert ratios[key] >= 100.0, (mutation, ratios)
