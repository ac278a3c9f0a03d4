"""CPU checks of the extended-precision model of the new prior (tests/prior_np.py) and of the windows the GPU comparison runs on
(tests/test_gpu_prior.py).

Per case: the size of the new prior, the condition on the dropped block (every eigenvalue > 1e3 marg_eps: the reference's
pseudo-inverse is the inverse), a_scale <= A_SCALE_MAX, and the gap condition on the discrete results (no eigenvalue of A_ref and
no LDL^T pivot inside [marg_eps / G, marg_eps G], G = %(G)g: every case keeps all n rows in both modes — see prior_np's
docstring for why a rank-deficient prior cannot meet it).

Per case and square root (marg_sqrt 0: eigen, 1: pivoted LDL^T), two FP64 constructions against the model — the oracle's
gfo_marginalize and a plain numpy statement (sums, Schur complement by Cholesky, eigh with threshold / numpy_pivoted_ldlt_sqrt) —
on the quantities of prior_np.check_prior, in units of u = 2^-53:
    rA = max(|J0^T J0 - A_ref| - marg_eps, 0)_max / a_scale
    rb = |J0^T r0 - P b_ref|_max / max(b_scale, 1e-2 a_scale),  P the projector on the row space of the J0 under test
    ro = largest off-diagonal entry of J0 J0^T / its largest diagonal entry (eigen mode)
with the block table, x0 and the number of non-zero rows exact.

Sizes reached (n_out): MARGIN_OLD 85, 86, 87, 88, 89, 90, 91, 132, 133, 176, 177, 71 (first GNSS window), 76 (first window
without wheel); MARGIN_SECOND_NEW 91 -> 85 and 96 -> 90.

Largest CPU ratios r_cpu, measured 77.35 / 213.7 / 7.696 and recorded rounded up (asserted below): rA %(rA).4g (the oracle's
eigen mode on old_91; the numpy Cholesky statement stays under 5), rb %(rb).4g (the oracle's eigen mode on the GNSS window),
ro %(ro).4g (the oracle on old_85). Device bounds K = smallest power of two >= 4 r_cpu: rA %(KA)g, rb %(Kb)g, ro %(Ko)g.
"""
import numpy as np
import pytest

import normal_equations_np as ne
import prior_np as pn
from _gfbe_import import gf

abi = gf.abi
__doc__ = __doc__ % dict(pn.R_CPU, G=pn.G, KA=pn.K["rA"], Kb=pn.K["rb"], Ko=pn.K["ro"])


@pytest.fixture(autouse=True)
def _extended_precision():
    ne.require_extended_precision()


def test_bound_constants_follow_from_the_measurement():
    for q, r in pn.R_CPU.items():
        assert pn.K[q] == 2.0 ** np.ceil(np.log2(4.0 * r)) and pn.K[q] >= 4.0 * r > pn.K[q] / 2
    assert pn.G - 1 >= 64 * pn.U * pn.A_SCALE_MAX / pn.MARG_EPS and pn.G == 2.0 ** 20


def test_the_sizes_sit_on_every_boundary_of_the_launch_logic():
    old = sorted(c[5] for c in pn.CASES.values() if c[4] == abi.MARGIN_OLD and c[0] == "grown")
    assert old == [85, 86, 87, 88, 89, 90, 91, 132, 133, 176, 177]
    assert sorted(c[5] for c in pn.CASES.values() if c[4] == abi.MARGIN_SECOND_NEW) == [85, 90]
    assert max(len(e) for e in pn.EXTRA.values()) + 18 <= abi.MAX_PRIOR_BLOCKS


@pytest.mark.parametrize("name", list(pn.CASES))
def test_case_meets_its_conditions(oracle, name):
    kind, seed, base, extra, flag, n_out = pn.CASES[name]
    snap, flag, ref = pn.case_reference(name, oracle)
    assert ref["n"] == n_out
    if kind == "grown":
        assert snap["prior"]["n"] == 86 + extra and sum(abi.block_local_size(b) for b in pn.EXTRA[extra]) == extra
        plain, _, _, rc = oracle.marginalize(dict(snap, prior=pn.grow_prior(pn._cache[("second", seed)][2], snap, [], 0)), abi.MARGIN_OLD)
        assert rc == 0 and plain["n"] == base                      # what the prior gives without extra blocks
        assert n_out == (base if flag == abi.MARGIN_OLD else 86 - 6) + extra
    else:      # a first window: the identity prior lists only blocks the marginalisation set touches anyway
        bare, _, _, rc = oracle.marginalize(dict(snap, prior=None), flag)
        assert rc == 0 and bare["n"] == n_out and bare["block_id"].tolist() == list(ref["block_id"])
        assert ref["n_dropped"] - len(set(np.asarray(snap["vis_feature_index"])[np.asarray(snap["vis_imu_i"]) == 0].tolist())) == (20 if kind == "gnss" else 15)
    assert len(snap["prior"]["block_id"]) <= abi.MAX_PRIOR_BLOCKS and len(ref["block_id"]) <= abi.MAX_PRIOR_BLOCKS
    assert ref["dropped_min_eig"] > pn.DROP_MARGIN * pn.MARG_EPS
    assert ref["a_scale"] <= pn.A_SCALE_MAX
    eig_in, piv_in = pn.gap_violations(ref)
    assert not eig_in and not piv_in, (eig_in, piv_in)
    assert ref["rank"] == {0: n_out, 1: n_out} and ref["eig"].min() > pn.MARG_EPS * pn.G


def test_host_bound_of_the_cases(oracle):
    """marg_nmax of a batch decides which LDL^T kernels are launched: WITHIN_88 are exactly the MARGIN_OLD cases bounded by 88."""
    bound = {n: pn.host_marg_bound(pn.build_case(n, oracle)[0]) for n, c in pn.CASES.items() if c[4] == abi.MARGIN_OLD}
    assert sorted(n for n, b in bound.items() if b <= 88) == sorted(pn.WITHIN_88)
    assert [bound[n] for n in pn.WITHIN_88] == [86, 87, 88] and bound["old_85"] == bound["gnss"] == bound["nowheel"] == 91
    for n, b in bound.items():
        assert b >= pn.CASES[n][5]


_measured = {}


def cpu_ratios(oracle, name, mode):
    if (name, mode) not in _measured:
        snap, flag, ref = pn.case_reference(name, oracle)
        pr, _, _, rc = oracle.with_options(marg_sqrt=mode).marginalize(snap, flag)
        assert rc == 0
        _measured[(name, mode)] = (pn.check_prior(pr, ref, mode, "oracle " + name), pn.check_prior(pn.fp64_prior(oracle, snap, flag, mode), ref, mode, "numpy " + name))
    return _measured[(name, mode)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(pn.CASES))
def test_oracle_and_numpy_against_the_model(oracle, name, mode):
    got_o, got_n = cpu_ratios(oracle, name, mode)
    print(name, "marg_sqrt", mode, "oracle", {q: "%.3g" % v for q, v in got_o.items()}, "numpy", {q: "%.3g" % v for q, v in got_n.items()})
    for got in (got_o, got_n):
        for q, v in got.items():
            assert v <= pn.R_CPU[q], (name, mode, q, v)
    for q, v in got_o.items():      # the oracle itself is within the device bound
        assert v <= pn.K[q]


def test_r_cpu_is_the_largest_measured_ratio(oracle):
    worst = dict(rA=0.0, rb=0.0, ro=0.0)
    for name in pn.CASES:
        for mode in (0, 1):
            for got in cpu_ratios(oracle, name, mode):
                for q, v in got.items():
                    worst[q] = max(worst[q], v)
    print("r_cpu", worst)
    for q in worst:      # the recorded figure is the measured one rounded up, by a tenth at the most
        assert worst[q] <= pn.R_CPU[q] <= 1.1 * worst[q], (q, worst[q], pn.R_CPU[q])


def test_ldlt_statement_moved_here_is_the_one_the_oracle_test_uses():
    import test_oracle_solver as tos
    assert tos.numpy_pivoted_ldlt_sqrt is pn.numpy_pivoted_ldlt_sqrt
