"""CPU checks of the extended-precision pose-graph model (tests/posegraph_np.py), of the oracle (oracle/gfo_posegraph.cpp) against
it, and of the bounds the device comparison runs on (tests/test_gpu_posegraph_model.py). Nothing here needs a GPU.

The model alone. The Romberg difference quotients resolve every Jacobian block to below posegraph_np.JAC_ERR = 1e-13 of the block's
scale (measured: 1e-19, the longdouble rounding of the quotients), the structural zeros come out as exact zeros, the dense LDL^T and
the block recurrence agree on the step of n33 (SOLVER_AGREEMENT below), and every decision of the fifteen-iteration loops — rho against
1e-3, the gradient, parameter and function tolerances, the sign of the model change — is at least posegraph_np.MARGIN_MIN = 1e-6
(relative) away from its threshold: measured minimum 0.10 (the gradient test that ends one_fix). Rounding decides none of these runs.

The oracle. gfo_pg_eval on every factor case, block by block, under K_FACTOR; gfo_pg_solve with max_iterations = 1 and 15 on the solve
cases: the model's accept sequence, iteration count, termination and status, and poses and costs within the stored floors. No
disagreement was found: the hand-derived Jacobians of the oracle (and with them the device's, which are the same formulas) are the
derivatives of the reference's functors through QuaternionParameterization::Plus, non-unit quaternions and rotations next to pi
included.

Deriving the bounds (posegraph_np.K_MEASURED, K_FACTOR, STEP_FLOOR, LOOP_FLOOR; figures in that module's docstring). Every figure is
measured here and asserted against the stored one from both sides, so none is a loose cover: K_MEASURED to within 15 %% (the oracle
and this module's own FP64 formulas are deterministic), the floors — stored as 1.25 x the measurement, rounded up — to within [1/4, 1] of the stored value (pcr_fp64
spells its FP64 products out term by term, so that no host's BLAS decides a figure).
pcr_fp64, the device's method in plain FP64 numpy, stays at the oracle's level on every case, one_fix and split included (worst
pcr_fp64 / oracle: 2.2 on one_fix and on huber): cyclic reduction with explicit inverses loses nothing measurable on these Levenberg-Marquardt
systems, whose smallest diagonal is clamp(diag) / 1e4.

Sharpness. Each mutation below was applied once to a scratch copy of oracle/gfo_posegraph.cpp (nothing of it is committed) and this
module was run against the mutated library. "old check, one-sided": whether the comparisons of tests/test_gpu_posegraph.py (its ten
CPU-runnable cases and tolerances, the unmutated oracle standing in for the device) notice the mutated library, i.e. whether the
oracle-against-device style of check sees the mistake when only ONE side makes it. A mistake both sides share (they were written
from the same formulas by the same hand) is invisible to it by construction, whatever this column says; every row that fails here
fails whoever else makes the same mistake.
%(SHARP)s
"""
import numpy as np
import pytest

import posegraph_np as pg
from _gfbe_import import gf

abi = gf.abi
LD = pg.LD
SOLVER_AGREEMENT = 1e-15        # |y dense - y recurrence| / max |y|: both are backward stable in longdouble (u_ld = 5.4e-20) and the regularised
#                                 system's condition is <= max diag / (1e-6 / 1e4) ~ 1e4 on n33 (diag2 ~ 1): 5.4e-20 * 1e4 with a factor 2 to spare

SHARPNESS = """\
    mutation                                        tests of this module that fail                                              old check, one-sided
    sign of the dq_i rotation block                 factor_blocks (5 cases), first_step (11), whole_loop (10), factor_floor     seen (all 10 cases)
    factor 2 of the quaternion Jacobian dropped     factor_blocks (5), first_step (11), whole_loop (10), factor_floor           seen (all 10)
    rs not applied to the Huber residual            factor_blocks (5), first_step (10), whole_loop (9), factor_floor            seen (all 10)
    Ho used untransposed (back substitution)        first_step (11), whole_loop (10)                                            seen (9: every solve)
    diag2 recomputed on a rejected step             NONE - see below                                                            not seen
    diag2 kept after an ACCEPTED step               whole_loop (n33, n64, split: a rejection followed by an accepted step)      seen (1 case of 10)
    fix_r returned in sorted order                  factor_blocks (mixed, gaps, nonunit, near_pi, far), factor_floor            NOT seen
  The fifth mutation changes nothing, here or anywhere: a rejected step leaves x where it was, the linearisation at x is not formed
  again, and clamp(diag(S H S)) of the same H is the same diag2 to the bit — for the oracle (L is re-evaluated only on acceptance) as
  for the device (PgState::lb keeps pointing at the set linearised at x). Ceres keeps the diagonal to save the work, not to change the
  value. No test can fail on it; the mutation next to it that does change the value (the diagonal kept across an accepted step)
  is in the table instead and fails three whole-loop cases. fix_r in sorted order is invisible to the old check even one-sided:
  every graph of synth.pose_graph has its fixes sorted."""
__doc__ = __doc__ % dict(SHARP=SHARPNESS)


@pytest.fixture(scope="module", autouse=True)
def _extended_precision():
    pg.require_extended_precision()


@pytest.fixture(scope="module")
def orc(oracle):
    return abi.PoseGraph(oracle.lib, "gfo_", None)


def _pose_diff(a, b):
    return float(np.max(np.abs(np.asarray(a, LD) - b)))


def test_status_codes_and_constants():
    assert (pg.OK, pg.NO_CONVERGENCE, pg.NUMERICAL_FAILURE, pg.BAD_INPUT) == (abi.OK, abi.NO_CONVERGENCE, abi.NUMERICAL_FAILURE, abi.BAD_INPUT)
    top = pg.K_MARGIN * max(pg.K_MEASURED.values())
    assert pg.K_FACTOR == 2.0 ** np.ceil(np.log2(top)) and pg.K_MARGIN == 8.0 and pg.STEP_MARGIN == 16.0
    assert set(pg.STEP_FLOOR) == set(pg.SOLVE_CASES) and set(pg.LOOP_FLOOR) == set(pg.LOOP_CASES)
    assert pg.LOOP_CASES == ("n1", "n2", "n3", "n32", "n33", "n64", "n65", "n257", "one_fix", "split", "huber")


def test_cases_are_what_their_names_say():
    n = {name: len(pg.case(name)["pose"]) for name in pg.FACTOR_CASES + pg.COST_CASES + pg.SOLVE_CASES}
    assert [n[k] for k in pg.FACTOR_CASES] == [33, 65, 33, 9, 33, 1, 1]
    assert [n[k] for k in pg.COST_CASES] == [4097, 8200]
    assert [n[k] for k in pg.SOLVE_CASES] == [1, 2, 3, 32, 33, 64, 65, 257, 1025, 65, 65, 64]
    g, ref = pg.case("mixed"), pg.reference_eval("mixed")
    ri, fi = g["rel_i"].tolist(), g["fix_i"].tolist()
    assert sorted(ri) == list(range(32)) and ri != sorted(ri)
    assert fi != sorted(fi) and fi.count(8) == 2 and len(set(fi)) == len(fi) - 1
    k8 = [k for k, i in enumerate(fi) if i == 8]
    assert k8[1] - k8[0] > 1 and not np.array_equal(g["fix_meas"][k8[0]], g["fix_meas"][k8[1]])
    sq = np.sum(ref["fix_raw"] ** 2, axis=1)
    assert sq[fi.index(12)] > 1e3 and ref["outlier"][fi.index(12)] and sq[fi.index(16)] == 0 and not ref["fix_r"][fi.index(16)].any()
    assert ref["outlier"].any() and not ref["outlier"].all()
    g = pg.case("gaps")
    assert sorted(set(range(64)) - set(g["rel_i"].tolist())) == [0, 31, 63]
    g = pg.case("nonunit")
    for q in (g["pose"][:, 3:], g["rel_meas"][:, 3:]):
        d = np.abs(np.linalg.norm(q, axis=1) - 1)
        assert d.min() > 4e-4 and d.max() < 1.1e-3
    g = pg.case("near_pi")
    e = pg.qmul(pg.qconj(g["rel_meas"][:, 3:]), pg.qmul(pg.qconj(g["pose"][:-1, 3:]), g["pose"][1:, 3:]))
    ang = 2 * np.arctan2(np.linalg.norm(e[:, 1:], axis=1), np.abs(e[:, 0]))
    assert np.abs(ang - np.pi).max() < 1e-3 * (1 + 1e-9) and np.abs(ang - np.pi).max() > 5e-4 and np.abs(e[:, 0]).max() < 5.1e-4
    g = pg.case("far")
    assert np.abs(g["pose"][:, :3]).min() > 9.9e3 and np.abs(g["fix_meas"][:, :3]).min() > 9.9e3
    assert len(pg.case("single")["fix_i"]) == 1 and len(pg.case("empty")["fix_i"]) == 0 and len(pg.case("empty")["rel_i"]) == 0
    for name in pg.SOLVE_CASES[:9]:
        g = pg.case(name)
        fi = g["fix_i"].tolist()
        assert sorted(fi) == list(range(0, n[name], 5)) and (len(fi) < 3 or fi != sorted(fi)) and len(g["rel_i"]) == n[name] - 1
    assert pg.case("one_fix")["fix_i"].tolist() == [64]
    g = pg.case("split")
    assert sorted(set(range(64)) - set(g["rel_i"].tolist())) == [20, 43]
    assert not [i for i in g["fix_i"] if 21 <= i <= 43] and [i for i in g["fix_i"] if i <= 20] and [i for i in g["fix_i"] if i >= 44]
    assert pg.residuals(pg.case("huber"))["outlier"].sum() >= 10


def test_near_pi_has_a_negated_measurement():
    g, plain = pg.case("near_pi"), pg.case("near_pi")
    plain["rel_meas"][3, 3:] *= -1
    a, b = pg.residuals(g)["rel_r"], pg.residuals(plain)["rel_r"]
    assert np.array_equal(a[3, 3:], -b[3, 3:]) and np.array_equal(np.delete(a, 3, 0), np.delete(b, 3, 0)) and np.array_equal(a[3, :3], b[3, :3])


@pytest.mark.parametrize("name", pg.FACTOR_CASES + ("n65", "huber"))
def test_difference_quotients_resolve_the_jacobian(name):
    ref = pg.reference_eval(name)
    E, S, J = ref["J_err"], ref["J_scale"], ref["rel_J"]
    if not E.size:
        return
    worst = float(np.max(E[S > 0] / S[S > 0]))
    print("%-8s Romberg error estimate / block scale: %.2e" % (name, worst))
    assert worst < pg.JAC_ERR
    assert not J[S == 0].any() and not E[S == 0].any()
    assert (np.abs(J[:, 3:, 0:3] + J[:, 3:, 6:9]) <= 2 * pg.JAC_ERR * S[:, 3:, 0:3]).all()      # d e / d dq_i = -d e / d dq_j, whatever the norms


def test_dense_and_recurrence_solvers_agree():
    g = pg.case("n33")
    lin = pg.linearise(g)
    a = pg.lm_system(g, 1e4, lin=lin, solver=pg.solve_dense)
    b = pg.lm_system(g, 1e4, lin=lin, solver=pg.solve_recurrence)
    gap = float(np.max(np.abs(a["y"] - b["y"])) / np.max(np.abs(a["y"])))
    res = pg.block_matvec(a["Breg"], a["As"], a["y"]) - a["rhs"]
    print("dense against recurrence: %.2e   residual of the dense step: %.2e" % (gap, float(np.max(np.abs(res)) / np.max(np.abs(a["rhs"])))))
    assert gap < SOLVER_AGREEMENT
    assert np.max(np.abs(res)) < 1e-17 * np.max(np.abs(a["rhs"]))
    assert 6 * 33 <= pg.DENSE_MAX < 6 * 257


def _measure_factor_floor(orc):
    worst = {}
    for name in pg.FACTOR_CASES + pg.COST_CASES:
        g = pg.case(name)
        if name in pg.COST_CASES:
            res = pg.residuals(g)
            for c in (orc.eval(g)["cost"], pg.fp64_eval(g)["cost"]):
                pg.merge_ratios(worst, dict(cost=pg._ratio(c, res["cost"], res["cost_scale"])))
            continue
        ref = pg.reference_eval(name)
        pg.merge_ratios(worst, pg.compare_eval(orc.eval(g), ref))
        pg.merge_ratios(worst, pg.compare_eval(pg.fp64_eval(g), ref))
    return worst


def test_the_measured_factor_floor_is_the_stored_one(orc):
    worst = _measure_factor_floor(orc)
    print("floor:", "   ".join("%s %.3g" % kv for kv in worst.items()))
    assert worst.pop("J_zeros") == 0.0
    assert set(worst) == set(pg.FAMILIES)
    for fam, r in worst.items():
        assert 0.85 * pg.K_MEASURED[fam] <= r <= pg.K_MEASURED[fam], (fam, r)


@pytest.mark.parametrize("name", pg.FACTOR_CASES)
def test_oracle_factor_blocks_match_the_model(orc, name):
    g, ref = pg.case(name), pg.reference_eval(name)
    got = orc.eval(g)
    ratios = pg.compare_eval(got, ref)
    print("%-8s " % name + "   ".join("%s %.3g" % kv for kv in ratios.items()))
    for fam, r in ratios.items():
        assert r <= pg.K_FACTOR, (name, fam, r)


def _first_step(orc, name):
    """(oracle result, model run, |oracle - model| of the pose, |pcr_fp64 - model| of the candidate)."""
    g, m = pg.case(name), pg.reference_solve(name, 1)
    o = orc.solve(g, max_iterations=1)
    S = pg.lm_system(g, 1e4)
    y = pg.pcr_fp64(S["Breg"], S["As"], S["rhs"])
    cand = pg.plus(np.asarray(g["pose"], LD), S["scale"] * np.asarray(y, LD))
    return o, m, _pose_diff(o["pose"], m["pose"]), _pose_diff(cand, m["first"]["candidate"])


@pytest.mark.parametrize("name", pg.SOLVE_CASES)
def test_oracle_first_step_matches_the_model(orc, name):
    o, m, d_or, d_pcr = _first_step(orc, name)
    so = o["summary"]
    print("%-8s first step: |oracle - model| %.3g   |pcr_fp64 - model| %.3g   stored %.3g" % (name, d_or, d_pcr, pg.STEP_FLOOR[name]))
    assert (so["iterations"], so["accepted"], so["termination"], so["status"]) == (m["iterations"], m["accepted"], m["termination"], m["status"])
    assert m["accepted"] == [0, 1]                    # every case's first step is accepted: pose_out is the candidate
    floor = max(d_or, d_pcr)
    assert 0.25 * pg.STEP_FLOOR[name] <= floor <= pg.STEP_FLOOR[name]
    pg.check_first_costs(pg.case(name), o["pose"], so["cost_history"], "oracle %s:" % name)


@pytest.mark.parametrize("name", pg.LOOP_CASES)
def test_oracle_whole_loop_matches_the_model(orc, name):
    m = pg.reference_solve(name, 15)
    o = orc.solve(pg.case(name), max_iterations=15)
    so = o["summary"]
    assert (so["iterations"], so["accepted"], so["termination"], so["status"]) == (m["iterations"], m["accepted"], m["termination"], m["status"])
    d_pose = _pose_diff(o["pose"], m["pose"])
    d_cost = float(max(abs(LD(a) - b) for a, b in zip(so["cost_history"], m["cost_history"])) / m["cost_history"][0])
    print("%-8s %2d iterations, termination %d: |pose| %.3g   |cost history| / initial cost %.3g   stored (%.3g, %.3g)"
          % ((name, m["iterations"], m["termination"], d_pose, d_cost) + tuple(pg.LOOP_FLOOR[name])))
    assert 0.25 * pg.LOOP_FLOOR[name][0] <= d_pose <= pg.LOOP_FLOOR[name][0]
    assert 0.25 * pg.LOOP_FLOOR[name][1] <= d_cost <= pg.LOOP_FLOOR[name][1]


@pytest.mark.parametrize("name", pg.LOOP_CASES)
def test_no_decision_of_the_model_is_a_matter_of_rounding(name):
    m = pg.reference_solve(name, 15)
    worst = min(m["margins"], key=lambda t: t[2])
    print("%-8s accepted %s termination %d   closest decision: %s of iteration %d, %.3g" % ((name, "".join(map(str, m["accepted"])), m["termination"]) + worst))
    assert worst[2] > pg.MARGIN_MIN
    assert len([t for t in m["margins"] if t[0] == "rho"]) >= min(m["iterations"], 1)


def test_the_loops_take_every_branch():
    runs = {name: pg.reference_solve(name, 15) for name in pg.LOOP_CASES}
    assert {r["termination"] for r in runs.values()} >= {0, 1, 2, 3}                     # the cap and the three tolerances
    assert any(0 in r["accepted"][1:r["iterations"]] for r in runs.values())             # a rejected step followed by another iteration: diag2 kept
    assert all(r["status"] in (pg.OK, pg.NO_CONVERGENCE) for r in runs.values())
