"""csrc/gfbe_posegraph.hip against the extended-precision model of tests/posegraph_np.py, through the C ABI, at every size at which the
file takes another path. tests/test_gpu_posegraph.py compares the device with the oracle, which was written from the same formulas;
here the reference shares nothing with either (difference quotients for the Jacobians, a longdouble LDL^T for the step), and every
bound was fixed on the CPU (tests/test_posegraph_model.py) before a device ran.

Paths no test reached before, and the test that reaches them now:
  two-stage reduction of gfbe_pg_solve (k_pg_reduce1 + the `partial` branch of k_pg_decide, n > 65536)   test_two_stage_reduction_beyond_65536_poses
  multi-segment host_sum of gfbe_pg_eval (n > 4096)                                                       test_cost_across_reduction_segments
  rel_of[i] = -1 inside a chain, the zeroed Ho, rel_i out of order         test_factor_blocks (gaps, mixed), test_first_step / test_whole_loop (split),
                                                                           test_out_of_order_and_duplicate_inputs
  fix_order and the CSR of fixes, two fixes on one pose                    test_factor_blocks (mixed), every solve case (fixes shuffled)
  n = 1 (no reduction sweep), n = 2, 3                                     test_factor_blocks (single, empty), test_first_step, test_whole_loop (n1, n2, n3, empty)
  the 32-pose workgroup edge of k_pg_lin_st, k_pg_system, k_pg_pcr         n32, n33, n64, n65 (and 257, 1025: one past a power of two)
  k_pg_lin_st's own blocks                                                 test_first_step: the step of the system they form, against the model's

Bounds (posegraph_np): a factor block within K_FACTOR u scale (K_FACTOR = %(K)g, 8 x the worst FP64 ratio measured on the CPU), a cost
within K_FACTOR u cost_scale, the first step within 16 x STEP_FLOOR[case], the whole loop within 16 x LOOP_FLOOR[case]; accept
sequence, iteration count, termination and status equal to the model's.

Measured on an MI355X (printed with -s), next to the CPU figures of the oracle in posegraph_np's docstring:
%(DEVICE)s
"""
import ctypes as C

import numpy as np
import pytest

import posegraph_np as pg
from _gfbe_import import gf

abi = gf.abi
LD = pg.LD
pytestmark = pytest.mark.gpu

DEVICE = """\
    factor blocks, worst ratio to u scale over the factor cases (bound K_FACTOR; the oracle's CPU figure in brackets):
        rel_r_t 1.01 (1.01)   rel_r_q 1.65 (1.65)   J_t_dqi 1.99 (1.99)   J_t_t 1.22 (1.22)   J_q_dq 3.06 (3.06)   fix_r 1.2 (1.2)   cost 0.48 (1.05)
        structural zeros exact; the blocks are the oracle's to the digit shown: the same formulas in the same order, now known to be right
    cost across segments:  cost4097 0.0036   cost8200 0.0006   (u cost_scale)
    first step, |device - model| / STEP_FLOOR (bound 16):
        n1 0.77   n2 0.54   n3 0.76   n32 1.03   n33 0.72   n64 1.41   n65 0.87   n257 1.97   n1025 0.70   one_fix 1.26   split 0.60   huber 0.44
    whole loop, (|pose|, |cost history|) / LOOP_FLOOR (bound 16):
        n1 (0.79, 0.80)   n2 (0.58, 0.49)   n3 (3.02, 0.45)   n32 (1.65, 1.56)   n33 (0.55, 0.33)   n64 (0.58, 0.46)   n65 (0.92, 0.26)
        n257 (0.90, 1.19)   one_fix (0.31, 1.37)   split (1.15, 0.91)   huber (0.26, 0.15)
    n = 65537 and 65536, 5 iterations against the oracle:  |t| 1.1e-13 m   |q| 7.6e-14;  initial cost 0.0014 / 0.0003 u cost_scale of the model's
    The device's cyclic reduction is at the rounding floor of its method (pcr_fp64) and of the oracle's block Cholesky on every case, the
    one-fix and the three-component graph included; no defect was found in csrc/gfbe_posegraph.hip."""
__doc__ = __doc__ % dict(K=pg.K_FACTOR, DEVICE=DEVICE)


@pytest.fixture(scope="module")
def dev():
    pg.require_extended_precision()
    be = gf.Backend(device=0)
    yield abi.PoseGraph(be.lib, "gfbe_", be.ctx)


@pytest.fixture(scope="module")
def orc(oracle):
    return abi.PoseGraph(oracle.lib, "gfo_", None)


def _pose_diff(a, b):
    return float(np.max(np.abs(np.asarray(a, LD) - b)))


def _sequence(s):
    return s["iterations"], list(s["accepted"]), s["termination"], s["status"]


@pytest.mark.parametrize("name", pg.FACTOR_CASES)
def test_factor_blocks_against_the_model(dev, name):
    """gfbe_pg_eval (k_pg_lin): every block within K_FACTOR u scale of the model, in the caller's order (the model's arrays are in the
    caller's order; mixed passes rel_i shuffled and the fixes unsorted with two on one pose), structural zeros of rel_J exact."""
    g, ref = pg.case(name), pg.reference_eval(name)
    got = dev.eval(g)
    ratios = pg.compare_eval(got, ref)
    print("%-8s " % name + "   ".join("%s %.3g" % kv for kv in ratios.items()))
    assert ratios.pop("J_zeros") == 0.0
    for fam, r in ratios.items():
        assert r <= pg.K_FACTOR, (name, fam, r)


@pytest.mark.parametrize("name", pg.COST_CASES)
def test_cost_across_reduction_segments(dev, name):
    g = pg.case(name)
    ref = pg.residuals(g)
    r = pg._ratio(dev.eval(g)["cost"], ref["cost"], ref["cost_scale"])
    print("%-8s cost %.3g u cost_scale" % (name, r))
    assert len(g["pose"]) > 4096 * (2 if name == "cost8200" else 1)
    assert r <= pg.K_FACTOR


@pytest.mark.parametrize("name", pg.SOLVE_CASES + ("empty",))
def test_first_step_against_the_model(dev, name):
    """gfbe_pg_solve(max_iterations = 1): k_pg_lin_st's blocks, k_pg_system, the reduction sweeps and k_pg_candidate in one figure."""
    g, m = pg.case(name), pg.reference_solve(name, 1)
    got = dev.solve(g, max_iterations=1)
    s = got["summary"]
    if name == "empty":
        assert _sequence(s) == (0, [0], 3, pg.OK) == _sequence(m)
        assert np.array_equal(got["pose"], g["pose"]) and s["cost_history"] == [0.0]
        return
    d = _pose_diff(got["pose"], m["pose"])
    print("%-8s first step: |device - model| %.3g = %.2f x the CPU floor (bound 16)" % (name, d, d / pg.STEP_FLOOR[name]))
    assert _sequence(s) == _sequence(m)
    assert d <= pg.STEP_MARGIN * pg.STEP_FLOOR[name]
    pg.check_first_costs(g, got["pose"], s["cost_history"], "device %s:" % name)


@pytest.mark.parametrize("name", pg.LOOP_CASES)
def test_whole_loop_against_the_model(dev, name):
    g, m = pg.case(name), pg.reference_solve(name, 15)
    got = dev.solve(g, max_iterations=15)
    s = got["summary"]
    assert _sequence(s) == _sequence(m)
    d_pose = _pose_diff(got["pose"], m["pose"])
    d_cost = float(max(abs(LD(a) - b) for a, b in zip(s["cost_history"], m["cost_history"])) / m["cost_history"][0])
    print("%-8s %2d iterations, termination %d: |pose| %.3g = %.2f x   |cost history| / initial cost %.3g = %.2f x the CPU floor (bound 16)"
          % (name, m["iterations"], m["termination"], d_pose, d_pose / pg.LOOP_FLOOR[name][0], d_cost, d_cost / pg.LOOP_FLOOR[name][1]))
    assert d_pose <= pg.STEP_MARGIN * pg.LOOP_FLOOR[name][0]
    assert d_cost <= pg.STEP_MARGIN * pg.LOOP_FLOOR[name][1]
    assert abs(LD(s["final_cost"]) - m["final_cost"]) <= pg.STEP_MARGIN * pg.LOOP_FLOOR[name][1] * m["cost_history"][0]


def _cut(g, n):
    keep_r, keep_f = g["rel_i"] + 1 < n, g["fix_i"] < n
    return dict(n=n, pose=g["pose"][:n].copy(), rel_i=g["rel_i"][keep_r], rel_meas=g["rel_meas"][keep_r], fix_i=g["fix_i"][keep_f], fix_meas=g["fix_meas"][keep_f])


def test_two_stage_reduction_beyond_65536_poses(dev, orc):
    """n = 65537: k_pg_reduce1 and the `partial` branch of k_pg_decide; the same graph cut to 65536 poses takes the direct branch. Initial
    cost against the model (vectorised over the poses); summary and poses against the oracle at test_solve_matches_oracle's tolerances."""
    big = pg.case("n65537")
    for g in (big, _cut(big, 65536)):
        n = len(g["pose"])
        got, ref = dev.solve(g, max_iterations=5), orc.solve(g, max_iterations=5)
        sg, sr = got["summary"], ref["summary"]
        res = pg.residuals(g)
        r = pg._ratio(sg["cost_history"][0], res["cost"], res["cost_scale"])
        print("n = %d: initial cost %.3g u cost_scale   %d iterations %s   |t| %.3g   |q| %.3g" % (n, r, sg["iterations"], sg["accepted"],
              np.abs(got["pose"][:, :3] - ref["pose"][:, :3]).max(), np.abs(got["pose"][:, 3:] - ref["pose"][:, 3:]).max()))
        assert r <= pg.K_FACTOR
        assert _sequence(sg) == _sequence(sr) and sg["iterations"] >= 1 and 1 in sg["accepted"]
        np.testing.assert_allclose(sg["cost_history"], sr["cost_history"], rtol=1e-9)
        assert np.abs(got["pose"][:, :3] - ref["pose"][:, :3]).max() < 1e-8
        assert np.abs(got["pose"][:, 3:] - ref["pose"][:, 3:]).max() < 1e-9


def test_out_of_order_and_duplicate_inputs(dev):
    g = pg.case("n65")
    rng = np.random.default_rng(5)
    order = np.argsort(g["fix_i"], kind="stable")
    a = dict(g, fix_i=g["fix_i"][order], fix_meas=g["fix_meas"][order])
    pr, pf = rng.permutation(len(g["rel_i"])), rng.permutation(len(g["fix_i"]))
    b = dict(g, rel_i=g["rel_i"][pr], rel_meas=g["rel_meas"][pr], fix_i=g["fix_i"][pf], fix_meas=g["fix_meas"][pf])
    assert a["rel_i"].tolist() == sorted(a["rel_i"].tolist()) and a["fix_i"].tolist() == sorted(a["fix_i"].tolist())
    assert b["rel_i"].tolist() != a["rel_i"].tolist() and b["fix_i"].tolist() != a["fix_i"].tolist()
    ra, rb = dev.solve(a, max_iterations=5), dev.solve(b, max_iterations=5)
    assert np.array_equal(ra["pose"], rb["pose"]) and ra["summary"] == rb["summary"] and ra["summary"]["iterations"] >= 1
    ea, eb = dev.eval(a), dev.eval(b)
    fix_r = np.empty_like(ea["fix_r"])
    fix_r[order] = ea["fix_r"]                      # (back into g's order, of which b's is the permutation pf)
    assert np.array_equal(ea["rel_r"][pr], eb["rel_r"]) and np.array_equal(ea["rel_J"][pr], eb["rel_J"]) and np.array_equal(fix_r[pf], eb["fix_r"])
    # a relative factor given twice: GFBE_BAD_INPUT, and pose_out is not written
    pose = abi._f64(g["pose"])
    ri, rm = abi._i32(np.append(g["rel_i"], g["rel_i"][7])), abi._f64(np.vstack([g["rel_meas"], g["rel_meas"][7]]))
    fi, fm = abi._i32(g["fix_i"]), abi._f64(g["fix_meas"])
    out, sm = np.full_like(pose, 7.25), abi.Summary()
    rc = dev.lib.gfbe_pg_solve(dev.ctx, len(pose), abi._pd(pose), len(ri), abi._pi(ri), abi._pd(rm), 0.1, 0.01, len(fi), abi._pi(fi), abi._pd(fm), 1.0, 5,
                               abi._pd(out), C.byref(sm))
    assert rc == abi.BAD_INPUT and (out == 7.25).all()
