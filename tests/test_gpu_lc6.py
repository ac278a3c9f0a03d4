"""gfbe_lc6_eval / gfbe_lc6_solve on the device against the longdouble model (tests/lc6_np.py), case by case (tests/lc6_cases.py):
n = 1, 3, 4, 5, 9, 65 and 257 poses (one, two, three, 17 and 65 super-blocks, ragged last super-blocks), 0 / 1 / 2 / 3 / 128 loop edges
(one capacitance tile, two, the cap with the grid-stride loops of the panel fill and the gather), loops within a super-block, between
neighbours, far apart and onto the constant pose, span 1 .. 4, two sequences with sequence 0 fixed, every pose fixed, the Huber loss
inactive and on a planted outlier, a first step that is rejected, free poses whose step is exactly zero, error quaternions with w < 0,
max_num_iterations 0 and 1.

Criterion: |X_dev - X_ref| <= K_X u A_X, K = lc6_cases.K from r_cpu (tests/test_lc6_model.py):
  K: r 16, J 32, eval_cost 4, pose 8, cost 4        (r_cpu: r 2.30, J 5.08, eval_cost 0.60, pose 1.46, cost 0.57)
Iteration count, accept / reject sequence, termination and status must be the model's; the cases' smallest decision margin is 6.8e4 u A
(n65_negated_q, function tolerance), asserted on the CPU by tests/test_lc6_model.py together with FP64 = longdouble decisions.

Device's worst ratios (MI355X, every case): r 2.30, J 5.08, eval_cost 0.31, pose 1.53, cost 0.57."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import lc6_cases as lc
import lc6_np as m
import posegraph_np as pg

abi = gf.abi
pytestmark = pytest.mark.gpu
CASES = lc.cases()
SENTINEL = -7.25


@pytest.fixture(scope="module")
def be():
    pg.require_extended_precision()
    return gf.Backend(device=0)


@pytest.fixture(scope="module")
def lg(be):
    return be.loop_graph6()


def _decisions(sm):
    return (sm["iterations"], tuple(int(x) for x in sm["accepted"][1:sm["iterations"] + 1]), sm["termination"], sm["status"], sm["num_successful"])


@pytest.mark.parametrize("name", list(CASES))
def test_factors_match_the_model_entry_by_entry(lg, name):
    e = lc.eval_case(name)
    dev = lg.eval(e["t"], e["q"], e["edge_i"], e["edge_j"], e["kind"], e["meas"], lg.options(**e["opt"]))
    ref = m.eval_edges(e["q"], e["t"], e["edge_i"], e["edge_j"], e["kind"], e["meas"], e["opt"], m.LD)
    rr = lc.eval_ratios(dev, ref)
    print(name, "edges", len(e["edge_i"]), "ratios", rr)
    assert rr["r"] <= lc.K["r"] and rr["J"] <= lc.K["J"] and rr["cost"] <= lc.K["eval_cost"]
    # NULL outputs are allowed: the cost alone
    rc = lg.lib.gfbe_lc6_eval(lg.ctx, None, len(e["t"]), abi._pd(abi._f64(e["t"])), abi._pd(abi._f64(e["q"])), 0, None, None, None, None, None, None, None)
    assert rc == abi.OK


@pytest.mark.parametrize("name", list(CASES))
def test_solve_matches_the_model(lg, name):
    c, ref = CASES[name], lc.reference(name)
    out = lg.solve(*lc.args(c), opt=lg.options(**c["opt"]))
    sm = out["summary"]
    print(name, "device", _decisions(sm), "model", lc.decisions(ref))
    assert _decisions(sm) == lc.decisions(ref)
    assert out["status"] == (abi.OK if ref["status"] != abi.NUMERICAL_FAILURE else abi.NUMERICAL_FAILURE)
    rr = lc.solve_ratios(dict(t=out["t"], q=out["q"], cost_history=sm["cost_history"]), ref)
    print(name, "ratios", rr)
    assert rr["pose"] <= lc.K["pose"] and rr["cost"] <= lc.K["cost"]
    assert float(abs(m.LD(sm["final_cost"]) - ref["final_cost"])) <= lc.K["cost"] * m.U * (ref["A_cost"][-1] + ref["g_l1"][-1] * ref["A_pose"])
    # drift of the last keyframe: a product of two quaternions and a rotated position, from the solved pose, within the pose bound
    # (R(q_drift) t_in carries 3 |t_in|_1 times the quaternion's bound)
    n = len(c["g"]["t"])
    tn = float(np.abs(c["g"]["t"][n - 1]).sum())
    A_d = ref["A_pose"] * (1 + 3 * tn) + 3 * tn + float(np.abs(ref["t"][n - 1]).sum()) + 1
    assert (np.abs(out["drift"].astype(m.LD) - ref["drift"]).astype(float) <= 2 * lc.K["pose"] * m.U * A_d).all()
    fixed = np.asarray(c["g"]["fixed"]).astype(bool)
    assert np.array_equal(out["t"][fixed], c["g"]["t"][fixed]) and np.array_equal(out["q"][fixed], c["g"]["q"][fixed])      # constant poses keep their bits
    if name in ("all_fixed", "n1"):
        assert sm["iterations"] == 0 and sm["termination"] == 3 and np.array_equal(out["t"], c["g"]["t"]) and np.array_equal(out["q"], c["g"]["q"])
    if name == "n65_identity_tail":      # |d| = 0 in Plus: free poses with an exactly zero step keep their bits
        lo, hi = c["g"]["identity_tail"]
        assert sm["num_successful"] >= 1 and np.array_equal(out["q"][lo:hi], c["g"]["q"][lo:hi]) and not out["t"][lo:hi].any()


def test_consecutive_sequence_edges_agree_with_the_pose_graph_kernel(be, lg):
    """Two device implementations of RelativeRTError: kind-0 edges (i, i + 1) through gfbe_lc6_eval and the same poses and measurements
    through gfbe_pg_eval (csrc/gfbe_posegraph.hip: rel_factor), each within its own bound of its own longdouble model, and hence of
    each other within the sum of the two."""
    e = lc.eval_case("n65_shapes")
    keep = (e["kind"] == 0) & (e["edge_j"] == e["edge_i"] + 1)
    ei, meas = e["edge_i"][keep], e["meas"][keep]
    assert len(ei) == 64
    mine = lg.eval(e["t"], e["q"], ei, ei + 1, np.zeros(len(ei), np.uint8), meas)
    ref6 = m.eval_edges(e["q"], e["t"], ei, ei + 1, np.zeros(len(ei), np.int64), meas, m.options(), m.LD)
    r6 = lc.eval_ratios(mine, ref6)
    assert r6["r"] <= lc.K["r"] and r6["J"] <= lc.K["J"]
    g = dict(pose=np.concatenate([e["t"], e["q"]], axis=1), rel_i=ei.astype(np.int32), rel_meas=meas, fix_i=np.zeros(0, np.int32), fix_meas=np.zeros((0, 4)))
    theirs = abi.PoseGraph(be.lib, "gfbe_", be.ctx).eval(g)
    J, E, _ = pg.jacobians(g)
    refp = dict(pg.residuals(g), rel_J=J, J_err=E)
    rp = pg.compare_eval(theirs, refp)
    print("lc6", r6, "pg", rp)
    assert rp.pop("J_zeros") == 0.0 and all(v <= pg.K_FACTOR for k, v in rp.items() if k != "fix_r")
    assert (np.abs(mine["r"] - theirs["rel_r"]) <= m.U * (lc.K["r"] * ref6["A_r"] + pg.K_FACTOR * refp["rel_scale"].astype(float))).all()
    assert (np.abs(mine["J"] - theirs["rel_J"]) <= m.U * (lc.K["J"] * ref6["A_J"] + pg.K_FACTOR * refp["J_scale"].astype(float)) + refp["J_err"].astype(float)).all()


def test_same_bits_alone_and_after_a_larger_graph(lg):
    """The panels, band sets and the capacitance system live in the context's grow-only scratch: a graph solved on a fresh context and
    the same graph solved after the largest one (more poses, more loop edges) on a used context give the same bits; so do two calls in a
    row."""
    small, big = CASES["n65_shapes"], CASES["n257_128_loops"]
    be2 = gf.Backend(device=0)
    alone = be2.loop_graph6().solve(*lc.args(small))
    lg.solve(*lc.args(big), opt=lg.options(**big["opt"]))
    after = lg.solve(*lc.args(small))
    again = lg.solve(*lc.args(small))
    for other in (after, again):
        for k in ("t", "q", "drift"):
            assert np.array_equal(alone[k], other[k]), k
        assert alone["summary"] == other["summary"]
    e = lc.eval_case("n65_shapes")
    a, b = (lg.eval(e["t"], e["q"], e["edge_i"], e["edge_j"], e["kind"], e["meas"]) for _ in range(2))
    assert np.array_equal(a["r"], b["r"]) and np.array_equal(a["J"], b["J"]) and a["cost"] == b["cost"]


def test_every_refusal_on_a_device_writes_nothing(be, lg):
    g = gf.synth.loop_graph6(n=100, n_loop=4, seed=3)
    base = dict(zip(lc.ARG_KEYS, (g[k] for k in lc.ARG_KEYS)))

    def bad(opt=None, **kw):
        a = dict(base)
        a.update(kw)
        rc, out = lg.solve_rc(*[a[k] for k in lc.ARG_KEYS], opt=opt, fill=SENTINEL)
        assert rc == abi.BAD_INPUT, kw
        assert (out["t"] == SENTINEL).all() and (out["q"] == SENTINEL).all() and (out["drift"] == SENTINEL).all() and out["summary"]["iterations"] == 0, kw
    many = gf.synth.loop_graph6(n=300, n_loop=129, seed=3)
    bad(**{k: many[k] for k in lc.ARG_KEYS})                                                          # n_loop > GFBE_LC6_MAX_LOOPS
    assert "GFBE_LC6_MAX_LOOPS" in be._err()
    li, lcc = g["loop_i"].copy(), g["loop_c"].copy()
    bad(loop_i=np.array([100, *li[1:]], np.int32))                                                   # an index out of range
    bad(loop_c=np.array([-1, *lcc[1:]], np.int32))
    bad(loop_c=np.array([li[0], *lcc[1:]], np.int32))                                                # loop_c >= loop_i
    bad(loop_i=np.array([li[1], *li[1:]], np.int32), loop_c=np.array([0, *lcc[1:]], np.int32))       # two loops on one loop_i
    for key, at in (("t", (7, 1)), ("q", (50, 2)), ("loop_meas", (3, 6))):                           # a non-finite pose or measurement
        arr = np.array(g[key], np.float64).copy()
        arr[at] = np.nan
        bad(**{key: arr})
    bad(opt=lg.options(struct_size=C.sizeof(abi.Lc6Options) - 8))                                # an options struct of another size
    # and the context still solves
    out = lg.solve(*[base[k] for k in lc.ARG_KEYS])
    assert out["summary"]["num_successful"] >= 1 and np.isfinite(out["t"]).all()
