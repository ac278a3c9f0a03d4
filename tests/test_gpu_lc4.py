"""gfbe_lc4_eval / gfbe_lc4_solve on the device against the longdouble model (tests/lc4_np.py), case by case (tests/lc4_cases.py):
n = 2, 5, 63, 64, 65, 257 and 1001 poses (super-block counts on both sides of a power of two, a ragged last super-block), 0 / 1 / 64
loop edges, a loop into the constant first pose, a loop within one super-block, two sequences with sequence 0 fixed, every pose fixed,
yaw crossing +-180, max_num_iterations 0 and 1, and loop measurements far off the start (rejected steps); a graph of non-finite values
gives the five invalid steps.

Criterion: |X_dev - X_ref| <= K_X u A_X, K = lc4_cases.K from r_cpu (tests/test_lc4_model.py):
  K: r 8, J 8, eval_cost 1, pose 2, cost 1        (r_cpu: r 1.43, J 1.42, eval_cost 0.17, pose 0.28, cost 0.13)
Iteration count, accept / reject sequence, termination and status must be the model's; the cases' smallest decision margin is 1.0e5 u A
(n65_64_loops, function tolerance), asserted on the CPU by tests/test_lc4_model.py together with FP64 = longdouble decisions.

Device's worst ratios (MI355X, every case): r 1.43, J 1.42, eval_cost 0.086, pose 0.28, cost 0.13."""
import numpy as np
import pytest

from _gfbe_import import gf
import lc4_cases as lc
import lc4_np as m

abi = gf.abi
pytestmark = pytest.mark.gpu
CASES = lc.cases()


@pytest.fixture(scope="module")
def lg():
    be = gf.Backend(device=0)
    g = abi.LoopGraph(be.lib, "gfbe_", be.ctx)
    g._be = be      # (keeps the context alive)
    return g


def _decisions(sm):
    return (sm["iterations"], tuple(int(x) for x in sm["accepted"][1:sm["iterations"] + 1]), sm["termination"], sm["status"], sm["num_successful"])


@pytest.mark.parametrize("name", list(CASES))
def test_factors_match_the_model_entry_by_entry(lg, name):
    e = lc.eval_case(name)
    dev = lg.eval(e["t"], e["ypr"], e["edge_i"], e["edge_j"], e["kind"], e["meas"], lg.options(**e["opt"]))
    ref = m.eval_edges(e["ypr"][:, 0], e["t"], e["edge_i"], e["edge_j"], e["kind"], e["meas"], e["opt"], m.LD)
    rr = lc.eval_ratios(dev, ref)
    print(name, "edges", len(e["edge_i"]), "ratios", rr)
    assert rr["r"] <= lc.K["r"] and rr["J"] <= lc.K["J"] and rr["cost"] <= lc.K["eval_cost"]
    # NULL outputs are allowed: the cost alone
    rc = getattr(lg.lib, "gfbe_lc4_eval")(lg.ctx, None, len(e["t"]), abi._pd(abi._f64(e["t"])), abi._pd(abi._f64(e["ypr"])), 0, None, None, None, None, None, None, None)
    assert rc == abi.OK


@pytest.mark.parametrize("name", list(CASES))
def test_solve_matches_the_model(lg, name):
    c, ref = CASES[name], lc.reference(name)
    out = lg.solve(*c["args"], opt=lg.options(**c["opt"]))
    sm = out["summary"]
    print(name, "device", _decisions(sm), "model", lc.decisions(ref))
    assert _decisions(sm) == lc.decisions(ref)
    assert out["status"] == (abi.OK if ref["status"] != abi.NUMERICAL_FAILURE else abi.NUMERICAL_FAILURE)
    rr = lc.solve_ratios(dict(t=out["t"], yaw=out["yaw"], cost_history=sm["cost_history"]), ref)
    print(name, "ratios", rr)
    assert rr["pose"] <= lc.K["pose"] and rr["cost"] <= lc.K["cost"]
    assert float(abs(m.LD(sm["final_cost"]) - ref["final_cost"])) <= lc.K["cost"] * m.U * (ref["A_cost"][-1] + ref["g_l1"][-1] * ref["A_pose"])
    # drift of the last keyframe: yaw_drift and t_drift from the solved pose, within the pose bound (the rotation of the VIO position by
    # yaw_drift carries |t| times the yaw's bound in radians)
    n = len(c["g"]["t"])
    A_d = ref["A_pose"] * (1 + np.abs(c["g"]["t"][n - 1]).sum() * np.pi / 180) + np.abs(c["g"]["t"][n - 1]).sum() + np.abs(ref["t"][n - 1].astype(float)).sum()
    assert (np.abs(out["drift"].astype(m.LD) - ref["drift"]).astype(float) <= 2 * lc.K["pose"] * m.U * A_d).all()
    fixed = np.asarray(c["g"]["fixed"]).astype(bool)
    assert np.array_equal(out["t"][fixed], c["g"]["t"][fixed]) and np.array_equal(out["yaw"][fixed], c["g"]["ypr"][fixed, 0])      # constant poses keep their bits
    if name == "all_fixed":
        assert sm["iterations"] == 0 and sm["termination"] == 3 and np.array_equal(out["t"], c["g"]["t"])


def test_converges_towards_the_truth(lg):
    c = CASES["n1001_convergence"]
    g = c["g"]
    out = lg.solve(*c["args"], opt=lg.options(**c["opt"]))
    h, acc = out["summary"]["cost_history"], out["summary"]["accepted"]
    assert out["summary"]["num_successful"] >= 3
    for k in range(1, out["summary"]["iterations"] + 1):
        assert (h[k] < h[k - 1]) if acc[k] else (h[k] == h[k - 1])
    before = np.sqrt(((g["t"] - g["true_t"]) ** 2).sum(axis=1).mean())
    after = np.sqrt(((out["t"] - g["true_t"]) ** 2).sum(axis=1).mean())
    assert after < before


def test_same_bits_alone_and_after_a_larger_graph(lg):
    """The panels, band sets and the capacitance system live in the context's grow-only scratch: a graph solved on a fresh context and
    the same graph solved after a larger one (more poses, more loop edges) on a used context give the same bits."""
    small, big = CASES["n63_one_loop"], CASES["n257_64_loops"]
    be2 = gf.Backend(device=0)
    alone = abi.LoopGraph(be2.lib, "gfbe_", be2.ctx).solve(*small["args"])
    lg.solve(*big["args"])
    after = lg.solve(*small["args"])
    again = lg.solve(*small["args"])
    for other in (after, again):
        for k in ("t", "yaw", "drift"):
            assert np.array_equal(alone[k], other[k]), k
        assert alone["summary"] == other["summary"]


def test_non_finite_graph_ends_as_numerical_failure(lg):
    u = lc.unusable_case()
    ref = m.solve(*u["args"], opt=u["opt"])
    rc, out = lg.solve_rc(*u["args"])
    sm = out["summary"]
    assert rc == abi.NUMERICAL_FAILURE
    assert (sm["iterations"], sm["termination"], sm["status"], sm["num_successful"]) == (ref["iterations"], ref["termination"], ref["status"], 0) == (5, 4, 2, 0)


def test_bad_input_on_a_device_writes_nothing(lg):
    g = gf.synth.loop_graph(n=100, n_loop=65, seed=3)
    rc, out = lg.solve_rc(*[g[k] for k in lc.ARG_KEYS])
    assert rc == abi.BAD_INPUT and np.isnan(out["t"]).all() and np.isnan(out["yaw"]).all() and np.isnan(out["drift"]).all()
