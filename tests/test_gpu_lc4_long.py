"""gfbe_lc4_solve_long on the device against the longdouble model (tests/lc4_np.py), case by case (tests/lc4_long_cases.py): 65, 66, 70,
80, 129 and 512 loop edges — 17, 20, 33 (ragged, identity padding) and 128 tile columns of capacitance, two sequences with a dropped
loop edge, headings across +-180; the 512-loop case against its recorded reference (tests/golden/lc4_long_cap.npz). Up to 64 loop
edges the call has to return the bits of gfbe_lc4_solve.

Criterion: that of tests/test_gpu_lc4.py, |X_dev - X_ref| <= K_X u A_X with K = lc4_cases.K (pose 2, cost 1); iteration count,
accept / reject sequence, termination and status must be the model's. tests/test_lc4_long_host.py asserts on the CPU that the cases'
r_cpu stays below a quarter of K and that no decision is nearer to its threshold than 1e3 u A.

Device's worst ratios (MI355X, every case): pose 4.4e-4 (n260_129_loops), cost 0.020 (n132_65_loops); n700_512_loops pose 1.1e-4,
cost 1.7e-3."""
import numpy as np
import pytest

from _gfbe_import import gf
import lc4_cases as lc
import lc4_long_cases as ll
import lc4_np as m

abi = gf.abi
pytestmark = pytest.mark.gpu
CASES = ll.all_cases()
SHORT = lc.cases()


@pytest.fixture(scope="module")
def lg():
    be = gf.Backend(device=0)
    g = abi.LoopGraph(be.lib, "gfbe_", be.ctx)
    g._be = be      # (keeps the context alive)
    return g


def _decisions(sm):
    return (sm["iterations"], tuple(int(x) for x in sm["accepted"][1:sm["iterations"] + 1]), sm["termination"], sm["status"], sm["num_successful"])


@pytest.mark.parametrize("name", list(CASES))
def test_solve_long_matches_the_model(lg, name):
    c, ref = CASES[name], ll.reference(name)
    out = lg.solve_long(*c["args"], opt=lg.options(**c["opt"]))
    sm = out["summary"]
    print(name, "device", _decisions(sm), "model", lc.decisions(ref))
    assert _decisions(sm) == lc.decisions(ref)
    assert out["status"] == (abi.OK if ref["status"] != abi.NUMERICAL_FAILURE else abi.NUMERICAL_FAILURE)
    rr = lc.solve_ratios(dict(t=out["t"], yaw=out["yaw"], cost_history=sm["cost_history"]), ref)
    print(name, "ratios", rr)
    assert rr["pose"] <= lc.K["pose"] and rr["cost"] <= lc.K["cost"]
    assert float(abs(m.LD(sm["final_cost"]) - ref["final_cost"])) <= lc.K["cost"] * m.U * (ref["A_cost"][-1] + ref["g_l1"][-1] * ref["A_pose"])
    # drift of the last keyframe, within the pose bound (the bound of tests/test_gpu_lc4.py)
    n = len(c["g"]["t"])
    A_d = ref["A_pose"] * (1 + np.abs(c["g"]["t"][n - 1]).sum() * np.pi / 180) + np.abs(c["g"]["t"][n - 1]).sum() + np.abs(ref["t"][n - 1].astype(float)).sum()
    assert (np.abs(out["drift"].astype(m.LD) - ref["drift"]).astype(float) <= 2 * lc.K["pose"] * m.U * A_d).all()
    fixed = np.asarray(c["g"]["fixed"]).astype(bool)
    assert np.array_equal(out["t"][fixed], c["g"]["t"][fixed]) and np.array_equal(out["yaw"][fixed], c["g"]["ypr"][fixed, 0])      # constant poses keep their bits


@pytest.mark.parametrize("name", list(SHORT))
def test_up_to_64_loops_the_bits_of_solve(lg, name):
    c = SHORT[name]
    a = lg.solve(*c["args"], opt=lg.options(**c["opt"]))
    b = lg.solve_long(*c["args"], opt=lg.options(**c["opt"]))
    for k in ("t", "yaw", "drift"):
        assert np.array_equal(a[k], b[k]), k
    assert a["summary"] == b["summary"] and a["status"] == b["status"]


def test_same_bits_alone_and_after_the_largest_graph(lg):
    """S, L, the pivot inverses and v live in the context's grow-only scratch: the 65-loop graph solved on a fresh context, after the
    512-loop graph on a used one, and once more give the same bits."""
    small, big = CASES["n132_65_loops"], CASES[ll.CAP]
    be2 = gf.Backend(device=0)
    alone = abi.LoopGraph(be2.lib, "gfbe_", be2.ctx).solve_long(*small["args"])
    lg.solve_long(*big["args"], opt=lg.options(**big["opt"]))
    after = lg.solve_long(*small["args"])
    again = lg.solve_long(*small["args"])
    for other in (after, again):
        for k in ("t", "yaw", "drift"):
            assert np.array_equal(alone[k], other[k]), k
        assert alone["summary"] == other["summary"]


def test_non_finite_graph_ends_as_numerical_failure(lg):
    u = ll.unusable_case()
    ref = m.solve(*u["args"], opt=u["opt"])
    rc, out = lg.solve_long_rc(*u["args"])
    sm = out["summary"]
    assert rc == abi.NUMERICAL_FAILURE
    assert (sm["iterations"], sm["termination"], sm["status"], sm["num_successful"]) == (ref["iterations"], ref["termination"], ref["status"], 0) == (5, 4, 2, 0)


def test_bad_input_on_a_device_writes_nothing(lg):
    g = gf.synth.loop_graph(n=1100, n_loop=513, seed=3)
    assert len(g["loop_i"]) == 513
    rc, out = lg.solve_long_rc(*[g[k] for k in lc.ARG_KEYS])
    assert rc == abi.BAD_INPUT and np.isnan(out["t"]).all() and np.isnan(out["yaw"]).all() and np.isnan(out["drift"]).all()
