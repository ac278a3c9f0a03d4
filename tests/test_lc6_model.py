"""The model of the 6-DoF loop-closure pose graph (tests/lc6_np.py) against itself, without a GPU: analytic Jacobians against
Romberg-extrapolated central differences through Plus in longdouble (the scheme of posegraph_np.jacobians, on a residual written
another way: the quaternion sandwich instead of the rotation matrix), the band + Woodbury path against the dense path, the FP64 model
against the longdouble model (r_cpu, from which the bounds K of tests/lc6_cases.py follow), the decision margins of every case, and
that the cases reach the paths they are named for.

Measured here (FP64 against longdouble, every case of lc6_cases.cases(), units u A_X):
  r_cpu: r 2.30, J 5.08, eval_cost 0.60, pose 1.46, cost 0.57  ->  K: r 16, J 32, eval_cost 4, pose 8, cost 4.
Smallest decision margin of any case, in units of u x the absolute sum behind the quantity compared: 6.8e4 (n65_negated_q, the
function-tolerance test of its last iteration); the bound asks for 1e3, above every K."""
import numpy as np
import pytest

import lc6_cases as lc
import lc6_np as m
import posegraph_np as pg

CASES = lc.cases()


@pytest.fixture(scope="module")
def both():
    pg.require_extended_precision()
    return {name: (lc.reference(name, "f64"), lc.reference(name, "ld")) for name in CASES}


def _q(axis_angle):
    v = np.asarray(axis_angle, m.LD)
    return m.plus(np.array([[1.0, 0, 0, 0]], m.LD), np.zeros((1, 3), m.LD), np.concatenate([v, np.zeros(3, m.LD)])[None], m.LD)[0][0]


# (kind, rotation vector / 2 of q_i, of q_j, of the measurement, translation offset of the measurement): small and large rotations, a
# relative rotation beyond 90 degrees, an error quaternion with w < 0 (the measurement negated), kind 1 below and above the threshold
JAC_CASES = [
    (0, (0.1, -0.2, 0.3), (0.2, 0.1, -0.1), (0.05, 0.1, -0.2), 0.3, 1),
    (0, (0.7, 0.2, -0.4), (-0.5, 0.9, 0.3), (0.3, -0.2, 0.6), 0.3, 1),
    (0, (0.0, 0.0, 0.2), (0.0, 0.0, 1.3), (0.0, 0.0, 0.1), 0.3, 1),
    (0, (0.1, -0.2, 0.3), (0.2, 0.1, -0.1), (0.05, 0.1, -0.2), 0.3, -1),
    (1, (0.1, -0.2, 0.3), (0.2, 0.1, -0.1), None, 0.0005, 1),
    (1, (0.1, -0.2, 0.3), (0.2, 0.1, -0.1), (0.05, 0.1, -0.2), 0.3, 1),
    (1, (0.7, 0.2, -0.4), (-0.5, 0.9, 0.3), (0.3, -0.2, 0.6), 0.3, 1),
]
W_NEGATIVE = [False, True, False, True, False, False, True]      # the error quaternion's w < 0: by a rotation error beyond 180 degrees, or by the measurement's sign


@pytest.mark.parametrize("case,w_negative", list(zip(JAC_CASES, W_NEGATIVE)))
def test_analytic_jacobians_agree_with_romberg_differences_through_plus(case, w_negative):
    kind, vi, vj, vm, toff, sign = case
    pg.require_extended_precision()
    dt = m.LD
    opt = m.options()
    qi, qj = _q(vi), _q(vj)
    ti, tj = np.array([1.0, 2.0, 3.0], dt), np.array([1.5, 1.0, 3.2], dt)
    small = vm is None      # the kind-1 case below the Huber threshold: a measurement near the truth
    qm = m.qmul(m.qconj(qi), qj) if small else _q(vm)
    if small:
        qm = m.qmul(qm, _q((2e-6, -1e-6, 1e-6)))
    R = m.quat_to_R(qi[None], dt)[0][0].reshape(3, 3)
    meas = np.concatenate([R.T @ (tj - ti) + dt(toff), sign * qm])[None]
    ev = m.eval_edges(np.stack([qi, qj]), np.stack([ti, tj]), [0], [1], [kind], meas, opt, dt)
    r0, J = ev["r"][0], ev["J"][0]
    raw_r, raw_J = m.factor(qi[None], ti[None], qj[None], tj[None], meas, opt["t_var"], opt["q_var"], dt)[:2]
    assert (raw_r[0] @ raw_r[0] > 0.01) == (not small)
    e = m.qmul(m.qconj(meas[0, 3:]), m.qmul(m.qconj(qi), qj))
    assert (e[0] < 0) == w_negative
    # the residual the difference quotients are taken of: posegraph_np's statement of RelativeRTError (the rotation as q v q*)
    pi, pj = np.concatenate([ti, qi])[None], np.concatenate([tj, qj])[None]
    assert np.abs(pg.rel_residual(pi, pj, meas, dt(opt["t_var"]), dt(opt["q_var"]))[0] - raw_r[0]).max() < 1e-17 * (1 + np.abs(raw_r[0]).max())
    for col in range(12):
        def f(h, col=col):
            d6 = np.zeros((1, 6), dt)
            d6[0, col % 6] = h
            a, b = (pg.plus(pi, d6), pj) if col < 6 else (pi, pg.plus(pj, d6))
            return pg.rel_residual(a, b, meas, dt(opt["t_var"]), dt(opt["q_var"]))[0]
        num, err = pg._romberg(f)
        scale = max(float(np.abs(raw_J[0]).max()), 1.0)
        assert float(err.max()) <= pg.JAC_ERR * scale
        if kind == 1 and not small:
            # the corrector's Jacobian is Ceres' Gauss-Newton form s1 (J - alpha r r^T J / |r|^2), alpha = 0 for Huber: sqrt(rho') J
            s1 = np.sqrt(dt(opt["huber_delta"]) / np.sqrt(raw_r[0] @ raw_r[0]))
            assert np.abs(J[:, col] - s1 * raw_J[0][:, col]).max() <= 4 * m.U * scale
            assert np.abs(r0 - s1 * raw_r[0]).max() <= 4 * m.U * np.abs(raw_r[0]).max()
        else:
            assert np.array_equal(J[:, col], raw_J[0][:, col])
        assert float(np.abs(num - raw_J[0][:, col]).max()) <= 4 * pg.JAC_ERR * scale, (col, num, raw_J[0][:, col])


def test_plus_with_a_zero_step_is_the_identity_and_small_steps_are_continuous():
    q = _q((0.3, -0.1, 0.2)).astype(np.float64)[None]
    t = np.zeros((1, 3))
    out, _ = m.plus(q, t, np.zeros((1, 6)), np.float64)
    assert np.array_equal(out, q)
    out, _ = m.plus(q, t, np.array([[1e-200, 0, 0, 0, 0, 0]]), np.float64)
    assert np.abs(out - q).max() < 1e-16


@pytest.mark.parametrize("name", ["n3_loop_into_constant", "n4_two_loops", "n5_three_loops", "n9_span1", "n9_span3", "n9_huber_inactive", "n65_shapes", "n65_outlier",
                                  "n65_identity_tail", "far_start"])
def test_band_and_woodbury_path_equals_the_dense_path(both, name):
    c = CASES[name]
    band = both[name][0]
    dense = m.solve(*lc.args(c), opt=c["opt"], dt=np.float64, path="dense")
    assert lc.decisions(band) == lc.decisions(dense)
    A = max(band["A_pose"], 1e-300)
    err = max(np.abs(band["t"] - dense["t"]).max(), np.abs(band["q"] - dense["q"]).max())
    print(name, "band against dense, units u A_pose:", err / (m.U * A))
    assert err <= lc.K["pose"] * m.U * A
    for a, b, Ac in zip(band["cost_history"], dense["cost_history"], band["A_cost"]):
        assert abs(a - b) <= lc.K["cost"] * m.U * (Ac + band["g_l1"][0] * A)


def test_band_path_solves_one_step_as_the_dense_path_in_longdouble():
    pg.require_extended_precision()
    for name in ("n5_three_loops", "n65_shapes"):
        c = CASES[name]
        G = m.build_graph(*lc.args(c), c["opt"])
        lin = m.linearize(G, np.asarray(c["g"]["q"], m.LD), np.asarray(c["g"]["t"], m.LD), c["opt"], m.LD)
        act = lin["active"]
        scale = np.where(act, 1 / (1 + np.sqrt(np.where(act, lin["diag0"], 0))), m.LD(1))
        diag2 = np.minimum(np.maximum(lin["diag0"] * scale * scale, m.LD(1e-6)), m.LD(1e32))
        for radius in (1e4, 1e8):
            yb, mb = m.lm_step(lin, scale, diag2, m.LD(radius), m.LD, "band")
            yd, md = m.lm_step(lin, scale, diag2, m.LD(radius), m.LD, "dense")
            rel = float(np.abs(yb - yd).max() / np.abs(yd).max())
            print(name, "radius", radius, "relative difference", rel)
            assert rel < 1e-14 and abs(float(mb - md)) < 1e-14 * abs(float(md))
            assert not yb[~act].any()      # rows out of the problem (constant poses, padding rows, padding poses) do not move


def test_decisions_agree_between_precisions_with_margin(both):
    worst = np.inf
    assert lc.MARGIN >= max(lc.K.values())
    for name, (a, b) in both.items():
        assert lc.decisions(a) == lc.decisions(b), name
        mr = min(lc.margin_ratio(a), lc.margin_ratio(b))
        print(name, lc.decisions(b), "smallest margin / (u A): %.3g" % mr)
        assert mr >= lc.MARGIN, name
        worst = min(worst, mr)
    print("smallest margin of any case: %.3g" % worst)


def test_cases_cover_the_paths(both):
    ref = {name: b for name, (_, b) in both.items()}
    assert sorted({len(c["g"]["t"]) for c in CASES.values()} & {1, 3, 4, 5, 9, 65, 257}) == [1, 3, 4, 5, 9, 65, 257]
    assert {len(c["g"]["loop_i"]) for c in CASES.values()} >= {0, 1, 2, 3, 128} and m.MAX_LOOPS == 128
    assert {c["opt"]["span"] for c in CASES.values()} == {1, 2, 3, 4}
    assert ref["far_start"]["accepted"][0] == 0 and 1 in ref["far_start"]["accepted"]              # a first step that is rejected
    assert ref["all_fixed"]["iterations"] == 0 and ref["all_fixed"]["termination"] == 3 and ref["n1"]["iterations"] == 0
    assert ref["max_it_0"]["iterations"] == 0 and ref["max_it_1"]["iterations"] == 1
    g = CASES["n65_shapes"]["g"]
    assert g["loop_c"][0] == 0 and any(i // 4 == c // 4 for i, c in zip(g["loop_i"], g["loop_c"]))      # onto the constant pose; within one super-block
    g = CASES["n5_three_loops"]["g"]
    assert any(i // 4 == c // 4 + 1 for i, c in zip(g["loop_i"], g["loop_c"]))                     # between neighbouring super-blocks
    g = CASES["n9_span1"]["g"]
    assert any(i // 4 >= c // 4 + 2 for i, c in zip(g["loop_i"], g["loop_c"]))                     # far apart
    g = CASES["n257_two_sequences"]["g"]
    assert set(g["sequence"]) == {0, 1} and g["fixed"][g["sequence"] == 0].all() and (g["sequence"][g["loop_c"]] == 0).any()
    # the Huber loss: inactive on every loop edge of one case at its start, active on the planted outlier of another
    def loop_sq(name):
        c = CASES[name]
        G = m.build_graph(*lc.args(c), c["opt"])
        r = m.factor(c["g"]["q"][G["edge_i"]], c["g"]["t"][G["edge_i"]], c["g"]["q"][G["edge_j"]], c["g"]["t"][G["edge_j"]], G["meas"], 0.1, 0.01, np.float64)[0]
        return (r * r).sum(axis=1)[G["kind"] == 1]
    assert (loop_sq("n9_huber_inactive") < 0.01).all() and ref["n9_huber_inactive"]["iterations"] >= 1
    assert loop_sq("n65_outlier")[2] > 100 * 0.01
    # free poses at the identity whose step is exactly zero
    lo, hi = CASES["n65_identity_tail"]["g"]["identity_tail"]
    r = ref["n65_identity_tail"]
    assert r["graph"]["free"][lo:hi].all() and r["num_successful"] >= 1
    assert np.array_equal(r["q"][lo:hi], np.tile([1.0, 0, 0, 0], (hi - lo, 1))) and not r["t"][lo:hi].any()
    # a relative rotation beyond 90 degrees whose error quaternion has w < 0
    c = CASES["n65_negated_q"]["g"]
    e = m.qmul(m.qconj(c["loop_meas"][:, 3:]), m.qmul(m.qconj(c["q"][c["loop_c"]]), c["q"][c["loop_i"]]))
    assert (e[:, 0] < 0).all() and (np.abs(c["loop_meas"][:, 3]) < np.cos(np.pi / 4)).any()


def _measured(both):
    worst = dict(r=0.0, J=0.0, eval_cost=0.0, pose=0.0, cost=0.0)
    for name, (a, b) in both.items():
        rr = lc.solve_ratios(a, b)
        e = lc.eval_case(name)
        ev = [m.eval_edges(e["q"], e["t"], e["edge_i"], e["edge_j"], e["kind"], e["meas"], e["opt"], dt) for dt in (np.float64, m.LD)]
        er = lc.eval_ratios(ev[0], ev[1])
        for k, v in (("r", er["r"]), ("J", er["J"]), ("eval_cost", er["cost"]), ("pose", rr["pose"]), ("cost", rr["cost"])):
            worst[k] = max(worst[k], v)
    return worst


def test_bounds_cover_four_times_the_cpu_ratio(both):
    worst = _measured(both)
    print("r_cpu", worst)
    for k, v in worst.items():
        assert lc.K[k] == 2.0 ** np.ceil(np.log2(4 * v)), (k, v)


def test_accepted_steps_lower_the_cost(both):
    for name in ("n257_two_sequences", "n257_128_loops", "n65_outlier"):
        r = both[name][0]
        h = [float(c) for c in r["cost_history"]]
        assert r["num_successful"] >= 2
        for k, acc in enumerate(r["accepted"]):
            assert (h[k + 1] < h[k]) if acc else (h[k + 1] == h[k])
