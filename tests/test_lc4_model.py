"""The model of the loop-closure pose graph (tests/lc4_np.py) against itself, without a GPU: analytic Jacobians against central
differences through Plus, the band + Woodbury path against the dense path, the FP64 model against the longdouble model (r_cpu, from
which the bounds K of tests/lc4_cases.py follow), the decision margins of every case, and the closed loop on a figure-of-eight.

Measured here (FP64 against longdouble, every case of lc4_cases.cases(), units u A_X):
  r_cpu: r 1.43, J 1.42, eval_cost 0.17, pose 0.28, cost 0.13  ->  K: r 8, J 8, eval_cost 1, pose 2, cost 1.
Smallest decision margin of any case, in units of u x the absolute sum behind the quantity compared: 1.0e5 (n65_64_loops, the
function-tolerance test of its last iteration); the bound asks for 1e3."""
import numpy as np
import pytest

import lc4_cases as lc
import lc4_np as m

CASES = lc.cases()


@pytest.fixture(scope="module")
def both():
    return {name: (lc.reference(name, "f64"), lc.reference(name, "ld")) for name in CASES}


def _edge(kind, yaw_i, ti, yaw_j, tj, meas, dt, opt=None):
    ev = m.eval_edges(np.array([yaw_i, yaw_j], dt), np.array([ti, tj], dt), [0], [1], [kind], np.asarray(meas, dt).reshape(1, 6), opt or m.options(), dt)
    return ev["r"][0], ev["J"][0]


# yaw_j - yaw_i - relative_yaw on both sides of +180 and of -180, away from it, and with non-zero pitch and roll; kind 1 below and above
# the Huber threshold
JAC_CASES = [
    (0, 10.0, 25.0, 14.0, 0.0, 0.0), (0, 170.0, -175.0, 14.0, 3.0, -2.0), (0, 100.0, -70.0, 11.0, 5.0, 4.0), (0, 100.0, -70.0, 9.0, 5.0, 4.0),
    (0, -100.0, 70.0, -11.0, -6.0, 2.5), (0, -100.0, 70.0, -9.0, -6.0, 2.5), (1, 30.0, 31.0, 0.99, 1.0, -1.0), (1, 170.0, -175.0, 14.0, 3.0, -2.0),
    (1, 100.0, -70.0, 11.0, 5.0, 4.0), (1, -100.0, 70.0, -9.0, -6.0, 2.5),
]


@pytest.mark.parametrize("kind,yaw_i,yaw_j,rel_yaw,pitch,roll", JAC_CASES)
def test_analytic_jacobians_agree_with_central_differences_through_plus(kind, yaw_i, yaw_j, rel_yaw, pitch, roll):
    dt = m.LD
    ti, tj = np.array([1.0, 2.0, 3.0], dt), np.array([1.5, 1.0, 3.2], dt)
    small = kind == 1 and abs(yaw_j - yaw_i - rel_yaw) < 2      # the kind-1 case below the Huber threshold: a measurement near the truth
    R = m.ypr_to_R(np.array([yaw_i], dt), np.array([pitch], dt), np.array([roll], dt), dt)[0][0].reshape(3, 3)
    tm = (R.T @ (tj - ti)).astype(np.float64) + (0.01 if small else 0.3)
    meas = [tm[0], tm[1], tm[2], rel_yaw, pitch, roll]
    r0, J = _edge(kind, yaw_i, ti, yaw_j, tj, meas, dt)
    assert (r0 @ r0 > 0.01) == (not small) or kind == 0
    h = dt(1e-7)
    x = np.array([[yaw_i, *ti], [yaw_j, *tj]], dt)
    for col in range(8):
        d = np.zeros((2, 4), dt)
        d[col // 4, col % 4] = h
        yp, tp = m.plus(x[:, 0], x[:, 1:], d, dt)
        ym, tmm = m.plus(x[:, 0], x[:, 1:], -d, dt)
        rp, _ = _edge(kind, yp[0], tp[0], yp[1], tp[1], meas, dt)
        rm, _ = _edge(kind, ym[0], tmm[0], ym[1], tmm[1], meas, dt)
        num = (rp - rm) / (2 * h)
        if kind == 1 and not small:
            # the corrector's Jacobian is Ceres' Gauss-Newton form s1 (J - alpha r r^T J / |r|^2), alpha = 0 for Huber: sqrt(rho') J, not the
            # derivative of the corrected residual; compare what it scales
            r_raw, J_raw = m.factor(x[:1, 0], x[:1, 1:], x[1:, 0], x[1:, 1:], np.asarray(meas, dt).reshape(1, 6), np.array([dt(1) / 10], dt), dt)[:2]
            s1 = np.sqrt(dt(0.1) / np.sqrt(r_raw[0] @ r_raw[0]))
            assert np.abs(J[:, col] - s1 * J_raw[0][:, col]).max() < 1e-15
            continue
        assert np.abs(num - J[:, col]).max() < 1e-9, (col, num, J[:, col])


def test_wrapped_residual_is_continuous_across_the_wrap():
    ti, tj = np.zeros(3), np.ones(3)
    for e in (179.9, 180.1, -179.9, -180.1):
        r, _ = _edge(0, 0.0, ti, e, tj, [0, 0, 0, 0.0, 0, 0], np.float64)
        assert abs(abs(r[3]) - 179.9) < 1e-9


@pytest.mark.parametrize("name", ["n2_loop_into_constant", "n5_no_loop", "n63_one_loop", "n64_shapes", "n65_64_loops", "yaw_wrap", "far_start"])
def test_band_and_woodbury_path_equals_the_dense_path(both, name):
    c = CASES[name]
    band = both[name][0]
    dense = m.solve(*c["args"], opt=c["opt"], dt=np.float64, path="dense")
    assert lc.decisions(band) == lc.decisions(dense)
    A = max(band["A_pose"], 1e-300)
    err = max(np.abs(band["t"] - dense["t"]).max(), np.abs(band["yaw"] - dense["yaw"]).max())
    print(name, "band against dense, units u A_pose:", err / (m.U * A))
    assert err <= lc.K["pose"] * m.U * A
    for a, b, Ac in zip(band["cost_history"], dense["cost_history"], band["A_cost"]):
        assert abs(a - b) <= 4 * m.U * (Ac + band["g_l1"][0] * A)


def test_band_path_solves_one_step_as_the_dense_path_in_longdouble():
    c = CASES["n65_64_loops"]
    G = m.build_graph(*c["args"], c["opt"])
    lin = m.linearize(G, np.asarray(c["g"]["ypr"][:, 0], m.LD), np.asarray(c["g"]["t"], m.LD), c["opt"], m.LD)
    act = lin["active"]
    scale = np.where(act, 1 / (1 + np.sqrt(np.where(act, lin["diag0"], 0))), m.LD(1))
    diag2 = np.minimum(np.maximum(lin["diag0"] * scale * scale, m.LD(1e-6)), m.LD(1e32))
    for radius in (1e4, 1e8):
        yb, mb = m.lm_step(lin, scale, diag2, m.LD(radius), m.LD, "band")
        yd, md = m.lm_step(lin, scale, diag2, m.LD(radius), m.LD, "dense")
        rel = float(np.abs(yb - yd).max() / np.abs(yd).max())
        print("radius", radius, "relative difference", rel)
        assert rel < 1e-15 and abs(float(mb - md)) < 1e-15 * abs(float(md))


def test_decisions_agree_between_precisions_with_margin(both):
    worst = np.inf
    for name, (a, b) in both.items():
        assert lc.decisions(a) == lc.decisions(b), name
        mr = min(lc.margin_ratio(a), lc.margin_ratio(b))
        print(name, lc.decisions(b), "smallest margin / (u A): %.3g" % mr)
        assert mr >= 1e3, name
        worst = min(worst, mr)
    print("smallest margin of any case: %.3g" % worst)


def test_cases_cover_the_paths():
    assert any(0 in r["accepted"][:-1] for r in (lc.reference("far_start", "f64"),))                  # rejected steps inside the run
    assert lc.reference("all_fixed", "f64")["iterations"] == 0 and lc.reference("all_fixed", "f64")["termination"] == 3
    assert lc.reference("max_it_0", "f64")["iterations"] == 0 and lc.reference("max_it_1", "f64")["iterations"] == 1
    c = CASES["yaw_wrap"]["g"]
    assert (np.abs(c["ypr"][:, 0]) > 170).any() and (c["ypr"][:, 0] > 90).any() and (c["ypr"][:, 0] < -90).any()
    g = CASES["n64_shapes"]["g"]
    assert g["loop_c"][0] == 0 and any(i // 4 == c // 4 for i, c in zip(g["loop_i"], g["loop_c"]))
    g = CASES["n257_two_sequences"]["g"]
    assert set(g["sequence"]) == {0, 1} and g["fixed"][g["sequence"] == 0].all() and (g["sequence"][g["loop_c"]] == 0).any()
    assert len(CASES["n65_64_loops"]["g"]["loop_i"]) == 64 and len(CASES["n257_64_loops"]["g"]["loop_i"]) == 64


def test_unusable_graph_ends_as_a_numerical_failure():
    u = lc.unusable_case()
    for dt in (np.float64, m.LD):
        r = m.solve(*u["args"], opt=u["opt"], dt=dt)
        assert (r["iterations"], r["termination"], r["status"], r["accepted"]) == (5, 4, 2, [0] * 5)


def _measured(both):
    worst = dict(r=0.0, J=0.0, eval_cost=0.0, pose=0.0, cost=0.0)
    for name, (a, b) in both.items():
        rr = lc.solve_ratios(a, b)
        e = lc.eval_case(name)
        ev = [m.eval_edges(e["ypr"][:, 0], e["t"], e["edge_i"], e["edge_j"], e["kind"], e["meas"], e["opt"], dt) for dt in (np.float64, m.LD)]
        er = lc.eval_ratios(ev[0], ev[1])
        for k, v in (("r", er["r"]), ("J", er["J"]), ("eval_cost", er["cost"]), ("pose", rr["pose"]), ("cost", rr["cost"])):
            worst[k] = max(worst[k], v)
    return worst


def test_bounds_cover_four_times_the_cpu_ratio(both):
    worst = _measured(both)
    print("r_cpu", worst)
    for k, v in worst.items():
        assert lc.K[k] == 2.0 ** np.ceil(np.log2(4 * v)), (k, v)


@pytest.mark.parametrize("name", ["n1001_convergence", "n257_64_loops"])
def test_closed_loop_on_a_figure_of_eight(both, name):
    """Drifted VIO poses and loop edges: every accepted step lowers the cost, and the result is closer to the truth than the start."""
    r, g = both[name][0], CASES[name]["g"]
    h = [float(c) for c in r["cost_history"]]
    assert r["num_successful"] >= 3
    for k, acc in enumerate(r["accepted"]):
        assert (h[k + 1] < h[k]) if acc else (h[k + 1] == h[k])
    before = np.sqrt(((g["t"] - g["true_t"]) ** 2).sum(axis=1).mean())
    after = np.sqrt(((r["t"] - g["true_t"]) ** 2).sum(axis=1).mean())
    yb = np.abs((g["ypr"][:, 0] - g["true_yaw"] + 180) % 360 - 180).mean()
    ya = np.abs((r["yaw"] - g["true_yaw"] + 180) % 360 - 180).mean()
    print(name, "rms position error %.3f -> %.3f m, mean yaw error %.3f -> %.3f deg" % (before, after, yb, ya))
    assert after < before and ya < yb
