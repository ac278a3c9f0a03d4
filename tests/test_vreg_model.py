"""The numpy model of the registration loop (tests/vreg_np.py) checked on the CPU: its Jacobians against central differences on the
manifold, its LM loop against a brute-force restatement of the radius and acceptance rules, convergence and decision margins of every
case of tests/vreg_cases.py, the bounds K_X (r_cpu: the FP64 model against the longdouble model over one outer iteration from the same
start), and the contract of the new entry points without a device.

Bounds (unit u A): pose A = kappa (|delta|_1 + |x|_inf), kappa the condition number of the scaled, regularised matrix of the last
accepted step and delta the iteration's total step; it bounds the FP64 model as it is (r_cpu 0.45). Two sums are wider than the plain
absolute sum, and why: the final cost is taken at the final pose, so its A carries |g|_1 A_pose (without it far_start measured
r_cpu 19); diff_rot goes through an acos near 1, so its A carries 8 / max(theta, sqrt(8 u)) per half."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import vmap_np as vm
import vreg_cases as vc
import vreg_np as vr

abi = gf.abi
CASES = vc.cases()
_cache = {}


def model_run(name):
    """(case, model map, the FP64 model's whole registration), computed once and shared."""
    if name not in _cache:
        c = CASES[name]
        m = vc.build_map(c)
        _cache[name] = (c, m, vr.register(m, c["ct"], c["raw"], c["alpha"], c["pb"], c["pe"], c["o"], c["prev_t"], c["prev_q"]))
    return _cache[name]


def _num_grad(f, x, step, n, h=1e-6):
    g = np.zeros(n)
    for a in range(n):
        d = np.zeros(n)
        d[a] = h
        g[a] = (f(step(x, d)) - f(step(x, -d))) / (2 * h)
    return g


def test_consistency_jacobians_against_central_differences():
    rng = np.random.default_rng(3)
    o = vr.options(beta_location_consistency=0.7, beta_orientation_consistency=1.3, beta_small_velocity=2.0)
    x = np.concatenate([vc._perturb(np.array([0.1, -0.2, 0.3, 0, 0, 0, 1.0]), rng, 0.2, 20.0), vc._perturb(np.array([0.2, -0.1, 0.35, 0, 0, 0, 1.0]), rng, 0.2, 25.0)])
    prev_t, prev_q = rng.normal(size=3), vc._perturb(np.array([0, 0, 0, 0, 0, 0, 1.0]), rng, 0.0, 15.0)[3:]

    def step(xa, d):
        return np.concatenate([vr.plus(xa[:7], d[:6], np.float64), vr.plus(xa[7:], d[6:], np.float64)])
    facs = vr.consistency(x, 200, o, prev_t, prev_q, np.float64)
    assert len(facs) == 3
    for i, (r, J) in enumerate(facs):
        for k in range(3):
            num = _num_grad(lambda xx: vr.consistency(xx, 200, o, prev_t, prev_q, np.float64)[i][0][k], x, step, 12)
            assert np.abs(num - J[k]).max() < 1e-7 * max(1.0, np.abs(J).max()), (i, k)


@pytest.mark.parametrize("delta", [0.5, 0.0])
def test_robustified_point_to_plane_gradient(delta):
    """ct = 0 (the ct = 1 rotation blocks are the reference's approximation, quantified in test_lio_oracle.py): the gradient of the
    robustified cost rho(r^2) / 2 equals J'^T r' of the corrected factor, for an inlier and an outlier."""
    rng = np.random.default_rng(5)
    pose = vc._perturb(np.array([0.3, 0.1, -0.2, 0, 0, 0, 1.0]), rng, 0.1, 30.0)
    seen = set()
    for off in (0.0, 0.05):
        p, nv = rng.normal(size=3), rng.normal(size=3)
        nv /= np.linalg.norm(nv)
        w, si = 0.8, np.sqrt(1.0 / 0.001)

        def cost(xx):
            r, J, _ = vr.row(0, p, nv, off0, w, 0.0, si, xx, xx, np.float64)
            return float(vr.huber(r, J, np.float64(delta), np.float64)[2])
        r_at = vr.row(0, p, nv, 0.0, w, 0.0, si, pose, pose, np.float64)[0]
        off0 = off - r_at / (si * w)      # residual = si w off: 0 (inlier) or 1.26 (outlier of delta 0.5)
        r, J, _ = vr.row(0, p, nv, off0, w, 0.0, si, pose, pose, np.float64)
        r2, J2, _, outlier = vr.huber(r, J, np.float64(delta), np.float64)
        seen.add(bool(outlier))
        num = _num_grad(cost, pose, lambda xa, d: vr.plus(xa, d, np.float64), 6)
        assert np.abs(num - J2 * r2).max() < 1e-6 * max(1.0, np.abs(J2 * r2).max())
    assert seen == ({False, True} if delta > 0 else {False})


def test_lm_against_a_brute_force_restatement():
    """A 12-dimensional quadratic plus Huber terms: the model's accept / reject sequence, radii and end point against a plain loop that
    solves each regularised system with numpy and applies the radius rules literally."""
    rng = np.random.default_rng(9)
    A, b = rng.normal(size=(40, 12)), rng.normal(size=40) * 3

    def evaluate(x):
        H, g, c = np.zeros((12, 12)), np.zeros(12), 0.0
        for k in range(40):
            r2, J2, ck, _ = vr.huber(np.float64(A[k] @ x - b[k]), A[k].copy(), np.float64(1.0), np.float64)
            H, g, c = H + np.outer(J2, J2), g + J2 * r2, c + ck
        return H, g, np.float64(c), float(c)
    x0 = rng.normal(size=12) * 5
    res = vr.lm(evaluate, x0.copy(), lambda x, d: x + d, 16, np.float64)
    # brute force
    x, radius, dec, acc, it = x0.copy(), 1e4, 2.0, [], 0
    H, g, c, _ = evaluate(x)
    s = 1 / (1 + np.sqrt(np.diag(H)))
    D = None
    while it < 16 and np.abs(g).max() > 1e-10:
        it += 1
        Hs = H * np.outer(s, s)
        if D is None:
            D = np.clip(np.diag(Hs), 1e-6, 1e32)
        y = np.linalg.solve(Hs + np.diag(D / radius), -s * g)
        mc = -((s * g) @ y + 0.5 * y @ Hs @ y)
        cand = x + s * y
        cc = evaluate(cand)[2]
        if np.linalg.norm(cand - x) <= 1e-8 * (np.linalg.norm(x) + 1e-8) or abs(c - cc) <= 1e-6 * c:
            break
        rho = (c - cc) / mc
        if rho > 1e-3:
            x, c, radius, dec, D = cand, cc, min(1e16, radius / max(1 / 3, 1 - (2 * rho - 1) ** 3)), 2.0, None
            H, g = evaluate(x)[:2]
            acc.append(1)
        else:
            radius, dec = radius / dec, dec * 2
            acc.append(0)
    assert res["iterations"] == it
    assert [int(t["accepted"]) for t in res["trace"]] == acc[:len(res["trace"])]
    assert np.abs(res["x"] - x).max() < 1e-9 * np.abs(x).max()
    assert abs(res["final_radius"] - radius) <= 1e-9 * radius


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["converging"]])
def test_model_converges(name):
    """Final registration error (vreg_cases.pose_error) below a quarter of the start error. Measured: ct1_default 0.150, ct0_default
    0.097, clutter 0.144, no_loss 0.130, betas_zero 0.245, betas_mixed 0.089, rows_* 0.12-0.13, equal_rotations 0.181."""
    c, _, res = model_run(name)
    e0, e1 = vc.pose_error(np.concatenate([c["pb"], c["pe"]]), c), vc.pose_error(res["x"], c)
    print(name, "pose error %.4f -> %.4f" % (e0, e1), "outer", res["outer_iterations"], "converged", res["converged"])
    assert e1 < 0.25 * e0


def test_cases_take_the_paths_they_are_named_for():
    r = {n: model_run(n)[2] for n in CASES}
    assert r["ct1_default"]["converged"] and 2 <= r["ct1_default"]["outer_iterations"] < 10
    assert not r["cap"]["converged"] and r["cap"]["outer_iterations"] == 2
    assert all(it["lm"]["iterations"] == 0 for it in r["lm0"]["iterations"])
    assert any(t["valid"] and not t["accepted"] for it in r["far_start"]["iterations"] for t in it["lm"]["trace"])
    assert r["clutter"]["iterations"][0]["n_outliers_first"] > 0
    assert r["empty_map"]["no_residuals"] == 1 and r["empty_map"]["outer_iterations"] == 0
    assert r["below_min"]["too_few_residuals"] == 1 and r["ct1_default"]["too_few_residuals"] == 1 and r["cap"]["too_few_residuals"] == 0
    for cut in (vc.WG - 1, vc.WG, vc.WG + 1):
        assert all(it["n_res"] == cut for it in r["rows_%d" % cut]["iterations"])
    assert all(it["n_res"] == 1 for it in r["one_row"]["iterations"])
    eq = r["equal_rotations"]["iterations"]
    # the clamp is needed: the unclamped argument of the carried pose is above 1, where an unclamped acos is NaN and the model's is 0
    assert all(it["acos_args"][1] > 1.0 for it in eq)
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.arccos(np.float64(eq[0]["acos_args"][1])))
    assert all(np.isfinite(float(it["diff_rot"])) and abs(it["acos_args"][1] - 1.0) < 1e-15 for it in eq) and r["equal_rotations"]["converged"]


def test_unusable_solve_in_the_model():
    """Five invalid steps in a row: the model reports failure, keeps the poses and stops after this outer iteration."""
    c = vc.unusable_case()
    with np.errstate(invalid="ignore"):
        res = vr.register(vc.build_map(c), c["ct"], c["raw"], c["alpha"], c["pb"], c["pe"], c["o"], c["prev_t"], c["prev_q"])
    l = res["iterations"][0]["lm"]
    assert res["failed"] and res["outer_iterations"] == 1 and len(res["iterations"]) == 1 and not res["converged"]
    assert (l["iterations"], l["accepted"], l["termination"]) == (5, 0, 4) and all(not t["valid"] for t in l["trace"])
    assert np.array_equal(res["x"], np.concatenate([c["pb"], c["pe"]]))


def _iteration_pairs(name):
    """For every outer iteration of the FP64 run: (the FP64 and the longdouble model over that iteration from the same float64 start)."""
    c, m, res = model_run(name)
    x = np.concatenate([c["pb"], c["pe"]])
    for it in res["iterations"]:
        ld = vr.outer_iteration(m, c["ct"], c["raw"], c["alpha"], x, c["o"], c["prev_t"], c["prev_q"], False, vm.LD)
        yield c, it, ld
        if it["n_res"]:
            x = np.asarray(it["x"], np.float64)


def ratios(got, ld):
    """|got - ld| / (u A) of one outer iteration: got = dict(x, cost_initial, cost_final, diff_trans, diff_rot) in float64."""
    l = ld["lm"]
    f = lambda v: np.asarray(v, vm.LD)
    return dict(pose=float(np.abs(f(got["x"]) - ld["x"]).max()) / (vm.U * ld["A_pose"]),
                cost=max(float(abs(f(got["cost_initial"]) - l["cost_initial"])) / (vm.U * l["A_cost_initial"]), float(abs(f(got["cost_final"]) - l["cost_final"])) / (vm.U * l["A_cost_final"])),
                diff_trans=float(abs(f(got["diff_trans"]) - ld["diff_trans"])) / (vm.U * ld["A_dt"]), diff_rot=float(abs(f(got["diff_rot"]) - ld["diff_rot"])) / (vm.U * ld["A_dr"]))


def test_bounds_cover_four_times_the_cpu_ratio():
    worst = dict(pose=0.0, cost=0.0, diff_trans=0.0, diff_rot=0.0)
    for name in CASES:
        for c, it, ld in _iteration_pairs(name):
            assert it["n_res"] == ld["n_res"], name
            if not it["n_res"]:
                continue
            a, b = it["lm"], ld["lm"]
            assert (a["iterations"], a["accepted"], a["termination"]) == (b["iterations"], b["accepted"], b["termination"]), name
            r = ratios(dict(x=it["x"], cost_initial=a["cost_initial"], cost_final=a["cost_final"], diff_trans=it["diff_trans"], diff_rot=it["diff_rot"]), ld)
            for k in worst:
                worst[k] = max(worst[k], r[k])
    print("r_cpu", worst)
    for k, r in worst.items():
        want = 1
        while want < 4 * r:
            want *= 2
        assert vc.K[k] == want, (k, r, want)


def test_decision_margins():
    """No discrete decision of any case is nearer to its threshold than 1e3 times the bound K u A of the quantity compared."""
    for name in CASES:
        for c, it, ld in _iteration_pairs(name):
            if not ld["n_res"]:
                continue
            kq = dict(gradient=1.0, parameter=vc.K["pose"], function=vc.K["cost"], quality=vc.K["cost"], exit_trans=vc.K["diff_trans"], exit_rot=vc.K["diff_rot"])
            for kind, gap, A in ld["lm"]["margins"]:
                assert gap >= 1e3 * kq[kind] * vm.U * A, (name, kind, gap, A)
            for gap, A_r in ld["hub"]:
                assert gap >= 1e3 * 4 * vm.U * A_r, (name, "huber", gap, A_r)
            assert ld["rows"]["margin"]["tie"] > 1e-9 and ld["rows"]["margin"]["plane"] > 1e-9 and ld["rows"]["relgap_res"].min() > 1e-3, name


def test_abi_contract_without_a_device():
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    for s in ("gfbe_vreg_default_options", "gfbe_vmap_register", "gfbe_vmap_add_scan"):
        assert s in gf.backend.EXPORTS and hasattr(lib, s), s
    lib.gfbe_create.restype = abi.c_i
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    opt = abi.vreg_default_options(lib)
    assert opt.struct_size == C.sizeof(abi.VregOptions) == 72
    for k, v in vr.DEFAULTS.items():
        assert getattr(opt, k) == v, k
    assert C.sizeof(abi.VregSummary) == 8 * (3 + 3 + 4 * 16 + 4 * 32 + 32 * 14)
    lib.gfbe_vmap_register.restype = abi.c_i
    lib.gfbe_vmap_add_scan.restype = abi.c_i
    pose, out_b, out_e = np.array([0, 0, 0, 0, 0, 0, 1.0]), np.full(7, 7.0), np.full(7, 7.0)
    P = lambda a: a.ctypes.data_as(abi.PD)
    args = (0, 0, None, None, P(pose), P(pose), None, None, 0, P(out_b), P(out_e), None)
    assert lib.gfbe_vmap_register(ctx, None, C.byref(opt), *args) == abi.NO_DEVICE
    assert lib.gfbe_vmap_register(ctx, None, None, *args) == abi.NO_DEVICE
    bad = abi.vreg_default_options(lib)
    bad.struct_size = 64
    assert lib.gfbe_vmap_register(ctx, None, C.byref(bad), *args) == abi.BAD_INPUT
    assert lib.gfbe_vmap_register(None, None, C.byref(opt), *args) == abi.BAD_INPUT
    assert lib.gfbe_vmap_add_scan(ctx, None, 0, 0, None, None, P(pose), P(pose), 0, None) == abi.NO_DEVICE
    assert np.all(out_b == 7.0) and np.all(out_e == 7.0)
    lib.gfbe_destroy(ctx)
