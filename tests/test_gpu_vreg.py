"""gfbe_vmap_register / gfbe_vmap_add_scan on the device against the numpy model (tests/vreg_np.py), one outer iteration at a time: for
outer iteration k the model is started from the device's own pose_trace[k - 1] (the input poses for k = 0), so one iteration's rounding
is not amplified through the next association. Discrete results (n_res, lm_iterations, lm_accepted, lm_termination, the flags) must be
equal; pose_trace, the costs and the two diffs must lie within K_X u A_X of the longdouble model (vreg_cases.K, measured on the CPU by
test_vreg_model.py), sv within vmap_cases.K["sv"].

Held association: the handle holds the LAST association, which ran at the poses the last outer iteration started from; the fresh
associate it is compared with is therefore made at those poses (pose_trace[-2], or the input), and both are linearised at the returned
poses."""
import numpy as np
import pytest

from _gfbe_import import gf
import vmap_cases
import vmap_np as vm
import vreg_cases as vc
import vreg_np as vr

pytestmark = pytest.mark.gpu
abi = gf.abi
CASES = vc.cases()


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


def device_map(be, case, seed_from=None):
    v = be.voxel_map(case["cap"], **case["vopt"])
    if seed_from is not None:
        d = seed_from.download()
        v.upload(d["keys"], d["counts"], d["points"])
    elif len(case["map"]):
        v.add_points(case["map"], 0)
    return v


def run_device(v, c, **kw):
    return v.register_raw(c["ct"], c["raw"], c["alpha"], c["pb"], c["pe"], c["prev_t"], c["prev_q"], False, **dict(c["o"], **kw))


def check_against_model(m, c, x_in, sm, ob, oe, worst):
    """Every outer iteration of the device's summary against one model iteration from the device's own start."""
    x = np.asarray(x_in, np.float64)
    k, last = 0, None
    while True:
        ld = vr.outer_iteration(m, c["ct"], c["raw"], c["alpha"], x, c["o"], c["prev_t"], c["prev_q"], False, vm.LD)
        last = ld
        assert sm["n_res"][k] == ld["n_res"], k
        if ld["n_res"] == 0:
            assert sm["no_residuals"] == 1 and sm["outer_iterations"] == k
            break
        l = ld["lm"]
        assert (sm["lm_iterations"][k], sm["lm_accepted"][k], sm["lm_termination"][k]) == (l["iterations"], l["accepted"], l["termination"]), k
        f = lambda a: np.asarray(a, vm.LD)
        r = dict(pose=float(np.abs(f(sm["pose_trace"][k]) - ld["x"]).max()) / (vm.U * ld["A_pose"]),
                 cost=max(float(abs(f(sm["cost_initial"][k]) - l["cost_initial"])) / (vm.U * l["A_cost_initial"]), float(abs(f(sm["cost_final"][k]) - l["cost_final"])) / (vm.U * l["A_cost_final"])),
                 diff_trans=float(abs(f(sm["diff_trans"][k]) - ld["diff_trans"])) / (vm.U * ld["A_dt"]), diff_rot=float(abs(f(sm["diff_rot"][k]) - ld["diff_rot"])) / (vm.U * ld["A_dr"]))
        for q, val in r.items():
            worst[q] = max(worst.get(q, 0.0), val)
        x = sm["pose_trace"][k].copy()
        k += 1
        if ld["converged"] or k >= c["o"]["max_num_iteration"]:
            assert sm["converged"] == int(ld["converged"]) and sm["no_residuals"] == 0
            break
    assert sm["outer_iterations"] == k
    assert np.array_equal(np.concatenate([ob, oe]), x)
    sv, deg, A_sv = vm.localizability(last["rows"]["normals"], last["rows"]["relgap_res"], vm.LD)
    assert sm["degenerate"] == int(deg)
    if last["n_res"]:
        ok = np.isfinite(A_sv)
        worst["sv"] = max(worst.get("sv", 0.0), float((np.abs(sm["sv"].astype(vm.LD) - sv).astype(float)[ok] / (vm.U * A_sv[ok])).max()) if ok.any() else 0.0)
    return k


@pytest.mark.parametrize("name", list(CASES))
def test_case_against_the_model(be, name):
    """Worst ratios |device - longdouble model| / (u A) measured on the MI355X over all cases: pose 0.33, cost 0.56, diff_trans 0.24,
    diff_rot 0.35, sv 0.25 (bounds: K = 2, 4, 2, 2 and 2)."""
    c = CASES[name]
    m = vc.build_map(c)
    v = device_map(be, c)
    try:
        rc, ob, oe, sm = run_device(v, c)
        assert rc == abi.OK
        worst = {}
        n_it = check_against_model(m, c, np.concatenate([c["pb"], c["pe"]]), sm, ob, oe, worst)
        print(name, "outer", n_it, "worst ratios", {k: round(val, 3) for k, val in worst.items()})
        few = any(sm["n_res"][k] < c["o"]["min_num_residuals"] for k in range(max(1, n_it if sm["no_residuals"] == 0 else n_it + 1)))
        assert sm["too_few_residuals"] == int(few)
        for q, val in worst.items():
            assert val <= (vmap_cases.K["sv"] if q == "sv" else vc.K[q]), (q, val)
        if c["converging"]:
            e0, e1 = vc.pose_error(np.concatenate([c["pb"], c["pe"]]), c), vc.pose_error(np.concatenate([ob, oe]), c)
            assert e1 < 0.5 * e0, (e0, e1)
        # held association: linearize on the handle == lio_linearize on a fresh associate at the poses the last association ran at
        if sm["no_residuals"] == 0:
            x_last = sm["pose_trace"][n_it - 2] if n_it >= 2 else np.concatenate([c["pb"], c["pe"]])
            si = float(np.sqrt(1.0 / c["o"]["laser_point_cov"]))
            held = v.linearize(c["ct"], si, ob, oe)
            v2 = device_map(be, c, seed_from=v)
            rows = v2.associate(c["ct"], c["raw"], c["alpha"], x_last[:7], x_last[7:])
            fresh = abi.lio_linearize(be.lib, "gfbe_", be.ctx, c["ct"], rows["pts"], rows["normals"], rows["offsets"], rows["alpha"], rows["weights"], si, ob, oe, blocks=False)
            v2.close()
            assert np.array_equal(held["H"], fresh["H"]) and np.array_equal(held["g"], fresh["g"]) and held["cost"] == fresh["cost"]
            v.add_points(c["map"][:3] + 0.01, 0)
            assert v.linearize_raw(c["ct"], si, ob, oe)[0] == abi.BAD_INPUT
    finally:
        v.close()


def _same(a, b):
    (rc1, ob1, oe1, s1), (rc2, ob2, oe2, s2) = a, b
    assert rc1 == rc2 and np.array_equal(ob1, ob2) and np.array_equal(oe1, oe2)
    for k in s1:
        assert np.array_equal(np.asarray(s1[k]), np.asarray(s2[k])), k


@pytest.mark.parametrize("name", ["ct1_default", "ct0_default", "rows_257"])
def test_same_bits_twice_and_on_a_seeded_handle(be, name):
    c = CASES[name]
    v = device_map(be, c)
    v2 = device_map(be, c, seed_from=v)
    try:
        a = run_device(v, c)
        _same(a, run_device(v, c))
        _same(a, run_device(v2, c))
    finally:
        v.close()
        v2.close()


@pytest.mark.parametrize("ct", [0, 1])
def test_add_scan(be, ct):
    c = CASES["ct1_default" if ct else "ct0_default"]
    v, v2 = device_map(be, c), device_map(be, c)
    m = vc.build_map(c)
    try:
        world = v.add_scan(ct, c["raw"], c["alpha"], c["true_b"], c["true_e"], 0, want_world=True)
        ref = np.array([vm.world_point(ct, c["true_b"].astype(vm.LD), c["true_e"].astype(vm.LD), vm.LD(c["alpha"][i]) if ct else vm.LD(0), c["raw"][i].astype(vm.LD), vm.LD) for i in range(len(c["raw"]))])
        # world-point bound: u (|R| |p| + |t|) per rounding of the rotation, the product and the sum: 8 u (|p|_1 + |t|_1 + 1)
        bound = 8 * vm.U * (np.abs(c["raw"]).sum(axis=1) + np.abs(c["true_b"][:3]).sum() + np.abs(c["true_e"][:3]).sum() + 1)
        assert (np.abs(world.astype(vm.LD) - ref).astype(float).max(axis=1) <= bound).all()
        m.add_points(world, 0)
        got, want = v.download(), m.download()
        for k in ("keys", "counts", "points"):
            assert np.array_equal(got[k], want[k]), k
        assert v2.add_scan(ct, c["raw"], c["alpha"], c["true_b"], c["true_e"], 0) is None
        got2 = v2.download()
        for k in ("keys", "counts", "points"):
            assert np.array_equal(got2[k], want[k]), k
    finally:
        v.close()
        v2.close()


def test_frame_loop(be):
    """register -> add_scan -> erase_far over three rounds of the room; every registration checked as above, the map against the model
    fed with the device's world points."""
    vopt, cap, steps = vmap_cases.room_rounds(n_kp=360)
    v = be.voxel_map(cap, **vopt)
    m = vm.Map(cap, **vopt)
    o = vr.options(min_num_residuals=50, max_num_iteration=3)
    worst = {}
    try:
        first = True
        for pts, loc, sc, pb, pe in steps:
            if first:
                v.add_points(pts, 0)
                m.add_points(pts, 0)
                first = False
            rng = np.random.default_rng(5)
            c = dict(ct=1, raw=sc["raw"], alpha=sc["alpha"], pb=vc._perturb(pb, rng, 0.02, 0.3), pe=vc._perturb(pe, rng, 0.02, 0.3), prev_t=pb[:3], prev_q=pb[3:], o=o)
            rc, ob, oe, sm = run_device(v, c)
            assert rc == abi.OK
            check_against_model(m, c, np.concatenate([c["pb"], c["pe"]]), sm, ob, oe, worst)
            world = v.add_scan(1, sc["raw"], sc["alpha"], ob, oe, 0, want_world=True)
            m.add_points(world, 0)
            v.erase_far(loc)
            m.erase_far(loc)
            got, want = v.download(), m.download()
            for k in ("keys", "counts", "points"):
                assert np.array_equal(got[k], want[k]), k
        print("frame loop worst ratios", worst)
        for q, val in worst.items():
            assert val <= (vmap_cases.K["sv"] if q == "sv" else vc.K[q]), (q, val)
    finally:
        v.close()


def test_unusable_solve_returns_numerical_failure(be):
    """The third deviation: where the reference throws, the call returns GFBE_NUMERICAL_FAILURE and every output is written at the
    last accepted poses (here the input: no step was ever valid)."""
    c = vc.unusable_case()
    m = vc.build_map(c)
    v = device_map(be, c)
    try:
        rc, ob, oe, sm = run_device(v, c)
        with np.errstate(invalid="ignore"):
            ref = vr.register(m, c["ct"], c["raw"], c["alpha"], c["pb"], c["pe"], c["o"], c["prev_t"], c["prev_q"])
        assert ref["failed"]
        assert rc == abi.NUMERICAL_FAILURE
        assert np.array_equal(ob, c["pb"]) and np.array_equal(oe, c["pe"])
        assert sm["outer_iterations"] == 1 and sm["converged"] == 0 and sm["no_residuals"] == 0
        assert sm["n_res"][0] == ref["iterations"][0]["n_res"] > 0
        assert (sm["lm_iterations"][0], sm["lm_accepted"][0], sm["lm_termination"][0]) == (5, 0, 4)
        assert np.array_equal(sm["pose_trace"][0], np.concatenate([c["pb"], c["pe"]])) and sm["diff_trans"][0] == 0.0 and np.isfinite(sm["diff_rot"][0])
        assert np.isnan(sm["cost_initial"][0]) and not sm["n_res"][1:].any()
        sv, deg, _ = vm.localizability(ref["iterations"][0]["rows"]["normals"], None, np.float64)
        assert sm["degenerate"] == int(deg) and np.allclose(sm["sv"], sv.astype(float), rtol=1e-12)
    finally:
        v.close()


def test_overflow_flag_refuses_and_leaves_outputs(be):
    c = CASES["ct0_default"]
    v = be.voxel_map(8, **c["vopt"])
    try:
        v.add_points(c["map"][:4] * 0.1, 0)
        v.add_points(c["map"], 0)      # would pass the capacity: sticky flag
        assert v.size()["overflow"] == 1
        rc, ob, oe, sm = run_device(v, c)
        assert rc == abi.BAD_INPUT and np.isnan(ob).all() and np.isnan(oe).all() and sm["outer_iterations"] == 0 and not sm["n_res"].any()
    finally:
        v.close()
