"""Line landmarks on the GPU: gfbe_line_eval against the numpy restatement, and gfbe_line_refine (onlyLineOpt + removeLineOutlier,
estimator.cpp:4264-4332, feature_manager.cpp:1372-1460) against tests/line_np.py's Levenberg-Marquardt loop and culling."""
import numpy as np
import pytest

from _gfbe_import import gf
import line_np as ln

abi, synth_line = gf.abi, gf.synth_line
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return gf.Backend(device=0)


def _factor_cases(lw):
    Rwc, twc = ln.cam_poses(lw)
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])])
    pose, orth, obs = [], [], []
    for l in np.flatnonzero(ln.eligible(lw)):
        s = lw["start_frame"][l]
        x = ln.plk_to_orth(ln.plk_to_pose(lw["line_plucker"][l], Rwc[s], twc[s]))
        for k in range(lw["n_obs"][l]):
            pose.append(lw["pose"][s + k]); orth.append(x); obs.append(lw["obs"][off[l] + k])
    return np.array(pose), np.array(orth), np.array(obs)


@pytest.mark.parametrize("robustify", [False, True])
def test_line_eval_matches_numpy(be, robustify):
    lw = synth_line.line_window(seed=21)
    pose, orth, obs = _factor_cases(lw)
    got = be.line_eval(pose, lw["ex_cam"], orth, obs, 400.0, robustify)
    want = ln.eval_robust(pose, lw["ex_cam"], orth, obs, 400.0, robustify)
    for k in ("r", "J_pose", "J_ex", "J_orth"):
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * max(1.0, np.abs(want[k]).max()), k
    assert abs(got["cost"] - want["cost"]) <= 1e-12 * want["cost"]


def check_window(lw, got, want, strict=None):
    """got (device) against want (tests/line_np.py). Tolerances: 1e-9 (final cost relative, lines absolute); where the checker's own
    result moves under a rounding-sized change of the input (line_np.sensitivity), 1e3 times that movement. strict: the windows whose
    checker is stable to 1e-10 must meet 1e-9 outright — returns whether this one did."""
    el = ln.eligible(lw)
    cs, ls = ln.sensitivity(lw)
    tol_c, tol_l = max(1e-9, 1e3 * cs), np.maximum(1e-9, 1e3 * ls)
    sg, sw = got["summary"], want["summary"]
    for k in ("status", "iterations", "num_successful", "termination"):
        assert sg[k] == sw[k], (k, sg[k], sw[k])
    assert sg["accepted"] == sw["accepted"][:len(sg["accepted"])] and len(sg["accepted"]) == sw["iterations"] + 1
    if sw["iterations"]:
        assert abs(sg["final_cost"] - sw["final_cost"]) <= tol_c * sw["final_cost"]
        assert abs(sg["initial_cost"] - sw["initial_cost"]) <= 1e-12 * sw["initial_cost"]
    # ineligible lines (and every line after the < 4 exit) come back bit for bit
    same = ~el if sw["termination"] != 5 else np.ones(len(el), bool)
    assert np.array_equal(got["plucker"][same], np.asarray(lw["line_plucker"])[same])
    assert (np.abs(got["plucker"] - want["plucker"]).max(1) <= tol_l).all()
    assert got["keep"].tolist() == want["keep"].tolist()
    stable = cs <= 1e-10 and ls.max() <= 1e-10
    if stable:
        assert not sw["iterations"] or abs(sg["final_cost"] - sw["final_cost"]) <= 1e-9 * sw["final_cost"]
        assert np.abs(got["plucker"] - want["plucker"]).max() <= 1e-9
    return stable


def test_line_refine_matches_numpy_on_seeded_windows(be):
    wins = [synth_line.line_window(seed=100 + k, n_ok=20 + 7 * k, init_sigma=0.02) for k in range(24)]
    got = be.line_refine(wins)
    n_acc = n_rej = n_stable = 0
    for lw, g in zip(wins, got):
        want = ln.refine(lw)
        n_stable += check_window(lw, g, want)
        n_acc += sum(want["summary"]["accepted"][1:])
        n_rej += len(want["summary"]["accepted"]) - 1 - sum(want["summary"]["accepted"][1:])
    assert n_acc > 0 and n_rej > 0       # both branches of the trust region were taken
    assert n_stable >= 8, n_stable       # and most windows are held to 1e-9 outright


def test_fewer_than_four_eligible_lines_solve_nothing(be):
    lw = synth_line.line_window(seed=3, n_ok=1, n_behind=1, n_long=0, n_outlier=1)      # 3 eligible lines, one of them behind the cameras
    assert ln.eligible(lw).sum() == 3
    g = be.line_refine([lw])[0]
    assert np.array_equal(g["plucker"], lw["line_plucker"]) and g["keep"].all()
    assert g["summary"]["iterations"] == 0 and g["summary"]["termination"] == 5 and g["summary"]["status"] == abi.OK
    check_window(lw, g, ln.refine(lw))
    # one more eligible line: the solve runs, and the line behind the cameras is culled
    lw4 = synth_line.line_window(seed=3, n_ok=2, n_behind=1, n_long=0, n_outlier=1)
    g4 = be.line_refine([lw4])[0]
    assert g4["summary"]["iterations"] > 0 and not g4["keep"][lw4["kind"] == "behind"].any()
    check_window(lw4, g4, ln.refine(lw4))


def test_each_culling_reason(be):
    wins = [synth_line.line_window(seed=300 + k, n_behind=2, n_long=2, n_outlier=2) for k in range(4)]
    got = be.line_refine(wins)
    reasons = {"behind": "behind", "long": "far", "outlier_obs": "reprojection"}
    hits = dict.fromkeys(reasons.values(), 0)
    for lw, g in zip(wins, got):
        want = ln.refine(lw)
        check_window(lw, g, want)
        for kind, reason in reasons.items():
            sel = [l for l in np.flatnonzero(lw["kind"] == kind) if want["reason"][l] == reason]
            hits[reason] += len(sel)
            assert not g["keep"][sel].any(), kind
        assert {want["reason"][l] for l in np.flatnonzero(lw["kind"] == "behind")} == {"behind"}
        assert {want["reason"][l] for l in np.flatnonzero(lw["kind"] == "outlier_obs")} == {"reprojection"}
        ok = np.flatnonzero(lw["kind"] == "ok")
        assert g["keep"][ok].mean() > 0.9
        assert g["keep"][~ln.eligible(lw)].all()
    assert min(hits.values()) >= 4, hits


def _line_error(a, b):
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    return np.minimum(np.linalg.norm(a - b, axis=1), np.linalg.norm(a + b, axis=1))


def test_perturbed_start_converges_towards_the_true_lines(be):
    lw = synth_line.line_window(seed=9, n_ok=80, init_sigma=0.15)
    g = be.line_refine([lw])[0]
    ok = np.flatnonzero(lw["kind"] == "ok")
    before = _line_error(lw["line_plucker"][ok], lw["true_plucker"][ok])
    after = _line_error(g["plucker"][ok], lw["true_plucker"][ok])
    assert g["summary"]["num_successful"] > 0 and g["summary"]["final_cost"] < 0.5 * g["summary"]["initial_cost"]
    assert np.median(after) < 0.6 * np.median(before)


def test_window_alone_equals_window_in_a_batch_and_runs_repeat(be):
    wins = [synth_line.line_window(seed=500 + k, n_ok=10 + (k * 37) % 400) for k in range(257)]
    holders = [abi.LineWindowHolder(w) for w in wins]
    full = be.line_refine(holders)
    again = be.line_refine(holders)
    for w in (0, 128, 256):
        alone = be.line_refine([holders[w]])[0]
        for other in (full[w], again[w]):
            assert np.array_equal(alone["plucker"], other["plucker"]) and np.array_equal(alone["keep"], other["keep"])
            assert alone["summary"] == other["summary"]
    for a, b in zip(full, again):
        assert np.array_equal(a["plucker"], b["plucker"]) and np.array_equal(a["keep"], b["keep"]) and a["summary"] == b["summary"]
