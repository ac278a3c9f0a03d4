"""The loop verification on the device (gfbe_pnp_*, include/gfbe_pnp.h) against the model (tests/pnp_np.py) on the cases of
tests/pnp_cases.py, whose case condition tests/test_pnp_model.py checks on the CPU: every output equals the model with np.array_equal,
double bits included; relative_yaw alone has a tolerance, pnp_cases.YAW_ATOL = 1e-12 degrees (two atan2 at 2 ulp, the degree conversion and
one subtraction stay under 8 ulp of 180 = 2.3e-13; the decade above). Then: the same bits alone and after a larger handle lived on the
context; find_connection and find_connection_kfd against gfbe_ldb_match / gfbe_kfd_match, a host gather and gfbe_pnp_verify; and the
refusals. The non-positive pivot of V6 is tested on the solver in test_pnp_model.py only: no problem was found that triggers it."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import kfd_cases as kc
import ldb_cases as lc
import pnp_cases as pc
import pnp_np as m

pytestmark = pytest.mark.gpu
abi = gf.abi
F = np.float32
PI, PD, PF = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)
KEYS = ("status", "n_inliers", "has_loop", "loop_info", "pnp_pose", "best", "refine_flag")
DIAG = ("sample_idx", "n_solutions", "hyp_pose", "hyp_count")


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


def _run(be, name, diagnostics=True):
    kw, problems = pc.CASES[name]
    v = be.loop_verifier(**kw)
    try:
        return v.verify(*pc.pack(problems), diagnostics=diagnostics)
    finally:
        v.close()


def _bytes(r, keys):
    return [np.ascontiguousarray(r[k]).tobytes() for k in keys]


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_cases_against_the_model(be, name):
    """n = 25 (no PnP); 26, 63, 64 and 65 inliers (the lane-stride edges of V6); n = max_points of a small handle and of the default one
    (4096: eight tiles of k_pnp_score, the whole inlier list of k_pnp_finish); 513 and 1025 points (one past a tile); B = 1 and 4 with an empty problem; one
    hypothesis; no refinement; all outliers; ties; a collinear sample; yaw and translation beyond their limits, and within wider ones:
    every output and the diagnostics sample_idx / n_solutions / hyp_pose / hyp_count."""
    got = _run(be, name)
    pc.assert_equals_model(got, pc.pack(pc.CASES[name][1])[0], pc.expected(name))
    assert (got["hyp_pose"][got["n_solutions"][..., None] <= np.arange(4)] == 0).all()      # the rows beyond n_solutions are zero


def test_outputs_may_be_null(be):
    want = _run(be, "batch3")
    assert _bytes(_run(be, "batch3", diagnostics=False), KEYS) == _bytes(want, KEYS)
    kw, problems = pc.CASES["batch3"]
    off, p3, pn, pcur, tq = pc.pack(problems)
    v = be.loop_verifier(**kw)
    try:
        has = np.full(4, -7, np.int32)
        args = [off.ctypes.data_as(PI), p3.ctypes.data_as(PF), pn.ctypes.data_as(PF), pcur.ctypes.data_as(PD), tq.ctypes.data_as(PD)]
        assert be.lib.gfbe_pnp_verify(be.ctx, v.h, 4, *args, None, None, has.ctypes.data_as(PI), *([None] * 8)) == abi.OK
        assert np.array_equal(has, want["has_loop"])
        assert be.lib.gfbe_pnp_verify(be.ctx, v.h, 0, *([None] * 16)) == abi.OK
    finally:
        v.close()


def test_same_bits_alone_and_after_a_larger_handle(be):
    """Nothing depends on what an allocation held before: a case alone, then after a handle of 1024 hypotheses ran bigger problems and was
    destroyed, then twice on one handle after another case."""
    alone = _bytes(_run(be, "in65"), KEYS + DIAG)
    big = be.loop_verifier(iterations=1024, max_problems=8)
    try:
        big.verify(*pc.pack(pc.CASES["batch3"][1]), diagnostics=True)
    finally:
        big.close()
    assert _bytes(_run(be, "in65"), KEYS + DIAG) == alone
    v = be.loop_verifier()
    try:
        v.verify(*pc.pack(pc.CASES["batch3"][1]), diagnostics=True)
        a = v.verify(*pc.pack(pc.CASES["in65"][1]), diagnostics=True)
        v.verify(*pc.pack(pc.CASES["outliers"][1]))
        b = v.verify(*pc.pack(pc.CASES["in65"][1]), diagnostics=True)
        assert _bytes(a, KEYS + DIAG) == _bytes(b, KEYS + DIAG) == alone
    finally:
        v.close()


def _scene(be, rows, cols, seed, extra):
    """A keyframe of one camera held by a describer and a loop database, window points on its own corners plus `extra` others, and world
    points planted behind the corners' keypoints_norm: (describer, database, window points, point_3d, frame, corners)"""
    img = kc.texture(rows, cols, seed)
    d = be.describer(1, rows, cols, kc.pattern(), [kc.CAMERAS["plain"]], window_capacity=512)
    db = be.loop_database(lc.trees()["k10L3"], 4, 4096)
    d.push_image(0, img[None])
    lists = d.extract(0)[0]
    assert d.add_keyframe(0, db, False)["index"] == 0
    rng = np.random.default_rng(seed)
    f = pc.frame(rng)
    n = len(lists["pts"])
    wp = np.concatenate([lists["pts"], np.stack([rng.uniform(8, cols - 8, extra), rng.uniform(8, rows - 8, extra)], 1).astype(F)]).astype(F)
    depth = rng.uniform(2.0, 8.0, n)
    Xc = np.concatenate([lists["pts_norm"].astype(np.float64) * depth[:, None], depth[:, None]], 1)
    p3 = np.concatenate([Xc @ f["R_wc"].T + f["t_wc"], rng.uniform(-5, 5, (extra, 3))]).astype(F)
    return d, db, wp, p3, f, n


@pytest.mark.parametrize("rows, cols, seed, extra, loop", [(120, 160, 1, 12, 1), (48, 64, 20, 6, 0)])
def test_find_connection_against_match_gather_verify(be, rows, cols, seed, extra, loop):
    """One wait against two: the chain on the device equals gfbe_ldb_match / gfbe_kfd_match, a host gather by matched_src and
    gfbe_pnp_verify, in the match lists and in every bit of V7 / V8; 184 corners (a loop) and 16 corners (25 or fewer matches: no PnP)."""
    d, db, wp, p3, f, n_corners = _scene(be, rows, cols, seed, extra)
    v = be.loop_verifier()
    try:
        wdesc = d.describe(0, [wp])[0]["desc"]
        ma, mk = db.match(0, wdesc), d.match(0, db, 0, len(wp))
        nm = ma["n_matched"]
        assert nm >= n_corners and (nm > 25) == bool(loop)
        ref = v.verify([0, nm], p3[ma["matched_src"]], ma["matched_pt_norm"], f["pose_cur"], f["tic_qic"])
        a = v.find_connection(db, 0, wdesc, p3, f["pose_cur"], f["tic_qic"])
        b = v.find_connection_kfd(d, 0, db, 0, len(wp), p3, f["pose_cur"], f["tic_qic"])
        for got in (a, b):
            for k in ("n_matched", "matched_src", "matched_pt", "matched_pt_norm"):
                assert np.array_equal(got[k], ma[k]) and np.array_equal(got[k], mk[k]), k
            assert np.array_equal(got["status_pnp"], ref["status"])
            for k in KEYS[1:]:
                assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(ref[k][0]).tobytes(), k
            for k in ("matched_src", "matched_pt", "matched_pt_norm", "status_pnp"):      # nothing is written behind n_matched
                assert (got["raw"][k][nm:] == (-7 % 256 if k == "status_pnp" else -7)).all(), k
        # the matches exist only now: their case condition is checked here, before anything is compared with the model
        ok, want, why = pc.condition(m.options(), dict(point_3d=p3[ma["matched_src"]], pt_norm=ma["matched_pt_norm"], pose_cur=f["pose_cur"], tic_qic=f["tic_qic"]))
        assert ok, why
        assert a["has_loop"] == want["has_loop"] == loop and a["n_inliers"] == want["n_inliers"] and np.array_equal(a["status_pnp"], want["status"])
        if loop:
            assert a["n_inliers"] > 0.8 * n_corners and np.abs(a["pnp_pose"] - np.concatenate([f["T_wi"], f["R_wi"].ravel()])).max() < 1e-5
        else:
            assert not a["loop_info"].any() and not a["pnp_pose"].any() and a["best"].tolist() == [-1, -1]
        # an empty window
        e = v.find_connection(db, 0, np.zeros((0, 4), np.uint64), np.zeros((0, 3), F), f["pose_cur"], f["tic_qic"])
        assert (e["n_matched"], e["has_loop"], e["n_inliers"]) == (0, 0, 0)
    finally:
        v.close()
        d.close()
        db.close()


def test_bad_arguments_leave_the_handle_unchanged(be):
    kw, problems = pc.CASES["in26"]
    off, p3, pn, pcur, tq = pc.pack(problems)
    d, db, wp, w3, f, _ = _scene(be, 48, 64, 20, 4)
    other = gf.Backend(device=0)
    v = be.loop_verifier(max_problems=2, max_points=64)
    try:
        untouched = lambda r: all((np.asarray(r[k]) == (-7 % 256 if k == "status" else -7)).all() for k in KEYS)
        for args in (([0, 10, 5], p3[:10], pn[:10], np.stack([pcur[0]] * 2), np.stack([tq[0]] * 2)),      # offsets descend
                     ([1, 11], p3[:11], pn[:11], pcur, tq),                                              # not from 0
                     ([0, 65], np.zeros((65, 3), F), np.zeros((65, 2), F), pcur, tq),                    # above max_points
                     ([0, 1, 2, 3], p3[:3], pn[:3], np.stack([pcur[0]] * 3), np.stack([tq[0]] * 3))):    # above max_problems
            rc, r = v.verify_raw(*args)
            assert rc == abi.BAD_INPUT and untouched(r), args[0]
        out = np.full(4, -7, np.int32)
        assert be.lib.gfbe_pnp_verify(be.ctx, v.h, 1, off.ctypes.data_as(PI), None, None, pcur.ctypes.data_as(PD), tq.ctypes.data_as(PD), None, out.ctypes.data_as(PI),
                                      *([None] * 9)) == abi.BAD_INPUT and (out == -7).all()
        assert be.lib.gfbe_pnp_verify(other.ctx, v.h, 1, off.ctypes.data_as(PI), p3.ctypes.data_as(PF), pn.ctypes.data_as(PF), pcur.ctypes.data_as(PD), tq.ctypes.data_as(PD),
                                      None, out.ctypes.data_as(PI), *([None] * 9)) == abi.BAD_INPUT and (out == -7).all()
        wdesc = d.describe(0, [wp])[0]["desc"]
        gone = lambda r: r["n_matched"] == -7 and (r["raw"]["matched_src"] == -7).all() and r["n_inliers"] == -7 and (r["loop_info"] == -7).all()
        for rc, r in (v.find_connection_raw(db, 1, wdesc, w3, f["pose_cur"], f["tic_qic"]),                                             # no such keyframe
                      v.find_connection_raw(db, 0, np.zeros((65, 4), np.uint64), np.zeros((65, 3), F), f["pose_cur"], f["tic_qic"]),      # above max_points
                      v.find_connection_kfd_raw(d, 1, db, 0, len(wp), w3, f["pose_cur"], f["tic_qic"]),                                  # no such camera
                      v.find_connection_kfd_raw(d, 0, db, -1, len(wp), w3, f["pose_cur"], f["tic_qic"])):
            assert rc == abi.BAD_INPUT and gone(r)
        fresh = be.describer(1, 48, 64, kc.pattern(), [kc.CAMERAS["plain"]])
        try:
            assert v.find_connection_kfd_raw(fresh, 0, db, 0, 0, np.zeros((0, 3), F), f["pose_cur"], f["tic_qic"])[0] == abi.BAD_INPUT      # nothing described
        finally:
            fresh.close()
        # the handle still works, and gives the model's bits
        pc.assert_equals_model(v.verify(off, p3, pn, pcur, tq, diagnostics=True), off, pc.expected("in26"))
        assert v.find_connection(db, 0, wdesc, w3, f["pose_cur"], f["tic_qic"])["n_matched"] >= 16
    finally:
        v.close()
        d.close()
        db.close()
        other.close()
