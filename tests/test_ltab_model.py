"""The line tables' checker (tests/ltab_np.py) against hand-derived lists and against geometry, and the no-device contract of
gfbe_ltab_create. CPU only."""
import ctypes as C

import numpy as np
import pytest

import line_np as ln
import ltab_np as lt
from _gfbe_import import gf

abi, synth_line = gf.abi, gf.synth_line
U = 2.0 ** -53


def _lists(tab):
    return [(l["id"], l["start"], len(l["obs"])) for l in tab.lines]


def _obs(lid, frame):
    return np.array([lid, frame, lid + 0.5, frame + 0.25], float)      # (recognisable: which line, which frame)


def test_hand_written_script_of_14_frames():
    """Fourteen frames through one list: the window fills (frames 0..10), then four slides — MARGIN_OLD with the shift, MARGIN_SECOND_NEW,
    MARGIN_OLD without the shift (removeBackline), MARGIN_OLD with the shift. The expected (id, start_frame, n_obs) lists were derived by
    hand from feature_manager.cpp:149-170, 896-911, 958-975, 1499-1527."""
    seen = [{1, 2}, {1, 2, 3}, {1, 3}, {1, 3}, {1, 3}, {1, 3, 4}, {1, 3, 4}, {1, 3}, {1, 3, 5}, {1, 3, 5}, {1, 3, 5, 6},
            {3, 6, 7}, {3, 6, 7, 8}, {3, 8}]
    counters = [[0, 2], [2, 1], [2, 0], [2, 0], [2, 0], [2, 1], [3, 0], [2, 0], [2, 1], [3, 0], [3, 1], [2, 1], [3, 1], [2, 0]]
    eye = np.concatenate([np.zeros(3), np.eye(3).ravel()])
    tab = lt.LineTable()
    after_add, after_slide = {}, {}
    fc = 0
    for g, ids in enumerate(seen):
        ids = sorted(ids)
        assert tab.add_frame(fc, ids, [_obs(i, g) for i in ids]) == counters[g], g
        after_add[g] = _lists(tab)
        if fc < lt.WINDOW_SIZE:
            fc += 1
            continue
        if g in (10, 13):
            tab.remove_back_shift(eye, eye)
        elif g == 11:
            tab.remove_front(fc)
        else:
            tab.remove_back()
        after_slide[g] = _lists(tab)
    assert after_add[4] == [(1, 0, 5), (2, 0, 2), (3, 1, 4)]
    assert after_add[10] == [(1, 0, 11), (2, 0, 2), (3, 1, 10), (4, 5, 2), (5, 8, 3), (6, 10, 1)]
    assert after_slide[10] == [(1, 0, 10), (3, 0, 10), (4, 4, 2), (5, 7, 3), (6, 9, 1)]                    # line 2: one observation left, < 2
    assert after_add[11] == [(1, 0, 10), (3, 0, 11), (4, 4, 2), (5, 7, 3), (6, 9, 2), (7, 10, 1)]
    assert after_slide[11] == [(1, 0, 9), (3, 0, 10), (4, 4, 2), (5, 7, 2), (6, 9, 1), (7, 9, 1)]          # line 4 ended before frame 9: untouched
    assert after_add[12] == [(1, 0, 9), (3, 0, 11), (4, 4, 2), (5, 7, 2), (6, 9, 2), (7, 9, 2), (8, 10, 1)]
    assert after_slide[12] == [(1, 0, 8), (3, 0, 10), (4, 3, 2), (5, 6, 2), (6, 8, 2), (7, 8, 2), (8, 9, 1)]
    assert after_add[13] == [(1, 0, 8), (3, 0, 11), (4, 3, 2), (5, 6, 2), (6, 8, 2), (7, 8, 2), (8, 9, 2)]
    assert after_slide[13] == [(1, 0, 7), (3, 0, 10), (4, 2, 2), (5, 5, 2), (6, 7, 2), (7, 7, 2), (8, 8, 2)]
    # which observations went: line 1 lost frame 0 (slide), frame 10 (second-new: its observation 9), frames 1 and 2 (slides); line 5 its third
    by_id = {l["id"]: l for l in tab.lines}
    assert [o[1] for o in by_id[1]["obs"]] == [3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]
    assert [o[1] for o in by_id[5]["obs"]] == [8.0, 9.0]
    assert [o[1] for o in by_id[6]["obs"]] == [11.0, 12.0]
    # the two erasure thresholds: removeBackline erases at 0 observations left, the shift at fewer than 2
    for n_obs, back, shift in ((1, [], []), (2, [(9, 0, 1)], []), (3, [(9, 0, 2)], [(9, 0, 2)])):
        for op, want in (("remove_back", back), ("remove_back_shift", shift)):
            t2 = lt.LineTable()
            for k in range(n_obs):
                t2.add_frame(0, [9], [_obs(9, k)])
            t2.remove_back() if op == "remove_back" else t2.remove_back_shift(eye, eye)
            assert _lists(t2) == want, (n_obs, op)


def _fill(stream, n=lt.NFRAMES, dtype=np.float64):
    tab = lt.LineTable(dtype)
    for g in range(n):
        ids, obs = stream.frame(g)
        tab.add_frame(g, ids, obs)
    pose7 = np.array([stream.pose7(g) for g in range(n)])
    return tab, pose7


def test_triangulated_lines_contain_the_true_segments():
    """Noise-free segments: every triangulated line has n . v = 0 and p x v = n for both true endpoints p (start camera frame).

    Sign and scale. pipi_plk(pi_i, pi_j) of the planes pi_i = (a, alpha), pi_j = (b, beta) is n = beta a - alpha b, v = b x a. A point p on
    both planes has a . p = -alpha, b . p = -beta, so p x v = b (p . a) - a (p . b) = beta a - alpha b = n: the convention is p x v = +n for
    every line, at the line's own (unnormalised) scale.

    Bound. The planes are formed from rounded inputs by a rotation product, a translation and two cross products; the partner's points
    are (R p + t) - t with |p| ~ 1 (a normalised image point) and |t| <= T, the camera's travel inside the window, so its normal b and
    offset beta carry relative errors of at most c (1 + T)^2 u against |b| and |b| (|x| + T), with c a small count of operations; take
    c = 64. Then |p x v - n| <= c (1 + T)^2 u |a| |b| (|p| + |x| + T) with x the nearest point of the line, while |n| = |v| d =
    |a| |b| sin(theta) d, d the distance of the line from the start camera and theta the angle between the planes. The gate
    min_cos_theta <= 0.998 guarantees sin(theta) >= sqrt(1 - 0.998^2) = 0.0632 (3.6 degrees), so, with |x| <= |p|,

        |p x v - n| / |n|  <=  64 (1 + T)^2 u (2 |p| + T) / (0.0632 d).

    n . v vanishes identically for ANY two planes (beta a . (b x a) = alpha b . (b x a) = 0); rounded: |n . v| <= 16 u A, A the absolute
    sum of the six products. Lines whose every partner is inside the gate stay untriangulated and keep a zero Plücker vector."""
    n_tri = n_gated = 0
    for seed in range(6):
        stream = synth_line.LineStream(seed=seed, noise=0.0)
        tab, pose7 = _fill(stream)
        pr = abi.pose_rows(pose7)
        tic_ric = abi.pose_rows(stream.ex_cam[None])[0]
        margins = {m[0]: m for m in tab.triangulate(pr, tic_ric)}
        Rwc = [pr[f, 3:].reshape(3, 3) @ tic_ric[3:].reshape(3, 3) for f in range(lt.NFRAMES)]
        twc = [pr[f, :3] + pr[f, 3:].reshape(3, 3) @ tic_ric[:3] for f in range(lt.NFRAMES)]
        T = max(np.linalg.norm(twc[f] - twc[0]) for f in range(lt.NFRAMES))
        for l in tab.lines:
            if l["id"] not in margins:
                assert not l["tri"] and not l["plk"].any()
                continue
            if not margins[l["id"]][3]:
                n_gated += 1
                assert not l["tri"] and not l["plk"].any()
                continue
            n_tri += 1
            n, v = l["plk"][:3], l["plk"][3:]
            assert abs(n @ v) <= 16 * U * (np.abs(n) @ np.abs(v))
            s = l["start"]
            for P in stream.endpoints(l["id"]):
                p = Rwc[s].T @ (P - twc[s])
                d = np.linalg.norm(np.cross(v, n)) / (v @ v)
                bound = 64 * (1 + T) ** 2 * U * (2 * np.linalg.norm(p) + T) / (0.0632 * d)
                assert np.linalg.norm(np.cross(p, v) - n) <= bound * np.linalg.norm(n), (seed, l["id"])
    assert n_tri >= 60 and n_gated >= 5, (n_tri, n_gated)


def test_shifted_line_projects_to_the_same_image_line():
    """remove_back_shift moves line_plucker from the removed frame 0 into the new one. Independent statement: two points of the unshifted
    line, carried into the new camera as points, span with the camera centre the plane whose normal is the shifted line's n."""
    stream = synth_line.LineStream(seed=11, noise=0.0)
    tab, pose7 = _fill(stream)
    pr, tic_ric = abi.pose_rows(pose7), abi.pose_rows(stream.ex_cam[None])[0]
    tab.triangulate(pr, tic_ric)
    before = {l["id"]: (l["plk"].copy(), l["start"]) for l in tab.lines if l["tri"] and l["start"] == 0 and len(l["obs"]) >= 3}
    assert len(before) >= 3
    c0, c1 = lt.cam_pr(pose7[0], stream.ex_cam), lt.cam_pr(pose7[1], stream.ex_cam)
    tab.remove_back_shift(c0, c1)
    R0, P0, R1, P1 = c0[3:].reshape(3, 3), c0[:3], c1[3:].reshape(3, 3), c1[:3]
    after = {l["id"]: l for l in tab.lines}
    for lid, (plk, _) in before.items():
        n, v = plk[:3], plk[3:]
        x = np.cross(v, n) / (v @ v)
        pts = [R1.T @ (R0 @ q + P0 - P1) for q in (x, x + v / np.linalg.norm(v))]
        want = np.cross(pts[0], pts[1])
        got = after[lid]["plk"][:3]
        assert after[lid]["start"] == 0
        assert np.linalg.norm(np.cross(want / np.linalg.norm(want), got / np.linalg.norm(got))) <= 1e-12
        assert (want @ got) > 0


def test_longdouble_and_float64_models_agree_within_the_absolute_sum():
    """The FP64 run of the checker against its own extended-precision run: every Plücker component within 64 u of its absolute sum
    (a plain FP64 evaluation of a sum of products). Measured: 4e-4 — the absolute sums are pessimistic: they carry the window positions
    (|P| ~ 10) through (R p + t) - t and two cross products, A ~ 1e4 |x|."""
    worst = 0.0
    for seed in (3, 4):
        stream = synth_line.LineStream(seed=seed)
        a, pose7 = _fill(stream)
        b, _ = _fill(stream, dtype=np.longdouble)
        pr, tic_ric = abi.pose_rows(pose7), abi.pose_rows(stream.ex_cam[None])[0]
        a.triangulate(pr, tic_ric)
        b.triangulate(pr, tic_ric)
        sa, sb = a.snapshot(), b.snapshot()
        np.testing.assert_array_equal(sa["is_triangulation"], sb["is_triangulation"])
        assert sa["is_triangulation"].sum() >= 10
        ratio = np.abs(sa["line_plucker"] - sb["line_plucker"]) / np.maximum(U * sb["plucker_abs"], 1e-300)
        ratio[sb["plucker_abs"] == 0] = 0.0
        worst = max(worst, float(ratio.max()))
    assert worst <= 64, worst


def test_create_without_device_reports_no_device():
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    lib.gfbe_create.restype = abi.c_i
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    lib.gfbe_ltab_create.restype = abi.c_i
    out = C.c_void_p(0xDEAD)
    assert lib.gfbe_ltab_create(ctx, 3, 64, C.byref(out)) == abi.NO_DEVICE
    assert not out.value
    with pytest.raises(RuntimeError):
        abi.LineTables(lib, "gfbe_", ctx, 1, 16)
    lib.gfbe_destroy(ctx)
