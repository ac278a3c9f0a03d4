"""The keyframe descriptors on the device (gfbe_kfd_*, include/gfbe_kfd.h) against the model (tests/kfd_np.py), bit for bit, on the cases
of tests/kfd_cases.py: the blurred plane, the score plane after suppression, the ordered lists, pts_norm and the descriptors; the corner
counts around the wave and the capacity; the plateau; corners on the frame's edge; three cameras of different images and calibrations in
one handle; describe on window points of every kind; the ring; capture from a tracker against push_image of the same bytes; the
hand-over to the loop database against gfbe_ldb_add_keyframe / gfbe_ldb_match fed with the downloaded lists; a second run of a whole
sequence; and the refusals. Nothing is a tolerance: every rule is integer arithmetic, one float addition with a truncation, or the
lift of gfbe_obs.h."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import kfd_cases as kc
import kfd_np as m
import ldb_cases as lc

pytestmark = pytest.mark.gpu
abi = gf.abi
F = np.float32
PAT = kc.pattern()
PLAIN, DIST = kc.CAMERAS["plain"], kc.CAMERAS["distorted"]


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


def _b32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same_camera(got, want, planes=None):
    assert got["counters"] == dict(zip(abi.KFD_COUNTERS, want["counters"].tolist()))
    assert np.array_equal(_b32(got["pts"]), _b32(want["pts"])) and np.array_equal(got["score"], want["score"])
    assert np.array_equal(_b32(got["pts_norm"]), _b32(want["pts_norm"])) and np.array_equal(got["desc"], want["desc"])
    if planes is not None:
        assert np.array_equal(planes["blurred"], want["blurred"]) and np.array_equal(planes["score"], want["plane"])


def _one(be, img, cam=PLAIN, **opt):
    """extract of a single camera: (lists, planes)."""
    rows, cols = img.shape
    d = be.describer(1, rows, cols, PAT, [cam], **opt)
    try:
        d.push_image(0, img[None])
        return d.extract(0)[0], d.planes(0, 0)
    finally:
        d.close()


@pytest.mark.parametrize("size", kc.SIZES + (kc.BIG,))
def test_extract_against_the_model(be, size):
    """7 x 7 (the single legal centre pixel, here a planted corner), 64 x 48, 97 x 61 (no size a multiple of a tile) and 640 x 480."""
    rows, cols = size
    if size == (7, 7):
        img, want = kc.planted(7, 7, 1), kc.expected_of(kc.planted(7, 7, 1), "distorted")
    else:
        img, want = kc.texture(rows, cols, 1), kc.expected(rows, cols, 1, "distorted")
    assert want["counters"][1] > 0
    got, planes = _one(be, img, DIST)
    _same_camera(got, want, planes)


@pytest.mark.parametrize("n", kc.PLANT_COUNTS)
def test_corner_counts(be, n):
    """0 (a flat image), 1, 63, 64, 65, exactly keypoint_capacity and capacity + 1 isolated corners: the overflow flag and the ordered truncation."""
    img = kc.planted(61, 97, n)
    want = kc.expected_of(img, cap=kc.PLANT_CAP)
    assert want["counters"].tolist() == [n, n, min(n, kc.PLANT_CAP), int(n > kc.PLANT_CAP)]
    got, planes = _one(be, img, keypoint_capacity=kc.PLANT_CAP)
    _same_camera(got, want, planes)


def test_plateau_and_edges(be):
    """Two equal adjacent scores: neither survives. Corners at x = 3, x = cols - 4, y = 3, y = rows - 4, whose pairs leave the image."""
    for img in (kc.plateau(), kc.edges()):
        want = kc.expected_of(img)
        got, planes = _one(be, img)
        _same_camera(got, want, planes)
    assert planes["score"][20, 3] == 109 and planes["score"][44, 60] == 59 and int((planes["score"] > 0).sum()) == 6


def test_thresholds(be):
    img = kc.texture(61, 97, 2)
    for t in (0, 60, 255):
        got, planes = _one(be, img, fast_threshold=t)
        _same_camera(got, kc.expected_of(img, t=t), planes)


def _three(be, **opt):
    imgs = np.stack([kc.texture(61, 97, 4), kc.planted(61, 97, 5), kc.texture(61, 97, 6)])
    cams = [PLAIN, DIST, DIST]
    return imgs, cams, be.describer(3, 61, 97, PAT, cams, **opt)


def test_three_cameras_in_one_handle(be):
    imgs, cams, d = _three(be)
    try:
        d.push_image(0, imgs)
        got = d.extract(0)
        for k in range(3):
            _same_camera(got[k], m.extract(imgs[k], PAT, cams[k]), d.planes(0, k))
        only = d.extract(0, outputs=False)
        assert [g["counters"] for g in only] == [g["counters"] for g in got] and only[0]["pts"] is None
    finally:
        d.close()


def test_describe(be):
    """Fractional, negative, edge, non-finite and huge window points; 0 and 1 points in a camera between two full cameras."""
    imgs, cams, d = _three(be, window_capacity=64)
    try:
        d.push_image(1, imgs)
        wp = kc.window_points(61, 97)
        rng = np.random.default_rng(3)
        full = np.concatenate([wp, (rng.uniform(0, 1, (40, 2)) * [97, 61]).astype(F)]).astype(F)
        for mid in (np.zeros((0, 2), F), wp[1:2]):
            lists = [full, mid, full[::-1].copy()]
            got = d.describe(1, lists)
            for k in range(3):
                desc, bad = m.brief(m.blur(imgs[k]), PAT, lists[k])
                assert np.array_equal(got[k]["desc"], desc) and (got[k]["points"], got[k]["zeroed"]) == (len(lists[k]), bad), k
        assert got[0]["zeroed"] == 6
        rc, _ = d.describe_raw(1, [full, np.zeros((65, 2), F), full])      # above window_capacity
        assert rc == abi.BAD_INPUT
    finally:
        d.close()


def test_ring(be):
    """Two slots filled in turn; the older slot extracted after the newer one was filled, and describe on either."""
    a, b = kc.texture(48, 64, 7), kc.texture(48, 64, 8)
    d = be.describer(1, 48, 64, PAT, [PLAIN], ring_slots=2)
    try:
        d.push_image(0, a[None])
        d.push_image(1, b[None])
        _same_camera(d.extract(0)[0], kc.expected(48, 64, 7), d.planes(0, 0))
        _same_camera(d.extract(1)[0], kc.expected(48, 64, 8), d.planes(1, 0))
        assert np.array_equal(d.planes(0, 0)["score"], kc.expected(48, 64, 7)["plane"])      # (a slot's planes are its own)
        d.push_image(0, b[None])      # refilled: the score plane of the slot is void until its next extract
        rc = d._f("download")(d.ctx, d.h, 0, 0, None, np.zeros((48, 64), np.uint8).ctypes.data_as(abi.PU8))
        assert rc == abi.BAD_INPUT
        assert np.array_equal(d.planes(0, 0, score=False)["blurred"], kc.expected(48, 64, 8)["blurred"])
        wp = kc.window_points(48, 64)
        assert np.array_equal(d.describe(1, [wp])[0]["desc"], m.brief(kc.expected(48, 64, 8)["blurred"], PAT, wp)[0])
    finally:
        d.close()


def test_capture_equals_push_image(be):
    """capture from a gfbe_klt handle after its push_image equals push_image of the same bytes into the describer, in every output; the
    keyframe's image is still in its slot two tracker pushes later (K6)."""
    imgs = np.stack([kc.texture(61, 97, 4), kc.texture(61, 97, 9)])
    later = np.stack([kc.texture(61, 97, 10), kc.texture(61, 97, 11)])
    cams = [DIST, PLAIN]
    t = be.tracker(2, 61, 97, 64)
    d = be.describer(2, 61, 97, PAT, cams)
    e = be.describer(2, 61, 97, PAT, cams)
    try:
        assert d.capture_raw(t, 0) == abi.BAD_INPUT      # no image has been pushed
        t.push_image(imgs)
        d.capture(t, 0)
        t.push_image(later)
        t.push_image(imgs[::-1].copy())
        e.push_image(2, imgs)
        got, ref = d.extract(0), e.extract(2)
        for k in range(2):
            want = m.extract(imgs[k], PAT, cams[k])
            _same_camera(got[k], want, d.planes(0, k))
            _same_camera(ref[k], want, e.planes(2, k))
        wp = kc.window_points(61, 97)
        a, b = d.describe(0, [wp, wp[:3]]), e.describe(2, [wp, wp[:3]])
        assert all(np.array_equal(x["desc"], y["desc"]) and x["zeroed"] == y["zeroed"] for x, y in zip(a, b))
    finally:
        e.close()
        d.close()
        t.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_step(got, want):
    assert got["index"] == want["index"] and got["loop_index"] == want["loop_index"], (got, want)
    assert np.array_equal(got["result_id"], want["result_id"]) and np.array_equal(_bits(got["result_score"]), _bits(want["result_score"]))


def _same_entries(a, b):
    assert a.size() == b.size()
    for e in range(a.size()["n_keyframes"]):
        x, y = a.entry(e), b.entry(e)
        assert np.array_equal(x["bow_word"], y["bow_word"]) and np.array_equal(_bits(x["bow_value"]), _bits(y["bow_value"]))
        for k in ("desc", "pts", "pts_norm"):
            assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), (e, k)


def _hand_over(be):
    """Six keyframes, a repeat of the first, then a keyframe that no longer fits: one database fed from the device, one from the host."""
    voc = lc.trees()["k10L3"]
    opt = dict(query_gap=3, min_loop_frame=3)
    seeds = [20, 21, 22, 23, 24, 25, 20, 26]
    wp = np.concatenate([kc.expected(48, 64, 20)["pts"] + F(0.25), kc.window_points(48, 64)]).astype(F)
    d = be.describer(2, 48, 64, PAT, [PLAIN, DIST])
    a, b = be.loop_database(voc, 7, 4096, **opt), be.loop_database(voc, 7, 4096, **opt)
    log = []
    try:
        for step, seed in enumerate(seeds):
            imgs = np.stack([kc.texture(48, 64, 99), kc.texture(48, 64, seed)])      # the keyframes are camera 1's
            d.push_image(step % 3, imgs)
            lists = d.extract(step % 3)[1]
            detect = step != 1      # (one add without a query)
            ga, gb = d.add_keyframe(1, a, detect), b.add_keyframe(lists["desc"], lists["pts"], lists["pts_norm"], detect)
            _same_step(ga, gb)
            log.append((ga["index"], ga["loop_index"], ga["result_id"].tolist(), _bits(ga["result_score"]).tolist(), lists["desc"].tobytes()))
            if step == 6:
                assert ga["loop_index"] == gb["loop_index"] == 0 and ga["index"] == 6      # the repeated image finds keyframe 0
                w = d.describe(step % 3, [wp[:5], wp])[1]["desc"]
                ma, mb = d.match(1, a, 0, len(wp)), b.match(0, w)
                for k in ("status", "best_index", "best_dist", "n_matched", "matched_src", "matched_pt", "matched_pt_norm"):
                    assert np.array_equal(ma[k], mb[k]), k
                assert ma["n_matched"] >= len(kc.expected(48, 64, 20)["pts"]) // 2
                log.append((ma["n_matched"], ma["best_index"].tolist(), ma["best_dist"].tolist()))
            if step == 7:
                assert ga["index"] == gb["index"] == -1      # the pool is full: refused on both
        _same_entries(a, b)
        assert a.size()["n_keyframes"] == 7 and a.size()["n_refused"] == 1
    finally:
        a.close()
        b.close()
        d.close()
    return log


def test_hand_over_to_the_loop_database(be):
    first = _hand_over(be)
    assert _hand_over(be) == first      # a second run of the whole sequence gives the same bits


def test_refusals(be):
    img = kc.texture(48, 64, 7)
    d = be.describer(1, 48, 64, PAT, [PLAIN], ring_slots=2, window_capacity=8)
    t = be.tracker(2, 48, 64, 16)
    t1 = be.tracker(1, 61, 97, 16)
    db = be.loop_database(lc.trees()["k3L2"], 4, 64)
    other = gf.Backend(device=0)
    lib, ctx = be.lib, be.ctx
    out = np.full(16, -7, np.int32)
    pi = out.ctypes.data_as(C.POINTER(C.c_int32))
    try:
        h = C.c_void_p(7)
        cams = np.ascontiguousarray(PLAIN)
        pd = cams.ctypes.data_as(C.POINTER(C.c_double))
        pp = np.ascontiguousarray(PAT).ctypes.data_as(C.POINTER(C.c_int32))
        for kw in (dict(ring_slots=0), dict(ring_slots=9), dict(fast_threshold=256), dict(keypoint_capacity=4097), dict(window_capacity=0), dict(struct_size=16)):
            assert lib.gfbe_kfd_create(ctx, 1, 48, 64, pp, pd, C.byref(abi.kfd_default_options(lib, **kw)), C.byref(h)) == abi.BAD_INPUT and not h.value, kw
        assert lib.gfbe_kfd_create(ctx, 1, 6, 64, pp, pd, None, C.byref(h)) == abi.BAD_INPUT and not h.value
        bad = np.ascontiguousarray(PAT.copy())
        bad[0, 0] = 65
        assert lib.gfbe_kfd_create(ctx, 1, 48, 64, bad.ctypes.data_as(C.POINTER(C.c_int32)), pd, None, C.byref(h)) == abi.BAD_INPUT and not h.value
        # a slot never filled, a bad slot, a bad camera
        assert d.extract_raw(0)[0] == abi.BAD_INPUT and d.describe_raw(0, [np.zeros((1, 2), F)])[0] == abi.BAD_INPUT
        assert d.push_image_raw(2, img[None]) == abi.BAD_INPUT and d.push_image_raw(-1, img[None]) == abi.BAD_INPUT
        assert d.capture_raw(t, 0) == abi.BAD_INPUT and d.capture_raw(t1, 0) == abi.BAD_INPUT      # mismatching trackers
        d.push_image(0, img[None])
        assert d.extract_raw(1)[0] == abi.BAD_INPUT
        # add_keyframe / match before an extract / describe
        assert d.add_keyframe_raw(0, db)[0] == abi.BAD_INPUT and d.match_raw(0, db, 0, 0)[0] == abi.BAD_INPUT
        assert db.size()["n_keyframes"] == 0
        got = d.extract(0)[0]
        assert d.add_keyframe_raw(1, db)[0] == abi.BAD_INPUT and d.add_keyframe_raw(-1, db)[0] == abi.BAD_INPUT
        assert d.match_raw(0, db, 0, 0)[0] == abi.BAD_INPUT      # still no describe
        assert d.describe_raw(0, [np.zeros((9, 2), F)])[0] == abi.BAD_INPUT      # above window_capacity
        d.describe(0, [got["pts"][:4]])
        assert d.match_raw(0, db, 0, 4)[0] == abi.BAD_INPUT      # old_index is not a held keyframe
        assert d.add_keyframe(0, db)["index"] == 0
        assert d.match(0, db, 0, 4)["n_matched"] == 4
        assert lib.gfbe_kfd_download(ctx, d.h, 0, 1, None, None) == abi.BAD_INPUT and lib.gfbe_kfd_download(ctx, d.h, 1, 0, None, None) == abi.BAD_INPUT
        # a handle of another context
        assert other.lib.gfbe_kfd_extract(other.ctx, d.h, 0, None, None, None, None, None, pi) == abi.BAD_INPUT and (out == -7).all()
    finally:
        other.close()
        db.close()
        t1.close()
        t.close()
        d.close()
