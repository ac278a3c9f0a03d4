"""Corner detection on the device (gfbe_det_*, include/gfbe_det.h) against the model (tests/det_np.py), bit for bit, on the cases of
tests/det_cases.py: the response plane and the applied mask, the mask-free corners with their responses, detect with its four arrays,
offsets and counters over the frames of a case; the hand-over (a track after detect gives the bits it gives after set_points with the
model's lists); the same bits alone and after a larger handle; the refusals with their outputs untouched. Float results are compared
as bit patterns."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import det_cases as dc
import det_np as m

pytestmark = pytest.mark.gpu
abi = gf.abi
PF, PI, PU8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


class Pair:
    """A tracker with the case's first image and held points, and its detector."""

    def __init__(self, be, c, **options):
        self.t = be.tracker(len(c["pts"]), c["rows"], c["cols"], c["capacity"])
        try:
            self.t.push_image(c["images"][0])
            self.t.set_points(c["pts"], c["ids"], c["cnt"])
            self.d = be.detector(self.t, **dict(c["options"], **options))
            self.d.set_next_id(c["next_id"])
        except Exception:
            self.t.close()
            raise

    def close(self):
        if getattr(self, "d", None) is not None:
            self.d.close()
        self.t.close()


def _same_detect(got, want, where):
    for k, (g, w) in enumerate(zip(got, want)):
        assert list(g["counters"].values()) == w["counters"].tolist(), (where, k, g["counters"], w["counters"])
        assert np.array_equal(_bits(g["pts"]), _bits(w["pts"])), (where, k)
        assert np.array_equal(g["ids"], w["ids"]) and np.array_equal(g["track_cnt"], w["track_cnt"]), (where, k)


@pytest.mark.parametrize("name", dc.NAMES)
def test_detect_planes_and_corners_are_the_models(be, name):
    c, want, wc = dc.case(name), dc.expected(name), dc.expected_corners(name)
    p = Pair(be, c)
    try:
        for k in range(len(c["pts"])):      # before the first detect: the mask is clear
            got = p.d.planes(k)
            assert np.array_equal(_bits(got["eig"]), _bits(want[0][k]["eig"])) and (got["mask"] == 255).all(), k
        mc, q, md = c["corners"]
        for g, w in zip(p.d.corners(mc, q, md), wc):
            assert np.array_equal(_bits(g["pts"]), _bits(w["pts"])) and np.array_equal(_bits(g["response"]), _bits(w["response"]))
        assert p.t.held == [len(x) for x in c["pts"]]      # corners left the held points alone
        for f, per_cam in enumerate(want):
            if f:
                p.t.push_image(c["images"][f])
            _same_detect(p.d.detect(), per_cam, (name, f))
            assert p.t.held == [len(w["ids"]) for w in per_cam]
            for k, w in enumerate(per_cam):
                got = p.d.planes(k)
                assert np.array_equal(_bits(got["eig"]), _bits(w["eig"])) and np.array_equal(got["mask"], w["mask"]), (f, k)
    finally:
        p.close()


@pytest.mark.parametrize("name", ["s64x48_three_cameras", "two_frames", "s91x89_min_dist_30"])
def test_a_track_after_detect_is_a_track_after_set_points(be, name):
    """The hand-over: after detect the tracker is in the state gfbe_klt_set_points with the model's lists leaves it in."""
    c, want = dc.case(name), dc.expected(name)[0]
    nxt = np.ascontiguousarray(np.roll(c["images"][0], 1, axis=2))      # the scene moved by one pixel: most points track
    p = Pair(be, c)
    t2 = be.tracker(len(c["pts"]), c["rows"], c["cols"], c["capacity"])
    try:
        p.d.detect()
        p.t.push_image(nxt)
        a = p.t.track()
        t2.push_image(c["images"][0])
        t2.set_points([w["pts"] for w in want], [w["ids"] for w in want], [w["track_cnt"] for w in want])
        t2.push_image(nxt)
        b = t2.track()
        assert sum(len(x["ids"]) for x in b) > 0
        for x, y in zip(a, b):
            assert x["counters"] == y["counters"]
            assert all(np.array_equal(np.ascontiguousarray(x[k]).view(np.uint8), np.ascontiguousarray(y[k]).view(np.uint8)) for k in ("prev_pts", "cur_pts", "ids", "track_cnt"))
        # and a second detect on the survivors runs on the same state
        d2 = be.detector(t2, **c["options"])
        try:
            d2.set_next_id([w["next_id"] for w in want])
            _same_detect(d2.detect(), [dict(pts=g["pts"], ids=g["ids"], track_cnt=g["track_cnt"], counters=np.array(list(g["counters"].values()))) for g in p.d.detect()], name)
        finally:
            d2.close()
    finally:
        t2.close()
        p.close()


def test_same_bits_alone_and_after_a_larger_handle(be):
    """A handle's results depend on nothing a larger handle left behind (allocations are reused by the runtime)."""
    small, big = dc.case("s64x48_three_cameras"), dc.case("noise_default_chunk")

    def run():
        p = Pair(be, small)
        try:
            return p.d.corners(*small["corners"]), p.d.detect(), [p.d.planes(k) for k in range(3)]
        finally:
            p.close()
    first = run()
    pb = Pair(be, big)
    pb.d.detect()
    pb.close()
    second = run()
    for a, b in zip(first[0], second[0]):
        assert np.array_equal(_bits(a["pts"]), _bits(b["pts"])) and np.array_equal(_bits(a["response"]), _bits(b["response"]))
    for a, b in zip(first[2], second[2]):
        assert np.array_equal(_bits(a["eig"]), _bits(b["eig"])) and np.array_equal(a["mask"], b["mask"])
    _same_detect(second[1], dc.expected("s64x48_three_cameras")[0], "after")
    _same_detect(first[1], dc.expected("s64x48_three_cameras")[0], "alone")


def test_refusals_leave_the_outputs_untouched(be):
    c = dc.case("s64x48_three_cameras")
    lib, ctx = be.lib, be.ctx
    t = be.tracker(3, c["rows"], c["cols"], c["capacity"])
    wide = be.tracker(1, 48, 64, abi.DET_MAX_POINTS + 1)
    try:
        h = C.c_void_p()
        for kw in (dict(struct_size=24), dict(max_cnt=c["capacity"] + 1), dict(max_cnt=0), dict(min_dist=-1), dict(sort_chunk=100), dict(quality=-1.0), dict(candidate_capacity=-1)):
            assert lib.gfbe_det_create(ctx, t.h, C.byref(abi.det_default_options(lib, **dict(dict(max_cnt=40), **kw))), C.byref(h)) == abi.BAD_INPUT and not h.value, kw
        assert lib.gfbe_det_create(ctx, wide.h, C.byref(abi.det_default_options(lib, max_cnt=40)), C.byref(h)) == abi.BAD_INPUT and not h.value
        assert b"GFBE_DET_MAX_POINTS" in lib.gfbe_last_error(ctx)
        assert lib.gfbe_det_create(ctx, None, None, C.byref(h)) == abi.BAD_INPUT and not h.value
        d = be.detector(t, **c["options"])
        try:
            # no image yet: everything is refused
            rc, raw = d.detect_raw()
            assert rc == abi.BAD_INPUT and all((v == -7).all() for v in raw.values()) and b"no image" in lib.gfbe_last_error(ctx)
            rc, raw = d.corners_raw(10)
            assert rc == abi.BAD_INPUT and all((v == -7).all() for v in raw.values())
            eig = np.full((c["rows"], c["cols"]), -7, np.float32)
            assert lib.gfbe_det_download(ctx, d.h, 0, eig.ctypes.data_as(PF), None) == abi.BAD_INPUT and (eig == -7).all()
            t.push_image(c["images"][0])
            t.set_points(c["pts"], c["ids"], c["cnt"])
            for mc in (0, -3, abi.DET_MAX_POINTS + 1):
                rc, raw = d.corners_raw(mc)
                assert rc == abi.BAD_INPUT and all((v == -7).all() for v in raw.values()), mc
            for q, md in ((-0.5, 10), (float("nan"), 10), (0.01, -1)):
                rc, raw = d.corners_raw(10, q, md)
                assert rc == abi.BAD_INPUT and all((v == -7).all() for v in raw.values()), (q, md)
            assert lib.gfbe_det_download(ctx, d.h, 3, eig.ctypes.data_as(PF), None) == abi.BAD_INPUT and (eig == -7).all()
            assert lib.gfbe_det_download(ctx, d.h, -1, eig.ctypes.data_as(PF), None) == abi.BAD_INPUT and (eig == -7).all()
            assert lib.gfbe_det_set_next_id(ctx, d.h, None) == abi.BAD_INPUT
            other = gf.Backend(device=0)
            try:
                out = np.full(8, -7, np.int32)
                assert other.lib.gfbe_det_detect(other.ctx, d.h, out.ctypes.data_as(PI), None, None, None, None) == abi.BAD_INPUT and (out == -7).all()      # another context's handle
                assert other.lib.gfbe_det_create(other.ctx, t.h, None, C.byref(h)) == abi.BAD_INPUT and not h.value
            finally:
                other.close()
            assert t.held == [len(x) for x in c["pts"]]
            _same_detect(d.detect(), dc.expected("s64x48_three_cameras")[0], "after the refusals")      # nothing was disturbed
        finally:
            d.close()
    finally:
        wide.close()
        t.close()
