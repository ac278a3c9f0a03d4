"""The optical-flow tracker on the device (gfbe_klt_*, include/gfbe_klt.h) against the model (tests/klt_np.py), bit for bit, on the
cases of tests/klt_cases.py: every level of both image sets, calcOpticalFlowPyrLK in both directions with and without an initial
flow at max_level 0, 1 and 3, and the tracking half of trackImage with its offsets and counters; the same bits alone and after a
larger handle; the refusals with their outputs untouched. Float results are compared as bit patterns."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import klt_cases as kc
import klt_np as m

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


def _tracker(be, c, pushes=2, capacity=None):
    t = be.tracker(len(c["pts"]), c["rows"], c["cols"], capacity or c["capacity"], **c["options"])
    t.push_image(c["images"][0])
    t.set_points(c["pts"], c["ids"], c["cnt"])
    for k in range(1, pushes):
        t.push_image(c["images"][k])
    return t


def _same_track(got, want, where):
    for k, (g, w) in enumerate(zip(got, want)):
        assert list(g["counters"].values()) == w["counters"].tolist(), (where, k)
        assert np.array_equal(_bits(g["prev_pts"]), _bits(w["prev_pts"])) and np.array_equal(_bits(g["cur_pts"]), _bits(w["cur_pts"])), (where, k)
        assert np.array_equal(g["ids"], w["ids"]) and np.array_equal(g["track_cnt"], w["track_cnt"]), (where, k)


@pytest.mark.parametrize("name", kc.NAMES)
def test_levels_of_both_sets_are_the_models(be, name):
    c, pyr = kc.case(name), kc.pyramids(name)
    t = _tracker(be, c)
    try:
        for which in (0, 1):
            for k in range(len(c["pts"])):
                for l, L in enumerate(pyr[which][k]):
                    got = t.level(which, k, l)
                    assert (got["w"], got["h"], got["n_levels"]) == (L["w"], L["h"], len(pyr[which][k]))
                    assert np.array_equal(got["image"], L["img"]) and np.array_equal(got["deriv"], L["der"]), (which, k, l)
    finally:
        t.close()


@pytest.mark.parametrize("name", kc.NAMES)
def test_flow_is_the_models(be, name):
    c, want = kc.case(name), kc.expected_flows(name)
    t = _tracker(be, c)
    try:
        for (d, ml, init), per_cam in want.items():
            got = t.flow(c["pts"], direction=d, max_level=ml, next_pts=[kc.initial_flow(c, k) for k in range(len(c["pts"]))] if init else None)
            for k, (g, w) in enumerate(zip(got, per_cam)):
                assert np.array_equal(g["status"], w["status"]), (d, ml, init, k)
                assert np.array_equal(_bits(g["next_pts"]), _bits(w["next_pts"])) and np.array_equal(_bits(g["err"]), _bits(w["err"])), (d, ml, init, k)
    finally:
        t.close()


@pytest.mark.parametrize("name", kc.NAMES)
def test_track_is_the_models(be, name):
    c, want = kc.case(name), kc.expected_tracks(name)
    t = _tracker(be, c)
    try:
        for step, per_cam in enumerate(want):
            if step:
                t.push_image(c["images"][step + 1])
            _same_track(t.track(c["predict"][step] if step == 0 else None), per_cam, (name, step))
            assert t.held == [len(w["ids"]) for w in per_cam]
    finally:
        t.close()


def test_same_bits_alone_and_after_a_larger_handle(be):
    """A handle's results depend on nothing a larger handle left behind (allocations are reused by the runtime)."""
    small, big = kc.case("s64x48_two_levels"), kc.case("s180x177_four_levels")

    def run():
        t = _tracker(be, small)
        try:
            lv = [t.level(w, 2, l) for w in (0, 1) for l in (0, 1)]
            fl = t.flow(small["pts"], direction=0, max_level=3)
            return lv, fl, t.track()
        finally:
            t.close()
    first = run()
    tb = _tracker(be, big, capacity=512)
    tb.track()
    tb.close()
    second = run()
    for a, b in zip(first[0], second[0]):
        assert np.array_equal(a["image"], b["image"]) and np.array_equal(a["deriv"], b["deriv"])
    for a, b in zip(first[1], second[1]):
        assert all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in ("next_pts", "status", "err"))
    _same_track(second[2], kc.expected_tracks("s64x48_two_levels")[0], "after")
    _same_track(first[2], kc.expected_tracks("s64x48_two_levels")[0], "alone")


def test_refusals_leave_the_outputs_untouched(be):
    c = kc.case("s64x48_two_levels")
    lib, ctx = be.lib, be.ctx
    h = C.c_void_p()
    assert lib.gfbe_klt_create(ctx, 1, 21, 64, 8, None, C.byref(h)) == abi.BAD_INPUT and not h.value
    assert lib.gfbe_klt_create(ctx, 1, 48, 64, 8, C.byref(abi.klt_default_options(lib, struct_size=48)), C.byref(h)) == abi.BAD_INPUT and not h.value
    t = be.tracker(3, c["rows"], c["cols"], 65)
    try:
        t.push_image(c["images"][0])
        t.set_points(c["pts"], c["ids"], c["cnt"])
        # one image only: track, flow and the previous set are refused
        rc, raw = t.track_raw()
        assert rc == abi.BAD_INPUT and all((v == -7).all() for v in raw.values()) and b"two images" in lib.gfbe_last_error(ctx)
        rc, out = t.flow_raw(c["pts"])
        assert rc == abi.BAD_INPUT and all((o["next_pts"] == -7).all() and (o["status"] == 249).all() and (o["err"] == -7).all() for o in out)
        dims = np.full(4, -7, np.int32)
        assert lib.gfbe_klt_download_level(ctx, t.h, 0, 0, 0, None, None, dims.ctypes.data_as(PI)) == abi.BAD_INPUT and (dims == -7).all()
        t.push_image(c["images"][1])
        assert lib.gfbe_klt_download_level(ctx, t.h, 1, 0, 2, None, None, dims.ctypes.data_as(PI)) == abi.BAD_INPUT and (dims == -7).all()      # a level that was not built
        assert lib.gfbe_klt_download_level(ctx, t.h, 1, 3, 0, None, None, dims.ctypes.data_as(PI)) == abi.BAD_INPUT and (dims == -7).all()
        # a count above the capacity, offsets that do not start at 0, a non-finite point: the held points stay as they were
        many = [np.zeros((66, 2), np.float32) + 20, c["pts"][1], c["pts"][2]]
        assert t.set_points_raw(many, [np.arange(66), c["ids"][1], c["ids"][2]], [np.ones(66), c["cnt"][1], c["cnt"][2]]) == abi.BAD_INPUT
        for bad in (np.nan, np.inf, -np.inf):
            p = [x.copy() for x in c["pts"]]
            p[2][7, 1] = bad
            assert t.set_points_raw(p, c["ids"], c["cnt"]) == abi.BAD_INPUT and b"non-finite" in lib.gfbe_last_error(ctx)
            rc, out = t.flow_raw(p)
            assert rc == abi.BAD_INPUT and all((o["next_pts"] == -7).all() and (o["err"] == -7).all() for o in out)
            nx = [x.copy() for x in c["pts"]]
            nx[0][3, 0] = bad
            keep = [x.copy() for x in nx]
            rc, out = t.flow_raw(c["pts"], next_pts=nx)
            assert rc == abi.BAD_INPUT and all(np.array_equal(o["next_pts"], k_, equal_nan=True) and (o["err"] == -7).all() for o, k_ in zip(out, keep))
            rc, raw = t.track_raw(predict=[p[0], None, p[2]])
            assert rc == abi.BAD_INPUT and all((v == -7).all() for v in raw.values())
        rc, out = t.flow_raw(many)
        assert rc == abi.BAD_INPUT
        assert lib.gfbe_klt_flow(ctx, t.h, 2, 3, 0, None, None, None, None, None) == abi.BAD_INPUT and lib.gfbe_klt_flow(ctx, t.h, 0, 8, 0, None, None, None, None, None) == abi.BAD_INPUT
        assert t.held == [63, 0, 65]
        _same_track(t.track(), kc.expected_tracks("s64x48_two_levels")[0], "after the refusals")      # nothing was disturbed
    finally:
        t.close()
    other = gf.Backend(device=0)
    try:
        t2 = be.tracker(1, 48, 64, 8)
        assert other.lib.gfbe_klt_push_image(other.ctx, t2.h, c["images"][0][0].ctypes.data_as(PU8)) == abi.BAD_INPUT      # another context's handle
        t2.close()
    finally:
        other.close()
