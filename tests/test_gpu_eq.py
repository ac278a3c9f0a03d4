"""The image equalisation on the device (gfbe_eq_*, include/gfbe_eq.h) against the model (tests/eq_np.py), bit for bit, on the cases of
tests/eq_cases.py with 1, 3 and 65 cameras: apply and the LUTs, out of place and in place; push_klt against a second tracker fed by
gfbe_klt_push_image with the model's equalised images, every built level, image and derivative, and a track on both; push_klt and
gfbe_klt_push_image interleaved on one tracker; two push_klt calls back to back without a wait between them; push_kfd against the blur
of the model's equalised image, and gfbe_kfd_capture from an equalised tracker; and the refusals on a live device. Nothing is a
tolerance: everything up to the LUT is integer arithmetic, E5 is IEEE single precision in a fixed order."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import eq_cases as ec
import eq_np as m
import kfd_cases as kc
import kfd_np

pytestmark = pytest.mark.gpu
abi = gf.abi
PU8 = C.POINTER(C.c_uint8)
TRACKER_SHAPES = tuple(s for s in ec.SHAPES if s[0] > 21 and s[1] > 21)      # the tracker's window is 21 x 21
IDS = [ec.shape_id(s) for s in ec.SHAPES]
TIDS = [ec.shape_id(s) for s in TRACKER_SHAPES]


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


def _eq(be, shape, n):
    rows, cols, tx, ty, clip = shape
    return be.equalizer(n, rows, cols, tiles_x=tx, tiles_y=ty, clip_limit=clip)


def _same_levels(a, b, n, which=(1,)):
    """Every built level of the sets `which` of every camera, image and derivative, of two trackers."""
    for w in which:
        for cam in range(n):
            la = a.level(w, cam, 0)
            for lv in range(la["n_levels"]):
                x, y = (la if lv == 0 else a.level(w, cam, lv)), b.level(w, cam, lv)
                assert np.array_equal(x["image"], y["image"]) and np.array_equal(x["deriv"], y["deriv"]), (w, cam, lv)


def test_the_tracker_shapes():
    assert len(TRACKER_SHAPES) == 5 and (120, 188, 8, 8, 40.0) in TRACKER_SHAPES


@pytest.mark.parametrize("n", ec.N_CAMERAS)
@pytest.mark.parametrize("shape", ec.SHAPES, ids=IDS)
def test_apply_against_the_model(be, shape, n):
    rows, cols = shape[:2]
    imgs = ec.stack(rows, cols, n)
    want, wlut = ec.expected(shape, n)
    e = _eq(be, shape, n)
    try:
        assert e.lut_raw()[0] == abi.BAD_INPUT                      # nothing is held yet
        out = e.apply(imgs)
        assert np.array_equal(out, want) and np.array_equal(e.lut(), wlut)
        same = np.array(imgs)                                        # in == out
        assert e.apply(same, out=same) is same and np.array_equal(same, want) and np.array_equal(e.lut(), wlut)
    finally:
        e.close()


@pytest.mark.parametrize("n", ec.N_CAMERAS)
@pytest.mark.parametrize("shape", TRACKER_SHAPES, ids=TIDS)
def test_push_klt_against_a_tracker(be, shape, n):
    rows, cols = shape[:2]
    imgs = ec.stack(rows, cols, n)
    want, wlut = ec.expected(shape, n)
    e, ta, tb = _eq(be, shape, n), be.tracker(n, rows, cols, 16), be.tracker(n, rows, cols, 16)
    try:
        e.push_klt(ta, imgs)
        tb.push_image(want)
        assert np.array_equal(e.lut(), wlut)
        _same_levels(ta, tb, n)
        lv = ta.level(1, n - 1, 0)
        assert np.array_equal(lv["image"][abi.KLT_WIN:-abi.KLT_WIN, abi.KLT_WIN:-abi.KLT_WIN], want[n - 1])
    finally:
        e.close(), ta.close(), tb.close()


def _pairs(rows, cols, n):
    a = np.stack([gf.synth.klt_texture(rows, cols, seed=k) for k in range(n)])
    b = np.stack([gf.synth.klt_texture(rows, cols, seed=k, shift=(-1.6 - 0.3 * k, 0.9)) for k in range(n)])
    return a, b


def test_a_track_after_two_pushes(be):
    shape, n = (120, 188, 8, 8, 40.0), 3
    rows, cols, tx, ty, clip = shape
    a, b = _pairs(rows, cols, n)
    ea, eb = m.equalize_stack(a, tx, ty, clip)[0], m.equalize_stack(b, tx, ty, clip)[0]
    ys, xs = np.mgrid[25:rows - 25:14, 25:cols - 25:17]
    pts = [np.stack([xs.ravel() + 0.25 * k, ys.ravel() + 0.5], 1).astype(np.float32) for k in range(n)]
    ids, cnt = [np.arange(len(p), dtype=np.int32) + 100 * k for k, p in enumerate(pts)], [np.ones(len(p), np.int32) for p in pts]
    e, ta, tb = _eq(be, shape, n), be.tracker(n, rows, cols, 64), be.tracker(n, rows, cols, 64)
    try:
        e.push_klt(ta, a), tb.push_image(ea)
        ta.set_points(pts, ids, cnt), tb.set_points(pts, ids, cnt)
        e.push_klt(ta, b), tb.push_image(eb)
        _same_levels(ta, tb, n, which=(0, 1))
        ra, rb = ta.track(), tb.track()
        kept = 0
        for ca, cb in zip(ra, rb):
            assert ca["counters"] == cb["counters"] and np.array_equal(ca["ids"], cb["ids"]) and np.array_equal(ca["track_cnt"], cb["track_cnt"])
            for k in ("prev_pts", "cur_pts"):
                assert np.array_equal(ca[k].view(np.uint32), cb[k].view(np.uint32)), k
            kept += len(ca["ids"])
        assert kept > len(pts[0])      # the comparison is of real tracks
    finally:
        e.close(), ta.close(), tb.close()


def test_interleaved_pushes(be):
    """push_klt and gfbe_klt_push_image alternate on one tracker: the previous and current sets are each what was pushed."""
    shape, n = (61, 97, 8, 8, 3.0), 3
    rows, cols, tx, ty, clip = shape
    seq = [ec.stack(rows, cols, 9)[3 * k:3 * k + 3] for k in range(3)] + [ec.stack(rows, cols, n)]
    eqd = [m.equalize_stack(s, tx, ty, clip)[0] for s in seq]
    e, ta, tb = _eq(be, shape, n), be.tracker(n, rows, cols, 16), be.tracker(n, rows, cols, 16)
    try:
        e.push_klt(ta, seq[0]), tb.push_image(eqd[0])
        ta.push_image(seq[1]), tb.push_image(seq[1])              # plain: not equalised
        _same_levels(ta, tb, n, which=(0, 1))
        e.push_klt(ta, seq[2]), tb.push_image(eqd[2])
        _same_levels(ta, tb, n, which=(0, 1))
        ta.push_image(seq[3]), tb.push_image(seq[3])
        e.push_klt(ta, seq[3]), tb.push_image(eqd[3])
        _same_levels(ta, tb, n, which=(0, 1))
        assert np.array_equal(e.lut(), m.equalize_stack(seq[3], tx, ty, clip)[1])
    finally:
        e.close(), ta.close(), tb.close()


@pytest.mark.parametrize("n", (1, 65))
def test_back_to_back_pushes(be, n):
    """Two push_klt calls of different images with no wait between them: the tracker's pinned mirror is reused, both sets are right."""
    shape = (120, 188, 8, 8, 40.0)
    rows, cols, tx, ty, clip = shape
    first = ec.stack(rows, cols, n)
    second = np.ascontiguousarray(first[::-1, ::-1, :])                # other images: the cameras reversed and flipped
    w1, w2 = ec.expected(shape, n)[0], m.equalize_stack(second, tx, ty, clip)
    e, ta, tb = _eq(be, shape, n), be.tracker(n, rows, cols, 16), be.tracker(n, rows, cols, 16)
    try:
        e.push_klt(ta, first)
        e.push_klt(ta, second)
        tb.push_image(w1), tb.push_image(w2[0])
        _same_levels(ta, tb, n, which=(0, 1))
        assert np.array_equal(e.lut(), w2[1])
    finally:
        e.close(), ta.close(), tb.close()


@pytest.mark.parametrize("shape", (ec.SHAPES[1], ec.SHAPES[4], ec.SHAPES[8]), ids=lambda s: ec.shape_id(s))
def test_push_kfd(be, shape):
    """blurred_out of gfbe_kfd_download is kfd_np.blur of the model's equalised image; a capture from an equalised tracker gives the same slot."""
    rows, cols = shape[:2]
    n = 3
    imgs = ec.stack(rows, cols, n)
    want, wlut = ec.expected(shape, n)
    e, d = _eq(be, shape, n), be.describer(n, rows, cols, kc.pattern(), [kc.CAMERAS["plain"]] * n)
    t = be.tracker(n, rows, cols, 16) if shape in TRACKER_SHAPES else None
    try:
        d.push_image(0, imgs)                                         # another slot, plain: it must stay as it is
        e.push_kfd(d, 1, imgs)
        assert np.array_equal(e.lut(), wlut)
        for k in range(n):
            assert np.array_equal(d.planes(1, k, score=False)["blurred"], kfd_np.blur(want[k])), k
            assert np.array_equal(d.planes(0, k, score=False)["blurred"], kfd_np.blur(imgs[k])), k
        if t is not None:
            e.push_klt(t, imgs)
            d.capture(t, 2)
            for k in range(n):
                assert np.array_equal(d.planes(2, k, score=False)["blurred"], d.planes(1, k, score=False)["blurred"]), k
            got, ref = d.extract(2), d.extract(1)
            for k in range(n):
                assert got[k]["counters"] == ref[k]["counters"] and np.array_equal(got[k]["desc"], ref[k]["desc"])
    finally:
        e.close(), d.close()
        if t is not None:
            t.close()


def test_refusals(be):
    """On a live device: GFBE_BAD_INPUT, nothing written, no state changed."""
    lib, ctx = be.lib, be.ctx
    rows, cols, n = 48, 64, 2
    imgs = ec.stack(rows, cols, n)
    want, wlut = m.equalize_stack(imgs)

    def create(opt=None, n_=n, rows_=rows, cols_=cols, out=True):
        h = C.c_void_p(7)
        rc = lib.gfbe_eq_create(ctx, n_, rows_, cols_, C.byref(opt) if opt is not None else None, C.byref(h) if out else None)
        assert not out or not h.value
        return rc
    for kw in (dict(struct_size=16), dict(tiles_x=0), dict(tiles_x=65), dict(tiles_y=0), dict(tiles_y=65), dict(tiles_x=64), dict(tiles_y=48), dict(clip_limit=-0.5),
               dict(clip_limit=float("inf")), dict(clip_limit=float("nan"))):
        assert create(abi.eq_default_options(lib, **kw)) == abi.BAD_INPUT, kw
    for kw in (dict(rows_=8), dict(cols_=8), dict(rows_=16385), dict(cols_=16385), dict(n_=0), dict(n_=65536), dict(out=False)):
        assert create(**kw) == abi.BAD_INPUT, kw
    other = gf.Backend(device=0)
    e, t, d = be.equalizer(n, rows, cols), be.tracker(n, rows, cols, 16), be.describer(n, rows, cols, kc.pattern(), [kc.CAMERAS["plain"]] * n)
    t_small, t_one = be.tracker(n, rows, cols - 1, 16), be.tracker(1, rows, cols, 16)
    d_small, d_one = be.describer(n, rows - 1, cols, kc.pattern(), [kc.CAMERAS["plain"]] * n), be.describer(1, rows, cols, kc.pattern(), [kc.CAMERAS["plain"]])
    t_other, d_other, e_other = other.tracker(n, rows, cols, 16), other.describer(n, rows, cols, kc.pattern(), [kc.CAMERAS["plain"]] * n), other.equalizer(n, rows, cols)
    every = [e, t, d, t_small, t_one, d_small, d_one, t_other, d_other, e_other]
    try:
        p = np.ascontiguousarray(imgs).ctypes.data_as(PU8)
        lut = np.full((n, 8, 8, 256), 7, np.uint8)
        out = np.full((n, rows, cols), 7, np.uint8)
        po, pl = out.ctypes.data_as(PU8), lut.ctypes.data_as(PU8)
        assert lib.gfbe_eq_download_lut(ctx, e.h, pl) == abi.BAD_INPUT and b"apply or push first" in lib.gfbe_last_error(ctx) and (lut == 7).all()
        # a state to leave alone: one plain push on the tracker, one plain slot on the describer, one apply on the handle
        t.push_image(imgs), d.push_image(0, imgs)
        assert np.array_equal(e.apply(imgs), want)
        before = [t.level(1, k, 0) for k in range(n)]
        blurred = [d.planes(0, k, score=False)["blurred"] for k in range(n)]
        bad = [lib.gfbe_eq_apply(ctx, e.h, None, po), lib.gfbe_eq_apply(ctx, e.h, p, None), lib.gfbe_eq_apply(ctx, None, p, po), lib.gfbe_eq_apply(ctx, e_other.h, p, po),
               lib.gfbe_eq_apply(other.ctx, e.h, p, po), lib.gfbe_eq_download_lut(ctx, e.h, None), lib.gfbe_eq_download_lut(ctx, e_other.h, pl),
               lib.gfbe_eq_push_klt(ctx, e.h, None, p), lib.gfbe_eq_push_klt(ctx, e.h, t.h, None), lib.gfbe_eq_push_klt(ctx, None, t.h, p), lib.gfbe_eq_push_klt(ctx, e.h, t_other.h, p),
               lib.gfbe_eq_push_klt(ctx, e_other.h, t.h, p), lib.gfbe_eq_push_klt(ctx, e.h, t_small.h, p), lib.gfbe_eq_push_klt(ctx, e.h, t_one.h, p),
               lib.gfbe_eq_push_kfd(ctx, e.h, None, 0, p), lib.gfbe_eq_push_kfd(ctx, e.h, d.h, 0, None), lib.gfbe_eq_push_kfd(ctx, None, d.h, 0, p), lib.gfbe_eq_push_kfd(ctx, e.h, d_other.h, 0, p),
               lib.gfbe_eq_push_kfd(ctx, e_other.h, d.h, 0, p), lib.gfbe_eq_push_kfd(ctx, e.h, d_small.h, 0, p), lib.gfbe_eq_push_kfd(ctx, e.h, d_one.h, 0, p),
               lib.gfbe_eq_push_kfd(ctx, e.h, d.h, -1, p), lib.gfbe_eq_push_kfd(ctx, e.h, d.h, d.opt.ring_slots, p)]
        assert bad == [abi.BAD_INPUT] * len(bad), bad
        assert (out == 7).all() and (lut == 7).all()
        assert np.array_equal(e.lut(), wlut)                                               # the handle's LUTs are those of its apply
        for k in range(n):
            now = t.level(1, k, 0)
            assert np.array_equal(now["image"], before[k]["image"]) and np.array_equal(now["deriv"], before[k]["deriv"])
            assert np.array_equal(d.planes(0, k, score=False)["blurred"], blurred[k])
        assert t.level(1, 0, 0)["n_levels"] >= 1
        rc = lib.gfbe_klt_download_level(ctx, t.h, 0, 0, 0, None, None, None)
        assert rc == abi.BAD_INPUT                                                         # still one push: no refused call counted as one
        for tt in (t_small, t_one):
            assert lib.gfbe_klt_download_level(ctx, tt.h, 1, 0, 0, None, None, None) == abi.BAD_INPUT      # never pushed
        for dd in (d_small, d_one):
            assert lib.gfbe_kfd_download(ctx, dd.h, 0, 0, None, None) == abi.BAD_INPUT                     # never filled
        assert lib.gfbe_kfd_download(ctx, d.h, 1, 0, None, None) == abi.BAD_INPUT
        e.push_klt(t, imgs)                                                                # and the handles still work
        assert np.array_equal(t.level(1, 1, 0)["image"][abi.KLT_WIN:-abi.KLT_WIN, abi.KLT_WIN:-abi.KLT_WIN], want[1])
    finally:
        for h in every:
            h.close()
        other.close()
