"""The life cycle of the nine device handles (gfbe_ftab, gfbe_ltab, gfbe_vmap, gfbe_scan, gfbe_dmap, gfbe_ldb, gfbe_klt, gfbe_det, gfbe_obs)
through the classes of abi.py: no device memory is lost over create / destroy, destroy(ctx, NULL) returns and changes nothing, a handle
of another context is refused with BAD_INPUT and its text while the handle stays usable on its own context, and a create that refuses
its capacity leaves *out null and no memory behind.

The bound of the memory checks is half of ONE handle's device footprint, computed below from the capacities as a lower bound of what
its create allocates (the arrays whose sizes follow from the capacities alone; scratch rows, staging and per-camera words are left out,
which only makes the bound tighter). Eight handles are created and destroyed: a handle that is not freed loses eight footprints, one
leaked array of the larger ones more than half a footprint. Every footprint is several megabytes, far above the allocator's granule."""
import ctypes as C

import numpy as np
import pytest
import torch

from _gfbe_import import gf
import ldb_cases as lc

pytestmark = pytest.mark.gpu
abi = gf.abi
PI = C.POINTER(abi.c_i)
TRK = dict(n_cameras=3, rows=768, cols=1024, point_capacity=512)      # the tracker the detector and the observer borrow from
SMALL_TRK = dict(n_cameras=1, rows=64, cols=64, point_capacity=256)
FTAB, LTAB, VMAP, VMAP_P, SCAN, DMAP, LDB = (1, 4096), (1, 8192), 4096, 20, 1 << 15, (1 << 15, 64), (8, 1 << 17)
VOC = lc.trees()["k3L2"]


def _pow2(n):
    s = 64
    while s < n:
        s <<= 1
    return s


def _cameras(trk):
    return np.tile(np.array([500.0, 500.0, trk["cols"] / 2, trk["rows"] / 2, 0, 0, 0, 0]), (trk["n_cameras"], 1))


def _i32(n):
    return np.zeros(n, np.int32)


def _size(n_out, split):
    """gfbe_<family>size with n_out int32 outputs: one pointer each (split), or one array."""
    def op(ctx, h):
        v = (abi.c_i * n_out)()
        return h._f("size")(ctx, h.h, *([C.cast(C.byref(v, 4 * k), PI) for k in range(n_out)] if split else [v]))
    return op


class Family:
    """make(backend, tracker) -> an abi.Handle; bytes: the lower bound of its device footprint; op(ctx, handle) -> status of one cheap
    call; bad(backend, tracker, out) -> status of a create whose capacity is out of range."""
    borrows = False

    def __init__(self, make, nbytes, op, bad, checks_owner):
        self.make, self.bytes, self.op, self.bad, self.checks_owner = make, int(nbytes), op, bad, checks_owner


def _families():
    f = {}
    W, cap = FTAB      # two halves of id start nobs eflag sflag, depth, obs [11][8], td [11]; keep, ndepth, ids
    f["ftab"] = Family(lambda b, t, s: abi.FeatureTables(b.lib, "gfbe_", b.ctx, *FTAB), W * cap * (2 * (5 * 4 + 8 + 8 * 11 * 8 + 8 * 11) + 4 + 8 + 4),
                       lambda ctx, h: h._f("size")(ctx, h.h, _i32(h.W).ctypes.data_as(PI)),
                       lambda b, t, out: b.lib.gfbe_ftab_create(b.ctx, 1, 16385, None, C.byref(out)), False)
    W, cap = LTAB      # two halves of id start nobs, tri, plk [6], obs [11][4]; keep, dst, plk_out [6], rkeep
    f["ltab"] = Family(lambda b, t, s: b.line_tables(*LTAB), W * cap * (2 * (3 * 4 + 1 + 48 + 11 * 4 * 8) + 4 + 4 + 48 + 1),
                       lambda ctx, h: h._f("size")(ctx, h.h, _i32(h.W).ctypes.data_as(PI)),
                       lambda b, t, out: b.lib.gfbe_ltab_create(b.ctx, 1, 16385, C.byref(out)), False)
    slots = _pow2(2 * VMAP)      # two halves of keys, cnt, pts [VMAP_P][3]
    f["vmap"] = Family(lambda b, t, s: b.voxel_map(VMAP, max_num_points_in_voxel=VMAP_P), 2 * slots * (8 + 4 + VMAP_P * 24), _size(4, True),
                       lambda b, t, out: b.lib.gfbe_vmap_create(b.ctx, (1 << 21) + 1, C.byref(abi.vmap_default_options(b.lib)), C.byref(out)), False)
    N, slots = SCAN, _pow2(2 * SCAN)      # two halves and the keypoints of src pts alpha ts; slot_of, world; keys, minidx
    f["scan"] = Family(lambda b, t, s: b.scan(SCAN), N * (3 * (4 + 24 + 8 + 8) + 4 + 24) + slots * (8 + 4), _size(3, True),
                       lambda b, t, out: b.lib.gfbe_scan_create(b.ctx, (1 << 21) + 1, C.byref(out)), True)
    N = DMAP[0]      # pool 19, cloud 23, slot_of won 8, cand 12, cslot keep_i 8, sorted out_xyz 24, keep_b out_rgb 4 per point; 40 per slot
    f["dmap"] = Family(lambda b, t, s: b.dense_map(*DMAP), N * 98 + _pow2(2 * N) * 40, _size(len(abi.DMAP_COUNTS), False),
                       lambda b, t, out: b.lib.gfbe_dmap_create(b.ctx, (1 << 26) + 1, DMAP[1], C.byref(abi.dmap_default_options(b.lib)), C.byref(out)), True)
    voc = abi.LdbVocabHolder(VOC)      # bow_word, bow_val, desc [4], pts [2], ptsn [2] per descriptor
    f["ldb"] = Family(lambda b, t, s: b.loop_database(voc, *LDB), LDB[1] * (4 + 8 + 32 + 8 + 8), _size(len(abi.LDB_COUNTS), False),
                      lambda b, t, out: b.lib.gfbe_ldb_create(b.ctx, C.byref(voc.c), LDB[0], (1 << 26) + 1, C.byref(abi.ldb_default_options(b.lib)), C.byref(out)), True)
    Cn, R, Cc = TRK["n_cameras"], TRK["rows"], TRK["cols"]      # the upload; two sets of level 0 with its border of 21: the image and two int16 derivatives
    f["klt"] = Family(lambda b, t, s: b.tracker(**(SMALL_TRK if s else TRK)), Cn * (R * Cc + 2 * 5 * (R + 42) * (Cc + 42)),
                      lambda ctx, h: h._f("push_image")(ctx, h.h, np.zeros((h.n_cameras, h.rows, h.cols), np.uint8).ctypes.data_as(abi.PU8)),
                      lambda b, t, out: b.lib.gfbe_klt_create(b.ctx, 1, 64, 64, (1 << 20) + 1, C.byref(abi.klt_default_options(b.lib)), C.byref(out)), True)
    f["det"] = Family(lambda b, t, s: b.detector(t), Cn * (R - 2) * (Cc - 2) * 8,      # the candidates: one key per interior pixel
                      lambda ctx, h: h._f("set_next_id")(ctx, h.h, _i32(h.tracker.n_cameras).ctypes.data_as(PI)),
                      lambda b, t, out: b.lib.gfbe_det_create(b.ctx, t.h, C.byref(abi.det_default_options(b.lib, max_cnt=t.cap + 1)), C.byref(out)), True)
    n = Cn * TRK["point_capacity"]      # the depth image; the frame's ids and rows [8]; two halves of ids and undistorted points
    f["obs"] = Family(lambda b, t, s: b.observer(t, _cameras(SMALL_TRK if s else TRK)), Cn * R * Cc * 2 + n * (4 + 64 + 2 * (4 + 8)),
                      lambda ctx, h: h._f("reset")(ctx, h.h),
                      lambda b, t, out: b.lib.gfbe_obs_create(b.ctx, t.h, _cameras(TRK).ctypes.data_as(C.POINTER(C.c_double)),
                                                              C.byref(abi.obs_default_options(b.lib, match_tile=100)), C.byref(out)), True)
    f["det"].borrows = f["obs"].borrows = True
    return f


FAMILIES = _families()
NAMES = list(FAMILIES)


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def trk(be):
    t = be.tracker(**TRK)
    yield t
    t.close()


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def _lost(fam, before, what):
    lost = before - _free()
    print("%s: footprint %d bytes, free memory fell by %d" % (what, fam.bytes, lost))
    return lost


@pytest.mark.parametrize("name", NAMES)
def test_footprint_is_several_megabytes(name):
    assert FAMILIES[name].bytes >= 4 << 20, FAMILIES[name].bytes


@pytest.mark.parametrize("name", NAMES)
def test_create_destroy_loses_no_device_memory(be, trk, name):
    fam = FAMILIES[name]
    fam.make(be, trk, False).close()      # the runtime's own first-use allocations
    before = _free()
    h = fam.make(be, trk, False)
    live = _lost(fam, before, name + " (one live handle)")      # the meter sees a handle: it would see one that is never freed
    h.close()
    assert live >= fam.bytes // 2
    for _ in range(8):
        h = fam.make(be, trk, False)
        assert h.h
        h.close()
    assert _lost(fam, before, name) <= fam.bytes // 2


@pytest.mark.parametrize("name", NAMES)
def test_destroy_of_null_changes_nothing(be, trk, name):
    fam = FAMILIES[name]
    h = fam.make(be, trk, False)
    try:
        assert fam.op(be.ctx, h) == abi.OK
        before = _free()
        h._f("destroy")(be.ctx, None)
        h._f("destroy")(None, None)
        assert abs(_lost(fam, before, name)) <= fam.bytes // 2
        assert fam.op(be.ctx, h) == abi.OK
    finally:
        h.close()


@pytest.mark.parametrize("name", [n for n in NAMES if FAMILIES[n].checks_owner])
def test_handle_of_another_context_is_refused(be, name):
    fam = FAMILIES[name]
    other = gf.Backend(device=0)
    t = other.tracker(**SMALL_TRK) if fam.borrows else None
    h = None
    try:
        h = fam.make(other, t, True)
        assert fam.op(other.ctx, h) == abi.OK
        assert fam.op(be.ctx, h) == abi.BAD_INPUT
        assert "belongs to another context" in be._err(), be._err()
        assert fam.op(other.ctx, h) == abi.OK
    finally:
        for x in (h, t):
            if x is not None:
                x.close()
        other.close()


@pytest.mark.parametrize("name", NAMES)
def test_refused_create_leaves_null_and_no_memory(be, trk, name):
    fam = FAMILIES[name]
    fam.make(be, trk, False).close()
    before = _free()
    out = C.c_void_p()
    assert fam.bad(be, trk, out) == abi.BAD_INPUT
    assert not out.value
    assert _lost(fam, before, name) <= fam.bytes // 2
