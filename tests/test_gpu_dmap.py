"""gfbe_dmap_* on the device against the model (tests/dmap_np.py) over tests/dmap_cases.py. Every output is compared for equality:
the counts, the cloud (world float32 bits, rgb, keyframe and pool index, in insertion order), every keyframe's list after every step,
the filter's keep flags, n_keep and compacted output. The cases keep every point K u A = 32 u A away from a float32 rounding
boundary and a gate and 1e-9 (relative) away from a voxel face (K from r_cpu = 4.13, tests/test_dmap_model.py), so the device's FP64
arithmetic cannot take another decision than the model's. Measured on the MI355X: every comparison of the 25 tests holds
(the whole file runs in 1.8 s; the largest case, 262 145 points, 0.1 s)."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import dmap_cases as dc
import dmap_np as dn

pytestmark = pytest.mark.gpu
abi = gf.abi
CASES = dc.cases()
FILT = dc.filter_cases()
COUNTS = ("n_keyframes", "n_stored", "n_cloud", "n_voxels", "n_skipped", "n_gated", "n_refused")
_MODELS = {}


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


def _model(name):
    """The model's run of a case, step by step: computed once and left unchanged."""
    if name not in _MODELS:
        c, m, snaps = CASES[name], dc.model_for(CASES[name]), []
        for s in c["steps"]:
            m.add_keyframe(*s[1:]) if s[0] == "add" else m.rebuild(s[1])
            snaps.append(dict(size=m.size(), xyz=m.xyz.copy(), rgb=m.rgb.copy(), kf=m.kf.copy(), src=m.src.copy(), pool=m.pool()))
        _MODELS[name] = (m, snaps)
    return _MODELS[name]


def _counts(dm):
    s = dm.size()
    return {k: s[k] for k in COUNTS}


def _check(dm, snap, keyframes=None):
    assert _counts(dm) == snap["size"]
    got = dm.cloud()
    for k in ("xyz", "rgb", "kf", "src"):
        assert np.array_equal(got[k], snap[k]), k
    assert got["xyz"].dtype == np.float32
    if keyframes is not None:      # (the keyframes' lists, in keyframe order, are the pool)
        lists = [dm.keyframe(k) for k in keyframes]
        assert np.array_equal(np.concatenate([x["pts"] for x in lists]), snap["pool"][0]) and np.array_equal(np.concatenate([x["rgb"] for x in lists]), snap["pool"][1])


def _run(dm, case, upto=None):
    for s in case["steps"][:upto]:
        dm.add_keyframe(*s[1:]) if s[0] == "add" else dm.rebuild(s[1])


@pytest.mark.parametrize("name", list(CASES))
def test_case_against_the_model(be, name):
    """Insert: n = 0, 1, 7 in one voxel (the first 3), a voxel at 2 then 3 candidates (one), the scan's workgroup boundaries 255 / 256 /
    257 / 513, the second level's chunk boundary 256 * 1024 + 1 and the same reversed, points ON and just outside the gates, NaN /
    infinite / outside-the-box points between good ones, negative coordinates. Rebuild: 3 and 40 keyframes at corrected poses, then an
    insert that meets full voxels. After every step: counts, cloud, src / kf columns; at the end every keyframe's list."""
    c = CASES[name]
    _, snaps = _model(name)
    dm = be.dense_map(c["pcap"], c["kcap"], **c["opt"])
    try:
        n_kf = 0
        for s, snap in zip(c["steps"], snaps):
            if s[0] == "add":
                dm.add_keyframe(*s[1:])
                n_kf += 1
            else:
                before = [dm.keyframe(k) for k in (0, n_kf - 1)]
                dm.rebuild(s[1])
                after = [dm.keyframe(k) for k in (0, n_kf - 1)]
                for a, b in zip(before, after):      # the pool is untouched by a rebuild
                    assert np.array_equal(a["pts"], b["pts"]) and np.array_equal(a["rgb"], b["rgb"])
            _check(dm, snap, range(n_kf) if s is c["steps"][-1] else None)
    finally:
        dm.close()


def test_rank_and_base_count_are_not_one_per_voxel(be):
    """What an implementation that keeps one point per voxel, or forgets the counts of earlier calls, gets wrong."""
    c = CASES["base2_then3"]
    dm = be.dense_map(64, 4)
    try:
        _run(dm, c)
        got = dm.cloud()
        assert got["kf"].tolist() == [0] * 5 + [1] * 3 and got["src"].tolist() == list(range(8))
        assert np.array_equal(dm.keyframe(1)["pts"], c["steps"][1][2][[0, 1, 4]])
        assert dm.size()["n_voxels"] == 5
    finally:
        dm.close()


def test_rebuild_at_unchanged_poses_equals_a_fresh_map(be):
    """A rebuild at the poses the keyframes were inserted at gives the cloud of a fresh map fed with the same lists under the
    rebuild's cap (no gate: the lists hold survivors of the gate only). The cap is 2 here, below the insert's 3, so that it drops points."""
    c = CASES["rebuild_40"]
    adds = [s for s in c["steps"][:-1] if s[0] == "add"]
    a = be.dense_map(c["pcap"], c["kcap"], **dict(c["opt"], rebuild_cap=2))
    b = be.dense_map(c["pcap"], c["kcap"], **dict(c["opt"], add_cap=2, **dc.OPEN))
    try:
        for s in adds:
            a.add_keyframe(*s[1:])
        lists = [a.keyframe(k) for k in range(len(adds))]
        a.rebuild(np.array([s[1] for s in adds]))
        for s, l in zip(adds, lists):
            b.add_keyframe(s[1], l["pts"], l["rgb"])
        ca, cb = a.cloud(), b.cloud()
        assert len(ca["xyz"]) > 0 and a.size()["n_voxels"] == b.size()["n_voxels"]
        for k in ("xyz", "rgb", "kf"):
            assert np.array_equal(ca[k], cb[k]), k
        assert (np.diff(ca["src"]) > 0).all() and len(ca["xyz"]) < a.size()["n_stored"]      # (pool order; the cap dropped points)
    finally:
        a.close()
        b.close()


def test_capacity_keeps_the_prefix(be):
    """The pool and the keyframe table one short of what is needed: the prefix is kept, n_refused is exact, the map stays usable."""
    c = CASES["rebuild_3"]
    full, _ = _model("rebuild_3")
    adds = [s for s in c["steps"] if s[0] == "add"]
    need = sum(len(p) for p in full.kf_pts)
    # the pool one short
    m = dn.DenseMapModel(need - 1, len(adds), **c["opt"])
    dm = be.dense_map(need - 1, len(adds), **c["opt"])
    try:
        for s in c["steps"]:
            (m.add_keyframe(*s[1:]), dm.add_keyframe(*s[1:])) if s[0] == "add" else (m.rebuild(s[1]), dm.rebuild(s[1]))
        assert m.n_refused == 1
        _check(dm, dict(size=m.size(), xyz=m.xyz, rgb=m.rgb, kf=m.kf, src=m.src, pool=m.pool()), range(len(adds)))
        # a full pool refuses the next call whole, all its points counted; the keyframe exists and is empty
        s = adds[0]
        m2, dm2 = dn.DenseMapModel(need - 1, len(adds) + 1, **c["opt"]), be.dense_map(need - 1, len(adds) + 1, **c["opt"])
        try:
            for t in c["steps"] + [s]:
                (m2.add_keyframe(*t[1:]), dm2.add_keyframe(*t[1:])) if t[0] == "add" else (m2.rebuild(t[1]), dm2.rebuild(t[1]))
            assert m2.n_refused == 1 + len(s[2]) and _counts(dm2) == m2.size() and len(dm2.keyframe(len(adds))["pts"]) == 0
            # ... and the map remains usable: a rebuild and the filter
            poses = np.array([t[1] for t in adds] + [s[1]])
            m2.rebuild(poses); dm2.rebuild(poses)
            _check(dm2, dict(size=m2.size(), xyz=m2.xyz, rgb=m2.rgb, kf=m2.kf, src=m2.src, pool=m2.pool()))
            assert np.array_equal(dm2.filter()["keep"], m2.filter())
        finally:
            dm2.close()
    finally:
        dm.close()
    # the keyframe table one short: the last insert is refused whole
    m = dn.DenseMapModel(need, len(adds) - 1, **c["opt"])
    dm = be.dense_map(need, len(adds) - 1, **c["opt"])
    try:
        for s in adds:
            m.add_keyframe(*s[1:]); dm.add_keyframe(*s[1:])
        assert m.n_refused == len(adds[-1][2]) and m.size()["n_keyframes"] == len(adds) - 1
        _check(dm, dict(size=m.size(), xyz=m.xyz, rgb=m.rgb, kf=m.kf, src=m.src, pool=m.pool()), range(len(adds) - 1))
        poses = np.array([t[1] for t in adds[:-1]])
        m.rebuild(poses); dm.rebuild(poses)
        _check(dm, dict(size=m.size(), xyz=m.xyz, rgb=m.rgb, kf=m.kf, src=m.src, pool=m.pool()))
    finally:
        dm.close()


def test_same_bits_alone_after_a_larger_map_and_again(be):
    c = CASES["rebuild_40"]

    def run():
        dm = be.dense_map(c["pcap"], c["kcap"], **c["opt"])
        try:
            _run(dm, c)
            return dm.cloud(), dm.size(), dm.filter()
        finally:
            dm.close()
    first = run()
    big = CASES["chunk_262145"]
    other = be.dense_map(big["pcap"], big["kcap"], **big["opt"])      # a larger map on the same context in between
    try:
        _run(other, big)
        other.filter(compact=False)
        for again in (run(), run()):
            assert again[1] == first[1]
            for k in first[0]:
                assert np.array_equal(again[0][k], first[0][k]), k
            for k in ("keep", "xyz", "rgb"):
                assert np.array_equal(again[2][k], first[2][k]), k
    finally:
        other.close()


@pytest.mark.parametrize("name", list(FILT))
def test_filter_against_the_brute_force(be, name):
    """An isolated point, clusters of exactly min_neighbors and min_neighbors + 1, two points exactly radius apart on dyadic coordinates,
    a dense cell (fast path) beside sparse neighbours (walk path), clusters across cell faces and the coordinate planes, 5 000 random
    points; the compacted output in cloud order; the fast path's count."""
    c = FILT[name]
    o = dict(dn.DEFAULTS, **c["opt"])
    dm = be.dense_map(len(c["pts"]), 2, **c["opt"])
    try:
        dm.add_keyframe(dc.IDENT, c["pts"], c["rgb"])
        want = dn.filter_brute(c["pts"], o["filter_radius"], o["filter_min_neighbors"])
        got = dm.filter()
        assert np.array_equal(dm.cloud()["xyz"], c["pts"])
        assert np.array_equal(got["keep"], want) and got["n_keep"] == int(want.sum())
        assert np.array_equal(got["xyz"], c["pts"][want == 1]) and np.array_equal(got["rgb"], c["rgb"][want == 1])
        cell = np.floor(c["pts"].astype(np.float64) / (o["filter_radius"] / 1.75)).astype(np.int64)
        _, inv, cnt = np.unique(cell, axis=0, return_inverse=True, return_counts=True)
        fast = int((cnt[inv.ravel()] > o["filter_min_neighbors"]).sum())
        assert dm.size()["n_fast"] == fast and (name == "exact_radius" or 0 < fast < got["n_keep"])      # both paths decide points
        again = dm.filter(compact=False)
        assert np.array_equal(again["keep"], want) and "xyz" not in again
    finally:
        dm.close()


def test_filter_of_a_rebuilt_map_and_of_an_empty_one(be):
    c = CASES["rebuild_3"]
    m, snaps = _model("rebuild_3")
    dm = be.dense_map(c["pcap"], c["kcap"], **c["opt"])
    try:
        got = dm.filter()
        assert got["n_keep"] == 0 and len(got["keep"]) == 0 and len(got["xyz"]) == 0
        _run(dm, c, upto=len(c["steps"]) - 1)      # up to the rebuild
        snap = snaps[-2]
        want = dn.filter_brute(snap["xyz"], 0.8, 10)
        got = dm.filter()
        assert np.array_equal(got["keep"], want) and np.array_equal(got["xyz"], snap["xyz"][want == 1]) and 0 < want.sum()
    finally:
        dm.close()


def test_bad_input_leaves_the_map_untouched(be):
    c = CASES["wg_257"]
    dm = be.dense_map(c["pcap"], 4, **c["opt"])
    other = gf.Backend(device=0)
    try:
        _run(dm, c)
        before = (dm.size(), dm.cloud())
        pose, pts, rgb = c["steps"][0][1:]
        f = dm._f("add_keyframe")
        PF, PU8, PD = abi.PF, abi.PU8, abi.PD
        p, q, r = np.ascontiguousarray(pose), np.ascontiguousarray(pts), np.ascontiguousarray(rgb)
        nan_pose = p.copy()
        nan_pose[4] = np.nan
        assert f(dm.ctx, dm.h, p.ctypes.data_as(PD), -1, q.ctypes.data_as(PF), r.ctypes.data_as(PU8)) == abi.BAD_INPUT
        assert f(dm.ctx, dm.h, p.ctypes.data_as(PD), 5, None, r.ctypes.data_as(PU8)) == abi.BAD_INPUT
        assert f(dm.ctx, dm.h, p.ctypes.data_as(PD), 5, q.ctypes.data_as(PF), None) == abi.BAD_INPUT
        assert f(dm.ctx, dm.h, None, 5, q.ctypes.data_as(PF), r.ctypes.data_as(PU8)) == abi.BAD_INPUT
        assert f(dm.ctx, dm.h, nan_pose.ctypes.data_as(PD), 5, q.ctypes.data_as(PF), r.ctypes.data_as(PU8)) == abi.BAD_INPUT
        assert f(other.ctx, dm.h, p.ctypes.data_as(PD), 5, q.ctypes.data_as(PF), r.ctypes.data_as(PU8)) == abi.BAD_INPUT      # a handle of another context
        assert dm.add_keyframe_raw(pose, np.zeros((c["pcap"] + 1, 3), np.float32), np.zeros((c["pcap"] + 1, 3), np.uint8)) == abi.BAD_INPUT
        assert dm.rebuild_raw(np.zeros((0, 7))) == abi.BAD_INPUT and dm.rebuild_raw(np.tile(pose, (2, 1))) == abi.BAD_INPUT      # one keyframe is held
        assert dm.rebuild_raw(nan_pose) == abi.BAD_INPUT
        assert dm._f("rebuild")(other.ctx, dm.h, 1, p.ctypes.data_as(PD)) == abi.BAD_INPUT
        assert dm._f("filter")(other.ctx, dm.h, None, None, None, None) == abi.BAD_INPUT
        assert dm._f("filter")(dm.ctx, dm.h, None, None, q.ctypes.data_as(PF), None) == abi.BAD_INPUT
        n = abi.c_i(-7)
        assert dm._f("download_keyframe")(dm.ctx, dm.h, 1, C.byref(n), None, None) == abi.BAD_INPUT and n.value == -7
        assert dm._f("download_keyframe")(dm.ctx, dm.h, -1, C.byref(n), None, None) == abi.BAD_INPUT
        for kw in (dict(add_cap=0), dict(rebuild_cap=9), dict(struct_size=8), dict(filter_radius=float("nan"))):
            with pytest.raises(gf.BackendError):
                be.dense_map(64, 4, **kw)
        after = (dm.size(), dm.cloud())
        assert after[0] == before[0] and all(np.array_equal(after[1][k], before[1][k]) for k in before[1])
    finally:
        other.close()
        dm.close()
