"""The frame observations on the device (gfbe_obs_*, include/gfbe_obs.h) against the model (tests/obs_np.py), bit for bit, on the cases
of tests/obs_cases.py: offsets, ids, rows, counters and the previous list over the calls of a case, with and without depth images; the
whole frame push_image -> track -> detect -> observe against the chain of the three models; the hand-over (a table fed by
gfbe_obs_add_frame against one fed by gfbe_ftab_add_frame with the lists observe returned, identical after every frame);
remove_outliers (a track after it gives the bits it gives after set_points with the model's survivors); predict against the model and
into gfbe_klt_track; the same bits alone and after a larger handle; the refusals with their outputs untouched. Float and double results
are compared as bit patterns."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import det_cases as dc
import det_np as dm
import klt_np as km
import obs_cases as oc
import obs_np as m

pytestmark = pytest.mark.gpu
abi = gf.abi
PF, PI, PD = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
F = np.float32


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


def _b32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _b64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _tables(be, n, capacity):
    return abi.FeatureTables(be.lib, "gfbe_", be.ctx, n, capacity)


class Rig:
    """A tracker with one image pushed and its observer."""

    def __init__(self, be, cameras, capacity, rows=oc.ROWS, cols=oc.COLS, images=None, **options):
        n = len(cameras)
        self.t = be.tracker(n, rows, cols, capacity)
        self.o = None
        try:
            self.t.push_image(images if images is not None else np.zeros((n, rows, cols), np.uint8))
            self.o = be.observer(self.t, cameras, **options)
        except Exception:
            self.t.close()
            raise

    def close(self):
        if self.o is not None:
            self.o.close()
        self.t.close()


def _same_frame(got, want, where):
    for k, (g, w) in enumerate(zip(got, want)):
        assert list(g["counters"].values()) == w["counters"].tolist(), (where, k, g["counters"], w["counters"])
        assert np.array_equal(g["ids"], w["ids"]) and np.array_equal(_b64(g["obs8"]), _b64(w["obs8"])), (where, k)


def _run_case(be, name):
    """Every call of a case on the device, checked against the model; returns what the device gave."""
    c, want = oc.case(name), oc.expected(name)
    r = Rig(be, c["cameras"], c["capacity"], depth_cam=c["depth_cam"])
    out = []
    try:
        for f, (call, w) in enumerate(zip(c["calls"], want)):
            if "held" in call:
                r.t.set_points([h[0] for h in call["held"]], [h[1] for h in call["held"]], [h[2] for h in call["held"]])
            else:
                r.o.remove_outliers(call["drop"])
            assert r.t.held == [len(h[1]) for h in w["held"]], (name, f)
            got = r.o.observe(call["time"], np.stack(call["depth"]) if call["depth"] is not None else None)
            _same_frame(got, w["frame"], (name, f))
            prev = [r.o.previous(k) for k in range(len(c["cameras"]))]
            for k, p in enumerate(prev):
                assert np.array_equal(p["ids"], w["frame"][k]["prev"][0]) and np.array_equal(_b32(p["un_pts"]), _b32(w["frame"][k]["prev"][1])), (name, f, k)
            out.append((got, prev))
        # NULL outputs: the counters alone come back (every id is in the previous list by now)
        last, w = c["calls"][-1], want[-1]
        rc, quiet = r.o.observe_raw([t + 0.25 for t in last["time"]], np.stack(last["depth"]) if last["depth"] is not None else None, outputs=False)
        assert rc == abi.OK and all(x["ids"] is None for x in quiet)
        for k, x in enumerate(quiet):
            n, _, outside, dup = w["frame"][k]["counters"].tolist()
            assert list(x["counters"].values()) == [n, n, outside, dup], (name, k)
    finally:
        r.close()
    return out


@pytest.mark.parametrize("name", oc.NAMES)
def test_observe_is_the_models(be, name):
    _run_case(be, name)


def test_the_whole_frame_is_the_chain_of_the_three_models(be):
    c, want = dc.case("two_frames"), dc.expected("two_frames")
    cams = np.stack([oc.golden_cameras()["cam0_pinhole.yaml"], oc.STRONG])
    depth = np.stack([oc.depth_image(c["rows"], c["cols"])] * 2)
    t = be.tracker(2, c["rows"], c["cols"], c["capacity"])
    d = o = None
    try:
        t.push_image(c["images"][0])
        t.set_points(c["pts"], c["ids"], c["cnt"])
        d = be.detector(t, **c["options"])
        d.set_next_id(c["next_id"])
        o = be.observer(t, cams)
        d.detect()
        f0 = o.observe([0.0, 0.0], depth)
        w0 = [m.observe(cams[k], want[0][k]["pts"], want[0][k]["ids"], m.EMPTY_PREV, 0.0, depth[k]) for k in range(2)]
        _same_frame(f0, w0, "first")
        t.push_image(c["images"][1])
        t.track()
        d.detect()
        f1 = o.observe([0.05, 0.07], depth)
        w1 = []
        for k in range(2):
            tr = km.track(km.build(c["images"][0][k], 3), km.build(c["images"][1][k], 3), want[0][k]["pts"], want[0][k]["ids"], want[0][k]["track_cnt"])
            de = dm.detect(c["images"][1][k], tr["cur_pts"], tr["ids"], tr["track_cnt"], want[0][k]["next_id"], **c["options"])
            w1.append(m.observe(cams[k], de["pts"], de["ids"], w0[k]["prev"], np.float64([0.05, 0.07][k]) - 0.0, depth[k]))
        _same_frame(f1, w1, "second")
        assert sum(int(w["counters"][0]) for w in w1) > 20
    finally:
        for h in (o, d):
            if h is not None:
                h.close()
        t.close()


# ---- the hand-over to the tables and the way back
def _scene(f):
    base = np.stack([dc.texture(oc.ROWS, oc.COLS, 31), dc.texture(oc.ROWS, oc.COLS, 32)])
    return np.ascontiguousarray(np.roll(base, f, axis=2))      # the scene moves by one pixel a frame


HAND_CAMS = np.stack([oc.golden_cameras()["wt_cam2.yaml"], oc.NO_DISTORTION])
TABLE_KEYS = ("feature_id", "start_frame", "n_obs", "obs8", "obs_td", "estimated_depth", "estimate_flag", "solve_flag")


def _same_tables(a, b, where):
    for w in range(a.W):
        x, y = a.download(w), b.download(w)
        for k in TABLE_KEYS:
            assert np.array_equal(np.ascontiguousarray(x[k]).view(np.uint8), np.ascontiguousarray(y[k]).view(np.uint8)), (where, w, k)


class Loop:
    """Six frames of push_image -> track -> detect -> observe -> add_frame on two cameras, table A fed on the device, table B through
    the host with the lists observe returned; some points are dropped on the way so that new features start late."""

    def __init__(self, be, frames=6):
        self.t = be.tracker(2, oc.ROWS, oc.COLS, 64)
        self.d = self.o = self.A = self.B = None
        self.dropped = [[], []]
        try:
            self.d = be.detector(self.t, max_cnt=30, min_dist=5)
            self.o = be.observer(self.t, HAND_CAMS)
            self.A, self.B = _tables(be, 2, 256), _tables(be, 2, 256)
            depth = np.stack([oc.depth_image(), oc.depth_image()])
            for f in range(frames):
                self.t.push_image(_scene(f))
                if f:
                    self.t.track()
                self.held = self.d.detect()
                fr = self.o.observe([0.1 * f, 0.1 * f + 0.5], depth)
                a = self.o.add_frame(self.A, [f, f], [0.0, 0.01])
                b = self.B.add_frame([f, f], [x["ids"] for x in fr], [x["obs8"] for x in fr], [0.0, 0.01])
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(_b64(a[2]), _b64(b[2])), (f, a, b)
                _same_tables(self.A, self.B, f)
                if f in (2, 4):
                    drop = [h["ids"][:3] for h in self.held]
                    for k in range(2):
                        self.dropped[k] += [int(i) for i in drop[k]]
                    self.o.remove_outliers(drop)
                    self.held = [dict(pts=h["pts"][3:], ids=h["ids"][3:], track_cnt=h["track_cnt"][3:]) for h in self.held]
                    assert self.t.held == [len(h["ids"]) for h in self.held]
            self.frames = frames
        except Exception:
            self.close()
            raise

    def close(self):
        for h in (self.o, self.d, self.A, self.B):
            if h is not None:
                h.close()
        self.t.close()


def test_a_table_fed_on_the_device_is_the_table_fed_through_the_host(be):
    lp = Loop(be)
    try:
        n_obs = np.concatenate([lp.A.download(w)["n_obs"] for w in range(2)])
        assert (n_obs >= 4).sum() >= 8 and (n_obs == 6).any()      # features reach four observations and more
    finally:
        lp.close()


def test_predict_is_the_models_and_feeds_the_tracker(be):
    lp = Loop(be)
    t2 = None
    try:
        fc = lp.frames - 1
        eye = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
        poses = np.zeros((2, 11, 12))
        poses[:, :, 3:] = eye
        poses[:, :, 0] = -0.02 * np.arange(11)[None, :]      # the cameras slide along x against the scene's one pixel a frame
        tic_ric = np.tile(np.concatenate([[0.0, 0.0, 0.0], eye]), (2, 1))
        lp.A.triangulate(poses, tic_ric)
        tabs = [lp.A.download(w) for w in range(2)]
        # the held points of the last detect, and behind them the points dropped at frame 4: their features ended before frame_count
        held = []
        for k in range(2):
            ended = [i for i in lp.dropped[k][3:]]
            p = np.concatenate([lp.held[k]["pts"], np.array([[20.0 + 3 * j, 30.0] for j in range(len(ended))], F).reshape(-1, 2)])
            held.append((p, np.concatenate([lp.held[k]["ids"], ended]).astype(np.int32), np.concatenate([lp.held[k]["track_cnt"], np.ones(len(ended), np.int32)])))
        lp.t.set_points([h[0] for h in held], [h[1] for h in held], [h[2] for h in held])
        # the next pose: camera 0 at the depth of one predicting feature (its Z is exactly 0), camera 1 a step further along x
        tab0 = tabs[0]
        at = {int(f): j for j, f in enumerate(tab0["feature_id"])}
        cand = [int(i) for i in held[0][1] if m.predicts(tab0["estimated_depth"][at[int(i)]], tab0["n_obs"][at[int(i)]], tab0["start_frame"][at[int(i)]], fc)]
        assert len(cand) >= 2, cand
        j = at[cand[0]]
        pw = m.chain_world(tab0["obs8"][j, 0, :3], tab0["estimated_depth"][j], poses[0, tab0["start_frame"][j]], tic_ric[0])
        next_pose = np.stack([np.concatenate([[-0.12, 0.0, float(pw[2])], eye]), np.concatenate([[-0.12, 0.0, 0.0], eye])])
        want = [m.predict(HAND_CAMS[k], held[k][0], held[k][1], tabs[k], fc, poses[k], tic_ric[k], next_pose[k]) for k in range(2)]
        pred, npred = lp.o.predict(lp.A, [fc, fc], poses, tic_ric, next_pose)
        for k in range(2):
            assert npred[k] == want[k][1] and np.array_equal(_b32(pred[k]), _b32(want[k][0])), (k, npred, want[k][1])
        # what the table holds for the held ids: each kind is there
        kinds = dict(no_depth=0, one_obs=0, ended=0, predicts=0)
        for k in range(2):
            at = {int(f): j for j, f in enumerate(tabs[k]["feature_id"])}
            for i in held[k][1]:
                j = at[int(i)]
                dep, no, st = tabs[k]["estimated_depth"][j], tabs[k]["n_obs"][j], tabs[k]["start_frame"][j]
                kinds["no_depth"] += int(not dep > 0)
                kinds["one_obs"] += int(no == 1)
                kinds["ended"] += int(dep > 0 and no >= 2 and st + no - 1 < fc)
                kinds["predicts"] += int(m.predicts(dep, no, st, fc))
        assert all(v > 0 for v in kinds.values()), kinds
        z0 = list(held[0][1]).index(cand[0])
        assert np.array_equal(pred[0][z0], held[0][0][z0]) and npred[0] < kinds_of(tabs[0], held[0][1], fc)      # Z == 0 falls back to the held point
        assert npred[0] >= 1 and npred[1] >= 2
        # into the tracker as it is
        nxt = _scene(lp.frames)
        t2 = be.tracker(2, oc.ROWS, oc.COLS, 64)
        t2.push_image(_scene(fc))
        t2.set_points([h[0] for h in held], [h[1] for h in held], [h[2] for h in held])
        t2.push_image(nxt)
        lp.t.push_image(nxt)
        rc, a = lp.t.track_raw(predict=pred)
        assert rc == abi.OK
        b = t2.track(predict=[w[0] for w in want])
        for x, y in zip(a, b):
            assert x["counters"] == y["counters"]
            assert all(np.array_equal(np.ascontiguousarray(x[q]).view(np.uint8), np.ascontiguousarray(y[q]).view(np.uint8)) for q in ("prev_pts", "cur_pts", "ids", "track_cnt"))
    finally:
        if t2 is not None:
            t2.close()
        lp.close()


def kinds_of(tab, ids, fc):
    """The held ids whose table feature predicts."""
    at = {int(f): j for j, f in enumerate(tab["feature_id"])}
    return sum(int(m.predicts(tab["estimated_depth"][at[int(i)]], tab["n_obs"][at[int(i)]], tab["start_frame"][at[int(i)]], fc)) for i in ids)


def test_a_track_after_remove_outliers_is_a_track_after_set_points(be):
    """The hand-over back: after remove_outliers the tracker is in the state gfbe_klt_set_points with the model's survivors leaves it in."""
    c = dc.case("s64x48_three_cameras")
    want = dc.expected("s64x48_three_cameras")[0]
    nxt = np.ascontiguousarray(np.roll(c["images"][0], 1, axis=2))
    cams = np.stack([oc.NO_DISTORTION, oc.STRONG, oc.NO_DISTORTION])
    r = Rig(be, cams, c["capacity"], images=c["images"][0], depth_cam=0)
    t2 = be.tracker(3, c["rows"], c["cols"], c["capacity"])
    try:
        lists = [(w["pts"], w["ids"], w["track_cnt"]) for w in want]
        r.t.set_points([x[0] for x in lists], [x[1] for x in lists], [x[2] for x in lists])
        drop = [lists[0][1][1::3], np.array([12345], np.int32), lists[2][1][:2]]
        r.o.remove_outliers(drop)
        left = [m.remove_outliers(x[0], x[1], x[2], dr) for x, dr in zip(lists, drop)]
        assert r.t.held == [len(x[1]) for x in left] and sum(r.t.held) < sum(len(x[1]) for x in lists)
        r.t.push_image(nxt)
        a = r.t.track()
        t2.push_image(c["images"][0])
        t2.set_points([x[0] for x in left], [x[1] for x in left], [x[2] for x in left])
        t2.push_image(nxt)
        b = t2.track()
        assert sum(len(x["ids"]) for x in b) > 0
        for x, y in zip(a, b):
            assert x["counters"] == y["counters"]
            assert all(np.array_equal(np.ascontiguousarray(x[q]).view(np.uint8), np.ascontiguousarray(y[q]).view(np.uint8)) for q in ("prev_pts", "cur_pts", "ids", "track_cnt"))
    finally:
        t2.close()
        r.close()


def test_same_bits_alone_and_after_a_larger_handle(be):
    """A handle's results depend on nothing a larger handle left behind (allocations are reused by the runtime)."""
    first = _run_case(be, "three_cameras")
    _run_case(be, "capacity_2048")
    second = _run_case(be, "three_cameras")
    for (fa, pa), (fb, pb) in zip(first, second):
        for x, y in zip(fa, fb):
            assert x["counters"] == y["counters"] and np.array_equal(x["ids"], y["ids"]) and np.array_equal(_b64(x["obs8"]), _b64(y["obs8"]))
        for x, y in zip(pa, pb):
            assert np.array_equal(x["ids"], y["ids"]) and np.array_equal(_b32(x["un_pts"]), _b32(y["un_pts"]))


def test_refusals_leave_the_outputs_untouched(be):
    c, want = oc.case("three_cameras"), oc.expected("three_cameras")
    lib, ctx = be.lib, be.ctx
    cams = np.ascontiguousarray(c["cameras"])
    depth = np.stack(c["calls"][0]["depth"])
    t = be.tracker(3, oc.ROWS, oc.COLS, 64)
    wide = be.tracker(1, oc.ROWS, oc.COLS, abi.DET_MAX_POINTS + 1)
    tabs, tabs2 = _tables(be, 3, 128), _tables(be, 2, 128)
    o = None
    try:
        h = C.c_void_p()
        pd = lambda a: a.ctypes.data_as(PD)
        for kw in (dict(struct_size=8), dict(depth_cam=2), dict(match_tile=100), dict(match_tile=2048)):
            assert lib.gfbe_obs_create(ctx, t.h, pd(cams), C.byref(abi.obs_default_options(lib, **kw)), C.byref(h)) == abi.BAD_INPUT and not h.value, kw
        for k, v in ((0, 0.0), (9, 0.0), (4, float("nan")), (2, float("inf")), (23, float("-inf"))):      # fx, fy of 0; a parameter that is not finite
            bad = cams.copy()
            bad.ravel()[k] = v
            assert lib.gfbe_obs_create(ctx, t.h, pd(bad), None, C.byref(h)) == abi.BAD_INPUT and not h.value, (k, v)
        assert lib.gfbe_obs_create(ctx, wide.h, pd(cams), None, C.byref(h)) == abi.BAD_INPUT and not h.value and b"GFBE_DET_MAX_POINTS" in lib.gfbe_last_error(ctx)
        assert lib.gfbe_obs_create(ctx, None, pd(cams), None, C.byref(h)) == abi.BAD_INPUT and not h.value
        assert lib.gfbe_obs_create(ctx, t.h, None, None, C.byref(h)) == abi.BAD_INPUT and not h.value
        o = be.observer(t, cams)
        untouched = lambda raw: all((np.asarray(v) == -7).all() for v in (raw.values() if isinstance(raw, dict) else raw))
        # no image yet
        rc, raw = o.observe_raw([1.0] * 3, depth)
        assert rc == abi.BAD_INPUT and untouched(raw) and b"no image" in lib.gfbe_last_error(ctx)
        assert o.remove_outliers_raw([[1], [], []]) == abi.BAD_INPUT
        rc, raw = o.predict_raw(tabs, [1] * 3, np.zeros((3, 132)), np.zeros((3, 12)), np.zeros((3, 12)))
        assert rc == abi.BAD_INPUT and (raw[1] == -7).all()
        t.push_image(np.zeros((3, oc.ROWS, oc.COLS), np.uint8))
        held = want[0]["held"]
        t.set_points([x[0] for x in held], [x[1] for x in held], [x[2] for x in held])
        # add_frame before observe
        rc, raw = o.add_frame_raw(tabs, [0] * 3, [0.0] * 3)
        assert rc == abi.BAD_INPUT and untouched(raw) and b"no frame" in lib.gfbe_last_error(ctx)
        # a missing depth image, times that are not finite
        for tm, dp in (([1.0] * 3, None), ([1.0, float("nan"), 1.0], depth), ([float("inf")] * 3, depth)):
            rc, raw = o.observe_raw(tm, dp)
            assert rc == abi.BAD_INPUT and untouched(raw), tm
        first = o.observe(c["calls"][0]["time"], depth)
        _same_frame(first, want[0]["frame"], "after the refusals")
        for tm in (c["calls"][0]["time"], [0.5, 5.0, 5.0]):      # not greater than the previous time
            rc, raw = o.observe_raw(tm, depth)
            assert rc == abi.BAD_INPUT and untouched(raw), tm
        # a table count that does not fit; another context's handle
        rc, raw = o.add_frame_raw(tabs2, [0] * 3, [0.0] * 3)
        assert rc == abi.BAD_INPUT and untouched(raw)
        rc, raw = o.predict_raw(tabs2, [1] * 3, np.zeros((3, 132)), np.zeros((3, 12)), np.zeros((3, 12)))
        assert rc == abi.BAD_INPUT and (raw[1] == -7).all()
        off = np.array([0, 2, 1, 1], np.int32)
        assert lib.gfbe_obs_remove_outliers(ctx, o.h, off.ctypes.data_as(PI), off.ctypes.data_as(PI), None) == abi.BAD_INPUT      # offsets that do not ascend
        n = C.c_int32(-7)
        assert lib.gfbe_obs_download_prev(ctx, o.h, 3, C.byref(n), None, None) == abi.BAD_INPUT and n.value == -7
        other = gf.Backend(device=0)
        try:
            out = np.full(16, -7, np.int32)
            tm = np.array([9.0] * 3)
            assert other.lib.gfbe_obs_observe(other.ctx, o.h, pd(tm), depth.ctypes.data_as(C.POINTER(C.c_uint16)), None, None, None, out.ctypes.data_as(PI)) == abi.BAD_INPUT and (out == -7).all()
            assert other.lib.gfbe_obs_create(other.ctx, t.h, pd(cams), None, C.byref(h)) == abi.BAD_INPUT and not h.value
        finally:
            other.close()
        # the frame is still the one observe left: it is added once, and only once
        assert t.held == [len(x[1]) for x in held]
        kf, cnt, avg = o.add_frame(tabs, [0] * 3, [0.0] * 3)
        assert cnt[:, 1].tolist() == [0, 1, 37]
        before = [tabs.download(w) for w in range(3)]
        rc, raw = o.add_frame_raw(tabs, [1] * 3, [0.0] * 3)
        assert rc == abi.BAD_INPUT and untouched(raw) and b"already added" in lib.gfbe_last_error(ctx)
        # a frame with a duplicate id: observe reports it, add_frame refuses, both tables stay as they were
        dup = (np.concatenate([held[2][0], held[2][0][:1]]), np.concatenate([held[2][1], held[2][1][3:4]]), np.concatenate([held[2][2], [1]]).astype(np.int32))
        t.set_points([held[0][0], held[1][0], dup[0]], [held[0][1], held[1][1], dup[1]], [held[0][2], held[1][2], dup[2]])
        fr = o.observe([t_ + 1.0 for t_ in c["calls"][0]["time"]], depth)
        assert [x["counters"]["duplicate"] for x in fr] == [0, 0, 1]
        other_tabs = _tables(be, 3, 128)
        try:
            for tb in (tabs, other_tabs):
                rc, raw = o.add_frame_raw(tb, [1] * 3, [0.0] * 3)
                assert rc == abi.BAD_INPUT and untouched(raw) and b"same id" in lib.gfbe_last_error(ctx)
            assert other_tabs.size().tolist() == [0, 0, 0]
        finally:
            other_tabs.close()
        after = [tabs.download(w) for w in range(3)]
        for x, y in zip(before, after):
            assert all(np.array_equal(np.ascontiguousarray(x[k]).view(np.uint8), np.ascontiguousarray(y[k]).view(np.uint8)) for k in TABLE_KEYS)
    finally:
        if o is not None:
            o.close()
        tabs.close()
        tabs2.close()
        wide.close()
        t.close()
