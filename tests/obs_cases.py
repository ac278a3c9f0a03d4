"""TEST INFRASTRUCTURE. The cases of the frame observations (include/gfbe_obs.h) for tests/test_obs_model.py (the host build of
csrc/gfbe_obs.h against the model) and tests/test_gpu_obs.py (the device against the model), and what the model tests/obs_np.py gives
for them. Images are 64 x 48 throughout. A case is a list of calls; each call sets the held points of every camera (as a track and a
detect would leave them), optionally drops ids first (remove_outliers on the previous call's points), and observes."""
import functools
import json
import os

import numpy as np

import obs_np as m

F = np.float32
ROWS, COLS = 48, 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obs_cameras.json")


@functools.lru_cache(maxsize=None)
def golden_cameras():
    """name -> [fx fy cx cy k1 k2 p1 p2] of the reference's PINHOLE calibrations."""
    return {k: np.array(v, np.float64) for k, v in json.load(open(GOLDEN))["cameras"].items()}


NO_DISTORTION = np.array([60.0, 61.0, 31.5, 23.25, 0.0, 0.0, 0.0, 0.0])
STRONG = np.array([58.0, 57.0, 30.0, 25.0, -0.4, 0.2, 0.01, -0.02])      # (focal lengths of a 64 x 48 image: the whole image is inside the model's range)
TANGENTIAL_ONLY = np.array([600.0, 601.0, 320.0, 240.0, 0.0, 0.0, 0.003, -0.002])
SYNTHETIC = dict(no_distortion=NO_DISTORTION, strong=STRONG, tangential_only=TANGENTIAL_ONLY)


def all_cameras():
    return dict(golden_cameras(), **SYNTHETIC)


def depth_image(rows=ROWS, cols=COLS, planted=()):
    """Pixel (y, x) holds (y * cols + x) % 65536; planted: ((x, y, value), ...)."""
    d = ((np.arange(rows)[:, None] * cols + np.arange(cols)[None, :]) % 65536).astype(np.uint16)
    for x, y, v in planted:
        d[y, x] = v
    return d


def _points(n, seed, first_id, step=3):
    """n points inside the image on quarter pixels, ids out of order with gaps."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.integers(4, 4 * (COLS - 2), n), rng.integers(4, 4 * (ROWS - 2), n)], 1).astype(F) / F(4)
    ids = (first_id + step * rng.permutation(n)).astype(np.int32)
    return p, ids, (np.arange(n, dtype=np.int32) % 5 + 1).astype(np.int32)


NONE = (np.zeros((0, 2), F), np.zeros(0, np.int32), np.zeros(0, np.int32))


def _three_cameras(depth_cam):
    cams = np.stack([NO_DISTORTION, golden_cameras()["cam0_pinhole.yaml"], STRONG])
    p, ids, cnt = _points(37, 1, 100)
    # halves (C's round goes away from zero: 10.5 -> 11, 11.5 -> 12, not the 10 and 12 of cvRound), planted depths, a point outside the image
    p[0], p[1], p[2], p[3], p[4] = (10.5, 20.5), (11.5, 7.5), (30.0, 40.0), (50.25, 3.0), (-3.0, 5.0)
    p[5] = (63.5, 47.25)      # rounds to column 64: outside
    one = (np.array([[12.5, 33.0]], F), np.array([7], np.int32), np.array([2], np.int32))
    depth = np.stack([depth_image(), depth_image(), depth_image(planted=((30, 40, 0), (50, 3, 65535)))])
    # second call: 20 of the ids survive at moved positions (in another order), 9 are new; camera 1 keeps its point, camera 0 gains two
    rng = np.random.default_rng(2)
    keep = rng.permutation(37)[:20]
    p2 = np.concatenate([p[keep] + rng.integers(-4, 5, (20, 2)).astype(F) / F(4), _points(9, 3, 1000)[0]])
    p2 = np.clip(p2, 1.0, [COLS - 2.0, ROWS - 2.0]).astype(F)
    ids2 = np.concatenate([ids[keep], np.arange(9, dtype=np.int32) * 2 + 1000]).astype(np.int32)
    cnt2 = np.concatenate([cnt[keep] + 1, np.ones(9, np.int32)]).astype(np.int32)
    one2 = (np.array([[13.0, 32.5]], F), one[1], one[2] + 1)
    two = (np.array([[5.0, 6.0], [7.5, 8.5]], F), np.array([3, -2], np.int32), np.array([1, 1], np.int32))      # (a negative id sorts first)
    drop = [two[1][:1], np.array([99], np.int32), np.concatenate([ids2[::4], [5]]).astype(np.int32)]              # third call: after remove_outliers
    calls = [dict(held=[NONE, one, (p, ids, cnt)], time=[1.0, 1.0, 2.0]),
             dict(held=[two, one2, (p2, ids2, cnt2)], time=[1.1, 1.1, 2.1]),
             dict(drop=drop, time=[1.1999, 1.1999, 2.1999])]
    for c in calls:
        c["depth"] = depth if depth_cam else None
    return dict(rows=ROWS, cols=COLS, capacity=64, cameras=cams, depth_cam=depth_cam, calls=calls)


def _capacity_2048():
    cams = golden_cameras()["idc_cam.yaml"][None]
    calls, last = [], np.zeros(0, np.int32)
    for k, n in enumerate((2048, 65, 64, 63)):
        rng = np.random.default_rng(10 + k)
        p = np.stack([rng.integers(4, 4 * (COLS - 2), n), rng.integers(4, 4 * (ROWS - 2), n)], 1).astype(F) / F(4)
        known = last[rng.permutation(len(last))[:n // 2]]              # half of the ids are in the previous list, some are negative
        ids = np.concatenate([known, 10000 * (k + 1) + rng.permutation(4096)[:n - len(known)] - 1000]).astype(np.int32)[rng.permutation(n)]
        last = ids
        calls.append(dict(held=[(p, ids, np.ones(n, np.int32))], time=[0.5 + 0.05 * k], depth=depth_image()[None]))
    return dict(rows=ROWS, cols=COLS, capacity=2048, cameras=cams, depth_cam=1, calls=calls)


def _duplicate():
    p, ids, cnt = _points(9, 5, 40)
    ids = ids.copy()
    ids[6] = ids[2]
    return dict(rows=ROWS, cols=COLS, capacity=16, cameras=np.stack([STRONG, NO_DISTORTION]), depth_cam=0,
                calls=[dict(held=[(p, ids, cnt), _points(4, 6, 10)], time=[0.0, 0.0], depth=None)])


CASES = {"three_cameras": lambda: _three_cameras(1), "three_cameras_no_depth": lambda: _three_cameras(0), "capacity_2048": _capacity_2048, "duplicate": _duplicate}
NAMES = sorted(CASES)
SORT_LENGTHS = (0, 1, 2, 63, 64, 65, 2048)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """Per call: dict(held = the lists the tracker holds at the call, per camera; frame = the model's observe per camera)."""
    c = case(name)
    C_ = len(c["cameras"])
    prev, tprev, held, out = [m.EMPTY_PREV] * C_, [0.0] * C_, None, []
    for call in c["calls"]:
        if "held" in call:
            held = [tuple(np.asarray(a) for a in h) for h in call["held"]]
        else:
            held = [m.remove_outliers(held[k][0], held[k][1], held[k][2], call["drop"][k]) for k in range(C_)]
        frame = [m.observe(c["cameras"][k], held[k][0], held[k][1], prev[k], np.float64(call["time"][k]) - np.float64(tprev[k]),
                           call["depth"][k] if call["depth"] is not None else None) for k in range(C_)]
        prev, tprev = [f["prev"] for f in frame], list(call["time"])
        out.append(dict(held=held, frame=frame))
    return out


def sort_ids(n, seed=0, duplicate=False):
    rng = np.random.default_rng(seed + n)
    ids = (rng.permutation(max(3 * n, 1))[:n] - n).astype(np.int32)
    if duplicate and n >= 2:
        ids[n - 1] = ids[0]
    return ids


@functools.lru_cache(maxsize=None)
def predict_case():
    """A synthetic table and window for O8: features that predict, one without depth, one with one observation, one that ended before
    frame_count, one whose Z is exactly 0 (and one with X = Z = 0), one the held points do not know."""
    rng = np.random.default_rng(7)
    n, fc = 14, 6

    def rot(a, b, c):
        ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
        return (np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]) @ np.array([[1, 0, 0], [0, cc, -sc], [0, sc, cc]])).ravel()
    poses = np.zeros((11, 12))
    for f in range(11):
        poses[f, :3], poses[f, 3:] = (0.1 * f, 0.02 * f, -0.01 * f), rot(0.01 * f, -0.02 * f, 0.005 * f)
    tic_ric = np.concatenate([[0.05, -0.02, 0.01], rot(0.02, 0.01, -0.03)])
    next_pose = np.concatenate([[0.72, 0.14, -0.07], rot(0.07, -0.14, 0.035)])
    tab = dict(feature_id=(np.arange(n, dtype=np.int32) * 7 + 3), start_frame=np.zeros(n, np.int32), n_obs=np.zeros(n, np.int32), obs8=np.zeros((n, 11, 8)),
               estimated_depth=rng.uniform(1.0, 8.0, n))
    for k in range(n):
        tab["start_frame"][k] = rng.integers(0, 4)
        tab["n_obs"][k] = fc - tab["start_frame"][k] + 1
        tab["obs8"][k, :, 0], tab["obs8"][k, :, 1], tab["obs8"][k, :, 2] = rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), 1.0
    tab["estimated_depth"][1] = -1.0                                   # no depth
    tab["start_frame"][2], tab["n_obs"][2] = fc, 1                      # one observation
    tab["n_obs"][3] -= 1                                                # ended before frame_count
    tab["estimated_depth"][4] = 0.0                                     # depth 0 is not > 0
    ids = np.concatenate([tab["feature_id"][::-1][:12], [9999]]).astype(np.int32)      # two features are not held; one held point is unknown
    pts = np.stack([rng.uniform(2, COLS - 3, len(ids)), rng.uniform(2, ROWS - 3, len(ids))], 1).astype(F)
    # a window in which feature 5 has Z == 0 and feature 6 has X == Z == 0: identity rotations, no extrinsic offset
    eye = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
    flat_poses = np.zeros((11, 12))
    flat_poses[:, 3:] = eye
    flat_tic_ric = np.concatenate([[0.0, 0.0, 0.0], eye])
    tab0 = {k: v.copy() for k, v in tab.items()}
    tab0["estimated_depth"][5:7] = 2.0
    tab0["obs8"][6, :, 0] = 0.0
    flat_next = np.concatenate([[0.0, 0.0, 2.0], eye])
    return dict(frame_count=fc, table=tab, poses=poses, tic_ric=tic_ric, next_pose=next_pose, pts=pts, ids=ids,
                flat=dict(table=tab0, poses=flat_poses, tic_ric=flat_tic_ric, next_pose=flat_next))
