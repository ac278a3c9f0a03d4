"""Seeded cases of the corner detector, shared by tests/test_det_model.py (host build against the model, branch coverage) and
tests/test_gpu_det.py (device against the model): the smallest shapes at which a kernel can go wrong. A case is
dict(rows, cols, images [frames][n_cameras, rows, cols], pts / ids / cnt per camera (the held points at the first frame), options,
capacity (the tracker's point_capacity), next_id per camera, corners = (max_corners, quality, min_dist) of the mask-free call).
expected(name) runs the model once per case and is shared by every test: [frame][camera] -> det_np.detect's result; the result of a
frame is the held list of the next."""
import functools

import numpy as np

from _gfbe_import import gf
import det_np as m

synth = gf.synth
F = np.float32


def squares(rows, cols, seed=0):
    """10 x 10 squares of grey 200 every 24 pixels on a background of 40 + noise in 0 .. 3, and the pixels of their corners."""
    rng = np.random.default_rng(seed)
    im = (40 + rng.integers(0, 4, (rows, cols))).astype(np.uint8)
    planted = []
    for j in range((rows - 8) // 24):
        for i in range((cols - 8) // 24):
            y, x = 7 + 24 * j, 7 + 24 * i
            im[y:y + 10, x:x + 10] = 200
            planted += [(x, y), (x + 9, y), (x, y + 9), (x + 9, y + 9)]
    return im, np.array(planted, np.int64)


def noise(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols)).astype(np.uint8)


def texture(rows, cols, seed):
    return synth.klt_texture(rows, cols, seed)


def periodic(rows, cols):
    yy, xx = np.mgrid[0:rows, 0:cols]
    return ((((xx // 2) + (yy // 2)) % 2) * 140 + 50).astype(np.uint8)


def border_peaks(rows, cols):
    """Camera 0: the only structure is a bright spot in row 0, camera 1: in column 0; a faint square inside gives both real candidates."""
    out = []
    for k in range(2):
        im = np.full((rows, cols), 60, np.uint8)
        im[rows // 2:rows // 2 + 6, cols // 2:cols // 2 + 6] = 90
        if k == 0:
            im[0, cols // 3:cols // 3 + 2] = 255
        else:
            im[rows // 3:rows // 3 + 2, 0] = 255
        out.append(im)
    return np.stack(out)


def _held(rows, cols, n, seed, cnt_mod=7):
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(1, cols - 2, n), rng.uniform(1, rows - 2, n)], 1).astype(F)
    return p, (np.arange(n, dtype=np.int32) * 3 + 10), ((np.arange(n, dtype=np.int32) * 5) % cnt_mod + 1).astype(np.int32)


def _case(images, held, options, capacity=None, next_id=None, corners=(50, 0.01, 10)):
    images = [np.ascontiguousarray(f, np.uint8) for f in images]
    C = images[0].shape[0]
    pts, ids, cnt = [h[0] for h in held], [h[1] for h in held], [h[2] for h in held]
    o = dict(m.DEFAULTS, **options)
    return dict(rows=images[0].shape[1], cols=images[0].shape[2], images=images, pts=pts, ids=ids, cnt=cnt, options=options,
                capacity=capacity or max([o["max_cnt"]] + [len(p) for p in pts]), next_id=list(next_id or [0] * C), corners=corners)


NONE = (np.zeros((0, 2), F), np.zeros(0, np.int32), np.zeros(0, np.int32))


def _special_held(rows, cols):
    """Ties in track_cnt, two points on one pixel, a point inside an earlier disc, discs over each edge and corner, points whose pixel is
    outside the image (dropped), halves that round to even."""
    p = [(20.25, 20.0), (20.4, 19.75),                     # one pixel (20, 20): the second goes
         (23.0, 24.0), (24.0, 24.0),                         # d^2 = 25 from (20, 20): inside its disc at min_dist 5; d^2 = 32: kept
         (2.0, rows / 2.0), (cols - 2.0, rows / 2.0), (cols / 2.0, 1.0), (cols / 2.0, rows - 2.0),      # discs over each edge
         (0.0, 0.0), (cols - 1.0, 0.0), (0.0, rows - 1.0), (cols - 1.0, rows - 1.0),                    # and each corner
         (-0.5, 10.0), (cols - 0.5, 10.0), (-1.0, 10.0), (10.0, rows + 0.0), (-60.0, -60.0), (1e9, 5.0), (5.0, -3e9),      # -0.5 -> 0 inside; cols - 0.5 by parity; outside
         (40.5, 9.5), (41.5, 10.5)]                          # halves: 40, 10 and 42, 10 (d^2 = 4)
    p = np.array(p, F)
    n = len(p)
    cnt = np.array([5, 5, 5, 5, 9, 9, 9, 9, 2, 2, 2, 2, 7, 7, 7, 7, 7, 7, 7, 3, 3], np.int32)
    return p, np.arange(n, dtype=np.int32) + 500, cnt


def _noise_case(**options):
    im = noise(177, 180, 5)[None]
    o = dict(dict(max_cnt=1000, min_dist=5), **options)
    return _case([im], [_held(177, 180, 12, 3)], o, capacity=1024, corners=(1000, 0.01, 5))


def _two_frames():
    a = np.stack([texture(89, 91, 21), texture(89, 91, 22)])
    b = np.stack([texture(89, 91, 23), texture(89, 91, 24)])
    return _case([a, b], [_held(89, 91, 9, 4), NONE], dict(max_cnt=40, min_dist=9), next_id=[100, 5])


CASES = {
    "s23_first_frame": lambda: _case([texture(23, 23, 1)[None]], [NONE], dict(max_cnt=20, min_dist=5)),
    "s64x48_three_cameras": lambda: _case([np.stack([texture(48, 64, 2), texture(48, 64, 3), squares(48, 64, 1)[0]])], [_special_held(48, 64), NONE, _held(48, 64, 6, 1)],
                                          dict(max_cnt=40, min_dist=5)),
    "s91x89_min_dist_30": lambda: _case([texture(89, 91, 4)[None]], [_special_held(89, 91)], dict(max_cnt=60, min_dist=30)),
    "s91x89_min_dist_0": lambda: _case([texture(89, 91, 4)[None]], [_special_held(89, 91)], dict(max_cnt=150, min_dist=0), corners=(50, 0.01, 0)),
    "s91x89_min_dist_1": lambda: _case([texture(89, 91, 4)[None]], [_special_held(89, 91)], dict(max_cnt=150, min_dist=1), corners=(50, 0.01, 1)),
    "s91x89_quality_0": lambda: _case([texture(89, 91, 5)[None]], [_held(89, 91, 10, 2)], dict(max_cnt=150, min_dist=5, quality=0.0), corners=(50, 0.0, 10)),
    "held_equal_max_cnt": lambda: _case([squares(89, 91, 2)[0][None]], [_held(89, 91, 20, 5)], dict(max_cnt=20, min_dist=1)),
    "held_above_max_cnt": lambda: _case([squares(89, 91, 2)[0][None]], [_held(89, 91, 24, 6)], dict(max_cnt=10, min_dist=1), capacity=32),
    "fully_masked": lambda: _case([texture(48, 64, 6)[None]], [(np.array([[32.0, 24.0]], F), np.array([7], np.int32), np.array([3], np.int32))], dict(max_cnt=30, min_dist=100)),
    "flat": lambda: _case([np.full((1, 48, 64), 77, np.uint8)], [_held(48, 64, 3, 7)], dict(max_cnt=30, min_dist=5)),
    "border_peaks": lambda: _case([border_peaks(48, 64)], [NONE, NONE], dict(max_cnt=30, min_dist=5)),
    "periodic": lambda: _case([periodic(48, 64)[None]], [NONE], dict(max_cnt=400, min_dist=1), corners=(400, 0.01, 2)),
    "noise_default_chunk": lambda: _noise_case(),
    "noise_smallest_chunk": lambda: _noise_case(sort_chunk=64),
    "noise_overflow": lambda: _noise_case(candidate_capacity=500),
    "noise_mid_chunk": lambda: _noise_case(sort_chunk=64, max_cnt=112),
    "s640x480": lambda: _case([squares(480, 640, 3)[0][None]], [_held(480, 640, 100, 8)], dict()),
    "two_frames": _two_frames,
}
NAMES = sorted(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    held = [(c["pts"][k], c["ids"][k], c["cnt"][k]) for k in range(len(c["pts"]))]
    nid = list(c["next_id"])
    out = []
    for f in c["images"]:
        res = [m.detect(f[k], held[k][0], held[k][1], held[k][2], nid[k], **c["options"]) for k in range(len(held))]
        out.append(res)
        held = [(r["pts"], r["ids"], r["track_cnt"]) for r in res]
        nid = [r["next_id"] for r in res]
    return out


@functools.lru_cache(maxsize=None)
def expected_corners(name):
    c = case(name)
    mc, q, md = c["corners"]
    return [m.corners(c["images"][0][k], mc, q, md, dict(m.DEFAULTS, **c["options"])["candidate_capacity"]) for k in range(len(c["pts"]))]
