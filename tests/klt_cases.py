"""Seeded cases of the optical-flow tracker, shared by tests/test_klt_model.py (host build against the model, branch coverage) and
tests/test_gpu_klt.py (device against the model): the smallest shapes at which a kernel can go wrong. A case is
dict(rows, cols, images [pushes][n_cameras, rows, cols], pts / ids / cnt per camera (the points of the first image), predict per track,
options, capacity). expected_flows(name) / expected_tracks(name) run the model once per case and are shared by every test.

The images are the analytic texture of synth.klt_texture moved by a planted translation, with four painted regions where the image
is large enough: a flat block (the minEig test fails at level 0 and, at its centre, one level up), a saturated block, a small
saturated spot that moves with the scene (the grey rule), and a 2-pixel checkerboard that jumps by one row between the images (the
oscillation rule and the iteration cap)."""
import functools

import numpy as np

from _gfbe_import import gf
import klt_np as m

synth = gf.synth
F = np.float32


def paint(a, b, shift):
    rows, cols = a.shape
    if rows < 80 or cols < 80:
        return a, b
    a, b = a.copy(), b.copy()
    s = min(rows, cols) // 3
    for im in (a, b):
        im[4:4 + s, 4:4 + s] = 90                                   # flat
        im[rows - 4 - s // 2:rows - 4, cols - 4 - s // 2:cols - 4] = 255      # saturated
    yy, xx = np.mgrid[0:rows, 0:cols]
    chk = ((((xx // 2) + (yy // 2)) % 2) * 140 + 50).astype(np.uint8)
    r0, c0 = rows - 8 - s, 8
    a[r0:r0 + s, c0:c0 + s] = chk[r0:r0 + s, c0:c0 + s]
    b[r0:r0 + s, c0:c0 + s] = chk[r0 + 1:r0 + s + 1, c0:c0 + s]
    sy, sx = 12, cols - 30                                          # the spot, moved by the rounded translation
    a[sy - 2:sy + 3, sx - 2:sx + 3] = 255
    dy, dx = int(round(shift[1])), int(round(shift[0]))
    b[sy - 2 + dy:sy + 3 + dy, sx - 2 + dx:sx + 3 + dx] = 255
    return a, b


def regions(rows, cols):
    s = min(rows, cols) // 3
    return dict(flat=(4 + s / 2.0, 4 + s / 2.0), saturated=(cols - 4 - s / 4.0, rows - 4 - s / 4.0), checker=(8 + s / 2.0, rows - 8 - s / 2.0), spot=(cols - 30.0, 12.0), s=s)


def pair(rows, cols, seed, shift):
    a, b = synth.klt_image_pair(rows, cols, seed, shift)
    return paint(a, b, shift)


def special_points(rows, cols):
    """Points for every edge and region of an image: windows over each edge, a start left of -21, starts beyond the far edges, the flat
    block (centre: flat one level up too), the saturated block, the spot, the checkerboard, coordinates on multiples of 2^-15."""
    r = regions(rows, cols)
    p = [(3.25, rows / 2.0), (cols - 3.5, rows / 2.0), (cols / 2.0, 2.75), (cols / 2.0, rows - 3.25),      # the four edges
         (0.0, 0.0), (cols - 1.0, rows - 1.0), (-5.5, 20.0), (cols + 4.5, rows + 3.0),
         (-11.5, rows / 2.0), (-40.0, 10.0), (cols + 10.5, 30.0), (30.0, rows + 40.0),                      # iprevPt.x = -22 and beyond
         (cols / 2.0 + 2.0 ** -15, rows / 2.0), (cols / 2.0 + 3 * 2.0 ** -15, rows / 2.0 + 0.5),           # a weight product on a half
         (40.0 + 5 * 2.0 ** -15, 60.0)]
    if rows >= 80 and cols >= 80:
        p += [r["flat"], (r["flat"][0] + 3.0, r["flat"][1] - 2.5), (6.0, 6.0), r["saturated"], r["spot"], (r["spot"][0] + 0.5, r["spot"][1] - 0.25)]
        cx, cy = r["checker"]
        p += [(cx + dx, cy + dy) for dx in (-12.25, -4.0, 3.5, 10.75) for dy in (-11.0, -3.25, 4.5, 12.0)]
    return np.array(p, np.float32)


def _case(rows, cols, seed, shift, counts, n_images=2, predict=None, options=None, special=None, capacity=None):
    """counts: points per camera; camera k sees the texture of seed + k; special: the camera that gets special_points first."""
    C = len(counts)
    frames = []
    for k in range(C):
        ims = [pair(rows, cols, seed + k, shift)]
        for t in range(2, n_images):
            ims.append(pair(rows, cols, seed + k, (shift[0] * t, shift[1] * t)))
        frames.append([ims[0][0]] + [x[1] for x in ims])
    images = [np.stack([frames[k][t] for k in range(C)]) for t in range(n_images)]
    pts = []
    for k, n in enumerate(counts):
        sp = special_points(rows, cols) if special == k else np.zeros((0, 2), np.float32)
        sp = sp[:n]
        g = synth.klt_grid_points(rows, cols, n - len(sp), seed=seed + 31 * k, margin=min(12.0, rows / 4.0))
        pts.append(np.concatenate([sp, g]).astype(np.float32))
    ids = [np.arange(n, dtype=np.int32) * 3 + 1000 * k for k, n in enumerate(counts)]
    cnt = [(np.arange(n, dtype=np.int32) % 7) + 1 for n in counts]
    return dict(rows=rows, cols=cols, images=images, pts=pts, ids=ids, cnt=cnt, predict=predict or [None] * (n_images - 1), options=options or {},
                capacity=capacity or max(max(counts), 1), shift=shift)


def _junk(n, cols, rows):
    """Points that can never succeed: they start outside the image."""
    return np.stack([np.full(n, -60.0), np.linspace(5.0, rows - 5.0, n)], 1).astype(np.float32)


def _prediction_case():
    """Three cameras with a prediction: camera 0 has 10 good points and junk (no fallback), camera 1 has 9 good points and junk (fewer
    than 10 successes: the fallback), camera 2 has no prediction. The good points get their true displacement as the prediction."""
    rows, cols, shift = 89, 91, (2.6, -1.3)
    c = _case(rows, cols, 11, shift, [16, 15, 12])
    for k, good in ((0, 10), (1, 9)):
        n = len(c["pts"][k])
        inner = synth.klt_grid_points(rows, cols, good, seed=77 + k, margin=28.0)
        c["pts"][k] = np.concatenate([inner, _junk(n - good, cols, rows)]).astype(np.float32)
    c["predict"] = [[c["pts"][0] + F(shift), c["pts"][1] + F(shift), None]]
    return c


def _boundary_case(below):
    """The reverse test at its boundary. No input can be planted so that the reverse flow lands at a distance of exactly 0.5, so the
    boundary is put where a point lands: flow_back_dist is the exact double distance of one kept point as the model computes it
    (<= keeps the point), or with `below` the next double under it (the point goes). The device has to form the same double."""
    c = _case(48, 64, 21, (0.3, 0.2), [12])
    pa, pb = m.build(c["images"][0][0], 3), m.build(c["images"][1][0], 3)
    r = m.track(pa, pb, c["pts"][0], c["ids"][0], c["cnt"][0])
    d = [m.distance(c["pts"][0][i], r["reverse"][i]) for i in range(12) if r["decisions"][i] == 3]
    d = sorted(x for x in d if x > 0.0)
    c["options"] = dict(flow_back_dist=float(np.nextafter(d[len(d) // 2], 0.0)) if below else d[len(d) // 2])
    return c


def _in_border_case(rows, cols):
    """inBorder's rounding on planted cur_pts. With max_count = 0 no level iterates, so a prediction passes through the descent
    unchanged (x 0.5 at level 1, x 2 at level 0, both exact) and the reverse call hands back prev_pts: cur_pts equals predict_pts
    bit for bit. Points 0 .. 2 are predicted at x = 0.5, 1.5, cols - 1.5, points 3 .. 5 at y = 0.5, 1.5, rows - 1.5 (half to even:
    0.5 -> 0 outside, 1.5 -> 2 inside, n - 1.5 -> n - 2 inside for even n, n - 1 outside for odd n); the rest are inside, so that
    the prediction has its 10 successes."""
    c = _case(rows, cols, 31, (0.0, 0.0), [16], options=dict(max_count=0))
    pred = c["pts"][0].copy()
    mid_x, mid_y = F(cols // 2 + 0.25), F(rows // 2 + 0.25)
    pred[:6] = [(0.5, mid_y), (1.5, mid_y), (cols - 1.5, mid_y), (mid_x, 0.5), (mid_x, 1.5), (mid_x, rows - 1.5)]
    c["predict"] = [[pred]]
    return c


CASES = {
    "in_border_even": lambda: _in_border_case(48, 64),
    "in_border_odd": lambda: _in_border_case(89, 91),
    "s23_level0_only": lambda: _case(23, 23, 1, (0.3, 0.2), [5], special=0),
    "s64x48_two_levels": lambda: _case(48, 64, 2, (0.3, 0.2), [63, 0, 65], special=2),
    "s91x89_three_levels": lambda: _case(89, 91, 3, (2.6, -1.3), [64, 1, 257], special=0, capacity=257),
    "s180x177_four_levels": lambda: _case(177, 180, 4, (7.3, -4.6), [70], special=0),
    "s640x480": lambda: _case(480, 640, 5, (7.3, -4.6), [96], special=0),
    "prediction": _prediction_case,
    "flow_back_off": lambda: _case(89, 91, 6, (2.6, -1.3), [40, 3], options=dict(flow_back=0), special=0),
    "three_images": lambda: _case(89, 91, 7, (1.3, 0.7), [65, 0, 20], n_images=3, special=0),
    "reverse_boundary_kept": lambda: _boundary_case(False),
    "reverse_boundary_gone": lambda: _boundary_case(True),
    "loose_options": lambda: _case(177, 180, 8, (2.6, -1.3), [40], options=dict(max_level=1, max_count=5, epsilon=0.1, border=0, grey_max=200), special=0),
}
NAMES = sorted(CASES)
# (direction, max_level, with an initial flow)
FLOWS = [(0, 3, False), (1, 3, False), (0, 0, False), (0, 1, True), (1, 1, True), (1, 0, True), (0, 3, True)]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def initial_flow(c, k):
    """A seeded initial flow for camera k: the points moved by the planted translation and a little more."""
    rng = np.random.default_rng(99 + k)
    p = c["pts"][k]
    return (p + F(c["shift"]) + (np.rint(rng.uniform(-1.5, 1.5, p.shape) * 32) / 32).astype(np.float32)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pyramids(name):
    """[push][camera] -> the model's pyramid (levels as the handle builds them: at least level 1 is asked for)."""
    c = case(name)
    ml = max(dict(m.DEFAULTS, **c["options"])["max_level"], 1)
    return [[m.build(im[k], ml) for k in range(len(im))] for im in c["images"]]


@functools.lru_cache(maxsize=None)
def expected_flows(name):
    """{(direction, max_level, initial): [per camera model result with trace]} on the first two images."""
    c, pyr = case(name), pyramids(name)
    P = m.params(**dict(m.DEFAULTS, **c["options"]))
    out = {}
    for d, ml, init in FLOWS:
        res = []
        for k, p in enumerate(c["pts"]):
            I, J = (pyr[0][k], pyr[1][k]) if d == 0 else (pyr[1][k], pyr[0][k])
            res.append(m.flow(I, J, p, initial_flow(c, k) if init else None, ml, P, trace=True))
        out[(d, ml, init)] = res
    return out


@functools.lru_cache(maxsize=None)
def expected_tracks(name):
    """[track][camera] -> the model's track; the survivors of a track are the points of the next."""
    c, pyr = case(name), pyramids(name)
    held = [(c["pts"][k], c["ids"][k], c["cnt"][k]) for k in range(len(c["pts"]))]
    out = []
    for t in range(len(c["images"]) - 1):
        res = []
        for k, (p, i_, n_) in enumerate(held):
            pred = c["predict"][t][k] if c["predict"][t] is not None else None
            if pred is not None and t > 0:
                pred = None
            res.append(m.track(pyr[t][k], pyr[t + 1][k], p, i_, n_, pred, **c["options"]))
        out.append(res)
        held = [(r["cur_pts"], r["ids"], r["track_cnt"]) for r in res]
    return out
