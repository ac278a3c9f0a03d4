"""TEST INFRASTRUCTURE. The model of the keyframe descriptors (include/gfbe_kfd.h, rules K1 .. K5), written from the rules' text in numpy
integers and np.float32, with an independent second statement of each of K1, K2 and K4:

  K1  blur            separable passes on the reflect-padded array      blur_dense: one dense 9 x 9 integer correlation
  K2  fast_scores     minima over the arcs by rolled arrays              fast_score_brute: "corner at threshold s" as a predicate over the
                                                                         16 rotations, the score the largest s in 0 .. 254 that holds
  K4  brief           vectorised float32 addition and truncation         brief_scalar: a loop on Python floats and ints

K5 is obs_np.lift (the model of gfbe_obs.h's O3). What K1 and K2 say about cv::GaussianBlur and cv::FAST is their documented behaviour,
an assumption: the model is unpinned against the reference."""
import math

import numpy as np

import obs_np

F = np.float32
TAPS = np.array([7, 17, 32, 46, 52, 46, 32, 17, 7], np.int64)
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))      # (dx, dy)
DEFAULTS = dict(ring_slots=3, fast_threshold=20, keypoint_capacity=4096, window_capacity=2048)
POINT_LIMIT = 1048576.0      # 2^20


def taps_from_gaussian():
    """exp(-x^2 / 8), normalised, rounded to 8 fractional bits."""
    g = np.exp(-np.arange(-4, 5, dtype=np.float64) ** 2 / 8.0)
    return np.rint(256.0 * g / g.sum()).astype(np.int64)


# ---- K1
def blur(img):
    p = np.pad(np.asarray(img, np.uint8).astype(np.int64), 4, mode="reflect")      # (numpy's "reflect" is BORDER_REFLECT_101)
    rows, cols = np.asarray(img).shape
    h = sum(TAPS[k] * p[:, k:k + cols] for k in range(9))
    v = sum(TAPS[k] * h[k:k + rows, :] for k in range(9))
    return ((v + 32768) >> 16).astype(np.uint8)


def blur_dense(img):
    """The second statement: out[y][x] = (sum_ij k_i k_j p[y + i][x + j] + 32768) >> 16, pixel by pixel."""
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape
    p = np.pad(img.astype(np.int64), 4, mode="reflect")
    K = np.outer(TAPS, TAPS)
    out = np.zeros((rows, cols), np.uint8)
    for y in range(rows):
        for x in range(cols):
            out[y, x] = (int((K * p[y:y + 9, x:x + 9]).sum()) + 32768) >> 16
    return out


# ---- K2
def clamp_threshold(t):
    return max(0, min(255, int(t)))


def fast_scores(img, t=20):
    """[rows, cols] int: M - 1 where M > t, else 0; 0 on the frame of 3 pixels."""
    img = np.asarray(img, np.uint8).astype(np.int64)
    rows, cols = img.shape
    t = clamp_threshold(t)
    v = img[3:rows - 3, 3:cols - 3]
    d = np.stack([img[3 + dy:rows - 3 + dy, 3 + dx:cols - 3 + dx] - v for dx, dy in RING])      # [16, h, w]
    M = np.full(v.shape, -256, np.int64)
    for s in range(16):
        arc = d[[(s + k) % 16 for k in range(9)]]
        M = np.maximum(M, np.maximum(arc.min(0), (-arc).min(0)))
    out = np.zeros((rows, cols), np.int64)
    out[3:rows - 3, 3:cols - 3] = np.where(M > t, M - 1, 0)
    return out


def _corner_at(v, ring, s):
    """FAST's definition: 9 contiguous ring pixels all brighter than v + s, or all darker than v - s."""
    for r in range(16):
        arc = [ring[(r + k) % 16] for k in range(9)]
        if all(p > v + s for p in arc) or all(p < v - s for p in arc):
            return True
    return False


def fast_score_brute(img, x, y, t=20):
    """The second statement for one pixel: the largest s in 0 .. 254 at which the pixel is a corner, when it is one at t; else 0."""
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape
    if x < 3 or y < 3 or x > cols - 4 or y > rows - 4:
        return 0
    v = int(img[y, x])
    ring = [int(img[y + dy, x + dx]) for dx, dy in RING]
    if not _corner_at(v, ring, clamp_threshold(t)):
        return 0
    return max(s for s in range(255) if _corner_at(v, ring, s))


def suppress(scores):
    """The plane after the suppression: the score where it is positive and strictly above all 8 neighbours, else 0."""
    s = np.asarray(scores, np.int64)
    p = np.pad(s, 1)
    keep = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= s > p[1 + dy:1 + dy + s.shape[0], 1 + dx:1 + dx + s.shape[1]]
    return np.where(keep, s, 0).astype(np.uint8)


def fast(img, t=20, cap=4096):
    """dict(plane uint8, pts [n, 2] float32, score [n] int32, counters [4]) of one image: K2 and K3."""
    raw = fast_scores(img, t)
    plane = suppress(raw)
    ys, xs = np.nonzero(plane)      # (row-major: y, then x ascending)
    kept = len(xs)
    n = min(kept, int(cap))
    pts = np.stack([xs[:n].astype(F), ys[:n].astype(F)], 1).reshape(-1, 2)
    return dict(plane=plane, pts=pts, score=plane[ys[:n], xs[:n]].astype(np.int32), counters=np.array([int((raw > 0).sum()), kept, n, int(kept > cap)], np.int32))


# ---- K4
def pattern_ok(pattern):
    p = np.asarray(pattern)
    return p.shape == (4, 256) and bool((np.abs(p) <= 64).all())


def point_ok(pts):
    with np.errstate(invalid="ignore"):
        return (np.abs(pts[:, 0]) < F(POINT_LIMIT)) & (np.abs(pts[:, 1]) < F(POINT_LIMIT))      # (false for a NaN)


def brief(blurred, pattern, pts):
    """(desc [n, 4] uint64, the number of points of the deviation)."""
    blurred = np.asarray(blurred, np.uint8)
    rows, cols = blurred.shape
    pts = np.asarray(pts, F).reshape(-1, 2)
    pat = np.asarray(pattern, np.int32).reshape(4, 256)
    ok = point_ok(pts)
    safe = np.where(ok[:, None], pts, F(0))
    co = [(safe[:, a % 2, None] + pat[a][None, :].astype(F)).astype(F) for a in range(4)]      # x1 y1 x2 y2, one float32 addition each
    x1, y1, x2, y2 = [np.trunc(c).astype(np.int64) for c in co]      # toward zero
    inside = (x1 >= 0) & (x1 < cols) & (y1 >= 0) & (y1 < rows) & (x2 >= 0) & (x2 < cols) & (y2 >= 0) & (y2 < rows)
    cl = lambda a, n: np.clip(a, 0, n - 1)
    bits = inside & (blurred[cl(y1, rows), cl(x1, cols)] < blurred[cl(y2, rows), cl(x2, cols)]) & ok[:, None]
    w = (bits.reshape(-1, 4, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, None, :]).sum(2, dtype=np.uint64)
    return w.reshape(-1, 4), int((~ok).sum())


def _f(x):
    return float(np.float32(x))


def brief_scalar(blurred, pattern, px, py):
    """The second statement for one point: [4] Python ints."""
    rows, cols = len(blurred), len(blurred[0])
    w = [0, 0, 0, 0]
    px, py = _f(px), _f(py)
    if not (math.isfinite(px) and math.isfinite(py) and abs(px) < POINT_LIMIT and abs(py) < POINT_LIMIT):
        return w
    for i in range(256):
        c = [int(_f((px if a % 2 == 0 else py) + float(pattern[a][i]))) for a in range(4)]      # (the sum of two floats, rounded to float; int() is toward zero)
        x1, y1, x2, y2 = c
        if 0 <= x1 < cols and 0 <= y1 < rows and 0 <= x2 < cols and 0 <= y2 < rows and int(blurred[y1][x1]) < int(blurred[y2][x2]):
            w[i // 64] |= 1 << (i % 64)
    return w


# ---- K5
def norm(cam8, pts):
    return obs_np.lift(obs_np.camera(cam8), np.asarray(pts, F).reshape(-1, 2))


# ---- a keyframe
def extract(img, pattern, cam8, t=20, cap=4096):
    """What gfbe_kfd_extract leaves for one camera: dict(blurred, plane, pts, score, pts_norm, desc, counters)."""
    out = fast(img, t, cap)
    out["blurred"] = blur(img)
    out["desc"], bad = brief(out["blurred"], pattern, out["pts"])
    assert bad == 0
    out["pts_norm"] = norm(cam8, out["pts"])
    return out


def hamming(a, b):
    """[n] distances of two [n, 4] uint64 descriptor arrays."""
    x = np.bitwise_xor(np.asarray(a, np.uint64), np.asarray(b, np.uint64))
    return np.unpackbits(x.view(np.uint8).reshape(len(x), -1), axis=1).sum(1)
