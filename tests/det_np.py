"""TEST INFRASTRUCTURE. The model of the corner detector (include/gfbe_det.h, rules G1 .. G5) in numpy: integer arrays for every
sum, np.float32 for every float statement in the order the header writes it. Each rule has a second, independent statement
(scipy.ndimage correlations for G2, maximum_filter for the local maximum, an all-pairs matrix for the walk, a rasterised mask for
G1); tests/test_det_model.py holds the pairs against each other bit for bit."""
import numpy as np

from klt_np import kround

F = np.float32
DEFAULTS = dict(max_cnt=150, min_dist=30, candidate_capacity=0, sort_chunk=512, quality=0.01)
S2 = F((1.0 / (4.0 * 3.0 * 255.0)) * (1.0 / (4.0 * 3.0 * 255.0)))
SOBEL_X = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.int64)


# ---- G2
def _box3(p):
    """the 3 x 3 sums of an integer plane reflected without its edge"""
    q = np.pad(p, 1, mode="reflect")
    h, w = p.shape
    return sum(q[j:j + h, i:i + w] for j in range(3) for i in range(3))


def sums(image):
    """A, B, C of every pixel (int64)."""
    q = np.pad(np.asarray(image, np.int64), 1, mode="reflect")
    h, w = image.shape
    s = lambda j, i: q[1 + j:1 + j + h, 1 + i:1 + i + w]
    dx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    dy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    return _box3(dx * dx), _box3(dx * dy), _box3(dy * dy)


def sums_ndimage(image):
    """The same by scipy.ndimage correlations, mode "mirror" (BORDER_REFLECT_101)."""
    from scipy import ndimage
    im = np.asarray(image, np.int64)
    dx, dy = ndimage.correlate(im, SOBEL_X, mode="mirror"), ndimage.correlate(im, SOBEL_X.T, mode="mirror")
    box = lambda p: ndimage.correlate(p, np.ones((3, 3), np.int64), mode="mirror")
    return box(dx * dx), box(dx * dy), box(dy * dy)


def eig_of(A, B, C):
    assert max(np.abs(A).max(), np.abs(B).max(), np.abs(C).max()) < 1 << 24      # their conversion to float is exact
    a, b, c = F(0.5) * (A.astype(F) * S2), B.astype(F) * S2, F(0.5) * (C.astype(F) * S2)
    d = a - c
    return ((a + c) - np.sqrt(d * d + b * b)).astype(F)


def response(image):
    return eig_of(*sums(image))


# ---- G1
def pixel(p):
    return kround(F(p[0])), kround(F(p[1]))


def set_mask(pts, track_cnt, rows, cols, min_dist):
    """dict(order: list indices of the kept points in the order kept, xy [kept, 2] their pixels)."""
    order = np.argsort(-np.asarray(track_cnt, np.int64), kind="stable")
    r2 = int(min_dist) ** 2
    keep, xy = [], np.zeros((0, 2), np.int64)
    for i in order:
        px, py = pixel(pts[i])
        if not (0 <= px < cols and 0 <= py < rows):
            continue
        if len(xy) and (((xy[:, 0] - px) ** 2 + (xy[:, 1] - py) ** 2) <= r2).any():
            continue
        keep.append(int(i))
        xy = np.concatenate([xy, [[px, py]]])
    return dict(order=np.array(keep, np.int64), xy=xy)


def fill_disc(mask, px, py, r):
    """cv::circle(mask, p, r, 0, -1) as the row spans of the disc dx^2 + dy^2 <= r^2, clipped to the image"""
    rows, cols = mask.shape
    for dy in range(-r, r + 1):
        y = py + dy
        if not 0 <= y < rows:
            continue
        half = int(np.floor(np.sqrt(r * r - dy * dy) + 1e-9))
        while half * half + dy * dy > r * r:
            half -= 1
        while (half + 1) ** 2 + dy * dy <= r * r:
            half += 1
        mask[y, max(px - half, 0):max(min(px + half + 1, cols), 0)] = 0


def set_mask_raster(pts, track_cnt, rows, cols, min_dist):
    """setMask as the reference writes it: a mask image, read at the pixel and drawn into. Returns (order, mask)."""
    cnt = np.asarray(track_cnt, np.int64)
    order = sorted(range(len(cnt)), key=lambda i: (-int(cnt[i]), i))
    mask = np.full((rows, cols), 255, np.uint8)
    keep = []
    for i in order:
        px, py = pixel(pts[i])
        if 0 <= px < cols and 0 <= py < rows and mask[py, px] == 255:
            keep.append(i)
            fill_disc(mask, px, py, int(min_dist))
    return np.array(keep, np.int64), mask


def clear_mask(xy, rows, cols, min_dist):
    """255 where a pixel lies in no kept point's disc, else 0: the mask without an image of it being drawn"""
    m = np.full((rows, cols), 255, np.uint8)
    r = int(min_dist)
    for px, py in np.asarray(xy, np.int64).reshape(-1, 2):
        y0, y1, x0, x1 = max(py - r, 0), min(py + r + 1, rows), max(px - r, 0), min(px + r + 1, cols)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        m[y0:y1, x0:x1][(xx - px) ** 2 + (yy - py) ** 2 <= r * r] = 0
    return m


# ---- G3
def threshold(max_val, quality):
    return F(np.float64(max_val) * np.float64(quality))


def local_max(eig, t):
    """the largest thresholded value of the 3 x 3 neighbours inside the image, at every pixel"""
    th = np.where(eig > t, eig, F(0)).astype(F)
    q = np.pad(th, 1, mode="constant", constant_values=-np.inf)
    h, w = eig.shape
    return np.max([q[j:j + h, i:i + w] for j in range(3) for i in range(3)], axis=0).astype(F)


def local_max_filter(eig, t):
    from scipy import ndimage
    th = np.where(eig > t, eig, F(0)).astype(F)
    return ndimage.maximum_filter(th, size=3, mode="constant", cval=-np.inf)


def candidates(eig, mask, quality, lmax=local_max):
    """dict(x, y, eig) of the candidates in the order of G3 (descending eig, the larger y * cols + x first), t, max_val (None: no clear pixel)."""
    rows, cols = eig.shape
    clear = mask == 255
    empty = dict(x=np.zeros(0, np.int64), y=np.zeros(0, np.int64), eig=np.zeros(0, F), t=None, max_val=None)
    if not clear.any():
        return empty
    max_val = eig[clear].max()
    t = threshold(max_val, quality)
    ok = clear & (eig > t) & (eig != 0) & (eig == lmax(eig, t))
    ok[0, :] = ok[-1, :] = False
    ok[:, 0] = ok[:, -1] = False
    idx = np.flatnonzero(ok)
    v = eig.ravel()[idx]
    o = np.lexsort((idx, v))[::-1]
    idx, v = idx[o], v[o]
    return dict(x=idx % cols, y=idx // cols, eig=v.astype(F), t=t, max_val=max_val)


def walk(x, y, min_dist, max_corners):
    """the indices (into the ordered candidates) of the accepted corners"""
    r2, acc = int(min_dist) ** 2, []
    ax, ay = np.zeros(0, np.int64), np.zeros(0, np.int64)
    for i in range(len(x)):
        if len(acc) >= max_corners:
            break
        if len(acc) and (((ax - x[i]) ** 2 + (ay - y[i]) ** 2) < r2).any():
            continue
        acc.append(i)
        ax, ay = np.append(ax, x[i]), np.append(ay, y[i])
    return np.array(acc, np.int64)


def walk_all_pairs(x, y, min_dist, max_corners):
    """The same from the matrix of all pairs: candidate i is accepted when no accepted j < i conflicts with it."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    conflict = ((x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2) < int(min_dist) ** 2
    accepted = np.zeros(len(x), bool)
    n = 0
    for i in range(len(x)):
        if n >= max_corners:
            break
        if not (conflict[i, :i] & accepted[:i]).any():
            accepted[i] = True
            n += 1
    return np.flatnonzero(accepted)


# ---- the calls
def corners(image, max_corners, quality=0.01, min_dist=10, candidate_capacity=0):
    """gfbe_det_corners of one camera: dict(pts [n, 2] float32, response [n], n_candidates, overflow)."""
    eig = response(image)
    c = candidates(eig, np.full(eig.shape, 255, np.uint8), quality)
    over = bool(candidate_capacity > 0 and len(c["x"]) > candidate_capacity)
    a = np.zeros(0, np.int64) if over else walk(c["x"], c["y"], min_dist, max_corners)
    return dict(pts=np.stack([c["x"][a], c["y"][a]], 1).astype(F).reshape(-1, 2), response=c["eig"][a], n_candidates=len(c["x"]), overflow=over)


def detect(image, pts, ids, track_cnt, next_id=0, **options):
    """gfbe_det_detect of one camera: dict(pts, ids, track_cnt, counters [6], next_id, eig, mask, kept_order, cand: the ordered
    candidates, accepted: indices into them)."""
    o = dict(DEFAULTS, **options)
    rows, cols = image.shape
    pts, ids, cnt = np.asarray(pts, F).reshape(-1, 2), np.asarray(ids, np.int32), np.asarray(track_cnt, np.int32)
    g1 = set_mask(pts, cnt, rows, cols, o["min_dist"])
    kept = len(g1["order"])
    mask = clear_mask(g1["xy"], rows, cols, o["min_dist"])
    eig = response(image)
    want = o["max_cnt"] - kept
    cand = dict(x=np.zeros(0, np.int64), y=np.zeros(0, np.int64), eig=np.zeros(0, F), t=None, max_val=None)
    acc, over = np.zeros(0, np.int64), False
    if want > 0:
        cand = candidates(eig, mask, o["quality"])
        over = bool(o["candidate_capacity"] > 0 and len(cand["x"]) > o["candidate_capacity"])
        if not over:
            acc = walk(cand["x"], cand["y"], o["min_dist"], want)
    new = np.stack([cand["x"][acc], cand["y"][acc]], 1).astype(F).reshape(-1, 2)
    out_pts = np.concatenate([pts[g1["order"]], new]).astype(F)
    out_ids = np.concatenate([ids[g1["order"]], next_id + np.arange(len(acc))]).astype(np.int32)
    out_cnt = np.concatenate([cnt[g1["order"]], np.ones(len(acc))]).astype(np.int32)
    nid = int(next_id) + len(acc)
    return dict(pts=out_pts, ids=out_ids, track_cnt=out_cnt, counters=np.array([len(pts), kept, len(cand["x"]), len(acc), nid, int(over)], np.int32), next_id=nid,
                eig=eig, mask=mask, kept_order=g1["order"], kept_xy=g1["xy"], cand=cand, accepted=acc)
