"""TEST INFRASTRUCTURE. The model of the image equalisation (include/gfbe_eq.h, rules E1 .. E6): CLAHE of an 8-bit, one-channel image
as OpenCV documents it, each of E1 .. E5 in two statements that tests/test_eq_model.py holds against each other bit for bit:

  *_loop   statement for statement as the header words the rules: a materialised extended image, one tile, one bin, one column and
           one row at a time, the sequential residual loop, scalar single-precision arithmetic;
  (plain)  vectorised: reflected indices instead of an extended image, all tiles at once, the closed-form residual.

The device (tests/test_gpu_eq.py) and the host build of csrc/gfbe_eq.h are held against the plain form. Everything up to the LUT is
integer; E5 is IEEE single precision in a fixed order, written with numpy float32 values so that nothing is fused or widened."""
import numpy as np

F = np.float32
BINS = 256


# ---- E1 ---------------------------------------------------------------------------------------------------------------------------
def geometry(rows, cols, tiles_x=8, tiles_y=8, clip_limit=40.0):
    """dict(ext, ext_rows, ext_cols, tw, th, area, limit (0: no clipping), scale, inv_tw, inv_th)."""
    assert 1 <= tiles_x <= 64 and 1 <= tiles_y <= 64 and rows > tiles_y and cols > tiles_x and clip_limit >= 0.0
    ext = cols % tiles_x != 0 or rows % tiles_y != 0
    ext_rows = rows + (tiles_y - rows % tiles_y) if ext else rows
    ext_cols = cols + (tiles_x - cols % tiles_x) if ext else cols
    tw, th = ext_cols // tiles_x, ext_rows // tiles_y
    area = tw * th
    limit = 0
    if clip_limit > 0.0:
        q = float(clip_limit) * float(area) / 256.0
        limit = area if q >= area else max(int(q), 1)
    return dict(ext=ext, ext_rows=ext_rows, ext_cols=ext_cols, tw=tw, th=th, area=area, limit=limit, scale=F(255.0) / F(area), inv_tw=F(1.0) / F(tw), inv_th=F(1.0) / F(th))


def reflect101(i, n):
    i = np.asarray(i)
    return np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def extended_loop(img, g):
    """The extended image, materialised (BORDER_REFLECT_101 at the bottom and the right)."""
    rows, cols = img.shape
    if not g["ext"]:
        return img
    out = np.zeros((g["ext_rows"], g["ext_cols"]), np.uint8)
    for y in range(g["ext_rows"]):
        sy = y if y < rows else 2 * rows - 2 - y
        for x in range(g["ext_cols"]):
            out[y, x] = img[sy, x if x < cols else 2 * cols - 2 - x]
    return out


# ---- E2, E3 -----------------------------------------------------------------------------------------------------------------------
def hists_loop(img, tiles_x=8, tiles_y=8, clip_limit=40.0):
    """[tiles_y, tiles_x, 256] int64: the histograms after the clip and the redistribution."""
    g = geometry(*img.shape, tiles_x, tiles_y, clip_limit)
    big = extended_loop(img, g)
    out = np.zeros((tiles_y, tiles_x, BINS), np.int64)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            hist = [0] * BINS
            for v in big[ty * g["th"]:(ty + 1) * g["th"], tx * g["tw"]:(tx + 1) * g["tw"]].ravel().tolist():
                hist[v] += 1
            if clip_limit > 0.0:
                limit, clipped = g["limit"], 0
                for i in range(BINS):
                    if hist[i] > limit:
                        clipped += hist[i] - limit
                        hist[i] = limit
                batch, residual = clipped // BINS, clipped % BINS
                for i in range(BINS):
                    hist[i] += batch
                if residual > 0:
                    step = max(BINS // residual, 1)
                    i = 0
                    while i < BINS and residual > 0:
                        hist[i] += 1
                        i += step
                        residual -= 1
            out[ty, tx] = hist
    return out


def hists(img, tiles_x=8, tiles_y=8, clip_limit=40.0):
    rows, cols = img.shape
    g = geometry(rows, cols, tiles_x, tiles_y, clip_limit)
    yi, xi = reflect101(np.arange(g["ext_rows"]), rows), reflect101(np.arange(g["ext_cols"]), cols)
    tile_of = (np.arange(g["ext_rows"]) // g["th"])[:, None] * tiles_x + (np.arange(g["ext_cols"]) // g["tw"])[None, :]
    h = np.bincount((tile_of * BINS + img[yi][:, xi].astype(np.int64)).ravel(), minlength=tiles_x * tiles_y * BINS).reshape(tiles_y * tiles_x, BINS).astype(np.int64)
    if g["limit"] > 0:
        clipped = np.maximum(h - g["limit"], 0).sum(1)
        residual = clipped % BINS
        step = np.maximum(BINS // np.maximum(residual, 1), 1)
        i = np.arange(BINS)[None, :]
        h = np.minimum(h, g["limit"]) + (clipped // BINS)[:, None] + ((i % step[:, None] == 0) & (i // step[:, None] < residual[:, None]))
    return h.reshape(tiles_y, tiles_x, BINS)


# ---- E4 ---------------------------------------------------------------------------------------------------------------------------
def luts_loop(img, tiles_x=8, tiles_y=8, clip_limit=40.0):
    g = geometry(*img.shape, tiles_x, tiles_y, clip_limit)
    h = hists_loop(img, tiles_x, tiles_y, clip_limit)
    out = np.zeros((tiles_y, tiles_x, BINS), np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            s = 0
            for i in range(BINS):
                s += int(h[ty, tx, i])
                out[ty, tx, i] = min(max(int(np.rint(F(s) * g["scale"])), 0), 255)
    return out


def luts(img, tiles_x=8, tiles_y=8, clip_limit=40.0):
    """[tiles_y, tiles_x, 256] uint8."""
    g = geometry(*img.shape, tiles_x, tiles_y, clip_limit)
    s = np.cumsum(hists(img, tiles_x, tiles_y, clip_limit), axis=2)
    return np.clip(np.rint(s.astype(F) * g["scale"]), 0, 255).astype(np.uint8)


# ---- E5 ---------------------------------------------------------------------------------------------------------------------------
def axis_loop(n, inv_t, tiles):
    """Per index 0 .. n - 1: (t1, t2, a, a1), one index at a time in scalar single precision."""
    t1s, t2s, a_s, a1s = [], [], [], []
    for x in range(n):
        tf = F(x) * inv_t - F(0.5)
        t1 = int(np.floor(tf))
        a = tf - F(t1)
        a1 = F(1.0) - a
        t2 = t1 + 1
        t1s.append(max(t1, 0)), t2s.append(min(t2, tiles - 1)), a_s.append(a), a1s.append(a1)
    return np.array(t1s), np.array(t2s), np.array(a_s, F), np.array(a1s, F)


def axis(n, inv_t, tiles):
    tf = np.arange(n).astype(F) * inv_t - F(0.5)
    t1 = np.floor(tf)
    a = tf - t1
    t1 = t1.astype(np.int64)
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a.astype(F), (F(1.0) - a).astype(F)


def interp_pixel(img, lut, g, tiles_x, tiles_y, x, y):
    """E5 for one pixel, every value a scalar."""
    tx1, tx2, xa, xa1 = (q[x] for q in axis_loop(x + 1, g["inv_tw"], tiles_x))
    ty1, ty2, ya, ya1 = (q[y] for q in axis_loop(y + 1, g["inv_th"], tiles_y))
    v = int(img[y, x])
    res = (F(lut[ty1, tx1, v]) * xa1 + F(lut[ty1, tx2, v]) * xa) * ya1 + (F(lut[ty2, tx1, v]) * xa1 + F(lut[ty2, tx2, v]) * xa) * ya
    return min(max(int(np.rint(res)), 0), 255)


def interpolate_loop(img, lut, tiles_x=8, tiles_y=8):
    """A row at a time, with the coefficients of axis_loop."""
    rows, cols = img.shape
    g = geometry(rows, cols, tiles_x, tiles_y)
    tx1, tx2, xa, xa1 = axis_loop(cols, g["inv_tw"], tiles_x)
    ty1, ty2, ya, ya1 = axis_loop(rows, g["inv_th"], tiles_y)
    out = np.zeros_like(img)
    for y in range(rows):
        v = img[y].astype(np.int64)
        top = lut[ty1[y], tx1, v].astype(F) * xa1 + lut[ty1[y], tx2, v].astype(F) * xa
        bottom = lut[ty2[y], tx1, v].astype(F) * xa1 + lut[ty2[y], tx2, v].astype(F) * xa
        out[y] = np.clip(np.rint(top * ya1[y] + bottom * ya[y]), 0, 255).astype(np.uint8)
    return out


def interpolate(img, lut, tiles_x=8, tiles_y=8):
    rows, cols = img.shape
    g = geometry(rows, cols, tiles_x, tiles_y)
    tx1, tx2, xa, xa1 = axis(cols, g["inv_tw"], tiles_x)
    ty1, ty2, ya, ya1 = axis(rows, g["inv_th"], tiles_y)
    v = img.astype(np.int64)
    top = lut[ty1[:, None], tx1[None, :], v].astype(F) * xa1[None, :] + lut[ty1[:, None], tx2[None, :], v].astype(F) * xa[None, :]
    bottom = lut[ty2[:, None], tx1[None, :], v].astype(F) * xa1[None, :] + lut[ty2[:, None], tx2[None, :], v].astype(F) * xa[None, :]
    return np.clip(np.rint(top * ya1[:, None] + bottom * ya[:, None]), 0, 255).astype(np.uint8)


# ---- E1 .. E6 ---------------------------------------------------------------------------------------------------------------------
def equalize_loop(img, tiles_x=8, tiles_y=8, clip_limit=40.0):
    lut = luts_loop(img, tiles_x, tiles_y, clip_limit)
    return interpolate_loop(img, lut, tiles_x, tiles_y), lut


def equalize(img, tiles_x=8, tiles_y=8, clip_limit=40.0):
    """(equalised image [rows, cols] uint8, LUTs [tiles_y, tiles_x, 256] uint8) of one image."""
    lut = luts(img, tiles_x, tiles_y, clip_limit)
    return interpolate(img, lut, tiles_x, tiles_y), lut


def equalize_stack(imgs, tiles_x=8, tiles_y=8, clip_limit=40.0):
    """([n, rows, cols], [n, tiles_y, tiles_x, 256]) of a stack of images, each on its own."""
    res = [equalize(im, tiles_x, tiles_y, clip_limit) for im in imgs]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
