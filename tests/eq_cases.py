"""TEST INFRASTRUCTURE. The cases of the image equalisation (include/gfbe_eq.h) for tests/test_eq_model.py (the two statements of the
model against each other, the host build of csrc/gfbe_eq.h against the model) and tests/test_gpu_eq.py (the device against the model),
and what the model tests/eq_np.py gives for them, computed once."""
import functools

import numpy as np

from _gfbe_import import gf
import eq_np as m

# (rows, cols, tiles_x, tiles_y, clip_limit)
SHAPES = (
    (16, 16, 8, 8, 40.0),       # tile 2 x 2, limit 1, a residual
    (9, 9, 8, 8, 40.0),         # the largest legal padding
    (17, 23, 8, 8, 40.0),       # both dimensions padded
    (24, 20, 8, 8, 40.0),       # rows divisible, and yet padded by 8
    (61, 97, 8, 8, 3.0),
    (61, 97, 1, 1, 40.0),       # both clamps coincide
    (61, 97, 8, 8, 0.0),        # no clipping
    (33, 47, 5, 3, 2.0),
    (120, 188, 8, 8, 40.0),
)
BIG = (480, 752, 8, 8, 40.0)    # the model and the host build only
KINDS = ("texture", "ramp", "constant", "saturated")
N_CAMERAS = (1, 3, 65)


def shape_id(s):
    return "%dx%d_t%dx%d_c%g" % s


@functools.lru_cache(maxsize=None)
def image(kind, rows, cols, seed=0):
    """Read-only uint8 [rows, cols]: seeded texture; a narrow-range ramp (x + y) % 64 + 90, which clips hard; a constant image; a
    saturated image of 0 and 255."""
    if kind == "texture":
        img = np.array(gf.synth.klt_texture(rows, cols, seed=seed), np.uint8)
    elif kind == "ramp":
        y, x = np.mgrid[0:rows, 0:cols]
        img = ((x + y + seed) % 64 + 90).astype(np.uint8)
    elif kind == "constant":
        img = np.full((rows, cols), (137 + 31 * seed) % 256, np.uint8)
    elif kind == "saturated":
        img = (np.random.default_rng(1000 + seed).integers(0, 2, (rows, cols)) * 255).astype(np.uint8)
    else:
        raise KeyError(kind)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def stack(rows, cols, n):
    """n images of rows x cols, read-only: the four kinds in turn, with different seeds."""
    s = np.stack([image(KINDS[k % 4], rows, cols, k // 4) for k in range(n)])
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def expected(shape, n):
    """eq_np.equalize_stack of stack(rows, cols, n) with the shape's options: (images, LUTs), computed once, shared, left unchanged."""
    rows, cols, tx, ty, clip = shape
    out, lut = m.equalize_stack(stack(rows, cols, n), tx, ty, clip)
    out.setflags(write=False)
    lut.setflags(write=False)
    return out, lut
