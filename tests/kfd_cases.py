"""TEST INFRASTRUCTURE. The cases of the keyframe descriptors (include/gfbe_kfd.h) for tests/test_kfd_model.py (the two statements of the
model against each other, the host build of csrc/gfbe_kfd.h against the model) and tests/test_gpu_kfd.py (the device against the
model), and what the model tests/kfd_np.py gives for them, computed once."""
import functools
import json
import os

import numpy as np

from _gfbe_import import gf
import kfd_np as m
import obs_cases as oc

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brief_pattern.json")
SIZES = ((7, 7), (48, 64), (61, 97))      # (rows, cols): the single legal centre pixel; a tile's width; no size a multiple of a tile
BIG = (480, 640)
FLAT = 100
PLANT_CAP = 80                            # keypoint_capacity of the planted cases
PLANT_COUNTS = (0, 1, 63, 64, 65, PLANT_CAP, PLANT_CAP + 1)
CAMERAS = dict(plain=oc.NO_DISTORTION, distorted=oc.golden_cameras()["idc_cam.yaml"])


@functools.lru_cache(maxsize=None)
def pattern():
    """[4, 256] int32: x1, y1, x2, y2 of the reference's brief_pattern.yml."""
    d = json.load(open(GOLDEN))
    return np.array([d[k] for k in ("x1", "y1", "x2", "y2")], np.int32)


@functools.lru_cache(maxsize=None)
def texture(rows, cols, seed=0):
    """synth.klt_texture(rows, cols, seed), read-only (64 x 48 has 20 kept corners at t = 20, 97 x 61 has 54, 640 x 480 has 3 192; 7 x 7 none)."""
    img = gf.synth.klt_texture(rows, cols, seed=seed)
    img.setflags(write=False)
    return img


def plant_positions(rows, cols, step=7):
    """(x, y) of isolated pixels, row-major, `step` apart and 3 from the edges: no ring holds two of them side by side."""
    return [(x, y) for y in range(3, rows - 3, step) for x in range(3, cols - 3, step)]


def planted(rows, cols, n):
    """A flat image with n isolated bright pixels of differing values: exactly n kept corners, pixel k with score value - FLAT - 1."""
    img = np.full((rows, cols), FLAT, np.uint8)
    pos = plant_positions(rows, cols)
    assert n <= len(pos)
    for k, (x, y) in enumerate(pos[:n]):
        img[y, x] = 150 + (k * 7) % 100
    return img


def plateau(rows=48, cols=64):
    """Two equal adjacent bright pixels (neither survives), and one lone pixel that does."""
    img = np.full((rows, cols), FLAT, np.uint8)
    img[20, 30] = img[20, 31] = 200
    img[30, 10] = 180
    return img


def edges(rows=48, cols=64):
    """Corners on the first and last column and row that have a ring: their BRIEF pairs leave the image."""
    img = np.full((rows, cols), FLAT, np.uint8)
    for x, y, v in ((3, 20, 210), (cols - 4, 25, 190), (30, 3, 170), (35, rows - 4, 230), (3, 3, 220), (cols - 4, rows - 4, 160)):
        img[y, x] = v
    return img


def window_points(rows, cols):
    """Window points of describe: fractional, negative, on and beyond every edge, the -0.5 case, non-finite and huge."""
    r, c = float(rows), float(cols)
    return np.array([[10.25, 11.75], [-0.5, 5.0], [5.0, -0.5], [-0.5, -0.5], [-1.0, 4.0], [0.0, 0.0], [c - 1, r - 1], [c - 0.5, r - 0.5], [c, r], [c + 30, 7.0],
                     [c / 2, r / 2], [c / 2 + 0.999, r / 2 - 0.001], [-30.0, -30.0], [np.nan, 5.0], [5.0, np.inf], [-np.inf, np.nan], [1048576.0, 3.0], [3.0, -1048576.0],
                     [1048575.0, 3.0], [3e9, 3e9], [c - 24.5, r - 24.5], [23.5, 23.5]], F)


@functools.lru_cache(maxsize=None)
def expected(rows, cols, seed, camera="plain", t=20, cap=4096):
    """kfd_np.extract of texture(rows, cols, seed): computed once, shared, left unchanged."""
    return m.extract(texture(rows, cols, seed), pattern(), CAMERAS[camera], t, cap)


def expected_of(img, camera="plain", t=20, cap=4096):
    return m.extract(img, pattern(), CAMERAS[camera], t, cap)
