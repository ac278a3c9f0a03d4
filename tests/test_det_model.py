"""The corner detector without a GPU: the model (tests/det_np.py) against its own second statements of G1, G2, the local maximum and
the walk, bit for bit; the host build of ground-fusion2_amd/csrc/gfbe_det.h (tests/det_host_shim.cpp) against the model on every case,
bit for bit, with the branches the cases must reach; the walk's boundary on synthetic candidate lists; the same header under the
address and undefined-behaviour sanitizers in a program of its own (tests/det_host_main.cpp); a property test of the model alone on
planted corners; the binding (include/gfbe_det.h against signatures.DET, the layout of gfbe_det_options against a compiled C
program); and the C ABI's refusals without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import det_cases as dc
import det_np as m

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
HDRS = [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_det.h", "gfbe_klt.h")]
PF, PI, PU8, PU64 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
F = np.float32


def _cxx(src, out, extra):
    if not CXX:
        pytest.fail("no C++ compiler: gfbe_det.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + HDRS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_cxx(os.path.join(ROOT, "tests", "det_host_shim.cpp"), os.path.join(BUILD, "det_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_det_mask.argtypes = [C.c_int, PF, PI, C.c_int, C.c_int, C.c_int, PI, PI]
    lib.shim_det_planes.argtypes = [PU8, C.c_int, C.c_int, C.c_int, PI, C.c_int, PF, PU8]
    lib.shim_det_candidates.argtypes = [PF, C.c_int, C.c_int, C.c_int, PI, C.c_int, C.c_double, PU64, C.c_int]
    lib.shim_det_key.argtypes = [C.c_float, C.c_int]
    lib.shim_det_key.restype = C.c_uint64
    lib.shim_det_key_response.argtypes = [C.c_uint64]
    lib.shim_det_key_response.restype = C.c_float
    lib.shim_det_walk.argtypes = [PU64, C.c_int, C.c_int, C.c_int, C.c_int, PI, PF]
    lib.shim_det_corners.argtypes = [PU8, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, PF, PF, PI]
    lib.shim_det_detect.argtypes = [PU8, C.c_int, C.c_int, C.c_int, PF, PI, PI, C.c_int, C.c_int, C.c_double, C.c_int, PI, PF, PI, PI, PI]
    return lib


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_the_header_has_no_hip_in_it():
    src = open(HDRS[0]).read()
    assert "hip/hip_runtime" not in src and "hipLaunch" not in src and "__global__" not in src


# ---- the model against its second statements
IMAGES = [dc.texture(23, 23, 1), dc.texture(48, 64, 2), dc.noise(89, 91, 3), dc.squares(177, 180, 4)[0], dc.periodic(48, 64), dc.border_peaks(48, 64)[0], dc.border_peaks(48, 64)[1],
          np.full((30, 40), 255, np.uint8)]


@pytest.mark.parametrize("k", range(len(IMAGES)))
def test_two_statements_of_the_response_and_the_local_maximum_agree(k):
    im = IMAGES[k]
    a, b = m.sums(im), m.sums_ndimage(im)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    eig = m.response(im)
    assert eig.dtype == np.float32
    for q in (0.0, 0.01, 0.5):
        t = m.threshold(eig.max(), q)
        assert np.array_equal(_bits(m.local_max(eig, t)), _bits(m.local_max_filter(eig, t)))
        c1 = m.candidates(eig, np.full(eig.shape, 255, np.uint8), q)
        c2 = m.candidates(eig, np.full(eig.shape, 255, np.uint8), q, lmax=m.local_max_filter)
        assert np.array_equal(c1["x"], c2["x"]) and np.array_equal(c1["y"], c2["y"])


def test_the_sign_of_the_mixed_sum_at_the_border_is_the_reflected_planes():
    """B next to the border differs when the derivative is taken on the padded image instead of the planes being reflected: the
    model follows cornerMinEigenVal (boxFilter reflects the planes), as the ndimage statement does by construction."""
    im = dc.noise(30, 33, 1)
    q = np.pad(im.astype(np.int64), 2, mode="reflect")
    h, w = im.shape
    s = lambda j, i: q[2 + j - 1:2 + j + h + 1, 2 + i - 1:2 + i + w + 1]
    dx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    dy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    p = dx * dy
    wrong = sum(p[j:j + h, i:i + w] for j in range(3) for i in range(3))
    B = m.sums(im)[1]
    assert np.array_equal(wrong[1:-1, 1:-1], B[1:-1, 1:-1]) and not np.array_equal(wrong, B)


@pytest.mark.parametrize("r", [0, 1, 2, 3, 5, 10, 30])
def test_two_statements_of_the_mask_agree(r):
    rows, cols = 48, 64
    pts, _, cnt = dc._special_held(rows, cols)
    a = m.set_mask(pts, cnt, rows, cols, r)
    order, mask = m.set_mask_raster(pts, cnt, rows, cols, r)
    assert np.array_equal(a["order"], order) and np.array_equal(m.clear_mask(a["xy"], rows, cols, r), mask)
    # a disc's row spans, clipped at every edge, against the inequality
    one = np.full((rows, cols), 255, np.uint8)
    m.fill_disc(one, 2, rows - 2, r)
    yy, xx = np.mgrid[0:rows, 0:cols]
    assert np.array_equal(one == 0, (xx - 2) ** 2 + (yy - (rows - 2)) ** 2 <= r * r)


@pytest.mark.parametrize("name", ["noise_default_chunk", "periodic", "s64x48_three_cameras", "s91x89_min_dist_30"])
def test_two_statements_of_the_walk_agree(name):
    for k, r in enumerate(dc.expected(name)[0]):
        c = r["cand"]
        o = dict(m.DEFAULTS, **dc.case(name)["options"])
        for md, mc in ((o["min_dist"], o["max_cnt"] - r["counters"][1]), (0, 10 ** 6), (1, 10 ** 6), (7, 31)):
            assert np.array_equal(m.walk(c["x"], c["y"], md, mc), m.walk_all_pairs(c["x"], c["y"], md, mc)), (k, md, mc)


# ---- the host build against the model
def _host_detect(shim, im, pts, ids, cnt, nid, o):
    im = np.ascontiguousarray(im, np.uint8)
    p, i_, n_ = np.ascontiguousarray(pts, np.float32).reshape(-1, 2), np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(cnt, np.int32)
    n = len(p)
    room = max(n, o["max_cnt"])
    po, io, no, cn, nx = np.zeros((room, 2), np.float32), np.zeros(room, np.int32), np.zeros(room, np.int32), np.zeros(6, np.int32), np.array([nid], np.int32)
    tot = shim.shim_det_detect(im.ctypes.data_as(PU8), im.shape[1], im.shape[0], n, p.ctypes.data_as(PF), i_.ctypes.data_as(PI), n_.ctypes.data_as(PI), o["max_cnt"],
                               o["min_dist"], o["quality"], o["candidate_capacity"], nx.ctypes.data_as(PI), po.ctypes.data_as(PF), io.ctypes.data_as(PI), no.ctypes.data_as(PI),
                               cn.ctypes.data_as(PI))
    return dict(pts=po[:tot], ids=io[:tot], track_cnt=no[:tot], counters=cn, next_id=int(nx[0]))


@pytest.mark.parametrize("name", dc.NAMES)
def test_host_detect_is_the_models(shim, name):
    c, want = dc.case(name), dc.expected(name)
    o = dict(m.DEFAULTS, **c["options"])
    held = [(c["pts"][k], c["ids"][k], c["cnt"][k]) for k in range(len(c["pts"]))]
    nid = list(c["next_id"])
    for f, per_cam in enumerate(want):
        nxt = []
        for k, w in enumerate(per_cam):
            g = _host_detect(shim, c["images"][f][k], held[k][0], held[k][1], held[k][2], nid[k], o)
            assert np.array_equal(g["counters"], w["counters"]), (f, k, g["counters"], w["counters"])
            assert np.array_equal(_bits(g["pts"]), _bits(w["pts"])) and np.array_equal(g["ids"], w["ids"]) and np.array_equal(g["track_cnt"], w["track_cnt"]), (f, k)
            nxt.append((g["pts"].copy(), g["ids"].copy(), g["track_cnt"].copy()))
            nid[k] = g["next_id"]
        held = nxt


@pytest.mark.parametrize("name", dc.NAMES)
def test_host_planes_candidates_and_corners_are_the_models(shim, name):
    c, want, wc = dc.case(name), dc.expected(name)[0], dc.expected_corners(name)
    o = dict(m.DEFAULTS, **c["options"])
    rows, cols = c["rows"], c["cols"]
    for k, w in enumerate(want):
        im = np.ascontiguousarray(c["images"][0][k])
        p, n_ = np.ascontiguousarray(c["pts"][k], np.float32), np.ascontiguousarray(c["cnt"][k], np.int32)
        order, kxy = np.zeros(max(len(p), 1), np.int32), np.zeros((max(len(p), 1), 2), np.int32)
        kept = shim.shim_det_mask(len(p), p.ctypes.data_as(PF), n_.ctypes.data_as(PI), cols, rows, o["min_dist"], order.ctypes.data_as(PI), kxy.ctypes.data_as(PI))
        assert np.array_equal(order[:kept], w["kept_order"]) and np.array_equal(kxy[:kept], w["kept_xy"])
        eig, mask = np.zeros((rows, cols), np.float32), np.zeros((rows, cols), np.uint8)
        shim.shim_det_planes(im.ctypes.data_as(PU8), cols, rows, kept, kxy.ctypes.data_as(PI), o["min_dist"], eig.ctypes.data_as(PF), mask.ctypes.data_as(PU8))
        assert np.array_equal(_bits(eig), _bits(w["eig"])) and np.array_equal(mask, w["mask"])
        if w["counters"][1] < o["max_cnt"]:
            keys = np.zeros(max(len(w["cand"]["x"]), 1), np.uint64)
            n = shim.shim_det_candidates(eig.ctypes.data_as(PF), cols, rows, kept, kxy.ctypes.data_as(PI), o["min_dist"], o["quality"], keys.ctypes.data_as(PU64), len(keys))
            assert n == len(w["cand"]["x"]) == w["counters"][2]
            assert np.array_equal((keys[:n] & np.uint64(0xffffffff)).astype(np.int64), w["cand"]["y"] * cols + w["cand"]["x"])
            assert all(shim.shim_det_key(float(v), int(i)) == int(key) for v, i, key in list(zip(w["cand"]["eig"], w["cand"]["y"] * cols + w["cand"]["x"], keys[:n]))[:64])
        mc, q, md = c["corners"]
        po, ro, nc = np.zeros((mc, 2), np.float32), np.zeros(mc, np.float32), C.c_int32(-1)
        got = shim.shim_det_corners(im.ctypes.data_as(PU8), cols, rows, mc, q, md, o["candidate_capacity"], po.ctypes.data_as(PF), ro.ctypes.data_as(PF), C.byref(nc))
        assert got == len(wc[k]["pts"]) and nc.value == wc[k]["n_candidates"]
        assert np.array_equal(_bits(po[:got]), _bits(wc[k]["pts"])) and np.array_equal(_bits(ro[:got]), _bits(wc[k]["response"]))


def _walk_both(shim, xs, ys, cols, min_dist, max_corners):
    """The host walk and the model's on a synthetic candidate list given in the order of G3."""
    n = len(xs)
    vals = np.linspace(2.0, 1.0, n).astype(np.float32)
    keys = np.array([shim.shim_det_key(float(v), int(y * cols + x)) for v, x, y in zip(vals, xs, ys)], np.uint64)
    xy, resp = np.zeros((max(max_corners, 1), 2), np.int32), np.zeros(max(max_corners, 1), np.float32)
    shuffled = keys[np.random.default_rng(1).permutation(n)]      # (the host walk orders the list itself)
    got = shim.shim_det_walk(shuffled.ctypes.data_as(PU64), n, cols, min_dist, max_corners, xy.ctypes.data_as(PI), resp.ctypes.data_as(PF))
    a = m.walk(np.asarray(xs, np.int64), np.asarray(ys, np.int64), min_dist, max_corners)
    assert got == len(a) and np.array_equal(xy[:got, 0], np.asarray(xs)[a]) and np.array_equal(xy[:got, 1], np.asarray(ys)[a]) and np.array_equal(_bits(resp[:got]), _bits(vals[a]))
    return a.tolist()


def test_the_walk_at_its_boundary(shim):
    cols = 200
    # d^2 == min_dist^2 is accepted; the nearest smaller sums of two squares are rejected (24 = 5^2 - 1 is none)
    assert _walk_both(shim, [50, 53, 54], [50, 54, 52], cols, 5, 10) == [0, 1]            # (3, 4): 25 accepted; (4, 2) from the first: 20 < 25 rejected
    assert _walk_both(shim, [50, 55, 54], [50, 50, 50], cols, 5, 10) == [0, 1]            # (5, 0): 25 accepted; (4, 0): 16 rejected
    # min_dist^2 - 1 where it is a sum of two squares: 17^2 - 1 = 288 = 12^2 + 12^2, and 1^2 - 1 = 0 (the same pixel)
    assert _walk_both(shim, [50, 62, 67], [50, 62, 50], cols, 17, 10) == [0, 2]           # (12, 12): 288 rejected; (17, 0): 289 accepted
    assert _walk_both(shim, [50, 50, 51], [50, 50, 50], cols, 1, 10) == [0, 2]            # min_dist 1: the same pixel (0 < 1) goes, the neighbour (1 = 1) stays
    assert _walk_both(shim, [10, 11, 10, 11], [10, 10, 11, 11], cols, 1, 10) == [0, 1, 2, 3]
    assert _walk_both(shim, [10, 11, 12], [10, 10, 10], cols, 2, 10) == [0, 2]            # d^2 = 1 < 4 rejected, d^2 = 4 accepted
    assert _walk_both(shim, [10, 10, 11], [10, 10, 10], cols, 0, 10) == [0, 1, 2]         # min_dist 0 rejects nothing, not even the same pixel
    assert _walk_both(shim, [10, 11, 30, 50], [10, 10, 10, 10], cols, 0, 2) == [0, 1]     # max_corners stops the walk
    assert _walk_both(shim, [], [], cols, 5, 3) == []


def test_sanitized_stand_alone_program():
    """gfbe_det.h under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _cxx(os.path.join(ROOT, "tests", "det_host_main.cpp"), os.path.join(BUILD, "det_host_main"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the branches
def test_the_cases_reach_every_branch():
    E, o_of = dc.expected, lambda n: dict(m.DEFAULTS, **dc.case(n)["options"])
    assert {(dc.case(n)["cols"], dc.case(n)["rows"]) for n in dc.NAMES} >= {(23, 23), (64, 48), (91, 89), (180, 177), (640, 480)}
    assert len(dc.case("s64x48_three_cameras")["pts"]) == 3 and len(dc.case("s64x48_three_cameras")["pts"][1]) == 0
    first = E("s23_first_frame")[0][0]["counters"]
    assert first[0] == 0 and first[1] == 0 and first[3] > 0                                  # the first frame: no held points, corners added
    eq, ab = E("held_equal_max_cnt")[0][0]["counters"], E("held_above_max_cnt")[0][0]["counters"]
    assert eq[1] == o_of("held_equal_max_cnt")["max_cnt"] and eq[2] == eq[3] == 0             # G4: nothing wanted
    assert ab[1] > o_of("held_above_max_cnt")["max_cnt"] and ab[3] == 0 and len(E("held_above_max_cnt")[0][0]["ids"]) == ab[1]
    # G1: ties keep their list order, two points on one pixel, a point inside an earlier disc, dropped points, halves to even
    sp = E("s64x48_three_cameras")[0][0]
    ko = sp["kept_order"].tolist()
    assert ko[:4] == [4, 5, 6, 7] and 12 in ko and 13 not in ko and 14 not in ko and 15 not in ko and 16 not in ko and 17 not in ko and 18 not in ko      # cnt 9 first, in list order; -0.5 -> 0 kept; cols - 0.5 = 63.5 -> 64 outside
    assert 0 in ko and 1 not in ko and 2 not in ko and 3 in ko and 19 in ko and 20 not in ko
    assert sp["kept_xy"][ko.index(19)].tolist() == [40, 10]
    assert m.pixel((63.5, 10.0)) == (64, 10) and m.pixel((90.5, 10.0)) == (90, 10)      # cols - 0.5: outside for even cols, the last column for odd cols
    assert 13 in E("s91x89_min_dist_0")[0][0]["kept_order"].tolist()
    for px, py in ((2, 24), (62, 24), (32, 1), (32, 46), (0, 0), (63, 0), (0, 47), (63, 47)):      # discs over each edge and corner
        assert [px, py] in sp["kept_xy"].tolist()
    assert (E("fully_masked")[0][0]["mask"] == 0).all() and E("fully_masked")[0][0]["counters"].tolist()[1:4] == [1, 0, 0]
    fl = E("flat")[0][0]
    assert fl["cand"]["max_val"] == 0 and fl["counters"][2] == 0 and fl["counters"][1] > 0
    for k, axis in ((0, 0), (1, 1)):      # the strongest response in a border row / column: not a candidate, the inner ones are
        r = E("border_peaks")[0][k]
        y, x = np.unravel_index(np.argmax(r["eig"]), r["eig"].shape)
        assert (y, x)[axis] == 0 and r["counters"][3] > 0 and (r["pts"][:, 1 - axis] >= 1).all()
    pe = E("periodic")[0][0]
    v, cnts = np.unique(pe["cand"]["eig"], return_counts=True)
    assert cnts.max() > 100 and (np.diff((pe["cand"]["y"] * 64 + pe["cand"]["x"])[pe["cand"]["eig"] == v[np.argmax(cnts)]]) < 0).all()      # equal responses: the larger index first
    assert {o_of(n)["min_dist"] for n in dc.NAMES} >= {0, 1, 5, 30} and o_of("s91x89_quality_0")["quality"] == 0.0
    assert E("s91x89_quality_0")[0][0]["cand"]["t"] == 0
    a, b = E("noise_default_chunk")[0][0], E("noise_smallest_chunk")[0][0]
    assert a["counters"][2] > 20 * 64 and a["counters"][3] > 4 * 64 and all(np.array_equal(a[k], b[k]) for k in ("pts", "ids", "track_cnt", "counters"))
    acc = np.stack([a["cand"]["x"][a["accepted"]], a["cand"]["y"][a["accepted"]]], 1)
    d2 = ((acc[:, None, :] - acc[None, :, :]) ** 2).sum(2)
    assert (d2[np.triu_indices(len(acc), 1)] == 25).sum() > 10 and d2[np.triu_indices(len(acc), 1)].min() >= 25      # accepted pairs at exactly min_dist
    ov = E("noise_overflow")[0][0]
    assert ov["counters"][5] == 1 and ov["counters"][3] == 0 and ov["counters"][2] == a["counters"][2] > 500 and ov["counters"][1] == a["counters"][1] > 0
    assert np.array_equal(ov["pts"], a["pts"][:a["counters"][1]]) and ov["next_id"] == 0
    mid = E("noise_mid_chunk")[0][0]
    last = int(mid["accepted"][-1])
    assert mid["counters"][1] + mid["counters"][3] == 112 and last > 64 and (last + 1) % 64 != 0 and last + 1 < mid["counters"][2]      # max_corners reached inside a later chunk
    two = E("two_frames")
    assert two[0][0]["ids"][-1] == two[0][0]["next_id"] - 1 >= 100 and two[1][0]["counters"][0] == len(two[0][0]["ids"]) and two[0][1]["ids"][0] == 5
    assert two[1][0]["counters"][4] >= two[0][0]["counters"][4] and (two[1][0]["track_cnt"][:two[1][0]["counters"][1]] >= 1).all()
    big = E("s640x480")[0][0]
    assert big["counters"][0] == 100 and big["counters"][3] > 0 and len(big["ids"]) <= 150


# ---- the model alone: planted corners
# Measured with the committed model on the squares of det_cases.squares (seed 0, quality 0.01, min_dist 5, max_corners = the planted
# count): the worst distance from a planted corner to the nearest detected one is 0.0 px at 48 x 64, 89 x 91, 177 x 180 and 480 x 640
# (8, 36, 196 and 1 976 corners) and no other candidate exists. Four times the worst is 0: the floor of 1 px holds (a peak sits on a pixel).
K_CORNER = 1.0


@pytest.mark.parametrize("shape,count", [((48, 64), 8), ((89, 91), 36), ((177, 180), 196), ((480, 640), 1976)])
def test_model_finds_planted_corners(shape, count):
    """So that "bits equal the model" cannot hide a wrong model: the corners of the squares are known."""
    im, planted = dc.squares(shape[0], shape[1], 0)
    assert len(planted) == count
    r = m.corners(im, count, 0.01, 5)
    d = np.sqrt(((planted[:, None, :].astype(np.float64) - r["pts"][None, :, :]) ** 2).sum(2))
    worst = d.min(1).max()
    print("planted", shape, "corners", len(r["pts"]), "candidates", r["n_candidates"], "worst distance %.3f px" % worst)
    assert len(r["pts"]) == count and worst <= K_CORNER


@pytest.mark.parametrize("name", dc.NAMES)
def test_properties_of_a_result(name):
    c = dc.case(name)
    o = dict(m.DEFAULTS, **c["options"])
    for per_cam in dc.expected(name):
        for r in per_cam:
            kept, added = int(r["counters"][1]), int(r["counters"][3])
            new = r["pts"][kept:].astype(np.int64)
            assert len(new) == added
            if added > 1:
                d2 = ((new[:, None, :] - new[None, :, :]) ** 2).sum(2)
                assert d2[np.triu_indices(added, 1)].min() >= o["min_dist"] ** 2                  # all pairs of added corners at least min_dist apart
            if added and kept:
                d2 = ((new[:, None, :] - r["kept_xy"][None, :, :]) ** 2).sum(2)
                assert d2.min() > o["min_dist"] ** 2                                                # no added corner inside a kept point's disc
            assert (np.diff(r["track_cnt"][:kept]) <= 0).all()                                      # the kept points descend in track_cnt
            assert kept + added <= max(o["max_cnt"], kept) and (added == 0 or kept + added <= o["max_cnt"])
            assert (r["track_cnt"][kept:] == 1).all()


# ---- the binding
def _prototypes(header, prefix):
    spell = lambda t: re.sub(r"\s*\*\s*", "*", " ".join(t.replace("struct ", "").split()))
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    src = re.sub(r"//[^\n]*|^\s*#.*$", " ", src, flags=re.M)
    out = []
    for ret, name, args in re.findall(r"([A-Za-z_][\w \*]*?)\b(%s\w+)\s*\(([^()]*)\)\s*;" % prefix, src):
        if "typedef" in ret:
            continue
        params = []
        for a in ([] if args.strip() in ("", "void") else args.split(",")):
            t, _, dims = re.fullmatch(r"\s*(.*?)(\w+)\s*(\[\w*\])?\s*", a, flags=re.S).groups()
            params.append(spell(t + ("*" if dims else "")))
        out.append((spell(ret), name, params))
    return out


def test_signature_table_matches_the_header():
    P = C.POINTER
    par = {"int32_t": C.c_int32, "double": C.c_double, "gfbe_ctx*": C.c_void_p, "gfbe_klt*": C.c_void_p, "gfbe_det*": C.c_void_p, "gfbe_det**": P(C.c_void_p),
           "const gfbe_det_options*": P(abi.DetOptions), "gfbe_det_options*": P(abi.DetOptions), "float*": P(C.c_float), "const int32_t*": P(C.c_int32),
           "int32_t*": P(C.c_int32), "uint8_t*": P(C.c_uint8)}
    ret = {"void": None, "gfbe_status": C.c_int32}
    table = gf.signatures.DET
    protos = _prototypes("gfbe_det.h", "gfbe_det_")
    assert {p[1] for p in protos} == {"gfbe_det_" + k for k in table} == set(gf.backend.DET_EXPORTS) and len(protos) == 7
    assert gf.signatures.TABLES["gfbe_det_"] is table
    for r, name, params in protos:
        res, args = table[name[len("gfbe_det_"):]]
        assert res is ret[r], name
        assert len(args) == len(params), name
        for k, (p, a) in enumerate(zip(params, args)):
            assert a is par[p], (name, k, p, a)
    hdr = open(os.path.join(ROOT, "include", "gfbe_det.h")).read()
    assert "#define GFBE_DET_MAX_POINTS 2048" in hdr and abi.DET_MAX_POINTS == 2048
    others = set(gf.backend.EXPORTS) | set(gf.backend.LC6_EXPORTS) | set(gf.backend.KLT_EXPORTS)
    assert not set(gf.backend.DET_EXPORTS) & others      # the other surfaces are as they were


def test_no_signature_is_declared_outside_the_table():
    for f in ("abi.py", "backend.py"):
        src = open(os.path.join(ROOT, "ground-fusion2_amd", f)).read()
        tail = src[src.index("DET_PREFIX"):] if f == "abi.py" else src
        assert ".restype" not in tail and ".argtypes" not in tail, f


def test_options_struct_matches_the_c_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gfbe_det.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(gfbe_det_options));']
    for f, _ in abi.DetOptions._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(gfbe_det_options, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.DetOptions) == 32
    for f, _ in abi.DetOptions._fields_:
        assert int(got[f]) == getattr(abi.DetOptions, f).offset, f


def test_c_abi_without_a_device():
    gf.build_native()
    lib = abi.bind(abi.bind(abi.bind(C.CDLL(gf.lib_path()), "gfbe_"), abi.KLT_PREFIX), abi.DET_PREFIX)
    for name in gf.backend.DET_EXPORTS:
        assert hasattr(lib, name), name
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    o = abi.det_default_options(lib)
    assert (o.struct_size, o.max_cnt, o.min_dist, o.candidate_capacity, o.sort_chunk, o.reserved, o.quality) == (C.sizeof(abi.DetOptions), 150, 30, 0, 512, 0, 0.01)
    fake = C.c_void_p(1)

    def create(opt=None):
        h = C.c_void_p(7)
        rc = lib.gfbe_det_create(ctx, fake, C.byref(opt) if opt is not None else None, C.byref(h))
        assert not h.value      # no handle comes back
        return rc
    # a well-formed call fails loudly: no device, no CPU fallback (the tracker is not looked at: there can be none)
    assert create() == abi.NO_DEVICE and b"gfbe_det_create" in lib.gfbe_last_error(ctx) and b"no CPU fallback" in lib.gfbe_last_error(ctx)
    for kw in (dict(struct_size=C.sizeof(abi.DetOptions) - 8), dict(struct_size=0), dict(struct_size=C.sizeof(abi.KltOptions)), dict(max_cnt=0), dict(min_dist=-1),
               dict(min_dist=32769), dict(candidate_capacity=-1), dict(sort_chunk=96), dict(sort_chunk=32), dict(sort_chunk=4096), dict(quality=-0.01),
               dict(quality=float("nan")), dict(quality=float("inf"))):
        assert create(abi.det_default_options(lib, **kw)) == abi.BAD_INPUT, kw
    assert create(abi.det_default_options(lib, sort_chunk=64, min_dist=0, quality=0.0)) == abi.NO_DEVICE
    out = np.full(8, -7, np.int32)
    assert lib.gfbe_det_detect(ctx, fake, out.ctypes.data_as(PI), None, None, None, out.ctypes.data_as(PI)) == abi.NO_DEVICE and (out == -7).all()
    assert b"no CPU fallback" in lib.gfbe_last_error(ctx)
    assert lib.gfbe_det_corners(ctx, fake, 10, 0.01, 10, out.ctypes.data_as(PI), None, None) == abi.NO_DEVICE and (out == -7).all()
    assert lib.gfbe_det_set_next_id(ctx, fake, out.ctypes.data_as(PI)) == abi.NO_DEVICE
    assert lib.gfbe_det_download(ctx, fake, 0, None, None) == abi.NO_DEVICE
    lib.gfbe_det_destroy(ctx, None)
    lib.gfbe_destroy(ctx)
