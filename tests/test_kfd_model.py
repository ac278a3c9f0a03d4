"""The keyframe descriptors without a GPU: the two statements of each of K1, K2 and K4 of the model (tests/kfd_np.py) against each other,
bit for bit, on the cases of tests/kfd_cases.py; the host build of ground-fusion2_amd/csrc/gfbe_kfd.h (tests/kfd_host_shim.cpp) against
the model, bit for bit; the same header under the address and undefined-behaviour sanitizers in a program of its own
(tests/kfd_host_main.cpp); property tests of the model alone; the matching-quality figure of the model; the binding (include/gfbe_kfd.h
against signatures.KFD, the layout of gfbe_kfd_options against a compiled C program, the other surfaces unchanged); and the C ABI's
refusals without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import kfd_cases as kc
import kfd_np as m

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
HDRS = [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_kfd.h", "gfbe_obs.h", "gfbe_klt.h")]
PF, PI, PD, PU8, PU64 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
F = np.float32
IMAGES = [kc.texture(r, c, 1) for r, c in kc.SIZES[1:]] + [kc.planted(7, 7, 1)] + [kc.planted(61, 97, 65), kc.plateau(), kc.edges(), np.full((7, 7), 9, np.uint8)]


def _cxx(src, out, extra):
    if not CXX:
        pytest.fail("no C++ compiler: gfbe_kfd.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + HDRS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_cxx(os.path.join(ROOT, "tests", "kfd_host_shim.cpp"), os.path.join(BUILD, "kfd_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_kfd_taps.argtypes = [PI]
    lib.shim_kfd_ring.argtypes = [PI, PI]
    lib.shim_kfd_blur.argtypes = [PU8, C.c_int, C.c_int, PU8]
    lib.shim_kfd_fast_score.argtypes = [PU8] + [C.c_int] * 5
    lib.shim_kfd_fast.argtypes = [PU8, C.c_int, C.c_int, C.c_int, C.c_int, PU8, PF, PI, PI]
    lib.shim_kfd_pattern_ok.argtypes = [PI]
    lib.shim_kfd_brief.argtypes = [PU8, C.c_int, C.c_int, PI, C.c_int, PF, PU64]
    lib.shim_kfd_norm.argtypes = [PD, C.c_int, PF, PF]
    return lib


def _p(a, t):
    return a.ctypes.data_as(t)


def _b32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_the_header_has_no_hip_in_it():
    src = open(HDRS[0]).read()
    assert "hip/hip_runtime" not in src and "hipLaunch" not in src and "__global__" not in src


# ---- the two statements of the model against each other
def test_taps_are_the_rounded_gaussian():
    assert m.taps_from_gaussian().tolist() == m.TAPS.tolist() == [7, 17, 32, 46, 52, 46, 32, 17, 7] and int(m.TAPS.sum()) == 256


@pytest.mark.parametrize("k", range(len(IMAGES)))
def test_k1_two_statements(k):
    img = IMAGES[k]
    assert np.array_equal(m.blur(img), m.blur_dense(img))


@pytest.mark.parametrize("k", range(len(IMAGES)))
def test_k2_two_statements(k):
    img = IMAGES[k]
    rows, cols = img.shape
    for t in (20, 0, 7, 255, 300, -4):
        s = m.fast_scores(img, t)
        if t == 20 or rows * cols <= 49:
            pix = [(x, y) for y in range(rows) for x in range(cols)]
        else:      # (the brute-force predicate is slow: the corners, their neighbours and a seeded sample)
            rng = np.random.default_rng(k)
            ys, xs = np.nonzero(m.fast_scores(img, 20))
            pix = [(int(x) + dx, int(y) + dy) for x, y in zip(xs[:40], ys[:40]) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]
            pix += [(int(rng.integers(0, cols)), int(rng.integers(0, rows))) for _ in range(100)]
        for x, y in pix:
            if 0 <= x < cols and 0 <= y < rows:
                assert int(s[y, x]) == m.fast_score_brute(img, x, y, t), (x, y, t)


@pytest.mark.parametrize("k", range(len(IMAGES)))
def test_k4_two_statements(k):
    img = IMAGES[k]
    rows, cols = img.shape
    bl = m.blur(img)
    rng = np.random.default_rng(100 + k)
    pts = np.concatenate([kc.window_points(rows, cols), (rng.uniform(-30, 1.0, (40, 2)) * [1, 1] + rng.uniform(0, 1, (40, 2)) * [cols + 30, rows + 30]).astype(F)]).astype(F)
    desc, bad = m.brief(bl, kc.pattern(), pts)
    assert bad == 6
    rows_l, pat_l = bl.tolist(), kc.pattern().tolist()
    for j, (px, py) in enumerate(pts):
        assert [int(v) for v in desc[j]] == m.brief_scalar(rows_l, pat_l, px, py), (j, px, py)


# ---- the host build of the shared header against the model
def test_host_taps_and_ring(shim):
    t, dx, dy = np.zeros(9, np.int32), np.zeros(16, np.int32), np.zeros(16, np.int32)
    shim.shim_kfd_taps(_p(t, PI))
    shim.shim_kfd_ring(_p(dx, PI), _p(dy, PI))
    assert t.tolist() == m.TAPS.tolist() and list(zip(dx.tolist(), dy.tolist())) == list(m.RING)


@pytest.mark.parametrize("k", range(len(IMAGES)))
def test_host_build_equals_the_model(shim, k):
    img = np.ascontiguousarray(IMAGES[k])
    rows, cols = img.shape
    bl = np.zeros_like(img)
    shim.shim_kfd_blur(_p(img, PU8), rows, cols, _p(bl, PU8))
    assert np.array_equal(bl, m.blur(img))
    for t, cap in ((20, 4096), (20, 3), (0, 4096), (60, 10), (300, 4096), (-5, 50)):
        want = m.fast(img, t, cap)
        plane, pts, score, cn = np.zeros_like(img), np.full((cap, 2), -7, F), np.full(cap, -7, np.int32), np.zeros(4, np.int32)
        shim.shim_kfd_fast(_p(img, PU8), rows, cols, t, cap, _p(plane, PU8), _p(pts, PF), _p(score, PI), _p(cn, PI))
        n = int(cn[2])
        assert np.array_equal(cn, want["counters"]) and np.array_equal(plane, want["plane"]), (t, cap)
        assert np.array_equal(_b32(pts[:n]), _b32(want["pts"])) and np.array_equal(score[:n], want["score"]) and (pts[n:] == -7).all()
    s20 = m.fast_scores(img, 20)
    for y in range(0, rows, 5):
        for x in range(cols):
            assert shim.shim_kfd_fast_score(_p(img, PU8), rows, cols, x, y, 20) == s20[y, x]
    want = m.fast(img, 20, 4096)
    pts = np.ascontiguousarray(np.concatenate([want["pts"], kc.window_points(rows, cols)]), F)
    desc = np.zeros((len(pts), 4), np.uint64)
    pat = np.ascontiguousarray(kc.pattern())
    bad = shim.shim_kfd_brief(_p(bl, PU8), rows, cols, _p(pat, PI), len(pts), _p(pts, PF), _p(desc, PU64))
    wdesc, wbad = m.brief(bl, kc.pattern(), pts)
    assert bad == wbad == 6 and np.array_equal(desc, wdesc)
    for name, cam in kc.CAMERAS.items():
        pn = np.zeros((len(want["pts"]), 2), F)
        cam = np.ascontiguousarray(cam)
        shim.shim_kfd_norm(_p(cam, PD), len(pn), _p(np.ascontiguousarray(want["pts"]), PF), _p(pn, PF))
        assert np.array_equal(_b32(pn), _b32(m.norm(cam, want["pts"]))), name


def test_host_pattern_check(shim):
    pat = np.ascontiguousarray(kc.pattern())
    assert shim.shim_kfd_pattern_ok(_p(pat, PI)) == 1 and m.pattern_ok(pat)
    for v in (65, -65, 1 << 20):
        bad = pat.copy()
        bad[3, 255] = v
        assert shim.shim_kfd_pattern_ok(_p(bad, PI)) == 0 and not m.pattern_ok(bad)
    ok = pat.copy()
    ok[0, 0], ok[1, 0] = 64, -64
    assert shim.shim_kfd_pattern_ok(_p(ok, PI)) == 1 and m.pattern_ok(ok)


def test_sanitized_stand_alone_program():
    """gfbe_kfd.h under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _cxx(os.path.join(ROOT, "tests", "kfd_host_main.cpp"), os.path.join(BUILD, "kfd_host_main"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the model alone, so that "bits equal the model" cannot hide a wrong model
@pytest.mark.parametrize("v", (0, 1, 127, 254, 255))
def test_blur_of_a_constant_is_the_constant(v):
    for rows, cols in ((7, 7), (9, 30), (33, 8)):
        assert (m.blur(np.full((rows, cols), v, np.uint8)) == v).all()


def test_blur_commutes_with_a_transpose():
    for img in IMAGES[:3]:
        assert np.array_equal(m.blur(img.T), m.blur(img).T)


@pytest.mark.parametrize("value", (121, 122, 200, 255))
def test_a_lone_bright_pixel_is_a_corner(value):
    img = np.full((31, 33), kc.FLAT, np.uint8)
    img[14, 17] = value
    s = m.fast_scores(img, 20)
    assert s[14, 17] == (value - kc.FLAT - 1 if value - kc.FLAT > 20 else 0)
    for dx, dy in m.RING:
        assert s[14 + dy, 17 + dx] == 0
    assert int((s > 0).sum()) == int(value - kc.FLAT > 20)
    out = m.fast(img, 20, 10)
    assert out["counters"].tolist() == ([1, 1, 1, 0] if value - kc.FLAT > 20 else [0, 0, 0, 0])


def test_planted_counts_and_plateau():
    for n in kc.PLANT_COUNTS:
        out = m.fast(kc.planted(61, 97, n), 20, kc.PLANT_CAP)
        assert out["counters"].tolist() == [n, n, min(n, kc.PLANT_CAP), int(n > kc.PLANT_CAP)], n
        assert [tuple(p) for p in out["pts"].astype(int).tolist()] == kc.plant_positions(61, 97)[:min(n, kc.PLANT_CAP)]
    out = m.fast(kc.plateau(), 20, 10)
    assert out["counters"].tolist() == [3, 1, 1, 0] and out["pts"].tolist() == [[10.0, 30.0]] and out["score"].tolist() == [79]
    assert m.fast(kc.edges(), 20, 10)["counters"].tolist() == [6, 6, 6, 0]
    assert m.fast(np.full((7, 7), 50, np.uint8), 20, 10)["counters"].tolist() == [0, 0, 0, 0]
    one = np.full((7, 7), 50, np.uint8)
    one[3, 3] = 99
    assert m.fast(one, 20, 10)["pts"].tolist() == [[3.0, 3.0]]


def test_descriptors_follow_an_integer_translation():
    """For interior points, descriptors of an image and of its integer translate are equal at translated points."""
    big = kc.texture(160, 200, 3)
    dx, dy = 7, 5
    a, b = big[20:120, 30:150], big[20 - dy:120 - dy, 30 - dx:150 - dx]      # b[y][x] = a[y - dy][x - dx]
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(40, 70, 50), rng.uniform(40, 50, 50)], 1).astype(F)      # 24 of the pattern, 4 of the blur and the shift from every edge
    pts[::2] = np.floor(pts[::2])
    da, _ = m.brief(m.blur(a), kc.pattern(), pts)
    db, _ = m.brief(m.blur(b), kc.pattern(), pts + np.array([dx, dy], F))
    assert np.array_equal(da, db) and len(np.unique(da, axis=0)) > 40


def test_pattern_fixture():
    pat = kc.pattern()
    assert pat.shape == (4, 256) and pat.dtype == np.int32 and int(np.abs(pat).max()) == 24 and m.pattern_ok(pat)
    assert len({tuple(c) for c in pat.T.tolist()}) == 256      # 256 different pairs within the 48-pixel patch


# Matching quality of the model (a sanity check of the model, not a tolerance of the device, whose tolerance is zero bits): the image pair
# is synth.klt_texture(480, 640, seed 0) and its translate by the non-integer shift (2.6, -1.3); a FAST corner p of the first image
# corresponds to the corner of the second nearest to p + shift when that lies within 1.5 px; the figure is the share of corresponding
# corners whose descriptors lie within match_max = 80 bits. MEASURED with the committed model: 208 corresponding corners (of 344 in
# the first image: FAST on this smooth texture is not very repeatable under a sub-pixel shift), all 208 within 80 bits: a share of
# 1.0000. The assertion is the power of two below it, 0.5.
MATCH_MEASURED = 1.0
MATCH_BOUND = 0.5


def matching_quality():
    a = gf.synth.klt_texture(480, 640, seed=0)
    shift = (2.6, -1.3)
    b = gf.synth.klt_texture(480, 640, seed=0, shift=(-shift[0], -shift[1]))
    ea, eb = m.extract(a, kc.pattern(), kc.CAMERAS["plain"]), m.extract(b, kc.pattern(), kc.CAMERAS["plain"])
    pairs = []
    for j, p in enumerate(ea["pts"]):
        if len(eb["pts"]) == 0:
            break
        d = np.hypot(eb["pts"][:, 0] - (p[0] + shift[0]), eb["pts"][:, 1] - (p[1] + shift[1]))
        q = int(np.argmin(d))
        if d[q] <= 1.5:
            pairs.append((j, q))
    if not pairs:
        return 0, 0.0
    ja, jb = np.array(pairs).T
    return len(pairs), float((m.hamming(ea["desc"][ja], eb["desc"][jb]) < 80).mean())


def test_matching_quality_of_the_model():
    n, share = matching_quality()
    print("matching quality: %d corresponding corners, share within 80 bits %.4f" % (n, share))
    assert n >= 50 and share >= MATCH_BOUND


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
    par = {"int32_t": C.c_int32, "gfbe_ctx*": C.c_void_p, "gfbe_klt*": C.c_void_p, "gfbe_kfd*": C.c_void_p, "gfbe_ldb*": C.c_void_p, "gfbe_kfd**": P(C.c_void_p),
           "const gfbe_kfd_options*": P(abi.KfdOptions), "gfbe_kfd_options*": P(abi.KfdOptions), "float*": P(C.c_float), "const float*": P(C.c_float), "const int32_t*": P(C.c_int32),
           "int32_t*": P(C.c_int32), "const double*": P(C.c_double), "double*": P(C.c_double), "const uint8_t*": P(C.c_uint8), "uint8_t*": P(C.c_uint8), "uint64_t*": P(C.c_uint64)}
    ret = {"void": None, "gfbe_status": C.c_int32}
    table = gf.signatures.KFD
    protos = _prototypes("gfbe_kfd.h", "gfbe_kfd_")
    assert {p[1] for p in protos} == {"gfbe_kfd_" + k for k in table} == set(gf.backend.KFD_EXPORTS) and len(protos) == 10
    assert gf.signatures.TABLES["gfbe_kfd_"] is table
    for r, name, params in protos:
        res, args = table[name[len("gfbe_kfd_"):]]
        assert res is ret[r], name
        assert len(args) == len(params), name
        for k, (p, a) in enumerate(zip(params, args)):
            assert a is par[p], (name, k, p, a)


def test_the_other_surfaces_are_unchanged():
    b, s = gf.backend, gf.signatures
    assert (len(b.EXPORTS), len(b.LC6_EXPORTS), len(b.KLT_EXPORTS), len(b.DET_EXPORTS), len(b.OBS_EXPORTS)) == (len(s.GFBE), 3, 8, 7, 9)
    others = set(b.EXPORTS) | set(b.LC6_EXPORTS) | set(b.KLT_EXPORTS) | set(b.DET_EXPORTS) | set(b.OBS_EXPORTS)
    assert not set(b.KFD_EXPORTS) & others and len(others) == len(b.EXPORTS) + 27
    assert s.GFBE["ldb_add_keyframe"] == (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, PU64, PF, PF, C.c_int32, PI, PI, PI, PI, PD])
    assert s.GFBE["ldb_match"] == (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, PU64, PU8, PI, PI, PI, PI, PF, PF])
    declared = {p[1] for p in _prototypes("gfbe.h", "gfbe_")}
    assert declared == set(b.EXPORTS), declared ^ set(b.EXPORTS)


def test_no_signature_is_declared_outside_the_table():
    src = open(os.path.join(ROOT, "ground-fusion2_amd", "abi.py")).read()
    tail = src[src.index("KFD_PREFIX"):]
    assert ".restype" not in tail and ".argtypes" not in tail and "class KeyframeDescriber(Handle)" in tail


def test_options_struct_matches_the_c_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gfbe_kfd.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(gfbe_kfd_options));']
    for f, _ in abi.KfdOptions._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(gfbe_kfd_options, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.KfdOptions) == 24
    for f, _ in abi.KfdOptions._fields_:
        assert int(got[f]) == getattr(abi.KfdOptions, f).offset, f


def test_c_abi_without_a_device():
    gf.build_native()
    lib = abi.bind(abi.bind(C.CDLL(gf.lib_path()), "gfbe_"), abi.KFD_PREFIX)
    for name in gf.backend.KFD_EXPORTS:
        assert hasattr(lib, name), name
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    o = abi.kfd_default_options(lib)
    assert (o.struct_size, o.ring_slots, o.fast_threshold, o.keypoint_capacity, o.window_capacity, o.reserved) == (C.sizeof(abi.KfdOptions), 3, 20, 4096, 2048, 0)
    fake = C.c_void_p(1)
    pat = np.ascontiguousarray(kc.pattern())
    cams = np.ascontiguousarray(np.stack([kc.CAMERAS["plain"], kc.CAMERAS["distorted"]]))

    def create(opt=None, n=2, rows=48, cols=64, pattern=pat, cameras=cams):
        h = C.c_void_p(7)
        rc = lib.gfbe_kfd_create(ctx, n, rows, cols, _p(pattern, PI) if pattern is not None else None, _p(cameras, PD) if cameras is not None else None,
                                 C.byref(opt) if opt is not None else None, C.byref(h))
        assert not h.value      # no handle comes back
        return rc
    # a well-formed call fails loudly: no device, no CPU fallback
    assert create() == abi.NO_DEVICE and b"gfbe_kfd_create" in lib.gfbe_last_error(ctx) and b"no CPU fallback" in lib.gfbe_last_error(ctx)
    assert create(rows=7, cols=7) == abi.NO_DEVICE
    for kw in (dict(struct_size=C.sizeof(abi.KfdOptions) - 8), dict(struct_size=0), dict(struct_size=C.sizeof(abi.ObsOptions)), dict(ring_slots=0), dict(ring_slots=9),
               dict(fast_threshold=-1), dict(fast_threshold=256), dict(keypoint_capacity=0), dict(keypoint_capacity=abi.LDB_MAX_KEYFRAME_DESCRIPTORS + 1),
               dict(window_capacity=0), dict(window_capacity=(1 << 20) + 1)):
        assert create(abi.kfd_default_options(lib, **kw)) == abi.BAD_INPUT, kw
    assert create(abi.kfd_default_options(lib, ring_slots=8, fast_threshold=255, keypoint_capacity=1, window_capacity=1 << 20)) == abi.NO_DEVICE
    for kw in (dict(rows=6), dict(cols=6), dict(rows=(1 << 14) + 1), dict(n=0), dict(pattern=None), dict(cameras=None)):
        assert create(**kw) == abi.BAD_INPUT, kw
    for v in (65, -65):
        bad = pat.copy()
        bad[2, 100] = v
        assert create(pattern=bad) == abi.BAD_INPUT and b"pattern" in lib.gfbe_last_error(ctx)
    badc = cams.copy()
    badc[1, 0] = 0.0
    assert create(cameras=badc) == abi.BAD_INPUT
    badc[1, 0] = np.nan
    assert create(cameras=badc) == abi.BAD_INPUT
    out = np.full(8, -7, np.int32)
    img = np.zeros((2, 48, 64), np.uint8)
    pi = _p(out, PI)
    assert lib.gfbe_kfd_push_image(ctx, fake, 0, _p(img, PU8)) == abi.NO_DEVICE and b"no CPU fallback" in lib.gfbe_last_error(ctx)
    assert lib.gfbe_kfd_capture(ctx, fake, fake, 0) == abi.NO_DEVICE
    assert lib.gfbe_kfd_extract(ctx, fake, 0, pi, None, None, None, None, pi) == abi.NO_DEVICE and (out == -7).all()
    assert lib.gfbe_kfd_describe(ctx, fake, 0, pi, None, None, pi) == abi.NO_DEVICE and (out == -7).all()
    assert lib.gfbe_kfd_add_keyframe(ctx, fake, 0, fake, 1, pi, pi, pi, pi, None) == abi.NO_DEVICE and (out == -7).all()
    assert lib.gfbe_kfd_match(ctx, fake, 0, fake, 0, None, pi, pi, pi, pi, None, None) == abi.NO_DEVICE and (out == -7).all()
    assert lib.gfbe_kfd_download(ctx, fake, 0, 0, None, None) == abi.NO_DEVICE
    lib.gfbe_kfd_destroy(ctx, None)
    lib.gfbe_destroy(ctx)
