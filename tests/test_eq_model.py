"""The image equalisation without a GPU: the two statements of each of E1 .. E5 of the model (tests/eq_np.py) against each other, bit
for bit, on the cases of tests/eq_cases.py; the host build of ground-fusion2_amd/csrc/gfbe_eq.h (tests/eq_host_shim.cpp) against the
model, bit for bit, LUTs and image; the same header under the address and undefined-behaviour sanitizers in a program of its own
(tests/eq_host_main.cpp); properties of the model alone; the binding (include/gfbe_eq.h against signatures.EQ and backend.EQ_EXPORTS,
the layout of gfbe_eq_options against a compiled C program, the other surfaces disjoint from the new one); and the C ABI's refusals
without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import eq_cases as ec
import eq_np as m

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
HDRS = [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_eq.h", "gfbe_klt.h")]
PF, PI, PU8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
ALL = ec.SHAPES + (ec.BIG,)
IDS = [ec.shape_id(s) for s in ALL]


def _cxx(src, out, extra):
    if not CXX:
        pytest.fail("no C++ compiler: gfbe_eq.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + HDRS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_cxx(os.path.join(ROOT, "tests", "eq_host_shim.cpp"), os.path.join(BUILD, "eq_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_eq_refused.argtypes = [C.c_int] * 4 + [C.c_double]
    lib.shim_eq_geom.argtypes = [C.c_int] * 4 + [C.c_double, PI, PF]
    lib.shim_eq.argtypes = [PU8] + [C.c_int] * 4 + [C.c_double, PU8, PU8]
    lib.shim_eq_redistribute.argtypes = [C.c_int] * 4
    return lib


def _p(a, t):
    return a.ctypes.data_as(t)


def _images(shape):
    rows, cols = shape[:2]
    return [ec.image(k, rows, cols) for k in ec.KINDS]


def test_the_header_has_no_hip_in_it():
    src = open(HDRS[0]).read()
    assert "hip/hip_runtime" not in src and "hipLaunch" not in src and "__global__" not in src and "E1 geometry" in src and "E6 in place" in src


# ---- the two statements of the model against each other
def test_geometry_of_the_cases():
    want = {(16, 16, 8, 8, 40.0): (2, 2, 1), (9, 9, 8, 8, 40.0): (2, 2, 1), (17, 23, 8, 8, 40.0): (3, 3, 1), (24, 20, 8, 8, 40.0): (3, 4, 1), (61, 97, 8, 8, 3.0): (13, 8, 1),
            (61, 97, 1, 1, 40.0): (97, 61, 924), (61, 97, 8, 8, 0.0): (13, 8, 0), (33, 47, 5, 3, 2.0): (10, 12, 1), (120, 188, 8, 8, 40.0): (24, 16, 60),
            (480, 752, 8, 8, 40.0): (94, 60, 881)}
    for s in ALL:
        g = m.geometry(*s)
        assert (g["tw"], g["th"], g["limit"]) == want[s], s
    assert m.geometry(24, 20, 8, 8)["ext_rows"] == 32 and m.geometry(9, 9, 8, 8)["ext_cols"] == 16 and not m.geometry(480, 752)["ext"]


@pytest.mark.parametrize("shape", ALL, ids=IDS)
def test_two_statements(shape):
    rows, cols, tx, ty, clip = shape
    for img in _images(shape):
        g = m.geometry(rows, cols, tx, ty, clip)
        yi, xi = m.reflect101(np.arange(g["ext_rows"]), rows), m.reflect101(np.arange(g["ext_cols"]), cols)
        if shape != ec.BIG:
            assert np.array_equal(m.extended_loop(img, g), img[yi][:, xi])                                  # E1
        assert np.array_equal(m.hists_loop(img, tx, ty, clip), m.hists(img, tx, ty, clip))                  # E2, E3
        lut = m.luts(img, tx, ty, clip)
        assert np.array_equal(m.luts_loop(img, tx, ty, clip), lut)                                          # E4
        out = m.interpolate(img, lut, tx, ty)
        assert np.array_equal(m.interpolate_loop(img, lut, tx, ty), out)                                    # E5
        rng = np.random.default_rng(rows * cols)
        pix = [(0, 0), (cols - 1, rows - 1), (cols - 1, 0), (0, rows - 1)] + [(int(rng.integers(0, cols)), int(rng.integers(0, rows))) for _ in range(60)]
        for x, y in pix:
            assert m.interp_pixel(img, lut, g, tx, ty, x, y) == out[y, x], (x, y)
    for q in (m.axis, m.axis_loop):
        a, b = q(cols, m.geometry(*shape)["inv_tw"], tx), q(rows, m.geometry(*shape)["inv_th"], ty)
        for t1, t2, w, w1 in (a, b):
            assert t1.min() >= 0 and (t2 >= t1).all() and (t2 - t1 <= 1).all() and w.dtype == np.float32 and (w >= 0).all() and (w <= 1).all() and (np.diff(t1) >= 0).all()
        assert a[1].max() <= tx - 1 and b[1].max() <= ty - 1


def test_the_sequential_residual_equals_the_closed_form(shim):
    """Every residual 0 .. 255 at a few limits: the loop of E3 against `i % step == 0 && i / step < residual`, and the header's."""
    for residual in range(256):
        for batch in (0, 3):
            clipped = 256 * batch + residual
            seq = [batch] * 256
            if residual > 0:
                step, i, r = max(256 // residual, 1), 0, residual
                while i < 256 and r > 0:
                    seq[i] += 1
                    i += step
                    r -= 1
                assert r == 0                      # the bound i < 256 never bites
            assert sum(seq) == clipped
            assert [shim.shim_eq_redistribute(0, i, 5, clipped) for i in range(256)] == seq
    assert shim.shim_eq_redistribute(9, 0, 5, 256 + 1) == 5 + 1 + 1 and shim.shim_eq_redistribute(9, 3, 0, 777) == 9


# ---- the host build of the shared header against the model
@pytest.mark.parametrize("shape", ALL, ids=IDS)
def test_host_build_equals_the_model(shim, shape):
    rows, cols, tx, ty, clip = shape
    g = m.geometry(*shape)
    ints, floats = np.zeros(3, np.int32), np.zeros(3, np.float32)
    assert shim.shim_eq_refused(*shape) == 0
    shim.shim_eq_geom(rows, cols, tx, ty, clip, _p(ints, PI), _p(floats, PF))
    assert ints.tolist() == [g["tw"], g["th"], g["limit"]]
    assert floats.view(np.uint32).tolist() == np.array([g["scale"], g["inv_tw"], g["inv_th"]], np.float32).view(np.uint32).tolist()
    for img in _images(shape):
        want, wlut = m.equalize(img, tx, ty, clip)
        src = np.ascontiguousarray(img).copy()
        lut, out = np.full((ty, tx, 256), 7, np.uint8), np.zeros_like(src)
        shim.shim_eq(_p(src, PU8), rows, cols, tx, ty, clip, _p(lut, PU8), _p(out, PU8))
        assert np.array_equal(lut, wlut) and np.array_equal(out, want) and np.array_equal(src, img)
        shim.shim_eq(_p(src, PU8), rows, cols, tx, ty, clip, _p(lut, PU8), _p(src, PU8))      # E6
        assert np.array_equal(src, want)


def test_host_refusals(shim):
    for bad in ((9, 9, 0, 8, 40.0), (9, 9, 8, 65, 40.0), (8, 9, 8, 8, 40.0), (9, 8, 8, 8, 40.0), (16385, 64, 8, 8, 40.0), (64, 16385, 8, 8, 40.0), (64, 64, 8, 8, -1e-300),
                (64, 64, 8, 8, float("inf")), (64, 64, 8, 8, float("nan"))):
        assert shim.shim_eq_refused(*bad) == 1, bad
    for ok in ((9, 9, 8, 8, 0.0), (16384, 16384, 64, 64, 1e308), (2, 2, 1, 1, 40.0)):
        assert shim.shim_eq_refused(*ok) == 0, ok


def test_sanitized_stand_alone_program():
    """gfbe_eq.h under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _cxx(os.path.join(ROOT, "tests", "eq_host_main.cpp"), os.path.join(BUILD, "eq_host_main"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the model alone, so that "bits equal the model" cannot hide a wrong model
@pytest.mark.parametrize("shape", ALL, ids=IDS)
def test_properties_of_the_model(shape):
    rows, cols, tx, ty, clip = shape
    g = m.geometry(*shape)
    for kind, img in zip(ec.KINDS, _images(shape)):
        h = m.hists(img, tx, ty, clip)
        assert (h.sum(2) == g["area"]).all() and (h >= 0).all()                      # the clipped histogram sums to the tile area
        if g["limit"] > 0:
            assert h.max() <= g["limit"] + (g["area"] + 255) // 256 + 1
        out, lut = m.equalize(img, tx, ty, clip)
        assert (np.diff(lut.astype(int), axis=2) >= 0).all() and (lut[:, :, 255] == 255).all()      # monotone, ends in 255
        if kind == "constant":
            assert len(np.unique(out)) == 1                                          # a constant image maps to one value
    # a limit of the area or more clips nothing
    tex = _images(shape)[0]
    assert np.array_equal(m.hists(tex, tx, ty, 256.0), m.hists(tex, tx, ty, 0.0)) and np.array_equal(m.hists(tex, tx, ty, 1e308), m.hists(tex, tx, ty, 0.0))


def test_output_is_independent_of_the_stacking():
    shape = (61, 97, 8, 8, 3.0)
    out3, lut3 = ec.expected(shape, 3)
    out65, lut65 = ec.expected(shape, 65)
    assert np.array_equal(out65[:3], out3) and np.array_equal(lut65[:3], lut3)
    for k in (0, 2, 64):
        o, l = m.equalize(ec.stack(61, 97, 65)[k], 8, 8, 3.0)
        assert np.array_equal(o, out65[k]) and np.array_equal(l, lut65[k])
    assert len({out65[k].tobytes() for k in range(65)}) > 40      # the cameras differ


def test_equalisation_spreads_a_narrow_range():
    """The ramp occupies 64 grey levels; with the default options its equalised image spans most of the range, and more than with a low limit."""
    img = ec.image("ramp", 120, 188)
    assert int(img.max()) - int(img.min()) == 63
    wide, low = m.equalize(img)[0], m.equalize(img, clip_limit=1.0)[0]
    span = lambda a: int(a.max()) - int(a.min())
    assert span(wide) > 200 and span(low) < span(wide)


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
    par = {"int32_t": C.c_int32, "gfbe_ctx*": C.c_void_p, "gfbe_klt*": C.c_void_p, "gfbe_kfd*": C.c_void_p, "gfbe_eq*": C.c_void_p, "gfbe_eq**": P(C.c_void_p),
           "const gfbe_eq_options*": P(abi.EqOptions), "gfbe_eq_options*": P(abi.EqOptions), "const uint8_t*": P(C.c_uint8), "uint8_t*": P(C.c_uint8)}
    ret = {"void": None, "gfbe_status": C.c_int32}
    table = gf.signatures.EQ
    protos = _prototypes("gfbe_eq.h", "gfbe_eq_")
    assert {p[1] for p in protos} == {"gfbe_eq_" + k for k in table} == set(gf.backend.EQ_EXPORTS) and len(protos) == 7
    assert gf.signatures.TABLES["gfbe_eq_"] is table and abi.EQ_PREFIX == "gfbe_eq_"
    for r, name, params in protos:
        res, args = table[name[len("gfbe_eq_"):]]
        assert res is ret[r], name
        assert len(args) == len(params), name
        for k, (p, a) in enumerate(zip(params, args)):
            assert a is par[p], (name, k, p, a)


def test_the_other_surfaces_are_disjoint_from_the_new_one():
    b, s = gf.backend, gf.signatures
    assert (len(b.EXPORTS), len(b.LC6_EXPORTS), len(b.KLT_EXPORTS), len(b.DET_EXPORTS), len(b.OBS_EXPORTS), len(b.KFD_EXPORTS), len(b.PNP_EXPORTS)) == (len(s.GFBE), 3, 8, 7, 9, 10, 6)
    others = set(b.EXPORTS) | set(b.LC6_EXPORTS) | set(b.KLT_EXPORTS) | set(b.DET_EXPORTS) | set(b.OBS_EXPORTS) | set(b.KFD_EXPORTS) | set(b.PNP_EXPORTS)
    assert not set(b.EQ_EXPORTS) & others and len(others) == len(b.EXPORTS) + 43 and all(n.startswith("gfbe_eq_") for n in b.EQ_EXPORTS)
    declared = {p[1] for p in _prototypes("gfbe.h", "gfbe_")}
    assert declared == set(b.EXPORTS), declared ^ set(b.EXPORTS)
    for header, prefix, n in (("gfbe_klt.h", "gfbe_klt_", 8), ("gfbe_kfd.h", "gfbe_kfd_", 10)):
        assert len(_prototypes(header, prefix)) == n and not _prototypes(header, "gfbe_eq_")


def test_no_signature_is_declared_outside_the_table():
    src = open(os.path.join(ROOT, "ground-fusion2_amd", "abi.py")).read()
    tail = src[src.index("EQ_PREFIX"):]
    assert ".restype" not in tail and ".argtypes" not in tail and "class Equalizer(Handle)" in tail


def test_options_struct_matches_the_c_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gfbe_eq.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(gfbe_eq_options));']
    for f, _ in abi.EqOptions._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(gfbe_eq_options, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.EqOptions) == 24
    for f, _ in abi.EqOptions._fields_:
        assert int(got[f]) == getattr(abi.EqOptions, f).offset, f


def test_c_abi_without_a_device():
    gf.build_native()
    lib = abi.bind(abi.bind(C.CDLL(gf.lib_path()), "gfbe_"), abi.EQ_PREFIX)
    for name in gf.backend.EQ_EXPORTS:
        assert hasattr(lib, name), name
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    o = abi.eq_default_options(lib)
    assert (o.struct_size, o.tiles_x, o.tiles_y, o.reserved, o.clip_limit) == (C.sizeof(abi.EqOptions), 8, 8, 0, 40.0)
    fake = C.c_void_p(1)

    def create(opt=None, n=2, rows=48, cols=64):
        h = C.c_void_p(7)
        rc = lib.gfbe_eq_create(ctx, n, rows, cols, C.byref(opt) if opt is not None else None, C.byref(h))
        assert not h.value      # no handle comes back
        return rc
    # a well-formed call fails loudly: no device, no CPU fallback
    assert create() == abi.NO_DEVICE and b"gfbe_eq_create" in lib.gfbe_last_error(ctx) and b"no CPU fallback" in lib.gfbe_last_error(ctx)
    assert create(rows=9, cols=9) == abi.NO_DEVICE and create(rows=16384, cols=16384) == abi.NO_DEVICE
    for kw in (dict(struct_size=C.sizeof(abi.EqOptions) - 8), dict(struct_size=0), dict(struct_size=C.sizeof(abi.KltOptions)), dict(tiles_x=0), dict(tiles_x=65), dict(tiles_y=0),
               dict(tiles_y=65), dict(tiles_y=-8), dict(clip_limit=-1.0), dict(clip_limit=float("inf")), dict(clip_limit=float("nan")), dict(tiles_x=64), dict(tiles_y=48)):
        assert create(abi.eq_default_options(lib, **kw)) == abi.BAD_INPUT, kw
        assert b"gfbe_eq_create" in lib.gfbe_last_error(ctx)
    assert create(abi.eq_default_options(lib, tiles_x=63, tiles_y=47, clip_limit=0.0)) == abi.NO_DEVICE
    assert create(abi.eq_default_options(lib, tiles_x=1, tiles_y=1, clip_limit=1e308)) == abi.NO_DEVICE
    for kw in (dict(rows=8), dict(cols=8), dict(rows=(1 << 14) + 1), dict(cols=(1 << 14) + 1), dict(n=0), dict(n=65536), dict(n=-1)):
        assert create(**kw) == abi.BAD_INPUT, kw
    assert lib.gfbe_eq_create(ctx, 1, 48, 64, None, None) == abi.BAD_INPUT
    img = np.full((2, 48, 64), 9, np.uint8)
    out = np.full((2, 48, 64), 7, np.uint8)
    lut = np.full((2, 8, 8, 256), 7, np.uint8)
    assert lib.gfbe_eq_apply(ctx, fake, _p(img, PU8), _p(out, PU8)) == abi.NO_DEVICE and b"no CPU fallback" in lib.gfbe_last_error(ctx) and (out == 7).all()
    assert lib.gfbe_eq_push_klt(ctx, fake, fake, _p(img, PU8)) == abi.NO_DEVICE and b"gfbe_eq_push_klt" in lib.gfbe_last_error(ctx)
    assert lib.gfbe_eq_push_kfd(ctx, fake, fake, 0, _p(img, PU8)) == abi.NO_DEVICE and b"gfbe_eq_push_kfd" in lib.gfbe_last_error(ctx)
    assert lib.gfbe_eq_download_lut(ctx, fake, _p(lut, PU8)) == abi.NO_DEVICE and (lut == 7).all() and (img == 9).all()
    assert lib.gfbe_eq_apply(None, fake, _p(img, PU8), _p(out, PU8)) == abi.BAD_INPUT
    lib.gfbe_eq_destroy(ctx, None)
    lib.gfbe_destroy(ctx)
