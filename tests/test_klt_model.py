"""The optical-flow tracker without a GPU: the model (tests/klt_np.py) against its own second restatement of R1, R2 and the window
values, bit for bit; the host build of ground-fusion2_amd/csrc/gfbe_klt.h (tests/klt_host_shim.cpp) against the model on every case,
bit for bit, with the branches the cases must reach; the same header under the address and undefined-behaviour sanitizers in a
program of its own (tests/klt_host_main.cpp); a property test of the model alone on planted translations; the binding
(include/gfbe_klt.h against signatures.KLT, the layout of gfbe_klt_options against a compiled C program); and the C ABI's refusals
without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import klt_cases as kc
import klt_np as m

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
HDR = os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_klt.h")
PF, PI, PU8, PI16 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
F = np.float32


def _cxx(src, out, extra):
    if not CXX:
        pytest.fail("no C++ compiler: gfbe_klt.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, HDR)):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_cxx(os.path.join(ROOT, "tests", "klt_host_shim.cpp"), os.path.join(BUILD, "klt_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_klt_build.restype = C.c_void_p
    lib.shim_klt_build.argtypes = [PU8, C.c_int, C.c_int, C.c_int]
    lib.shim_klt_free.argtypes = [C.c_void_p]
    lib.shim_klt_levels.argtypes = [C.c_void_p]
    lib.shim_klt_level.argtypes = [C.c_void_p, C.c_int, PU8, PI16, PI]
    lib.shim_klt_flow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, PF, PF, PU8, PF, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, PI]
    lib.shim_klt_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int, PF, PI, PI, C.c_int, PF, PI, C.POINTER(C.c_double), PF, PF, PI, PI, PI]
    lib.shim_klt_check_points.argtypes = [C.c_int, PI, C.c_int, PF]
    lib.shim_klt_in_border.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
    lib.shim_klt_distance.argtypes = [C.c_float] * 4
    lib.shim_klt_distance.restype = C.c_double
    lib.shim_klt_floor.argtypes = lib.shim_klt_round.argtypes = [C.c_float]
    lib.shim_klt_weights.argtypes = [C.c_float, C.c_float, PI]
    return lib


class HostPyramid:
    def __init__(self, lib, image, max_level):
        self.lib, self.im = lib, np.ascontiguousarray(image, np.uint8)
        self.p = lib.shim_klt_build(self.im.ctypes.data_as(PU8), self.im.shape[1], self.im.shape[0], max_level)

    def level(self, l):
        d = np.zeros(3, np.int32)
        self.lib.shim_klt_level(self.p, l, None, None, d.ctypes.data_as(PI))
        img, der = np.zeros((d[1] + 42, d[0] + 42), np.uint8), np.zeros((d[1] + 42, d[0] + 42, 2), np.int16)
        self.lib.shim_klt_level(self.p, l, img.ctypes.data_as(PU8), der.ctypes.data_as(PI16), d.ctypes.data_as(PI))
        return img, der

    def __del__(self):
        self.lib.shim_klt_free(self.p)


def _host_pyramids(shim, name):
    c = kc.case(name)
    ml = max(dict(m.DEFAULTS, **c["options"])["max_level"], 1)
    return [[HostPyramid(shim, im[k], ml) for k in range(len(im))] for im in c["images"]]


def test_the_header_has_no_hip_in_it():
    src = open(HDR).read()
    assert "hip/hip_runtime" not in src and "hipLaunch" not in src and "__global__" not in src


# ---- the model against its second restatement
@pytest.mark.parametrize("shape", [(23, 23), (48, 64), (89, 91), (177, 180), (22, 57)])
def test_two_restatements_of_pyramid_and_derivative_agree(shape):
    a, _ = kc.pair(shape[0], shape[1], 9, (1.0, 1.0))
    cur = a
    for _ in range(4):
        assert np.array_equal(m.scharr(cur), m.scharr_separable(cur))
        if min(cur.shape) < 6:
            break
        d1, d2 = m.pyr_down(cur), m.pyr_down_dense(cur)
        assert d1.shape == ((cur.shape[0] + 1) // 2, (cur.shape[1] + 1) // 2) and np.array_equal(d1, d2)
        cur = d1


def test_levels_stop_as_the_reference_stops(shim):
    """The stop rule of :604-613 in the model and in the header's klt_plan_levels (through the host pyramid builder)."""
    table = [(23, 23, 3, 1), (64, 48, 3, 2), (91, 89, 3, 3), (180, 177, 3, 4), (180, 177, 7, 4), (640, 480, 3, 4), (640, 480, 7, 5), (44, 44, 3, 2), (43, 44, 3, 2),
             (42, 44, 3, 1), (44, 42, 3, 1), (180, 177, 0, 1), (180, 177, 1, 2)]
    for cols, rows, ml, want in table:
        assert len(m.plan_levels(cols, rows, ml)) == want, (cols, rows, ml)
        hp = HostPyramid(shim, np.zeros((rows, cols), np.uint8), ml)
        assert shim.shim_klt_levels(hp.p) == want, (cols, rows, ml)
        d = np.zeros(3, np.int32)
        shim.shim_klt_level(hp.p, want - 1, None, None, d.ctypes.data_as(PI))
        assert (int(d[0]), int(d[1])) == m.plan_levels(cols, rows, ml)[-1] and d[2] == d[0] + 42
    assert m.plan_levels(640, 480, 7)[-1] == (40, 30)


def test_two_restatements_of_the_window_values_agree():
    pyr = kc.pyramids("s180x177_four_levels")[0][0]
    rng = np.random.default_rng(5)
    for L in pyr:
        for _ in range(12):
            x0, y0 = int(rng.integers(-21, L["w"])), int(rng.integers(-21, L["h"]))
            wt = m.weights(F(rng.integers(0, 1 << 15)) / F(1 << 15), F(rng.uniform()))
            for key, shift in (("i64", 9), ("dx64", 14), ("dy64", 14)):
                assert np.array_equal(m.window(L[key], x0, y0, wt, shift), m.window_resampled(L[key], x0, y0, wt, shift))


# ---- the host build against the model
def test_host_scalars_are_the_models(shim):
    for v in (0.5, 1.5, 2.5, -0.5, -1.5, 3.4999, 1e30, -1e30, np.inf, -np.inf, np.nan, 178.5, 179.5):
        assert shim.shim_klt_round(v) == m.kround(F(v)) and shim.shim_klt_floor(v) == m.kfloor(F(v)), v
    assert (m.kround(F(0.5)), m.kround(F(1.5)), m.kround(F(2.5)), m.kfloor(F(-0.5))) == (0, 2, 2, -1)
    rng = np.random.default_rng(3)
    halves = 0
    for k in range(400):
        a, b = (F(rng.integers(0, 1 << 15)) / F(1 << 15), F(0)) if k % 2 else (F(rng.uniform()), F(rng.uniform()))
        w = (C.c_int32 * 4)()
        shim.shim_klt_weights(a, b, w)
        assert tuple(w) == m.weights(a, b) and sum(w) == 1 << 14
        t = (a * (F(1) - b)) * F(16384)
        halves += int(t - np.floor(t) == F(0.5))
    assert halves > 0      # a multiple of 2^-15 puts a weight product exactly on a half: rounding to even is exercised
    # inBorder rounds half to even: x = 0.5 -> 0 (outside), 1.5 -> 2 (inside), cols - 1.5 -> cols - 2 or cols - 1 by the parity of cols
    for cols in (90, 91):
        for x, want in ((0.5, False), (1.5, True), (cols - 1.5, m.kround(F(cols - 1.5)) < cols - 1), (2.5, True)):
            assert bool(shim.shim_klt_in_border(x, 5.0, cols, 40, 1)) == m.in_border((F(x), F(5.0)), cols, 40, 1) == want, (cols, x)
    assert shim.shim_klt_distance(10.0, 10.0, 10.5, 10.0) == m.distance((10.0, 10.0), (10.5, 10.0)) == 0.5      # exactly the bound: kept
    for _ in range(100):
        p = rng.uniform(0, 600, 4).astype(np.float32)
        assert shim.shim_klt_distance(*[float(v) for v in p]) == m.distance(p[:2], p[2:])


@pytest.mark.parametrize("name", kc.NAMES)
def test_host_pyramids_are_the_models(shim, name):
    hp, mp = _host_pyramids(shim, name), kc.pyramids(name)
    for t in range(len(mp)):
        for k in range(len(mp[t])):
            assert shim.shim_klt_levels(hp[t][k].p) == len(mp[t][k])
            for l, L in enumerate(mp[t][k]):
                img, der = hp[t][k].level(l)
                assert np.array_equal(img, L["img"]) and np.array_equal(der, L["der"]), (t, k, l)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", kc.NAMES)
def test_host_flow_is_the_models(shim, name):
    c, hp, want = kc.case(name), _host_pyramids(shim, name), kc.expected_flows(name)
    o = dict(m.DEFAULTS, **c["options"])
    for (d, ml, init), per_cam in want.items():
        for k, w in enumerate(per_cam):
            p = np.ascontiguousarray(c["pts"][k], np.float32)
            n = len(p)
            nx = np.ascontiguousarray(kc.initial_flow(c, k)) if init else np.full((n, 2), -7, np.float32)
            st, er, tr = np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros((n, m.MAX_LEVELS), np.int32)
            I, J = (hp[0][k], hp[1][k]) if d == 0 else (hp[1][k], hp[0][k])
            shim.shim_klt_flow(I.p, J.p, n, p.ctypes.data_as(PF), nx.ctypes.data_as(PF), st.ctypes.data_as(PU8), er.ctypes.data_as(PF), ml, int(init), o["max_count"],
                               o["epsilon"], o["min_eig_threshold"], tr.ctypes.data_as(PI))
            assert np.array_equal(_bits(nx), _bits(w["next_pts"])) and np.array_equal(st, w["status"]) and np.array_equal(_bits(er), _bits(w["err"])), (d, ml, init, k)
            assert np.array_equal(tr, w["trace"]), (d, ml, init, k)


@pytest.mark.parametrize("name", kc.NAMES)
def test_host_track_is_the_models(shim, name):
    c, hp, want = kc.case(name), _host_pyramids(shim, name), kc.expected_tracks(name)
    o = dict(m.DEFAULTS, **c["options"])
    iopt = np.array([o["max_level"], o["flow_back"], o["border"], o["grey_max"], o["prediction_min_success"], o["max_count"]], np.int32)
    dopt = np.array([o["flow_back_dist"], o["epsilon"], o["min_eig_threshold"]], np.float64)
    held = [(c["pts"][k], c["ids"][k], c["cnt"][k]) for k in range(len(c["pts"]))]
    for t, per_cam in enumerate(want):
        nxt = []
        for k, w in enumerate(per_cam):
            p, i_, n_ = (np.ascontiguousarray(held[k][0], np.float32), np.ascontiguousarray(held[k][1], np.int32), np.ascontiguousarray(held[k][2], np.int32))
            n = len(p)
            pred = c["predict"][t][k] if (c["predict"][t] is not None and t == 0) else None
            pp = np.ascontiguousarray(pred if pred is not None else np.zeros((n, 2)), np.float32)
            po, co, io, no, cn = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(4, np.int32)
            kept = shim.shim_klt_track(hp[t][k].p, hp[t + 1][k].p, n, p.ctypes.data_as(PF), i_.ctypes.data_as(PI), n_.ctypes.data_as(PI), int(pred is not None),
                                       pp.ctypes.data_as(PF), iopt.ctypes.data_as(PI), dopt.ctypes.data_as(C.POINTER(C.c_double)), po.ctypes.data_as(PF), co.ctypes.data_as(PF),
                                       io.ctypes.data_as(PI), no.ctypes.data_as(PI), cn.ctypes.data_as(PI))
            assert kept == len(w["ids"]) and np.array_equal(cn, w["counters"]), (t, k)
            assert np.array_equal(_bits(po[:kept]), _bits(w["prev_pts"])) and np.array_equal(_bits(co[:kept]), _bits(w["cur_pts"]))
            assert np.array_equal(io[:kept], w["ids"]) and np.array_equal(no[:kept], w["track_cnt"])
            nxt.append((co[:kept].copy(), io[:kept].copy(), no[:kept].copy()))
        held = nxt


def _levels_with(name, bit, key=None):
    out = set()
    for k_, per_cam in kc.expected_flows(name).items():
        if key is not None and k_ != key:
            continue
        for w in per_cam:
            out |= {l for l in range(m.MAX_LEVELS) if ((w["trace"][:, l] & bit) == bit).any()}
    return out


def test_the_cases_reach_every_branch():
    """Found by search in the model, asserted here: every way a level can end, at the levels the cases are meant to reach."""
    big = "s180x177_four_levels"
    assert {0, 1} <= _levels_with(big, m.T_PREV_OUT)                       # iprevPt.x < -21 (and beyond the far edges)
    assert {0, 1} <= _levels_with(big, m.T_FLAT)                           # the flat block: level 0 and one level up
    assert {0, 1} <= _levels_with(big, m.T_NEXT_OUT | m.T_MOVED)           # leaves J in mid-iteration at level 0 and at level 1
    assert 0 in _levels_with(big, m.T_EPS) and 0 in _levels_with(big, m.T_OSC) and 0 in _levels_with(big, m.T_COUNT)      # the three terminations
    assert _levels_with(big, m.T_HALF)                                     # a weight product exactly on a half
    assert _levels_with("s640x480", m.T_OSC) and _levels_with("s640x480", m.T_COUNT)
    # the tracking flow: no fallback with 10 successes, the fallback with 9, no prediction
    pr = kc.expected_tracks("prediction")[0]
    assert [r["fallback"] for r in pr] == [False, True, False]
    c = kc.case("prediction")
    P = m.params()
    pyr = kc.pyramids("prediction")
    first = [int(m.flow(pyr[0][k], pyr[1][k], c["pts"][k], c["predict"][0][k], 1, P)["status"].sum()) for k in (0, 1)]
    assert first == [10, 9]
    # every decision of R5 occurs; the grey rule rejects a point that tracked and is in the border
    d = kc.expected_tracks(big)[0][0]["decisions"]
    assert {0, 1, 2, 3} <= set(d.tolist())
    tr = kc.expected_tracks(big)[0][0]
    grey_hits = 0
    full = m.flow(kc.pyramids(big)[0][0], kc.pyramids(big)[1][0], kc.case(big)["pts"][0], None, 3, P)
    for i in np.nonzero(d == 2)[0]:
        cur = full["next_pts"][i]
        if m.in_border(cur, 180, 177, 1):
            grey_hits += int(kc.pyramids(big)[1][0][0]["img"][int(cur[1]) + 21, int(cur[0]) + 21] > 250)
    assert grey_hits >= 1 and len(tr["ids"]) == tr["counters"][3]
    # the reverse test at its boundary: the same point kept at <= and gone one double below
    a, b = kc.expected_tracks("reverse_boundary_kept")[0][0], kc.expected_tracks("reverse_boundary_gone")[0][0]
    assert a["counters"][2] == b["counters"][2] + 1
    # inBorder's rounding on planted cur_pts (x = 0.5, 1.5, cols - 1.5, then the same in y): outside, inside, and by the parity of the size
    for name, far in (("in_border_even", 3), ("in_border_odd", 2)):
        r, c = kc.expected_tracks(name)[0][0], kc.case(name)
        assert not r["fallback"] and r["counters"][1] == r["counters"][2] == 16      # every point tracked and passed the reverse test
        assert r["decisions"][:6].tolist() == [2, 3, far, 2, 3, far], name
        assert np.array_equal(r["cur_pts"].view(np.uint32), c["predict"][0][0][r["decisions"] == 3].view(np.uint32))      # cur_pts is the prediction, bit for bit
    # two consecutive tracks: the second starts from the survivors of the first
    t3 = kc.expected_tracks("three_images")
    assert t3[1][0]["counters"][0] == t3[0][0]["counters"][3] > 0 and (t3[1][0]["track_cnt"] >= 3).all()
    assert kc.expected_tracks("flow_back_off")[0][0]["counters"][1] == kc.expected_tracks("flow_back_off")[0][0]["counters"][2]


def test_sanitized_stand_alone_program():
    """gfbe_klt.h under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _cxx(os.path.join(ROOT, "tests", "klt_host_main.cpp"), os.path.join(BUILD, "klt_host_main"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the model alone: planted translations
# Measured with this texture (seed 1, 200 x 240, 120 points 30 px inside): worst position error of the accepted points 0.0149,
# 0.0172 and 0.0171 px at the translations below, every point accepted. K = the power of two at or above four times the worst
# (0.069): 2^-3.
PLANTED = [(0.3, -0.2), (2.6, 1.3), (7.3, -4.6)]
K_POSITION = 2.0 ** -3


@pytest.mark.parametrize("shift", PLANTED)
def test_model_recovers_a_planted_translation(shift):
    """So that "bits equal the model" cannot hide a wrong model: the texture is sampled analytically at the translation, so the true
    position of every point is known. A condition on the inputs, checked on the CPU."""
    rows, cols = 200, 240
    a, b = gf.synth.klt_image_pair(rows, cols, 1, shift)
    pts = gf.synth.klt_grid_points(rows, cols, 120, seed=1, margin=30.0)
    r = m.track(m.build(a), m.build(b), pts, np.arange(120), np.ones(120))
    err = np.abs(r["cur_pts"].astype(np.float64) - (r["prev_pts"].astype(np.float64) + np.array(shift))).max()
    share = len(r["ids"]) / 120.0
    print("planted", shift, "worst error %.4f px" % err, "accepted %.2f" % share)
    assert err <= K_POSITION and share >= 0.5


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
    par = {"int32_t": C.c_int32, "gfbe_ctx*": C.c_void_p, "gfbe_klt*": C.c_void_p, "gfbe_klt**": P(C.c_void_p), "const gfbe_klt_options*": P(abi.KltOptions),
           "gfbe_klt_options*": P(abi.KltOptions), "const float*": P(C.c_float), "float*": P(C.c_float), "const int32_t*": P(C.c_int32), "int32_t*": P(C.c_int32),
           "const uint8_t*": P(C.c_uint8), "uint8_t*": P(C.c_uint8), "int16_t*": P(C.c_int16)}
    ret = {"void": None, "gfbe_status": C.c_int32}
    table = gf.signatures.KLT
    protos = _prototypes("gfbe_klt.h", "gfbe_klt_")
    assert {p[1] for p in protos} == {"gfbe_klt_" + k for k in table} == set(gf.backend.KLT_EXPORTS) and len(protos) == 8
    assert gf.signatures.TABLES["gfbe_klt_"] is table
    for r, name, params in protos:
        res, args = table[name[len("gfbe_klt_"):]]
        assert res is ret[r], name
        assert len(args) == len(params), name
        for k, (p, a) in enumerate(zip(params, args)):
            assert a is par[p], (name, k, p, a)
    hdr = open(os.path.join(ROOT, "include", "gfbe_klt.h")).read()
    assert "#define GFBE_KLT_WIN 21" in hdr and "#define GFBE_KLT_MAX_LEVEL 7" in hdr and (abi.KLT_WIN, abi.KLT_MAX_LEVEL) == (m.WIN, m.MAX_LEVELS - 1) == (21, 7)
    assert not set(gf.backend.KLT_EXPORTS) & set(gf.backend.EXPORTS) and not set(gf.backend.KLT_EXPORTS) & set(gf.backend.LC6_EXPORTS)      # the surface of gfbe.h is as it was


def test_options_struct_matches_the_c_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gfbe_klt.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(gfbe_klt_options));']
    for f, _ in abi.KltOptions._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(gfbe_klt_options, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.KltOptions) == 56
    for f, _ in abi.KltOptions._fields_:
        assert int(got[f]) == getattr(abi.KltOptions, f).offset, f


def test_c_abi_without_a_device():
    gf.build_native()
    lib = abi.bind(abi.bind(C.CDLL(gf.lib_path()), "gfbe_"), abi.KLT_PREFIX)
    for name in gf.backend.KLT_EXPORTS:
        assert hasattr(lib, name), name
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    o = abi.klt_default_options(lib)
    assert (o.struct_size, o.max_level, o.max_count, o.flow_back, o.border, o.grey_max, o.prediction_min_success, o.reserved, o.epsilon, o.min_eig_threshold,
            o.flow_back_dist) == (C.sizeof(abi.KltOptions), 3, 30, 1, 1, 250, 10, 0, 0.01, 1e-4, 0.5)

    def create(rows=48, cols=64, n=1, cap=16, opt=None):
        h = C.c_void_p(7)
        rc = lib.gfbe_klt_create(ctx, n, rows, cols, cap, C.byref(opt) if opt is not None else None, C.byref(h))
        assert not h.value      # no handle comes back
        return rc
    # a well-formed call fails loudly: no device, no CPU fallback
    assert create() == abi.NO_DEVICE and b"gfbe_klt_create" in lib.gfbe_last_error(ctx) and b"no CPU fallback" in lib.gfbe_last_error(ctx)
    for rows, cols in ((21, 64), (48, 21), (0, 0), (-5, 64)):      # rows or cols <= 21
        assert create(rows, cols) == abi.BAD_INPUT and b"21 x 21" in lib.gfbe_last_error(ctx)
    assert create(22, 22) == abi.NO_DEVICE
    assert create(n=0) == abi.BAD_INPUT and create(cap=0) == abi.BAD_INPUT
    for kw in (dict(struct_size=C.sizeof(abi.KltOptions) - 8), dict(struct_size=0), dict(struct_size=C.sizeof(abi.Lc6Options)), dict(max_level=8), dict(max_level=-1),
               dict(border=-1), dict(epsilon=float("nan"))):
        assert create(opt=abi.klt_default_options(lib, **kw)) == abi.BAD_INPUT, kw
    # the calls on a handle: no device comes first (there can be no handle)
    fake = C.c_void_p(1)
    assert lib.gfbe_klt_push_image(ctx, fake, None) == abi.NO_DEVICE and b"no CPU fallback" in lib.gfbe_last_error(ctx)
    out = np.full(8, -7, np.int32)
    assert lib.gfbe_klt_track(ctx, fake, None, None, out.ctypes.data_as(PI), None, None, None, None, None) == abi.NO_DEVICE and (out == -7).all()
    assert lib.gfbe_klt_flow(ctx, fake, 0, 3, 0, out.ctypes.data_as(PI), None, None, None, None) == abi.NO_DEVICE
    assert lib.gfbe_klt_set_points(ctx, fake, out.ctypes.data_as(PI), None, None, None) == abi.NO_DEVICE
    assert lib.gfbe_klt_download_level(ctx, fake, 0, 0, 0, None, None, out.ctypes.data_as(PI)) == abi.NO_DEVICE and (out == -7).all()
    lib.gfbe_klt_destroy(ctx, None)
    lib.gfbe_destroy(ctx)


def test_point_checks_name_the_rule(shim):
    def chk(off, cap, pts):
        o, p = np.array(off, np.int32), np.ascontiguousarray(pts, np.float32)
        return shim.shim_klt_check_points(len(o) - 1, o.ctypes.data_as(PI), cap, p.ctypes.data_as(PF))
    p = np.arange(12, dtype=np.float32)
    assert chk([0, 2, 6], 4, p) == 0 and chk([0, 0, 0], 4, p) == 0
    assert chk([0, 5, 6], 4, p) == 1 and chk([1, 2, 6], 4, p) == 1 and chk([0, 4, 3], 4, p) == 1      # above the capacity, not from 0, descending
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[7] = bad
        assert chk([0, 2, 6], 4, q) == 2 and chk([0, 2, 3], 4, q) == 0
