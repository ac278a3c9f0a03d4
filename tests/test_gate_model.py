"""The sensor gate without a GPU: the host build of ground-fusion2_amd/csrc/gfbe_gate.h (tests/gate_host_shim.cpp) against the model
tests/gate_np.py, bit for bit, on the cases of tests/gate_cases.py; G5's fixed-order sum against the reference's sequential sum in
numpy.longdouble; G2 against an independent statement with rotation matrices; the case condition of every case the GPU test uses; the same
header under the address and undefined-behaviour sanitizers in a program of its own (tests/gate_host_main.cpp); the binding
(include/gfbe_gate.h against signatures.GATE, the layout of gfbe_gate_options against a compiled C program, the other surfaces disjoint);
and the C ABI's refusals that need no device (the ones that need a handle are in tests/test_gpu_gate.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import gate_cases as gc
import gate_np as m

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = gc.CASES
PD = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def shim():
    try:
        return gc.load_shim()
    except (RuntimeError, subprocess.CalledProcessError) as e:
        pytest.fail(str(e))


def opts(name):
    return m.options(**CASES[name][0])


def test_the_header_has_no_hip_in_it():
    src = open(gc.HEADER).read()
    assert "hip/hip_runtime" not in src and "hipLaunch" not in src and "__global__" not in src and "__shfl" not in src


# ---- the host build of the shared header against the model
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_build_equals_the_model(shim, name):
    o, tabs, want = opts(name), gc.tables(name), gc.expected(name)
    gc.assert_same(gc.shim_frame(shim, o, tabs, CASES[name][2]), want["frame"], (name, "frame"))
    for mode in (0, 1):
        gc.assert_same(gc.shim_stats(shim, o, mode, tabs), want["stats"][mode], (name, "pair_stats", mode))
        for l, r in gc.LR:
            for b, t in enumerate(tabs):
                a, bb = gc.shim_corres(shim, o, mode, t, l, r)
                wa, wb = want["corres"][mode, l, r][b]
                assert np.array_equal(gc.bits(a), gc.bits(wa)) and np.array_equal(gc.bits(bb), gc.bits(wb)), (name, mode, l, r, b)


def test_frame_statistics_are_the_pair_statistics_of_its_mode():
    for name in CASES:
        e = gc.expected(name)
        gc.assert_same(e["frame"], e["stats"][opts(name)["depth_mode"]], name)


# ---- G5: the fixed-order sum against the reference's sequential sum
def test_sum_order_against_the_sequential_sum():
    """Both are sums of n non-negative terms in some order, each with at most n - 1 roundings of relative size 2^-53 on partial sums that
    never exceed the exact sum S (1 + 2^-53)^(n - 1): either lies within (n - 1) 2^-53 S (first order) of S, so they differ by at most
    2 (n - 1) 2^-53 S. The longdouble sum's own roundings (2^-64) are far inside that."""
    flips = []
    for name in sorted(CASES):
        o = opts(name)
        for mode in (0, 1):
            st = gc.expected(name)["stats"][mode]
            for b, t in enumerate(gc.tables(name)):
                seq = np.zeros(m.NL, np.longdouble)
                for l in range(m.NL):
                    seq[l], n = m.sequential_sum(o, mode, t, l)
                    assert n == st["pair_count"][b, l]
                    got = np.longdouble(st["pair_sum"][b, l])
                    assert abs(got - seq[l]) <= 2 * max(n - 1, 0) * np.longdouble(2.0) ** -53 * seq[l], (name, mode, b, l, got, seq[l])
                d_seq = m.decide(o, st["pair_count"][b], seq.astype(np.float64))
                if d_seq != (st["l_still"][b], st["l_init"][b]):
                    flips.append((name, mode, b))
    # only the tables built to sit on a threshold may depend on the order (their terms are the same in both modes: depth 1, z 1)
    assert all(f[0] == "straddle" for f in flips), flips


# ---- G2 by a method that shares nothing with the model: rotation matrices from synth.qrot, numpy products
def wheel_independent(rb):
    P, R, V = np.array(rb["pose"][:3]), np.array(rb["pose"][3:]).reshape(3, 3), np.array(rb["vel_ba"][:3])
    v0, g0, dPw = np.array(rb["wheel_first"][:3]), np.array(rb["wheel_first"][3:]), np.zeros(3)
    if rb["frame_count"] == 0:
        return dPw, P, R, V
    for s in rb["wheel"]:
        dt, v, w = s[0], s[1:4], s[4:7]
        un_vel_0 = R @ v0
        if not rb["stationary_prev"]:
            q = np.concatenate([0.5 * (g0 + w) * dt / 2.0, [1.0]])
            R = R @ gf.synth.qrot(q / np.linalg.norm(q))
            V = 0.5 * (R @ v + un_vel_0)
            P = P + dt * V
        else:
            V = np.zeros(3)
        dPw = dPw + dt * np.array([-V[1], V[0], -V[2]])
        v0, g0 = v, w
    return dPw, P, R, V


def test_wheel_prediction_against_rotation_matrices():
    seen = 0
    for name in sorted(CASES):
        for rb in CASES[name][2]:
            got = m.wheel_predict(rb["frame_count"], rb["wheel"], rb["wheel_first"], rb["stationary_prev"], rb["pose"][:3], rb["pose"][3:], rb["vel_ba"][:3])
            for g, w in zip(got, wheel_independent(rb)):
                g, w = np.array(g, np.float64).ravel(), np.asarray(w).ravel()
                assert np.abs(g - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), name
            seen += len(rb["wheel"]) > 0 and rb["frame_count"] != 0
    assert seen >= 8


def test_delta_rot_is_a_rotation(shim):
    rng = np.random.default_rng(5)
    for _ in range(20):
        th = rng.normal(0, 0.3, 3)
        M = np.zeros(9)
        shim.shim_gate_delta_rot(th.ctypes.data_as(PD), M.ctypes.data_as(PD))
        assert np.array_equal(gc.bits(M), gc.bits(m.delta_rot(m.f64(th))))
        M = M.reshape(3, 3)
        assert np.abs(M.T @ M - np.eye(3)).max() < 1e-15 * 8 and abs(np.linalg.det(M) - 1) < 1e-15 * 8


def test_var_without_guards(shim):
    """G4: M == 1 and a zero sum_dt give NaN by IEEE rules (the quiet NaN, deviation c), M == 2 gives 0"""
    for frames, want_nan in ((np.array([[0.1, 0.2, 0.3, 0.1]]), True), (np.array([[0.0, 0, 0, 0.1], [0.1, 0.2, 0.3, 0.0], [0.1, 0.2, 0.3, 0.1]]), True),
                             (np.array([[0.0, 0, 0, 0.1], [0.0, 0.0, 0.0, 0.0]]), True), (np.array([[0.0, 0, 0, 0.1], [0.1, 0.2, 0.3, 0.1]]), False)):
        got, want = shim.shim_gate_var(frames.ctypes.data_as(PD), len(frames)), m.var_of(frames)
        assert np.array_equal(gc.bits([got]), gc.bits([want])) and bool(np.isnan(got)) == want_nan
        if want_nan:
            assert gc.bits([got])[0] == 0x7FF8000000000000
        else:
            assert got == 0.0


# ---- the case condition of every case the GPU test uses
def test_cases_are_what_they_claim():
    E = {name: gc.expected(name) for name in CASES}
    assert sorted(gc.GPU_CASES) == sorted(CASES)
    T = gc.tables("mix3")
    assert [len(t["start_frame"]) for t in T] == [0, 30, 1100] and (1100 + 1023) // 1024 == 2 and 1100 % 2 == 0 and 1100 // 2 < 1024      # chunks of 2, threads 550 .. 1023 idle
    for name in ("mix3", "pingpong", "depth0"):
        for t in gc.tables(name)[-1:]:
            s, n = t["start_frame"], t["n_obs"]
            assert (n == 11).any() and ((s + n - 1 < 10) & (s == 0)).any() and (s > 0).any() and len(set(s.tolist())) >= 4 and len(set(n.tolist())) >= 5, name
    f = E["mix3"]["frame"]
    assert np.isnan(f["var"][0]) and np.isnan(f["var"][1]) and f["var"][2] > 0.35 and f["flags"][2] & m.ANOMALY and f["dis"][2] > 0.02 and f["l_init"][2] == 0
    assert [len(r["imu"]) for r in CASES["mix3"][2]] == [0, 1, 20] and [len(r["wheel"]) for r in CASES["mix3"][2]] == [0, 1, 5]
    assert [len(r["frames"]) for r in CASES["mix3"][2]] == [1, 6, 12] and (CASES["mix3"][2][1]["frames"][:, 3] == 0).any()
    assert [r["stationary_prev"] for r in CASES["mix3"][2]] == [0, 1, 0] and (f["vel_out"][1] == 0).all()      # (the zero-velocity update)
    assert not (f["pose_out"][2] == CASES["mix3"][2][2]["pose"]).all()
    # at rest every detector agrees
    f = E["rest1"]["frame"]
    assert f["flags"][0] == m.WHEEL | m.PREINT | m.VAR | m.VISUAL | m.IMU | m.SYSTEM and f["l_still"][0] >= 0
    assert max(np.linalg.norm(f["dP_imu"][0]), np.linalg.norm(f["dP_wheel"][0])) < 0.001
    # the other half of the ping-pong buffers: the model's table after remove_back differs from the one before it
    before = gc.model_tables(CASES["pingpong"][1][:-2], 1)[0]
    after = gc.tables("pingpong")[0]
    assert CASES["pingpong"][1][-2] == ("remove_back",) and len(before["start_frame"]) != len(after["start_frame"])
    assert E["pingpong"]["frame"]["pair_count"].max() > 20 and not E["pingpong"]["frame"]["flags"][0] & m.ANOMALY and E["pingpong"]["frame"]["dis"][0] < 0.02
    for name in ("short", "fc0"):
        f = E[name]["frame"]
        assert not f["pair_count"].any() and (f["l_still"] == -1).all() and (f["l_init"] == -1).all(), name
    assert CASES["short"][2][0]["frame_count"] == 5 and max(t["start_frame"].max() for t in gc.tables("short")) == 5
    f = E["fc0"]["frame"]
    assert not f["dP_imu"].any() and not f["dP_wheel"].any() and all(len(r["imu"]) for r in CASES["fc0"][2]) and (f["pose_out"] == [r["pose"] for r in CASES["fc0"][2]]).all()
    f = E["nowheel"]["frame"]
    assert not (f["flags"] & (m.ANOMALY | m.WHEEL | m.PREINT | m.IMU)).any() and not f["dP_wheel"].any() and f["flags"][0] & m.VAR and f["flags"][0] & m.VISUAL
    assert not f["flags"][0] & m.SYSTEM and np.array_equal(f["dis"], np.linalg.norm(f["dP_imu"], axis=1)) and (f["vel_out"] == [r["vel_ba"][:3] for r in CASES["nowheel"][2]]).all()
    f = E["nodetect"]["frame"]
    assert f["dis"][0] > 0.02 and not f["flags"][0] & m.ANOMALY
    assert any(not np.array_equal(E["depth0"]["stats"][0][k], E["depth0"]["stats"][1][k]) for k in ("pair_count", "l_still"))
    # thresholds: 20 members do not count, 21 do, and the earlier pair does not block the later one; the depth bounds are inside; the lowest l wins
    s0, s1 = E["thresholds"]["stats"][0], E["thresholds"]["stats"][1]
    assert s1["pair_count"][0].tolist() == [20] + [21] * 9 and s1["l_still"][0] == 1 and s1["pair_sum"][0, 0] / 20 * 460 < 0.5
    assert s1["pair_count"][1].tolist() == [24] * 10 and s0["pair_count"][1].tolist() == [34] * 10
    t = gc.tables("thresholds")[1]["obs8"][:, :, 7]
    assert (t == 0.1).any() and (t == 10.0).any() and (t == np.nextafter(0.1, 0)).any() and (t == np.nextafter(10.0, 11)).any()
    assert s1["l_init"][2] == 0 and (s1["pair_sum"][2] / 25 * 460 > 30).all() and (s1["pair_count"][2] == 25).all()
    # the straddling pairs: one step of one feature's coordinate flips the model's decision
    s1, T = E["straddle"]["stats"][1], gc.tables("straddle")
    assert s1["l_still"].tolist()[:2] == [0, 1] and s1["l_init"].tolist()[2:] == [-1, 0]
    for a, b in ((0, 1), (2, 3)):
        xa, xb = T[a]["obs8"][0, 0, 0], T[b]["obs8"][0, 0, 0]
        assert np.nextafter(xa, np.inf) == xb and np.array_equal(np.delete(T[a]["obs8"][:, :, :3].ravel(), 0), np.delete(T[b]["obs8"][:, :, :3].ravel(), 0))


# ---- the sanitized stand-alone program
def test_sanitized_stand_alone_program(tmp_path):
    """gfbe_gate.h under -fsanitize=address,undefined in a program of its own (never on code loaded into Python): every case, byte for byte."""
    try:
        exe = gc.build(os.path.join(ROOT, "tests", "gate_host_main.cpp"), os.path.join(gc.BUILD, "gate_host_main"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    except (RuntimeError, subprocess.CalledProcessError) as e:
        pytest.fail(str(e))
    path = str(tmp_path / "cases.bin")
    gc.dump(path, sorted(CASES))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


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
    par = {"int32_t": C.c_int32, "double": C.c_double, "gfbe_ctx*": C.c_void_p, "gfbe_gate*": C.c_void_p, "gfbe_ftab*": C.c_void_p, "gfbe_gate**": P(C.c_void_p),
           "const gfbe_gate_options*": P(abi.GateOptions), "gfbe_gate_options*": P(abi.GateOptions), "const int32_t*": P(C.c_int32), "int32_t*": P(C.c_int32),
           "const double*": P(C.c_double), "double*": P(C.c_double)}
    ret = {"void": None, "gfbe_status": C.c_int32}
    table = gf.signatures.GATE
    protos = _prototypes("gfbe_gate.h", "gfbe_gate_")
    assert {p[1] for p in protos} == {"gfbe_gate_" + k for k in table} == set(gf.backend.GATE_EXPORTS) and len(protos) == 6
    assert gf.signatures.TABLES["gfbe_gate_"] is table and abi.GATE_PREFIX == "gfbe_gate_"
    for r, name, params in protos:
        res, args = table[name[len("gfbe_gate_"):]]
        assert res is ret[r], name
        assert len(args) == len(params), name
        for k, (p, a) in enumerate(zip(params, args)):
            assert a is par[p], (name, k, p, a)
    src = open(os.path.join(ROOT, "include", "gfbe_gate.h")).read()
    for bit, name in ((m.ANOMALY, "WHEEL_ANOMALY"), (m.WHEEL, "WHEEL_STATIONARY"), (m.PREINT, "PREINT_STATIONARY"), (m.VAR, "VAR_STATIONARY"), (m.EXCITED, "IMU_EXCITED"),
                      (m.VISUAL, "VISUAL_STATIONARY"), (m.IMU, "IMU_STATIONARY"), (m.SYSTEM, "SYSTEM_STATIONARY")):
        assert re.search(r"GFBE_GATE_%s = %d\b" % (name, bit), src) and getattr(abi, "GATE_" + name) == bit, name


def test_the_other_surfaces_are_disjoint():
    b = gf.backend
    others = (set(b.EXPORTS) | set(b.LC6_EXPORTS) | set(b.KLT_EXPORTS) | set(b.DET_EXPORTS) | set(b.OBS_EXPORTS) | set(b.KFD_EXPORTS) | set(b.PNP_EXPORTS) | set(b.EQ_EXPORTS) |
              set(b.RCCL_EXPORTS))
    assert not set(b.GATE_EXPORTS) & others and all(n.startswith("gfbe_gate_") for n in b.GATE_EXPORTS)
    assert len(others) == len(b.EXPORTS) + 50 + len(b.RCCL_EXPORTS)      # (the seven companion headers before this one: 3 + 8 + 7 + 9 + 10 + 6 + 7)
    src = open(os.path.join(ROOT, "ground-fusion2_amd", "abi.py")).read()
    tail = src[src.index("GATE_PREFIX"):]
    assert ".restype" not in tail and ".argtypes" not in tail and "class SensorGate(Handle)" in tail


def test_options_struct_matches_the_c_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gfbe_gate.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(gfbe_gate_options));']
    for f, _ in abi.GateOptions._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(gfbe_gate_options, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.GateOptions) == 112
    for f, _ in abi.GateOptions._fields_:
        assert int(got[f]) == getattr(abi.GateOptions, f).offset, f


# ---- the refusals that need no device
def test_c_abi_without_a_device():
    gf.build_native()
    lib = abi.bind(abi.bind(C.CDLL(gf.lib_path()), "gfbe_"), abi.GATE_PREFIX)
    for name in gf.backend.GATE_EXPORTS:
        assert hasattr(lib, name), name
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    o = abi.gate_default_options(lib)
    assert o.struct_size == C.sizeof(abi.GateOptions) and {k: getattr(o, k) for k in m.DEFAULTS} == m.DEFAULTS and o.reserved == 0

    def create(opt=None, n=3):
        h = C.c_void_p(7)
        rc = lib.gfbe_gate_create(ctx, n, C.byref(opt) if opt is not None else None, C.byref(h))
        assert not h.value      # no handle comes back
        return rc
    # a well-formed call fails loudly: no device, no CPU fallback
    assert create() == abi.NO_DEVICE and b"gfbe_gate_create" in lib.gfbe_last_error(ctx) and b"no CPU fallback" in lib.gfbe_last_error(ctx)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(struct_size=C.sizeof(abi.GateOptions) - 8), dict(struct_size=0), dict(max_samples=0), dict(max_samples=65537), dict(max_frames=0), dict(max_frames=4097),
               dict(use_wheel=2), dict(use_wheel=-1), dict(wdetect=2), dict(depth_mode=2), dict(depth_mode=-1), dict(min_pair_count=-1), dict(dis_threshold=-1.0),
               dict(dis_threshold=nan), dict(wheel_still_norm=-1e-9), dict(preint_still_norm=inf), dict(var_still=nan), dict(var_excited=inf), dict(still_parallax_px=nan),
               dict(init_parallax_px=inf), dict(parallax_focal=0.0), dict(parallax_focal=nan), dict(depth_min=nan), dict(depth_max=inf), dict(depth_min=2.0, depth_max=1.0)):
        assert create(abi.gate_default_options(lib, **kw)) == abi.BAD_INPUT and b"gfbe_gate_create" in lib.gfbe_last_error(ctx), kw
    assert create(n=0) == abi.BAD_INPUT and create(n=65537) == abi.BAD_INPUT
    assert create(abi.gate_default_options(lib, max_samples=65536, max_frames=4096, use_wheel=0, wdetect=0, depth_mode=0, min_pair_count=0, depth_min=1.0, depth_max=1.0), n=65536) == abi.NO_DEVICE
    fake = C.c_void_p(1)
    oi, od = np.full(40, -7, np.int32), np.full(40, -7.0)
    pi, pd = oi.ctypes.data_as(C.POINTER(C.c_int32)), od.ctypes.data_as(PD)
    assert lib.gfbe_gate_frame(ctx, fake, fake, pi, pi, pd, pd, pi, pd, pd, pd, pd, 9.8, pi, pi, pd, pi, pi, pi, pi, pd, pd, pd, pd, pd, pd, pd) == abi.NO_DEVICE
    assert b"no CPU fallback" in lib.gfbe_last_error(ctx)
    assert lib.gfbe_gate_pair_stats(ctx, fake, fake, 1, pi, pd, pi, pi) == abi.NO_DEVICE
    assert lib.gfbe_gate_corresponding(ctx, fake, fake, 1, pi, pi, pi, pd, pd, pi) == abi.NO_DEVICE
    assert (oi == -7).all() and (od == -7.0).all()
    assert lib.gfbe_gate_frame(None, fake, fake, pi, pi, pd, pd, pi, pd, pd, pd, pd, 9.8, pi, pi, pd, pi, pi, pi, pi, pd, pd, pd, pd, pd, pd, pd) == abi.BAD_INPUT
    lib.gfbe_gate_destroy(ctx, None)
    lib.gfbe_destroy(ctx)
