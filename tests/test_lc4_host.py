"""The HIP-free half of the loop-closure pose graph (ground-fusion2_amd/csrc/gfbe_loopgraph.h) without a GPU: compiled for the host by a
plain C++ compiler through tests/lc4_host_shim.cpp and held against the model (tests/lc4_np.py) on factors, sequence measurements and
plan; the same header under the address and undefined-behaviour sanitizers in a program of its own (tests/lc4_host_main.cpp); and the
C ABI's contract without a device: GFBE_NO_DEVICE, and every GFBE_BAD_INPUT case with nothing written."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import lc4_cases as lc
import lc4_np as m

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
HDR = os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_loopgraph.h")
PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _p(a):
    return a.ctypes.data_as(PD)


def _cxx(src, out, extra):
    if not CXX:
        pytest.fail("no C++ compiler: gfbe_loopgraph.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, HDR)):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_cxx(os.path.join(ROOT, "tests", "lc4_host_shim.cpp"), os.path.join(BUILD, "lc4_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_lc4_normalize_angle.restype = C.c_double
    lib.shim_lc4_normalize_angle.argtypes = [C.c_double]
    lib.shim_lc4_eval.argtypes = [C.c_int, PD, PD, PI, PI, C.POINTER(C.c_ubyte), PD, C.c_double, C.c_double, PD, PD, PD]
    lib.shim_lc4_sequence_meas.argtypes = [PD, PD, PD, PD, PD]
    lib.shim_lc4_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    lib.shim_lc4_check_graph.argtypes = [C.c_int, C.c_int, PI, PI, C.c_int, C.POINTER(C.c_ubyte)]
    return lib


def test_the_header_has_no_hip_in_it():
    src = open(HDR).read()
    assert "hip/hip_runtime" not in src and "hipLaunch" not in src and "__global__" not in src


def test_normalize_angle_is_a_single_wrap(shim):
    for a in (0.0, 180.0, -180.0, 180.0000001, -180.0000001, 359.0, -359.0, 541.0, -541.0):
        assert shim.shim_lc4_normalize_angle(a) == float(m.normalize_angle(np.float64(a)))
    assert shim.shim_lc4_normalize_angle(541.0) == 181.0      # one wrap only, as the reference's NormalizeAngle


def _host_eval(shim, e):
    t, ypr, meas = (np.ascontiguousarray(e[k], np.float64) for k in ("t", "ypr", "meas"))
    ei, ej, kd = np.ascontiguousarray(e["edge_i"], np.int32), np.ascontiguousarray(e["edge_j"], np.int32), np.ascontiguousarray(e["kind"], np.uint8)
    E = len(ei)
    r, J, ce = np.zeros((E, 4)), np.zeros((E, 4, 8)), np.zeros(E)
    shim.shim_lc4_eval(E, _p(t), _p(ypr), ei.ctypes.data_as(PI), ej.ctypes.data_as(PI), kd.ctypes.data_as(C.POINTER(C.c_ubyte)), _p(meas),
                       e["opt"]["huber_delta"], e["opt"]["loop_yaw_div"], _p(r), _p(J), _p(ce))
    return dict(r=r, J=J, cost=float(np.sum(ce)), cost_e=ce)


@pytest.mark.parametrize("name", ["n2_loop_into_constant", "n64_shapes", "n65_64_loops", "n257_two_sequences", "yaw_wrap", "far_start"])
def test_host_build_agrees_with_the_model_on_factors(shim, name):
    e = lc.eval_case(name)
    got = _host_eval(shim, e)
    ref = m.eval_edges(e["ypr"][:, 0], e["t"], e["edge_i"], e["edge_j"], e["kind"], e["meas"], e["opt"], m.LD)
    rr = lc.eval_ratios(got, ref)
    print(name, "host build worst ratios", rr)
    assert rr["r"] <= lc.K["r"] and rr["J"] <= lc.K["J"] and rr["cost"] <= lc.K["eval_cost"]
    # the structure of the Jacobian: d r_t / d t_j = -d r_t / d t_i, the yaw row is -w, +w, nothing else
    J = got["J"]
    assert np.array_equal(J[:, :3, 1:4], -J[:, :3, 5:8]) and not J[:, :3, 4].any() and not J[:, 3, 1:4].any() and not J[:, 3, 5:8].any()
    assert np.array_equal(J[:, 3, 0], -J[:, 3, 4])


def test_host_build_forms_the_sequence_measurement_of_the_model(shim):
    g = lc.cases()["n64_shapes"]["g"]
    t, ypr = np.ascontiguousarray(g["t"]), np.ascontiguousarray(g["ypr"])
    for a, b in ((0, 1), (3, 7), (10, 12), (59, 63)):
        out = np.zeros(6)
        shim.shim_lc4_sequence_meas(_p(t[a]), _p(ypr[a]), _p(t[b]), _p(ypr[b]), _p(out))
        want = m.sequence_meas(t[a], ypr[a], t[b], ypr[b], m.LD)
        A = np.abs(t[a]).sum() + np.abs(t[b]).sum()
        assert (np.abs(out[:3].astype(m.LD) - want[:3]).astype(float) <= 8 * m.U * (1 + np.abs(np.deg2rad(ypr[a])).sum()) * A).all()
        assert out[3] == ypr[b, 0] - ypr[a, 0] and out[4] == ypr[a, 1] and out[5] == ypr[a, 2]      # un-normalised; pitch and roll of the first pose


# n: (super-blocks, padding poses, sweeps)
PLAN = {1: (1, 3, 0), 2: (1, 2, 0), 4: (1, 0, 0), 5: (2, 3, 1), 63: (16, 1, 4), 64: (16, 0, 4), 65: (17, 3, 5)}


@pytest.mark.parametrize("n", sorted(PLAN))
def test_plan_padding_and_sweeps(shim, n):
    for L in (0, 1, 3, 4, 63, 64):
        out = (C.c_longlong * 11)()
        assert shim.shim_lc4_plan(n, L, out) == 1
        M, rows, pad, sweeps, ncol, ld, ntile, cap, cap_ld, total, ok = list(out)
        assert (M, pad, sweeps) == PLAN[n] and rows == 16 * M
        assert ncol == 1 + 4 * L and ld == 16 * ntile and ld >= ncol > ld - 16
        assert cap == 4 * L and cap_ld % 16 == 0 and cap_ld >= max(cap, 16) and cap_ld < max(cap, 1) + 16
        p = m.plan(n, L)
        assert (M, rows, pad, sweeps, ncol, ntile, ld, cap, cap_ld) == tuple(p[k] for k in ("M", "rows", "pad_poses", "sweeps", "ncol", "ntile", "ld", "cap", "cap_ld"))
        assert ok == 1 and total > 0      # every carved array lies inside the slab, on a 256-byte boundary, in order
    out = (C.c_longlong * 11)()
    assert shim.shim_lc4_plan(0, 0, out) == 0 and shim.shim_lc4_plan(n, 65, out) == 0 and shim.shim_lc4_plan(n, -1, out) == 0


def test_graph_check_names_the_rule(shim):
    def chk(n, li, lc_, span=4):
        a, b = np.array(li, np.int32), np.array(lc_, np.int32)
        return shim.shim_lc4_check_graph(n, len(a), a.ctypes.data_as(PI), b.ctypes.data_as(PI), span, (C.c_ubyte * n)())
    assert chk(8, [3, 5, 7], [0, 2, 6]) == 0 and chk(8, [], []) == 0
    assert chk(8, [8], [0]) == 4 and chk(8, [3], [-1]) == 4
    assert chk(8, [2], [2]) == 5 and chk(8, [2], [5]) == 5
    assert chk(8, [3, 3], [0, 1]) == 6
    assert chk(8, [3], [0], span=5) == 3 and chk(8, [3], [0], span=0) == 3
    assert chk(100, list(range(1, 66)), [0] * 65) == 2


def test_sanitized_stand_alone_program():
    """gfbe_loopgraph.h under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _cxx(os.path.join(ROOT, "tests", "lc4_host_main.cpp"), os.path.join(BUILD, "lc4_host_main"),
               ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_c_abi_without_a_device():
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    lib.gfbe_create.restype = abi.c_i
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    lg = abi.LoopGraph(lib, "gfbe_", ctx)
    o = lg.options()
    assert (o.struct_size, o.max_num_iterations, o.span, o.huber_delta, o.loop_yaw_div) == (C.sizeof(abi.Lc4Options), 5, 4, 0.1, 10.0)
    assert abi.LC4_MAX_LOOPS == m.MAX_LOOPS == 64
    hdr = open(os.path.join(ROOT, "include", "gfbe.h")).read()
    assert "#define GFBE_LC4_MAX_LOOPS 64" in hdr
    g = gf.synth.loop_graph(n=100, n_loop=4, seed=3)
    args = [g[k] for k in lc.ARG_KEYS]
    e = lc.eval_case("n5_no_loop")
    ev = (e["t"], e["ypr"], e["edge_i"], e["edge_j"], e["kind"], e["meas"])
    # a well-formed call fails loudly: no device, no CPU fallback
    rc, out = lg.solve_rc(*args)
    assert rc == abi.NO_DEVICE and np.isnan(out["t"]).all() and np.isnan(out["yaw"]).all() and np.isnan(out["drift"]).all()
    assert lg.eval_rc(*ev)[0] == abi.NO_DEVICE
    lib.gfbe_last_error.restype = C.c_char_p
    lib.gfbe_last_error.argtypes = [C.c_void_p]
    assert b"no CPU fallback" in lib.gfbe_last_error(ctx)

    def bad(**kw):
        a = dict(zip(lc.ARG_KEYS, args))
        opt = kw.pop("opt", None)
        a.update(kw)
        rc, out = lg.solve_rc(*[a[k] for k in lc.ARG_KEYS], opt=opt)
        assert rc == abi.BAD_INPUT, kw
        assert np.isnan(out["t"]).all() and np.isnan(out["yaw"]).all() and np.isnan(out["drift"]).all() and out["summary"]["iterations"] == 0      # nothing written
    many = gf.synth.loop_graph(n=100, n_loop=65, seed=3)
    bad(loop_i=many["loop_i"], loop_c=many["loop_c"], loop_meas=many["loop_meas"])                   # n_loop > 64
    li, lcc = g["loop_i"].copy(), g["loop_c"].copy()
    bad(loop_i=np.array([100, *li[1:]], np.int32))                                                   # an index out of range
    bad(loop_c=np.array([-1, *lcc[1:]], np.int32))
    bad(loop_c=np.array([li[0], *lcc[1:]], np.int32))                                                # loop_c >= loop_i
    bad(loop_c=np.array([li[0] + 1, *lcc[1:]], np.int32))
    bad(loop_i=np.array([li[1], *li[1:]], np.int32), loop_c=np.array([0, *lcc[1:]], np.int32))       # two loops on one pose
    bad(opt=lg.options(struct_size=C.sizeof(abi.Lc4Options) - 8))                                    # a struct of another size
    bad(opt=lg.options(struct_size=0))
    bad(opt=lg.options(span=5))
    assert lg.eval_rc(*ev, opt=lg.options(struct_size=4))[0] == abi.BAD_INPUT
    ej = np.array(e["edge_j"]).copy()
    ej[0] = len(e["t"])
    assert lg.eval_rc(e["t"], e["ypr"], e["edge_i"], ej, e["kind"], e["meas"])[0] == abi.BAD_INPUT
    lib.gfbe_destroy(ctx)
