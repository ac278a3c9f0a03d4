"""gfbe_lc4_solve_long without a GPU: the plan and the graph check of the long path (ground-fusion2_amd/csrc/gfbe_loopgraph.h) compiled
for the host through tests/lc4_long_host_shim.cpp and held against the model's plan; the same header under the address and
undefined-behaviour sanitizers in a program of its own (tests/lc4_long_host_main.cpp); the C ABI's contract without a device; and the
rules the cases of tests/lc4_long_cases.py have to satisfy before the device is compared with them (tests/test_gpu_lc4_long.py):
decision margins >= 1e3 u A, FP64 and longdouble decide alike, 4 r_cpu <= K of tests/lc4_cases.py, and the recorded reference of the
512-loop case belongs to the arrays synth.loop_graph produces today.

Measured here (FP64 against longdouble, units u A_X): r_cpu pose 4.0e-4, cost 0.015 over the live cases, 9.9e-5 / 0.0093 recorded for
n700_512_loops; smallest decision margin 7.5e4 u A (n200_80_loops)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import lc4_cases as lc
import lc4_long_cases as ll
import lc4_np as m

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
HDR = os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_loopgraph.h")
PI = C.POINTER(C.c_int)
LIVE = list(ll.cases())


def _cxx(src, out, extra):
    if not CXX:
        pytest.fail("no C++ compiler: gfbe_loopgraph.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, HDR)):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_cxx(os.path.join(ROOT, "tests", "lc4_long_host_shim.cpp"), os.path.join(BUILD, "lc4_long_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_lc4_long_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    lib.shim_lc4_long_check_graph.argtypes = [C.c_int, C.c_int, PI, PI, C.c_int, C.POINTER(C.c_ubyte)]
    return lib


@pytest.mark.parametrize("n", [1, 5, 64, 65, 700, 5000])
def test_long_plan_is_the_models_plan(shim, n):
    last = 0
    for L in (0, 64, 65, 129, 512):
        out = (C.c_longlong * 11)()
        assert shim.shim_lc4_long_plan(n, L, out) == 1
        M, rows, pad, sweeps, ncol, ld, ntile, cap, cap_ld, total, ok = list(out)
        p = m.plan(n, L)
        assert (M, rows, pad, sweeps, ncol, ntile, ld, cap, cap_ld) == tuple(p[k] for k in ("M", "rows", "pad_poses", "sweeps", "ncol", "ntile", "ld", "cap", "cap_ld"))
        assert ok == 1      # every carved array on a 256-byte boundary, in order, the last inside total
        assert total >= 2 * rows * ld + 2 * cap_ld * cap_ld and total > last
        last = total
    out = (C.c_longlong * 11)()
    assert shim.shim_lc4_long_plan(n, 513, out) == 0 and shim.shim_lc4_long_plan(n, -1, out) == 0 and shim.shim_lc4_long_plan(0, 65, out) == 0
    assert shim.shim_lc4_long_max_loops() == 512


def test_scratch_at_the_cap_is_what_the_header_states(shim):
    out = (C.c_longlong * 11)()
    assert shim.shim_lc4_long_plan(5000, 512, out) == 1
    rows, ld, cap_ld, total = out[1], out[5], out[8], out[9]
    assert (rows, ld, cap_ld) == (20000, 2064, 2048) and rows * ld > 2 ** 25
    assert 0.74e9 < 8 * total < 0.76e9      # the plan's 0.75 GB (gfbe_loopgraph.h); with the linearisation sets include/gfbe.h states 0.78 GB
    assert 0 <= total - (2 * rows * ld + 2 * cap_ld ** 2 + 161 * rows + 18 * cap_ld) < 32 * 20      # the formula, rounded up to 256-byte units
    assert 8 * (2 * rows * ld + 2 * cap_ld ** 2 + 330 * rows + 140 * 512 + 18 * cap_ld) < 0.79e9


def test_long_graph_check_lifts_the_limit_only(shim):
    def chk(n, li, lc_, span=4):
        a, b = np.array(li, np.int32), np.array(lc_, np.int32)
        return shim.shim_lc4_long_check_graph(n, len(a), a.ctypes.data_as(PI), b.ctypes.data_as(PI), span, (C.c_ubyte * n)())
    assert chk(100, list(range(1, 66)), [0] * 65) == 0
    assert chk(600, list(range(1, 513)), [0] * 512) == 0
    assert chk(600, list(range(1, 514)), [0] * 513) == 2      # too many loop edges
    assert chk(600, list(range(1, 513)), [0] * 511 + [512]) == 5 and chk(600, [1, 2, 2] + list(range(4, 513)), [0] * 512) == 6
    assert chk(600, list(range(1, 512)) + [600], [0] * 512) == 4 and chk(600, list(range(1, 513)), [0] * 512, span=5) == 3


def test_sanitized_stand_alone_program():
    """The long plan and graph check under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _cxx(os.path.join(ROOT, "tests", "lc4_long_host_main.cpp"), os.path.join(BUILD, "lc4_long_host_main"),
               ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_entry_point_is_declared_exported_and_listed():
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    assert hasattr(lib, "gfbe_lc4_solve_long") and "gfbe_lc4_solve_long" in gf.backend.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "gfbe.h")).read()
    assert "gfbe_status gfbe_lc4_solve_long(gfbe_ctx *ctx, const gfbe_lc4_options *opt" in hdr
    assert "#define GFBE_LC4_LONG_MAX_LOOPS 512" in hdr and abi.LC4_LONG_MAX_LOOPS == 512
    assert "#define GFBE_LC4_MAX_LOOPS 64" in hdr and abi.LC4_MAX_LOOPS == 64      # the short call keeps its limit
    assert "constexpr int LC4_LONG_MAX_LOOPS = 512;" in open(HDR).read()


def test_c_abi_without_a_device():
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    lib.gfbe_create.restype = abi.c_i
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    lg = abi.LoopGraph(lib, "gfbe_", ctx)
    lib.gfbe_last_error.restype = C.c_char_p
    lib.gfbe_last_error.argtypes = [C.c_void_p]
    g = gf.synth.loop_graph(n=132, n_loop=65, seed=21)
    args = [g[k] for k in lc.ARG_KEYS]
    # a well-formed 65-loop call fails loudly: no device, no CPU fallback — and the short call still refuses it
    rc, out = lg.solve_long_rc(*args)
    assert rc == abi.NO_DEVICE and np.isnan(out["t"]).all() and np.isnan(out["yaw"]).all() and np.isnan(out["drift"]).all()
    assert b"gfbe_lc4_solve_long: no device (no CPU fallback)" in lib.gfbe_last_error(ctx)
    assert lg.solve_rc(*args)[0] == abi.BAD_INPUT
    small = gf.synth.loop_graph(n=100, n_loop=4, seed=3)
    assert lg.solve_long_rc(*[small[k] for k in lc.ARG_KEYS])[0] == abi.NO_DEVICE

    def bad(**kw):
        a = dict(zip(lc.ARG_KEYS, args))
        opt = kw.pop("opt", None)
        a.update(kw)
        rc, out = lg.solve_long_rc(*[a[k] for k in lc.ARG_KEYS], opt=opt)
        assert rc == abi.BAD_INPUT, kw
        assert np.isnan(out["t"]).all() and np.isnan(out["yaw"]).all() and np.isnan(out["drift"]).all() and out["summary"]["iterations"] == 0      # nothing written
    many = gf.synth.loop_graph(n=1100, n_loop=513, seed=3)
    assert len(many["loop_i"]) == 513
    rc, out = lg.solve_long_rc(*[many[k] for k in lc.ARG_KEYS])                                      # n_loop > 512
    assert rc == abi.BAD_INPUT and np.isnan(out["t"]).all() and np.isnan(out["yaw"]).all() and np.isnan(out["drift"]).all() and out["summary"]["iterations"] == 0
    assert b"GFBE_LC4_LONG_MAX_LOOPS" in lib.gfbe_last_error(ctx)
    li, lcc = g["loop_i"].copy(), g["loop_c"].copy()
    bad(loop_i=np.array([li[1], *li[1:]], np.int32), loop_c=np.array([0, *lcc[1:]], np.int32))       # two loops on one pose
    bad(loop_c=np.array([li[0], *lcc[1:]], np.int32))                                                # loop_c >= loop_i
    bad(loop_c=np.array([li[0] + 1, *lcc[1:]], np.int32))
    bad(loop_i=np.array([132, *li[1:]], np.int32))                                                   # an index out of range
    bad(opt=lg.options(struct_size=C.sizeof(abi.Lc4Options) - 8))                                    # a struct of another size
    bad(opt=lg.options(struct_size=0))
    lib.gfbe_destroy(ctx)


# ---- the cases
@pytest.fixture(scope="module")
def both():
    return {name: (ll.reference(name, "f64"), ll.reference(name, "ld")) for name in LIVE}


def test_live_cases_decide_alike_with_margin(both):
    for name, (a, b) in both.items():
        assert lc.decisions(a) == lc.decisions(b), name
        mr = min(lc.margin_ratio(a), lc.margin_ratio(b))
        print(name, lc.decisions(b), "smallest margin / (u A): %.3g" % mr)
        assert mr >= 1e3, name


def test_bounds_of_lc4_cases_cover_four_times_the_cpu_ratio(both):
    for name, (a, b) in both.items():
        rr = lc.solve_ratios(a, b)
        print(name, "r_cpu", rr)
        assert 4 * rr["pose"] <= lc.K["pose"] and 4 * rr["cost"] <= lc.K["cost"], name


def test_cases_cover_the_paths(both):
    shapes = {name: m.plan(len(c["g"]["t"]), len(c["g"]["loop_i"])) for name, c in ll.all_cases().items()}
    assert all(len(c["g"]["loop_i"]) > m.MAX_LOOPS for c in ll.all_cases().values())
    assert shapes["n132_65_loops"]["cap_ld"] == 17 * 16 and shapes["n200_80_loops"]["cap_ld"] == 20 * 16
    assert shapes["n260_129_loops"]["cap"] == 516 and shapes["n260_129_loops"]["cap_ld"] == 528      # a ragged last tile
    assert (shapes[ll.CAP]["cap_ld"], shapes[ll.CAP]["rows"], shapes[ll.CAP]["ld"], shapes[ll.CAP]["M"]) == (2048, 2800, 2064, 175)
    assert both["n200_80_loops"][1]["iterations"] == 5 and 0 in both["n200_80_loops"][1]["accepted"] and 1 in both["n200_80_loops"][1]["accepted"]
    g = ll.cases()["n300_two_sequences_70_loops"]["g"]
    assert set(g["sequence"]) == {0, 1} and g["fixed"][g["sequence"] == 0].all() and (g["sequence"][g["loop_c"]] == 0).sum() >= 35
    on = both["n300_two_sequences_70_loops"][1]["graph"]["loop_on"]
    assert len(on) == 70 and (~on).sum() == 1      # one loop edge between two constant poses, dropped
    y = ll.cases()["n140_yaw_wrap_66_loops"]["g"]["ypr"][:, 0]
    assert (np.abs(y) > 170).any() and (y > 90).any() and (y < -90).any()
    u = ll.unusable_case()
    r = m.solve(*u["args"], opt=u["opt"])
    assert len(u["g"]["loop_i"]) == 65 and (r["iterations"], r["termination"], r["status"], r["accepted"]) == (5, 4, 2, [0] * 5)


def test_golden_belongs_to_todays_inputs_and_keeps_the_rules():
    gd = ll.golden()
    assert os.path.getsize(ll.GOLDEN) < 100 * 1024
    assert gd["digest"] == ll.input_digest(ll.cap_case())      # else: run tests/golden/make_golden_lc4_long.py again
    ref, f64 = gd["ref"], gd["f64"]
    assert lc.decisions(ref) == lc.decisions(f64) and ref["iterations"] == 2
    assert gd["margin"] >= 1e3
    assert 4 * gd["r_cpu"]["pose"] <= lc.K["pose"] and 4 * gd["r_cpu"]["cost"] <= lc.K["cost"]
    n = len(ll.cap_case()["g"]["t"])
    assert ref["t"].shape == (n, 3) and ref["yaw"].shape == (n,) and ref["t"].dtype == m.LD and len(ref["cost_history"]) == len(ref["A_cost"]) == len(ref["g_l1"]) == 3
    assert ref["A_pose"] > 0 and all(a > 0 for a in ref["A_cost"])
