"""The HIP-free half of the 6-DoF loop-closure pose graph (ground-fusion2_amd/csrc/gfbe_loopgraph6.h) without a GPU: compiled for the
host by a plain C++ compiler through tests/lc6_host_shim.cpp and held against the model (tests/lc6_np.py) on factors, sequence
measurements, Plus and plan; the same header under the address and undefined-behaviour sanitizers in a program of its own
(tests/lc6_host_main.cpp); the binding (include/gfbe_lc6.h against signatures.LC6, the layout of gfbe_lc6_options against a compiled C
program); and the C ABI's contract without a device: GFBE_NO_DEVICE, and every GFBE_BAD_INPUT case with nothing written."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import lc6_cases as lc
import lc6_np as m
import posegraph_np as pg

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
HDRS = [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_loopgraph6.h", "gfbe_loopgraph.h")]
PD, PI, PU8 = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
SENTINEL = -7.25


def _p(a):
    return a.ctypes.data_as(PD)


def _cxx(src, out, extra):
    if not CXX:
        pytest.fail("no C++ compiler: gfbe_loopgraph6.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + HDRS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def shim():
    return C.CDLL(_cxx(os.path.join(ROOT, "tests", "lc6_host_shim.cpp"), os.path.join(BUILD, "lc6_host_shim.so"), ["-fPIC", "-shared"]))


def test_the_header_has_no_hip_in_it():
    for h in HDRS:
        src = open(h).read()
        assert "hip/hip_runtime" not in src and "hipLaunch" not in src and "__global__" not in src


def _host_eval(shim, e):
    t, q, meas = (np.ascontiguousarray(e[k], np.float64) for k in ("t", "q", "meas"))
    ei, ej, kd = np.ascontiguousarray(e["edge_i"], np.int32), np.ascontiguousarray(e["edge_j"], np.int32), np.ascontiguousarray(e["kind"], np.uint8)
    E = len(ei)
    r, J, ce = np.zeros((E, 6)), np.zeros((E, 6, 12)), np.zeros(E)
    shim.shim_lc6_eval(C.c_int(E), _p(t), _p(q), ei.ctypes.data_as(PI), ej.ctypes.data_as(PI), kd.ctypes.data_as(PU8), _p(meas), C.c_double(e["opt"]["huber_delta"]),
                       C.c_double(e["opt"]["t_var"]), C.c_double(e["opt"]["q_var"]), _p(r), _p(J), _p(ce))
    return dict(r=r, J=J, cost=float(np.sum(ce)), cost_e=ce)


@pytest.mark.parametrize("name", ["n3_loop_into_constant", "n5_three_loops", "n9_span2", "n65_shapes", "n65_outlier", "n65_negated_q", "n257_two_sequences", "far_start"])
def test_host_build_agrees_with_the_model_on_factors(shim, name):
    pg.require_extended_precision()
    e = lc.eval_case(name)
    got = _host_eval(shim, e)
    ref = m.eval_edges(e["q"], e["t"], e["edge_i"], e["edge_j"], e["kind"], e["meas"], e["opt"], m.LD)
    rr = lc.eval_ratios(got, ref)
    print(name, "host build worst ratios", rr)
    assert rr["r"] <= lc.K["r"] and rr["J"] <= lc.K["J"] and rr["cost"] <= lc.K["eval_cost"]
    # the structure of the Jacobian: d r_t / d t_j = -d r_t / d t_i, d r_q / d dq_j = -d r_q / d dq_i, the other blocks zero
    J = got["J"]
    assert np.array_equal(J[:, :3, 3:6], -J[:, :3, 9:12]) and np.array_equal(J[:, 3:, 0:3], -J[:, 3:, 6:9])
    assert not J[:, :3, 6:9].any() and not J[:, 3:, 3:6].any() and not J[:, 3:, 9:12].any()


def test_host_build_forms_the_sequence_measurement_of_the_model(shim):
    pg.require_extended_precision()
    g = lc.cases()["n65_shapes"]["g"]
    t, q = np.ascontiguousarray(g["t"]), np.ascontiguousarray(g["q"])
    for a, b in ((0, 1), (3, 7), (10, 12), (59, 63)):
        out = np.zeros(7)
        shim.shim_lc6_sequence_meas(_p(t[a]), _p(q[a]), _p(t[b]), _p(q[b]), _p(out))
        want = m.sequence_meas(t[a], q[a], t[b], q[b], m.LD)
        A = np.abs(t[a]).sum() + np.abs(t[b]).sum()
        assert (np.abs(out[:3].astype(m.LD) - want[:3]).astype(float) <= 16 * m.U * 3 * A).all()      # (|R| entries <= 3 in absolute sums)
        assert (np.abs(out[3:].astype(m.LD) - want[3:]).astype(float) <= 4 * m.U * 2).all()           # (four products of unit quaternions' entries)
        assert np.array_equal(out, m.sequence_meas(t[a], q[a], t[b], q[b], np.float64))               # the FP64 model forms the same bits: one graph


def test_host_plus_is_the_models(shim):
    q = np.array([0.5, -0.5, 0.5, 0.5])
    for d in ([0.0, 0.0, 0.0], [0.1, -0.2, 0.3], [1e-9, 0.0, 0.0], [2.0, 1.0, -3.0]):
        out = np.zeros(4)
        shim.shim_lc6_plus(_p(q), _p(np.array(d)), _p(out))
        want, _ = m.plus(q[None], np.zeros((1, 3)), np.array([d + [0.0, 0.0, 0.0]]), np.float64)
        assert np.abs(out - want[0]).max() <= 4 * m.U
        if not any(d):
            assert np.array_equal(out, q)      # |d| = 0: the quaternion as it is


# n: (super-blocks, padding poses, sweeps)
PLAN = {1: (1, 3, 0), 2: (1, 2, 0), 4: (1, 0, 0), 5: (2, 3, 1), 63: (16, 1, 4), 64: (16, 0, 4), 65: (17, 3, 5)}


@pytest.mark.parametrize("n", sorted(PLAN))
def test_plan_padding_and_sweeps(shim, n):
    for L in (0, 1, 2, 3, 5, 127, 128):
        out = (C.c_longlong * 11)()
        assert shim.shim_lc6_plan(n, L, out) == 1
        M, rows, pad, sweeps, ncol, ld, ntile, cap, cap_ld, total, ok = list(out)
        assert (M, pad, sweeps) == PLAN[n] and rows == 32 * M
        assert ncol == 1 + 6 * L and ld == 16 * ntile and ld >= ncol > ld - 16
        assert cap == 6 * L and cap_ld % 16 == 0 and cap_ld >= max(cap, 16) and cap_ld < max(cap, 1) + 16 and cap_ld <= 768
        p = m.plan(n, L)
        assert (M, rows, pad, sweeps, ncol, ntile, ld, cap, cap_ld) == tuple(p[k] for k in ("M", "rows", "pad_poses", "sweeps", "ncol", "ntile", "ld", "cap", "cap_ld"))
        assert ok == 1 and total > 0      # every carved array lies inside the slab, on a 256-byte boundary, in order
    out = (C.c_longlong * 11)()
    assert shim.shim_lc6_plan(0, 0, out) == 0 and shim.shim_lc6_plan(n, 129, out) == 0 and shim.shim_lc6_plan(n, -1, out) == 0


def test_graph_check_names_the_rule(shim):
    def chk(n, li, lc_, span=4):
        a, b = np.array(li, np.int32), np.array(lc_, np.int32)
        return shim.shim_lc6_check_graph(n, len(a), a.ctypes.data_as(PI), b.ctypes.data_as(PI), span, (C.c_ubyte * n)())
    assert chk(8, [3, 5, 7], [0, 2, 6]) == 0 and chk(8, [], []) == 0
    assert chk(8, [8], [0]) == 4 and chk(8, [3], [-1]) == 4
    assert chk(8, [2], [2]) == 5 and chk(8, [2], [5]) == 5
    assert chk(8, [3, 3], [0, 1]) == 6
    assert chk(8, [3], [0], span=5) == 3 and chk(8, [3], [0], span=0) == 3
    assert chk(200, list(range(1, 130)), [0] * 129) == 2 and chk(200, list(range(1, 129)), [0] * 128) == 0
    for bad in (np.nan, np.inf, -np.inf):
        v = np.array([1.0, bad, 2.0])
        assert shim.shim_lc6_all_finite(_p(v), C.c_longlong(3)) == 0 and shim.shim_lc6_all_finite(_p(v), C.c_longlong(1)) == 1


def test_sanitized_stand_alone_program():
    """gfbe_loopgraph6.h under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _cxx(os.path.join(ROOT, "tests", "lc6_host_main.cpp"), os.path.join(BUILD, "lc6_host_main"),
               ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the binding
def _prototypes(header, prefix):
    """[(return spelling, name, [parameter spellings])] of every `ret name(args);` of the header, comments stripped (the approach of
    tests/test_abi.py::test_signature_table_matches_the_header)."""
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
    par = {"int32_t": C.c_int32, "gfbe_ctx*": C.c_void_p, "const gfbe_lc6_options*": P(abi.Lc6Options), "gfbe_lc6_options*": P(abi.Lc6Options),
           "const double*": P(C.c_double), "double*": P(C.c_double), "const int32_t*": P(C.c_int32), "const uint8_t*": P(C.c_uint8), "gfbe_summary*": P(abi.Summary)}
    ret = {"void": None, "gfbe_status": C.c_int32}
    table = gf.signatures.LC6
    protos = _prototypes("gfbe_lc6.h", "gfbe_lc6_")
    assert {p[1] for p in protos} == {"gfbe_lc6_" + k for k in table} == set(gf.backend.LC6_EXPORTS) and len(protos) == 3
    assert gf.signatures.TABLES["gfbe_lc6_"] is table
    for r, name, params in protos:
        res, args = table[name[len("gfbe_lc6_"):]]
        assert res is ret[r], name
        assert len(args) == len(params), name
        for k, (p, a) in enumerate(zip(params, args)):
            assert a is par[p], (name, k, p, a)
    hdr = open(os.path.join(ROOT, "include", "gfbe_lc6.h")).read()
    assert "#define GFBE_LC6_MAX_LOOPS 128" in hdr and abi.LC6_MAX_LOOPS == m.MAX_LOOPS == 128
    assert not set(gf.backend.LC6_EXPORTS) & set(gf.backend.EXPORTS)      # the surface of gfbe.h is as it was


def test_options_struct_matches_the_c_header(tmp_path):
    """sizeof and every field offset of abi.Lc6Options against what a C compiler makes of include/gfbe_lc6.h."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gfbe_lc6.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(gfbe_lc6_options));']
    for f, _ in abi.Lc6Options._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(gfbe_lc6_options, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.Lc6Options) == 40
    for f, _ in abi.Lc6Options._fields_:
        assert int(got[f]) == getattr(abi.Lc6Options, f).offset, f


def test_c_abi_without_a_device():
    gf.build_native()
    lib = abi.bind(C.CDLL(gf.lib_path()), "gfbe_")
    for name in gf.backend.LC6_EXPORTS:
        assert hasattr(lib, name), name
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    lg = abi.LoopGraph6(lib, ctx)
    o = lg.options()
    assert (o.struct_size, o.max_num_iterations, o.span, o.reserved, o.huber_delta, o.t_var, o.q_var) == (C.sizeof(abi.Lc6Options), 5, 4, 0, 0.1, 0.1, 0.01)
    g = gf.synth.loop_graph6(n=100, n_loop=4, seed=3)
    args = [g[k] for k in lc.ARG_KEYS]
    e = lc.eval_case("n5_three_loops")
    ev = (e["t"], e["q"], e["edge_i"], e["edge_j"], e["kind"], e["meas"])

    def untouched(out):
        return (out["t"] == SENTINEL).all() and (out["q"] == SENTINEL).all() and (out["drift"] == SENTINEL).all() and out["summary"]["iterations"] == 0
    # a well-formed call fails loudly: no device, no CPU fallback
    rc, out = lg.solve_rc(*args, fill=SENTINEL)
    assert rc == abi.NO_DEVICE and untouched(out)
    assert b"gfbe_lc6_solve" in lib.gfbe_last_error(ctx) and b"no CPU fallback" in lib.gfbe_last_error(ctx)
    assert lg.eval_rc(*ev)[0] == abi.NO_DEVICE and b"no CPU fallback" in lib.gfbe_last_error(ctx)

    def bad(**kw):
        a = dict(zip(lc.ARG_KEYS, args))
        opt = kw.pop("opt", None)
        a.update(kw)
        rc, out = lg.solve_rc(*[a[k] for k in lc.ARG_KEYS], opt=opt, fill=SENTINEL)
        assert rc == abi.BAD_INPUT, kw
        assert untouched(out), kw      # nothing written
    many = gf.synth.loop_graph6(n=300, n_loop=129, seed=3)
    rc, out = lg.solve_rc(*[many[k] for k in lc.ARG_KEYS], fill=SENTINEL)                            # n_loop > 128
    assert rc == abi.BAD_INPUT and untouched(out) and b"GFBE_LC6_MAX_LOOPS" in lib.gfbe_last_error(ctx)
    li, lcc = g["loop_i"].copy(), g["loop_c"].copy()
    bad(loop_i=np.array([100, *li[1:]], np.int32))                                                   # an index out of range
    bad(loop_c=np.array([-1, *lcc[1:]], np.int32))
    bad(loop_c=np.array([li[0], *lcc[1:]], np.int32))                                                # loop_c >= loop_i
    bad(loop_c=np.array([li[0] + 1, *lcc[1:]], np.int32))
    bad(loop_i=np.array([li[1], *li[1:]], np.int32), loop_c=np.array([0, *lcc[1:]], np.int32))       # two loops on one pose
    for key, at in (("t", (7, 1)), ("q", (50, 2)), ("loop_meas", (1, 0)), ("loop_meas", (3, 6))):    # a non-finite pose or measurement
        for v in (np.nan, np.inf):
            arr = np.array(g[key], np.float64).copy()
            arr[at] = v
            bad(**{key: arr})
    bad(opt=lg.options(struct_size=C.sizeof(abi.Lc6Options) - 8))                                    # a struct of another size
    bad(opt=lg.options(struct_size=C.sizeof(abi.Lc4Options)))
    bad(opt=lg.options(struct_size=0))
    bad(opt=lg.options(span=5))
    assert lg.eval_rc(*ev, opt=lg.options(struct_size=4))[0] == abi.BAD_INPUT
    ej = np.array(e["edge_j"]).copy()
    ej[0] = len(e["t"])
    assert lg.eval_rc(e["t"], e["q"], e["edge_i"], ej, e["kind"], e["meas"])[0] == abi.BAD_INPUT
    lib.gfbe_destroy(ctx)
