"""The step half of a joint iteration over the line blocks (gfbe_line_step / gfbe_ltab_step / gfbe_ltab_commit) without a GPU: the numpy
checker (tests/line_step_np.py) against the dense joint system it is derived from, the per-line device functions of csrc/gfbe_line.h
compiled for the host (tests/line_step_host_shim.cpp) against the checker, a closed trust-region loop against a dense joint
Gauss-Newton, the bounds K of the GPU test, and the C ABI of the entry points (exports, struct_size, the no-device contract).
tests/test_gpu_line_step.py repeats the comparison on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import line_reduce_np as lr
import line_step_np as ls

abi, synth_line = gf.abi, gf.synth_line
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "_build", "libline_step_host_shim.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PD = C.POINTER(C.c_double)
LD = ls.LD


def _p(a):
    return a.ctypes.data_as(PD)


def _small_window(seed=41):
    return synth_line.line_window(seed=seed, n_ok=12, n_short=2, n_late=1, n_untri=1, n_behind=0, n_long=0, n_outlier=0)


def _joint(lw, mu, seed=5):
    """The dense joint system of a small window in longdouble: A = [[U + P, W], [W^T, V]] (no mu), g = [bp + q; bl], D^2, and the
    step-side inputs derived from the REDUCED system."""
    if np.finfo(LD).nmant < 63:
        pytest.skip("numpy.longdouble has no extended precision on this host")
    red = lr.reduce(lw, lr.SOLVE, mu=mu, dtype=LD)
    x, V, _ = ls.line_blocks(lw, dtype=LD)
    n = red["n_eligible"]
    assert n >= 2 and red["n_failed"] == 0
    scale = float(np.median(np.diag(red["U"].astype(float))))
    P, q = (a.astype(LD) for a in ls.rest_of_window(seed, scale))
    y, v, rest, Dp2 = ls.caller_side(red["H"], red["g"], red["U"], red["bp"], P, q, mu, 3.0, LD)
    N = ls.D + 4 * n
    A, g, D2 = np.zeros((N, N), LD), np.zeros(N, LD), np.zeros(N, LD)
    A[:72, :72], g[:72], D2[:72] = red["U"] + P, red["bp"] + q, Dp2
    for k in range(n):
        s = slice(72 + 4 * k, 76 + 4 * k)
        A[:72, s], A[s, :72], A[s, s], g[s] = red["W"][k], red["W"][k].T, V[k], red["bl"][k]
        D2[s] = np.clip(np.diag(V[k]), LD(1e-6), LD(1e32))
    return dict(red=red, rec=ls.records_of(red, V), x=x, y=y, v=v, rest=rest, A=A, g=g, D2=D2, n=n)


@pytest.mark.parametrize("mu", [1e-3, 1.0])
def test_back_substitution_equals_the_dense_joint_solution(mu):
    """Item 1: with y_p the longdouble solution of the reduced system, [y_p; y_l] solves [[U + P + mu D_p^2, W], [W^T, V']]."""
    lw = _small_window()
    J = _joint(lw, mu)
    xj = ls.solve(J["A"] + LD(mu) * np.diag(J["D2"]), J["g"])
    st = ls.step(lw, J["rec"], J["y"], J["v"], J["rest"], 1.0, dtype=LD)
    got = np.concatenate([J["y"], st["y_l"].reshape(-1)])
    assert float(np.abs(got - xj).max()) <= 1e-12 * float(np.abs(xj).max())
    vj = J["g"] / J["D2"]
    assert float(np.abs(np.concatenate([J["v"], st["v_l"].reshape(-1)]) - vj).max()) <= 1e-16 * float(np.abs(vj).max())


@pytest.mark.parametrize("mu", [1e-3, 1.0])
def test_totals_and_model_change_equal_the_dense_joint_quantities(mu):
    """Items 2 and 3: the eight totals from the dense joint J^T J, g, D; model_change = -(g . step + 1/2 step^T J^T J step) on all three
    dogleg branches, each of which is taken."""
    lw = _small_window()
    J = _joint(lw, mu)
    A, g, D2 = J["A"], J["g"], J["D2"]
    xj = ls.solve(A + LD(mu) * np.diag(D2), g)
    vj = g / D2
    xm = ls.orth_plus(J["x"], -J["red"]["bl"])
    want = np.array([(g * g / D2).sum(), (D2 * xj * xj).sum(), g @ xj, vj @ A @ vj, vj @ A @ xj, xj @ A @ xj,
                     max(np.abs(g[:72]).max(), np.abs(J["x"] - xm).max()), LD(3.0) + (J["x"] ** 2).sum()])
    T = ls.step(lw, J["rec"], J["y"], J["v"], J["rest"], 1.0, dtype=LD)["total"]
    assert float((np.abs(T - want) / np.abs(want)).max()) <= 1e-11
    # a gradient for which all three branches exist (line_step_np.prepare designs one from FP64 inputs; the same rule, here in longdouble)
    red = {k: J["red"][k].astype(float) for k in ("H", "g", "U", "bp")}
    y, v, rest, radii, (P, q) = ls.prepare("default", lw, red, J["rec"], mu, 400.0, 1.0)
    g2 = g.copy()
    A2 = A.copy()
    A2[:72, :72] = J["red"]["U"] + P.astype(LD)
    g2[:72] = J["red"]["bp"] + q.astype(LD)
    D2b = D2.copy()
    D2b[:72] = np.clip(np.diag(A2[:72, :72]), LD(1e-6), LD(1e32))
    yl, vl, restl, _ = ls.caller_side(J["red"]["H"], J["red"]["g"], J["red"]["U"], J["red"]["bp"], P, q, mu, 3.0, LD)
    xj = ls.solve(A2 + LD(mu) * np.diag(D2b), g2)
    vj = g2 / D2b
    seen = set()
    for radius in radii:
        st = ls.step(lw, J["rec"], yl, vl, restl, radius, dtype=LD)
        assert st["margin"] > 1e-9
        seen.add(st["branch"])
        c1, c2 = st["coef"][0], st["coef"][1]
        s = c1 * vj + c2 * xj
        mc = -(g2 @ s + LD(0.5) * (s @ A2 @ s))
        assert abs(float((st["coef"][3] - mc) / mc)) <= 1e-10, st["branch"]
        assert abs(float(np.sqrt((D2b * s * s).sum()) / st["coef"][2]) - 1) <= 1e-10      # step_norm is |D step|
        assert st["invalid"] == 0 and st["coef"][3] > 0
    assert seen == {0, 1, 2}


def test_bounds_K_and_branches_of_the_gpu_cases():
    """The bounds of tests/test_gpu_line_step.py: the checker in FP64 against itself in longdouble stays within R_CPU on every case, mu
    and radius (so K = the power of two >= 4 R_CPU is what the module says); every case takes the branch its radius was made for, no
    case sits within 1e-9 relative of a branch boundary, none is an invalid step."""
    if np.finfo(LD).nmant < 63:
        pytest.skip("numpy.longdouble has no extended precision on this host")
    worst = {}
    for name in ls.case_names():
        lw, par = ls.build_case(name)
        for mu in ls.MUS:
            p = dict(par, mu=mu)
            red = lr.reduce(lw, lr.SOLVE, dtype=np.float64, **p)
            V = ls.line_blocks(lw, p["sqrt_info"], p["width"])[1]
            _, Vl, A_Vl = ls.line_blocks(lw, p["sqrt_info"], p["width"], LD)
            okl = (red["failed"] == 0) & np.isfinite(Vl.astype(float)).all((1, 2))
            nz = A_Vl[okl] > 0
            if nz.any():
                worst["V"] = max(worst.get("V", 0.0), float((np.abs(V.astype(LD) - Vl)[okl][nz] / (ls.UNIT * A_Vl[okl][nz])).max()))
            rec = ls.records_of(red, V)
            y, v, rest, radii, _ = ls.prepare(name, lw, red, rec, mu, p["sqrt_info"], p["width"])
            for want_branch, radius in enumerate(radii):
                a = ls.step(lw, rec, y, v, rest, radius, p["sqrt_info"], p["width"], np.float64)
                b = ls.step(lw, rec, y, v, rest, radius, p["sqrt_info"], p["width"], LD)
                assert a["branch"] == b["branch"] == want_branch and a["invalid"] == b["invalid"] == 0, (name, mu, radius)
                assert b["margin"] > 1e-9, (name, mu, radius)
                for k, (r, nz_) in ls.ratios(a, b).items():
                    assert nz_ == 0, (name, mu, k)
                    worst[k] = max(worst.get(k, 0.0), r)
    print("r_cpu", {k: float("%.3g" % v) for k, v in worst.items()})
    for k, r in worst.items():
        assert r <= ls.R_CPU[k], (k, r)
        assert ls.K[k] >= 4 * ls.R_CPU[k] and ls.K[k] < 8 * ls.R_CPU[k]


# ---- item 4: the per-line device functions, compiled for the host
@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not available: the per-line device functions cannot be built for the host")
    src = os.path.join(ROOT, "tests", "line_step_host_shim.cpp")
    csrc = os.path.join(ROOT, "ground-fusion2_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("gfbe_line.h", "gfbe_math.h", "gfbe_factors.h")]
    if not os.path.exists(SHIM) or any(os.path.getmtime(d) > os.path.getmtime(SHIM) for d in deps):
        os.makedirs(os.path.dirname(SHIM), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", SHIM, src], check=True)
    lib = C.CDLL(SHIM)
    lib.shim_step_candidate.restype = C.c_double
    return lib


def test_per_line_device_functions_match_checker(shim):
    if np.finfo(LD).nmant < 63:
        pytest.skip("numpy.longdouble has no extended precision on this host")
    name = "huber_active"
    lw, par = ls.build_case(name)
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])]).astype(int)
    pose, ex = np.ascontiguousarray(lw["pose"], float), np.ascontiguousarray(lw["ex_cam"], float)
    u = ls.UNIT
    for mu in ls.MUS:
        p = dict(par, mu=mu)
        red = lr.reduce(lw, lr.SOLVE, dtype=np.float64, **p)
        rec = ls.records_of(red, ls.line_blocks(lw, p["sqrt_info"], p["width"])[1])
        y, v, rest, radii, _ = ls.prepare(name, lw, red, rec, mu, p["sqrt_info"], p["width"])
        el = np.flatnonzero(lr.entering(lw, lr.SOLVE))
        for radius in radii:
            ref = ls.step(lw, rec, y, v, rest, radius, p["sqrt_info"], p["width"], LD)
            gram = np.zeros(8)
            yl, vl, xs = np.zeros((len(el), 4)), np.zeros((len(el), 4)), np.zeros((len(el), 4))
            for k, l in enumerate(el):
                sp = np.zeros(8)
                shim.shim_line_orth(_p(pose), _p(ex), _p(np.ascontiguousarray(lw["line_plucker"][l], float)), int(lw["start_frame"][l]), _p(xs[k]))
                shim.shim_step_shares(_p(np.ascontiguousarray(rec["W"][k])), _p(np.ascontiguousarray(rec["Vinv"][k])), _p(np.ascontiguousarray(rec["bl"][k])),
                                      _p(np.ascontiguousarray(rec["V"][k])), _p(y), _p(v), _p(xs[k]), _p(yl[k]), _p(vl[k]), _p(sp))
                gram += sp
                gram[6] = max(gram[6] - sp[6], sp[6])
            total = rest + gram
            total[6] = max(rest[6], gram[6])
            coef = np.zeros(4)
            branch = shim.shim_dogleg(_p(total), C.c_double(radius), _p(coef))
            assert branch == ref["branch"]
            got = dict(gram=gram, total=total, coef=coef, y_l=yl, v_l=vl)
            # candidate poses and lines
            pc, ec = np.zeros((11, 7)), np.zeros(7)
            for b in range(12):
                d6 = np.ascontiguousarray(coef[0] * v[6 * b:6 * b + 6] + coef[1] * y[6 * b:6 * b + 6])
                shim.shim_pose_plus(_p(np.ascontiguousarray(pose[b] if b < 11 else ex)), _p(d6), _p(pc[b] if b < 11 else ec))
            xc, plk, cost = np.zeros((len(el), 4)), np.zeros((len(el), 6)), 0.0
            for k, l in enumerate(el):
                m = int(lw["n_obs"][l])
                ob = np.ascontiguousarray(lw["obs"][off[l]:off[l] + m], float)
                cost += shim.shim_step_candidate(_p(pc), _p(ec), _p(xs[k]), _p(yl[k]), _p(vl[k]), C.c_double(coef[0]), C.c_double(coef[1]),
                                                 int(lw["start_frame"][l]), m, _p(ob), C.c_double(p["sqrt_info"]), C.c_double(p["width"]), _p(xc[k]), _p(plk[k]))
            got.update(orth_cand=xc, plucker_cand=plk, pose_cand=pc, ex_cand=ec, cost_cand=cost)
            for k, (r, nz) in ls.ratios(got, ref).items():
                assert nz == 0 and r <= ls.K[k], (k, r, ls.K[k], mu, radius)
    assert u > 0


# ---- item 5: a closed loop in numpy against a dense joint Gauss-Newton
def _perturbed(seed=3):
    lw = _small_window(43)
    rng = np.random.default_rng(seed)
    ref = np.concatenate([np.asarray(lw["pose"], float), np.asarray(lw["ex_cam"], float)[None]], 0)
    pose = np.array([ls.pose_plus(np.asarray(lw["pose"], float)[f], rng.normal(0, 2e-3, 6)) for f in range(11)])
    plk = np.asarray(lw["line_plucker"], float) + rng.normal(0, 2e-3, np.asarray(lw["line_plucker"]).shape)
    lw = dict(lw, pose=pose, line_plucker=plk)
    scale = float(np.median(np.diag(lr.reduce(lw, lr.SOLVE)["U"])))
    quad = ls.Quadratic(ls.rest_of_window(77, scale)[0], rng.normal(0, 1e-3, 72), ref)
    return lw, quad


def _dense_joint_gn(lw, quad, iterations=60):
    """Levenberg-Marquardt on the dense joint system [poses, extrinsic, lines] (no elimination), to convergence."""
    lw = dict(lw)
    mu, cost = 1e-6, None
    el = np.flatnonzero(lr.entering(lw, lr.SOLVE))
    for _ in range(iterations):
        red = lr.reduce(lw, lr.SOLVE, mu=0.0)
        x, V, _ = ls.line_blocks(lw)
        cP, P, qg = quad.at(np.asarray(lw["pose"], float), np.asarray(lw["ex_cam"], float))
        cost = float(red["cost"]) + cP
        n = len(el)
        N = 72 + 4 * n
        A, g = np.zeros((N, N)), np.zeros(N)
        A[:72, :72], g[:72] = red["U"] + P, red["bp"] + qg
        for k in range(n):
            s = slice(72 + 4 * k, 76 + 4 * k)
            A[:72, s], A[s, :72], A[s, s], g[s] = red["W"][k], red["W"][k].T, V[k], red["bl"][k]
        while mu < 1e12:
            d = -np.linalg.solve(A + mu * np.diag(np.clip(np.diag(A), 1e-6, 1e32)), g)
            blocks = ls.pose_plus(np.concatenate([np.asarray(lw["pose"], float), np.asarray(lw["ex_cam"], float)[None]], 0), d[:72].reshape(12, 6))
            xc = ls.orth_plus(x, d[72:].reshape(n, 4))
            Rc, tc = ls._cams(blocks[:11], blocks[11])
            sl = np.asarray(lw["start_frame"])[el].astype(int)
            plk = np.array(lw["line_plucker"], float)
            plk[el] = lr.plk_from_pose(lr.orth_to_plk(xc), Rc[sl], tc[sl])
            cand = dict(lw, pose=blocks[:11], ex_cam=blocks[11], line_plucker=plk)
            c = float(lr.reduce(cand, lr.SOLVE)["cost"]) + quad.at(blocks[:11], blocks[11])[0]
            if c < cost:
                lw, mu = cand, max(mu / 10, 1e-12)
                break
            mu *= 10
        else:
            break
        if cost - c <= 1e-15 * cost:
            cost = c
            break
    return cost


def test_closed_loop_reaches_the_dense_joint_minimum():
    lw, quad = _perturbed()
    res = ls.closed_loop(ls.NumpyOps(lw), quad, lw["pose"], lw["ex_cam"])
    costs = res["costs"]
    print("closed loop:", res["trace"], ["%.12g" % c for c in costs])
    assert res["trace"].count("a") >= 2
    assert all(b < a for a, b in zip(costs, costs[1:]))            # every accepted step lowers the total cost
    dense = _dense_joint_gn(lw, quad)
    print("dense joint Gauss-Newton: %.12g" % dense)
    assert abs(res["cost"] - dense) <= 1e-9 * dense


# ---- item 6: the C ABI without a device (fails before the entry points exist)
@pytest.fixture(scope="module")
def lib():
    gf.build_native()
    return C.CDLL(gf.lib_path())


def test_step_exports_present(lib):
    names = ("gfbe_line_step", "gfbe_ltab_keep_records", "gfbe_ltab_step", "gfbe_ltab_commit")
    hdr = open(os.path.join(ROOT, "include", "gfbe.h")).read()
    for name in names:
        assert name in gf.backend.EXPORTS
        assert hasattr(lib, name), name
        assert "gfbe_status %s(" % name in hdr
    assert C.sizeof(abi.LineStepped) == 8 + 12 * 8
    assert C.sizeof(abi.LineReducedV) == C.sizeof(abi.LineReduced) + 8


def test_public_structs_match_the_c_header(tmp_path):
    pairs = [("gfbe_line_reduced", abi.LineReducedV), ("gfbe_line_stepped", abi.LineStepped)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gfbe.h"', 'int main(void) {',
             '  printf("v0 %d\\n", (int)GFBE_LINE_REDUCED_SIZE_V0);']
    for cname, cls in pairs:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["v0"]) == C.sizeof(abi.LineReduced)
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, "%s.%s" % (cname, f)


def test_step_without_device_fails_loudly_and_touches_nothing(lib):
    ctx = C.c_void_p()
    lib.gfbe_create.restype = abi.c_i
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    try:
        lws = [synth_line.line_window(seed=11), synth_line.line_window(seed=12)]
        holders = [abi.LineWindowHolder(w) for w in lws]
        records = []
        for w in lws:
            red = lr.reduce(w, lr.SOLVE)
            records.append(ls.records_of(red, ls.line_blocks(w)[1]))
        rb, ne = abi.line_records_pack(records)
        red = abi.line_reduced_struct_v(rb)
        bufs = abi.line_stepped_buffers(2, int(ne.sum()), fill=7)
        before = {k: v.copy() for k, v in bufs.items()}
        out = abi.line_stepped_struct(bufs)
        y, v, rest, radius = np.ones((2, 72)), np.ones((2, 72)), np.ones((2, 8)), np.ones(2)

        def untouched():
            return all(np.array_equal(bufs[k], before[k]) for k in bufs)

        def call(mu=0.0, y=y, v=v, rest=rest, radius=radius, r=red, o=out):
            return abi.line_step_raw(lib, "gfbe_", ctx, holders, r, 400.0, 1.0, mu, y, v, rest, radius, o)
        assert call() == abi.NO_DEVICE and untouched()
        lib.gfbe_last_error.restype = C.c_char_p
        lib.gfbe_last_error.argtypes = [C.c_void_p]
        assert b"no CPU fallback" in lib.gfbe_last_error(ctx)
        bad = np.ones((2, 72))
        bad[1, 5] = np.nan
        bad8 = np.ones((2, 8))
        bad8[0, 3] = np.inf
        for kw in (dict(mu=-1e-3), dict(mu=float("nan")), dict(mu=float("inf")), dict(radius=np.array([1.0, -1.0])),
                   dict(radius=np.array([np.inf, 1.0])), dict(y=bad), dict(v=bad), dict(rest=bad8), dict(r=None), dict(o=None)):
            assert call(**kw) == abi.BAD_INPUT and untouched(), list(kw)
        out.struct_size = C.sizeof(abi.LineStepped) - 8
        assert call() == abi.BAD_INPUT and untouched()
        out.struct_size = C.sizeof(abi.LineStepped)
        red.struct_size = C.sizeof(abi.LineReduced)          # the size without V: a missing record array
        assert call() == abi.BAD_INPUT and untouched()
        red.struct_size = C.sizeof(abi.LineReducedV)
        for k in ("Vinv", "bl", "W", "V", "failed", "n_eligible"):
            keep = C.cast(getattr(red, k), C.c_void_p).value
            setattr(red, k, None)
            assert call() == abi.BAD_INPUT and untouched(), k
            setattr(red, k, C.cast(keep, dict(abi.LineReducedV._fields_)[k]))
        rb["n_eligible"][0] += 1                             # not the window's own count
        assert call() == abi.BAD_INPUT and untouched()
        rb["n_eligible"][0] -= 1
        holders[1].c.struct_size = C.sizeof(abi.LineWindow) - 8
        assert call() == abi.BAD_INPUT and untouched()
        holders[1].c.struct_size = C.sizeof(abi.LineWindow)
        assert call() == abi.NO_DEVICE and untouched()
        # gfbe_line_reduce admits both sizes of its structure
        rbuf = abi.line_reduced_buffers_v(2, sum(h.n for h in holders), fill=7)
        rs = abi.line_reduced_struct_v(rbuf)
        f = lib.gfbe_line_reduce
        f.restype = abi.c_i
        f.argtypes = [C.c_void_p, abi.c_i, C.c_void_p, abi.c_i, C.c_double, C.c_double, C.c_double, C.c_void_p]
        arr = (C.POINTER(abi.LineWindow) * 2)(*[C.pointer(h.c) for h in holders])
        assert f(ctx, 2, arr, 0, 400.0, 1.0, 0.0, C.byref(rs)) == abi.NO_DEVICE
        rs.struct_size = C.sizeof(abi.LineReduced)
        assert f(ctx, 2, arr, 0, 400.0, 1.0, 0.0, C.byref(rs)) == abi.NO_DEVICE
        rs.struct_size = C.sizeof(abi.LineReduced) + 4
        assert f(ctx, 2, arr, 0, 400.0, 1.0, 0.0, C.byref(rs)) == abi.BAD_INPUT
        assert all((a == 7).all() for a in rbuf.values())
        # the table-fed entry points (no table can exist without a device: the argument checks and the device check come first)
        g = lib.gfbe_ltab_step
        g.restype = abi.c_i
        g.argtypes = [C.c_void_p, C.c_void_p, PD, PD, C.c_double, C.c_double, PD, PD, PD, PD, C.c_void_p]
        p7, e7 = np.zeros((1, 11, 7)), np.zeros((1, 7))
        assert g(ctx, None, _p(p7), _p(e7), 400.0, 1.0, _p(y), _p(v), _p(rest), _p(radius), C.byref(out)) == abi.NO_DEVICE and untouched()
        out.struct_size = 16
        assert g(ctx, None, _p(p7), _p(e7), 400.0, 1.0, _p(y), _p(v), _p(rest), _p(radius), C.byref(out)) == abi.BAD_INPUT and untouched()
        out.struct_size = C.sizeof(abi.LineStepped)
        assert g(ctx, None, _p(p7), _p(e7), 400.0, 1.0, _p(y), _p(v), _p(rest), _p(radius), None) == abi.BAD_INPUT
        for name, args in (("gfbe_ltab_keep_records", (ctx, None, 1)), ("gfbe_ltab_commit", (ctx, None, None))):
            h = getattr(lib, name)
            h.restype = abi.c_i
            h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] if name.endswith("commit") else [C.c_void_p, C.c_void_p, abi.c_i]
            assert h(*args) == abi.NO_DEVICE, name
            assert h(None, *args[1:]) == abi.BAD_INPUT, name
    finally:
        lib.gfbe_destroy(ctx)
