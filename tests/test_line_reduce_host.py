"""Reduced normal equations of the line factors (gfbe_line_reduce / gfbe_ltab_reduce) without a GPU: the numpy checker
(tests/line_reduce_np.py) against central differences and against the joint system it eliminates, the per-line device functions of
csrc/gfbe_line.h compiled for the host (tests/line_reduce_host_shim.cpp) against the checker, the bound K of the GPU test, and the C ABI
of the two entry points (exports, the no-device and bad-input contract). tests/test_gpu_line_reduce.py repeats the comparison on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import line_np as ln
import line_reduce_np as lr

abi, synth_line = gf.abi, gf.synth_line
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "_build", "libline_reduce_host_shim.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PD = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(PD)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(b).max())


@pytest.fixture(scope="module")
def lw():
    return synth_line.line_window(seed=11)


def _obs_cases(lw, n=60):
    Rwc, twc = ln.cam_poses(lw)
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])])
    out = []
    for l in np.flatnonzero(ln.eligible(lw)):
        s = lw["start_frame"][l]
        x = ln.plk_to_orth(ln.plk_to_pose(lw["line_plucker"][l], Rwc[s], twc[s]))
        for k in range(lw["n_obs"][l]):
            out.append((lw["pose"][s + k].copy(), lw["ex_cam"].copy(), x.copy(), lw["obs"][off[l] + k].copy()))
    return out[:n]


def test_checker_factor_matches_line_np_and_central_differences(lw):
    """Item 1: the dtype-generic factor equals line_np.factor; its pose / extrinsic Jacobians and the Huber-corrected ones against central
    differences through pose_plus, where the loss is inactive and where it is active (not at the kink)."""
    h = 1e-6
    seen = set()
    for pose, ex, x, ob in _obs_cases(lw):
        r, Jp, Je, Jo = lr.factor(pose, ex, x, ob)
        rn, Jpn, Jen, Jon = ln.factor(pose[None], ex, x[None], ob[None])
        assert _rel(r, rn) <= 1e-12 and _rel(Jp, Jpn[:, :, :6]) <= 1e-11 and _rel(Je, Jen[:, :, :6]) <= 1e-11 and _rel(Jo, Jon) <= 1e-11
        # a sqrt_info that leaves the loss inactive, and one that makes it active; the kink |r|^2 = 1 is kept away from
        for si in (400.0, 400.0 * 0.2 / max(np.linalg.norm(r[0]), 1e-9), 400.0 * 5.0 / max(np.linalg.norm(r[0]), 1e-9)):
            rc, Jpc, Jec, _, _ = lr.eval_huber(pose, ex, x, ob, si, 1.0)
            s = float((lr.factor(pose, ex, x, ob, si, jac=False) ** 2).sum())
            if abs(s - 1.0) < 0.2:
                continue
            seen.add(s > 1.0)

            def corrected(p, e):
                rr = lr.factor(p, e, x, ob, si, jac=False)[0]
                return rr * lr.huber((rr * rr).sum(), 1.0)[1]
            for which, J in ((0, Jpc[0]), (1, Jec[0])):
                num = np.zeros((2, 6))
                for d in range(6):
                    e6 = np.zeros(6)
                    e6[d] = h
                    a = [pose, ex]
                    b = [pose, ex]
                    a[which], b[which] = ln.pose_plus(a[which], e6), ln.pose_plus(b[which], -e6)
                    num[:, d] = (corrected(*a) - corrected(*b)) / (2 * h)
                if s > 1.0:
                    # ceres' corrector with rho'' <= 0 scales J by sqrt(rho') and does NOT differentiate the scale: compare with the
                    # plain Jacobian times sqrt(rho'), and check that the true derivative differs (the loss really is active)
                    rr, Jp0, Je0, _ = lr.factor(pose, ex, x, ob, si)
                    sr = lr.huber((rr * rr).sum(), 1.0)[1]
                    assert _rel(J, (Jp0, Je0)[which][0] * sr) <= 1e-12
                    assert sr < 1.0
                else:
                    assert _rel(J, num) <= 1e-6, which
    assert seen == {True, False}
    # the loss itself: rho(s) = s inside, 2 a sqrt(s) - a^2 outside; continuous with a continuous derivative at the kink
    for a in (1.0, 0.5):
        c_in, s_in = lr.huber(np.float64(a * a * 0.99), a)
        c_out, s_out = lr.huber(np.float64(a * a * 1.01), a)
        assert s_in == 1.0 and abs(c_in - 0.5 * a * a * 0.99) < 1e-15 and abs(c_out - 0.5 * (2 * a * np.sqrt(a * a * 1.01) - a * a)) < 1e-15
        assert abs(s_out - (1 / 1.01) ** 0.25) < 1e-12
    assert lr.huber(np.float64(25.0), 0.0) == (12.5, 1.0)


def test_nested_elimination_equals_joint_system():
    """Item 2: [[U + I, W], [W^T, V']] [xp; xl] = [bp; bl] solved densely in longdouble equals (H + I) xp = g and the back-substitution
    xl = Vinv (bl - W^T xp) — the sign and layout conventions the join into the window solve relies on."""
    lw = synth_line.line_window(seed=41, n_ok=12, n_short=2, n_late=1, n_untri=1, n_behind=0, n_long=0, n_outlier=0)
    for mode in (lr.SOLVE, lr.MARG_OLD):
        ref = lr.reduce(lw, mode, mu=1e-3, dtype=lr.LD)
        n, D = ref["n_eligible"], lr.NP_DIM
        assert n >= 2 and ref["n_failed"] == 0
        A, b = np.zeros((D + 4 * n, D + 4 * n), lr.LD), np.zeros(D + 4 * n, lr.LD)
        A[:D, :D] = ref["U"] + np.eye(D)
        b[:D] = ref["bp"]
        for q in range(n):
            A[:D, D + 4 * q:D + 4 * q + 4] = ref["W"][q]
            A[D + 4 * q:D + 4 * q + 4, :D] = ref["W"][q].T
            A[D + 4 * q:D + 4 * q + 4, D + 4 * q:D + 4 * q + 4] = ref["Vp"][q]
            b[D + 4 * q:D + 4 * q + 4] = ref["bl"][q]
        x = _solve_ld(A, b)
        xp = _solve_ld(ref["H"] + np.eye(D), ref["g"])
        assert float(np.abs(x[:D] - xp).max()) <= 1e-12 * float(np.abs(xp).max())
        for q in range(n):
            xl = ref["Vinv"][q] @ (ref["bl"][q] - ref["W"][q].T @ xp)
            assert float(np.abs(x[D + 4 * q:D + 4 * q + 4] - xl).max()) <= 1e-10 * max(1.0, float(np.abs(xl).max()))
        assert np.array_equal(ref["H"], ref["H"].T) or float(np.abs(ref["H"] - ref["H"].T).max()) <= 1e-15 * float(np.abs(ref["H"]).max())


def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in longdouble (numpy.linalg has no extended precision)."""
    A, b = A.astype(lr.LD).copy(), b.astype(lr.LD).copy()
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:]
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, lr.LD)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def test_marginalise_old_mode(lw):
    """Item 3: rows and columns of pose 0 exactly zero; lines with start_frame != 0 contribute nothing."""
    ref = lr.reduce(lw, lr.MARG_OLD)
    assert ref["n_eligible"] == int((ln.eligible(lw) & (lw["start_frame"] == 0)).sum()) > 0
    for k in ("H", "U"):
        assert not ref[k][:6].any() and not ref[k][:, :6].any()
    assert not ref["g"][:6].any() and not ref["bp"][:6].any() and not ref["W"][:, :6].any()
    only0 = lr._take(lw, np.flatnonzero(lw["start_frame"] == 0))
    again = lr.reduce(only0, lr.MARG_OLD)
    for k in ("H", "g", "U", "bp", "W", "Vinv", "bl"):
        assert np.array_equal(ref[k], again[k]), k
    assert lr.reduce(lr._take(lw, np.flatnonzero(lw["start_frame"] != 0)), lr.MARG_OLD)["n_eligible"] == 0
    # and the solve mode does see the start frame's own observation
    assert lr.reduce(lw, lr.SOLVE)["U"][:6, :6].any()


def test_bound_K_and_cases_hold_no_line_that_fails_by_rounding():
    """The bound of tests/test_gpu_line_reduce.py: the checker in FP64 against itself in longdouble stays within R_CPU on every case and
    mode (so K = max(1024, 4 R_CPU) per array is what the module says), and no case contains a failed line in either precision."""
    if np.finfo(lr.LD).nmant < 63:
        pytest.skip("numpy.longdouble has no extended precision on this host")
    worst = {}
    for name in lr.case_names():
        lw, par = lr.build_case(name)
        for mode in (lr.SOLVE, lr.MARG_OLD):
            a, b = lr.reduce(lw, mode, dtype=np.float64, **par), lr.reduce(lw, mode, dtype=lr.LD, **par)
            assert a["n_failed"] == 0 and b["n_failed"] == 0, (name, mode)
            for k, (r, nz) in lr.ratios(a, b).items():
                assert nz == 0
                worst[k] = max(worst.get(k, 0.0), r)
    print("r_cpu", {k: round(v, 1) for k, v in worst.items()})
    for k, r in worst.items():
        assert r <= lr.R_CPU[k], (k, r)
        assert lr.K[k] >= 4 * lr.R_CPU[k] and lr.K[k] >= 1024.0
    bad, without, victim = lr.nan_case()
    for mode in (lr.SOLVE, lr.MARG_OLD):
        a, b = lr.reduce(bad, mode), lr.reduce(without, mode)
        assert a["n_failed"] == 1 and b["n_failed"] == 0 and a["n_eligible"] == b["n_eligible"] + 1
        assert np.array_equal(a["H"], b["H"]) and np.array_equal(a["g"], b["g"])


# ---- item 4: the per-line device functions, compiled for the host

def _cams(lw):
    pose, ex = np.asarray(lw["pose"], lr.LD), np.asarray(lw["ex_cam"], lr.LD)
    Rs, Rbc = lr._quat_R(pose[:, 3:]), lr._quat_R(ex[3:])
    return Rs @ Rbc, pose[:, :3] + lr._mv(Rs, np.broadcast_to(ex[:3], (11, 3)))


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not available: the per-line device functions cannot be built for the host")
    src = os.path.join(ROOT, "tests", "line_reduce_host_shim.cpp")
    deps = [src, os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_line.h"), os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_math.h")]
    if not os.path.exists(SHIM) or any(os.path.getmtime(d) > os.path.getmtime(SHIM) for d in deps):
        os.makedirs(os.path.dirname(SHIM), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", SHIM, src], check=True)
    lib = C.CDLL(SHIM)
    lib.shim_huber.restype = C.c_double
    return lib


def test_per_line_device_functions_match_checker(shim):
    for s in (0.0, 0.3, 0.99, 1.01, 17.0, 4e3):
        for a in (1.0, 0.5, 0.0, -1.0):
            sr = C.c_double()
            c = shim.shim_huber(C.c_double(s), C.c_double(a), C.byref(sr))
            cn, srn = lr.huber(np.float64(s), a)
            assert abs(c - cn) <= 1e-15 * max(1.0, cn) and abs(sr.value - srn) <= 1e-15
    lw, par = lr.build_case("huber_active")
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])]).astype(int)
    pose, ex = np.ascontiguousarray(lw["pose"]), np.ascontiguousarray(lw["ex_cam"])
    for mode, mu in ((lr.SOLVE, 0.0), (lr.SOLVE, 1e-4), (lr.MARG_OLD, 1.0)):
        ref = lr.reduce(lw, mode, mu=mu, dtype=lr.LD, **{k: v for k, v in par.items() if k != "mu"})
        el = np.flatnonzero(lr.entering(lw, mode))
        assert len(el) >= 5
        for q, l in enumerate(el):
            W, J, Vi, bl, cost, Y = np.zeros((72, 4)), np.zeros((11, 26)), np.zeros((4, 4)), np.zeros(4), C.c_double(), np.zeros((72, 4))
            m = int(lw["n_obs"][l])
            ob = np.ascontiguousarray(lw["obs"][off[l]:off[l] + m])
            ok = shim.shim_reduce_line(_p(pose), _p(ex), _p(np.ascontiguousarray(lw["line_plucker"][l])), int(lw["start_frame"][l]), int(mode == lr.MARG_OLD), m,
                                       _p(ob), C.c_double(par["sqrt_info"]), C.c_double(par["width"]), C.c_double(mu), _p(W), _p(J), _p(Vi), _p(bl),
                                       C.byref(cost), _p(Y))
            assert ok == 1
            u = lr.UNIT
            assert (np.abs(W - ref["W"][q]) <= lr.K["W"] * u * ref["A_W"][q]).all() and not W[ref["A_W"][q] == 0].any()
            assert (np.abs(bl - ref["bl"][q]) <= lr.K["bl"] * u * ref["A_bl"][q]).all()
            assert (np.abs(Vi - ref["Vinv"][q]) <= lr.K["Vinv"] * u * ref["A_Vinv"][q]).all() and np.array_equal(Vi, Vi.T)
            # Y is the product of the two arrays just checked: four-term dot products, within a few roundings of their absolute sums
            assert (np.abs(Y - W @ Vi) <= 8 * u * (np.abs(W) @ np.abs(Vi))).all()
            # the observation records [r | Jp | Je] and the cost against the checker's corrected factor (the factor's own accuracy, as
            # tests/test_line_host.py takes it: 1e-11 of the largest entry per block; the cost is a sum of squares of r)
            k0 = int(mode == lr.MARG_OLD)
            s0 = int(lw["start_frame"][l])
            fr = np.arange(s0 + k0, s0 + m)
            x = lr.plk_to_orth(lr.plk_to_pose(np.asarray(lw["line_plucker"][l], lr.LD), *[a[s0] for a in _cams(lw)]))
            rr, Jpr, Jer, _, cr = lr.eval_huber(pose[fr], ex, np.broadcast_to(x, (len(fr), 4)), ob[k0:], par["sqrt_info"], par["width"], lr.LD)
            assert not J[:k0].any() and not J[m:].any()
            assert _rel(J[k0:m, :2], rr.astype(float)) <= 1e-11 * max(1.0, par["sqrt_info"])
            assert _rel(J[k0:m, 2:14].reshape(-1, 2, 6), Jpr.astype(float)) <= 1e-11 and _rel(J[k0:m, 14:].reshape(-1, 2, 6), Jer.astype(float)) <= 1e-11
            assert abs(cost.value - float(cr.sum())) <= 1e-11 * max(1.0, float(cr.sum()))
    # the Cholesky verdicts: zero and NaN blocks fail, the clamp rescues a zero block
    Vi = np.zeros(16)
    assert shim.shim_chol4_inv(_p(np.zeros(16)), C.c_double(0.0), _p(Vi)) == 0
    assert shim.shim_chol4_inv(_p(np.full(16, np.nan)), C.c_double(1.0), _p(Vi)) == 0
    assert shim.shim_chol4_inv(_p(np.zeros(16)), C.c_double(1.0), _p(Vi)) == 1
    assert np.array_equal(Vi.reshape(4, 4), np.diag(np.full(4, 1.0 / 1e-6)))


# ---- item 5: the C ABI of the two entry points, without a device

@pytest.fixture(scope="module")
def lib():
    gf.build_native()
    return C.CDLL(gf.lib_path())


def test_reduce_exports_present(lib):
    for name in ("gfbe_line_reduce", "gfbe_ltab_reduce"):
        assert name in gf.backend.EXPORTS
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "gfbe.h")).read()
    assert "gfbe_status gfbe_line_reduce(" in hdr and "gfbe_status gfbe_ltab_reduce(" in hdr
    assert C.sizeof(abi.LineReduced) == 8 + 12 * 8


def test_reduce_without_device_fails_loudly_and_touches_nothing(lib, lw):
    ctx = C.c_void_p()
    lib.gfbe_create.restype = abi.c_i
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    try:
        holders = [abi.LineWindowHolder(lw), abi.LineWindowHolder(synth_line.line_window(seed=12))]
        bufs = abi.line_reduced_buffers(2, sum(h.n for h in holders), fill=7)
        before = {k: v.copy() for k, v in bufs.items()}
        red = abi.line_reduced_struct(bufs)

        def untouched():
            return all(np.array_equal(bufs[k], before[k]) for k in bufs)
        call = lambda mode=0, mu=0.0, r=red: abi.line_reduce_raw(lib, "gfbe_", ctx, holders, mode, 400.0, 1.0, mu, r)   # noqa: E731
        assert call() == abi.NO_DEVICE and untouched()
        lib.gfbe_last_error.restype = C.c_char_p
        lib.gfbe_last_error.argtypes = [C.c_void_p]
        assert b"no CPU fallback" in lib.gfbe_last_error(ctx)
        for kw in (dict(mode=2), dict(mode=-1), dict(mu=-1e-3), dict(mu=float("nan")), dict(mu=float("inf")), dict(r=None)):
            assert call(**kw) == abi.BAD_INPUT and untouched(), kw
        red.struct_size = C.sizeof(abi.LineReduced) - 8
        assert call() == abi.BAD_INPUT and untouched()
        red.struct_size = C.sizeof(abi.LineReduced)
        holders[1].c.struct_size = C.sizeof(abi.LineWindow) - 8
        assert call() == abi.BAD_INPUT and untouched()
        holders[1].c.struct_size = C.sizeof(abi.LineWindow)
        # the table-fed entry point (no table can exist without a device: the argument checks and the device check come first)
        f = lib.gfbe_ltab_reduce
        f.restype = abi.c_i
        f.argtypes = [C.c_void_p, C.c_void_p, abi.c_i, PD, PD, C.c_double, C.c_double, C.c_double, C.POINTER(abi.LineReduced)]
        p7, e7 = np.zeros((1, 11, 7)), np.zeros((1, 7))
        assert f(ctx, None, 0, _p(p7), _p(e7), 400.0, 1.0, 0.0, C.byref(red)) == abi.NO_DEVICE and untouched()
        assert f(ctx, None, 3, _p(p7), _p(e7), 400.0, 1.0, 0.0, C.byref(red)) == abi.BAD_INPUT
        assert f(ctx, None, 0, _p(p7), _p(e7), 400.0, 1.0, -1.0, C.byref(red)) == abi.BAD_INPUT
        red.struct_size = 16
        assert f(ctx, None, 0, _p(p7), _p(e7), 400.0, 1.0, 0.0, C.byref(red)) == abi.BAD_INPUT and untouched()
    finally:
        lib.gfbe_destroy(ctx)
