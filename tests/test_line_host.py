"""The line arithmetic of the product (csrc/gfbe_line.h, __host__ __device__) compiled for the host by tests/line_host_shim.cpp and pinned
against the numpy restatement (tests/line_np.py) and central differences through the manifolds' Plus; the C ABI of the line entry
points (exports, the no-device and bad-input contract). Runs without a GPU; tests/test_gpu_line.py repeats the comparison on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import line_np as ln

abi, synth_line = gf.abi, gf.synth_line
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "_build", "libline_host_shim.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PD = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(PD)


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "tests", "line_host_shim.cpp")
    deps = [src, os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_line.h"), os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_math.h")]
    if not os.path.exists(SHIM) or any(os.path.getmtime(d) > os.path.getmtime(SHIM) for d in deps):
        os.makedirs(os.path.dirname(SHIM), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", SHIM, src], check=True)
    lib = C.CDLL(SHIM)
    lib.shim_cauchy.restype = C.c_double
    lib.shim_reprojection_error.restype = C.c_double
    return lib


@pytest.fixture(scope="module")
def lw():
    return synth_line.line_window(seed=11)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(b).max())


def _cases(lw):
    """(pose, ex, orth, obs) of every observation of the window's eligible lines (their initial world lines)."""
    Rwc, twc = ln.cam_poses(lw)
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])])
    out = []
    for l in np.flatnonzero(ln.eligible(lw)):
        s = lw["start_frame"][l]
        x = ln.plk_to_orth(ln.plk_to_pose(lw["line_plucker"][l], Rwc[s], twc[s]))
        for k in range(lw["n_obs"][l]):
            out.append((lw["pose"][s + k].copy(), lw["ex_cam"].copy(), x.copy(), lw["obs"][off[l] + k].copy()))
    return out


def test_conversions_and_plus_match_numpy(shim, lw):
    rng = np.random.default_rng(5)
    for plk in lw["line_plucker"]:
        o, p2, a, b = np.zeros(4), np.zeros(6), np.zeros(6), np.zeros(6)
        shim.shim_plk_to_orth(_p(plk), _p(o))
        assert _rel(o, ln.plk_to_orth(plk)) <= 1e-12
        shim.shim_orth_to_plk(_p(o), _p(p2))
        assert _rel(p2, ln.orth_to_plk(o)) <= 1e-12
        # the round trip keeps the line (normalised to |n|^2 + |v|^2 = 1)
        assert _rel(p2, plk / np.linalg.norm(plk)) <= 1e-12
        pose = lw["pose"][rng.integers(0, 11)]
        shim.shim_plk_to_pose(_p(plk), _p(pose), _p(a))
        shim.shim_plk_from_pose(_p(plk), _p(pose), _p(b))
        R, t = ln.quat_R(pose[3:]), pose[:3]
        assert _rel(a, ln.plk_to_pose(plk, R, t)) <= 1e-12
        assert _rel(b, ln.plk_from_pose(plk, R, t)) <= 1e-12
        d, xo = rng.normal(0, 0.1, 4), np.zeros(4)
        shim.shim_orth_plus(_p(o), _p(d), _p(xo))
        assert _rel(xo, ln.orth_plus(o, d)) <= 1e-12


def test_residual_and_jacobians_match_numpy_and_central_differences(shim, lw):
    h = 1e-6
    for pose, ex, x, ob in _cases(lw)[:120]:
        r, Jp, Je, Jo = np.zeros(2), np.zeros(14), np.zeros(14), np.zeros(8)
        shim.shim_line_factor(_p(pose), _p(ex), _p(x), _p(ob), C.c_double(400.0), _p(r), _p(Jp), _p(Je), _p(Jo))
        rn, Jpn, Jen, Jon = ln.factor(pose[None], ex, x[None], ob[None])
        assert _rel(r, rn[0]) <= 1e-12
        for got, want in ((Jp, Jpn), (Je, Jen), (Jo, Jon)):
            assert _rel(got.reshape(want[0].shape), want[0]) <= 1e-11
        assert Jp[6] == 0.0 and Jp[13] == 0.0 and Je[6] == 0.0 and Je[13] == 0.0
        # central differences through each block's own Plus
        for which, J, nd, plus in ((0, Jp.reshape(2, 7), 6, ln.pose_plus), (1, Je.reshape(2, 7), 6, ln.pose_plus),
                                   (2, Jo.reshape(2, 4), 4, ln.orth_plus)):
            num = np.zeros((2, nd))
            for d in range(nd):
                e = np.zeros(nd)
                e[d] = h
                args_a, args_b = [pose, ex, x], [pose, ex, x]
                base = args_a[which]
                args_a[which], args_b[which] = plus(base, e), plus(base, -e)
                ra = ln.factor(args_a[0][None], args_a[1], args_a[2][None], ob[None], jac=False)[0]
                rb = ln.factor(args_b[0][None], args_b[1], args_b[2][None], ob[None], jac=False)[0]
                num[:, d] = (ra - rb) / (2 * h)
            assert _rel(J[:, :nd], num) <= 1e-7, which


def test_cauchy_and_culling_match_numpy(shim, lw):
    for s in (0.0, 1e-4, 0.3, 1.0, 17.0, 4e3):
        sr = C.c_double()
        c = shim.shim_cauchy(C.c_double(s), C.c_double(1.0), C.byref(sr))
        cn, srn = ln.cauchy(s)
        assert abs(c - cn) <= 1e-12 * max(1.0, cn) and abs(sr.value - srn) <= 1e-15
    res = ln.refine(lw)
    Rwc, twc = ln.cam_poses(lw)
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])])
    seen = set()
    for l in np.flatnonzero(ln.eligible(lw)):
        plk, s = res["plucker"][l], lw["start_frame"][l]
        reason = res["reason"][l]
        seen.add(reason)
        assert bool(shim.shim_endpoints_bad(_p(plk), _p(lw["obs"][off[l]].copy()))) == (reason in ("behind", "far"))
        lw_w = ln.plk_to_pose(plk, Rwc[s], twc[s])
        for k in range(lw["n_obs"][l]):
            cam = np.concatenate([twc[s + k], synth_line._quat_xyzw(Rwc[s + k])])
            e = shim.shim_reprojection_error(_p(lw["obs"][off[l] + k].copy()), _p(cam), _p(lw_w))
            lc = ln.plk_from_pose(lw_w, ln.quat_R(cam[3:]), cam[:3])
            n = lc[:3] / np.linalg.norm(lc[:2])
            ob = lw["obs"][off[l] + k]
            want = (abs(n @ [ob[0], ob[1], 1.0]) + abs(n @ [ob[2], ob[3], 1.0])) / 2
            assert abs(e - want) <= 1e-12 * max(1e-3, want)
    assert {None, "behind", "far", "reprojection"} <= seen


# ---- the C ABI of the line entry points, without a device

@pytest.fixture(scope="module")
def lib():
    gf.build_native()
    return C.CDLL(gf.lib_path())


def test_line_exports_present(lib):
    for name in ("gfbe_line_eval", "gfbe_line_refine"):
        assert name in gf.backend.EXPORTS
        assert hasattr(lib, name), name
    assert C.sizeof(abi.LineWindow) == 4 + 4 + 5 * 8 + 77 * 8 + 7 * 8


def _host_ctx(lib):
    ctx = C.c_void_p()
    lib.gfbe_create.restype = abi.c_i
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    return ctx


def test_line_refine_without_device_fails_loudly_and_touches_nothing(lib, lw):
    ctx = _host_ctx(lib)
    try:
        holders = [abi.LineWindowHolder(lw), abi.LineWindowHolder(synth_line.line_window(seed=12))]
        n = sum(h.n for h in holders)
        plk, keep = np.full((n, 6), 7.25), np.full(n, 9, np.uint8)
        sums = (abi.Summary * 2)()
        sums[0].iterations = sums[1].iterations = 77
        rc, _, _, _ = abi.line_refine_raw(lib, "gfbe_", ctx, holders, plucker_out=plk, keep_out=keep, summary=sums)
        assert rc == abi.NO_DEVICE
        assert (plk == 7.25).all() and (keep == 9).all() and sums[0].iterations == 77 and sums[1].iterations == 77
        lib.gfbe_last_error.restype = C.c_char_p
        lib.gfbe_last_error.argtypes = [C.c_void_p]
        assert b"no CPU fallback" in lib.gfbe_last_error(ctx)
        # a structure of another size is refused before anything else
        holders[1].c.struct_size = C.sizeof(abi.LineWindow) - 8
        rc, _, _, _ = abi.line_refine_raw(lib, "gfbe_", ctx, holders, plucker_out=plk, keep_out=keep, summary=sums)
        assert rc == abi.BAD_INPUT and (plk == 7.25).all() and (keep == 9).all()
        # and observations that run past the window
        h = abi.LineWindowHolder(lw)
        h.sf[0] = 11 - h.no[0] + 1
        rc, _, _, _ = abi.line_refine_raw(lib, "gfbe_", ctx, [h], plucker_out=plk[:h.n], keep_out=keep[:h.n], summary=sums)
        assert rc == abi.BAD_INPUT and (plk == 7.25).all()
        # the stand-alone evaluation as well
        with pytest.raises(RuntimeError, match="status 5"):
            abi.line_eval(lib, "gfbe_", ctx, lw["pose"][:3], lw["ex_cam"], np.zeros((3, 4)), lw["obs"][:3])
    finally:
        lib.gfbe_destroy(ctx)
