"""CPU checks of the device-resident LiDAR scan (no GPU): the numpy model (tests/scan_np.py) against its independent restatements,
the host build of the per-point device functions (ground-fusion2_amd/csrc/gfbe_scan.h through tests/scan_host_shim.cpp) against
the model, the bound of the GPU test, a sanitized stand-alone program, and the C ABI without a device.

Measured here: r_cpu = the worst |FP64 model - longdouble model| / (u A) over scan_cases.undistort_cases() = 3.47 (states_512, a
point 51 segments in front of the first state; 1.58 .. 2.84 for the other cases), so K = 16 (the smallest power of two >= 4 r_cpu).
The host build of gfbe_scan.h against the longdouble model: the same 3.47 (it gives the FP64 model's bits on these cases). On the
MI355X the device's worst ratio over the same cases is 3.47 as well, case by case the CPU's figures (tests/test_gpu_scan.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import scan_cases as sc
import scan_np as sn
import vmap_np as vm

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SHIM = os.path.join(BUILD, "libscan_host_shim.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PD = C.POINTER(C.c_double)
SUB = sc.subsample_cases()
UND = sc.undistort_cases()


def _p(a):
    return a.ctypes.data_as(PD)


def _ld():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("numpy.longdouble is no wider than float64 here: the extended-precision reference is not available")


@pytest.mark.parametrize("name", list(SUB))
def test_subsample_model_against_the_dictionary(name):
    c = SUB[name]
    kept, skipped = sn.subsample(c["pts"], c["size"])
    kept2, skipped2 = sn.subsample_dict(c["pts"], c["size"])
    assert np.array_equal(kept, kept2) and skipped == skipped2
    assert (np.diff(kept) > 0).all()


def test_subsample_hand_cases():
    assert len(sn.subsample(SUB["empty"]["pts"], 0.2)[0]) == 0
    assert sn.subsample(SUB["one"]["pts"], 0.2)[0].tolist() == [0]
    assert sn.subsample(SUB["one_voxel_257"]["pts"], 0.2)[0].tolist() == [0]
    kept, _ = sn.subsample(SUB["thousand_voxels"]["pts"], 0.2)
    assert kept.tolist() == list(range(1000))
    assert sn.subsample(SUB["origin"]["pts"], 0.2)[0].tolist() == [0, 3, 4]      # (+-0.19 share the voxel at the origin)
    kept, skipped = sn.subsample(SUB["out_of_range"]["pts"], 0.2)
    assert skipped == 8 and kept[0] == 4 and 15 not in kept and 25 not in kept      # (the good point between the dropped ones is kept, its repeats are not)
    assert set(range(5, 15)) - set(kept.tolist()) == {i for i in range(5, 15) if vm.point_key(SUB["out_of_range"]["pts"][i], 0.2) == (0, 0, 0)}
    # the reversed cloud keeps the OTHER point of every voxel that holds more than one
    a, _ = sn.subsample(SUB["cube_70000"]["pts"], 0.05)
    b, _ = sn.subsample(SUB["cube_70000_reversed"]["pts"], 0.05)
    n = len(SUB["cube_70000"]["pts"])
    assert len(a) == len(b) < n
    lost = np.setdiff1d(np.arange(n), a)
    assert len(lost) > 0 and not np.array_equal(np.sort(n - 1 - b), a)
    # a voxel's last point in the forward cloud is its first in the reversed one
    last = {}
    for i, p in enumerate(SUB["cube_70000"]["pts"]):
        last[vm.point_key(p, 0.05)] = i
    assert np.array_equal(np.sort(n - 1 - b), np.array(sorted(last.values())))


@pytest.mark.parametrize("name", list(UND))
def test_segment_against_the_linear_scan(name):
    c = UND[name]
    extra = np.concatenate([c["t"], np.nextafter(c["t"], np.inf), np.nextafter(c["t"], -np.inf), [np.nan, -np.inf, np.inf]])
    for q in np.concatenate([c["ts"], extra]):
        assert sn.segment(c["t"], q) == sn.segment_brute(c["t"], q), q


def test_time_rule_hand_cases():
    t = np.array([1.0, 2.0, 2.0 + 5e-7, 3.0])
    P = sc.states(9, 4)[1]
    assert sn.segment(t, 3.2) == -1 and sn.segment(t, 3.9) == -1      # behind the last state, inside and outside 0.5 s
    assert np.array_equal(sn.pose_at(t, P, 3.2)[1], P[-1]) and np.array_equal(sn.pose_at(t, P, 3.9)[1], P[-1])
    assert sn.segment(t, 3.0) == 2                                      # equal to the last time: a segment, not 'behind'
    assert sn.segment(t, 1.5) == 0 and sn.segment(t, 2.0) == 0          # t_k < q && t_k+1 >= q: the >= side
    assert sn.segment(t, 1.0) == 0 and sn.segment(t, 0.5) == 0          # no such k: segment 0
    k, Ti = sn.pose_at(t, P, 0.5)                                       # ... with s = -0.5: extrapolation
    assert k == 0 and np.allclose(Ti[:3], P[0, :3] * 1.5 - P[1, :3] * 0.5, rtol=0, atol=1e-15)
    k, Ti = sn.pose_at(t, P, 2.0 + 5e-7)                                # a segment shorter than 1e-6 s: T_k
    assert k == 1 and np.array_equal(Ti, P[1])
    assert sn.segment(t[:1], 0.0) == -1 and np.array_equal(sn.pose_at(t[:1], P[:1], 0.0)[1], P[0])      # one state: T_end
    k, Ti = sn.pose_at(t, P, 2.0)                                       # s = 1 exactly: the next state
    assert k == 0 and np.allclose(Ti, P[1], rtol=0, atol=4e-16)
    # T_end^-1 T_end p = p up to rounding; a point at the last state's time does not move
    out, A = sn.undistort_point(P[-1], P[-1], np.array([1.0, -2.0, 3.0]))
    assert (np.abs(out - [1.0, -2.0, 3.0]) <= 4 * sn.U * A).all()


@pytest.fixture(scope="module")
def measured():
    _ld()
    worst = 0.0
    for name, c in UND.items():
        a, b = sn.undistort(c["pts"], c["ts"], c["t"], c["poses"], np.float64), sn.undistort(c["pts"], c["ts"], c["t"], c["poses"], sn.LD)
        assert np.array_equal(a["seg"], b["seg"])
        worst = max(worst, sc.ratio(a["pts"], b))
    return worst


def test_bound_covers_four_times_the_cpu_ratio(measured):
    print("r_cpu", measured)
    assert sc.K_POINT == 2.0 ** np.ceil(np.log2(4 * measured)), measured


def _hipcc(src, out, extra):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not available: gfbe_scan.h cannot be built for the host")
    deps = [src] + [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_scan.h", "gfbe_lio_pose.h", "gfbe_vmap.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_hipcc(os.path.join(ROOT, "tests", "scan_host_shim.cpp"), SHIM, ["-fPIC", "-shared"]))
    lib.shim_scan_segment.argtypes = [C.c_int, PD, C.c_double]
    lib.shim_scan_pose_at.argtypes = [C.c_int, PD, PD, C.c_double, PD]
    lib.shim_scan_key.argtypes = [PD, C.c_double, C.POINTER(C.c_int)]
    return lib


@pytest.mark.parametrize("name", list(UND))
def test_host_compiled_device_functions_agree_with_the_model(shim, name):
    _ld()
    c = UND[name]
    t, P = np.ascontiguousarray(c["t"]), np.ascontiguousarray(c["poses"])
    pts, ts = np.ascontiguousarray(c["pts"]), np.ascontiguousarray(c["ts"])
    for q in np.concatenate([ts, t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf), [np.nan]]):
        assert shim.shim_scan_segment(len(t), _p(t), float(q)) == sn.segment(t, q), q
    out, seg = np.zeros((len(pts), 3)), np.zeros(len(pts), np.int32)
    shim.shim_scan_undistort(len(t), _p(t), _p(P), len(pts), _p(pts), _p(ts), _p(out), seg.ctypes.data_as(C.POINTER(C.c_int)))
    ref = sn.undistort(pts, ts, t, P, sn.LD)
    assert np.array_equal(seg, ref["seg"])
    r = sc.ratio(out, ref)
    print(name, "host build worst ratio", r)
    assert r <= sc.K_POINT
    # the interpolated pose itself, within K u A: A = |p_k| |1 - s| + |p_k+1| |s| behind a translation, 2 (|1 - s| + |s|) behind an entry
    # of the quaternion (the two weighted unit quaternions, then the normalisation)
    for q in ts[:20]:
        Ti = np.zeros(7)
        k = shim.shim_scan_pose_at(len(t), _p(t), _p(P), float(q), _p(Ti))
        k2, want = sn.pose_at(t, P, q, sn.LD)
        assert k == k2
        if k < 0 or abs(t[k + 1] - t[k]) < 1e-6:
            assert np.array_equal(Ti, want.astype(np.float64))
            continue
        s = (q - t[k]) / (t[k + 1] - t[k])
        A = np.concatenate([np.abs(P[k, :3]) * abs(1 - s) + np.abs(P[k + 1, :3]) * abs(s), np.full(4, 2 * (abs(1 - s) + abs(s)))])
        assert (np.abs(Ti.astype(sn.LD) - want).astype(float) <= sc.K_POINT * sn.U * A).all(), q


def test_host_compiled_key_and_til(shim):
    for name, c in SUB.items():
        for p in c["pts"][:300]:
            key = (C.c_int * 3)()
            ok = shim.shim_scan_key(_p(np.ascontiguousarray(p)), c["size"], key)
            assert (tuple(key) if ok else None) == vm.point_key(p, c["size"])
    til = np.array([0.05, -0.02, 0.1, *sc._axis_angle([1, 2, 3], 0.4)])
    for p in UND["branches"]["pts"][:50]:
        out = np.zeros(3)
        shim.shim_scan_til(_p(til), _p(np.ascontiguousarray(p)), _p(out))
        assert np.array_equal(out, sn.til_point(til, p, np.float64))      # the same products and sums in the same order


def test_sanitized_stand_alone_program():
    """gfbe_scan.h under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _hipcc(os.path.join(ROOT, "tests", "scan_host_main.cpp"), os.path.join(BUILD, "scan_host_main"),
                 ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_c_abi_without_a_device():
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    new = [s for s in gf.backend.EXPORTS if s.startswith("gfbe_scan_")] + ["gfbe_vmap_register_scan", "gfbe_vmap_add_scan_handle"]
    assert len(new) == 10
    for s in new:
        assert hasattr(lib, s), s
        getattr(lib, s).restype = None if s == "gfbe_scan_destroy" else abi.c_i
    lib.gfbe_create.restype = abi.c_i
    lib.gfbe_scan_subsample.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
    lib.gfbe_scan_keypoints.argtypes = [C.c_void_p, C.c_void_p, abi.c_i, PD, PD, C.c_double, C.POINTER(abi.c_i)]
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    out = C.c_void_p(0xDEAD)
    assert lib.gfbe_scan_create(ctx, 1024, C.byref(out)) == abi.NO_DEVICE and not out.value
    for cap in (0, -1, (1 << 21) + 1):
        assert lib.gfbe_scan_create(ctx, cap, C.byref(out)) == abi.BAD_INPUT, cap
    assert lib.gfbe_scan_create(ctx, 1024, None) == abi.BAD_INPUT and lib.gfbe_scan_create(None, 1024, C.byref(out)) == abi.BAD_INPUT
    pose, n = np.array([0, 0, 0, 0, 0, 0, 1.0]), abi.c_i(0)
    calls = dict(
        upload=lambda c: lib.gfbe_scan_upload(c, None, 0, None, None, None, None),
        subsample=lambda c: lib.gfbe_scan_subsample(c, None, 0.2),
        undistort=lambda c: lib.gfbe_scan_undistort(c, None, 1, _p(pose), _p(pose)),
        keypoints=lambda c: lib.gfbe_scan_keypoints(c, None, 0, _p(pose), _p(pose), 0.2, C.byref(n)),
        size=lambda c: lib.gfbe_scan_size(c, None, None, None, None),
        download=lambda c: lib.gfbe_scan_download(c, None, 0, None, None, None, None),
        register_scan=lambda c: lib.gfbe_vmap_register_scan(c, None, None, 0, None, _p(pose), _p(pose), None, None, 0, _p(pose.copy()), _p(pose.copy()), None),
        add_scan_handle=lambda c: lib.gfbe_vmap_add_scan_handle(c, None, 0, None, _p(pose), _p(pose), 0))
    for name, f in calls.items():
        assert f(ctx) == abi.NO_DEVICE, name      # no device: whatever the other arguments are
        assert f(None) == abi.BAD_INPUT, name     # no context
    lib.gfbe_scan_destroy(ctx, None)
    with pytest.raises(RuntimeError):
        abi.Scan(lib, "gfbe_", ctx, 64)
    lib.gfbe_destroy(ctx)


def test_no_device_calls_name_themselves():
    """Every gfbe_scan_* call on a context without a device leaves its own name and the "no CPU fallback" text in gfbe_last_error."""
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    for s in gf.backend.EXPORTS:
        if s.startswith("gfbe_scan_") and s != "gfbe_scan_destroy":
            getattr(lib, s).restype = abi.c_i
    lib.gfbe_create.restype = abi.c_i
    lib.gfbe_last_error.restype = C.c_char_p
    lib.gfbe_scan_subsample.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
    lib.gfbe_scan_keypoints.argtypes = [C.c_void_p, C.c_void_p, abi.c_i, PD, PD, C.c_double, C.POINTER(abi.c_i)]
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    pose, n = np.array([0, 0, 0, 0, 0, 0, 1.0]), abi.c_i(0)
    calls = dict(
        upload=lambda: lib.gfbe_scan_upload(ctx, None, 0, None, None, None, None),
        subsample=lambda: lib.gfbe_scan_subsample(ctx, None, 0.2),
        undistort=lambda: lib.gfbe_scan_undistort(ctx, None, 1, _p(pose), _p(pose)),
        keypoints=lambda: lib.gfbe_scan_keypoints(ctx, None, 0, _p(pose), _p(pose), 0.2, C.byref(n)),
        size=lambda: lib.gfbe_scan_size(ctx, None, None, None, None),
        download=lambda: lib.gfbe_scan_download(ctx, None, 0, None, None, None, None))
    for name, f in calls.items():
        assert f() == abi.NO_DEVICE, name
        msg = lib.gfbe_last_error(ctx) or b""
        assert msg.startswith(b"gfbe_scan_" + name.encode() + b":") and b"no CPU fallback" in msg, (name, msg)
    lib.gfbe_destroy(ctx)
