"""The voxel map and the scan-to-map association (gfbe_vmap_*) without a GPU: the numpy model (tests/vmap_np.py) against brute force
and against the reference's rules, the __host__ __device__ pieces of csrc/gfbe_vmap.h compiled for the host
(tests/vmap_host_shim.cpp) against the model, the margins and bounds of the GPU test, and the C ABI without a device.

Measured here (FP64 model against the longdouble model over vmap_cases.cases() and the three-round room scene), worst
|X64 - Xld| / (u A_X): normals 1.17, offsets 0.92, weights 0.80, a2D 1.27, sv 0.37 -> K = 8, 4, 4, 8, 2 (vmap_cases.K)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import vmap_cases as vc
import vmap_np as vm

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "_build", "libvmap_host_shim.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PD = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(PD)


def _ld():
    if np.finfo(vm.LD).nmant < 63:
        pytest.skip("numpy.longdouble has no extended precision on this host")


def test_key_truncates_toward_zero():
    assert vm.point_key([0.19, -0.19, 0.0], 0.2) == (0, 0, 0)
    assert vm.point_key([-0.21, 0.41, -0.59], 0.2) == (-1, 2, -2)
    assert vm.point_key([6553.3, 0, 0], 0.2) == (32766, 0, 0)
    assert vm.point_key([6553.5, 0, 0], 0.2) is None and vm.point_key([0, -6553.5, 0], 0.2) is None and vm.point_key([0, 0, np.nan], 0.2) is None
    m = vm.Map()
    m.add_points([[0.1, 0.1, 0.1], [-0.1, -0.1, -0.1]])      # the voxel at the origin is twice as wide: both share it
    assert m.size()["n_voxels"] == 1 and m.size()["n_points"] == 2


def test_insert_order_full_voxel_and_min_distance():
    m = vm.Map(max_num_points_in_voxel=3, min_distance_points=0.05)
    m.add_points([[0.45, 0.45, 0.45], [0.46, 0.45, 0.45], [0.55, 0.45, 0.45], [0.45, 0.55, 0.45], [0.55, 0.55, 0.55]])
    d = m.download()
    assert d["counts"].tolist() == [3]      # the second point is too close to the first; the fifth finds the voxel full
    assert np.array_equal(d["points"], [[0.45, 0.45, 0.45], [0.55, 0.45, 0.45], [0.45, 0.55, 0.45]])
    m2 = vm.Map(max_num_points_in_voxel=3, min_distance_points=0.05)
    m2.add_points([[0.46, 0.45, 0.45], [0.45, 0.45, 0.45]])      # the other order keeps the other point
    assert np.array_equal(m2.download()["points"], [[0.46, 0.45, 0.45]])


def test_min_num_points_creates_no_voxel_and_gates_growth():
    m = vm.Map()
    m.add_points([[0.5, 0.5, 0.5]], min_num_points=1)
    assert m.size()["n_voxels"] == 0
    m.add_points([[0.5, 0.5, 0.5]])
    m.add_points([[0.58, 0.5, 0.5]], min_num_points=2)      # the voxel holds one point: below min_num_points
    assert m.size()["n_points"] == 1
    m.add_points([[0.58, 0.5, 0.5]], min_num_points=1)
    assert m.size()["n_points"] == 2


def test_erase_far_uses_the_first_point():
    m = vm.Map(max_distance=1.0, size_voxel_map=1.0, min_distance_points=0.01)
    m.add_points([[0.1, 0.1, 0.1], [0.95, 0.1, 0.1], [1.9, 0.5, 0.5], [1.05, 0.5, 0.5]])
    m.erase_far([-0.2, 0.1, 0.1])      # voxel 0: first point near (its second is far); voxel 1: first point far (its second is near)
    assert m.download()["keys"].tolist() == [[0, 0, 0]]


def test_capacity_rule_is_all_or_nothing_and_sticky():
    m = vm.Map(2)
    m.add_points([[0.1, 0.1, 0.1], [0.5, 0.1, 0.1]])
    m.add_points([[0.15, 0.1, 0.1], [0.9, 0.1, 0.1]])
    assert m.size() == dict(n_voxels=2, n_points=2, n_skipped=0, overflow=1)


def test_k_nearest_equals_brute_force_inside_the_guaranteed_radius():
    room = gf.synth_scan.Room(seed=4)
    m = vm.Map()
    m.add_points(room.surface(3000, 0.05))
    allp = m.all_points()
    checked = 0
    for v in (1, 2):
        for pw in room.surface(60, 0.3):
            best, _ = vm.search(m, pw, v, 1, 20, np.float64)
            if len(best) < 20:
                continue
            if best[-1][0] < vm.guaranteed_radius(pw, vm.point_key(pw, 0.2), v, 0.2):
                d = np.sort(np.sqrt(((allp - pw) ** 2).sum(1)))[:20]
                assert np.allclose([e[0] for e in best], d, rtol=1e-14, atol=0)
                checked += 1
    assert checked >= 20


def test_residual_cap_cuts_where_the_two_breaks_cut():
    case = dict(vc.cases()["residual_cap"])
    _, cut = vc.run_model(case)
    case["opt"] = dict(case["opt"], max_num_residuals=2000)
    _, full = vc.run_model(case)
    assert full["n_res"] > 3 and cut["n_res"] == 3
    assert cut["src"].tolist() == full["src"][:3].tolist() == [0, 0, 1]      # the second keypoint keeps one of its two rows
    assert np.array_equal(cut["offsets"], full["offsets"][:3])


@pytest.fixture(scope="module")
def measured():
    """Per quantity the worst FP64-against-longdouble ratio, the smallest decision margins and the smallest relative eigen-gap over
    every case of the GPU test."""
    _ld()
    worst, margin, gap = {}, {}, np.inf
    runs = []
    for name, case in vc.cases().items():
        m64, a = vc.run_model(case)
        _, b = vc.run_model(case, vm.LD)
        runs.append((name, a, b, m64.min_margin))
    opt, cap, steps = vc.room_rounds()
    ms = [vm.Map(cap, **opt), vm.Map(cap, **opt)]
    for r, (add, loc, sc, pb, pe) in enumerate(steps):
        for m in ms:
            m.add_points(add)
            m.erase_far(loc)
        a = vm.associate(ms[0], 1, sc["raw"], sc["alpha"], pb, pe)
        b = vm.associate(ms[1], 1, sc["raw"], sc["alpha"], pb, pe, dtype=vm.LD)
        runs.append(("room_round_%d" % r, a, b, ms[0].min_margin))
    for name, a, b, mm in runs:
        assert a["n_res"] == b["n_res"] and np.array_equal(a["src"], b["src"]) and a["neighbors"] == b["neighbors"], name
        r = vc.ratios(a, b)
        if b["n_res"] > 10:
            sa, sb = vm.localizability(a["normals"]), vm.localizability(b["normals"], b["relgap_res"], vm.LD)
            r["sv"] = float((np.abs(sa[0].astype(vm.LD) - sb[0]).astype(float) / (vm.U * sb[2])).max())
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        for k, v in dict(b["margin"], mindist=mm).items():
            margin[k] = min(margin.get(k, np.inf), v)
        g = b["relgap_res"]
        if len(g):
            gap = min(gap, float(g.min()))
    return worst, margin, gap


def test_no_decision_is_near_its_threshold(measured):
    _, margin, gap = measured
    print("margins", margin, "smallest relative eigen-gap", gap)
    for k, v in margin.items():
        assert v >= 1e-9, (k, v)
    assert gap >= 1e-3, gap


def test_bounds_cover_four_times_the_cpu_ratio(measured):
    worst, _, _ = measured
    print("r_cpu", worst)
    for k, v in worst.items():
        want = 2.0 ** np.ceil(np.log2(4 * v))
        assert vc.K[k] == want, (k, v, want)


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not available: the device functions of the voxel map cannot be built for the host")
    src = os.path.join(ROOT, "tests", "vmap_host_shim.cpp")
    deps = [src, os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_vmap.h")]
    if not os.path.exists(SHIM) or any(os.path.getmtime(d) > os.path.getmtime(SHIM) for d in deps):
        os.makedirs(os.path.dirname(SHIM), exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", SHIM, src], check=True)
    lib = C.CDLL(SHIM)
    lib.shim_vmap_plane.restype = C.c_double
    lib.shim_vmap_weight.restype = C.c_double
    lib.shim_vmap_weight.argtypes = [C.c_double] * 6 + [C.c_int]
    lib.shim_vmap_key.argtypes = [PD, C.c_double, C.POINTER(C.c_int)]
    return lib


def test_host_compiled_device_functions_agree_with_the_model(shim):
    _ld()
    rng = np.random.default_rng(2)
    for p in np.vstack([rng.uniform(-3, 3, (200, 3)), [[0.19, -0.19, 0.0], [6553.3, -6553.3, 0.0], [6553.5, 0, 0], [0, 0, -7000.0]]]):
        key = (C.c_int * 3)()
        ok = shim.shim_vmap_key(_p(np.ascontiguousarray(p)), 0.2, key)
        want = vm.point_key(p, 0.2)
        assert (tuple(key) if ok else None) == want
    o = vm.options()
    worst = {"normals": 0.0, "a2D": 0.0, "weights": 0.0}
    for trial in range(40):
        nb = np.ascontiguousarray(rng.uniform(-0.3, 0.3, (20, 3)) * [1.0, 1.0, 0.02] + rng.uniform(-2, 2, 3))
        cov, nrm = np.zeros(6), np.zeros(3)
        a2d = shim.shim_vmap_plane(_p(nb), 20, _p(cov), _p(nrm))
        _, cov64 = vm.moments(list(nb), np.float64)
        assert np.array_equal(cov, cov64)      # the same sums in the same order
        _, covl = vm.moments([q.astype(vm.LD) for q in nb], vm.LD)
        nl, al, lam = vm.normal_a2d(covl, vm.LD)
        if float(nl @ nrm) < 0:
            nl = -nl
        nC = float(np.sqrt(covl[0] ** 2 + covl[3] ** 2 + covl[5] ** 2 + 2 * (covl[1] ** 2 + covl[2] ** 2 + covl[4] ** 2)))
        relgap = float(lam[1] - lam[0]) / nC
        s1, s2, s3 = (float(np.sqrt(abs(x))) for x in (lam[2], lam[1], lam[0]))
        A_a2d = nC * (1 / (s2 * s1) + 1 / (s3 * s1)) / 2 + float(al) * nC / (2 * s1 * s1) + float(al)
        worst["normals"] = max(worst["normals"], float(np.abs(nrm.astype(vm.LD) - nl).max()) * relgap / vm.U)
        worst["a2D"] = max(worst["a2D"], abs(float(vm.LD(a2d) - al)) / (vm.U * A_a2d))
        d0 = float(rng.uniform(0.01, 0.2))
        w = shim.shim_vmap_weight(a2d, d0, o["weight_alpha"], o["weight_neighborhood"], o["power_planarity"], o["max_dist_to_plane_icp"], o["min_number_neighbors"])
        wl = vm.weight(vm.LD(a2d), vm.LD(d0), o, vm.LD)
        worst["weights"] = max(worst["weights"], abs(float(vm.LD(w) - wl)) / (vm.U * float(wl)))
    print("host-compiled against longdouble", worst)
    for k, v in worst.items():
        assert v <= vc.K[k], (k, v)


def host_map(lib, o):
    """A host-restatement map (tests/vmap_host_shim.cpp, hmap_*) with the options dict o."""
    iopt = np.array([o[k] for k in ("max_num_points_in_voxel", "voxel_neighborhood", "max_number_neighbors", "min_number_neighbors",
                                    "threshold_voxel_occupancy", "num_closest_neighbors", "max_num_residuals")], np.int32)
    dopt = np.array([o[k] for k in ("size_voxel_map", "min_distance_points", "max_distance", "max_dist_to_plane_icp", "power_planarity",
                                    "weight_alpha", "weight_neighborhood")], np.float64)
    lib.hmap_create.restype = C.c_void_p
    return C.c_void_p(lib.hmap_create(iopt.ctypes.data_as(C.POINTER(C.c_int)), _p(dopt)))


def host_associate(lib, h, o, ct, raw, alpha, pb, pe, frame_init=False):
    raw, al = np.ascontiguousarray(raw, np.float64).reshape(-1, 3), np.ascontiguousarray(alpha if alpha is not None else np.zeros(len(raw)), np.float64)
    pb, pe = np.ascontiguousarray(pb, np.float64), np.ascontiguousarray(pe, np.float64)
    R = o["max_num_residuals"]
    src, pts, nrm, off, alo, w = np.zeros(R, np.int32), np.zeros((R, 3)), np.zeros((R, 3)), np.zeros(R), np.zeros(R), np.zeros(R)
    n = lib.hmap_associate(h, int(ct), len(raw), _p(raw), _p(al), _p(pb), _p(pe), int(frame_init), src.ctypes.data_as(C.POINTER(C.c_int)),
                           _p(pts), _p(nrm), _p(off), _p(alo), _p(w))
    return dict(n_res=n, src=src[:n], pts=pts[:n], normals=nrm[:n], offsets=off[:n], alpha=alo[:n], weights=w[:n])


def test_host_restatement_agrees_with_the_model(shim):
    """The std::unordered_map restatement that tools/diag_vmap_bench.py times computes what the model computes."""
    _ld()
    for name in ("room_ct0", "scan_65", "two_closest", "residual_cap", "min_num_points", "out_of_range"):
        case = vc.cases()[name]
        m, _ = vc.run_model(case)
        _, ref = vc.run_model(case, vm.LD)
        h = host_map(shim, m.opt)
        for op in case["ops"]:
            pts = np.ascontiguousarray(op[1], np.float64).reshape(-1, 3)
            shim.hmap_add_points(h, len(pts), _p(pts), int(op[2]))
        sz = (C.c_int * 2)()
        shim.hmap_size(h, sz)
        assert (sz[0], sz[1]) == (m.size()["n_voxels"], m.size()["n_points"]), name
        got = host_associate(shim, h, m.opt, case["ct"], case["raw"], case["alpha"], case["pb"], case["pe"], case["frame_init"])
        assert got["n_res"] == ref["n_res"] and np.array_equal(got["src"], ref["src"]), name
        for k, v in vc.ratios(dict(got, a2D=ref["a2D"].astype(np.float64)), ref).items():
            assert v <= vc.K[k], (name, k, v)
        shim.hmap_destroy(h)


def test_abi_contract_without_a_device():
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    for s in gf.backend.EXPORTS:
        if s.startswith("gfbe_vmap_"):
            assert hasattr(lib, s), s
    lib.gfbe_create.restype = abi.c_i
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    opt = abi.vmap_default_options(lib)
    assert opt.struct_size == C.sizeof(abi.VmapOptions) == 88
    for k, v in vm.DEFAULTS.items():
        assert getattr(opt, k) == v, k
    lib.gfbe_vmap_create.restype = abi.c_i
    out = C.c_void_p(0xDEAD)
    assert lib.gfbe_vmap_create(ctx, 64, C.byref(opt), C.byref(out)) == abi.NO_DEVICE and not out.value
    assert lib.gfbe_vmap_create(ctx, 64, None, C.byref(out)) == abi.NO_DEVICE
    for field, bad in (("struct_size", 80), ("voxel_neighborhood", 3), ("voxel_neighborhood", -1), ("max_num_points_in_voxel", 33),
                       ("max_number_neighbors", 33), ("num_closest_neighbors", 0), ("size_voxel_map", 0.0), ("max_num_residuals", 0)):
        o2 = abi.vmap_default_options(lib)
        setattr(o2, field, bad)
        assert lib.gfbe_vmap_create(ctx, 64, C.byref(o2), C.byref(out)) == abi.BAD_INPUT, field
    assert lib.gfbe_vmap_create(ctx, 0, C.byref(opt), C.byref(out)) == abi.BAD_INPUT
    for name in ("add_points", "erase_far", "size", "download", "upload", "associate", "linearize", "localizability"):
        f = getattr(lib, "gfbe_vmap_" + name)
        f.restype = abi.c_i
    loc = np.zeros(3)
    assert lib.gfbe_vmap_erase_far(ctx, None, _p(loc)) == abi.NO_DEVICE
    assert lib.gfbe_vmap_add_points(ctx, None, 0, None, 0) == abi.NO_DEVICE
    assert lib.gfbe_vmap_size(ctx, None, None, None, None, None) == abi.NO_DEVICE
    assert lib.gfbe_vmap_localizability(ctx, None, None, None) == abi.NO_DEVICE
    with pytest.raises(RuntimeError):
        abi.VoxelMap(lib, "gfbe_", ctx, 64)
    lib.gfbe_destroy(ctx)
