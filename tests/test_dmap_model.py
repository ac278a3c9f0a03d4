"""CPU checks of the dense RGB-D map (no GPU): the model (tests/dmap_np.py, a sequential dictionary walk) against its independent
restatement (a stable sort by (key, index)) and against hand cases, the FP64 model against the longdouble model on every case, the
host build of the per-point device functions (ground-fusion2_amd/csrc/gfbe_dmap.h through tests/dmap_host_shim.cpp) against the
model, the margin K of the cases, a sanitized stand-alone program, and the C ABI without a device.

Measured here: r_cpu = the worst |FP64 model - longdouble model| / (u A) over every world coordinate dmap_cases.cases() forms = 4.13
(rebuild_40; rebuild_3 3.67, gates_posed 2.57, wg_* 1.2 .. 2.4, negative 0.99, the identity cases 0), so K = 32 (the smallest power of
two >= 4 r_cpu). With that margin no point is within reach of a float32 rounding boundary or a gate, so FP64, longdouble and the device
take the same decision for every point and every comparison is exact: integers, order and float32 bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import dmap_cases as dc
import dmap_np as dn

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PD, PF = C.POINTER(C.c_double), C.POINTER(C.c_float)
CASES = dc.cases()
FILT = dc.filter_cases()
COLS = ("xyz", "rgb", "kf", "src")


def _ld():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("numpy.longdouble is no wider than float64 here: the extended-precision reference is not available")


def _same(a, b):
    assert a.size() == b.size()
    for k in COLS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for x, y in zip(a.pool(), b.pool()):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("name", list(CASES))
def test_walk_against_the_sort_and_longdouble(name):
    _ld()
    c = CASES[name]
    walk = dc.replay(c, dc.model_for(c))
    _same(walk, dc.replay(c, dc.model_for(c, restate=True)))
    _same(walk, dc.replay(c, dc.model_for(c, dtype=dn.LD)))
    assert (np.diff(walk.src) > 0).all() or len(walk.src) < 2      # (pool order within the cloud)


def test_hand_cases():
    m = dc.replay(CASES["n0"], dc.model_for(CASES["n0"]))
    assert m.size() == dict(n_keyframes=1, n_stored=0, n_cloud=0, n_voxels=0, n_skipped=0, n_gated=0, n_refused=0)
    m = dc.model_for(CASES["seven_in_one_voxel"])
    assert m.add_keyframe(*CASES["seven_in_one_voxel"]["steps"][0][1:]).tolist() == [0, 1, 2] and m.size()["n_voxels"] == 1
    c = CASES["base2_then3"]
    m = dc.model_for(c)
    assert m.add_keyframe(*c["steps"][0][1:]).tolist() == [0, 1, 2, 3, 4]
    assert m.add_keyframe(*c["steps"][1][1:]).tolist() == [0, 1, 4]      # voxel 7 held 2: ONE of its three candidates; voxel 1 held 1
    assert m.kf.tolist() == [0] * 5 + [1] * 3 and m.src.tolist() == list(range(8))
    one = dn.DenseMapModel(add_cap=1)      # "one per voxel" is another map
    one.add_keyframe(*c["steps"][0][1:])
    assert len(one.xyz) == 4
    c = CASES["gates"]
    m = dc.model_for(c)
    assert m.add_keyframe(*c["steps"][0][1:]).tolist() == [0, 2, 4, 5, 6] and m.n_gated == 2      # ON a gate is kept
    c = CASES["bad_points"]
    m = dc.model_for(c)
    assert m.add_keyframe(*c["steps"][0][1:]).tolist() == [1, 3, 5, 7, 11] and m.n_skipped + m.n_gated == 6      # [5 5 5] x 3 of 4, [6 6 6] x 2
    # reversed: the kept SET differs (the first three of a voxel in list order are other points)
    a = dc.replay(CASES["chunk_262145"], dc.model_for(CASES["chunk_262145"]))
    b = dc.replay(CASES["chunk_262145_reversed"], dc.model_for(CASES["chunk_262145_reversed"]))
    n = len(CASES["chunk_262145"]["steps"][0][2])
    assert len(a.last_kept) == len(b.last_kept) < n and not np.array_equal(np.sort(n - 1 - b.last_kept), a.last_kept)
    # a rebuild fills voxels to 5, the insert behind it (cap 3) keeps nothing in a voxel that holds 3 or more
    for name in ("rebuild_3", "rebuild_40"):
        c = CASES[name]
        m = dc.model_for(c)
        for s in c["steps"][:-1]:
            m.add_keyframe(*s[1:]) if s[0] == "add" else m.rebuild(s[1])
        before = dict(m.counts)
        assert max(before.values()) == 5 if name == "rebuild_40" else max(before.values()) >= 1
        pose, pts, rgb = c["steps"][-1][1:]
        kept = m.add_keyframe(pose, pts, rgb)
        ok, k = dn.keys(dn.to_float(dn.world(pose, c["opt"]["ex_cam"], pts)[0]), -10000.0, 0.01)
        packed = dn.pack(k)
        assert all(before.get(int(p), 0) < 3 for p in packed[kept])
        if name == "rebuild_40":
            full = [i for i in np.flatnonzero(ok) if before.get(int(packed[i]), 0) >= 3]
            assert len(full) > 0 and not set(full) & set(kept.tolist())
    # capacity: the prefix of the kept list, the rest counted; a full pool or keyframe table refuses a call whole
    c = CASES["wg_257"]
    full = dc.replay(c, dc.model_for(c))
    short = dn.DenseMapModel(len(full.xyz) - 1, 4, **c["opt"])
    assert np.array_equal(short.add_keyframe(*c["steps"][0][1:]), full.last_kept[:-1]) and short.n_refused == 1
    assert len(short.add_keyframe(*c["steps"][0][1:])) == 0 and short.n_refused == 1 + 257 and short.size()["n_keyframes"] == 2


def test_filter_hand_cases():
    c = FILT["hand"]
    keep = dn.filter_brute(c["pts"], 0.8, 10)
    assert keep[0] == 0 and not keep[1:11].any() and keep[11:22].all() and keep[22:82].all()      # isolated, 10, 11, the dense blob
    assert keep[82:94].sum() >= 6 and keep[94:105].all() and not keep[105:115].any() and keep[115:].all()
    c = FILT["exact_radius"]
    assert dn.filter_brute(c["pts"], 0.5, 1).tolist() == [1, 1, 0, 0, 1, 1]
    keep = dn.filter_brute(FILT["random_5000"]["pts"], 0.8, 10)
    assert 500 < keep.sum() < 4500


@pytest.fixture(scope="module")
def measured():
    _ld()
    return {name: dc.world_ratio(c) for name, c in CASES.items()}


def test_bound_covers_four_times_the_cpu_ratio(measured):
    print("r_cpu", measured)
    worst = max(measured.values())
    assert dc.K_WORLD == 2.0 ** np.ceil(np.log2(4 * worst)), worst


def _hipcc(src, out, extra):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not available: gfbe_dmap.h cannot be built for the host")
    deps = [src] + [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_dmap.h", "gfbe_math.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_hipcc(os.path.join(ROOT, "tests", "dmap_host_shim.cpp"), os.path.join(BUILD, "libdmap_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_dmap_rot.argtypes = [PD, PD]
    lib.shim_dmap_world.argtypes = [PD, PD, C.c_int, PF, PD, PF]
    lib.shim_dmap_gated.argtypes = [C.c_double] * 3
    lib.shim_dmap_key.argtypes = [PF, C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
    lib.shim_dmap_sqdist.argtypes, lib.shim_dmap_sqdist.restype = [PF, PF], C.c_double
    lib.shim_dmap_cell_side.argtypes, lib.shim_dmap_cell_side.restype = [C.c_double], C.c_double
    lib.shim_dmap_cell.argtypes = [PF, C.c_double, C.POINTER(C.c_int)]
    lib.shim_dmap_cells_fit.argtypes = [C.c_double] * 3
    return lib


def _pf(a):
    return a.ctypes.data_as(PF)


@pytest.mark.parametrize("name", list(CASES))
def test_host_compiled_device_functions_agree_with_the_model(shim, name):
    """World-point bits (FP64 and float), gate, key and its packing round trip of every point of every step, rebuild poses included."""
    c = CASES[name]
    o = dict(dn.DEFAULTS, **c["opt"])
    ex = np.ascontiguousarray(o["ex_cam"], np.float64)
    lists, todo = [], []
    for s in c["steps"]:
        if s[0] == "add":
            todo.append((s[1], s[2]))
            lists.append(s[2])
        else:
            todo += [(pose, pts) for pose, pts in zip(s[1], lists)]
    for pose, pts in todo[:12]:
        pose, pts = np.ascontiguousarray(pose, np.float64), np.ascontiguousarray(pts[:4000], np.float32)
        R = np.zeros(9)
        assert shim.shim_dmap_rot(pose[3:].ctypes.data_as(PD), R.ctypes.data_as(PD)) == 1      # (the bits of qrot, gfbe_math.h)
        assert np.array_equal(R.reshape(3, 3), dn.rot(pose[3:]))
        pw, pf = np.zeros((len(pts), 3)), np.zeros((len(pts), 3), np.float32)
        shim.shim_dmap_world(pose.ctypes.data_as(PD), ex.ctypes.data_as(PD), len(pts), _pf(pts), pw.ctypes.data_as(PD), _pf(pf))
        want = dn.world(pose, ex, pts)[0]
        assert np.array_equal(pw, want, equal_nan=True) and np.array_equal(pf, dn.to_float(want), equal_nan=True)
        ok, k = dn.keys(pf, o["origin"], o["resolution"])
        g = dn.gated(want[:, 2], o["z_min"], o["z_max"])
        for i in range(min(len(pts), 400)):
            key, packed = (C.c_int * 3)(), C.c_ulonglong()
            rc = shim.shim_dmap_key(_pf(pf[i]), o["origin"], o["resolution"], key, C.byref(packed))
            assert rc == (1 if ok[i] else 0), (i, rc)
            if ok[i]:
                assert tuple(key) == tuple(k[i]) == dn.unpack(packed.value) and packed.value == int(dn.pack(k[i])) < 2 ** 63
            assert shim.shim_dmap_gated(float(want[i, 2]), o["z_min"], o["z_max"]) == int(g[i]) or np.isnan(want[i, 2])


def test_host_compiled_distance_and_coarse_cell(shim):
    for radius in (0.8, 0.5, 0.05, 3.0):
        s = shim.shim_dmap_cell_side(radius)
        assert s * np.sqrt(3.0) <= radius <= 2 * s      # one cell lies within the radius; the radius reaches at most two cells
    assert shim.shim_dmap_cells_fit(-10000.0, 0.01, 0.8) == 1 and shim.shim_dmap_cells_fit(-10000.0, 0.01, 0.018) == 0
    assert shim.shim_dmap_cells_fit(-10000.0, 0.01, float("nan")) == 0 and shim.shim_dmap_cells_fit(-10000.0, 0.0, 0.8) == 0
    pts = np.ascontiguousarray(FILT["random_5000"]["pts"][:600])
    s = shim.shim_dmap_cell_side(0.8)
    cells = np.zeros((len(pts), 3), np.int32)
    for i in range(len(pts)):
        shim.shim_dmap_cell(_pf(pts[i]), s, cells[i].ctypes.data_as(C.POINTER(C.c_int)))
    assert np.array_equal(cells, np.floor(pts.astype(np.float64) / s).astype(np.int64) + (1 << 20))
    p = pts.astype(np.float64)
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    for i, j in [(0, 1), (5, 5), (17, 300), (599, 2)]:
        assert shim.shim_dmap_sqdist(_pf(pts[i]), _pf(pts[j])) == d2[i, j]
    same = (cells[:, None, :] == cells[None, :, :]).all(2)
    assert (d2[same] <= 0.8 * 0.8).all()                                          # containment: two points of one cell are within the radius
    assert (np.abs(cells[:, None, :] - cells[None, :, :]).max(2)[d2 <= 0.64] <= 2).all()      # and a neighbour is at most two cells away


def test_sanitized_stand_alone_program():
    """gfbe_dmap.h under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _hipcc(os.path.join(ROOT, "tests", "dmap_host_main.cpp"), os.path.join(BUILD, "dmap_host_main"),
                 ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_c_abi_without_a_device():
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    new = [s for s in gf.backend.EXPORTS if s.startswith("gfbe_dmap_")]
    assert len(new) == 9
    for s in new:
        assert hasattr(lib, s), s
        getattr(lib, s).restype = None if s in ("gfbe_dmap_destroy", "gfbe_dmap_default_options") else abi.c_i
    lib.gfbe_create.restype = abi.c_i
    lib.gfbe_last_error.restype = C.c_char_p
    o = abi.dmap_default_options(lib)
    assert o.struct_size == C.sizeof(abi.DmapOptions) == 112 and (o.add_cap, o.rebuild_cap, o.filter_min_neighbors) == (3, 5, 10)
    assert (o.resolution, o.origin, o.z_min, o.z_max, o.filter_radius) == (0.01, -10000.0, -0.5, 2.0, 0.8) and list(o.ex_cam) == [0, 0, 0, 0, 0, 0, 1]
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    out = C.c_void_p(0xDEAD)
    assert lib.gfbe_dmap_create(ctx, 1024, 16, C.byref(o), C.byref(out)) == abi.NO_DEVICE and not out.value
    assert lib.gfbe_dmap_create(ctx, 1024, 16, None, C.byref(out)) == abi.NO_DEVICE

    def bad(**kw):
        b = abi.dmap_default_options(lib)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    for b in (bad(add_cap=0), bad(add_cap=9), bad(rebuild_cap=0), bad(rebuild_cap=9), bad(struct_size=108), bad(struct_size=0), bad(resolution=0.0),
              bad(resolution=float("nan")), bad(origin=float("inf")), bad(filter_radius=0.0), bad(filter_radius=0.015), bad(filter_min_neighbors=-1), bad(z_min=float("nan"))):
        out = C.c_void_p(0xDEAD)
        assert lib.gfbe_dmap_create(ctx, 1024, 16, C.byref(b), C.byref(out)) == abi.BAD_INPUT and not out.value
        assert lib.gfbe_last_error(ctx)
    for pc, kc in ((0, 16), (-1, 16), ((1 << 26) + 1, 16), (1024, 0)):
        assert lib.gfbe_dmap_create(ctx, pc, kc, C.byref(o), C.byref(out)) == abi.BAD_INPUT, (pc, kc)
    assert lib.gfbe_dmap_create(ctx, 1024, 16, C.byref(o), None) == abi.BAD_INPUT and lib.gfbe_dmap_create(None, 1024, 16, C.byref(o), C.byref(out)) == abi.BAD_INPUT
    pose, n = np.array([0, 0, 0, 0, 0, 0, 1.0]), abi.c_i(-7)
    counts = (abi.c_i * 8)(*[-7] * 8)
    calls = dict(
        add_keyframe=lambda c: lib.gfbe_dmap_add_keyframe(c, None, pose.ctypes.data_as(PD), 0, None, None),
        rebuild=lambda c: lib.gfbe_dmap_rebuild(c, None, 0, None),
        filter=lambda c: lib.gfbe_dmap_filter(c, None, None, C.byref(n), None, None),
        size=lambda c: lib.gfbe_dmap_size(c, None, counts),
        download_cloud=lambda c: lib.gfbe_dmap_download_cloud(c, None, None, None, None, None),
        download_keyframe=lambda c: lib.gfbe_dmap_download_keyframe(c, None, 0, C.byref(n), None, None))
    for name, f in calls.items():
        assert f(ctx) == abi.NO_DEVICE, name      # no device: whatever the other arguments are
        assert f(None) == abi.BAD_INPUT, name     # no context
    assert n.value == -7 and list(counts) == [-7] * 8      # nothing written
    lib.gfbe_dmap_destroy(ctx, None)
    with pytest.raises(RuntimeError):
        abi.DenseMap(lib, "gfbe_", ctx, 64, 4)
    lib.gfbe_destroy(ctx)


def test_no_device_calls_name_themselves():
    """Every gfbe_dmap_* call on a context without a device leaves its own name and the "no CPU fallback" text in gfbe_last_error."""
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    for s in gf.backend.EXPORTS:
        if s.startswith("gfbe_dmap_") and s not in ("gfbe_dmap_destroy", "gfbe_dmap_default_options"):
            getattr(lib, s).restype = abi.c_i
    lib.gfbe_create.restype = abi.c_i
    lib.gfbe_last_error.restype = C.c_char_p
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    pose, n = np.array([0, 0, 0, 0, 0, 0, 1.0]), abi.c_i(-7)
    counts = (abi.c_i * 8)(*[-7] * 8)
    calls = dict(
        add_keyframe=lambda: lib.gfbe_dmap_add_keyframe(ctx, None, pose.ctypes.data_as(PD), 0, None, None),
        rebuild=lambda: lib.gfbe_dmap_rebuild(ctx, None, 0, None),
        filter=lambda: lib.gfbe_dmap_filter(ctx, None, None, C.byref(n), None, None),
        size=lambda: lib.gfbe_dmap_size(ctx, None, counts),
        download_cloud=lambda: lib.gfbe_dmap_download_cloud(ctx, None, None, None, None, None),
        download_keyframe=lambda: lib.gfbe_dmap_download_keyframe(ctx, None, 0, C.byref(n), None, None))
    for name, f in calls.items():
        assert f() == abi.NO_DEVICE, name
        msg = lib.gfbe_last_error(ctx) or b""
        assert msg.startswith(b"gfbe_dmap_" + name.encode() + b":") and b"no CPU fallback" in msg, (name, msg)
    lib.gfbe_destroy(ctx)
