"""The frame observations without a GPU: the model (tests/obs_np.py) against its second statements of O2, O3, O4 and O8 (a scalar walk
on Python floats), bit for bit, on every camera of tests/golden/obs_cameras.json and the synthetic ones; the host build of
ground-fusion2_amd/csrc/gfbe_obs.h (tests/obs_host_shim.cpp) against the model on every case, bit for bit, with the id sort and the
duplicate flag at the list lengths that matter; the same header under the address and undefined-behaviour sanitizers in a program of
its own (tests/obs_host_main.cpp); a property test of the model alone (spaceToPlane(lift(p)) returns to p); the rounding rule of O5;
the binding (include/gfbe_obs.h against signatures.OBS, the layout of gfbe_obs_options against a compiled C program, the other
surfaces unchanged); and the C ABI's refusals without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import obs_cases as oc
import obs_np as m

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
HDRS = [os.path.join(ROOT, "ground-fusion2_amd", "csrc", h) for h in ("gfbe_obs.h", "gfbe_klt.h")]
PF, PI, PD, PU16 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint16)
F, D = np.float32, np.float64
CAMERAS = oc.all_cameras()
CAM_NAMES = sorted(CAMERAS)


def _cxx(src, out, extra):
    if not CXX:
        pytest.fail("no C++ compiler: gfbe_obs.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + HDRS):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_cxx(os.path.join(ROOT, "tests", "obs_host_shim.cpp"), os.path.join(BUILD, "obs_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_obs_distortion.argtypes = [PD, C.c_double, C.c_double, PD, PD]
    lib.shim_obs_lift.argtypes = [PD, C.c_int, PF, PF]
    lib.shim_obs_camera_ok.argtypes = [PD]
    lib.shim_obs_velocity.argtypes = [C.c_float, C.c_float, C.c_double]
    lib.shim_obs_velocity.restype = C.c_float
    lib.shim_obs_depth_index.argtypes = [C.c_float, C.c_float, C.c_int, C.c_int, PI, PI]
    lib.shim_obs_sort.argtypes = [C.c_int, PI, PI]
    lib.shim_obs_observe.argtypes = [PD, C.c_int, PF, PI, C.c_int, PI, PF, C.c_double, PU16, C.c_int, C.c_int, PI, PD, PF, PI]
    lib.shim_obs_predict.argtypes = [PD, C.c_int, PF, PI, C.c_int, PI, PI, PI, PD, PD, C.c_int, PD, PD, PD, PF]
    return lib


def _b32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _b64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _pd(a):
    return a.ctypes.data_as(PD)


def _grid(step, name=None):
    """Pixels of the camera's image (640 x 480; 64 x 48 for the two small synthetic ones), the last row and column and fractional pixels among them."""
    k = 10.0 if name in ("strong", "no_distortion") else 1.0
    xs, ys = np.arange(0, 640 / k, step / k, dtype=F), np.arange(0, 480 / k, step / k, dtype=F)
    g = np.stack(np.meshgrid(np.concatenate([xs, [640 / k - 1, 32.25, 10.5]]).astype(F), np.concatenate([ys, [480 / k - 1, 24.75, 11.5]]).astype(F)), -1).reshape(-1, 2)
    return np.ascontiguousarray(g, F)


def test_the_header_has_no_hip_in_it():
    src = open(HDRS[0]).read()
    assert "hip/hip_runtime" not in src and "hipLaunch" not in src and "__global__" not in src


# ---- the model against its second statements
@pytest.mark.parametrize("name", CAM_NAMES)
def test_two_statements_of_the_distortion_the_lift_and_the_velocity_agree(name):
    cam, c = CAMERAS[name], m.camera(CAMERAS[name])
    assert c["no_distortion"] == (not cam[4:].any())
    pts = _grid(53.0, name)
    un = m.lift(c, pts)
    assert un.dtype == np.float32
    x64, y64 = m.lift64(c, pts)
    dx, dy = m.distortion(c, x64, y64)
    prev = un[::-1].copy()
    vel = m.velocity(un, prev, 0.0999)
    for i, (u, v) in enumerate(pts):
        a, b = m.lift_scalar(cam, u, v)
        assert _b32(a) == _b32(un[i, 0]) and _b32(b) == _b32(un[i, 1]), (name, i)
        ddx, ddy = m.distortion_scalar(cam, float(x64[i]), float(y64[i]))
        assert _b64(ddx) == _b64(dx[i]) and _b64(ddy) == _b64(dy[i]), (name, i)
        assert _b32(m.velocity_scalar(un[i, 0], prev[i, 0], 0.0999)) == _b32(vel[i, 0]) and _b32(m.velocity_scalar(un[i, 1], prev[i, 1], 0.0999)) == _b32(vel[i, 1])


@pytest.mark.parametrize("name", CAM_NAMES)
def test_two_statements_of_the_prediction_agree(name):
    pc, cam = oc.predict_case(), CAMERAS[name]
    c = m.camera(cam)
    n_finite = 0
    for w in (pc, dict(pc, **pc["flat"])):
        t = w["table"]
        for k in range(len(t["feature_id"])):
            a, fa = m.predict_one(c, t["obs8"][k, 0, :3], t["estimated_depth"][k], w["poses"][t["start_frame"][k]], w["tic_ric"], w["next_pose"])
            b, fb = m.predict_scalar(cam, t["obs8"][k, 0, :3], t["estimated_depth"][k], w["poses"][t["start_frame"][k]], w["tic_ric"], w["next_pose"])
            assert fa == fb and (not fa or np.array_equal(_b32(a), _b32(b))), (name, k, a, b)      # (a prediction that is not finite is never used)
            n_finite += fa
    assert n_finite >= 20
    pred, count = m.predict(cam, pc["pts"], pc["ids"], pc["flat"]["table"], pc["frame_count"], pc["flat"]["poses"], pc["flat"]["tic_ric"], pc["flat"]["next_pose"])
    held = {int(i): k for k, i in enumerate(pc["ids"])}
    for fid in pc["flat"]["table"]["feature_id"][5:7]:      # Z == 0 and 0 / 0: the held point stays
        assert np.array_equal(pred[held[int(fid)]], pc["pts"][held[int(fid)]])
    assert 0 < count < len(pc["ids"]) - 2


# ---- the host build against the model
@pytest.mark.parametrize("name", CAM_NAMES)
def test_host_lift_distortion_and_prediction_are_the_models(shim, name):
    cam = np.ascontiguousarray(CAMERAS[name])
    c = m.camera(cam)
    pts = _grid(7.0, name)
    un = np.zeros_like(pts)
    shim.shim_obs_lift(_pd(cam), len(pts), pts.ctypes.data_as(PF), un.ctypes.data_as(PF))
    assert np.array_equal(_b32(un), _b32(m.lift(c, pts)))
    prev = un[::-1].copy()
    vel = m.velocity(un[::31], prev[::31], 0.0999)
    assert all(_b32(shim.shim_obs_velocity(float(a), float(b), 0.0999)) == _b32(v) for a, b, v in zip(un[::31].ravel(), prev[::31].ravel(), vel.ravel()))
    bad = cam.copy()
    bad[1] = 0.0
    assert shim.shim_obs_camera_ok(_pd(cam)) == 1 and shim.shim_obs_camera_ok(_pd(bad)) == 0 and shim.shim_obs_camera_ok(_pd(np.where(np.arange(8) == 6, np.nan, cam))) == 0
    x64, y64 = m.lift64(c, pts[::97])
    dx, dy = m.distortion(c, x64, y64)
    for i in range(len(x64)):
        a, b = C.c_double(), C.c_double()
        shim.shim_obs_distortion(_pd(cam), float(x64[i]), float(y64[i]), C.byref(a), C.byref(b))
        assert _b64(a.value) == _b64(dx[i]) and _b64(b.value) == _b64(dy[i])
    pc = oc.predict_case()
    for w in (pc, dict(pc, **pc["flat"])):
        t = w["table"]
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        f64 = lambda a: np.ascontiguousarray(a, np.float64)
        want, count = m.predict(cam, w["pts"], w["ids"], t, w["frame_count"], w["poses"], w["tic_ric"], w["next_pose"])
        got = np.zeros_like(want)
        fid, st, no, de, o0, po, tr, nx, pt, hi = i32(t["feature_id"]), i32(t["start_frame"]), i32(t["n_obs"]), f64(t["estimated_depth"]), f64(t["obs8"][:, 0, :]), \
            f64(w["poses"]), f64(w["tic_ric"]), f64(w["next_pose"]), np.ascontiguousarray(w["pts"], F), i32(w["ids"])
        n = shim.shim_obs_predict(_pd(cam), len(hi), pt.ctypes.data_as(PF), hi.ctypes.data_as(PI), len(fid), fid.ctypes.data_as(PI), st.ctypes.data_as(PI), no.ctypes.data_as(PI),
                                  _pd(de), _pd(o0), w["frame_count"], _pd(po), _pd(tr), _pd(nx), got.ctypes.data_as(PF))
        assert n == count and np.array_equal(_b32(got), _b32(want))


def _host_observe(shim, cam, pts, ids, prev, dt, depth, cols, rows):
    cam = np.ascontiguousarray(cam, D)
    p, i_ = np.ascontiguousarray(pts, F).reshape(-1, 2), np.ascontiguousarray(ids, np.int32)
    pi_, pu = np.ascontiguousarray(prev[0], np.int32), np.ascontiguousarray(prev[1], F)
    n = len(i_)
    io, ob, un, cn = np.zeros(n, np.int32), np.zeros((n, 8)), np.zeros((n, 2), F), np.zeros(4, np.int32)
    dp = np.ascontiguousarray(depth, np.uint16) if depth is not None else None
    shim.shim_obs_observe(_pd(cam), n, p.ctypes.data_as(PF), i_.ctypes.data_as(PI), len(pi_), pi_.ctypes.data_as(PI), pu.ctypes.data_as(PF), float(dt),
                          dp.ctypes.data_as(PU16) if dp is not None else None, cols, rows, io.ctypes.data_as(PI), _pd(ob), un.ctypes.data_as(PF), cn.ctypes.data_as(PI))
    return dict(ids=io, obs8=ob, counters=cn, prev=(io.copy(), un))


@pytest.mark.parametrize("name", oc.NAMES)
def test_host_observe_is_the_models(shim, name):
    c, want = oc.case(name), oc.expected(name)
    C_ = len(c["cameras"])
    prev, tprev = [m.EMPTY_PREV] * C_, [0.0] * C_
    for f, (call, w) in enumerate(zip(c["calls"], want)):
        for k in range(C_):
            pts, ids, _ = w["held"][k]
            g = _host_observe(shim, c["cameras"][k], pts, ids, prev[k], np.float64(call["time"][k]) - np.float64(tprev[k]), call["depth"][k] if call["depth"] is not None else None,
                              c["cols"], c["rows"])
            x = w["frame"][k]
            assert np.array_equal(g["counters"], x["counters"]), (f, k, g["counters"], x["counters"])
            assert np.array_equal(g["ids"], x["ids"]) and np.array_equal(_b64(g["obs8"]), _b64(x["obs8"])), (f, k)
            assert np.array_equal(g["prev"][0], x["prev"][0]) and np.array_equal(_b32(g["prev"][1]), _b32(x["prev"][1])), (f, k)
            prev[k] = g["prev"]
        tprev = list(call["time"])


def test_the_cases_reach_every_branch():
    E = oc.expected
    a = E("three_cameras")
    assert [len(h[1]) for h in a[0]["held"]] == [0, 1, 37] and (a[0]["frame"][2]["obs8"][:, 5:7] == 0).all()                # the first call: no velocity
    assert a[1]["frame"][2]["counters"].tolist()[:2] == [29, 20] and a[1]["frame"][0]["counters"].tolist()[:2] == [2, 0]    # known and new ids
    assert (a[1]["frame"][2]["obs8"][:, 5:7] != 0).any() and a[1]["frame"][1]["counters"][1] == 1
    assert a[1]["frame"][0]["ids"].tolist() == [-2, 3] and (np.diff(a[0]["frame"][2]["ids"]) > 0).all() and (np.diff(oc.case("three_cameras")["calls"][0]["held"][2][1]) < 0).any()
    assert a[2]["frame"][2]["counters"][0] == 29 - 8 and a[2]["frame"][0]["ids"].tolist() == [-2] and a[2]["frame"][2]["counters"][1] == 21      # after remove_outliers
    d0 = a[0]["frame"][2]
    assert d0["counters"][2] == 2 and set(d0["obs8"][:, 7]) >= {0.0, 65.535}                                               # two reads outside; the planted 0 and 65535
    row = {int(i): r for i, r in zip(d0["ids"], d0["obs8"])}
    ids0 = oc.case("three_cameras")["calls"][0]["held"][2][1]
    assert row[int(ids0[0])][7] == (21 * 64 + 11) / 1000 and row[int(ids0[1])][7] == (8 * 64 + 12) / 1000               # 10.5 -> 11, 20.5 -> 21; 11.5 -> 12, 7.5 -> 8
    assert (E("three_cameras_no_depth")[0]["frame"][2]["obs8"][:, 7] == -2.4).all()
    assert [w["frame"][0]["counters"][0] for w in E("capacity_2048")] == [2048, 65, 64, 63] and all(w["frame"][0]["counters"][1] > 0 for w in E("capacity_2048")[1:])
    assert E("duplicate")[0]["frame"][0]["counters"][3] == 1 and E("duplicate")[0]["frame"][1]["counters"][3] == 0
    assert all(w["frame"][k]["counters"][3] == 0 for n in ("three_cameras", "capacity_2048") for w in E(n) for k in range(len(w["frame"])))


@pytest.mark.parametrize("n", oc.SORT_LENGTHS)
def test_host_sort_and_duplicate_flag_are_the_models(shim, n):
    for dup in (False, True):
        ids = oc.sort_ids(n, duplicate=dup)
        order = np.zeros(max(n, 1), np.int32)
        flag = shim.shim_obs_sort(n, ids.ctypes.data_as(PI), order.ctypes.data_as(PI))
        want, wflag = m.sort_ids(ids)
        assert flag == wflag == int(dup and n >= 2) and np.array_equal(order[:n], want), (n, dup)


def test_sanitized_stand_alone_program():
    """gfbe_obs.h under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _cxx(os.path.join(ROOT, "tests", "obs_host_main.cpp"), os.path.join(BUILD, "obs_host_main"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the rounding rule of O5
def test_depth_rounds_half_away_from_zero(shim):
    d = oc.depth_image()
    dep, outside = m.depth_lookup(np.array([[10.5, 3.0], [11.5, 3.0], [12.49, 2.5], [-0.5, 3.0], [-0.25, 3.0], [63.5, 3.0], [5.0, 47.5]], F), d)
    assert outside == 3 and dep.tolist() == [(3 * 64 + 11) / 1000, (3 * 64 + 12) / 1000, (3 * 64 + 12) / 1000, 0.0, (3 * 64) / 1000, 0.0, 0.0]
    assert m.c_round([10.5, 11.5, -0.5, -1.5, 0.49999997, 2.5]).tolist() == [11, 12, -1, -2, 0, 3]
    for u, col in ((10.5, 11), (11.5, 12)):
        x, y = C.c_int32(), C.c_int32()
        assert shim.shim_obs_depth_index(u, 3.0, 64, 48, C.byref(x), C.byref(y)) == 1 and (x.value, y.value) == (col, 3)
    assert gf.abi is abi and round(10.5) == 10      # (Python's own round and cvRound go to even: neither is the rule)


# ---- the model alone: spaceToPlane(lift(p)) returns to p
# Measured with the committed model on the grid of _grid(16) (every 16th pixel of 640 x 480, the last row and column and three fractional
# pixels; the lift in double, before its cast to float): the largest |spaceToPlane(lift(p)) - p| in pixels is
#   no distortion (cam1_pinhole, color, gctestcam, isaacsim_cam0/1, wt_cam)   <= 1.14e-13
#   cam0_pinhole 3.69e-08      idc_cam 4.00e-03      wt_cam2 1.11e-10
# (eight fixed-point steps do not converge to the last bit at the image corners of the distorted models). The bound is the power of ten
# above the largest, 4.00e-03 px: 1e-2 px. A correction with the wrong sign gives 11.8 px (cam0_pinhole), 22.0 px (idc_cam) and 16.9 px
# (wt_cam2), three orders above the bound; swapped p1 / p2 give 1.83 px (cam0_pinhole) and 9.50 px (idc_cam), two to three orders above
# it. wt_cam2 (p1 = p2 = 0) cannot see a swap and is asserted on the sign alone.
K_ROUND_TRIP = 1e-2


def _round_trip(c, pts, c_back=None):
    x, y = m.lift64(c, pts)
    u, v = m.space_to_plane(c_back or c, x, y)
    return float(max(np.abs(u - pts[:, 0].astype(D)).max(), np.abs(v - pts[:, 1].astype(D)).max()))


@pytest.mark.parametrize("name", sorted(oc.golden_cameras()))
def test_model_round_trip(name):
    """So that "bits equal the model" cannot hide a wrong model: projecting the lifted point must give the pixel back."""
    cam = oc.golden_cameras()[name]
    c, pts = m.camera(cam), _grid(16.0)
    worst = _round_trip(c, pts)
    print("round trip", name, "worst %.3e px" % worst)
    assert worst <= K_ROUND_TRIP
    if not c["no_distortion"]:
        flipped = dict(c, **{k: -c[k] for k in ("k1", "k2", "p1", "p2")})      # the correction applied with the wrong sign
        wrong_sign = _round_trip(flipped, pts, c)
        print("  wrong sign %.3e px" % wrong_sign)
        assert wrong_sign > 100 * K_ROUND_TRIP
        if c["p1"] != 0.0 or c["p2"] != 0.0:
            swapped = _round_trip(dict(c, p1=c["p2"], p2=c["p1"]), pts, c)
            print("  swapped p1 / p2 %.3e px" % swapped)
            assert swapped > 100 * K_ROUND_TRIP


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
    par = {"int32_t": C.c_int32, "gfbe_ctx*": C.c_void_p, "gfbe_klt*": C.c_void_p, "gfbe_obs*": C.c_void_p, "gfbe_ftab*": C.c_void_p, "gfbe_obs**": P(C.c_void_p),
           "const gfbe_obs_options*": P(abi.ObsOptions), "gfbe_obs_options*": P(abi.ObsOptions), "float*": P(C.c_float), "const int32_t*": P(C.c_int32),
           "int32_t*": P(C.c_int32), "const double*": P(C.c_double), "double*": P(C.c_double), "const uint16_t*": P(C.c_uint16)}
    ret = {"void": None, "gfbe_status": C.c_int32}
    table = gf.signatures.OBS
    protos = _prototypes("gfbe_obs.h", "gfbe_obs_")
    assert {p[1] for p in protos} == {"gfbe_obs_" + k for k in table} == set(gf.backend.OBS_EXPORTS) and len(protos) == 9
    assert gf.signatures.TABLES["gfbe_obs_"] is table
    for r, name, params in protos:
        res, args = table[name[len("gfbe_obs_"):]]
        assert res is ret[r], name
        assert len(args) == len(params), name
        for k, (p, a) in enumerate(zip(params, args)):
            assert a is par[p], (name, k, p, a)


def test_the_other_surfaces_are_unchanged():
    """EXPORTS, LC6_EXPORTS, KLT_EXPORTS and DET_EXPORTS: the names and signatures the headers declare, none of them the new ones."""
    b, s = gf.backend, gf.signatures
    assert (len(b.EXPORTS), len(b.LC6_EXPORTS), len(b.KLT_EXPORTS), len(b.DET_EXPORTS)) == (len(s.GFBE), 3, 8, 7)
    others = set(b.EXPORTS) | set(b.LC6_EXPORTS) | set(b.KLT_EXPORTS) | set(b.DET_EXPORTS)
    assert not set(b.OBS_EXPORTS) & others and len(others) == len(b.EXPORTS) + 18
    assert s.GFBE["ftab_add_frame"] == (C.c_int32, [C.c_void_p, C.c_void_p] + [C.POINTER(C.c_int32)] * 3 + [C.POINTER(C.c_double)] * 2 + [C.POINTER(C.c_int32)] * 2 + [C.POINTER(C.c_double)])
    for header, prefix, table in (("gfbe_klt.h", "gfbe_klt_", s.KLT), ("gfbe_det.h", "gfbe_det_", s.DET), ("gfbe_lc6.h", "gfbe_lc6_", s.LC6)):
        assert {p[1] for p in _prototypes(header, prefix)} == {prefix + k for k in table}, header
    declared = {p[1] for p in _prototypes("gfbe.h", "gfbe_")}
    assert declared == set(b.EXPORTS), declared ^ set(b.EXPORTS)


def test_no_signature_is_declared_outside_the_table():
    src = open(os.path.join(ROOT, "ground-fusion2_amd", "abi.py")).read()
    tail = src[src.index("OBS_PREFIX"):]
    assert ".restype" not in tail and ".argtypes" not in tail


def test_options_struct_matches_the_c_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gfbe_obs.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(gfbe_obs_options));']
    for f, _ in abi.ObsOptions._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(gfbe_obs_options, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.ObsOptions) == 16
    for f, _ in abi.ObsOptions._fields_:
        assert int(got[f]) == getattr(abi.ObsOptions, f).offset, f


def test_c_abi_without_a_device():
    gf.build_native()
    lib = abi.bind(abi.bind(abi.bind(C.CDLL(gf.lib_path()), "gfbe_"), abi.KLT_PREFIX), abi.OBS_PREFIX)
    for name in gf.backend.OBS_EXPORTS:
        assert hasattr(lib, name), name
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    o = abi.obs_default_options(lib)
    assert (o.struct_size, o.depth_cam, o.match_tile, o.reserved) == (C.sizeof(abi.ObsOptions), 1, 256, 0)
    fake = C.c_void_p(1)
    cams = np.ascontiguousarray(np.stack([oc.NO_DISTORTION, oc.STRONG]))

    def create(opt=None):
        h = C.c_void_p(7)
        rc = lib.gfbe_obs_create(ctx, fake, _pd(cams), C.byref(opt) if opt is not None else None, C.byref(h))
        assert not h.value      # no handle comes back
        return rc
    # a well-formed call fails loudly: no device, no CPU fallback (the tracker is not looked at: there can be none)
    assert create() == abi.NO_DEVICE and b"gfbe_obs_create" in lib.gfbe_last_error(ctx) and b"no CPU fallback" in lib.gfbe_last_error(ctx)
    for kw in (dict(struct_size=C.sizeof(abi.ObsOptions) - 8), dict(struct_size=0), dict(struct_size=C.sizeof(abi.DetOptions)), dict(depth_cam=2), dict(depth_cam=-1),
               dict(match_tile=96), dict(match_tile=32), dict(match_tile=2048), dict(match_tile=0)):
        assert create(abi.obs_default_options(lib, **kw)) == abi.BAD_INPUT, kw
    assert create(abi.obs_default_options(lib, depth_cam=0, match_tile=64)) == abi.NO_DEVICE
    out, t = np.full(8, -7, np.int32), np.zeros(2)
    assert lib.gfbe_obs_observe(ctx, fake, _pd(t), None, out.ctypes.data_as(PI), None, None, out.ctypes.data_as(PI)) == abi.NO_DEVICE and (out == -7).all()
    assert b"no CPU fallback" in lib.gfbe_last_error(ctx)
    assert lib.gfbe_obs_add_frame(ctx, fake, fake, out.ctypes.data_as(PI), _pd(t), out.ctypes.data_as(PI), None, None) == abi.NO_DEVICE and (out == -7).all()
    assert lib.gfbe_obs_remove_outliers(ctx, fake, out.ctypes.data_as(PI), None, out.ctypes.data_as(PI)) == abi.NO_DEVICE and (out == -7).all()
    assert lib.gfbe_obs_predict(ctx, fake, fake, out.ctypes.data_as(PI), _pd(t), _pd(t), _pd(t), None, out.ctypes.data_as(PI)) == abi.NO_DEVICE and (out == -7).all()
    assert lib.gfbe_obs_download_prev(ctx, fake, 0, out.ctypes.data_as(PI), None, None) == abi.NO_DEVICE and (out == -7).all()
    assert lib.gfbe_obs_reset(ctx, fake) == abi.NO_DEVICE
    lib.gfbe_obs_destroy(ctx, None)
    lib.gfbe_destroy(ctx)
