"""TEST INFRASTRUCTURE. The cases of the sensor gate, shared by tests/test_gate_model.py (the host build of the header, on the CPU) and
tests/test_gpu_gate.py (the device). A case is (options, script, robots): the script fills the W tables of one handle through add_frame /
remove_back (the device's FeatureTables and ftab_model.PyFeatureManager run the same script), robots holds the interval of each robot. The
expected outputs are the model's (tests/gate_np.py), computed once per case."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np

from _gfbe_import import gf
import ftab_model
import gate_np as m

G_NORM = 9.805
CAPACITY = 2048
LR = [(0, 10), (9, 10), (3, 7), (0, 1), (5, 10)]      # the (l, r) of G8 every case is asked for


# ---- tables: a track is (id, start, rows [n_obs, 8]); a script is a list of ("add", frame_counts, ids, obs) and ("remove_back",)
def row(x, y, depth, z=1.0):
    return [x, y, z, 320.0 + 460.0 * x, 240.0 + 460.0 * y, 0.0, 0.0, depth]


def random_tracks(rng, n, first_id=0, static=False, depth=(0.05, 12.0)):
    """n tracks whose start and length vary: full-window ones (11 observations), ones that end before frame 10, ones that start late"""
    out = []
    for k in range(n):
        start = int(rng.choice([0, 0, 0, 0, 1, 2, 3, 5, 8, 9, 10]))
        nobs = 11 - start if rng.random() < 0.6 else int(rng.integers(1, 12 - start))
        x, y, d = rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(*depth)
        step = 1e-6 if static else rng.uniform(0.001, 0.02)
        rows = [row(x + step * j + rng.normal(0, step / 10), y - 0.5 * step * j, d + 0.01 * j) for j in range(nobs)]
        out.append((first_id + k, start, np.array(rows)))
    return out


def fixed_tracks(n, first_id, start, xs_l0, depth_l=1.0, depth_r=1.0):
    """n full tracks from `start` on: observation j has x = xs_l0[k] in its first frame and 0 afterwards, y = 0.1 and the depths given"""
    out = []
    for k in range(n):
        nobs = 11 - start
        rows = [row(xs_l0[k] if j == 0 else 0.0, 0.1, depth_r if j == nobs - 1 else depth_l) for j in range(nobs)]
        out.append((first_id + k, start, np.array(rows)))
    return out


def script_of(tables, n_frames=11):
    """The add_frame calls that build W lists of tracks, frame by frame (ids ascending inside a frame)"""
    sc = []
    for fc in range(n_frames):
        ids, obs = [], []
        for tr in tables:
            live = sorted((t for t in tr if t[1] <= fc < t[1] + len(t[2])), key=lambda t: t[0])
            ids.append([t[0] for t in live])
            obs.append(np.array([t[2][fc - t[1]] for t in live]).reshape(-1, 8))
        sc.append(("add", [fc] * len(tables), ids, obs))
    return sc


def run_script(script, tables):
    """tables: W objects with add_frame(fc, ids, obs, td) and remove_back() (ftab_model.PyFeatureManager, or ftab_model.OneTable per table)"""
    for op in script:
        for w, t in enumerate(tables):
            if op[0] == "add":
                t.add_frame(op[1][w], op[2][w], op[3][w], 0.0)
            else:
                t.remove_back()


def run_script_device(script, ft):
    """The same on an abi.FeatureTables of W tables"""
    for op in script:
        if op[0] == "add":
            ft.add_frame(op[1], op[2], op[3], [0.0] * ft.W)
        else:
            ft.remove_back()


def model_tables(script, W):
    t = [ftab_model.PyFeatureManager() for _ in range(W)]
    run_script(script, t)
    return [x.snapshot() for x in t]


# ---- intervals
def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def robot(rng, n_imu, n_wheel, M, stationary_prev=0, frame_count=10, kind="moving", zero_dt=False):
    """kind: moving (IMU and wheel agree: dis small), slip (the wheel reports three times the speed), rest, turning (any motion)"""
    ba = rng.normal(0, 0.02, 3)
    g = np.array([0.0, 0.0, G_NORM])
    if kind in ("moving", "slip"):
        R, V, v_wheel, w = np.eye(3), np.array([0.0, 0.8, 0.0]), np.array([0.8 * (3.0 if kind == "slip" else 1.0), 0.0, 0.0]), np.zeros(3)
    elif kind == "rest":
        R, V, v_wheel, w = rot_z(0.3), np.zeros(3), np.zeros(3), np.zeros(3)
    else:
        R, V, v_wheel, w = rot_z(rng.uniform(-3, 3)) @ rot_z(0.4)[[2, 0, 1]][:, [2, 0, 1]], rng.normal(0, 1.0, 3), rng.normal(0, 1.0, 3), rng.normal(0, 0.5, 3)
    noise = 0.0 if kind == "rest" else 0.05
    acc = lambda: R.T @ g + ba + rng.normal(0, noise, 3)
    imu = np.array([np.concatenate([[0.005], acc(), rng.normal(0, 0.1, 3)]) for _ in range(n_imu)]).reshape(-1, 7)
    wheel = np.array([np.concatenate([[0.02], v_wheel + rng.normal(0, noise / 10, 3), w + rng.normal(0, noise / 10, 3)]) for _ in range(n_wheel)]).reshape(-1, 7)
    spread = 0.001 if kind == "rest" else 0.6
    frames = np.array([np.concatenate([(g + rng.normal(0, spread, 3)) * 0.1, [0.1]]) for _ in range(M)]).reshape(-1, 4)
    if zero_dt:
        frames[M // 2, 3] = 0.0
    return dict(frame_count=frame_count, imu=imu, imu_first=np.concatenate([acc(), rng.normal(0, 0.1, 3)]), wheel=wheel, wheel_first=np.concatenate([v_wheel, w]),
                stationary_prev=stationary_prev, pose=np.concatenate([rng.normal(0, 2.0, 3), R.ravel()]), vel_ba=np.concatenate([V, ba]), g_norm=G_NORM, frames=frames)


# ---- the straddling tables: 21 full tracks whose pair 0 has parallax d each (depth 1, z 1: the term is |d| exactly), the others 0. The mean
#      of pair 0 sits one step of one feature's d either side of threshold / focal: found by bisection over the doubles on the model's own sum.
def straddle(px, still):
    """still: the test is mean * 460 < px (G6's l_still); otherwise mean * 460 > px (l_init). Returns the tracks below and above the flip."""
    o = m.options()
    t = model_tables(script_of([fixed_tracks(21, 0, 0, [px / 460.0] * 21)]), 1)[0]

    def decision(d0):
        t["obs8"][0, 0, 0] = d0      # (feature 0 of the list in frame 0)
        terms = m.pair_terms(o, 1, t, 0)
        assert len(terms) == 21
        v = m.device_sum(21, terms) / np.float64(21) * np.float64(460.0)
        return bool(v < np.float64(px)) if still else not bool(v > np.float64(px)), [d0] + [px / 460.0] * 20
    lo, hi = px / 460.0 * (1 - 1e-6), px / 460.0 * (1 + 1e-6)
    assert decision(lo)[0] and not decision(hi)[0]
    while np.nextafter(lo, np.inf) < hi:      # (the sum, the quotient and the product are monotone in d0)
        mid = lo + (hi - lo) / 2
        if decision(mid)[0]:
            lo = mid
        else:
            hi = mid
    assert np.nextafter(lo, np.inf) == hi
    return fixed_tracks(21, 0, 0, decision(lo)[1]), fixed_tracks(21, 0, 0, decision(hi)[1])


def _cases():
    rng = np.random.default_rng(20261021)
    cs = {}
    # three tables in one handle: empty, 30 features, 1100 features (chunks of 2 with a ragged tail and threads with an empty chunk)
    cs["mix3"] = ({}, script_of([[], random_tracks(rng, 30), random_tracks(rng, 1100, depth=(0.08, 11.0))]),
                 [robot(rng, 0, 0, 1), robot(rng, 1, 1, 6, stationary_prev=1, kind="turning", zero_dt=True), robot(rng, 20, 5, 12, kind="slip")])
    # one robot at rest: every detector agrees
    cs["rest1"] = ({}, script_of([random_tracks(rng, 60, static=True, depth=(0.5, 8.0))]), [robot(rng, 20, 5, 12, kind="rest")])
    # remove_back, then a frame again: the tables live in the other half of the ping-pong buffers
    tr = random_tracks(rng, 80, depth=(0.5, 8.0))
    again = sorted(t for t in tr if t[1] + len(t[2]) == 11)[:40]
    sc = script_of([tr]) + [("remove_back",), ("add", [10], [[t[0] for t in again] + [500, 501]],
                                               [np.array([row(t[2][-1][0] + 0.01, t[2][-1][1], 2.0) for t in again] + [row(0.2, 0.2, 3.0), row(-0.2, 0.1, 3.0)])])]
    cs["pingpong"] = ({}, sc, [robot(rng, 20, 5, 12, kind="moving")])
    # frame_count below WINDOW_SIZE: nothing spans to r
    cs["short"] = ({}, script_of([random_tracks(rng, 50)], n_frames=6), [robot(rng, 20, 5, 6, frame_count=5, kind="turning")])
    # frame_count 0: both displacements are 0 whatever the samples say
    cs["fc0"] = ({}, script_of([random_tracks(rng, 10), []], n_frames=1), [robot(rng, 20, 5, 1, frame_count=0, kind="turning"), robot(rng, 1, 0, 2, frame_count=0, kind="slip")])
    cs["nowheel"] = (dict(use_wheel=0), script_of([random_tracks(rng, 40, static=True, depth=(0.5, 8.0)), random_tracks(rng, 25)]),
                    [robot(rng, 20, 5, 12, kind="rest"), robot(rng, 20, 5, 12, kind="slip")])
    cs["nodetect"] = (dict(wdetect=0), script_of([random_tracks(rng, 25)]), [robot(rng, 20, 5, 12, kind="slip")])
    cs["depth0"] = (dict(depth_mode=0), script_of([random_tracks(rng, 45), random_tracks(rng, 45, static=True)]),
                   [robot(rng, 20, 5, 12, kind="moving", stationary_prev=1), robot(rng, 1, 5, 12, kind="turning")])
    # thresholds. Table 0: pair 0 has exactly 20 members and pair 1 has 21, all still: pair 0 does not count and does not block pair 1.
    # Table 1: depths exactly 0.1 and 10.0 are kept, the next doubles outside are dropped. Table 2: every pair qualifies for l_init, the lowest wins.
    lo_d, hi_d = np.nextafter(0.1, 0.0), np.nextafter(10.0, np.inf)
    edge = (fixed_tracks(6, 0, 0, [0.0] * 6, 0.1, 10.0) + fixed_tracks(6, 10, 0, [0.0] * 6, 10.0, 0.1) + fixed_tracks(5, 20, 0, [0.0] * 5, lo_d, 1.0) +
            fixed_tracks(5, 30, 0, [0.0] * 5, 1.0, hi_d) + fixed_tracks(12, 40, 0, [0.0] * 12, 0.1, 0.1))
    far = [(k, 0, np.array([row(0.01 * k + 0.1 * j, 0.0, 2.0) for j in range(11)])) for k in range(25)]
    cs["thresholds"] = ({}, script_of([fixed_tracks(20, 0, 0, [1e-5] * 20) + fixed_tracks(1, 20, 1, [1e-5]), edge, far]),
                       [robot(rng, 20, 5, 12, kind="rest"), robot(rng, 1, 1, 12, kind="moving"), robot(rng, 20, 5, 12, kind="turning")])
    s_lo, s_hi = straddle(0.5, True)
    i_lo, i_hi = straddle(30.0, False)
    cs["straddle"] = ({}, script_of([s_lo, s_hi, i_lo, i_hi]), [robot(rng, 1, 1, 3, kind="rest") for _ in range(4)])
    return cs


CASES = _cases()
GPU_CASES = sorted(CASES)


@functools.lru_cache(maxsize=None)
def tables(name):
    return model_tables(CASES[name][1], len(CASES[name][2]))


@functools.lru_cache(maxsize=None)
def expected(name):
    """dict(frame=..., stats={mode: ...}, corres={(mode, l, r): [(a, b) per table]}) of the model"""
    kw, _, robots = CASES[name]
    o, t = m.options(**kw), tables(name)
    return dict(frame=m.frame(o, t, robots), stats={mode: m.stats_all(o, mode, t) for mode in (0, 1)},
                corres={(mode, l, r): [m.corresponding(o, mode, x, l, r) for x in t] for mode in (0, 1) for l, r in LR})


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def assert_same(got, want, what):
    """Integers exactly, doubles as bytes"""
    for k, w in want.items():
        g = np.asarray(got[k])
        if np.asarray(w).dtype.kind == "f":
            assert g.shape == np.asarray(w).shape and np.array_equal(bits(g), bits(w)), (what, k, g, w)
        else:
            assert np.array_equal(g, w), (what, k, g, w)


def pack_tables(tabs):
    """(toff [B + 1], start [N], nobs [N], obs [N, 11, 8]) of a list of table dicts"""
    toff = np.zeros(len(tabs) + 1, np.int32)
    toff[1:] = np.cumsum([len(t["start_frame"]) for t in tabs])
    cat = lambda k, shape, dt: np.ascontiguousarray(np.concatenate([np.asarray(t[k], dt).reshape(shape) for t in tabs]) if tabs else np.zeros(shape, dt).reshape(shape))
    return toff, cat("start_frame", (-1,), np.int32), cat("n_obs", (-1,), np.int32), cat("obs8", (-1, 11, 8), np.float64)


def pack_robots(robots):
    """The packed arguments of gfbe_gate_frame between the tables and the outputs, as a dict of arrays (wheel arrays always present)"""
    col = lambda k: [r[k] for r in robots]
    rag = lambda k, w: gf.abi.gate_ragged(col(k), w)      # (the packing abi.SensorGate.frame does)
    io, iv = rag("imu", 7)
    wo, wv = rag("wheel", 7)
    fo, fv = rag("frames", 4)
    f8 = lambda k, w: np.ascontiguousarray(np.array(col(k), np.float64).reshape(len(robots), w))
    return dict(frame_count=np.array(col("frame_count"), np.int32), imu_off=io, imu=iv, imu_first=f8("imu_first", 6), wheel_off=wo, wheel=wv, wheel_first=f8("wheel_first", 6),
                pose=f8("pose", 12), vel_ba=f8("vel_ba", 6), g_norm=float(robots[0]["g_norm"]), stationary_prev=np.array(col("stationary_prev"), np.int32), frames_off=fo, frames=fv)


DOPT = ("dis_threshold", "wheel_still_norm", "preint_still_norm", "var_still", "var_excited", "still_parallax_px", "init_parallax_px", "parallax_focal", "depth_min", "depth_max")


def opt_arrays(o, mode):
    return np.array([o["use_wheel"], o["wdetect"], o["min_pair_count"], mode], np.int32), np.array([o[k] for k in DOPT], np.float64)


def dump(path, names):
    """The file tests/gate_host_main.cpp reads: every case and the model's outputs of gfbe_gate_frame"""
    parts = [np.array([len(names)], np.int32)]
    for name in names:
        kw, _, robots = CASES[name]
        o, e, p = m.options(**kw), expected(name)["frame"], pack_robots(robots)
        parts += list(opt_arrays(o, o["depth_mode"])) + [np.array([len(robots)], np.int32)] + list(pack_tables(tables(name)))
        parts += [p["frame_count"], p["imu_off"], p["imu"], p["imu_first"], p["wheel_off"], p["wheel"], p["wheel_first"], p["pose"], p["vel_ba"], np.array([p["g_norm"]]),
                  p["stationary_prev"], p["frames_off"], p["frames"]]
        parts += [np.asarray(e[k], np.int32) for k in ("flags", "l_still", "l_init", "pair_count")]
        parts += [np.asarray(e[k], np.float64) for k in ("pair_sum", "dP_imu", "dP_wheel", "dis", "var", "pose_out", "vel_out")]
    with open(path, "wb") as f:
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())


# ---- the host build of ground-fusion2_amd/csrc/gfbe_gate.h with a plain C++ compiler (g++ -O2 -ffp-contract=off, no HIP)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
HEADER = os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_gate.h")
PI, PD = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def build(src, out, extra):
    """src -> out when out is older than src or the header; returns out"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if not cxx:
        raise RuntimeError("no C++ compiler: gfbe_gate.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, HEADER)):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


def load_shim():
    lib = C.CDLL(build(os.path.join(ROOT, "tests", "gate_host_shim.cpp"), os.path.join(BUILD, "gate_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_gate_delta_rot.argtypes = [PD, PD]
    lib.shim_gate_var.restype, lib.shim_gate_var.argtypes = C.c_double, [PD, C.c_int]
    lib.shim_gate_frame.argtypes = [PI, PD, C.c_int, PI, PI, PI, PD, PI, PI, PD, PD, PI, PD, PD, PD, PD, C.c_double, PI, PI, PD, PI, PI, PI, PI, PD, PD, PD, PD, PD, PD, PD]
    lib.shim_gate_pair_stats.argtypes = [PI, PD, C.c_int, PI, PI, PI, PD, PI, PD, PI, PI]
    lib.shim_gate_corresponding.argtypes = [PI, PD, C.c_int, PI, PI, PD, C.c_int, C.c_int, C.c_int, PD, PD]
    return lib


def _p(a):
    return a.ctypes.data_as(PI if a.dtype == np.int32 else PD)


def shim_frame(lib, o, tabs, robots, packed=None):
    """gfbe_gate_frame's outputs from the host build, as abi.SensorGate.frame returns them (packed: pack_tables(tabs), pack_robots(robots) made before)"""
    B = len(robots)
    io, do = opt_arrays(o, o["depth_mode"])
    (toff, start, nobs, obs), p = packed or (pack_tables(tabs), pack_robots(robots))
    r = dict(flags=np.zeros(B, np.int32), l_still=np.zeros(B, np.int32), l_init=np.zeros(B, np.int32), pair_count=np.zeros((B, 10), np.int32), pair_sum=np.zeros((B, 10)),
             dP_imu=np.zeros((B, 3)), dP_wheel=np.zeros((B, 3)), dis=np.zeros(B), var=np.zeros(B), pose_out=np.zeros((B, 12)), vel_out=np.zeros((B, 3)))
    wh = [_p(p["wheel_off"]), _p(p["wheel"]), _p(p["wheel_first"])] if o["use_wheel"] else [None, None, None]
    lib.shim_gate_frame(_p(io), _p(do), B, _p(toff), _p(start), _p(nobs), _p(obs), _p(p["frame_count"]), _p(p["imu_off"]), _p(p["imu"]), _p(p["imu_first"]), *wh, _p(p["pose"]),
                        _p(p["vel_ba"]), p["g_norm"], _p(p["stationary_prev"]), _p(p["frames_off"]), _p(p["frames"]),
                        *[_p(r[k]) for k in ("flags", "l_still", "l_init", "pair_count", "pair_sum", "dP_imu", "dP_wheel", "dis", "var", "pose_out", "vel_out")])
    return r


def shim_stats(lib, o, mode, tabs):
    B = len(tabs)
    io, do = opt_arrays(o, mode)
    toff, start, nobs, obs = pack_tables(tabs)
    r = dict(pair_count=np.zeros((B, 10), np.int32), pair_sum=np.zeros((B, 10)), l_still=np.zeros(B, np.int32), l_init=np.zeros(B, np.int32))
    lib.shim_gate_pair_stats(_p(io), _p(do), B, _p(toff), _p(start), _p(nobs), _p(obs), _p(r["pair_count"]), _p(r["pair_sum"]), _p(r["l_still"]), _p(r["l_init"]))
    return r


def shim_corres(lib, o, mode, tab, l, r):
    io, do = opt_arrays(o, mode)
    _, start, nobs, obs = pack_tables([tab])
    n = len(start)
    a0 = np.zeros((0, 3))
    c = lib.shim_gate_corresponding(_p(io), _p(do), n, _p(start), _p(nobs), _p(obs), l, r, 0, _p(a0), _p(a0))
    a, b = np.zeros((c, 3)), np.zeros((c, 3))
    assert lib.shim_gate_corresponding(_p(io), _p(do), n, _p(start), _p(nobs), _p(obs), l, r, c, _p(a), _p(b)) == c
    return a, b


def frame_args(robots):
    """The arguments of abi.SensorGate.frame after `tables`"""
    col = lambda k: [r[k] for r in robots]
    return (col("frame_count"), col("imu"), np.array(col("imu_first")), col("wheel"), np.array(col("wheel_first")), np.array(col("pose")), np.array(col("vel_ba")), robots[0]["g_norm"],
            col("stationary_prev"), col("frames"))
