"""Windows with GNSS inside the solve (gfbe_window.gnss_ready; estimator.cpp:2965-3002, 3239-3291, 3462-3496): shared by the CPU
and GPU tests. The measurements come from the scenario's true trajectory through the independent numpy statement of the
pseudo-range / Doppler model in tests/gnss_cases.py (not through the C restatements), so that a solve has something to converge to."""
import numpy as np

from _gfbe_import import gf
import gnss_cases as gc

abi, synth = gf.abi, gf.synth
W = abi.WINDOW_SIZE


class GnssTruth:
    """Receiver clock, anchor and yaw of a whole scenario run + the observations of every keyframe (deterministic in the seed)."""

    def __init__(self, scn, seed, n_per_frame=8, lat=22.3, lon=114.17, h=30.0, two_sided=True):
        self.scn = scn
        rng = np.random.default_rng(seed + 4242)
        self.anc = gc.geo2ecef(lat, lon, h)
        self.yaw = float(rng.uniform(-3.0, 3.0))
        n = scn.n_kf
        self.frame_dt = np.diff(scn.kf_t)
        self.ddt = 30.0 + np.cumsum(rng.normal(0, 0.05, n))
        self.dt = np.zeros((n, 4))
        self.dt[0] = rng.uniform(-2e5, 2e5, 4)
        for i in range(n - 1):
            self.dt[i + 1] = self.dt[i] + 0.5 * (self.ddt[i] + self.ddt[i + 1]) * self.frame_dt[i]
        e, nn, u = gc.enu_axes(lat, lon)
        self.epochs = []          # per keyframe: list of (offset of the observation time from the keyframe, observation dict)
        for g in range(n):
            obs = []
            off0 = float(rng.uniform(-0.02, 0.02))
            for q in range(n_per_frame):
                off = -off0 if (two_sided and q == 0) else off0        # one satellite on the other side of the keyframe time
                t = scn.kf_t[g] + off
                p, _, v, _, _ = scn.kinematics(t)
                az, el = rng.uniform(0, 2 * np.pi), np.radians(rng.uniform(12.0, 88.0))
                los = np.cos(el) * np.sin(az) * e + np.cos(el) * np.cos(az) * nn + np.sin(el) * u
                o = dict(sv_pos=self.anc + rng.uniform(2.0e7, 2.55e7) * los, sv_vel=rng.normal(0, 1800.0, 3), svdt=rng.uniform(-5e-4, 5e-4),
                         svddt=rng.normal(0, 1e-11), tgd=rng.normal(0, 6e-9), pr_uura=rng.uniform(2.0, 6.0), dp_uura=rng.uniform(0.2, 0.6),
                         wavelength=gc.C_LIGHT / rng.choice([1575.42e6, 1602.0e6, 1561.098e6]), ratio=1.0, doy=rng.uniform(1, 366),
                         tow=rng.uniform(0, 604800), frame=0, lower_idx=0, sys_idx=int(rng.integers(0, 4)), psr=0.0, dopp=0.0)
                r, nom = gc.psr_dopp_residual(o, gc.IONO, p, v, p, v, self.dt[g, o["sys_idx"]], self.ddt[g], self.yaw, self.anc)
                wp, wd = nom["sin2"] / o["pr_uura"] * 10.0, nom["sin2"] / o["dp_uura"] * 50.0
                o["psr"] = r[0] / wp + rng.normal(0, 1.0)
                o["dopp"] = -(r[1] / wd + rng.normal(0, 0.1)) / o["wavelength"]
                obs.append((off, o))
            self.epochs.append(obs)

    def window_obs(self, k0):
        """Observations of window k0 the way estimator.cpp:3245-3263 indexes them: frame i, lower_idx, ts_ratio."""
        out = []
        t = self.scn.kf_t
        for i in range(W + 1):
            for off, o in self.epochs[k0 + i]:
                ts = t[k0 + i] + off
                lower = (0 if i == 0 else i - 1) if t[k0 + i] > ts else (W - 1 if i == W else i)
                ratio = (t[k0 + lower + 1] - ts) / (t[k0 + lower + 1] - t[k0 + lower])
                out.append(dict(o, frame=i, lower_idx=lower, ratio=float(ratio)))
        return out

    def state(self, k0, seed, noise=True):
        rng = np.random.default_rng(seed + 99 + k0)
        sc = 1.0 if noise else 0.0
        return dict(rcv_dt=self.dt[k0:k0 + W + 1] + sc * rng.normal(0, 0.5, (W + 1, 4)), rcv_ddt=self.ddt[k0:k0 + W + 1] + sc * rng.normal(0, 0.02, W + 1),
                    yaw_enu_local=self.yaw + sc * 0.002, anc_ecef=self.anc + sc * rng.normal(0, 1.0, 3))

    def block(self, k0, ready=1):
        return dict(obs=self.window_obs(k0), iono=gc.IONO, frame_dt=self.frame_dt[k0:k0 + W], ddt_weight=10.0, ready=ready)


def gnss_window(seed=81, L=150, n_per_frame=8, noise=True, anchor=False, **kw):
    """First window of a scenario with GNSS ready: returns (scenario, GNSS truth, snapshot)."""
    scn = synth.Scenario(seed=seed, n_landmarks=L, use_wheel=True, noise=noise)
    tru = GnssTruth(scn, seed, n_per_frame=n_per_frame, **kw)
    snap = scn.window(0)
    snap["gnss"], snap["gnss_state"] = tru.block(0), tru.state(0, seed, noise)
    if anchor:      # first_optimization && GNSS_ENABLE (estimator.cpp:3004-3012)
        snap["anchor"] = dict(pose=snap["pose"][0].copy(), sqrt_info=120.0)
    return scn, tru, snap


def next_gnss_window(scn, tru, res, seed=81):
    """The following window: slideWindow's shift of the state (estimator.cpp:3736-3743 for the receiver clock), the prior of `res`."""
    st = synth.shift_state_for_next_window(scn, res["state"], 1)
    nxt = scn.window(1, state=st, prior=res["prior"])
    g, fresh = res["state"]["gnss_state"], tru.state(1, seed)
    nxt["gnss_state"] = dict(rcv_dt=np.vstack([g["rcv_dt"][1:], fresh["rcv_dt"][-1:]]), rcv_ddt=np.concatenate([g["rcv_ddt"][1:], fresh["rcv_ddt"][-1:]]),
                             yaw_enu_local=g["yaw_enu_local"], anc_ecef=g["anc_ecef"])
    nxt["gnss"] = tru.block(1)
    return nxt


# ---------------------------------------------------------------------------------------------------------------- windows of the normal-equation pins
# Windows tests/test_gpu_gnss_normal_equations.py compares H and g of, entry by entry (60 landmarks each). Observations per frame 0..10:
NE_COUNTS = {
    "n8": [8] * 11,                                   # 88: staged in LDS, the work item of k_lin_small in the candidate pass
    "clock_only": [0] * 11,                           # gnss_ready without one observation: the clock chains alone
    "one_obs": [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0],
    "gaps": [8, 0, 8, 0, 0, 8, 0, 8, 0, 0, 8],        # empty frames between full ones, frame 10 among the full ones
    "one_frame": [0, 0, 0, 0, 0, 30, 0, 0, 0, 0, 0],
    "n256": [24] * 10 + [16],                         # GN_ITEM_MAX_OBS and one more: the launch of k_gnss in place of the work item
    "n257": [24] * 10 + [17],
    "n320": [30] * 10 + [20],                         # GN_LDS_OBS and one more: the sums from the global copy
    "n321": [30] * 10 + [21],
    "one_constellation": [6] * 11,
    "const_frame": [8] * 11,                          # pose 4 and speed-bias 4 constant: their rows and columns are structural zeros
    "anchor": [5] * 11,
    "all_three": [7] * 11,                            # GNSS, PlaneFactors (free plane blocks) and the anchor
    "lowspeed": [6] * 11,                             # no GNSS dim in the program
    # pose 0 constant: the P_0 columns of the observations of frames 0 and 1 drop out, and the gauge fix behind a solve is the identity,
    # so the state a solve hands back is the one its next linearisation ran at (the windows of the second-linearisation comparison)
    "n8_hold0": [8] * 11,
    "n257_hold0": [24] * 10 + [17],
}
NE_EXTRA = ("plane_free", "plane_const", "second", "plain")    # windows without GNSS with PlaneFactors (free / constant plane blocks); the window
                                                               # that follows a GNSS window, with its ~95-dim prior; a window with none of it
_ne_cache, _truth_cache = {}, {}


def ne_case_names():
    return [n for n in NE_COUNTS if n != "n257_hold0"] + list(NE_EXTRA) + ["n257_hold0"]      # (a case's place here is part of its seed)


def _truth(seed, n_per_frame, L=60):
    key = (seed, n_per_frame, L)
    if key not in _truth_cache:
        _truth_cache[key] = gnss_window(seed=seed, L=L, n_per_frame=n_per_frame)
    return _truth_cache[key]


def _with_plane(snap, seed, const):
    rng = np.random.default_rng(seed)
    q = synth.so3_exp(rng.normal(0, 0.01, 3))
    q[2] = 0.0
    snap["plane_R"] = q / np.linalg.norm(q)
    snap["plane_Z"] = -float(snap["ex_pose_wheel"][2]) + 0.02
    snap["plane"] = dict(noise_inv=[100.0, 100.0, 50.0], const=const)
    return snap


def ne_case(name, oracle=None):
    """The window of case `name`. Deterministic; cached per process and never modified afterwards."""
    if name in _ne_cache:
        return _ne_cache[name]
    seed = 8100 + ne_case_names().index(name)
    if name in NE_COUNTS:
        counts = NE_COUNTS[name]
        per = max(max(counts), 1)
        scn, tru, base = _truth(8100 if per > 8 else seed, 30 if per > 8 else per)      # (the large windows share one scenario's satellites)
        snap = dict(base)
        snap["gnss"] = dict(base["gnss"])
        seen, obs = [0] * 11, []
        for o in base["gnss"]["obs"]:                # frame-major; the first observation of a frame is the one on the other side of the keyframe
            if seen[o["frame"]] < counts[o["frame"]]:
                seen[o["frame"]] += 1
                obs.append(dict(o))
        assert seen == counts
        if name == "one_constellation":              # every satellite of constellation 2: the measurement moves with the clock bias it now meets
            for o in obs:
                o["psr"] += tru.dt[o["frame"], 2] - tru.dt[o["frame"], o["sys_idx"]]
                o["sys_idx"] = 2
        snap["gnss"]["obs"] = obs
        if name.endswith("_hold0"):
            snap["pose_const"] = np.zeros(11, np.uint8)
            snap["pose_const"][0] = 1
        if name == "const_frame":
            snap["pose_const"], snap["sb_const"] = np.zeros(11, np.uint8), np.zeros(11, np.uint8)
            snap["pose_const"][4] = snap["sb_const"][4] = 1
        if name in ("anchor", "all_three"):
            snap["anchor"] = dict(pose=snap["pose"][0].copy(), sqrt_info=120.0)
        if name == "all_three":
            _with_plane(snap, seed, 0)
        if name == "lowspeed":
            snap["speed_bias"] = np.array(snap["speed_bias"], float).copy()
            snap["speed_bias"][:, :2] *= 0.2
    elif name in ("plane_free", "plane_const"):
        snap = _with_plane(synth.Scenario(seed=seed, n_landmarks=60, use_wheel=True).window(0), seed, int(name == "plane_const"))
    elif name == "plain":
        snap = synth.Scenario(seed=seed, n_landmarks=60, use_wheel=True).window(0)
    elif name == "second":
        scn, tru, first = _truth(seed, 6)
        snap = next_gnss_window(scn, tru, oracle.solve(first, abi.MARGIN_OLD), seed=seed)
    else:
        raise KeyError(name)
    _ne_cache[name] = snap
    return snap


_ne_ref_cache = {}


def ne_reference(name, oracle):
    """(window, the oracle's per-factor blocks, the extended-precision reference system) of a case; cached per process, left unchanged."""
    import normal_equations_np as ne
    if name not in _ne_ref_cache:
        snap = ne_case(name, oracle)
        ev = oracle.eval_factors(snap, robustify=True)
        _ne_ref_cache[name] = (snap, ev, ne.reference_system(snap, ev))
    return _ne_ref_cache[name]


def at_state(snap, res):
    """The window `snap` at the state a solve left it in (res: one window's download). A solve hands every quaternion back through a
    rotation matrix, in the canonical sign; the solve itself carries q (x) dq along, and the inertial factor's 2 vec(q) arithmetic is
    not blind to the sign: each quaternion gets the sign that continues the window's own."""
    out = dict(snap, para_feature=np.array(res["feature"], float))
    for k, v in res["state"].items():
        if k in snap or k == "gnss_state":
            out[k] = v
    pose = np.array(out["pose"], float)
    flip = (pose[:, 3:] * np.asarray(snap["pose"], float)[:, 3:]).sum(axis=1) < 0
    pose[flip, 3:] *= -1.0
    out["pose"] = pose
    for k in ("ex_pose", "ex_pose_wheel"):
        q = np.array(out[k], float)
        if q[3:] @ np.asarray(snap[k], float)[3:] < 0:
            q[3:] *= -1.0
        out[k] = q
    if "gnss_state" not in snap:
        out.pop("gnss_state", None)
    return out
