"""ctypes mirror of include/gfbe.h (the C-ABI drop-in boundary of Estimator::optimization(),
reference: Ground-Fusion++/vins_estimator/src/estimator/estimator.cpp:2951-3698).

A *window snapshot* is a plain dict of numpy arrays holding everything one optimization() call
reads. `make_window` turns it into a `gfbe_window` whose pointers alias the
numpy buffers (the returned holder keeps them alive).
"""
import ctypes as C
import numpy as np

WINDOW_SIZE = 10
NFRAMES = 11
DENSE_DIM = 246
CORE_DIM = 187      # the tangent dims without the GNSS blocks
MAX_PRIOR_BLOCKS = 32
PRIOR_X0_CAP = NFRAMES * 16 + 32

OK, NO_CONVERGENCE, NUMERICAL_FAILURE, BAD_INPUT, DEVICE_ERROR, NO_DEVICE = range(6)
MARGIN_OLD, MARGIN_SECOND_NEW, MARGIN_NONE = 0, 1, 2

BLK_POSE0, BLK_SB0, BLK_EX_CAM, BLK_EX_WHEEL = 0, 11, 22, 23
BLK_SX, BLK_SY, BLK_SW, BLK_TD, BLK_TD_WHEEL, BLK_PLANE_R, BLK_PLANE_Z = 24, 25, 26, 27, 28, 29, 30
BLK_ANC_ECEF, BLK_YAW_ENU, BLK_RCV_DT0, BLK_RCV_DDT0, BLK_COUNT = 31, 32, 33, 77, 88     # GNSS blocks (rcv_dt: + 4 frame + constellation)

c_d = C.c_double
c_i = C.c_int32
c_u8 = C.c_uint8
PD = C.POINTER(c_d)
PI = C.POINTER(c_i)
PU8 = C.POINTER(c_u8)


def block_global_size(bid):
    if bid < BLK_SB0:
        return 7
    if bid < BLK_EX_CAM:
        return 9
    if bid in (BLK_EX_CAM, BLK_EX_WHEEL):
        return 7
    if bid == BLK_PLANE_R:
        return 4
    if bid == BLK_ANC_ECEF:
        return 3
    return 1


def block_tangent_offset(bid):
    """First tangent dim of block `bid` in the DENSE_DIM-wide layout of the solver."""
    if bid < BLK_SB0:
        return 6 * bid
    if bid < BLK_EX_CAM:
        return 73 + 9 * (bid - BLK_SB0)
    if bid >= BLK_RCV_DDT0:
        return 235 + (bid - BLK_RCV_DDT0)
    if bid >= BLK_RCV_DT0:
        return 191 + (bid - BLK_RCV_DT0)
    return {BLK_EX_CAM: 66, BLK_TD: 72, BLK_EX_WHEEL: 172, BLK_SX: 178, BLK_SY: 179, BLK_SW: 180, BLK_TD_WHEEL: 181, BLK_PLANE_R: 182,
            BLK_PLANE_Z: 186, BLK_ANC_ECEF: 187, BLK_YAW_ENU: 190}[bid]


def block_local_size(bid):
    g = block_global_size(bid)
    return 6 if g == 7 else g


class GnssObs(C.Structure):
    _fields_ = [("sv_pos", c_d * 3), ("sv_vel", c_d * 3), ("svdt", c_d), ("svddt", c_d), ("tgd", c_d), ("pr_uura", c_d), ("dp_uura", c_d),
                ("psr", c_d), ("dopp", c_d), ("wavelength", c_d), ("ratio", c_d), ("doy", c_d), ("tow", c_d),
                ("frame", c_i), ("lower_idx", c_i), ("sys_idx", c_i), ("_pad", c_i)]


class GnssState(C.Structure):
    _fields_ = [("rcv_dt", (c_d * 4) * NFRAMES), ("rcv_ddt", c_d * NFRAMES), ("yaw_enu_local", c_d), ("anc_ecef", c_d * 3)]


class State(C.Structure):
    _fields_ = [("para_Pose", (c_d * 7) * NFRAMES),
                ("para_SpeedBias", (c_d * 9) * NFRAMES),
                ("para_Ex_Pose", c_d * 7),
                ("para_Ex_Pose_wheel", c_d * 7),
                ("para_Ix_wheel", c_d * 3),
                ("para_Td", c_d),
                ("para_Td_wheel", c_d),
                ("para_plane_R", c_d * 4),
                ("para_plane_Z", c_d),
                ("gnss", GnssState)]


class ImuPreint(C.Structure):
    _fields_ = [("sum_dt", c_d), ("delta_p", c_d * 3), ("delta_q", c_d * 4), ("delta_v", c_d * 3),
                ("linearized_ba", c_d * 3), ("linearized_bg", c_d * 3),
                ("jacobian", c_d * 225), ("covariance", c_d * 225)]


class WheelPreint(C.Structure):
    _fields_ = [("sum_dt", c_d), ("delta_p", c_d * 3), ("delta_q", c_d * 4),
                ("linearized_sx", c_d), ("linearized_sy", c_d), ("linearized_sw", c_d), ("linearized_td", c_d),
                ("linearized_vel", c_d * 3), ("linearized_gyr", c_d * 3),
                ("vel_1", c_d * 3), ("gyr_1", c_d * 3),
                ("jacobian", c_d * 18), ("covariance", c_d * 36)]


IMU_DOUBLES = C.sizeof(ImuPreint) // 8      # 467
WHEEL_DOUBLES = C.sizeof(WheelPreint) // 8  # 78


class Prior(C.Structure):
    _fields_ = [("valid", c_i), ("n", c_i), ("n_blocks", c_i),
                ("block_id", c_i * MAX_PRIOR_BLOCKS), ("block_size", c_i * MAX_PRIOR_BLOCKS),
                ("block_idx", c_i * MAX_PRIOR_BLOCKS),
                ("x0", c_d * PRIOR_X0_CAP),
                ("J0", PD), ("r0", PD)]


class Visual(C.Structure):
    _fields_ = [("n_factor", c_i), ("feature_index", PI), ("imu_i", PI), ("imu_j", PI),
                ("pts_i", PD), ("pts_j", PD), ("vel_i", PD), ("vel_j", PD), ("td_i", PD), ("td_j", PD)]


class LioBlock(C.Structure):
    _fields_ = [("n", c_i), ("frame", c_i), ("pts", PD), ("normals", PD), ("offsets", PD), ("weights", PD),
                ("sqrt_info", c_d), ("huber_delta", c_d)]


class Window(C.Structure):
    _fields_ = [("frame_count", c_i), ("state", State),
                ("n_feature", c_i), ("para_Feature", PD), ("feature_const", PU8),
                ("pose_const", c_u8 * NFRAMES), ("sb_const", c_u8 * NFRAMES),
                ("ex_cam_const", c_u8), ("ex_wheel_const", c_u8), ("ix_wheel_const", c_u8),
                ("td_const", c_u8), ("td_wheel_const", c_u8),
                ("ex_cam_mask", c_u8 * 6), ("ex_wheel_mask", c_u8 * 6),
                ("use_plane", c_u8), ("plane_const", c_u8), ("use_anchor", c_u8),
                ("n_imu", c_i), ("imu_frame", PI), ("imu", C.POINTER(ImuPreint)),
                ("n_wheel", c_i), ("wheel_frame", PI), ("wheel", C.POINTER(WheelPreint)),
                ("vis", Visual),
                ("prior", C.POINTER(Prior)),
                ("lio", LioBlock),
                ("plane_noise_inv", c_d * 3), ("anchor_pose", c_d * 7), ("anchor_sqrt_info", c_d),
                ("gnss_ready", c_i), ("n_gnss", c_i), ("gnss_obs", C.POINTER(GnssObs)), ("gnss_iono", PD),
                ("gnss_frame_dt", c_d * WINDOW_SIZE), ("gnss_ddt_weight", c_d)]


class Options(C.Structure):
    _fields_ = [("struct_size", c_i), ("max_num_iterations", c_i), ("huber_delta", c_d), ("vis_sqrt_info", c_d), ("g_norm", c_d),
                ("initial_trust_region_radius", c_d), ("function_tolerance", c_d), ("gradient_tolerance", c_d),
                ("parameter_tolerance", c_d), ("min_relative_decrease", c_d), ("jacobi_scaling", c_i),
                ("marg_eps", c_d), ("marg_sqrt", c_i), ("use_graph", c_i), ("split_batch", c_i),
                ("max_solver_time_in_seconds", c_d), ("host_threads", c_i), ("solve_kernel", c_i),
                ("test_fail_chol_iter", c_i), ("test_fail_chol_count", c_i), ("sharded_mu_retries", c_i), ("speculative_linearization", c_i), ("merge_lin_schur", c_i)]


class Summary(C.Structure):
    _fields_ = [("status", c_i), ("iterations", c_i), ("num_successful", c_i), ("termination", c_i),
                ("initial_cost", c_d), ("final_cost", c_d), ("final_radius", c_d),
                ("cost_history", c_d * 16), ("accepted", c_u8 * 16),
                ("ms_solve", c_d), ("ms_marginalize", c_d), ("bytes_uploaded", c_d), ("bytes_downloaded", c_d)]


class FeatureList(C.Structure):
    _fields_ = [("n", c_i), ("start_frame", PI), ("n_obs", PI), ("obs_offset", PI),
                ("obs", PD), ("obs_td", PD), ("estimated_depth", PD), ("estimate_flag", PI)]


def default_options():
    """Solver options the reference runs with (estimator.cpp:193,2959,3364-3376; m3dgr.yaml:108-117)."""
    o = Options()
    o.struct_size = C.sizeof(Options)
    o.max_num_iterations = 8
    o.huber_delta = 1.0
    o.vis_sqrt_info = 600.0 / 1.5
    o.g_norm = 9.7944
    o.initial_trust_region_radius = 1e4
    o.function_tolerance = 1e-6
    o.gradient_tolerance = 1e-10
    o.parameter_tolerance = 1e-8
    o.min_relative_decrease = 1e-3
    o.jacobi_scaling = 1
    o.marg_eps = 1e-8
    o.marg_sqrt = 1
    o.use_graph = 0
    o.split_batch = 1
    o.max_solver_time_in_seconds = 0.0
    o.host_threads = 0
    o.solve_kernel = 0
    o.test_fail_chol_iter = 0
    o.test_fail_chol_count = 1
    o.sharded_mu_retries = 1
    o.speculative_linearization = 1
    o.merge_lin_schur = 0
    return o


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _pd(a):
    return a.ctypes.data_as(PD)


def _pi(a):
    return a.ctypes.data_as(PI)


def state_from_snapshot(snap, st=None):
    st = st or State()
    pose = _f64(snap["pose"]).reshape(NFRAMES, 7)
    sb = _f64(snap["speed_bias"]).reshape(NFRAMES, 9)
    for i in range(NFRAMES):
        st.para_Pose[i][:] = pose[i].tolist()
        st.para_SpeedBias[i][:] = sb[i].tolist()
    st.para_Ex_Pose[:] = _f64(snap["ex_pose"]).tolist()
    st.para_Ex_Pose_wheel[:] = _f64(snap["ex_pose_wheel"]).tolist()
    st.para_Ix_wheel[:] = _f64(snap["ix_wheel"]).tolist()
    st.para_Td = float(snap["td"])
    st.para_Td_wheel = float(snap["td_wheel"])
    st.para_plane_R[:] = _f64(snap.get("plane_R", [0.0, 0.0, 0.0, 1.0])).tolist()
    st.para_plane_Z = float(snap.get("plane_Z", 0.0))
    g = snap.get("gnss_state")
    if g is not None:
        rd = _f64(g["rcv_dt"]).reshape(NFRAMES, 4)
        for i in range(NFRAMES):
            st.gnss.rcv_dt[i][:] = rd[i].tolist()
        st.gnss.rcv_ddt[:] = _f64(g["rcv_ddt"]).tolist()
        st.gnss.yaw_enu_local = float(g["yaw_enu_local"])
        st.gnss.anc_ecef[:] = _f64(g["anc_ecef"]).tolist()
    return st


def state_to_dict(st):
    return {
        "pose": np.array([list(st.para_Pose[i]) for i in range(NFRAMES)]),
        "speed_bias": np.array([list(st.para_SpeedBias[i]) for i in range(NFRAMES)]),
        "ex_pose": np.array(list(st.para_Ex_Pose)),
        "ex_pose_wheel": np.array(list(st.para_Ex_Pose_wheel)),
        "ix_wheel": np.array(list(st.para_Ix_wheel)),
        "td": float(st.para_Td),
        "td_wheel": float(st.para_Td_wheel),
        "plane_R": np.array(list(st.para_plane_R)),
        "plane_Z": float(st.para_plane_Z),
        "gnss_state": {"rcv_dt": np.array([list(st.gnss.rcv_dt[i]) for i in range(NFRAMES)]), "rcv_ddt": np.array(list(st.gnss.rcv_ddt)),
                       "yaw_enu_local": float(st.gnss.yaw_enu_local), "anc_ecef": np.array(list(st.gnss.anc_ecef))},
    }


def flat_state(d):
    """A state dict with the GNSS blocks lifted to the top level (gnss_rcv_dt, ...): every value an array or a scalar."""
    out = {k: v for k, v in d.items() if k != "gnss_state"}
    for k, v in (d.get("gnss_state") or {}).items():
        out["gnss_" + k] = v
    return out


class PriorHolder:
    """Owns J0/r0 storage for a gfbe_prior (capacity DENSE_DIM) and converts to/from dicts."""

    def __init__(self, d=None):
        self.J0 = np.zeros(DENSE_DIM * DENSE_DIM)
        self.r0 = np.zeros(DENSE_DIM)
        self.c = Prior()
        self.c.J0 = _pd(self.J0)
        self.c.r0 = _pd(self.r0)
        self.c.valid = 0
        if d is not None:
            self.load(d)

    def load(self, d):
        n = int(d["n"])
        nb = len(d["block_id"])
        self.c.valid = int(d.get("valid", 1))
        self.c.n = n
        self.c.n_blocks = nb
        for k in range(nb):
            self.c.block_id[k] = int(d["block_id"][k])
            self.c.block_size[k] = int(d["block_size"][k])
            self.c.block_idx[k] = int(d["block_idx"][k])
        x0 = _f64(d["x0"]).ravel()
        for k in range(len(x0)):
            self.c.x0[k] = x0[k]
        self.J0[: n * n] = _f64(d["J0"]).ravel()
        self.r0[:n] = _f64(d["r0"]).ravel()

    def to_dict(self):
        n, nb = self.c.n, self.c.n_blocks
        sizes = [self.c.block_size[k] for k in range(nb)]
        return {"valid": int(self.c.valid), "n": n,
                "block_id": np.array([self.c.block_id[k] for k in range(nb)], dtype=np.int32),
                "block_size": np.array(sizes, dtype=np.int32),
                "block_idx": np.array([self.c.block_idx[k] for k in range(nb)], dtype=np.int32),
                "x0": np.array([self.c.x0[k] for k in range(sum(sizes))]),
                "J0": self.J0[: n * n].reshape(n, n).copy(), "r0": self.r0[:n].copy()}


class WindowHolder:
    """gfbe_window + the numpy buffers its pointers alias."""

    def __init__(self, snap):
        self.snap = snap
        w = Window()
        self.c = w
        w.frame_count = int(snap.get("frame_count", WINDOW_SIZE))
        state_from_snapshot(snap, w.state)
        self.lam = _f64(snap["para_feature"])
        L = self.lam.shape[0]
        self.fconst = _u8(snap.get("feature_const", np.zeros(L, np.uint8)))
        w.n_feature = L
        w.para_Feature = _pd(self.lam)
        w.feature_const = self.fconst.ctypes.data_as(PU8)
        w.pose_const[:] = _u8(snap.get("pose_const", np.zeros(NFRAMES))).tolist()
        w.sb_const[:] = _u8(snap.get("sb_const", np.zeros(NFRAMES))).tolist()
        w.ex_cam_const = int(snap.get("ex_cam_const", 1))
        w.ex_wheel_const = int(snap.get("ex_wheel_const", 0))
        w.ix_wheel_const = int(snap.get("ix_wheel_const", 1))
        w.td_const = int(snap.get("td_const", 1))
        w.td_wheel_const = int(snap.get("td_wheel_const", 1))
        w.ex_cam_mask[:] = _u8(snap.get("ex_cam_mask", np.zeros(6))).tolist()
        w.ex_wheel_mask[:] = _u8(snap.get("ex_wheel_mask", np.zeros(6))).tolist()
        # optional in-window factors: snap["plane"] = dict(noise_inv=[pitch, roll, zpw], const=0/1); snap["anchor"] = dict(pose=[7], sqrt_info=120)
        pl, an = snap.get("plane"), snap.get("anchor")
        if pl is not None:
            w.use_plane, w.plane_const = 1, int(pl.get("const", 0))
            w.plane_noise_inv[:] = _f64(pl["noise_inv"]).tolist()
        if an is not None:
            w.use_anchor = 1
            w.anchor_pose[:] = _f64(an["pose"]).tolist()
            w.anchor_sqrt_info = float(an.get("sqrt_info", 120.0))
        # GNSS inside the window: snap["gnss"] = dict(obs=[dicts as for gnss_eval], iono=[8] or None, frame_dt=[10], ddt_weight, ready=1);
        # the GNSS state blocks travel in snap["gnss_state"]
        gn = snap.get("gnss")
        if gn is not None:
            self.gnss_obs = gnss_obs_array(gn["obs"])
            self.gnss_iono = _f64(gn["iono"]) if gn.get("iono") is not None else None
            w.gnss_ready, w.n_gnss = int(gn.get("ready", 1)), len(gn["obs"])
            w.gnss_obs = self.gnss_obs
            if self.gnss_iono is not None:
                w.gnss_iono = _pd(self.gnss_iono)
            w.gnss_frame_dt[:] = _f64(gn["frame_dt"]).tolist()
            w.gnss_ddt_weight = float(gn["ddt_weight"])
        # IMU / wheel
        self.imu = _f64(snap.get("imu", np.zeros((0, IMU_DOUBLES)))).reshape(-1, IMU_DOUBLES)
        self.imu_frame = _i32(snap.get("imu_frame", np.zeros(0)))
        w.n_imu = self.imu.shape[0]
        w.imu_frame = _pi(self.imu_frame)
        w.imu = C.cast(self.imu.ctypes.data, C.POINTER(ImuPreint))
        self.wheel = _f64(snap.get("wheel", np.zeros((0, WHEEL_DOUBLES)))).reshape(-1, WHEEL_DOUBLES)
        self.wheel_frame = _i32(snap.get("wheel_frame", np.zeros(0)))
        w.n_wheel = self.wheel.shape[0]
        w.wheel_frame = _pi(self.wheel_frame)
        w.wheel = C.cast(self.wheel.ctypes.data, C.POINTER(WheelPreint))
        # visual
        self.v_idx = _i32(snap["vis_feature_index"])
        self.v_i = _i32(snap["vis_imu_i"])
        self.v_j = _i32(snap["vis_imu_j"])
        self.v_pi = _f64(snap["vis_pts_i"]).reshape(-1, 3)
        self.v_pj = _f64(snap["vis_pts_j"]).reshape(-1, 3)
        self.v_vi = _f64(snap["vis_vel_i"]).reshape(-1, 2)
        self.v_vj = _f64(snap["vis_vel_j"]).reshape(-1, 2)
        self.v_tdi = _f64(snap["vis_td_i"])
        self.v_tdj = _f64(snap["vis_td_j"])
        v = w.vis
        v.n_factor = self.v_idx.shape[0]
        v.feature_index, v.imu_i, v.imu_j = _pi(self.v_idx), _pi(self.v_i), _pi(self.v_j)
        v.pts_i, v.pts_j, v.vel_i, v.vel_j = _pd(self.v_pi), _pd(self.v_pj), _pd(self.v_vi), _pd(self.v_vj)
        v.td_i, v.td_j = _pd(self.v_tdi), _pd(self.v_tdj)
        # prior
        self.prior = None
        if snap.get("prior") is not None:
            self.prior = PriorHolder(snap["prior"])
            w.prior = C.pointer(self.prior.c)
        # LiDAR factors on one pose: snap["lio"] = dict(frame, pts, normals, offsets, weights=None, sqrt_info, huber_delta)
        lio = snap.get("lio")
        if lio is not None and len(lio["pts"]):
            self.lio_pts, self.lio_normals = _f64(lio["pts"]).reshape(-1, 3), _f64(lio["normals"]).reshape(-1, 3)
            self.lio_offsets = _f64(lio["offsets"])
            self.lio_weights = _f64(lio["weights"]) if lio.get("weights") is not None else None
            w.lio.n, w.lio.frame = len(self.lio_pts), int(lio.get("frame", w.frame_count))
            w.lio.pts, w.lio.normals, w.lio.offsets = _pd(self.lio_pts), _pd(self.lio_normals), _pd(self.lio_offsets)
            if self.lio_weights is not None:
                w.lio.weights = _pd(self.lio_weights)
            w.lio.sqrt_info, w.lio.huber_delta = float(lio.get("sqrt_info", 1.0)), float(lio.get("huber_delta", 0.5))

    @property
    def n_vis(self):
        return self.c.vis.n_factor

    @property
    def n_feature(self):
        return self.c.n_feature


def bind(lib, prefix):
    """Types every entry point of signatures.TABLES[prefix] that `lib` exports (gfbe_: the product, gfo_: the oracle,
    gfbe_rccl_: the all-reduce hook; any other prefix: the product's entry points under another name, as a test's host build has
    them) and returns `lib`. Once per library and prefix: a second call changes nothing."""
    from . import signatures      # (it imports the struct mirrors of this module)
    done = vars(lib).setdefault("_bound_prefixes", set())
    if prefix not in done:
        signatures.declare(lib, prefix, signatures.TABLES.get(prefix, signatures.GFBE))
        done.add(prefix)
    return lib


def make_feature_list(fl):
    """fl: dict(start_frame[n], n_obs[n], obs[sum,7], obs_td[sum], estimated_depth[n], estimate_flag[n])."""
    h = {}
    h["start_frame"] = _i32(fl["start_frame"])
    h["n_obs"] = _i32(fl["n_obs"])
    off = np.zeros(len(h["n_obs"]), np.int32)
    if len(off) > 1:
        off[1:] = np.cumsum(h["n_obs"])[:-1]
    h["obs_offset"] = off
    h["obs"] = _f64(fl["obs"]).reshape(-1, 7)
    h["obs_td"] = _f64(fl["obs_td"])
    h["estimated_depth"] = _f64(fl["estimated_depth"])
    h["estimate_flag"] = _i32(fl["estimate_flag"])
    c = FeatureList()
    c.n = len(h["n_obs"])
    c.start_frame, c.n_obs, c.obs_offset = _pi(h["start_frame"]), _pi(h["n_obs"]), _pi(h["obs_offset"])
    c.obs, c.obs_td, c.estimated_depth = _pd(h["obs"]), _pd(h["obs_td"]), _pd(h["estimated_depth"])
    c.estimate_flag = _pi(h["estimate_flag"])
    h["c"] = c
    return h


class CApi:
    """Pythonic calls shared by the product library (prefix gfbe_, first arg = gfbe_ctx*) and the
    CPU oracle (prefix gfo_, first arg = const gfbe_options*). Subclasses set .lib/.prefix/.head."""

    lib = None
    prefix = ""
    head = None          # ctypes object passed as the first argument of compute entry points

    def _fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def check(self, rc, what):
        if rc not in (OK, NO_CONVERGENCE):
            raise RuntimeError("%s%s failed with status %d" % (self.prefix, what, rc))
        return rc

    # ---- a13 bookkeeping
    def build_visual_factors(self, fl, only_start_frame0=False):
        h = make_feature_list(fl)
        c = C.byref(h["c"])
        L = self._fn("feature_count")(c)
        K = self._fn("visual_factor_count")(c, int(only_start_frame0))
        idx, ii, jj = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.int32)
        pi, pj = np.zeros((K, 3)), np.zeros((K, 3))
        vi, vj = np.zeros((K, 2)), np.zeros((K, 2))
        tdi, tdj = np.zeros(K), np.zeros(K)
        lam, fc = np.zeros(L), np.zeros(L, np.uint8)
        k = self._fn("build_visual_factors")(c, int(only_start_frame0), _pi(idx), _pi(ii), _pi(jj), _pd(pi), _pd(pj),
                                            _pd(vi), _pd(vj), _pd(tdi), _pd(tdj), _pd(lam),
                                            fc.ctypes.data_as(PU8))
        assert k == K
        return dict(vis_feature_index=idx, vis_imu_i=ii, vis_imu_j=jj, vis_pts_i=pi, vis_pts_j=pj,
                    vis_vel_i=vi, vis_vel_j=vj, vis_td_i=tdi, vis_td_j=tdj, para_feature=lam, feature_const=fc)

    def set_depth(self, fl, para_feature):
        h = make_feature_list(fl)
        est = h["estimated_depth"].copy()
        flag = np.zeros(len(est), np.int32)
        lam = _f64(para_feature)
        self._fn("set_depth")(C.byref(h["c"]), _pd(lam), _pd(est), _pi(flag))
        return est, flag

    # ---- factor evaluation (block-CSR out)
    def eval_factors(self, snap, robustify=False):
        wh = snap if isinstance(snap, WindowHolder) else WindowHolder(snap)
        K, ni, nw = wh.n_vis, wh.c.n_imu, wh.c.n_wheel
        out = dict(vis_r=np.zeros((K, 2)), vis_J=np.zeros((K, 2, 20)), imu_r=np.zeros((ni, 15)),
                   imu_J=np.zeros((ni, 15, 30)), wheel_r=np.zeros((nw, 6)), wheel_J=np.zeros((nw, 6, 22)))
        npr = wh.prior.c.n if wh.prior is not None else 0
        out["prior_r"] = np.zeros(npr)
        cost = c_d(0.0)
        rc = self._fn("eval_factors")(self.head, C.byref(wh.c), int(robustify), _pd(out["vis_r"]), _pd(out["vis_J"]), _pd(out["imu_r"]),
                                      _pd(out["imu_J"]), _pd(out["wheel_r"]), _pd(out["wheel_J"]),
                                      _pd(out["prior_r"]) if npr else None, C.byref(cost))
        self.check(rc, "eval_factors")
        out["cost"] = cost.value
        return out

    # ---- pre-integration
    def _preintegrate(self, name, intervals, lin, lin_w, noise, out_w, rec_t):
        """intervals: list of (samples[k,7], first[6]); lin: [lin_w] for every interval, or [n, lin_w] per interval."""
        n = len(intervals)
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s, _ in intervals])
        samples = _f64(np.concatenate([np.asarray(s, float).reshape(-1, 7) for s, _ in intervals])) if n else np.zeros((0, 7))
        first = _f64(np.array([f for _, f in intervals], float).reshape(n, 6))
        lin = np.asarray(lin, float)
        if lin.ndim == 1:
            lin = np.tile(lin, (n, 1))
        if lin.shape != (n, lin_w):
            raise ValueError("%s: linearisation point of shape %s, expected (%d,) or (%d, %d)" % (name, lin.shape, lin_w, n, lin_w))
        lin = _f64(lin)
        out = np.zeros((n, out_w))
        nz = _f64(noise)
        f = self._fn(name)
        args = [n, _pi(off), _pd(samples), _pd(first), _pd(lin), _pd(nz), C.cast(out.ctypes.data, C.POINTER(rec_t))]
        rc = f(*([self.head] * (len(f.argtypes) - len(args)) + args))      # (the product's takes its context first, the oracle's nothing)
        self.check(rc, name)
        return out

    def preintegrate_imu(self, intervals, lin_ba, lin_bg, noise):
        """intervals: list of (samples[k,7], first[6]). lin_ba, lin_bg: [3] each (one linearisation point for every interval) or
        [n, 3] each (one per interval: the C ABI's lin_ba_bg [n][6])."""
        lin_ba, lin_bg = np.asarray(lin_ba, float), np.asarray(lin_bg, float)
        if lin_ba.ndim != lin_bg.ndim:
            raise ValueError("preintegrate_imu: lin_ba and lin_bg must both be [3] or both [n, 3]")
        return self._preintegrate("preintegrate_imu", intervals, np.concatenate([lin_ba, lin_bg], axis=-1), 6, noise, IMU_DOUBLES, ImuPreint)

    def preintegrate_wheel(self, intervals, lin, noise):
        """lin: sx, sy, sw, td as [4] (for every interval) or [n, 4] (one per interval)."""
        return self._preintegrate("preintegrate_wheel", intervals, lin, 4, noise, WHEEL_DOUBLES, WheelPreint)

    # ---- the whole optimization() call
    def solve(self, snap, margin_flag=MARGIN_NONE):
        wh = snap if isinstance(snap, WindowHolder) else WindowHolder(snap)
        st = State()
        feat = np.zeros(wh.n_feature)
        pr = PriorHolder()
        sm = Summary()
        rc = self._fn("solve_window")(self.head, C.byref(wh.c), int(margin_flag), C.byref(st), _pd(feat), C.byref(pr.c), C.byref(sm))
        self.check(rc, "solve_window")
        return dict(state=state_to_dict(st), feature=feat, prior=pr.to_dict() if pr.c.valid else None,
                    summary=summary_to_dict(sm), perf=summary_perf(sm), status=rc)

    def solve_raw(self, wh, margin_flag=MARGIN_NONE):
        """solve_window into outputs kept on the holder: the bare C call (latency measurements)."""
        if not hasattr(wh, "_raw_out"):
            wh._raw_out = (State(), np.zeros(max(wh.n_feature, 1)), PriorHolder(), Summary())
        st, feat, pr, sm = wh._raw_out
        return self.check(self._fn("solve_window")(self.head, C.byref(wh.c), int(margin_flag), C.byref(st), _pd(feat), C.byref(pr.c), C.byref(sm)),
                          "solve_window")


def summary_to_dict(sm):
    n = sm.iterations + 1
    return dict(status=sm.status, iterations=sm.iterations, num_successful=sm.num_successful,
                termination=sm.termination, initial_cost=sm.initial_cost, final_cost=sm.final_cost,
                final_radius=sm.final_radius, cost_history=list(sm.cost_history)[:n],
                accepted=list(sm.accepted)[:n])


def summary_perf(sm):
    """The measured part of gfbe_summary (device phase times, PCIe bytes): kept apart from summary_to_dict, whose dicts the
    tests compare for bit-identity between runs."""
    return dict(ms_solve=sm.ms_solve, ms_marginalize=sm.ms_marginalize, bytes_uploaded=sm.bytes_uploaded,
                bytes_downloaded=sm.bytes_downloaded)


# ---------------------------------------------------------------------------------------------
# f1: feature tables (FeatureManager / slideWindow operations), shared by gfbe_ (device) and gfo_ (oracle)
# ---------------------------------------------------------------------------------------------
class FtabOptions(C.Structure):
    _fields_ = [("init_depth", c_d), ("min_parallax", c_d), ("focal_length", c_d), ("depth_threshold", c_d)]


def pose_rows(pose7):
    """[p, q(xyzw)] rows -> [P(3) | R(9, row-major)] rows, the pose argument of the feature-table calls."""
    pose7 = np.asarray(pose7, float).reshape(-1, 7)
    out = np.zeros((len(pose7), 12))
    for k, r in enumerate(pose7):
        x, y, z, w = r[3:] / np.linalg.norm(r[3:])
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        out[k, :3] = r[:3]
        out[k, 3:] = R.ravel()
    return out


def options_struct(lib, prefix, family, cls, fields=None):
    """A `cls` as <prefix><family>default_options fills it, then `fields` (a dict; an array-valued field takes a sequence). A name
    that is no field of the struct is refused."""
    o = cls()
    getattr(bind(lib, prefix), prefix + family + "default_options")(C.byref(o))
    for k, v in (fields or {}).items():
        if not hasattr(o, k):
            raise TypeError("gfbe_%soptions has no field %r" % (family, k))
        cur = getattr(o, k)
        setattr(o, k, type(cur)(*[float(x) for x in v]) if isinstance(cur, C.Array) else v)
    return o


class Handle:
    """Base of the classes that own one opaque handle `h` of a family of entry points <prefix><family>* behind `lib`."""
    family = ""

    def __init__(self, lib, prefix, ctx):
        self.lib, self.prefix, self.ctx, self.h = bind(lib, prefix), prefix, ctx, C.c_void_p()

    def _f(self, name):
        return getattr(self.lib, self.prefix + self.family + name)

    def _check(self, rc, what):
        if rc != OK:
            raise RuntimeError("%s%s%s failed with status %d" % (self.prefix, self.family, what, rc))

    def _options(self, cls, fields=None, family=None):
        return options_struct(self.lib, self.prefix, family or self.family, cls, fields)

    def close(self):
        if self.h:
            self._f("destroy")(self.ctx, self.h)
            self.h = C.c_void_p()


class FeatureTables(Handle):
    """W feature tables behind `lib` (prefix gfbe_: device-resident, ctx = gfbe_ctx*; prefix gfo_: the CPU oracle,
    ctx ignored). Per-table arguments are lists of length W."""
    family = "ftab_"

    def __init__(self, lib, prefix, ctx, n_tables=1, capacity=4096, options=None):
        Handle.__init__(self, lib, prefix, ctx)
        self.W, self.cap = n_tables, capacity
        opt = self._options(FtabOptions, options) if options is not None else None
        self._check(self._f("create")(self.ctx, int(n_tables), int(capacity), C.byref(opt) if opt is not None else None,
                                      C.byref(self.h)), "create")

    @staticmethod
    def _ragged(rows, dtype, width=None):
        off = np.zeros(len(rows) + 1, np.int32)
        off[1:] = np.cumsum([len(r) for r in rows])
        # (reshape(-1, width): a table without rows in the frame is [0, width])
        flat = np.concatenate([np.asarray(r, dtype).reshape(-1, width) if width else np.asarray(r, dtype).ravel() for r in rows]) \
            if off[-1] else np.zeros((0, width) if width else 0, dtype)
        return off, np.ascontiguousarray(flat)

    def add_frame(self, frame_count, ids, obs8, td):
        """ids[w]: ascending feature ids; obs8[w]: [n, 8]. Returns (keyframe[W], counters[W, 3], avg_parallax[W])."""
        off, fid = self._ragged(ids, np.int32)
        _, ob = self._ragged(obs8, np.float64, 8)
        fc, tdv = _i32(frame_count), _f64(td)
        kf, cnt, avg = np.zeros(self.W, np.int32), np.zeros((self.W, 3), np.int32), np.zeros(self.W)
        self._check(self._f("add_frame")(self.ctx, self.h, _pi(fc), _pi(off), _pi(fid), _pd(ob), _pd(tdv), _pi(kf), _pi(cnt), _pd(avg)), "add_frame")
        return kf, cnt, avg

    def remove_back_shift_depth(self, marg_pr, new_pr):
        a, b = _f64(marg_pr).reshape(self.W, 12), _f64(new_pr).reshape(self.W, 12)
        self._check(self._f("remove_back_shift_depth")(self.ctx, self.h, _pd(a), _pd(b)), "remove_back_shift_depth")

    def remove_back(self):
        self._check(self._f("remove_back")(self.ctx, self.h), "remove_back")

    def remove_front(self, frame_count):
        fc = _i32(frame_count)
        self._check(self._f("remove_front")(self.ctx, self.h, _pi(fc)), "remove_front")

    def remove_outlier(self, ids):
        off, flat = self._ragged(ids, np.int32)
        self._check(self._f("remove_outlier")(self.ctx, self.h, _pi(off), _pi(flat)), "remove_outlier")

    def remove_failures(self):
        self._check(self._f("remove_failures")(self.ctx, self.h), "remove_failures")

    def clear_depth(self):
        self._check(self._f("clear_depth")(self.ctx, self.h), "clear_depth")

    def set_depth(self, x):
        off, flat = self._ragged(x, np.float64)
        self._check(self._f("set_depth")(self.ctx, self.h, _pi(off), _pd(flat)), "set_depth")

    def get_depth_vector(self):
        off = (np.arange(self.W + 1) * self.cap).astype(np.int32)
        x, cnt = np.zeros(self.W * self.cap), np.zeros(self.W, np.int32)
        self._check(self._f("get_depth_vector")(self.ctx, self.h, _pi(off), _pd(x), _pi(cnt)), "get_depth_vector")
        return [x[off[w]:off[w] + cnt[w]].copy() for w in range(self.W)]

    def triangulate(self, poses, tic_ric, with_depth=False):
        p, e = _f64(poses).reshape(self.W, 11 * 12), _f64(tic_ric).reshape(self.W, 12)
        self._check(self._f("triangulate")(self.ctx, self.h, _pd(p), _pd(e), int(with_depth)), "triangulate")

    def check_outliers(self, poses, tic_ric, mode):
        p, e = _f64(poses).reshape(self.W, 11 * 12), _f64(tic_ric).reshape(self.W, 12)
        off = (np.arange(self.W + 1) * self.cap).astype(np.int32)
        ids, cnt = np.full(self.W * self.cap, -1, np.int32), np.zeros(self.W, np.int32)   # (touched pages: cheap pageable D2H)
        self._check(self._f("check_outliers")(self.ctx, self.h, _pd(p), _pd(e), int(mode), _pi(off), _pi(ids), _pi(cnt)), "check_outliers")
        return [ids[off[w]:off[w] + cnt[w]].copy() for w in range(self.W)]

    def size(self):
        n = np.zeros(self.W, np.int32)
        self._check(self._f("size")(self.ctx, self.h, _pi(n)), "size")
        return n

    def download(self, w=0):
        n = int(self.size()[w])
        out = dict(feature_id=np.zeros(n, np.int32), start_frame=np.zeros(n, np.int32), n_obs=np.zeros(n, np.int32),
                   obs8=np.zeros((n, 11, 8)), obs_td=np.zeros((n, 11)), estimated_depth=np.zeros(n),
                   estimate_flag=np.zeros(n, np.int32), solve_flag=np.zeros(n, np.int32))
        self._check(self._f("download")(self.ctx, self.h, int(w), _pi(out["feature_id"]), _pi(out["start_frame"]), _pi(out["n_obs"]),
                                        _pd(out["obs8"]), _pd(out["obs_td"]), _pd(out["estimated_depth"]), _pi(out["estimate_flag"]),
                                        _pi(out["solve_flag"])), "download")
        return out


def ftab_to_feature_list(tab):
    """FeatureTables.download() -> the flattened list gfbe_build_visual_factors consumes."""
    rows, tds = [], []
    for k in range(len(tab["n_obs"])):
        for o in range(tab["n_obs"][k]):
            rows.append(tab["obs8"][k, o, :7])
            tds.append(tab["obs_td"][k, o])
    return dict(start_frame=tab["start_frame"], n_obs=tab["n_obs"], obs=np.array(rows).reshape(-1, 7), obs_td=np.array(tds),
                estimated_depth=tab["estimated_depth"], estimate_flag=tab["estimate_flag"])


# ---------------------------------------------------------------------------------------------
# f3: global_fusion pose graph (gfbe_pg_* on the device, gfo_pg_* in the oracle)
# ---------------------------------------------------------------------------------------------
class PoseGraph:
    """Chain pose graph: poses [n,7] = t(3) q(wxyz); rel_i [m]; rel_meas [m,7]; fix_i [k]; fix_meas [k,4] = x y z var."""

    def __init__(self, lib, prefix, ctx):
        self.lib, self.prefix, self.ctx = bind(lib, prefix), prefix, ctx

    def _args(self, g):
        pose = _f64(g["pose"]).reshape(-1, 7)
        ri, rm = _i32(g["rel_i"]), _f64(g["rel_meas"]).reshape(-1, 7)
        fi, fmm = _i32(g["fix_i"]), _f64(g["fix_meas"]).reshape(-1, 4)
        return pose, ri, rm, fi, fmm

    def eval(self, g, t_var=0.1, q_var=0.01, huber=1.0):
        pose, ri, rm, fi, fmm = self._args(g)
        r, J, fr, cost = np.zeros((len(ri), 6)), np.zeros((len(ri), 6, 12)), np.zeros((len(fi), 3)), np.zeros(1)
        rc = getattr(self.lib, self.prefix + "pg_eval")(self.ctx, len(pose), _pd(pose), len(ri), _pi(ri), _pd(rm), t_var, q_var, len(fi),
                                                        _pi(fi), _pd(fmm), huber, _pd(r), _pd(J), _pd(fr), _pd(cost))
        if rc != OK:
            raise RuntimeError("%spg_eval failed with status %d" % (self.prefix, rc))
        return dict(rel_r=r, rel_J=J, fix_r=fr, cost=float(cost[0]))

    def solve(self, g, t_var=0.1, q_var=0.01, huber=1.0, max_iterations=5):
        pose, ri, rm, fi, fmm = self._args(g)
        out, sm = np.zeros_like(pose), Summary()
        rc = getattr(self.lib, self.prefix + "pg_solve")(self.ctx, len(pose), _pd(pose), len(ri), _pi(ri), _pd(rm), t_var, q_var, len(fi),
                                                         _pi(fi), _pd(fmm), huber, int(max_iterations), _pd(out), C.byref(sm))
        if rc not in (OK, NO_CONVERGENCE):
            raise RuntimeError("%spg_solve failed with status %d" % (self.prefix, rc))
        return dict(pose=out, summary=summary_to_dict(sm), status=rc)


def pg_plus(x, d6):
    """ceres::QuaternionParameterization::Plus on q (w,x,y,z) + identity on t; d6 = [dq(3), dt(3)]."""
    x, d6 = np.asarray(x, float), np.asarray(d6, float)
    nrm = np.linalg.norm(d6[:3])
    dq = np.concatenate([[np.cos(nrm)], np.sin(nrm) / nrm * d6[:3]]) if nrm > 0 else np.array([1.0, 0, 0, 0])
    a, b = dq, x[3:]
    q = np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                  a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])
    return np.concatenate([x[:3] + d6[3:], q])


# ---------------------------------------------------------------------------------------------
# f3b: loop-closure pose graph of dense_map, 4-DoF (gfbe_lc4_*; the model is tests/lc4_np.py, there is no oracle row)
# ---------------------------------------------------------------------------------------------
LC4_MAX_LOOPS = 64
LC4_LONG_MAX_LOOPS = 512


class Lc4Options(C.Structure):
    _fields_ = [("struct_size", c_i), ("max_num_iterations", c_i), ("span", c_i), ("reserved", c_i), ("huber_delta", c_d), ("loop_yaw_div", c_d)]


class LoopGraph:
    """Keyframes t [n,3], ypr [n,3] (degrees); see include/gfbe.h f3b."""

    def __init__(self, lib, prefix, ctx):
        self.lib, self.prefix, self.ctx = bind(lib, prefix), prefix, ctx

    def options(self, **kw):
        return options_struct(self.lib, self.prefix, "lc4_", Lc4Options, kw)

    def eval_rc(self, t, ypr, edge_i, edge_j, kind, meas, opt=None):
        t, ypr, meas = _f64(t).reshape(-1, 3), _f64(ypr).reshape(-1, 3), _f64(meas).reshape(-1, 6)
        ei, ej, kd = _i32(edge_i), _i32(edge_j), _u8(kind)
        E = len(ei)
        r, J, cost = np.zeros((E, 4)), np.zeros((E, 4, 8)), np.zeros(1)
        rc = getattr(self.lib, self.prefix + "lc4_eval")(self.ctx, C.byref(opt) if opt is not None else None, len(t), _pd(t), _pd(ypr), E, _pi(ei), _pi(ej),
                                                        kd.ctypes.data_as(PU8), _pd(meas), _pd(r), _pd(J), _pd(cost))
        return rc, dict(r=r, J=J, cost=float(cost[0]))

    def eval(self, *a, **kw):
        rc, out = self.eval_rc(*a, **kw)
        if rc != OK:
            raise RuntimeError("%slc4_eval failed with status %d" % (self.prefix, rc))
        return out

    def solve_rc(self, t, ypr, sequence, fixed, loop_i, loop_c, loop_meas, opt=None, entry="lc4_solve"):
        t, ypr, lm = _f64(t).reshape(-1, 3), _f64(ypr).reshape(-1, 3), _f64(loop_meas).reshape(-1, 4)
        seq, fx, li, lc = _i32(sequence), _u8(fixed), _i32(loop_i), _i32(loop_c)
        n = len(t)
        t_out, yaw_out, drift, sm = np.full((n, 3), np.nan), np.full(n, np.nan), np.full(4, np.nan), Summary()
        rc = getattr(self.lib, self.prefix + entry)(self.ctx, C.byref(opt) if opt is not None else None, n, _pd(t), _pd(ypr), _pi(seq), fx.ctypes.data_as(PU8),
                                                   len(li), _pi(li), _pi(lc), _pd(lm), _pd(t_out), _pd(yaw_out), _pd(drift), C.byref(sm))
        return rc, dict(t=t_out, yaw=yaw_out, drift=drift, summary=summary_to_dict(sm), status=rc)

    def solve(self, *a, **kw):
        rc, out = self.solve_rc(*a, **kw)
        if rc not in (OK, NO_CONVERGENCE):
            raise RuntimeError("%slc4_solve failed with status %d" % (self.prefix, rc))
        return out

    def solve_long_rc(self, *a, **kw):
        """gfbe_lc4_solve_long: up to LC4_LONG_MAX_LOOPS loop edges; arguments and result as solve_rc."""
        return self.solve_rc(*a, entry="lc4_solve_long", **kw)

    def solve_long(self, *a, **kw):
        rc, out = self.solve_long_rc(*a, **kw)
        if rc not in (OK, NO_CONVERGENCE):
            raise RuntimeError("%slc4_solve_long failed with status %d" % (self.prefix, rc))
        return out


# ---------------------------------------------------------------------------------------------
# loop-closure pose graph of dense_map, 6-DoF (gfbe_lc6_* of include/gfbe_lc6.h; the model is tests/lc6_np.py, there is no oracle row)
# ---------------------------------------------------------------------------------------------
LC6_MAX_LOOPS = 128
LC6_PREFIX = "gfbe_lc6_"


class Lc6Options(C.Structure):
    _fields_ = [("struct_size", c_i), ("max_num_iterations", c_i), ("span", c_i), ("reserved", c_i), ("huber_delta", c_d), ("t_var", c_d), ("q_var", c_d)]


def lc6_default_options(lib, **kw):
    return options_struct(lib, LC6_PREFIX, "", Lc6Options, kw)


class LoopGraph6:
    """Keyframes t [n,3], q [n,4] (w, x, y, z); see include/gfbe_lc6.h. `lib` is the product library."""

    def __init__(self, lib, ctx):
        self.lib, self.ctx = bind(lib, LC6_PREFIX), ctx

    def options(self, **kw):
        return lc6_default_options(self.lib, **kw)

    def eval_rc(self, t, q, edge_i, edge_j, kind, meas, opt=None):
        t, q, meas = _f64(t).reshape(-1, 3), _f64(q).reshape(-1, 4), _f64(meas).reshape(-1, 7)
        ei, ej, kd = _i32(edge_i), _i32(edge_j), _u8(kind)
        E = len(ei)
        r, J, cost = np.zeros((E, 6)), np.zeros((E, 6, 12)), np.zeros(1)
        rc = self.lib.gfbe_lc6_eval(self.ctx, C.byref(opt) if opt is not None else None, len(t), _pd(t), _pd(q), E, _pi(ei), _pi(ej), kd.ctypes.data_as(PU8),
                                    _pd(meas), _pd(r), _pd(J), _pd(cost))
        return rc, dict(r=r, J=J, cost=float(cost[0]))

    def eval(self, *a, **kw):
        rc, out = self.eval_rc(*a, **kw)
        if rc != OK:
            raise RuntimeError("gfbe_lc6_eval failed with status %d" % rc)
        return out

    def solve_rc(self, t, q, sequence, fixed, loop_i, loop_c, loop_meas, opt=None, fill=np.nan):
        """The outputs start as `fill`: a refused call leaves them so."""
        t, q, lm = _f64(t).reshape(-1, 3), _f64(q).reshape(-1, 4), _f64(loop_meas).reshape(-1, 7)
        seq, fx, li, lc = _i32(sequence), _u8(fixed), _i32(loop_i), _i32(loop_c)
        n = len(t)
        t_out, q_out, drift, sm = np.full((n, 3), fill), np.full((n, 4), fill), np.full(7, fill), Summary()
        rc = self.lib.gfbe_lc6_solve(self.ctx, C.byref(opt) if opt is not None else None, n, _pd(t), _pd(q), _pi(seq), fx.ctypes.data_as(PU8), len(li), _pi(li), _pi(lc),
                                     _pd(lm), _pd(t_out), _pd(q_out), _pd(drift), C.byref(sm))
        return rc, dict(t=t_out, q=q_out, drift=drift, summary=summary_to_dict(sm), status=rc)

    def solve(self, *a, **kw):
        rc, out = self.solve_rc(*a, **kw)
        if rc not in (OK, NO_CONVERGENCE):
            raise RuntimeError("gfbe_lc6_solve failed with status %d" % rc)
        return out


# ---------------------------------------------------------------------------------------------
# f4: LIO point-to-plane factors (gfbe_lio_linearize / gfo_lio_linearize)
# ---------------------------------------------------------------------------------------------
def lio_linearize(lib, prefix, ctx, ct, pts, normals, offsets, alpha, weights, sqrt_info, pose_begin, pose_end=None, blocks=True):
    """blocks = False: only the normal equations (H = J^T J, g = J^T r, cost) come back — what a caller that feeds a solver needs;
    the per-factor residuals / Jacobians (r [n], J [n][6 or 12]) are not produced or copied."""
    pts, normals, offsets = _f64(pts).reshape(-1, 3), _f64(normals).reshape(-1, 3), _f64(offsets)
    n, dn = len(pts), 12 if ct else 6
    al = _f64(alpha if alpha is not None else np.zeros(n))
    wg = _f64(weights if weights is not None else np.ones(n))
    pb = _f64(pose_begin)
    pe = _f64(pose_end if pose_end is not None else pose_begin)
    r, J = (np.zeros(n), np.zeros((n, dn))) if blocks else (None, None)
    H, g, cost = np.zeros((dn, dn)), np.zeros(dn), np.zeros(1)
    f = getattr(bind(lib, prefix), prefix + "lio_linearize")
    rc = f(ctx, int(ct), n, _pd(pts), _pd(normals), _pd(offsets), _pd(al), _pd(wg), float(sqrt_info), _pd(pb), _pd(pe),
           _pd(r) if blocks else None, _pd(J) if blocks else None, _pd(H), _pd(g), _pd(cost))
    if rc != OK:
        raise RuntimeError("%slio_linearize failed with status %d" % (prefix, rc))
    return dict(r=r, J=J, H=H, g=g, cost=float(cost[0]))


# ---------------------------------------------------------------------------------------------
# f2: optional in-window factors, evaluation only (gfbe_plane_eval / gfbe_anchor_eval / gfbe_orientation_subset_plus)
# ---------------------------------------------------------------------------------------------
def plane_eval(lib, prefix, ctx, pose, ex_wheel, plane_R, plane_Z, noise_inv):
    pose = _f64(pose).reshape(-1, 7)
    n = len(pose)
    ex, q, ni = _f64(ex_wheel), _f64(plane_R), _f64(noise_inv)
    r, J, cost = np.zeros((n, 3)), np.zeros((n, 3, 16)), np.zeros(1)
    f = getattr(bind(lib, prefix), prefix + "plane_eval")
    rc = f(ctx, n, _pd(pose), _pd(ex), _pd(q), float(plane_Z), _pd(ni), _pd(r), _pd(J), _pd(cost))
    if rc != OK:
        raise RuntimeError("%splane_eval failed with status %d" % (prefix, rc))
    return dict(r=r, J=J, cost=float(cost[0]))


def anchor_eval(lib, prefix, ctx, pose, anchor, sqrt_info=120.0):
    pose, anchor = _f64(pose).reshape(-1, 7), _f64(anchor).reshape(-1, 7)
    n = len(pose)
    r, J, cost = np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros(1)
    f = getattr(bind(lib, prefix), prefix + "anchor_eval")
    rc = f(ctx, n, _pd(pose), _pd(anchor), float(sqrt_info), _pd(r), _pd(J), _pd(cost))
    if rc != OK:
        raise RuntimeError("%sanchor_eval failed with status %d" % (prefix, rc))
    return dict(r=r, J=J, cost=float(cost[0]))


def orientation_subset_plus(lib, prefix, q, delta, constant=(0, 0, 1)):
    q, d, m, out = _f64(q), _f64(delta), _u8(constant), np.zeros(4)
    getattr(bind(lib, prefix), prefix + "orientation_subset_plus")(_pd(q), _pd(d), m.ctypes.data_as(PU8), _pd(out))
    return out


# ---------------------------------------------------------------------------------------------
# f2: GNSS factors, evaluation only (gfbe_gnss_eval)
# ---------------------------------------------------------------------------------------------
GNSS_OBS_KEYS = ("svdt", "svddt", "tgd", "pr_uura", "dp_uura", "psr", "dopp", "wavelength", "ratio", "doy", "tow", "frame", "lower_idx", "sys_idx")


def gnss_obs_array(obs):
    """list of dicts with sv_pos, sv_vel and GNSS_OBS_KEYS -> ctypes array of gfbe_gnss_obs"""
    arr = (GnssObs * max(len(obs), 1))()
    for k, o in enumerate(obs):
        arr[k].sv_pos[:] = [float(x) for x in o["sv_pos"]]
        arr[k].sv_vel[:] = [float(x) for x in o["sv_vel"]]
        for key in GNSS_OBS_KEYS:
            setattr(arr[k], key, o[key])
    return arr


def gnss_eval(lib, prefix, ctx, obs, iono, pose, speed_bias, rcv_dt, rcv_ddt, yaw_enu_local, anc_ecef, frame_dt, ddt_weight, want_J=True):
    """obs: list of dicts with sv_pos, sv_vel and GNSS_OBS_KEYS. pose [11][7], speed_bias [11][9] (the window state's blocks)."""
    n = len(obs)
    arr = gnss_obs_array(obs)
    st = State()
    p, sb = _f64(pose).reshape(NFRAMES, 7), _f64(speed_bias).reshape(NFRAMES, 9)
    for i in range(NFRAMES):
        st.para_Pose[i][:] = p[i].tolist()
        st.para_SpeedBias[i][:] = sb[i].tolist()
    g = GnssState()
    rd = _f64(rcv_dt).reshape(NFRAMES, 4)
    for i in range(NFRAMES):
        g.rcv_dt[i][:] = rd[i].tolist()
    g.rcv_ddt[:] = _f64(rcv_ddt).tolist()
    g.yaw_enu_local = float(yaw_enu_local)
    g.anc_ecef[:] = _f64(anc_ecef).tolist()
    fdt = _f64(frame_dt)
    assert fdt.shape == (WINDOW_SIZE,)
    io = _f64(iono) if iono is not None else None
    r, J, rc_, rs, cost = np.zeros((n, 2)), np.zeros((n, 2, 18)), np.zeros((4, WINDOW_SIZE)), np.zeros(WINDOW_SIZE), np.zeros(1)
    f = getattr(bind(lib, prefix), prefix + "gnss_eval")
    rc = f(ctx, n, arr, _pd(io) if io is not None else None, C.byref(st), C.byref(g), _pd(fdt), float(ddt_weight), _pd(r),
           _pd(J) if want_J else None, _pd(rc_), _pd(rs), _pd(cost))
    if rc != OK:
        raise RuntimeError("%sgnss_eval failed with status %d" % (prefix, rc))
    return dict(r=r, J=J if want_J else None, r_dt_ddt=rc_, r_smooth=rs, cost=float(cost[0]))


# ---------------------------------------------------------------------------------------------
# Line landmarks (gfbe_line_eval / gfbe_line_refine)
# ---------------------------------------------------------------------------------------------
class LineWindow(C.Structure):
    _fields_ = [("struct_size", c_i), ("n_lines", c_i), ("start_frame", PI), ("n_obs", PI), ("obs", PD),
                ("is_triangulation", PU8), ("line_plucker", PD), ("pose", (c_d * 7) * NFRAMES), ("ex_cam", c_d * 7)]


class LineWindowHolder:
    """A gfbe_line_window over the numpy arrays of a line-window dict (keys: start_frame, n_obs, obs [sum n_obs][4],
    is_triangulation, line_plucker [n][6], pose [11][7], ex_cam [7]); keeps the arrays alive."""

    def __init__(self, lw):
        self.sf, self.no = _i32(lw["start_frame"]), _i32(lw["n_obs"])
        self.obs, self.tri = _f64(lw["obs"]).reshape(-1, 4), _u8(lw["is_triangulation"])
        self.plk = _f64(lw["line_plucker"]).reshape(-1, 6)
        n = len(self.sf)
        assert len(self.no) == n and len(self.tri) == n and len(self.plk) == n and len(self.obs) == int(self.no.sum())
        self.c = LineWindow()
        self.c.struct_size, self.c.n_lines = C.sizeof(LineWindow), n
        self.c.start_frame, self.c.n_obs, self.c.obs = _pi(self.sf), _pi(self.no), _pd(self.obs)
        self.c.is_triangulation, self.c.line_plucker = self.tri.ctypes.data_as(PU8), _pd(self.plk)
        pose = _f64(lw["pose"]).reshape(NFRAMES, 7)
        for i in range(NFRAMES):
            self.c.pose[i][:] = pose[i].tolist()
        self.c.ex_cam[:] = _f64(lw["ex_cam"]).tolist()
        self.n = n


def line_eval(lib, prefix, ctx, pose, ex_cam, orth, obs, sqrt_info=400.0, robustify=True):
    pose, orth, obs, ex = _f64(pose).reshape(-1, 7), _f64(orth).reshape(-1, 4), _f64(obs).reshape(-1, 4), _f64(ex_cam)
    n = len(pose)
    assert len(orth) == n and len(obs) == n
    r, Jp, Je, Jo, cost = np.zeros((n, 2)), np.zeros((n, 2, 7)), np.zeros((n, 2, 7)), np.zeros((n, 2, 4)), np.zeros(1)
    f = getattr(bind(lib, prefix), prefix + "line_eval")
    rc = f(ctx, n, _pd(pose), _pd(ex), _pd(orth), _pd(obs), float(sqrt_info), int(bool(robustify)), _pd(r), _pd(Jp), _pd(Je), _pd(Jo), _pd(cost))
    if rc != OK:
        raise RuntimeError("%sline_eval failed with status %d" % (prefix, rc))
    return dict(r=r, J_pose=Jp, J_ex=Je, J_orth=Jo, cost=float(cost[0]))


def line_refine_raw(lib, prefix, ctx, holders, sqrt_info=400.0, cauchy_scale=1.0, max_num_iterations=8, plucker_out=None, keep_out=None,
                    summary=None):
    """gfbe_line_refine over prebuilt LineWindowHolders; returns (status, plucker_out, keep_out, summary array). The output buffers
    may be passed in (a failed call must leave them untouched)."""
    n_lines = sum(h.n for h in holders)
    arr = (C.POINTER(LineWindow) * max(len(holders), 1))(*[C.pointer(h.c) for h in holders])
    plk = np.zeros((n_lines, 6)) if plucker_out is None else plucker_out
    keep = np.zeros(n_lines, np.uint8) if keep_out is None else keep_out
    sums = (Summary * max(len(holders), 1))() if summary is None else summary
    f = getattr(bind(lib, prefix), prefix + "line_refine")
    rc = f(ctx, len(holders), arr, float(sqrt_info), float(cauchy_scale), int(max_num_iterations), _pd(plk), keep.ctypes.data_as(PU8), sums)
    return rc, plk, keep, sums


def line_refine(lib, prefix, ctx, windows, sqrt_info=400.0, cauchy_scale=1.0, max_num_iterations=8):
    """Batched onlyLineOpt + removeLineOutlier. windows: line-window dicts. Returns one dict per window: plucker [n][6], keep [n] (bool),
    summary (summary_to_dict), and the call's status."""
    holders = [w if isinstance(w, LineWindowHolder) else LineWindowHolder(w) for w in windows]
    rc, plk, keep, sums = line_refine_raw(lib, prefix, ctx, holders, sqrt_info, cauchy_scale, max_num_iterations)
    if rc not in (OK, NO_CONVERGENCE, NUMERICAL_FAILURE):
        raise RuntimeError("%sline_refine failed with status %d" % (prefix, rc))
    out, o = [], 0
    for k, h in enumerate(holders):
        out.append(dict(plucker=plk[o:o + h.n].copy(), keep=keep[o:o + h.n].astype(bool), summary=summary_to_dict(sums[k]),
                        perf=summary_perf(sums[k]), status=rc))
        o += h.n
    return out


# ---------------------------------------------------------------------------------------------
# Reduced normal equations of the line factors (gfbe_line_reduce / gfbe_ltab_reduce)
# ---------------------------------------------------------------------------------------------
LINE_REDUCE_SOLVE, LINE_REDUCE_MARG_OLD, LINE_REDUCE_DIM = 0, 1, 72


class LineReduced(C.Structure):
    _fields_ = [("struct_size", c_i), ("reserved", c_i), ("H", PD), ("g", PD), ("U", PD), ("bp", PD), ("cost", PD), ("n_eligible", PI),
                ("n_failed", PI), ("Vinv", PD), ("bl", PD), ("W", PD), ("failed", PU8), ("ms_kernel", PD)]


LINE_REDUCE_KEYS = ("H", "g", "U", "bp", "cost", "n_eligible", "n_failed", "Vinv", "bl", "W", "failed", "ms_kernel")


def line_reduced_buffers(n_windows, n_lines, want=LINE_REDUCE_KEYS, fill=0):
    """Output arrays of a reduce call over n_windows windows with n_lines lines in all (the bound of the eligible ones)."""
    D, W = LINE_REDUCE_DIM, n_windows
    shapes = dict(H=((W, D, D), np.float64), g=((W, D), np.float64), U=((W, D, D), np.float64), bp=((W, D), np.float64),
                  cost=((W,), np.float64), n_eligible=((W,), np.int32), n_failed=((W,), np.int32), Vinv=((n_lines, 4, 4), np.float64),
                  bl=((n_lines, 4), np.float64), W=((n_lines, D, 4), np.float64), failed=((n_lines,), np.uint8),
                  ms_kernel=((W, 2), np.float64))
    return {k: np.full(shapes[k][0], fill, shapes[k][1]) for k in want}


def line_reduced_struct(bufs):
    """A gfbe_line_reduced over the arrays of `bufs` (absent keys: NULL). Keep `bufs` alive during the call."""
    r = LineReduced()
    r.struct_size = C.sizeof(LineReduced)
    for k, a in bufs.items():
        assert a.flags["C_CONTIGUOUS"]
        setattr(r, k, a.ctypes.data_as(dict(LineReduced._fields_)[k]))
    return r


def _line_reduced_split(bufs):
    """Per-window views of a reduce call's outputs; the per-line records are cut at the windows' n_eligible."""
    ne = bufs["n_eligible"]
    off = np.concatenate([[0], np.cumsum(ne)]).astype(int)
    out = []
    for w in range(len(ne)):
        d = {}
        for k, a in bufs.items():
            d[k] = a[off[w]:off[w + 1]] if k in ("Vinv", "bl", "W", "failed") else a[w]
        out.append(d)
    return out


def line_reduce_raw(lib, prefix, ctx, holders, mode, sqrt_info, huber_width, mu, red):
    """gfbe_line_reduce over prebuilt LineWindowHolders into the LineReduced `red`; returns the status."""
    arr = (C.POINTER(LineWindow) * max(len(holders), 1))(*[C.pointer(h.c) for h in holders])
    f = getattr(bind(lib, prefix), prefix + "line_reduce")
    return f(ctx, len(holders), arr, int(mode), float(sqrt_info), float(huber_width), float(mu), _reduced_ptr(red))


def line_reduce(lib, prefix, ctx, windows, mode=LINE_REDUCE_SOLVE, sqrt_info=400.0, huber_width=1.0, mu=0.0, want=LINE_REDUCE_KEYS):
    """Reduced normal equations of the line factors of each window (line-window dicts or LineWindowHolders). One dict per window:
    H [72][72], g, U, bp, cost, n_eligible, n_failed, and the records Vinv, bl, W, failed of its eligible lines."""
    holders = [w if isinstance(w, LineWindowHolder) else LineWindowHolder(w) for w in windows]
    want = tuple(want) + tuple(k for k in ("n_eligible",) if k not in want)
    bufs = line_reduced_buffers(len(holders), sum(h.n for h in holders), want)
    rc = line_reduce_raw(lib, prefix, ctx, holders, mode, sqrt_info, huber_width, mu, line_reduced_struct(bufs))
    if rc != OK:
        raise RuntimeError("%sline_reduce failed with status %d" % (prefix, rc))
    return _line_reduced_split(bufs)


# ---------------------------------------------------------------------------------------------
# The step half of a joint iteration over the line blocks (gfbe_line_step / gfbe_ltab_step / gfbe_ltab_commit)
# ---------------------------------------------------------------------------------------------
class LineReducedV(C.Structure):
    """gfbe_line_reduced at its current size: LineReduced (the size before the member V, still admitted by the library) plus V."""
    _fields_ = LineReduced._fields_ + [("V", PD)]


def _reduced_ptr(red):
    """`red` (LineReduced or LineReducedV, told apart by struct_size: the library admits both; None: NULL) as the gfbe_line_reduced *
    of the signatures."""
    return C.cast(C.byref(red), C.POINTER(LineReducedV)) if red is not None else None


LINE_RECORD_KEYS = ("Vinv", "bl", "W", "V", "failed")
LINE_REDUCE_KEYS_V = LINE_REDUCE_KEYS + ("V",)


def line_reduced_buffers_v(n_windows, n_lines, want=LINE_REDUCE_KEYS_V, fill=0):
    """line_reduced_buffers with the record V [n_lines][10] (lower triangle of V_l, row-major)."""
    bufs = line_reduced_buffers(n_windows, n_lines, tuple(k for k in want if k != "V"), fill)
    if "V" in want:
        bufs["V"] = np.full((n_lines, 10), fill, np.float64)
    return bufs


def line_reduced_struct_v(bufs):
    """A gfbe_line_reduced (current size) over the arrays of `bufs` (absent keys: NULL). Keep `bufs` alive during the call."""
    r = LineReducedV()
    r.struct_size = C.sizeof(LineReducedV)
    for k, a in bufs.items():
        assert a.flags["C_CONTIGUOUS"]
        setattr(r, k, a.ctypes.data_as(dict(LineReducedV._fields_)[k]))
    return r


def _line_split(bufs, ne, per_line):
    off = np.concatenate([[0], np.cumsum(ne)]).astype(int)
    return [{k: (a[off[w]:off[w + 1]] if k in per_line else a[w]) for k, a in bufs.items()} for w in range(len(ne))]


def line_reduce_v(lib, prefix, ctx, windows, mode=LINE_REDUCE_SOLVE, sqrt_info=400.0, huber_width=1.0, mu=0.0, want=LINE_REDUCE_KEYS_V):
    """line_reduce through the current structure: the same outputs plus the record V."""
    holders = [w if isinstance(w, LineWindowHolder) else LineWindowHolder(w) for w in windows]
    want = tuple(want) + tuple(k for k in ("n_eligible",) if k not in want)
    bufs = line_reduced_buffers_v(len(holders), sum(h.n for h in holders), want)
    rc = line_reduce_raw(lib, prefix, ctx, holders, mode, sqrt_info, huber_width, mu, line_reduced_struct_v(bufs))
    if rc != OK:
        raise RuntimeError("%sline_reduce failed with status %d" % (prefix, rc))
    return _line_split(bufs, bufs["n_eligible"], LINE_RECORD_KEYS)


class LineStepped(C.Structure):
    _fields_ = [("struct_size", c_i), ("reserved", c_i), ("gram", PD), ("total", PD), ("coef", PD), ("invalid", PU8), ("y_l", PD),
                ("v_l", PD), ("orth_cand", PD), ("plucker_cand", PD), ("pose_cand", PD), ("ex_cand", PD), ("cost_cand", PD), ("ms_kernel", PD)]


LINE_STEP_KEYS = ("gram", "total", "coef", "invalid", "y_l", "v_l", "orth_cand", "plucker_cand", "pose_cand", "ex_cand", "cost_cand", "ms_kernel")
LINE_STEP_PER_LINE = ("y_l", "v_l", "orth_cand", "plucker_cand")


def line_stepped_buffers(n_windows, n_lines, want=LINE_STEP_KEYS, fill=0):
    """Output arrays of a step call over n_windows windows with n_lines entering lines in all (or a bound of them)."""
    W = n_windows
    shapes = dict(gram=((W, 8), np.float64), total=((W, 8), np.float64), coef=((W, 4), np.float64), invalid=((W,), np.uint8),
                  y_l=((n_lines, 4), np.float64), v_l=((n_lines, 4), np.float64), orth_cand=((n_lines, 4), np.float64),
                  plucker_cand=((n_lines, 6), np.float64), pose_cand=((W, NFRAMES, 7), np.float64), ex_cand=((W, 7), np.float64),
                  cost_cand=((W,), np.float64), ms_kernel=((W,), np.float64))
    return {k: np.full(shapes[k][0], fill, shapes[k][1]) for k in want}


def line_stepped_struct(bufs):
    r = LineStepped()
    r.struct_size = C.sizeof(LineStepped)
    for k, a in bufs.items():
        assert a.flags["C_CONTIGUOUS"]
        setattr(r, k, a.ctypes.data_as(dict(LineStepped._fields_)[k]))
    return r


def line_step_raw(lib, prefix, ctx, holders, red, sqrt_info, huber_width, mu, y_p, v_p, rest, radius, stepped):
    """gfbe_line_step over prebuilt LineWindowHolders; red: LineReducedV over the records (or None), stepped: LineStepped (or None);
    y_p, v_p [W][72], rest [W][8], radius [W] float64 contiguous. Returns the status."""
    arr = (C.POINTER(LineWindow) * max(len(holders), 1))(*[C.pointer(h.c) for h in holders])
    f = getattr(bind(lib, prefix), prefix + "line_step")
    return f(ctx, len(holders), arr, _reduced_ptr(red), float(sqrt_info), float(huber_width), float(mu),
             _pd(y_p), _pd(v_p), _pd(rest), _pd(radius), C.byref(stepped) if stepped is not None else None)


def line_records_pack(records):
    """The record arrays of gfbe_line_step, concatenated over the windows: records = one dict per window with Vinv, bl, W, V, failed."""
    ne = np.array([len(r["failed"]) for r in records], np.int32)
    shapes = dict(Vinv=(4, 4), bl=(4,), W=(LINE_REDUCE_DIM, 4), V=(10,))
    rb = dict(n_eligible=ne if len(ne) else np.zeros(1, np.int32))
    for k, sh in shapes.items():
        parts = [_f64(r[k]).reshape((-1,) + sh) for r in records]
        a = np.concatenate(parts) if parts else np.zeros((0,) + sh)
        rb[k] = np.ascontiguousarray(a if len(a) else np.zeros((1,) + sh))
    f = np.concatenate([_u8(r["failed"]) for r in records]) if len(records) else np.zeros(0, np.uint8)
    rb["failed"] = np.ascontiguousarray(f if len(f) else np.zeros(1, np.uint8))
    return rb, ne


def line_step(lib, prefix, ctx, windows, records, y_p, v_p, rest, radius, sqrt_info=400.0, huber_width=1.0, mu=0.0, want=LINE_STEP_KEYS):
    """The step half for each window. records: one dict per window with Vinv, bl, W, V, failed of its entering lines (what line_reduce_v
    returned). One dict per window: gram, total, coef, invalid, y_l, v_l, orth_cand, plucker_cand, pose_cand, ex_cand, cost_cand."""
    holders = [w if isinstance(w, LineWindowHolder) else LineWindowHolder(w) for w in windows]
    nW = len(holders)
    rb, ne = line_records_pack(records)
    bufs = line_stepped_buffers(nW, max(int(ne.sum()), 1), want)
    rc = line_step_raw(lib, prefix, ctx, holders, line_reduced_struct_v(rb), sqrt_info, huber_width, mu, _f64(y_p).reshape(nW, LINE_REDUCE_DIM),
                       _f64(v_p).reshape(nW, LINE_REDUCE_DIM), _f64(rest).reshape(nW, 8), _f64(radius).reshape(nW), line_stepped_struct(bufs))
    if rc != OK:
        raise RuntimeError("%sline_step failed with status %d" % (prefix, rc))
    return _line_split(bufs, ne, LINE_STEP_PER_LINE)


# ---------------------------------------------------------------------------------------------
# Line feature tables (gfbe_ltab_*): FeatureManager::linefeature on the device
# ---------------------------------------------------------------------------------------------
class LineTables(Handle):
    """W device-resident line tables behind `lib` (prefix gfbe_, ctx = gfbe_ctx*). Per-table arguments are lists of length W."""
    family = "ltab_"

    def __init__(self, lib, prefix, ctx, n_tables=1, capacity=1024):
        Handle.__init__(self, lib, prefix, ctx)
        self.W, self.cap = n_tables, capacity
        self._check(self._f("create")(self.ctx, int(n_tables), int(capacity), C.byref(self.h)), "create")

    def add_frame(self, frame_count, ids, obs4):
        """ids[w]: ascending line ids; obs4[w]: [n, 4]. Returns counters [W, 2] = [tracked, new]."""
        off, lid = FeatureTables._ragged(ids, np.int32)
        ob = np.ascontiguousarray(np.concatenate([np.asarray(r, np.float64).reshape(-1, 4) for r in obs4]))      # (a table may receive no line)
        assert len(ob) == len(lid)
        fc, cnt = _i32(frame_count), np.zeros((self.W, 2), np.int32)
        self._check(self._f("add_frame")(self.ctx, self.h, _pi(fc), _pi(off), _pi(lid), _pd(ob), _pi(cnt)), "add_frame")
        return cnt

    def triangulate(self, poses, tic_ric):
        p, e = _f64(poses).reshape(self.W, 11 * 12), _f64(tic_ric).reshape(self.W, 12)
        self._check(self._f("triangulate")(self.ctx, self.h, _pd(p), _pd(e)), "triangulate")

    def remove_back_shift(self, marg_pr, new_pr):
        a, b = _f64(marg_pr).reshape(self.W, 12), _f64(new_pr).reshape(self.W, 12)
        self._check(self._f("remove_back_shift")(self.ctx, self.h, _pd(a), _pd(b)), "remove_back_shift")

    def remove_back(self):
        self._check(self._f("remove_back")(self.ctx, self.h), "remove_back")

    def remove_front(self, frame_count):
        fc = _i32(frame_count)
        self._check(self._f("remove_front")(self.ctx, self.h, _pi(fc)), "remove_front")

    def refine_raw(self, pose7, ex_cam, sqrt_info=400.0, cauchy_scale=1.0, max_num_iterations=8, sums=None):
        """gfbe_ltab_refine on prepared arrays (pose7 [W][11][7], ex_cam [W][7], float64, contiguous): (status, Summary array)."""
        sums = (Summary * self.W)() if sums is None else sums
        rc = self._f("refine")(self.ctx, self.h, _pd(pose7), _pd(ex_cam), float(sqrt_info), float(cauchy_scale), int(max_num_iterations), sums)
        return rc, sums

    def refine(self, pose7, ex_cam, sqrt_info=400.0, cauchy_scale=1.0, max_num_iterations=8):
        """onlyLineOpt + removeLineOutlier on every table, in place. Returns one dict per table: summary, perf, status."""
        p, e = _f64(pose7).reshape(self.W, NFRAMES, 7), _f64(ex_cam).reshape(self.W, 7)
        rc, sums = self.refine_raw(p, e, sqrt_info, cauchy_scale, max_num_iterations)
        if rc not in (OK, NO_CONVERGENCE, NUMERICAL_FAILURE):
            raise RuntimeError("%sltab_refine failed with status %d" % (self.prefix, rc))
        return [dict(summary=summary_to_dict(sums[w]), perf=summary_perf(sums[w]), status=rc) for w in range(self.W)]

    def reduce_raw(self, pose7, ex_cam, mode, sqrt_info, huber_width, mu, red):
        """gfbe_ltab_reduce on prepared arrays (pose7 [W][11][7], ex_cam [W][7], float64, contiguous) into the LineReduced `red`."""
        return self._f("reduce")(self.ctx, self.h, int(mode), _pd(pose7), _pd(ex_cam), float(sqrt_info), float(huber_width), float(mu),
                                 _reduced_ptr(red))      # (LineReduced or LineReducedV: both sizes are admitted)

    def reduce(self, pose7, ex_cam, mode=LINE_REDUCE_SOLVE, sqrt_info=400.0, huber_width=1.0, mu=0.0, want=LINE_REDUCE_KEYS):
        """Reduced normal equations of the line factors of every table, read in place (abi.line_reduce's result per table)."""
        p, e = _f64(pose7).reshape(self.W, NFRAMES, 7), _f64(ex_cam).reshape(self.W, 7)
        want = tuple(want) + tuple(k for k in ("n_eligible",) if k not in want)
        bufs = line_reduced_buffers(self.W, int(self.size().sum()), want)
        rc = self.reduce_raw(p, e, mode, sqrt_info, huber_width, mu, line_reduced_struct(bufs))
        if rc != OK:
            raise RuntimeError("%sltab_reduce failed with status %d" % (self.prefix, rc))
        return _line_reduced_split(bufs)

    def size(self):
        n = np.zeros(self.W, np.int32)
        self._check(self._f("size")(self.ctx, self.h, _pi(n)), "size")
        return n

    def reduce_v(self, pose7, ex_cam, mode=LINE_REDUCE_SOLVE, sqrt_info=400.0, huber_width=1.0, mu=0.0, want=LINE_REDUCE_KEYS_V):
        """reduce() through the current structure: the same outputs plus the record V."""
        p, e = _f64(pose7).reshape(self.W, NFRAMES, 7), _f64(ex_cam).reshape(self.W, 7)
        want = tuple(want) + tuple(k for k in ("n_eligible",) if k not in want)
        bufs = line_reduced_buffers_v(self.W, int(self.size().sum()), want)
        rc = self.reduce_raw(p, e, mode, sqrt_info, huber_width, mu, line_reduced_struct_v(bufs))
        if rc != OK:
            raise RuntimeError("%sltab_reduce failed with status %d" % (self.prefix, rc))
        return _line_split(bufs, bufs["n_eligible"], LINE_RECORD_KEYS)

    def keep_records(self, on=True):
        """gfbe_ltab_keep_records: while on, a solve-mode reduce leaves its per-line records on the handle for step()."""
        self._check(self._f("keep_records")(self.ctx, self.h, int(bool(on))), "keep_records")

    def step_raw(self, pose7, ex_cam, sqrt_info, huber_width, y_p, v_p, rest, radius, stepped):
        """gfbe_ltab_step on prepared arrays (float64, contiguous) into the LineStepped `stepped`; returns the status."""
        return self._f("step")(self.ctx, self.h, _pd(pose7), _pd(ex_cam), float(sqrt_info), float(huber_width), _pd(y_p), _pd(v_p), _pd(rest),
                               _pd(radius), C.byref(stepped) if stepped is not None else None)

    def step(self, pose7, ex_cam, y_p, v_p, rest, radius, n_eligible, sqrt_info=400.0, huber_width=1.0, want=LINE_STEP_KEYS):
        """The step half on every table from the records the last solve-mode reduce kept (abi.line_step's result per table).
        n_eligible [W]: the entering lines per table, as that reduce reported them (they cut the per-line arrays)."""
        p, e = _f64(pose7).reshape(self.W, NFRAMES, 7), _f64(ex_cam).reshape(self.W, 7)
        ne = _i32(n_eligible).reshape(self.W)
        bufs = line_stepped_buffers(self.W, max(int(ne.sum()), 1), want)
        rc = self.step_raw(p, e, sqrt_info, huber_width, _f64(y_p).reshape(self.W, LINE_REDUCE_DIM), _f64(v_p).reshape(self.W, LINE_REDUCE_DIM),
                           _f64(rest).reshape(self.W, 8), _f64(radius).reshape(self.W), line_stepped_struct(bufs))
        if rc != OK:
            raise RuntimeError("%sltab_step failed with status %d" % (self.prefix, rc))
        return _line_split(bufs, ne, LINE_STEP_PER_LINE)

    def commit(self, accept):
        """gfbe_ltab_commit: tables with accept[w] != 0 take the candidate lines of the last step()."""
        a = _u8(accept).reshape(self.W)
        self._check(self._f("commit")(self.ctx, self.h, a.ctypes.data_as(PU8)), "commit")

    def line_count(self):
        n = np.zeros(self.W, np.int32)
        self._check(self._f("line_count")(self.ctx, self.h, _pi(n)), "line_count")
        return n

    def download(self, w=0):
        n = int(self.size()[w])
        out = dict(line_id=np.zeros(n, np.int32), start_frame=np.zeros(n, np.int32), n_obs=np.zeros(n, np.int32),
                   obs4=np.zeros((n, NFRAMES, 4)), is_triangulation=np.zeros(n, np.uint8), line_plucker=np.zeros((n, 6)))
        self._check(self._f("download")(self.ctx, self.h, int(w), _pi(out["line_id"]), _pi(out["start_frame"]), _pi(out["n_obs"]),
                                        _pd(out["obs4"]), out["is_triangulation"].ctypes.data_as(PU8), _pd(out["line_plucker"])), "download")
        return out

    def upload(self, w, tab):
        """Replaces table w by `tab` (the dict download() returns)."""
        lid, sf, no = _i32(tab["line_id"]), _i32(tab["start_frame"]), _i32(tab["n_obs"])
        ob, tri, plk = _f64(tab["obs4"]).reshape(-1, NFRAMES, 4), _u8(tab["is_triangulation"]), _f64(tab["line_plucker"]).reshape(-1, 6)
        n = len(lid)
        assert len(sf) == n and len(no) == n and len(ob) == n and len(tri) == n and len(plk) == n
        self._check(self._f("upload")(self.ctx, self.h, int(w), n, _pi(lid), _pi(sf), _pi(no), _pd(ob), tri.ctypes.data_as(PU8), _pd(plk)), "upload")


def ltab_to_line_window(tab, pose7, ex_cam):
    """LineTables.download() -> the line-window dict LineWindowHolder / gfbe_line_refine take (observations packed in line order)."""
    no = np.asarray(tab["n_obs"])
    obs = np.concatenate([tab["obs4"][i, :no[i]] for i in range(len(no))]) if len(no) else np.zeros((0, 4))
    return dict(start_frame=tab["start_frame"], n_obs=tab["n_obs"], obs=obs.reshape(-1, 4), is_triangulation=tab["is_triangulation"],
                line_plucker=tab["line_plucker"], pose=np.asarray(pose7, float).reshape(NFRAMES, 7), ex_cam=np.asarray(ex_cam, float))


# ---------------------------------------------------------------------------------------------
# Voxel map of the LiDAR odometry (gfbe_vmap_*): map_incremental, lasermap_fov_segment, the association of addSurfCostFactor
# ---------------------------------------------------------------------------------------------
class VmapOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("max_num_points_in_voxel", c_i), ("voxel_neighborhood", c_i), ("max_number_neighbors", c_i),
                ("min_number_neighbors", c_i), ("threshold_voxel_occupancy", c_i), ("num_closest_neighbors", c_i), ("max_num_residuals", c_i),
                ("size_voxel_map", c_d), ("min_distance_points", c_d), ("max_distance", c_d), ("max_dist_to_plane_icp", c_d),
                ("power_planarity", c_d), ("weight_alpha", c_d), ("weight_neighborhood", c_d)]


def vmap_default_options(lib, prefix="gfbe_"):
    return options_struct(lib, prefix, "vmap_", VmapOptions)


class VregOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("max_num_iteration", c_i), ("lm_max_num_iterations", c_i), ("min_num_residuals", c_i),
                ("laser_point_cov", c_d), ("huber_delta", c_d), ("beta_location_consistency", c_d), ("beta_orientation_consistency", c_d),
                ("beta_small_velocity", c_d), ("thres_translation_norm", c_d), ("thres_orientation_norm", c_d)]


class VregSummary(C.Structure):
    _fields_ = [("outer_iterations", c_i), ("converged", c_i), ("too_few_residuals", c_i), ("no_residuals", c_i), ("degenerate", c_i),
                ("sv", c_d * 3), ("n_res", c_i * 32), ("lm_iterations", c_i * 32), ("lm_accepted", c_i * 32), ("lm_termination", c_i * 32),
                ("cost_initial", c_d * 32), ("cost_final", c_d * 32), ("diff_trans", c_d * 32), ("diff_rot", c_d * 32), ("pose_trace", (c_d * 14) * 32)]


def vreg_default_options(lib, prefix="gfbe_"):
    return options_struct(lib, prefix, "vreg_", VregOptions)


def vreg_summary_to_dict(sm):
    d = dict(outer_iterations=sm.outer_iterations, converged=sm.converged, too_few_residuals=sm.too_few_residuals, no_residuals=sm.no_residuals,
             degenerate=sm.degenerate, sv=np.array(sm.sv[:]))
    for k in ("n_res", "lm_iterations", "lm_accepted", "lm_termination"):
        d[k] = np.array(getattr(sm, k)[:], np.int32)
    for k in ("cost_initial", "cost_final", "diff_trans", "diff_rot"):
        d[k] = np.array(getattr(sm, k)[:])
    d["pose_trace"] = np.array([row[:] for row in sm.pose_trace])
    return d


class VoxelMap(Handle):
    """A device-resident voxel map behind `lib` (prefix gfbe_, ctx = gfbe_ctx*). options: fields of gfbe_vmap_options."""
    family = "vmap_"
    PI16 = C.POINTER(C.c_int16)

    def __init__(self, lib, prefix, ctx, voxel_capacity=1 << 16, **options):
        Handle.__init__(self, lib, prefix, ctx)
        self.cap = voxel_capacity
        self.opt = self._options(VmapOptions, options)
        self._check(self._f("create")(self.ctx, int(voxel_capacity), C.byref(self.opt), C.byref(self.h)), "create")

    def add_points(self, pts_world, min_num_points=0):
        p = _f64(pts_world).reshape(-1, 3)
        self._check(self._f("add_points")(self.ctx, self.h, len(p), _pd(p), int(min_num_points)), "add_points")

    def erase_far(self, location):
        loc = _f64(location).reshape(3)
        self._check(self._f("erase_far")(self.ctx, self.h, _pd(loc)), "erase_far")

    def size(self):
        """dict(n_voxels, n_points, n_skipped, overflow)."""
        v = (c_i * 4)()
        self._check(self._f("size")(self.ctx, self.h, *[C.cast(C.byref(v, 4 * k), PI) for k in range(4)]), "size")
        return dict(n_voxels=v[0], n_points=v[1], n_skipped=v[2], overflow=v[3])

    def download(self):
        """Voxels in ascending key order: dict(keys [nv, 3] int16, counts [nv], points [np, 3])."""
        sz = self.size()
        nv, npt = sz["n_voxels"], sz["n_points"]
        keys, counts, pts = np.zeros((nv, 3), np.int16), np.zeros(nv, np.int32), np.zeros((npt, 3))
        self._check(self._f("download")(self.ctx, self.h, keys.ctypes.data_as(self.PI16), _pi(counts), _pd(pts)), "download")
        return dict(keys=keys, counts=counts, points=pts)

    def upload(self, keys, counts, points):
        k, cn, p = np.ascontiguousarray(keys, np.int16).reshape(-1, 3), _i32(counts), _f64(points).reshape(-1, 3)
        assert len(k) == len(cn) and int(cn.sum()) == len(p)
        self._check(self._f("upload")(self.ctx, self.h, len(k), k.ctypes.data_as(self.PI16), _pi(cn), _pd(p)), "upload")

    def associate(self, ct, raw_pts, alpha, pose_begin, pose_end=None, frame_init=False):
        """The loop body of addSurfCostFactor for a scan: dict(n_res, src, pts, normals, offsets, alpha, weights, neighbor_count, a2D,
        neighbor_visit, n_nan). The rows also stay on the handle for linearize() / localizability()."""
        raw = _f64(raw_pts).reshape(-1, 3)
        n = len(raw)
        al = _f64(alpha if alpha is not None else np.zeros(n))
        pb = _f64(pose_begin)
        pe = _f64(pose_end if pose_end is not None else pose_begin)
        R = max(1, min(n * self.opt.num_closest_neighbors, self.opt.max_num_residuals))
        src, pts, nrm, off, alo, w = np.zeros(R, np.int32), np.zeros((R, 3)), np.zeros((R, 3)), np.zeros(R), np.zeros(R), np.zeros(R)
        cnt, a2d = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1))
        vis = np.full((max(n, 1), self.opt.max_number_neighbors), -1, np.int32)
        nres, nnan = c_i(0), c_i(0)
        self._check(self._f("associate")(self.ctx, self.h, int(ct), n, _pd(raw), _pd(al), _pd(pb), _pd(pe), int(bool(frame_init)), C.byref(nres),
                                         _pi(src), _pd(pts), _pd(nrm), _pd(off), _pd(alo), _pd(w), _pi(cnt), _pd(a2d), C.byref(nnan), _pi(vis)), "associate")
        r = nres.value
        return dict(n_res=r, src=src[:r], pts=pts[:r], normals=nrm[:r], offsets=off[:r], alpha=alo[:r], weights=w[:r],
                    neighbor_count=cnt[:n], a2D=a2d[:n], neighbor_visit=vis[:n], n_nan=nnan.value)

    def linearize_raw(self, ct, sqrt_info, pose_begin, pose_end=None):
        """gfbe_vmap_linearize: (status, dict(H, g, cost)) on the rows held on the handle."""
        dn = 12 if ct else 6
        pb = _f64(pose_begin)
        pe = _f64(pose_end if pose_end is not None else pose_begin)
        H, g, cost = np.zeros((dn, dn)), np.zeros(dn), np.zeros(1)
        rc = self._f("linearize")(self.ctx, self.h, int(ct), float(sqrt_info), _pd(pb), _pd(pe), None, None, _pd(H), _pd(g), _pd(cost))
        return rc, dict(H=H, g=g, cost=float(cost[0]))

    def linearize(self, ct, sqrt_info, pose_begin, pose_end=None):
        rc, out = self.linearize_raw(ct, sqrt_info, pose_begin, pose_end)
        self._check(rc, "linearize")
        return out

    def localizability(self):
        """checkLocalizability on the held normals: (sv [3] descending, degenerate)."""
        sv, deg = np.zeros(3), c_i(0)
        self._check(self._f("localizability")(self.ctx, self.h, _pd(sv), C.byref(deg)), "localizability")
        return sv, bool(deg.value)

    def register_raw(self, ct, raw_pts, alpha, pose_begin, pose_end=None, prev_translation=None, prev_rotation=None, frame_init=False, **options):
        """gfbe_vmap_register: (status, pose_begin, pose_end, summary dict). options: fields of gfbe_vreg_options."""
        o = self._options(VregOptions, options, "vreg_")
        raw = _f64(raw_pts).reshape(-1, 3)
        n = len(raw)
        al = _f64(alpha if alpha is not None else np.zeros(n))
        pb = _f64(pose_begin)
        pe = _f64(pose_end if pose_end is not None else pose_begin)
        pt = _pd(_f64(prev_translation)) if prev_translation is not None else None
        pr = _pd(_f64(prev_rotation)) if prev_rotation is not None else None
        ob, oe, sm = np.full(7, np.nan), np.full(7, np.nan), VregSummary()
        rc = self._f("register")(self.ctx, self.h, C.byref(o), int(ct), n, _pd(raw), _pd(al), _pd(pb), _pd(pe), pt, pr, int(bool(frame_init)), _pd(ob), _pd(oe),
                                 C.byref(sm))
        return rc, ob, oe, vreg_summary_to_dict(sm)

    def register(self, ct, raw_pts, alpha, pose_begin, pose_end=None, prev_translation=None, prev_rotation=None, frame_init=False, **options):
        """One lidarodom::optimize on the device: (pose_begin, pose_end, summary dict); the last association stays on the handle."""
        rc, ob, oe, sm = self.register_raw(ct, raw_pts, alpha, pose_begin, pose_end, prev_translation, prev_rotation, frame_init, **options)
        self._check(rc, "register")
        return ob, oe, sm

    def add_scan(self, ct, raw_pts, alpha, pose_begin, pose_end=None, min_num_points=0, want_world=False):
        """transformKeypoints + map_incremental on the device; want_world: the world points [n, 3] (waits for them)."""
        raw = _f64(raw_pts).reshape(-1, 3)
        n = len(raw)
        al = _f64(alpha if alpha is not None else np.zeros(n))
        pb = _f64(pose_begin)
        pe = _f64(pose_end if pose_end is not None else pose_begin)
        out = np.zeros((n, 3)) if want_world else None
        self._check(self._f("add_scan")(self.ctx, self.h, int(ct), n, _pd(raw), _pd(al), _pd(pb), _pd(pe), int(min_num_points), _pd(out) if want_world else None), "add_scan")
        return out

    def register_scan_raw(self, ct, scan, pose_begin, pose_end=None, prev_translation=None, prev_rotation=None, frame_init=False, **options):
        """gfbe_vmap_register_scan on the KEYPOINTS of `scan` (abi.Scan): (status, pose_begin, pose_end, summary dict)."""
        o = self._options(VregOptions, options, "vreg_")
        pb = _f64(pose_begin)
        pe = _f64(pose_end if pose_end is not None else pose_begin)
        pt = _pd(_f64(prev_translation)) if prev_translation is not None else None
        pr = _pd(_f64(prev_rotation)) if prev_rotation is not None else None
        ob, oe, sm = np.full(7, np.nan), np.full(7, np.nan), VregSummary()
        rc = self._f("register_scan")(self.ctx, self.h, C.byref(o), int(ct), scan.h, _pd(pb), _pd(pe), pt, pr, int(bool(frame_init)), _pd(ob), _pd(oe), C.byref(sm))
        return rc, ob, oe, vreg_summary_to_dict(sm)

    def register_scan(self, ct, scan, pose_begin, pose_end=None, prev_translation=None, prev_rotation=None, frame_init=False, **options):
        rc, ob, oe, sm = self.register_scan_raw(ct, scan, pose_begin, pose_end, prev_translation, prev_rotation, frame_init, **options)
        self._check(rc, "register_scan")
        return ob, oe, sm

    def add_scan_handle_raw(self, ct, scan, pose_begin, pose_end=None, min_num_points=0):
        pb = _f64(pose_begin)
        pe = _f64(pose_end if pose_end is not None else pose_begin)
        return self._f("add_scan_handle")(self.ctx, self.h, int(ct), scan.h, _pd(pb), _pd(pe), int(min_num_points))

    def add_scan_handle(self, ct, scan, pose_begin, pose_end=None, min_num_points=0):
        """gfbe_vmap_add_scan on the POINTS of `scan` (abi.Scan); nothing crosses to the host."""
        self._check(self.add_scan_handle_raw(ct, scan, pose_begin, pose_end, min_num_points), "add_scan_handle")


# ---------------------------------------------------------------------------------------------
# A LiDAR scan held on the device (gfbe_scan_*): subSampleFrame, Undistort, transformPoint + gridSampling
# ---------------------------------------------------------------------------------------------
class Scan(Handle):
    """A device-resident scan behind `lib` (prefix gfbe_, ctx = gfbe_ctx*) of up to `capacity` points. The *_raw methods return the
    status; the others raise."""
    family = "scan_"

    def __init__(self, lib, prefix, ctx, capacity=1 << 16):
        Handle.__init__(self, lib, prefix, ctx)
        self.cap = capacity
        self._check(self._f("create")(self.ctx, int(capacity), C.byref(self.h)), "create")

    def upload_raw(self, raw_pts, alpha, timestamp=None, til=None):
        raw = _f64(raw_pts).reshape(-1, 3)
        n = len(raw)
        al = _f64(alpha if alpha is not None else np.zeros(n))
        ts = _f64(timestamp) if timestamp is not None else None
        tl = _f64(til) if til is not None else None
        assert len(al) == n and (ts is None or len(ts) == n)
        return self._f("upload")(self.ctx, self.h, n, _pd(raw), _pd(al), _pd(ts) if ts is not None else None, _pd(tl) if tl is not None else None)

    def upload(self, raw_pts, alpha, timestamp=None, til=None):
        self._check(self.upload_raw(raw_pts, alpha, timestamp, til), "upload")

    def subsample_raw(self, size_voxel):
        return self._f("subsample")(self.ctx, self.h, float(size_voxel))

    def subsample(self, size_voxel):
        self._check(self.subsample_raw(size_voxel), "subsample")

    def undistort_raw(self, state_time, state_pose):
        t, p = _f64(state_time), _f64(state_pose).reshape(-1, 7)
        assert len(t) == len(p)
        return self._f("undistort")(self.ctx, self.h, len(t), _pd(t), _pd(p))

    def undistort(self, state_time, state_pose):
        self._check(self.undistort_raw(state_time, state_pose), "undistort")

    def keypoints_raw(self, ct, pose_begin, pose_end, size_voxel):
        pb = _f64(pose_begin)
        pe = _f64(pose_end if pose_end is not None else pose_begin)
        n = c_i(-1)
        return self._f("keypoints")(self.ctx, self.h, int(ct), _pd(pb), _pd(pe), float(size_voxel), C.byref(n)), n.value

    def keypoints(self, ct, pose_begin, pose_end=None, size_voxel=0.2):
        """transformPoint + gridSampling at the poses; returns the keypoint count (waits)."""
        rc, n = self.keypoints_raw(ct, pose_begin, pose_end, size_voxel)
        self._check(rc, "keypoints")
        return n

    def size(self):
        """dict(n_points, n_keypoints, n_skipped)."""
        v = (c_i * 3)()
        self._check(self._f("size")(self.ctx, self.h, *[C.cast(C.byref(v, 4 * k), PI) for k in range(3)]), "size")
        return dict(n_points=v[0], n_keypoints=v[1], n_skipped=v[2])

    def download(self, which=0):
        """which 0: the points, 1: the keypoints: dict(src [n] index in the uploaded cloud, pts [n, 3], alpha [n], timestamp [n])."""
        sz = self.size()
        n = sz["n_keypoints"] if which else sz["n_points"]
        src, pts, al, ts = np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros(n), np.zeros(n)
        self._check(self._f("download")(self.ctx, self.h, int(which), _pi(src), _pd(pts), _pd(al), _pd(ts)), "download")
        return dict(src=src, pts=pts, alpha=al, timestamp=ts)


# ---------------------------------------------------------------------------------------------
# f3c: the dense RGB-D map of dense_map held on the device (gfbe_dmap_*; the model is tests/dmap_np.py)
# ---------------------------------------------------------------------------------------------
PF = C.POINTER(C.c_float)
DMAP_COUNTS = ("n_keyframes", "n_stored", "n_cloud", "n_voxels", "n_skipped", "n_gated", "n_refused", "n_fast")


class DmapOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("add_cap", c_i), ("rebuild_cap", c_i), ("filter_min_neighbors", c_i), ("resolution", c_d), ("origin", c_d),
                ("z_min", c_d), ("z_max", c_d), ("ex_cam", c_d * 7), ("filter_radius", c_d)]


def dmap_default_options(lib, prefix="gfbe_"):
    return options_struct(lib, prefix, "dmap_", DmapOptions)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class DenseMap(Handle):
    """The dense map behind `lib` (prefix gfbe_, ctx = gfbe_ctx*): addKeyFrame's capped insert, updatePath's rebuild and the radius
    filter of dense_map/src/pose_graph.cpp on up to `point_capacity` stored points of `keyframe_capacity` keyframes. options: fields
    of gfbe_dmap_options. The *_raw methods return the status; the others raise."""
    family = "dmap_"

    def __init__(self, lib, prefix, ctx, point_capacity=1 << 16, keyframe_capacity=1024, **options):
        Handle.__init__(self, lib, prefix, ctx)
        self.opt = self._options(DmapOptions, options)
        self._check(self._f("create")(self.ctx, int(point_capacity), int(keyframe_capacity), C.byref(self.opt), C.byref(self.h)), "create")

    def add_keyframe_raw(self, pose7, pts_cam, rgb):
        p, pts, col = _f64(pose7), _f32(pts_cam).reshape(-1, 3), _u8(rgb).reshape(-1, 3)
        assert len(p) == 7 and len(pts) == len(col)
        return self._f("add_keyframe")(self.ctx, self.h, _pd(p), len(pts), pts.ctypes.data_as(PF), col.ctypes.data_as(PU8))

    def add_keyframe(self, pose7, pts_cam, rgb):
        """addKeyFrame of one keyframe (returns without waiting for the device when the points fit a staging slot)."""
        self._check(self.add_keyframe_raw(pose7, pts_cam, rgb), "add_keyframe")

    def rebuild_raw(self, poses):
        p = _f64(poses).reshape(-1, 7)
        return self._f("rebuild")(self.ctx, self.h, len(p), _pd(p))

    def rebuild(self, poses):
        """updatePath's rebuild at the corrected poses [n_keyframes, 7] (returns without waiting)."""
        self._check(self.rebuild_raw(poses), "rebuild")

    def size(self):
        """dict of DMAP_COUNTS (waits)."""
        v = (c_i * len(DMAP_COUNTS))()
        self._check(self._f("size")(self.ctx, self.h, v), "size")
        return dict(zip(DMAP_COUNTS, list(v)))

    def filter(self, compact=True):
        """dict(keep [n_cloud] uint8, n_keep and, with compact, xyz [n_keep, 3] float32 / rgb [n_keep, 3] in cloud order)."""
        n = self.size()["n_cloud"]
        keep, nk = np.zeros(n, np.uint8), c_i(-1)
        xyz, rgb = (np.zeros((n, 3), np.float32), np.zeros((n, 3), np.uint8)) if compact else (None, None)
        self._check(self._f("filter")(self.ctx, self.h, keep.ctypes.data_as(PU8), C.byref(nk), xyz.ctypes.data_as(PF) if compact else None,
                                      rgb.ctypes.data_as(PU8) if compact else None), "filter")
        out = dict(keep=keep, n_keep=nk.value)
        if compact:
            out.update(xyz=xyz[:nk.value], rgb=rgb[:nk.value])
        return out

    def cloud(self):
        """dict(xyz [n, 3] float32 world, rgb [n, 3], kf [n], src [n] pool index) in insertion order."""
        n = self.size()["n_cloud"]
        xyz, rgb, kf, src = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._check(self._f("download_cloud")(self.ctx, self.h, xyz.ctypes.data_as(PF), rgb.ctypes.data_as(PU8), _pi(kf), _pi(src)), "download_cloud")
        return dict(xyz=xyz, rgb=rgb, kf=kf, src=src)

    def keyframe(self, k):
        """dict(pts [n, 3] float32 camera frame, rgb [n, 3]): keyframe k's list as it is now."""
        n = c_i(-1)
        self._check(self._f("download_keyframe")(self.ctx, self.h, int(k), C.byref(n), None, None), "download_keyframe")
        pts, rgb = np.zeros((n.value, 3), np.float32), np.zeros((n.value, 3), np.uint8)
        self._check(self._f("download_keyframe")(self.ctx, self.h, int(k), C.byref(n), pts.ctypes.data_as(PF), rgb.ctypes.data_as(PU8)), "download_keyframe")
        return dict(pts=pts, rgb=rgb)


# ---------------------------------------------------------------------------------------------
# f3d: the loop database of dense_map held on the device (gfbe_ldb_*; the model is tests/ldb_np.py)
# ---------------------------------------------------------------------------------------------
PU64 = C.POINTER(C.c_uint64)
LDB_COUNTS = ("n_keyframes", "n_descriptors", "n_bow", "n_refused")
LDB_MAX_CHILDREN, LDB_MAX_RESULTS, LDB_MAX_KEYFRAME_DESCRIPTORS = 256, 16, 4096


class LdbVocab(C.Structure):
    _fields_ = [("k", c_i), ("L", c_i), ("scoring", c_i), ("weighting", c_i), ("n_nodes", c_i), ("n_words", c_i), ("node_id", C.POINTER(c_i)),
                ("parent_id", C.POINTER(c_i)), ("weight", PD), ("descriptor", PU64), ("word_id", C.POINTER(c_i)), ("word_node", C.POINTER(c_i))]


class LdbOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("max_results", c_i), ("query_gap", c_i), ("min_loop_frame", c_i), ("max_keyframe_descriptors", c_i),
                ("match_start", c_i), ("match_max", c_i), ("reserved", c_i), ("score_first", c_d), ("score_other", c_d)]


def ldb_default_options(lib, prefix="gfbe_"):
    return options_struct(lib, prefix, "ldb_", LdbOptions)


def _u64(a, cols=4):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, cols)


class LdbVocabHolder:
    """gfbe_ldb_vocab over numpy arrays kept alive: dict(k, L, scoring, weighting, node_id, parent_id, weight, descriptor [n, 4] uint64,
    word_id, word_node) in the order of the vocabulary file."""

    def __init__(self, voc):
        self.node_id, self.parent_id = _i32(voc["node_id"]), _i32(voc["parent_id"])
        self.weight, self.descriptor = _f64(voc["weight"]), _u64(voc["descriptor"])
        self.word_id, self.word_node = _i32(voc["word_id"]), _i32(voc["word_node"])
        self.c = LdbVocab(int(voc["k"]), int(voc["L"]), int(voc.get("scoring", 0)), int(voc.get("weighting", 0)), len(self.node_id), len(self.word_id),
                          _pi(self.node_id), _pi(self.parent_id), _pd(self.weight), self.descriptor.ctypes.data_as(PU64), _pi(self.word_id), _pi(self.word_node))


class LoopDatabase(Handle):
    """The loop database behind `lib` (prefix gfbe_, ctx = gfbe_ctx*): detectLoop / addKeyFrameIntoVoc of dense_map/src/pose_graph.cpp and
    searchByBRIEFDes of keyframe.cpp over a vocabulary `voc` (LdbVocabHolder or its dict). options: fields of gfbe_ldb_options. The *_raw
    methods return the status; the others raise."""
    family = "ldb_"

    def __init__(self, lib, prefix, ctx, voc, keyframe_capacity=1024, descriptor_capacity=1 << 20, **options):
        Handle.__init__(self, lib, prefix, ctx)
        self.voc = voc if isinstance(voc, LdbVocabHolder) else LdbVocabHolder(voc)
        self.opt = self._options(LdbOptions, options)
        self._check(self._f("create")(self.ctx, C.byref(self.voc.c), int(keyframe_capacity), int(descriptor_capacity), C.byref(self.opt), C.byref(self.h)), "create")

    def transform(self, desc):
        """dict(word [n] the word of every descriptor, bow_word / bow_value the normalised BoW vector); no database change."""
        d = _u64(desc)
        word, nb, bw, bv = np.zeros(len(d), np.int32), c_i(-1), np.zeros(len(d), np.int32), np.zeros(len(d))
        self._check(self._f("transform")(self.ctx, self.h, len(d), d.ctypes.data_as(PU64), _pi(word), C.byref(nb), _pi(bw), _pd(bv)), "transform")
        return dict(word=word, bow_word=bw[:nb.value], bow_value=bv[:nb.value])

    def add_keyframe_raw(self, desc, pts, pts_norm, detect_loop=True):
        d, p, pn = _u64(desc), _f32(pts).reshape(-1, 2), _f32(pts_norm).reshape(-1, 2)
        assert len(d) == len(p) == len(pn)
        idx, loop, nr = c_i(-7), c_i(-7), c_i(-7)
        rid, rs = np.full(LDB_MAX_RESULTS, -7, np.int32), np.zeros(LDB_MAX_RESULTS)
        rc = self._f("add_keyframe")(self.ctx, self.h, len(d), d.ctypes.data_as(PU64), p.ctypes.data_as(PF), pn.ctypes.data_as(PF), int(bool(detect_loop)),
                                     C.byref(idx), C.byref(loop), C.byref(nr), _pi(rid), _pd(rs))
        n = max(nr.value, 0)
        return rc, dict(index=idx.value, loop_index=loop.value, result_id=rid[:n].copy(), result_score=rs[:n].copy())

    def add_keyframe(self, desc, pts, pts_norm, detect_loop=True):
        """detectLoop (detect_loop, waits for the results) or addKeyFrameIntoVoc of one keyframe: dict(index (-1: refused), loop_index,
        result_id, result_score)."""
        rc, out = self.add_keyframe_raw(desc, pts, pts_norm, detect_loop)
        self._check(rc, "add_keyframe")
        return out

    def match_raw(self, old_index, window_desc):
        w = _u64(window_desc)
        n = len(w)
        st, bi, bd, nm = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32), c_i(-7)
        src, pt, ptn = np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        rc = self._f("match")(self.ctx, self.h, int(old_index), n, w.ctypes.data_as(PU64), st.ctypes.data_as(PU8), _pi(bi), _pi(bd), C.byref(nm), _pi(src),
                              pt.ctypes.data_as(PF), ptn.ctypes.data_as(PF))
        m = max(nm.value, 0)
        return rc, dict(status=st, best_index=bi, best_dist=bd, n_matched=nm.value, matched_src=src[:m], matched_pt=pt[:m], matched_pt_norm=ptn[:m])

    def match(self, old_index, window_desc):
        """searchByBRIEFDes + reduceVector of the window descriptors against held keyframe old_index (waits)."""
        rc, out = self.match_raw(old_index, window_desc)
        self._check(rc, "match")
        return out

    def size(self):
        """dict of LDB_COUNTS (waits)."""
        v = (c_i * len(LDB_COUNTS))()
        self._check(self._f("size")(self.ctx, self.h, v), "size")
        return dict(zip(LDB_COUNTS, list(v)))

    def entry(self, e):
        """dict(bow_word, bow_value, desc [n, 4] uint64, pts, pts_norm [n, 2]) of entry e as it is held."""
        nb, nd = c_i(-1), c_i(-1)
        self._check(self._f("download_entry")(self.ctx, self.h, int(e), C.byref(nb), None, None, C.byref(nd), None, None, None), "download_entry")
        bw, bv = np.zeros(nb.value, np.int32), np.zeros(nb.value)
        d, p, pn = np.zeros((nd.value, 4), np.uint64), np.zeros((nd.value, 2), np.float32), np.zeros((nd.value, 2), np.float32)
        self._check(self._f("download_entry")(self.ctx, self.h, int(e), C.byref(nb), _pi(bw), _pd(bv), C.byref(nd), d.ctypes.data_as(PU64), p.ctypes.data_as(PF),
                                              pn.ctypes.data_as(PF)), "download_entry")
        return dict(bow_word=bw, bow_value=bv, desc=d, pts=p, pts_norm=pn)


# ---------------------------------------------------------------------------------------------
# the optical-flow tracker (gfbe_klt_* of include/gfbe_klt.h; the model is tests/klt_np.py, there is no oracle row)
# ---------------------------------------------------------------------------------------------
KLT_PREFIX = "gfbe_klt_"
KLT_WIN, KLT_MAX_LEVEL = 21, 7
KLT_COUNTERS = ("in", "forward", "reverse", "kept")
PI16 = C.POINTER(C.c_int16)


class KltOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("max_level", c_i), ("max_count", c_i), ("flow_back", c_i), ("border", c_i), ("grey_max", c_i),
                ("prediction_min_success", c_i), ("reserved", c_i), ("epsilon", c_d), ("min_eig_threshold", c_d), ("flow_back_dist", c_d)]


def klt_default_options(lib, **kw):
    return options_struct(lib, KLT_PREFIX, "", KltOptions, kw)


def _offsets(counts_or_lists):
    off = np.zeros(len(counts_or_lists) + 1, np.int32)
    off[1:] = np.cumsum([int(n) for n in counts_or_lists])
    return off


class Tracker(Handle):
    """The tracker behind `lib` (the product library, ctx = gfbe_ctx*) for n_cameras cameras of rows x cols uint8 images and up to
    point_capacity points a camera; see include/gfbe_klt.h. Per-camera arguments and results are lists of length n_cameras. options:
    fields of gfbe_klt_options. The *_raw methods return the status first; the others raise."""

    def __init__(self, lib, ctx, n_cameras, rows, cols, point_capacity=512, **options):
        Handle.__init__(self, lib, KLT_PREFIX, ctx)
        self.n_cameras, self.rows, self.cols, self.cap = int(n_cameras), int(rows), int(cols), int(point_capacity)
        self.opt = self._options(KltOptions, options)
        self._check(self._f("create")(self.ctx, self.n_cameras, self.rows, self.cols, self.cap, C.byref(self.opt), C.byref(self.h)), "create")
        self.held = [0] * self.n_cameras

    def push_image_raw(self, images):
        im = _u8(images)
        assert im.size == self.n_cameras * self.rows * self.cols, im.shape
        return self._f("push_image")(self.ctx, self.h, im.ctypes.data_as(PU8))

    def push_image(self, images):
        """images [n_cameras, rows, cols] uint8: the current set becomes the previous one (does not wait for the device)."""
        self._check(self.push_image_raw(images), "push_image")

    def set_points_raw(self, pts, ids, track_cnt):
        off = _offsets([len(p) for p in pts])
        cat = lambda xs, dt, shape: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(shape) for x in xs]) if len(xs) else np.zeros(shape, dt), dt)
        p, i_, t = cat(pts, np.float32, (-1, 2)), cat(ids, np.int32, (-1,)), cat(track_cnt, np.int32, (-1,))
        rc = self._f("set_points")(self.ctx, self.h, _pi(off), p.ctypes.data_as(PF), _pi(i_), _pi(t))
        if rc == OK:
            self.held = [int(n) for n in np.diff(off)]
        return rc

    def set_points(self, pts, ids, track_cnt):
        """The points of the current image, per camera: pts [n, 2] float32, ids [n], track_cnt [n]."""
        self._check(self.set_points_raw(pts, ids, track_cnt), "set_points")

    def track_raw(self, predict=None, fill=-7):
        """predict: None, or per camera None / [n, 2] predicted positions of the held points. Returns (status, per-camera list of
        dict(prev_pts, cur_pts, ids, track_cnt, counters)); the flat outputs start as `fill`."""
        n, C_ = sum(self.held), self.n_cameras
        has = np.zeros(C_, np.uint8)
        pp = np.zeros((n, 2), np.float32)
        if predict is not None:
            off = _offsets(self.held)
            for k, p in enumerate(predict):
                if p is not None:
                    has[k] = 1
                    pp[off[k]:off[k + 1]] = np.asarray(p, np.float32).reshape(-1, 2)
        off_out = np.full(C_ + 1, fill, np.int32)
        prev, cur = np.full((n, 2), fill, np.float32), np.full((n, 2), fill, np.float32)
        ids, cnt, counters = np.full(n, fill, np.int32), np.full(n, fill, np.int32), np.full((C_, 4), fill, np.int32)
        rc = self._f("track")(self.ctx, self.h, has.ctypes.data_as(PU8) if predict is not None else None, pp.ctypes.data_as(PF) if predict is not None else None,
                              _pi(off_out), prev.ctypes.data_as(PF), cur.ctypes.data_as(PF), _pi(ids), _pi(cnt), _pi(counters))
        raw = dict(offset=off_out, prev_pts=prev, cur_pts=cur, ids=ids, track_cnt=cnt, counters=counters)
        if rc != OK:
            return rc, raw
        self.held = [int(x) for x in np.diff(off_out)]
        out = []
        for k in range(C_):
            a, b = off_out[k], off_out[k + 1]
            out.append(dict(prev_pts=prev[a:b].copy(), cur_pts=cur[a:b].copy(), ids=ids[a:b].copy(), track_cnt=cnt[a:b].copy(),
                            counters=dict(zip(KLT_COUNTERS, counters[k].tolist()))))
        return rc, out

    def track(self, predict=None):
        """The tracking half of trackImage for every camera (one wait); the survivors become the held points."""
        rc, out = self.track_raw(predict)
        self._check(rc, "track")
        return out

    def flow_raw(self, pts, direction=0, max_level=3, next_pts=None, fill=-7):
        """calcOpticalFlowPyrLK on explicit per-camera points; next_pts: the per-camera initial flow (OPTFLOW_USE_INITIAL_FLOW) or None."""
        off = _offsets([len(p) for p in pts])
        n = int(off[-1])
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 2) for x in xs]) if len(xs) else np.zeros((0, 2)), np.float32)
        p = cat(pts)
        nx = cat(next_pts) if next_pts is not None else np.full((n, 2), fill, np.float32)
        st, err = np.full(n, fill % 256, np.uint8), np.full(n, fill, np.float32)
        rc = self._f("flow")(self.ctx, self.h, int(direction), int(max_level), int(next_pts is not None), _pi(off), p.ctypes.data_as(PF), nx.ctypes.data_as(PF),
                             st.ctypes.data_as(PU8), err.ctypes.data_as(PF))
        return rc, [dict(next_pts=nx[a:b], status=st[a:b], err=err[a:b]) for a, b in zip(off[:-1], off[1:])]

    def flow(self, *a, **kw):
        rc, out = self.flow_raw(*a, **kw)
        self._check(rc, "flow")
        return out

    def level(self, which, camera, level):
        """dict(image [(h + 42), (w + 42)] uint8, deriv [(h + 42), (w + 42), 2] int16, w, h, n_levels) of a level of set `which`
        (0: previous, 1: current) as the device holds it."""
        dims = np.zeros(4, np.int32)
        self._check(self._f("download_level")(self.ctx, self.h, int(which), int(camera), int(level), None, None, _pi(dims)), "download_level")
        w, h = int(dims[0]), int(dims[1])
        im, de = np.zeros((h + 2 * KLT_WIN, w + 2 * KLT_WIN), np.uint8), np.zeros((h + 2 * KLT_WIN, w + 2 * KLT_WIN, 2), np.int16)
        self._check(self._f("download_level")(self.ctx, self.h, int(which), int(camera), int(level), im.ctypes.data_as(PU8), de.ctypes.data_as(PI16), _pi(dims)),
                    "download_level")
        return dict(image=im, deriv=de, w=w, h=h, n_levels=int(dims[3]))


# ---------------------------------------------------------------------------------------------
# corner detection behind the tracker (gfbe_det_* of include/gfbe_det.h; the model is tests/det_np.py, there is no oracle row)
# ---------------------------------------------------------------------------------------------
DET_PREFIX = "gfbe_det_"
DET_MAX_POINTS = 2048
DET_COUNTERS = ("in", "kept", "candidates", "added", "next_id", "overflow")


class DetOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("max_cnt", c_i), ("min_dist", c_i), ("candidate_capacity", c_i), ("sort_chunk", c_i), ("reserved", c_i), ("quality", c_d)]


def det_default_options(lib, **kw):
    return options_struct(lib, DET_PREFIX, "", DetOptions, kw)


class Detector(Handle):
    """setMask, goodFeaturesToTrack and addPoints on the current image and the held points of `tracker` (a Tracker on the same library
    and context); see include/gfbe_det.h. Close it before the tracker. options: fields of gfbe_det_options. The *_raw methods return
    the status first; the others raise."""

    def __init__(self, lib, ctx, tracker, **options):
        Handle.__init__(self, lib, DET_PREFIX, ctx)
        self.tracker = tracker
        self.opt = self._options(DetOptions, options)
        self._check(self._f("create")(self.ctx, tracker.h, C.byref(self.opt), C.byref(self.h)), "create")

    def set_next_id(self, next_id):
        """n_id of addPoints per camera (it starts at 0)."""
        v = _i32(next_id)
        assert len(v) == self.tracker.n_cameras
        self._check(self._f("set_next_id")(self.ctx, self.h, _pi(v)), "set_next_id")

    def detect_raw(self, fill=-7):
        """Returns (status, per-camera list of dict(pts, ids, track_cnt, counters)); the flat outputs start as `fill`."""
        t = self.tracker
        C_ = t.n_cameras
        room = sum(max(n, self.opt.max_cnt) for n in t.held)
        off = np.full(C_ + 1, fill, np.int32)
        pts, ids, cnt = np.full((room, 2), fill, np.float32), np.full(room, fill, np.int32), np.full(room, fill, np.int32)
        counters = np.full((C_, 6), fill, np.int32)
        rc = self._f("detect")(self.ctx, self.h, _pi(off), pts.ctypes.data_as(PF), _pi(ids), _pi(cnt), _pi(counters))
        if rc != OK:
            return rc, dict(offset=off, pts=pts, ids=ids, track_cnt=cnt, counters=counters)
        t.held = [int(x) for x in np.diff(off)]
        return rc, [dict(pts=pts[a:b].copy(), ids=ids[a:b].copy(), track_cnt=cnt[a:b].copy(), counters=dict(zip(DET_COUNTERS, counters[k].tolist())))
                    for k, (a, b) in enumerate(zip(off[:-1], off[1:]))]

    def detect(self):
        """G1, G3, G4, G5 for every camera (one wait); the result becomes the tracker's held points."""
        rc, out = self.detect_raw()
        self._check(rc, "detect")
        return out

    def corners_raw(self, max_corners, quality=0.01, min_dist=10, fill=-7):
        """goodFeaturesToTrack with no mask: (status, per-camera list of dict(pts [n, 2], response [n]) in order of acceptance)."""
        C_ = self.tracker.n_cameras
        room = C_ * max(int(max_corners), 0)
        off, pts, resp = np.full(C_ + 1, fill, np.int32), np.full((room, 2), fill, np.float32), np.full(room, fill, np.float32)
        rc = self._f("corners")(self.ctx, self.h, int(max_corners), float(quality), int(min_dist), _pi(off), pts.ctypes.data_as(PF), resp.ctypes.data_as(PF))
        if rc != OK:
            return rc, dict(offset=off, pts=pts, response=resp)
        return rc, [dict(pts=pts[a:b].copy(), response=resp[a:b].copy()) for a, b in zip(off[:-1], off[1:])]

    def corners(self, max_corners, quality=0.01, min_dist=10):
        rc, out = self.corners_raw(max_corners, quality, min_dist)
        self._check(rc, "corners")
        return out

    def planes(self, camera):
        """dict(eig [rows, cols] float32, mask [rows, cols] uint8) of a camera: the response plane and the mask of the last detect."""
        t = self.tracker
        eig, mask = np.zeros((t.rows, t.cols), np.float32), np.zeros((t.rows, t.cols), np.uint8)
        self._check(self._f("download")(self.ctx, self.h, int(camera), eig.ctypes.data_as(PF), mask.ctypes.data_as(PU8)), "download")
        return dict(eig=eig, mask=mask)


# ---------------------------------------------------------------------------------------------
# the frame observations between the tracker and the feature tables (gfbe_obs_* of include/gfbe_obs.h; the model is tests/obs_np.py,
# there is no oracle row)
# ---------------------------------------------------------------------------------------------
OBS_PREFIX = "gfbe_obs_"
OBS_COUNTERS = ("points", "found", "outside", "duplicate")
PU16 = C.POINTER(C.c_uint16)


class ObsOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("depth_cam", c_i), ("match_tile", c_i), ("reserved", c_i)]


def obs_default_options(lib, **kw):
    return options_struct(lib, OBS_PREFIX, "", ObsOptions, kw)


class Observer(Handle):
    """undistortedPts, ptsVelocity, the depth lookup and the id-ordered frame on the held points of `tracker` (a Tracker on the same
    library and context), the frame's hand-over to a FeatureTables with one table a camera, removeOutliers and the prediction; see
    include/gfbe_obs.h. cameras [n_cameras, 8] = fx fy cx cy k1 k2 p1 p2. Close it before the tracker. options: fields of
    gfbe_obs_options. The *_raw methods return the status first; the others raise."""

    def __init__(self, lib, ctx, tracker, cameras, **options):
        Handle.__init__(self, lib, OBS_PREFIX, ctx)
        self.tracker = tracker
        self.opt = self._options(ObsOptions, options)
        cams = _f64(cameras).reshape(-1, 8)
        assert len(cams) == tracker.n_cameras, cams.shape
        self._check(self._f("create")(self.ctx, tracker.h, _pd(cams), C.byref(self.opt), C.byref(self.h)), "create")

    def reset(self):
        """Forgets the previous lists and the times."""
        self._check(self._f("reset")(self.ctx, self.h), "reset")

    def observe_raw(self, cur_time, depth=None, outputs=True, fill=-7):
        """cur_time [n_cameras]; depth [n_cameras, rows, cols] uint16 or None. Returns (status, per-camera list of dict(ids, obs8
        [n, 8], counters)); outputs False: only the counters are downloaded (ids / obs8 None). The flat outputs start as `fill`."""
        t = self.tracker
        C_, n = t.n_cameras, sum(t.held)
        tm = _f64(cur_time)
        assert len(tm) == C_
        dp = None
        if depth is not None:
            dp = np.ascontiguousarray(depth, np.uint16)
            assert dp.size == C_ * t.rows * t.cols, dp.shape
        off, counters = np.full(C_ + 1, fill, np.int32), np.full((C_, 4), fill, np.int32)
        ids, obs8 = np.full(n, fill, np.int32), np.full((n, 8), float(fill))
        rc = self._f("observe")(self.ctx, self.h, _pd(tm), dp.ctypes.data_as(PU16) if dp is not None else None, _pi(off) if outputs else None,
                                _pi(ids) if outputs else None, _pd(obs8) if outputs else None, _pi(counters))
        if rc != OK:
            return rc, dict(offset=off, ids=ids, obs8=obs8, counters=counters)
        if not outputs:
            return rc, [dict(ids=None, obs8=None, counters=dict(zip(OBS_COUNTERS, counters[k].tolist()))) for k in range(C_)]
        return rc, [dict(ids=ids[a:b].copy(), obs8=obs8[a:b].copy(), counters=dict(zip(OBS_COUNTERS, counters[k].tolist())))
                    for k, (a, b) in enumerate(zip(off[:-1], off[1:]))]

    def observe(self, cur_time, depth=None, outputs=True):
        """O3 .. O6 for every camera (one wait); the frame stays on the device for add_frame."""
        rc, out = self.observe_raw(cur_time, depth, outputs)
        self._check(rc, "observe")
        return out

    def add_frame_raw(self, tables, frame_count, td, fill=-7):
        """The held frame into `tables` (a FeatureTables of n_cameras tables). Returns (status, (keyframe, counters [W, 3], avg_parallax))."""
        W = self.tracker.n_cameras
        fc, tdv = _i32(frame_count), _f64(td)
        assert len(fc) == W and len(tdv) == W
        kf, cnt, avg = np.full(W, fill, np.int32), np.full((W, 3), fill, np.int32), np.full(W, float(fill))
        rc = self._f("add_frame")(self.ctx, self.h, tables.h, _pi(fc), _pd(tdv), _pi(kf), _pi(cnt), _pd(avg))
        return rc, (kf, cnt, avg)

    def add_frame(self, tables, frame_count, td):
        rc, out = self.add_frame_raw(tables, frame_count, td)
        self._check(rc, "add_frame")
        return out

    def remove_outliers_raw(self, ids):
        """ids: per camera the feature ids to drop from the held points."""
        off = _offsets([len(x) for x in ids])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32).ravel() for x in ids]) if len(ids) else np.zeros(0), np.int32)
        held = np.zeros(self.tracker.n_cameras, np.int32)
        rc = self._f("remove_outliers")(self.ctx, self.h, _pi(off), _pi(flat), _pi(held))
        if rc == OK:
            self.tracker.held = [int(x) for x in held]
        return rc

    def remove_outliers(self, ids):
        self._check(self.remove_outliers_raw(ids), "remove_outliers")

    def predict_raw(self, tables, frame_count, poses, tic_ric, next_pose, fill=-7):
        """poses [W, 11, 12], tic_ric [W, 12], next_pose [W, 12] (rows [P | R]). Returns (status, (per-camera predict_pts [n, 2] in held
        order, n_predicted [W]))."""
        t = self.tracker
        W, n = t.n_cameras, sum(t.held)
        fc, p, e, nx = _i32(frame_count), _f64(poses).reshape(W, 132), _f64(tic_ric).reshape(W, 12), _f64(next_pose).reshape(W, 12)
        assert len(fc) == W
        pred, npred = np.full((n, 2), fill, np.float32), np.full(W, fill, np.int32)
        rc = self._f("predict")(self.ctx, self.h, tables.h, _pi(fc), _pd(p), _pd(e), _pd(nx), pred.ctypes.data_as(PF), _pi(npred))
        off = _offsets(t.held)
        return rc, ([pred[a:b] for a, b in zip(off[:-1], off[1:])], npred)

    def predict(self, tables, frame_count, poses, tic_ric, next_pose):
        rc, out = self.predict_raw(tables, frame_count, poses, tic_ric, next_pose)
        self._check(rc, "predict")
        return out

    def previous(self, camera):
        """dict(ids [n], un_pts [n, 2]) of a camera's previous list, ascending in id."""
        cap = self.tracker.cap
        n, ids, un = c_i(-1), np.zeros(cap, np.int32), np.zeros((cap, 2), np.float32)
        self._check(self._f("download_prev")(self.ctx, self.h, int(camera), C.byref(n), _pi(ids), un.ctypes.data_as(PF)), "download_prev")
        return dict(ids=ids[:n.value].copy(), un_pts=un[:n.value].copy())


# ---------------------------------------------------------------------------------------------
# the keyframe descriptors between the tracker and the loop database (gfbe_kfd_* of include/gfbe_kfd.h; the model is tests/kfd_np.py,
# there is no oracle row)
# ---------------------------------------------------------------------------------------------
KFD_PREFIX = "gfbe_kfd_"
KFD_COUNTERS = ("corners", "kept", "listed", "overflow")


class KfdOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("ring_slots", c_i), ("fast_threshold", c_i), ("keypoint_capacity", c_i), ("window_capacity", c_i), ("reserved", c_i)]


def kfd_default_options(lib, **kw):
    return options_struct(lib, KFD_PREFIX, "", KfdOptions, kw)


class KeyframeDescriber(Handle):
    """The blurred image, FAST corners, BRIEF descriptors and keypoints_norm of a keyframe for n_cameras cameras of rows x cols uint8
    images, and their hand-over to a LoopDatabase on the same library and context; see include/gfbe_kfd.h. pattern [4, 256] int32 =
    x1 y1 x2 y2 of the pairs, cameras [n_cameras, 8] = fx fy cx cy k1 k2 p1 p2. options: fields of gfbe_kfd_options. The *_raw methods
    return the status first; the others raise."""

    def __init__(self, lib, ctx, n_cameras, rows, cols, pattern, cameras, **options):
        Handle.__init__(self, lib, KFD_PREFIX, ctx)
        self.n_cameras, self.rows, self.cols = int(n_cameras), int(rows), int(cols)
        self.opt = self._options(KfdOptions, options)
        pat, cams = _i32(pattern).reshape(4, 256), _f64(cameras).reshape(-1, 8)
        assert len(cams) == self.n_cameras, cams.shape
        self._check(self._f("create")(self.ctx, self.n_cameras, self.rows, self.cols, _pi(pat), _pd(cams), C.byref(self.opt), C.byref(self.h)), "create")

    def push_image_raw(self, slot, images):
        im = _u8(images)
        assert im.size == self.n_cameras * self.rows * self.cols, im.shape
        return self._f("push_image")(self.ctx, self.h, int(slot), im.ctypes.data_as(PU8))

    def push_image(self, slot, images):
        """images [n_cameras, rows, cols] uint8 into ring slot `slot` (K6), with the slot's blurred image."""
        self._check(self.push_image_raw(slot, images), "push_image")

    def capture_raw(self, tracker, slot):
        return self._f("capture")(self.ctx, self.h, tracker.h, int(slot))

    def capture(self, tracker, slot):
        """The current images of `tracker` (a Tracker of the same n_cameras, rows and cols) into ring slot `slot`; no wait."""
        self._check(self.capture_raw(tracker, slot), "capture")

    def extract_raw(self, slot, outputs=True, fill=-7):
        """K2 .. K5 on a slot. Returns (status, per-camera list of dict(pts [n, 2], score [n], pts_norm [n, 2], desc [n, 4] uint64,
        counters)); outputs False: only the counters come back (the lists None). The flat outputs start as `fill`."""
        C_, room = self.n_cameras, self.n_cameras * self.opt.keypoint_capacity if outputs else 0
        off, counters = np.full(C_ + 1, fill, np.int32), np.full((C_, 4), fill, np.int32)
        pts, ptsn = np.full((room, 2), fill, np.float32), np.full((room, 2), fill, np.float32)
        score, desc = np.full(room, fill, np.int32), np.full((room, 4), fill % (1 << 64), np.uint64)
        rc = self._f("extract")(self.ctx, self.h, int(slot), _pi(off), pts.ctypes.data_as(PF) if outputs else None, _pi(score) if outputs else None,
                                ptsn.ctypes.data_as(PF) if outputs else None, desc.ctypes.data_as(PU64) if outputs else None, _pi(counters))
        if rc != OK:
            return rc, dict(offset=off, pts=pts, score=score, pts_norm=ptsn, desc=desc, counters=counters)
        if not outputs:
            return rc, [dict(pts=None, score=None, pts_norm=None, desc=None, counters=dict(zip(KFD_COUNTERS, counters[k].tolist()))) for k in range(C_)]
        return rc, [dict(pts=pts[a:b].copy(), score=score[a:b].copy(), pts_norm=ptsn[a:b].copy(), desc=desc[a:b].copy(), counters=dict(zip(KFD_COUNTERS, counters[k].tolist())))
                    for k, (a, b) in enumerate(zip(off[:-1], off[1:]))]

    def extract(self, slot, outputs=True):
        rc, out = self.extract_raw(slot, outputs)
        self._check(rc, "extract")
        return out

    def describe_raw(self, slot, pts_uv, fill=-7):
        """K4 on per-camera window points pts_uv [n, 2]. Returns (status, per-camera list of dict(desc [n, 4], points, zeroed))."""
        off = _offsets([len(np.asarray(p).reshape(-1, 2)) for p in pts_uv])
        n = int(off[-1])
        p = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 2) for x in pts_uv]) if len(pts_uv) else np.zeros((0, 2)), np.float32)
        desc, counters = np.full((n, 4), fill % (1 << 64), np.uint64), np.full((self.n_cameras, 2), fill, np.int32)
        rc = self._f("describe")(self.ctx, self.h, int(slot), _pi(off), p.ctypes.data_as(PF), desc.ctypes.data_as(PU64), _pi(counters))
        if rc != OK:
            return rc, dict(desc=desc, counters=counters)
        return rc, [dict(desc=desc[a:b].copy(), points=int(counters[k, 0]), zeroed=int(counters[k, 1])) for k, (a, b) in enumerate(zip(off[:-1], off[1:]))]

    def describe(self, slot, pts_uv):
        rc, out = self.describe_raw(slot, pts_uv)
        self._check(rc, "describe")
        return out

    def add_keyframe_raw(self, camera, db, detect_loop=True):
        """LoopDatabase.add_keyframe_raw on `camera`'s lists of the last extract, from the device."""
        idx, loop, nr = c_i(-7), c_i(-7), c_i(-7)
        rid, rs = np.full(LDB_MAX_RESULTS, -7, np.int32), np.zeros(LDB_MAX_RESULTS)
        rc = self._f("add_keyframe")(self.ctx, self.h, int(camera), db.h, int(bool(detect_loop)), C.byref(idx), C.byref(loop), C.byref(nr), _pi(rid), _pd(rs))
        n = max(nr.value, 0)
        return rc, dict(index=idx.value, loop_index=loop.value, result_id=rid[:n].copy(), result_score=rs[:n].copy())

    def add_keyframe(self, camera, db, detect_loop=True):
        rc, out = self.add_keyframe_raw(camera, db, detect_loop)
        self._check(rc, "add_keyframe")
        return out

    def match_raw(self, camera, db, old_index, n_window):
        """LoopDatabase.match_raw with `camera`'s n_window window descriptors of the last describe, from the device."""
        n = int(n_window)
        st, bi, bd, nm = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32), c_i(-7)
        src, pt, ptn = np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        rc = self._f("match")(self.ctx, self.h, int(camera), db.h, int(old_index), st.ctypes.data_as(PU8), _pi(bi), _pi(bd), C.byref(nm), _pi(src), pt.ctypes.data_as(PF),
                              ptn.ctypes.data_as(PF))
        m = max(nm.value, 0)
        return rc, dict(status=st, best_index=bi, best_dist=bd, n_matched=nm.value, matched_src=src[:m], matched_pt=pt[:m], matched_pt_norm=ptn[:m])

    def match(self, camera, db, old_index, n_window):
        rc, out = self.match_raw(camera, db, old_index, n_window)
        self._check(rc, "match")
        return out

    def planes(self, slot, camera, score=True):
        """dict(blurred [rows, cols] uint8, score [rows, cols] uint8 after suppression) of a camera of a slot (score: after an extract)."""
        bl, sc = np.zeros((self.rows, self.cols), np.uint8), np.zeros((self.rows, self.cols), np.uint8)
        self._check(self._f("download")(self.ctx, self.h, int(slot), int(camera), bl.ctypes.data_as(PU8), sc.ctypes.data_as(PU8) if score else None), "download")
        return dict(blurred=bl, score=sc if score else None)


# ---------------------------------------------------------------------------------------------
# the loop verification between the loop database's matches and a loop edge (gfbe_pnp_* of include/gfbe_pnp.h; the model is
# tests/pnp_np.py, there is no oracle row)
# ---------------------------------------------------------------------------------------------
PNP_PREFIX = "gfbe_pnp_"


class PnpOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("max_problems", c_i), ("max_points", c_i), ("iterations", c_i), ("refine_iterations", c_i), ("min_loop_num", c_i),
                ("seed", C.c_uint64), ("reproj_threshold", c_d), ("max_yaw_deg", c_d), ("max_translation", c_d)]


def pnp_default_options(lib, **kw):
    return options_struct(lib, PNP_PREFIX, "", PnpOptions, kw)


class LoopVerifier(Handle):
    """PnPRANSAC and the loop_info half of KeyFrame::findConnection for a batch of problems, and the whole chain from window descriptors
    on a LoopDatabase (and a KeyframeDescriber) of the same library and context; see include/gfbe_pnp.h. options: fields of
    gfbe_pnp_options. The *_raw methods return the status first; the others raise."""

    def __init__(self, lib, ctx, **options):
        Handle.__init__(self, lib, PNP_PREFIX, ctx)
        self.opt = self._options(PnpOptions, options)
        self._check(self._f("create")(self.ctx, C.byref(self.opt), C.byref(self.h)), "create")

    @staticmethod
    def _results(B, fill):
        return dict(n_inliers=np.full(B, fill, np.int32), has_loop=np.full(B, fill, np.int32), loop_info=np.full((B, 8), float(fill)), pnp_pose=np.full((B, 12), float(fill)),
                    best=np.full((B, 2), fill, np.int32), refine_flag=np.full(B, fill, np.int32))

    @staticmethod
    def _result_args(r):
        return [_pi(r["n_inliers"]), _pi(r["has_loop"]), _pd(r["loop_info"]), _pd(r["pnp_pose"]), _pi(r["best"]), _pi(r["refine_flag"])]

    def verify_raw(self, offset, point_3d, pt_norm, pose_cur, tic_qic, diagnostics=False, fill=-7):
        """V1 .. V8 of len(offset) - 1 problems. Returns (status, dict(status [n] uint8, n_inliers, has_loop, refine_flag [B], loop_info
        [B, 8], pnp_pose [B, 12], best [B, 2]; diagnostics: sample_idx [B, H, 3], n_solutions [B, H], hyp_pose [B, H, 4, 12], hyp_count
        [B, H, 4])). The outputs start as `fill`."""
        off, p3, pn = _i32(offset), _f32(point_3d).reshape(-1, 3), _f32(pt_norm).reshape(-1, 2)
        pc, tq = _f64(pose_cur).reshape(-1, 12), _f64(tic_qic).reshape(-1, 12)
        B, H = len(off) - 1, self.opt.iterations
        assert len(p3) == len(pn) and len(pc) == len(tq) == B
        r = self._results(B, fill)
        r["status"] = np.full(len(p3), fill % 256, np.uint8)
        d = [None] * 4
        if diagnostics:
            r.update(sample_idx=np.full((B, H, 3), fill, np.int32), n_solutions=np.full((B, H), fill, np.int32), hyp_pose=np.full((B, H, 4, 12), float(fill)),
                     hyp_count=np.full((B, H, 4), fill, np.int32))
            d = [_pi(r["sample_idx"]), _pi(r["n_solutions"]), _pd(r["hyp_pose"]), _pi(r["hyp_count"])]
        rc = self._f("verify")(self.ctx, self.h, B, _pi(off), p3.ctypes.data_as(PF), pn.ctypes.data_as(PF), _pd(pc), _pd(tq), r["status"].ctypes.data_as(PU8),
                               *(self._result_args(r) + d))
        return rc, r

    def verify(self, offset, point_3d, pt_norm, pose_cur, tic_qic, diagnostics=False):
        rc, out = self.verify_raw(offset, point_3d, pt_norm, pose_cur, tic_qic, diagnostics)
        self._check(rc, "verify")
        return out

    def _connect(self, name, head, n_window, point_3d, pose_cur, tic_qic, fill):
        n = int(n_window)
        p3, pc, tq = _f32(point_3d).reshape(-1, 3), _f64(pose_cur).reshape(12), _f64(tic_qic).reshape(12)
        assert len(p3) == n, (p3.shape, n)
        nm, src, pt, ptn, stp = c_i(fill), np.full(n, fill, np.int32), np.full((n, 2), fill, np.float32), np.full((n, 2), fill, np.float32), np.full(n, fill % 256, np.uint8)
        r = self._results(1, fill)
        rc = self._f(name)(self.ctx, self.h, *(head + [p3.ctypes.data_as(PF), _pd(pc), _pd(tq), C.byref(nm), _pi(src), pt.ctypes.data_as(PF), ptn.ctypes.data_as(PF),
                                                       stp.ctypes.data_as(PU8)] + self._result_args(r)))
        m = max(nm.value, 0) if rc == OK else 0
        out = dict(n_matched=nm.value, matched_src=src[:m], matched_pt=pt[:m], matched_pt_norm=ptn[:m], status_pnp=stp[:m])
        out.update({k: v[0] for k, v in r.items()})
        out["raw"] = dict(matched_src=src, matched_pt=pt, matched_pt_norm=ptn, status_pnp=stp)
        return rc, out

    def find_connection_raw(self, db, old_index, window_desc, point_3d, pose_cur, tic_qic, fill=-7):
        """gfbe_ldb_match's rule 6 and reduceVector on window_desc [n_window, 4] against held keyframe old_index of `db`, the gather of
        point_3d [n_window, 3] by matched_src and V1 .. V8, with one wait. Returns (status, dict(n_matched, matched_src, matched_pt,
        matched_pt_norm, status_pnp, n_inliers, has_loop, loop_info [8], pnp_pose [12], best [2], refine_flag))."""
        w = _u64(window_desc)
        return self._connect("find_connection", [db.h, int(old_index), len(w), w.ctypes.data_as(PU64)], len(w), point_3d, pose_cur, tic_qic, fill)

    def find_connection(self, db, old_index, window_desc, point_3d, pose_cur, tic_qic):
        rc, out = self.find_connection_raw(db, old_index, window_desc, point_3d, pose_cur, tic_qic)
        self._check(rc, "find_connection")
        return out

    def find_connection_kfd_raw(self, describer, camera, db, old_index, n_window, point_3d, pose_cur, tic_qic, fill=-7):
        """find_connection_raw on `camera`'s n_window window descriptors of `describer`'s last describe, from the device."""
        return self._connect("find_connection_kfd", [describer.h, int(camera), db.h, int(old_index)], n_window, point_3d, pose_cur, tic_qic, fill)

    def find_connection_kfd(self, describer, camera, db, old_index, n_window, point_3d, pose_cur, tic_qic):
        rc, out = self.find_connection_kfd_raw(describer, camera, db, old_index, n_window, point_3d, pose_cur, tic_qic)
        self._check(rc, "find_connection_kfd")
        return out


# ---------------------------------------------------------------------------------------------
# the image equalisation in front of the tracker and the keyframe descriptors (gfbe_eq_* of include/gfbe_eq.h; the model is
# tests/eq_np.py, there is no oracle row)
# ---------------------------------------------------------------------------------------------
EQ_PREFIX = "gfbe_eq_"


class EqOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("tiles_x", c_i), ("tiles_y", c_i), ("reserved", c_i), ("clip_limit", c_d)]


def eq_default_options(lib, **kw):
    return options_struct(lib, EQ_PREFIX, "", EqOptions, kw)


class Equalizer(Handle):
    """CLAHE of n_cameras uint8 images of rows x cols on the device: on its own (apply), or in front of a Tracker's push_image
    (push_klt) and of a KeyframeDescriber's push_image (push_kfd) on the same library and context; see include/gfbe_eq.h. options:
    fields of gfbe_eq_options. The *_raw methods return the status first; the others raise."""

    def __init__(self, lib, ctx, n_cameras, rows, cols, **options):
        Handle.__init__(self, lib, EQ_PREFIX, ctx)
        self.n_cameras, self.rows, self.cols = int(n_cameras), int(rows), int(cols)
        self.opt = self._options(EqOptions, options)
        self._check(self._f("create")(self.ctx, self.n_cameras, self.rows, self.cols, C.byref(self.opt), C.byref(self.h)), "create")

    def _images(self, images):
        im = _u8(images)
        assert im.size == self.n_cameras * self.rows * self.cols, im.shape
        return im

    def apply_raw(self, images, out=None):
        """(status, equalised images [n_cameras, rows, cols]); out: the array to write (it may be `images` itself)."""
        im = self._images(images)
        res = np.zeros((self.n_cameras, self.rows, self.cols), np.uint8) if out is None else out
        return self._f("apply")(self.ctx, self.h, im.ctypes.data_as(PU8), res.ctypes.data_as(PU8)), res

    def apply(self, images, out=None):
        rc, res = self.apply_raw(images, out)
        self._check(rc, "apply")
        return res

    def push_klt_raw(self, tracker, images):
        return self._f("push_klt")(self.ctx, self.h, tracker.h, self._images(images).ctypes.data_as(PU8))

    def push_klt(self, tracker, images):
        """Tracker.push_image of the equalised images (does not wait for the device)."""
        self._check(self.push_klt_raw(tracker, images), "push_klt")

    def push_kfd_raw(self, describer, slot, images):
        return self._f("push_kfd")(self.ctx, self.h, describer.h, int(slot), self._images(images).ctypes.data_as(PU8))

    def push_kfd(self, describer, slot, images):
        """KeyframeDescriber.push_image of the equalised images into ring slot `slot`."""
        self._check(self.push_kfd_raw(describer, slot, images), "push_kfd")

    def lut_raw(self, fill=7):
        lut = np.full((self.n_cameras, self.opt.tiles_y, self.opt.tiles_x, 256), fill, np.uint8)
        return self._f("download_lut")(self.ctx, self.h, lut.ctypes.data_as(PU8)), lut

    def lut(self):
        """The LUTs [n_cameras, tiles_y, tiles_x, 256] of the last apply / push."""
        rc, lut = self.lut_raw()
        self._check(rc, "download_lut")
        return lut


# ---------------------------------------------------------------------------------------------
# the sensor gate on the feature tables: stationarity, wheel anomaly, the wheel prediction (gfbe_gate_* of include/gfbe_gate.h; the
# model is tests/gate_np.py, there is no oracle row)
# ---------------------------------------------------------------------------------------------
GATE_PREFIX = "gfbe_gate_"
GATE_WHEEL_ANOMALY, GATE_WHEEL_STATIONARY, GATE_PREINT_STATIONARY, GATE_VAR_STATIONARY = 1, 2, 4, 8
GATE_IMU_EXCITED, GATE_VISUAL_STATIONARY, GATE_IMU_STATIONARY, GATE_SYSTEM_STATIONARY = 16, 32, 64, 128


class GateOptions(C.Structure):
    _fields_ = [("struct_size", c_i), ("max_samples", c_i), ("max_frames", c_i), ("use_wheel", c_i), ("wdetect", c_i), ("depth_mode", c_i), ("min_pair_count", c_i),
                ("reserved", c_i), ("dis_threshold", c_d), ("wheel_still_norm", c_d), ("preint_still_norm", c_d), ("var_still", c_d), ("var_excited", c_d),
                ("still_parallax_px", c_d), ("init_parallax_px", c_d), ("parallax_focal", c_d), ("depth_min", c_d), ("depth_max", c_d)]


def gate_default_options(lib, **kw):
    return options_struct(lib, GATE_PREFIX, "", GateOptions, kw)


def gate_ragged(rows, width):
    """(offset [B + 1] int32, the rows of B lists [n, width] packed)"""
    rows = [np.asarray(r, np.float64).reshape(-1, width) for r in rows]
    off = np.zeros(len(rows) + 1, np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, width)))


class SensorGate(Handle):
    """The reference's per-frame sensor-state detectors and the wheel prediction of the newest frame for n_robots robots, robot b on
    table b of a FeatureTables of the same library and context; see include/gfbe_gate.h. options: fields of gfbe_gate_options. The
    *_raw methods return the status first; the others raise."""

    def __init__(self, lib, ctx, n_robots, **options):
        Handle.__init__(self, lib, GATE_PREFIX, ctx)
        self.B = int(n_robots)
        self.opt = self._options(GateOptions, options)
        self._check(self._f("create")(self.ctx, self.B, C.byref(self.opt), C.byref(self.h)), "create")

    def _stats(self, fill):
        B = self.B
        return dict(pair_count=np.full((B, 10), fill, np.int32), pair_sum=np.full((B, 10), float(fill)), l_still=np.full(B, fill, np.int32), l_init=np.full(B, fill, np.int32))

    def frame_raw(self, tables, frame_count, imu, imu_first, wheel, wheel_first, pose, vel_ba, g_norm, stationary_prev, frames, fill=-7):
        """G1 .. G7. imu / wheel: per robot [n, 7] rows (wheel, wheel_first: None with use_wheel == 0); frames: per robot [M, 4]; imu_first,
        wheel_first [B, 6]; pose [B, 12]; vel_ba [B, 6]. Returns (status, dict(flags, l_still, l_init [B], pair_count, pair_sum [B, 10],
        dP_imu, dP_wheel [B, 3], dis, var [B], pose_out [B, 12], vel_out [B, 3])). The outputs start as `fill`."""
        B = self.B
        io, iv = gate_ragged(imu, 7)
        fo, fv = gate_ragged(frames, 4)
        wo, wv, wf = (None, None, None) if wheel is None else gate_ragged(wheel, 7) + (_f64(wheel_first).reshape(B, 6),)
        fc, sp, i1, ps, vb = _i32(frame_count), _i32(stationary_prev), _f64(imu_first).reshape(B, 6), _f64(pose).reshape(B, 12), _f64(vel_ba).reshape(B, 6)
        assert len(fc) == len(sp) == len(io) - 1 == len(fo) - 1 == B
        r = self._stats(fill)
        r.update(flags=np.full(B, fill, np.int32), dP_imu=np.full((B, 3), float(fill)), dP_wheel=np.full((B, 3), float(fill)), dis=np.full(B, float(fill)),
                 var=np.full(B, float(fill)), pose_out=np.full((B, 12), float(fill)), vel_out=np.full((B, 3), float(fill)))
        opt = lambda a, f: f(a) if a is not None else None
        rc = self._f("frame")(self.ctx, self.h, tables.h, _pi(fc), _pi(io), _pd(iv), _pd(i1), opt(wo, _pi), opt(wv, _pd), opt(wf, _pd), _pd(ps), _pd(vb), float(g_norm), _pi(sp),
                              _pi(fo), _pd(fv), _pi(r["flags"]), _pi(r["l_still"]), _pi(r["l_init"]), _pi(r["pair_count"]), _pd(r["pair_sum"]), _pd(r["dP_imu"]),
                              _pd(r["dP_wheel"]), _pd(r["dis"]), _pd(r["var"]), _pd(r["pose_out"]), _pd(r["vel_out"]))
        return rc, r

    def frame(self, tables, frame_count, imu, imu_first, wheel, wheel_first, pose, vel_ba, g_norm, stationary_prev, frames):
        rc, out = self.frame_raw(tables, frame_count, imu, imu_first, wheel, wheel_first, pose, vel_ba, g_norm, stationary_prev, frames)
        self._check(rc, "frame")
        return out

    def pair_stats_raw(self, tables, mode, fill=-7):
        """G5, G6 alone: (status, dict(pair_count, pair_sum [B, 10], l_still, l_init [B]))."""
        r = self._stats(fill)
        return self._f("pair_stats")(self.ctx, self.h, tables.h, int(mode), _pi(r["pair_count"]), _pd(r["pair_sum"]), _pi(r["l_still"]), _pi(r["l_init"])), r

    def pair_stats(self, tables, mode):
        rc, out = self.pair_stats_raw(tables, mode)
        self._check(rc, "pair_stats")
        return out

    def corresponding_raw(self, tables, mode, l, r, room, fill=-7):
        """G8 with room[b] pairs of room for table b: (status, count [B], a, b [sum(room), 3], offset [B + 1])."""
        lv, rv = _i32(l), _i32(r)
        off = np.zeros(self.B + 1, np.int32)
        off[1:] = np.cumsum(_i32(room))
        a, b, cnt = np.full((int(off[-1]), 3), float(fill)), np.full((int(off[-1]), 3), float(fill)), np.full(self.B, fill, np.int32)
        return self._f("corresponding")(self.ctx, self.h, tables.h, int(mode), _pi(lv), _pi(rv), _pi(off), _pd(a), _pd(b), _pi(cnt)), cnt, a, b, off

    def corresponding(self, tables, mode, l, r):
        """The pairs of (l[b], r[b]) per table in list order: a list of (a [n, 3], b [n, 3]). Sizes with a first call without room."""
        rc, cnt, _, _, _ = self.corresponding_raw(tables, mode, l, r, np.zeros(self.B, np.int32))
        if rc != OK and (rc != BAD_INPUT or (cnt < 0).any()):
            self._check(rc, "corresponding")
        rc, cnt, a, b, off = self.corresponding_raw(tables, mode, l, r, cnt)
        self._check(rc, "corresponding")
        return [(a[off[q]:off[q] + cnt[q]].copy(), b[off[q]:off[q] + cnt[q]].copy()) for q in range(self.B)]
