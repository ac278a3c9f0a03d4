"""The normal equations of one linearisation, summed in extended precision from the oracle's per-factor blocks — the reference
tests/test_gpu_normal_equations.py holds the device's assembled H, g and Schur term E, eg against, entry by entry, and the windows
(prescribed landmark counts per start frame and track length) it does that on. CPU only; tests/test_normal_equations_reference.py
checks this module against the oracle's own FP64 linearisation and against dist.reduced_system.

What is compared, for every entry X[i, j] of H (lower triangle), g, E (73 x 73) and eg, with u = 2^-53:

    |X_dev[i, j] - X_ref[i, j]| <= K * u * A_X[i, j]

A_X is the ABSOLUTE sum that belongs to the entry: A_H = sum_k |J_k|^T |J_k| over the factors (the prior: |J0|^T |J0|),
A_g = sum_k |J_k|^T |r_k|, A_Hll = Hll, A_gl = sum |w|^T |r|, A_Hpl = sum |J|^T |w| (w: a factor's landmark column). The Schur term
is a sum of products of such sums, E = sum_l w_l h_l h_l^T with h_l = Hpl[l]: its scale carries the rounding of h_l along,
A_E = sum_l w_l A_Hpl[l] A_Hpl[l]^T and A_eg = sum_l w_l A_Hpl[l] A_gl[l] (>= sum_l w_l |h_l| |h_l|^T; equal where a landmark's
factors do not cancel). Where A_X is exactly zero — a constant block, a pose pair no factor couples, E of a window without landmarks —
the entry is a structural zero and the device must hold exactly 0.0.

Coordinates of E and eg (k_schur / k_visasm / k_assemble): the landmark side is Jacobi-scaled and mu-regularised through the weight
w_l = s_l^2 / (s_l^2 Hll + mu clamp(s_l^2 Hll)), s_l = 1 / (1 + sqrt(Hll)); the pose columns are the raw, unscaled ones of H and g.

K is measured against this reference, not against the device: test_normal_equations_reference.py computes, on every case below,
|X_fp64 - X_ref| / (u A_X) for the oracle's plain FP64 loop (gfo_linearize: H, g, Hll, gl, Hpl) and for an FP64 numpy contraction
in the style of dist.reduced_system (E, eg). Largest ratios over all cases (the CPU test asserts K_MEASURED so they cannot drift):

    H %(H)s   g %(g)s   Hll %(Hll)s   gl %(gl)s   Hpl %(Hpl)s   E %(E)s   eg %(eg)s        (in units of u A_X)

K = 8 x the largest, rounded up to a power of two. The margin of 8 is for what the device legitimately does differently from a
plain FP64 loop: another grouping of the sums, matrix-core accumulation, per-factor blocks that agree with the oracle's to 1e-12
and not to the bit, Hpl rows formed from the compressed D / x form. K = %(K)s. (Why a plain FP64 loop is 69 u off in H: the
inertial factors' ~1e9 are added first and every one of a pose's ~1 000 visual terms is then rounded at that magnitude.)
Entries the IMU factors reach have a second allowance, see IMU_BLOCK_TOL below.

Windows with GNSS, PlaneFactors or the PoseAnchorFactor (tests/gnss_window_cases.py: ne_case; tests/test_gpu_gnss_normal_equations.py):
the GNSS blocks come from the longdouble model of tests/gnss_np.py with that model's absolute sums, the plane and anchor blocks from
the oracle's stand-alone evaluators; g carries the allowance of the GNSS residuals' own rounding (_Acc.add_gnss), and those small
windows the allowance of the reference's own visual blocks (VIS_BLOCK_TOL).

The device against this bound (MI355X, worst entry over all cases, in u A_X): alone H 888, g 14, E 1023, eg 424; throughput batches
with uncompressed rows H 888, g 14, E 532, eg 424, with compressed rows H 317, g 2.9, E 1020, eg 424 (per case and launch shape in
tests/test_gpu_normal_equations.py).
"""
import numpy as np

from _gfbe_import import gf

abi, synth = gf.abi, gf.synth

LD = np.longdouble
U = 2.0 ** -53
NV = 73
ND = abi.DENSE_DIM
NF = abi.NFRAMES
LM_TILE, VIS_CHUNK = 64, 4                     # gfbe_device.h: landmarks per tile, tiles per wave of k_vis_chunk
GF_MIN_MU, GF_MIN_DIAG, GF_MAX_DIAG = 1e-8, 1e-6, 1e32      # gfbe_devutil.h == the oracle's trust-region loop (min_mu, min_diag, max_diag)

# oracle tangent layout (oracle/gfo_solver.cpp)
T_POSE = lambda k: 6 * k          # noqa: E731
T_EX, T_TD = 66, 72
T_SB = lambda k: 73 + 9 * k       # noqa: E731
T_EXW, T_SX, T_SY, T_SW, T_TDW = 172, 178, 179, 180, 181
T_PLR, T_PLZ = 182, 186
DIMS_IN_USE = 187                 # poses, extrinsic, td, speed-bias, wheel, ground plane; the rest are the GNSS blocks (anchor 187, yaw 190, rcv_dt 191, rcv_ddt 235)

# Largest |X_fp64 - X_ref| / (u A_X) over all cases, measured by tests/test_normal_equations_reference.py (which asserts them)
K_MEASURED = dict(H=69.0, g=67.0, Hll=2.4, gl=2.2, Hpl=2.7, E=13.0, eg=6.0)
K_MARGIN = 8.0
K = 1024.0                        # K_MARGIN x max(K_MEASURED) = 552, rounded up to a power of two
# The same measurement on the windows with GNSS, plane and anchor factors (gnss_window_cases.ne_case_names(); gfo_linearize includes those
# factors; g beyond its GNSS allowance): 8 x 14 = 112 -> 128, which is below K, so those windows are held to K as well.
# A pose pair with ONE visual factor (these windows have 60 landmarks) shows what a sum over hundreds hides: the per-factor visual
# blocks of two plain FP64 implementations — the oracle's, which the reference is summed from, and csrc/gfbe_factors.h compiled for the
# host — differ by up to VIS_BLOCK_MEASURED u of the block's largest entry (small entries of J are cancelling sums of terms of that
# size), which is hundreds of u of a small J^T J product. So, in these windows only, the entries the visual factors reach get the
# first-order allowance VIS_BLOCK_TOL V_H[a, b], V_H = sum_k Jmax_k sum_rows (|J_ka| + |J_kb|), V_g[a] = sum_k Jmax_k sum_rows (|r_k| + |J_ka|),
# VIS_BLOCK_TOL = 8 x the measured figure rounded up to a power of two (tests/test_gnss_reference.py measures and asserts it). The
# windows of tests/test_gpu_normal_equations.py keep their comparison without it.
# How it came about, and what it costs: it was introduced after the device had left K in three of these windows (anchor 4993, one_obs
# 1806, second 1240 u A_H, each in a pose pair with a single visual factor), and the CPU measurement above was made to find out whether the
# device or the reference was off; the host build of the device's arithmetic shows the same differences. It is NOT small against
# K u A_H: an absolute 500 u Jmax per Jacobian entry is, on an entry of H made of small Jacobian entries, a median of 40 and up to 2e4
# times K u A_H. It is zero on every entry no visual factor reaches (velocities, clocks, anchor, plane, wheel), and on the pose entries
# the GNSS observations reach it stays below 1e-5 of the GNSS share of A_H (4e-7 measured), in the window with ONE observation too (asserted in
# tests/test_gnss_reference.py) — the share of H this comparison exists for is held as tightly as without it. An absolute sum for the
# visual Jacobians that carried their internal cancellation, as A_J does for the line-of-sight differences, would be the cleaner scale.
VIS_BLOCK_MEASURED = 500.0
VIS_BLOCK_TOL = 4096.0 * U
# The SECOND linearisation is compared at the state a one-iteration solve hands back. In a window whose pose 0 is constant the gauge
# fix behind the solve (Estimator::double2vector; k_reanchor) is the identity, but the state still passes (P_i - P_0) + P_0 and a
# quaternion -> matrix -> quaternion round trip: it is the linearised state to STATE_ULPS_MEASURED u max(1, |P|) per component (measured on
# the CPU between the oracle's download and the independent loop's own state, tests/test_gnss_reference.py). Its first-order effect:
# dJ <= kappa Jmax |dx| with kappa = 8 for the Jacobians' relative change per unit of state (per radian; per metre over lever arms and
# depths of a metre and more), dr = J dx. state_tolerance() = K_MARGIN x STATE_ULPS_MEASURED u max(1, |P|) x kappa multiplies S_H, S_g.
STATE_ULPS_MEASURED = 5.0
STATE_KAPPA = 8.0


def state_tolerance(snap):
    return K_MARGIN * STATE_ULPS_MEASURED * U * max(1.0, float(np.abs(np.asarray(snap["pose"], float)[:, :3]).max())) * STATE_KAPPA


K_MEASURED_GNSS = dict(H=14.0, g=12.0, Hll=2.1, gl=2.1, Hpl=2.7, E=6.6, eg=3.6)
# Entries the IMU factors reach: the device's IMU blocks agree with the oracle's to IMU_BLOCK_TOL relative to the largest entry
# (tests/test_gpu_parity.py::test_factor_blocks_match_oracle: square-root information of a covariance of condition 1e12), so
# those entries get, on top of K u A, the first-order effect of such a difference on J^T J and J^T r, times the same margin:
#   K_MARGIN * IMU_BLOCK_TOL * I_H[a, b],   I_H[a, b] = sum_k Jmax sum_rows (|J_ka| + |J_kb|),   I_g[a] = sum_k (Jmax sum |r| + rmax sum |J_ka|)
# (Jmax, rmax: the scales of that test, max(1, max |.|) over the window's IMU blocks). Nothing else inherits it: E, eg and the entries
# of H no IMU factor reaches (poses two or more frames apart, extrinsic, td, wheel) have I = 0.
IMU_BLOCK_TOL = 1e-9
__doc__ = __doc__ % dict({k: "%.3g" % v for k, v in K_MEASURED.items()}, K="%g" % K)


def require_extended_precision():
    import pytest
    if np.finfo(LD).nmant < 63:
        pytest.skip("numpy.longdouble has a %d-bit mantissa on this host: no extended-precision reference" % np.finfo(LD).nmant)


def block_of(a):
    """Name of the parameter block tangent dim a belongs to (failure messages)."""
    if a < 66:
        return "pose %d" % (a // 6)
    if a < 72:
        return "extrinsic"
    if a == 72:
        return "td"
    if a < 172:
        return "speed-bias %d" % ((a - 73) // 9)
    if a < 182:
        return "wheel"
    if a < DIMS_IN_USE:
        return "ground plane"
    if a < 191:
        return "gnss anchor" if a < 190 else "gnss yaw"
    return "rcv_dt %d/%d" % ((a - 191) // 4, (a - 191) % 4) if a < 235 else "rcv_ddt %d" % (a - 235)


# ---------------------------------------------------------------------------------------------------------------- FP64 statement
def numpy_normal_equations(snap, ev):
    """H = sum J'J, g = sum J'r from the block-CSR factor outputs (robustified), plain FP64."""
    H, g = np.zeros((abi.DENSE_DIM, abi.DENSE_DIM)), np.zeros(abi.DENSE_DIM)
    L = len(snap["para_feature"])
    Hll, gl, Hpl = np.zeros(L), np.zeros(L), np.zeros((L, 73))
    for k in range(len(snap["vis_imu_i"])):
        i, j, l = snap["vis_imu_i"][k], snap["vis_imu_j"][k], snap["vis_feature_index"][k]
        cols = np.r_[T_POSE(i) + np.arange(6), T_POSE(j) + np.arange(6), T_EX + np.arange(6), T_TD]
        J = ev["vis_J"][k][:, np.r_[0:18, 19]]
        w = ev["vis_J"][k][:, 18]
        r = ev["vis_r"][k]
        H[np.ix_(cols, cols)] += J.T @ J
        g[cols] += J.T @ r
        Hll[l] += w @ w
        gl[l] += w @ r
        Hpl[l, cols] += J.T @ w
    for k, i in enumerate(snap["imu_frame"]):
        cols = np.r_[T_POSE(i) + np.arange(6), T_SB(i) + np.arange(9), T_POSE(i + 1) + np.arange(6), T_SB(i + 1) + np.arange(9)]
        J, r = ev["imu_J"][k], ev["imu_r"][k]
        H[np.ix_(cols, cols)] += J.T @ J
        g[cols] += J.T @ r
    for k, i in enumerate(snap.get("wheel_frame", [])):
        cols = np.r_[T_POSE(i) + np.arange(6), T_POSE(i + 1) + np.arange(6), T_EXW + np.arange(6), T_SX, T_SY, T_SW, T_TDW]
        J, r = ev["wheel_J"][k], ev["wheel_r"][k]
        H[np.ix_(cols, cols)] += J.T @ J
        g[cols] += J.T @ r
    return H, g, Hll, gl, Hpl


def lidar_blocks(snap, lio):
    """Per-factor (J [n, 6], r [n]) of the point-to-plane factors on pose lio["frame"], Huber-corrected (LidarPlaneNormFactor,
    lidarFactor.cpp:18-51; HuberLoss as in lidarodom.cpp:539), and the loss values rho."""
    x = snap["pose"][lio["frame"]]
    R, t = synth.qrot(x[3:]), x[:3]
    sw = lio["sqrt_info"] * lio["weights"]
    r = sw * ((lio["normals"] * (lio["pts"] @ R.T + t)).sum(axis=1) + lio["offsets"])
    nR = lio["normals"] @ R
    J = np.concatenate([sw[:, None] * lio["normals"], -sw[:, None] * np.cross(nR, lio["pts"])], axis=1)
    d = lio["huber_delta"]
    s = r * r
    rho = np.where(s <= d * d, s, 2 * d * np.sqrt(s) - d * d)
    scale = np.where(s <= d * d, 1.0, np.sqrt(d / np.sqrt(np.maximum(s, 1e-300))))
    return J * scale[:, None], r * scale, rho


# ---------------------------------------------------------------------------------------------------------------- the reference
def active_dims(snap):
    """Tangent dims of the reduced program: blocks some factor touches and that are not constant (Ceres drops the others;
    estimator.cpp:3294-3307 and the SetParameterBlockConstant flags; frames beyond frame_count are held)."""
    fc = int(snap.get("frame_count", abi.WINDOW_SIZE))
    used = set()
    for i in np.asarray(snap.get("imu_frame", []), int):
        used |= {abi.BLK_POSE0 + i, abi.BLK_SB0 + i, abi.BLK_POSE0 + i + 1, abi.BLK_SB0 + i + 1}
    for i in np.asarray(snap.get("wheel_frame", []), int):
        used |= {abi.BLK_POSE0 + i, abi.BLK_POSE0 + i + 1, abi.BLK_EX_WHEEL, abi.BLK_SX, abi.BLK_SY, abi.BLK_SW, abi.BLK_TD_WHEEL}
    if len(snap["vis_imu_i"]):
        used |= {abi.BLK_EX_CAM, abi.BLK_TD}
        used |= {abi.BLK_POSE0 + int(f) for f in np.unique(np.r_[snap["vis_imu_i"], snap["vis_imu_j"]])}
    pr = snap.get("prior")
    if pr is not None and pr.get("valid", 1) and pr["n"] > 0:
        used |= {int(b) for b in pr["block_id"]}
    if snap.get("lio") is not None and len(snap["lio"]["pts"]):
        used.add(abi.BLK_POSE0 + int(snap["lio"]["frame"]))
    if snap.get("plane") is not None and fc > 0:          # one PlaneFactor per pose i < frame_count (estimator.cpp:3214-3220)
        used |= {abi.BLK_POSE0 + i for i in range(fc)} | {abi.BLK_EX_WHEEL, abi.BLK_PLANE_R, abi.BLK_PLANE_Z}
    if snap.get("anchor") is not None:                    # PoseAnchorFactor on Pose[0] (estimator.cpp:3004-3012)
        used.add(abi.BLK_POSE0)
    if gnss_factors_on(snap):                             # estimator.cpp:3239-3291; without the factors (lowspeed) no GNSS dim is in the program
        for o in snap["gnss"]["obs"]:
            lo, fr = int(o["lower_idx"]), int(o["frame"])
            used |= {abi.BLK_POSE0 + lo, abi.BLK_SB0 + lo, abi.BLK_POSE0 + lo + 1, abi.BLK_SB0 + lo + 1, abi.BLK_RCV_DT0 + 4 * fr + int(o["sys_idx"]),
                     abi.BLK_RCV_DDT0 + fr, abi.BLK_YAW_ENU, abi.BLK_ANC_ECEF}
        used |= set(range(abi.BLK_RCV_DT0, abi.BLK_COUNT))      # the clock chains reach every rcv_dt / rcv_ddt, an unused constellation's too
    pose_const, sb_const = np.asarray(snap.get("pose_const", np.zeros(NF))), np.asarray(snap.get("sb_const", np.zeros(NF)))
    const = {abi.BLK_EX_CAM: snap.get("ex_cam_const", 1), abi.BLK_EX_WHEEL: snap.get("ex_wheel_const", 0), abi.BLK_TD: snap.get("td_const", 1),
             abi.BLK_TD_WHEEL: snap.get("td_wheel_const", 1)}
    for b in (abi.BLK_SX, abi.BLK_SY, abi.BLK_SW):
        const[b] = snap.get("ix_wheel_const", 1)
    const[abi.BLK_PLANE_R] = const[abi.BLK_PLANE_Z] = (snap.get("plane") or {}).get("const", 0)
    gn = snap.get("gnss")
    const[abi.BLK_YAW_ENU] = gn is not None and int(gn.get("ready", 1)) != 0      # held constant in a gnss_ready window (estimator.cpp:2991)
    const[abi.BLK_ANC_ECEF] = 0
    for b in range(abi.BLK_RCV_DT0, abi.BLK_COUNT):
        const[b] = 0
    for f in range(NF):
        const[abi.BLK_POSE0 + f] = pose_const[f] or f > fc
        const[abi.BLK_SB0 + f] = sb_const[f] or f > fc
    act = np.zeros(ND, bool)
    for b in used:
        if not const[b]:
            o = abi.block_tangent_offset(b)
            act[o:o + abi.block_local_size(b)] = True
    act[T_PLR + 3] = False      # the plane quaternion's fourth slot exists in the prior only (three tangent dims in the solve)
    return act


def gnss_factors_on(snap):
    """gnss_ready && !lowspeed (estimator.cpp:2965-2984, 3239): the mean absolute horizontal velocity over the window, as a vector."""
    gn = snap.get("gnss")
    if gn is None or not int(gn.get("ready", 1)):
        return False
    v = np.abs(np.asarray(snap["speed_bias"], float)[:, :2]).sum(axis=0) / NF
    return not np.sqrt(v[0] * v[0] + v[1] * v[1]) < 0.3


def gnss_case_of(snap):
    """The GNSS part of a window as a case of tests/gnss_np.py (the stand-alone evaluator's arguments)."""
    gn, gs = snap["gnss"], snap["gnss_state"]
    return dict(obs=gn["obs"], iono=gn.get("iono"), pose=np.asarray(snap["pose"], float), speed_bias=np.asarray(snap["speed_bias"], float),
                rcv_dt=np.asarray(gs["rcv_dt"], float), rcv_ddt=np.asarray(gs["rcv_ddt"], float), yaw=float(gs["yaw_enu_local"]),
                anc=np.asarray(gs["anc_ecef"], float), frame_dt=np.asarray(gn["frame_dt"], float), ddt_weight=float(gn["ddt_weight"]))


def gnss_blocks(snap, defect=None):
    """[(r, A_r, J, A_J, tangent dims)] of the GNSS residual blocks of a window in longdouble, from the model of tests/gnss_np.py (NOT
    from the oracle's FP64 rows) through the block and column tables of tests/test_gnss_solve_oracle.py::gnss_rows: pseudo-range /
    Doppler per observation (the leading three columns of the two poses and speed-biases it interpolates between, its constellation's
    rcv_dt and the rcv_ddt of its frame, yaw, anchor), then the DtDdt chains constellation-major and the DdtSmooth chain, whose
    Jacobians are the constants [-50, 50, -25 dt, -25 dt] and [w, -w]. defect: a wrong assembly (tests/test_gnss_reference.py)."""
    import gnss_np as gn_
    c = gnss_case_of(snap)
    e = gn_.eval_case(c, LD, iono=c["iono"])
    TOFF = abi.block_tangent_offset
    out = []
    for k, o in enumerate(c["obs"]):
        lo, fr, sys = int(o["lower_idx"]), int(o["frame"]), int(o["sys_idx"])
        if defect == "swap_constellations":
            sys = {0: 1, 1: 0}.get(sys, sys)
        cols = np.r_[TOFF(abi.BLK_POSE0 + lo) + np.arange(3), TOFF(abi.BLK_SB0 + lo) + np.arange(3), TOFF(abi.BLK_POSE0 + lo + 1) + np.arange(3),
                     TOFF(abi.BLK_SB0 + lo + 1) + np.arange(3), TOFF(abi.BLK_RCV_DT0 + 4 * fr + sys), TOFF(abi.BLK_RCV_DDT0 + fr), TOFF(abi.BLK_YAW_ENU),
                     TOFF(abi.BLK_ANC_ECEF) + np.arange(3)]
        J, AJ = e["J"][k].copy(), e["A_J"][k].copy()
        if defect == "drop_lower_pose" and lo == fr - 1:        # an observation of frame i between poses i - 1 and i: lost from the sums of pose i - 1
            J[:, 0:6] = 0
        out.append((e["r"][k], e["A_r"][k], J, AJ, cols, gn_.K_R))
    fdt, wgt = [LD(v) for v in c["frame_dt"]], LD(c["ddt_weight"])
    for s in range(4):
        for i in range(0 if defect != "no_first_interval" else 1, abi.WINDOW_SIZE):
            J = np.array([[LD(-50), LD(50), LD(-25) * fdt[i], LD(-25) * fdt[i]]], LD)
            cols = np.r_[TOFF(abi.BLK_RCV_DT0 + 4 * i + s), TOFF(abi.BLK_RCV_DT0 + 4 * (i + 1) + s), TOFF(abi.BLK_RCV_DDT0 + i), TOFF(abi.BLK_RCV_DDT0 + i + 1)]
            out.append((e["r_dt_ddt"][s, i:i + 1], e["A_dt_ddt"][s, i:i + 1], J, np.abs(J), cols, gn_.K_CLK))
    for i in range(0 if defect != "no_first_interval" else 1, abi.WINDOW_SIZE):
        J = np.array([[wgt, -wgt]], LD)
        out.append((e["r_smooth"][i:i + 1], e["A_smooth"][i:i + 1], J, np.abs(J), np.r_[TOFF(abi.BLK_RCV_DDT0 + i), TOFF(abi.BLK_RCV_DDT0 + i + 1)], gn_.K_CLK))
    return out


def idle_landmarks(snap):
    """Landmarks that are not in the reduced program: constant ones and those without any factor (weight zero in the Schur term)."""
    L = len(snap["para_feature"])
    has = np.zeros(L, bool)
    has[np.asarray(snap["vis_feature_index"], int)] = True
    return ~has | (np.asarray(snap.get("feature_const", np.zeros(L))) != 0)


class _Acc:
    """H / g (and their absolute sums) in longdouble."""

    def __init__(self):
        self.H, self.g = np.zeros((ND, ND), LD), np.zeros(ND, LD)
        self.AH, self.Ag = np.zeros((ND, ND), LD), np.zeros(ND, LD)
        self.IH, self.Ig = np.zeros((ND, ND)), np.zeros(ND)
        self.Gg = np.zeros(ND, LD)      # absolute allowance in g for the GNSS residuals' own rounding (see add_gnss)
        self.VH, self.Vg = np.zeros((ND, ND)), np.zeros(ND)      # scale of the visual blocks' own FP64 rounding (see VIS_BLOCK_TOL)
        self.SH, self.Sg = np.zeros((ND, ND)), np.zeros(ND)      # scale of a perturbation of the STATE, every factor kind (see state_tolerance)

    def state_scale(self, aJ, ar, cols):
        """aJ [k, rows, c], ar [k, rows] (absolute values, float): S_H[a, b] += sum_k Jmax_k sum_rows (|J_ka| + |J_kb|),
        S_g[a] += sum_k Jmax_k (sum |r_k| + c sum_rows |J_ka|) — d(J^T J) and d(J^T r) for dJ <= tol Jmax and dr = J dx <= tol c Jmax."""
        Jmax = aJ.max(axis=(1, 2))
        cs = (Jmax[:, None] * aJ.sum(axis=1)).sum(axis=0)
        self.SH[np.ix_(cols, cols)] += cs[:, None] + cs[None, :]
        self.Sg[cols] += aJ.shape[2] * cs + (Jmax * ar.sum(axis=1)).sum()

    def vis_allowance(self, J, w, r, cols):
        J, w, r = np.abs(np.asarray(J, float)), np.abs(np.asarray(w, float)), np.abs(np.asarray(r, float))
        Jmax = np.maximum(J.max(axis=(1, 2)), w.max(axis=1))
        cs = (Jmax[:, None] * J.sum(axis=1)).sum(axis=0)
        self.VH[np.ix_(cols, cols)] += cs[:, None] + cs[None, :]
        self.Vg[cols] += cs + (Jmax * r.sum(axis=1)).sum()

    def imu_allowance(self, J, r, cols, Jmax, rmax):
        cs, rs = np.abs(J).sum(axis=0), np.abs(r).sum()
        self.IH[np.ix_(cols, cols)] += Jmax * (cs[:, None] + cs[None, :])
        self.Ig[cols] += Jmax * rs + rmax * cs

    def add_gnss(self, r, Ar, J, AJ, cols, K_res):
        """One GNSS residual block from the model: the scales are the model's own absolute sums (A_J carries the weights' conditioning
        on the elevation, so H needs nothing beyond K u A_H). A GNSS residual carries its own rounding, K_res u A_r — 1e-9 and more
        of r, which is the difference of numbers of 2.5e7 —: g gets the first-order allowance sum_k |J_ka| K_res u A_r,k, which is
        separate from the IMU blocks' and not multiplied by IMU_BLOCK_TOL."""
        ix = np.ix_(cols, cols)
        aJ = np.abs(J)
        self.H[ix] += J.T @ J
        self.AH[ix] += AJ.T @ AJ
        self.g[cols] += J.T @ r
        self.Ag[cols] += AJ.T @ np.abs(r)
        self.Gg[cols] += aJ.T @ (LD(K_res) * LD(U) * Ar)
        self.state_scale(np.asarray(aJ, float)[None], np.abs(np.asarray(r, float))[None], cols)

    def add(self, J, r, cols):
        """J [n, rows, c] or [rows, c], r alike without the last axis: every factor's J^T J, J^T r at the tangent dims cols."""
        J, r = np.asarray(J, LD), np.asarray(r, LD)
        if J.ndim == 2:
            J, r = J[None], r[None]
        aJ, ar = np.abs(J), np.abs(r)
        ix = np.ix_(cols, cols)
        self.H[ix] += np.einsum("kra,krb->ab", J, J)
        self.AH[ix] += np.einsum("kra,krb->ab", aJ, aJ)
        self.g[cols] += np.einsum("kra,kr->a", J, r)
        self.Ag[cols] += np.einsum("kra,kr->a", aJ, ar)
        self.state_scale(np.asarray(aJ, float), np.asarray(ar, float), cols)


def optional_blocks(snap):
    """[(J, r, tangent dims)] of the PlaneFactors (poses 0 .. frame_count - 1: pose, wheel extrinsic, plane_R (3), plane_Z) and of the
    PoseAnchorFactor on pose 0, from the oracle's stand-alone evaluators like the other factor kinds (tests/test_gpu_optional.py holds
    the device's to them at 1e-13)."""
    out = []
    fc = int(snap.get("frame_count", abi.WINDOW_SIZE))
    if snap.get("plane") is None and snap.get("anchor") is None:
        return out
    import oracle_lib          # (only a window with one of the two factor kinds needs the oracle here)
    orc = oracle_lib.load()
    if snap.get("plane") is not None and fc > 0:
        e = abi.plane_eval(orc.lib, "gfo_", None, np.asarray(snap["pose"])[:fc], snap["ex_pose_wheel"], snap.get("plane_R", [0, 0, 0, 1.0]),
                           float(snap.get("plane_Z", 0.0)), snap["plane"]["noise_inv"])
        for i in range(fc):
            out.append((e["J"][i], e["r"][i], np.r_[T_POSE(i) + np.arange(6), T_EXW + np.arange(6), T_PLR + np.arange(3), T_PLZ]))
    if snap.get("anchor") is not None:
        e = abi.anchor_eval(orc.lib, "gfo_", None, np.asarray(snap["pose"])[:1], np.asarray(snap["anchor"]["pose"])[None], float(snap["anchor"].get("sqrt_info", 120.0)))
        out.append((e["J"][0], e["r"][0], T_POSE(0) + np.arange(6)))
    return out


def reference_normal_equations(snap, ev, gnss_defect=None):
    """The normal equations of snap at its state from the per-factor blocks ev = oracle.eval_factors(snap, robustify=True) — the GNSS
    blocks from the extended-precision model of tests/gnss_np.py instead, the plane and anchor blocks from the oracle's stand-alone
    evaluators —, summed in numpy.longdouble: dict with H, g [ND], Hll, gl [L], Hpl [L, 73] (constant dims removed, rows of idle landmarks zero), their absolute
    sums A_H, A_g, A_Hll, A_gl, A_Hpl, the mask act of the dims in the reduced program and idle, the landmarks outside it."""
    acc = _Acc()
    L = len(snap["para_feature"])
    Hll, gl, Agl = np.zeros(L, LD), np.zeros(L, LD), np.zeros(L, LD)
    Hpl, AHpl = np.zeros((L, NV), LD), np.zeros((L, NV), LD)
    vi, vj, vl = (np.asarray(snap[k], int) for k in ("vis_imu_i", "vis_imu_j", "vis_feature_index"))
    vJ, vr = np.asarray(ev["vis_J"], LD), np.asarray(ev["vis_r"], LD)
    for i, j in sorted(set(zip(vi.tolist(), vj.tolist()))):
        sel = np.where((vi == i) & (vj == j))[0]
        cols = np.r_[T_POSE(i) + np.arange(6), T_POSE(j) + np.arange(6), T_EX + np.arange(6), T_TD]
        J, w, r, l = vJ[sel][:, :, np.r_[0:18, 19]], vJ[sel][:, :, 18], vr[sel], vl[sel]
        acc.add(J, r, cols)
        acc.vis_allowance(J, w, r, cols)
        np.add.at(Hll, l, (w * w).sum(axis=1))
        np.add.at(gl, l, (w * r).sum(axis=1))
        np.add.at(Agl, l, np.abs(w * r).sum(axis=1))
        np.add.at(Hpl, (l[:, None], cols[None, :]), np.einsum("kra,kr->ka", J, w))
        np.add.at(AHpl, (l[:, None], cols[None, :]), np.einsum("kra,kr->ka", np.abs(J), np.abs(w)))
    for k, i in enumerate(np.asarray(snap.get("imu_frame", []), int)):
        cols = np.r_[T_POSE(i) + np.arange(6), T_SB(i) + np.arange(9), T_POSE(i + 1) + np.arange(6), T_SB(i + 1) + np.arange(9)]
        acc.add(ev["imu_J"][k], ev["imu_r"][k], cols)
        acc.imu_allowance(ev["imu_J"][k], ev["imu_r"][k], cols, max(1.0, np.abs(ev["imu_J"]).max()), max(1.0, np.abs(ev["imu_r"]).max()))
    for k, i in enumerate(np.asarray(snap.get("wheel_frame", []), int)):
        cols = np.r_[T_POSE(i) + np.arange(6), T_POSE(i + 1) + np.arange(6), T_EXW + np.arange(6), T_SX, T_SY, T_SW, T_TDW]
        acc.add(ev["wheel_J"][k], ev["wheel_r"][k], cols)
    pr = snap.get("prior")
    if pr is not None and pr.get("valid", 1) and pr["n"] > 0:      # the prior's share: J0^T J0, J0^T prior_r, placed by its block table
        cols = np.full(pr["n"], -1)
        for b, o in zip(pr["block_id"], pr["block_idx"]):
            n = abi.block_local_size(int(b))
            cols[o:o + n] = abi.block_tangent_offset(int(b)) + np.arange(n)
        assert (cols >= 0).all()
        acc.add(np.asarray(pr["J0"]).reshape(pr["n"], pr["n"]), ev["prior_r"], cols)
    if snap.get("lio") is not None and len(snap["lio"]["pts"]):
        J, r, _ = lidar_blocks(snap, snap["lio"])
        acc.add(J[:, None, :], r[:, None], T_POSE(int(snap["lio"]["frame"])) + np.arange(6))
    for J, r, cols in optional_blocks(snap):
        acc.add(J, r, cols)
    if gnss_factors_on(snap):
        for blk in gnss_blocks(snap, gnss_defect):
            acc.add_gnss(*blk)
    act, idle = active_dims(snap), idle_landmarks(snap)
    off = ~act
    for X in (acc.H, acc.AH, acc.IH, acc.VH, acc.SH):
        X[off, :] = 0
        X[:, off] = 0
    for X in (acc.g, acc.Ag, acc.Ig, acc.Gg, acc.Vg, acc.Sg):
        X[off] = 0
    for X in (Hpl, AHpl):
        X[:, off[:NV]] = 0
        X[idle] = 0
    for X in (Hll, gl, Agl):
        X[idle] = 0
    return dict(H=acc.H, g=acc.g, Hll=Hll, gl=gl, Hpl=Hpl, A_H=acc.AH, A_g=acc.Ag, A_Hll=Hll.copy(), A_gl=Agl, A_Hpl=AHpl, I_H=acc.IH, I_g=acc.Ig,
                G_g=acc.Gg, V_H=acc.VH, V_g=acc.Vg, S_H=acc.SH, S_g=acc.Sg, act=act, idle=idle)


def landmark_weights(Hll, mu, jacobi_scaling, idle_mask, clamp=True):
    """w_l = s_l^2 / (s_l^2 Hll + mu clamp(s_l^2 Hll)), s_l = 1 / (1 + sqrt(Hll)) (1 without Jacobi scaling): the inverse of the
    landmark's mu-regularised diagonal, back in unscaled landmark coordinates. Zero for idle landmarks. In the dtype of Hll."""
    Hll = np.asarray(Hll)
    one = Hll.dtype.type(1)
    s = one / (one + np.sqrt(Hll)) if jacobi_scaling else np.ones_like(Hll)
    hs2 = s * s * Hll
    d2 = np.clip(hs2, Hll.dtype.type(GF_MIN_DIAG), Hll.dtype.type(GF_MAX_DIAG)) if clamp else hs2
    den = hs2 + Hll.dtype.type(mu) * d2
    ok = ~np.asarray(idle_mask, bool) & (den > 0)
    return np.where(ok, s * s / np.where(ok, den, one), Hll.dtype.type(0))


def schur_reference(Hll, gl, Hpl, mu, jacobi_scaling, idle_mask, A_Hpl=None, A_gl=None, clamp=True):
    """E = sum_l w_l h_l h_l^T, eg = sum_l w_l h_l gl_l in the dtype of the inputs (longdouble for the reference), and the scales
    A_E = sum_l w_l a_l a_l^T, A_eg = sum_l w_l a_l A_gl_l with a_l = A_Hpl[l] (|h_l| when no absolute sums are given)."""
    w = landmark_weights(Hll, mu, jacobi_scaling, idle_mask, clamp)
    a = np.abs(Hpl) if A_Hpl is None else A_Hpl
    ag = np.abs(gl) if A_gl is None else A_gl
    return (Hpl * w[:, None]).T @ Hpl, Hpl.T @ (w * gl), (a * w[:, None]).T @ a, a.T @ (w * ag)


def reference_system(snap, ev, mu=GF_MIN_MU, jacobi_scaling=True, gnss_defect=None):
    """reference_normal_equations plus the Schur term of the first iteration (mu = the minimum, the trust-region loop's start)."""
    ref = reference_normal_equations(snap, ev, gnss_defect)
    ref["E"], ref["eg"], ref["A_E"], ref["A_eg"] = schur_reference(ref["Hll"], ref["gl"], ref["Hpl"], mu, jacobi_scaling, ref["idle"], ref["A_Hpl"], ref["A_gl"])
    return ref


def worst_ratio(name, X, Xref, A, lower=False, allow=None):
    """Entrywise comparison of X with the reference: (largest max(|X - Xref| - allow, 0) / (u A) over the entries with A > 0,
    description of that entry, number of entries with A == 0 that are not exactly 0.0, description of the first of them).
    lower: only j <= i. allow: an absolute allowance per entry (the IMU blocks'), none by default."""
    X, Xref, A = np.asarray(X, LD), np.asarray(Xref, LD), np.asarray(A, LD)
    if A.size == 0:
        return 0.0, name + ": empty", 0, ""
    use = np.ones(A.shape, bool) if not lower else np.tril(np.ones(A.shape, bool))
    pos = use & (A > 0)
    ratio = np.zeros(A.shape)
    err = np.abs(X - Xref) if allow is None else np.maximum(np.abs(X - Xref) - np.asarray(allow, LD), 0)
    ratio[pos] = (err[pos] / (LD(U) * A[pos])).astype(float)
    ratio[pos & ~np.isfinite(np.asarray(X, float))] = np.inf

    def where(ix):
        ix = tuple(int(q) for q in ix)
        blocks = " x ".join(block_of(q) for q in ix) if name in ("H", "g", "E", "eg") else "landmark %d" % ix[0]
        return "%s%s (%s): got %.17g want %.17g scale %.3g" % (name, list(ix), blocks, float(X[ix]), float(Xref[ix]), float(A[ix]))
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    bad0 = use & (A == 0) & (np.asarray(X, float) != 0.0)
    first0 = where(np.argwhere(bad0)[0]) if bad0.any() else ""
    return float(ratio[worst]), where(worst) + " ratio %.3g" % ratio[worst], int(bad0.sum()), first0


def compare_system(got, ref, K_bound, label="", names=("H", "g", "E", "eg"), vis_block_tol=0.0, state_tol=0.0):
    """got: dict with H [ND, ND] (lower triangle), g [ND], E [73, 73], eg [73]. Returns (ratios per array, list of failure messages):
    an entry outside K_bound u A (plus, in H and g, the allowance of the IMU blocks and, in g, of the GNSS residuals), or a non-zero
    where the reference has a structural zero."""
    ratios, fails = {}, []
    for name in names:
        allow = K_MARGIN * IMU_BLOCK_TOL * ref["I_" + name] if name in ("H", "g") else None
        if name == "g" and "G_g" in ref:
            allow = np.asarray(allow, LD) + ref["G_g"]
        if vis_block_tol and name in ("H", "g"):
            allow = np.asarray(allow, LD) + vis_block_tol * ref["V_" + name]
        if state_tol and name in ("H", "g"):
            allow = np.asarray(allow, LD) + state_tol * ref["S_" + name]
        r, where, n0, first0 = worst_ratio(name, got[name], ref[name], ref["A_" + name], lower=name in ("H", "E"), allow=allow)
        ratios[name] = r
        if not r <= K_bound:
            fails.append("%s worst entry %s > K = %g" % (label, where, K_bound))
        if n0:
            fails.append("%s %d structural zeros of %s are not 0.0, first %s" % (label, n0, name, first0))
    return ratios, fails


# ---------------------------------------------------------------------------------------------------------------- windows
def visual_factors_any_length(fl):
    """synth.build_visual_factors_np without its four-observation threshold: k-th feature with at least ONE observation <->
    para_Feature[k]; a feature with a single observation is a landmark without factors. (The C ABI takes any contiguous track of
    1..10 factors; the reference's list never holds a track under four observations.)"""
    idx, ii, jj, pi, pj, vi, vj, tdi, tdj, lam, fconst = [], [], [], [], [], [], [], [], [], [], []
    off = 0
    for k in range(len(fl["n_obs"])):
        n, s = int(fl["n_obs"][k]), int(fl["start_frame"][k])
        rows, tds = fl["obs"][off:off + n], fl["obs_td"][off:off + n]
        off += n
        lam.append(1.0 / fl["estimated_depth"][k])
        fconst.append(1 if fl["estimate_flag"][k] == 1 else 0)
        for o in range(1, n):
            idx.append(k); ii.append(s); jj.append(s + o)
            pi.append(rows[0, :3]); pj.append(rows[o, :3]); vi.append(rows[0, 5:7]); vj.append(rows[o, 5:7])
            tdi.append(tds[0]); tdj.append(tds[o])
    return dict(vis_feature_index=np.array(idx, np.int32), vis_imu_i=np.array(ii, np.int32), vis_imu_j=np.array(jj, np.int32),
                vis_pts_i=np.array(pi).reshape(-1, 3), vis_pts_j=np.array(pj).reshape(-1, 3), vis_vel_i=np.array(vi).reshape(-1, 2),
                vis_vel_j=np.array(vj).reshape(-1, 2), vis_td_i=np.array(tdi, float), vis_td_j=np.array(tdj, float),
                para_feature=np.array(lam, float), feature_const=np.array(fconst, np.uint8))


def shaped_window(scn, k0, counts, n_idle=0, frame_count=abi.WINDOW_SIZE, state=None, shuffle_seed=0):
    """A window of scn whose number of landmarks per (start frame s, number of factors m) is counts[(s, m)], m in 1 .. 10 - s, plus
    n_idle landmarks without any factor: features of scn.feature_list(k0) with their tracks cut short and, where no feature starts
    in s (s = 8, 9) or too few do, with their leading observations dropped (the initial inverse depth then belongs to another frame:
    these windows are linearised, not solved). The landmarks come in a shuffled order (the device sorts them itself)."""
    fl = scn.feature_list(k0)
    start, n_obs = fl["start_frame"], fl["n_obs"]
    off = np.r_[0, np.cumsum(n_obs)]
    free = np.ones(len(start), bool)
    picked = []                                             # (feature, observations dropped at the front, observations kept)
    for (s, m) in sorted(counts, key=lambda sm: (-(sm[0] + sm[1]), sm[0])):       # the tracks that end latest first: they have the fewest sources
        assert 0 <= s and 1 <= m and s + m <= frame_count, (s, m)
        fits = free & (start <= s) & (start + n_obs >= s + m + 1)
        order = np.argsort(np.where(fits, s - start, 99), kind="stable")          # a feature that starts in s itself before one cut at the front
        take = order[:counts[(s, m)]]
        assert fits[take].all(), "scenario too small for %d landmarks of start frame %d with %d factors" % (counts[(s, m)], s, m)
        free[take] = False
        picked += [(int(f), s - int(start[f]), m + 1) for f in take]
    for _ in range(n_idle):                                 # a single observation: a landmark, no factor
        f = int(np.argmax(free))
        assert free[f]
        free[f] = False
        picked.append((f, 0, 1))
    rng = np.random.default_rng(shuffle_seed)
    picked = [picked[q] for q in rng.permutation(len(picked))]
    rows = np.concatenate([np.arange(off[f] + d, off[f] + d + n) for f, d, n in picked]) if picked else np.zeros(0, int)
    feats = np.array([f for f, _, _ in picked], int)
    cut = dict(start_frame=np.array([start[f] + d for f, d, _ in picked], np.int32), n_obs=np.array([n for _, _, n in picked], np.int32),
               obs=fl["obs"][rows].reshape(-1, 7), obs_td=fl["obs_td"][rows], estimated_depth=fl["estimated_depth"][feats],
               estimate_flag=fl["estimate_flag"][feats])
    snap = scn.window(k0, state=state, factors=visual_factors_any_length(cut))
    if frame_count < abi.WINDOW_SIZE:
        trim_to_frame_count(snap, frame_count)
    return snap


def trim_to_frame_count(snap, fc):
    """A window that is still filling up: frames 0 .. fc, the factors that reach beyond dropped (their landmarks stay)."""
    keep = np.asarray(snap["vis_imu_j"]) <= fc
    for k in list(snap):
        if k.startswith("vis_"):
            snap[k] = snap[k][keep]
    snap["frame_count"] = fc
    for k in ("imu", "wheel"):
        if k in snap:
            snap[k], snap[k + "_frame"] = snap[k][:fc], snap[k + "_frame"][:fc]
    return snap


def layout_counts(snap):
    """{(start frame, number of factors): landmarks} of a window as scan_window (gfbe_upload.h) bins them: a landmark without factors
    counts for start frame 0 with 0 factors."""
    L = len(snap["para_feature"])
    m = np.bincount(np.asarray(snap["vis_feature_index"], int), minlength=L)
    s = np.zeros(L, int)
    s[np.asarray(snap["vis_feature_index"], int)] = np.asarray(snap["vis_imu_i"], int)
    out = {}
    for key in zip(s.tolist(), m.tolist()):
        out[key] = out.get(key, 0) + 1
    return out


def per_start_frame(counts):
    out = [0] * NF
    for (s, m), n in counts.items():
        if m > 0:
            out[s] += n
    return out


def _spread(total, s, lengths):
    """total landmarks of start frame s dealt over the track lengths (numbers of factors) `lengths`, the first ones get the rest."""
    lengths = [m for q, m in enumerate(lengths) if 1 <= m <= 10 - s and m not in lengths[:q]]
    share = [total // len(lengths) + (1 if q < total % len(lengths) else 0) for q in range(len(lengths))]
    return {(s, m): n for m, n in zip(lengths, share) if n}


def window_with_prior(oracle, seed, L, use_wheel=True):
    scn = synth.Scenario(seed=seed, n_landmarks=L, use_wheel=use_wheel)
    resA = oracle.solve(scn.window(0), abi.MARGIN_OLD)
    stB = synth.shift_state_for_next_window(scn, resA["state"], 1)
    return scn, scn.window(1, state=stB, prior=resA["prior"])


# landmarks per start frame 0..9 of the cases that prescribe them (tests/test_normal_equations_reference.py checks the windows against these)
CASE_PER_START = {
    "tile_edges": [64, 65, 63, 1, 0, 128, 129, 0, 2, 1, 0],
    "chunk_edges": [0, LM_TILE * VIS_CHUNK, 0, LM_TILE * VIS_CHUNK + 1, 0, 2 * LM_TILE * VIS_CHUNK + 1, 0, 0, 0, 0, 0],
    "one_group_0": [300, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    "one_group_2": [0, 0, 200, 0, 0, 0, 0, 0, 0, 0, 0],
    "one_group_4": [0, 0, 0, 0, 130, 0, 0, 0, 0, 0, 0],
    "one_group_7": [0, 0, 0, 0, 0, 0, 0, 70, 0, 0, 0],
    "short_tracks": [70, 30, 64, 20, 65, 10, 5, 40, 3, 2, 0],
}
_cache = {}


def case_names():
    return list(CASE_PER_START) + ["no_landmarks", "idle_landmarks", "full_columns", "robust", "partial", "prior_wheel_2k", "soak_349"]


def case_counts(name):
    """The prescribed {(start frame, factors): landmarks} of a shaped case."""
    per = CASE_PER_START[name]
    out = {}
    for s, n in enumerate(per):
        if not n:
            continue
        if name == "short_tracks":
            out[(s, 1)] = n
        elif name == "tile_edges":       # every start frame holds tracks of several lengths, the longest possible among them; start frames 8, 9: two- and one-factor tracks
            out.update(_spread(n, s, [10 - s, 3, 5, 1, 7] if s < 8 else [10 - s, 1]))
        else:
            out.update(_spread(n, s, [10 - s, 3, 4, 6, 2]))
    return out


def build_case(name, oracle):
    """The window of case `name` (see the table in tests/test_gpu_normal_equations.py). Deterministic; cached per process."""
    if name in _cache:
        return _cache[name]
    seed = 7000 + case_names().index(name)
    if name in CASE_PER_START:
        counts = case_counts(name)
        scn = synth.Scenario(seed=seed, n_landmarks=12 * sum(counts.values()) + 1500, use_wheel=name != "one_group_2")
        snap = shaped_window(scn, 0, counts)
    elif name == "no_landmarks":
        scn = synth.Scenario(seed=seed, n_landmarks=40, use_wheel=True)
        snap = shaped_window(scn, 0, {})
    elif name == "idle_landmarks":       # every third landmark constant, every fifth without any factor
        scn = synth.Scenario(seed=seed, n_landmarks=3000, use_wheel=True)
        snap = shaped_window(scn, 0, {(0, 10): 20, (0, 4): 50, (1, 5): 70, (2, 3): 40, (3, 7): 30, (5, 2): 45, (6, 4): 25, (8, 2): 10, (9, 1): 10})
        L = len(snap["para_feature"])
        keep = np.asarray(snap["vis_feature_index"]) % 5 != 4
        for k in list(snap):
            if k.startswith("vis_"):
                snap[k] = snap[k][keep]
        snap["feature_const"] = (np.arange(L) % 3 == 0).astype(np.uint8)
    elif name == "full_columns":         # camera extrinsic and td free: the uncompressed row format; stamps that differ from td
        scn = synth.Scenario(seed=seed, n_landmarks=3000, use_wheel=True)
        snap = shaped_window(scn, 0, {(0, 10): 30, (0, 5): 40, (1, 9): 10, (2, 4): 66, (4, 6): 50, (6, 3): 64, (7, 3): 30, (8, 1): 5})
        snap["ex_cam_const"], snap["td_const"] = 0, 0
        snap["td"] = 0.004
        snap["vis_td_j"] = np.asarray(snap["vis_td_j"], float) + 0.001 * (np.arange(len(snap["vis_td_j"])) % 3)
    elif name == "robust":               # 5 % of the observations displaced by 20 px, the others 0.5 px of noise around the true state and depths
        scn = synth.Scenario(seed=seed, n_landmarks=3000, use_wheel=True, noise=False)
        snap = shaped_window(scn, 0, {(0, 10): 10, (0, 6): 60, (1, 4): 80, (2, 8): 30, (3, 3): 70, (5, 5): 40, (7, 3): 60})
        rng = np.random.default_rng(seed)
        K = len(snap["vis_imu_i"])
        hit = rng.random(K) < 0.05
        ang = rng.uniform(0, 2 * np.pi, K)
        snap["vis_pts_j"] = snap["vis_pts_j"].copy()
        snap["vis_pts_j"][:, :2] += rng.normal(0, 0.5 / synth.FOCAL, (K, 2))
        snap["vis_pts_j"][hit, :2] += (20.0 / synth.FOCAL) * np.c_[np.cos(ang), np.sin(ang)][hit]
    elif name == "partial":
        scn = synth.Scenario(seed=seed, n_landmarks=3000, use_wheel=True)
        snap = shaped_window(scn, 0, {(0, 6): 40, (0, 3): 30, (1, 5): 64, (2, 2): 20, (3, 3): 65, (5, 1): 12}, frame_count=6)
    elif name == "prior_wheel_2k":       # the bench shape
        _, snap = window_with_prior(oracle, 20250709, 2000)
    elif name == "soak_349":             # L = 3500, a LiDAR block, a third of the landmarks constant, a window that is still filling up
        scn = synth.Scenario(seed=seed, n_landmarks=3500, use_wheel=True)
        snap = trim_to_frame_count(scn.window(0), 7)
        snap["lio"] = synth.lidar_block(scn, 0, n=700, seed=4, outliers=0.05, frame=7)
        snap["feature_const"] = (np.arange(3500) % 3 == 0).astype(np.uint8)
    else:
        raise KeyError(name)
    _cache[name] = snap
    return snap


_ref_cache = {}


def case_reference(name, oracle):
    """(window, per-factor blocks of the oracle, extended-precision reference system) of a case; cached per process."""
    if name not in _ref_cache:
        snap = build_case(name, oracle)
        ev = oracle.eval_factors(snap, robustify=True)
        _ref_cache[name] = (snap, ev, reference_system(snap, ev))
    return _ref_cache[name]


def fp64_system(oracle, snap, lin=None):
    """The same sums in plain FP64: the oracle's gfo_linearize for H, g, Hll, gl, Hpl and a numpy contraction for E, eg."""
    lin = lin or oracle.linearize(snap)
    idle = idle_landmarks(snap)
    E, eg, _, _ = schur_reference(lin["Hll"], lin["gl"], lin["Hpl"], GF_MIN_MU, True, idle)
    return dict(lin, E=E, eg=eg)


def device_system(batch, w):
    """H (all rows), g, E (all rows), eg of window w of a batch after one iteration, through gfbe_debug_vector."""
    H = np.array([batch.debug_vector(1000 + r, w) for r in range(ND)])
    E = np.array([batch.debug_vector(2000 + r, w)[:NV] for r in range(NV)])
    return dict(H=H, g=batch.debug_vector(3, w), E=E, eg=batch.debug_vector(2000 + NV, w)[:NV])
