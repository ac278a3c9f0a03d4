"""Numpy model of the device-resident LiDAR scan (the checker of gfbe_scan_*), written from the reference's host steps between the
driver's cloud and lidarodom::optimize: subSampleFrame (lio/src/common/utility.cpp:34-54), PoseInterp (common/math_utils.h:530-585),
Undistort (liw/lio/lidarodom.cpp:1578-1600), transformPoint + gridSampling (common/utility.cpp:56-111), with the rules include/gfbe.h
(f4d) states:

  voxel key      (short)(p / size) per axis, truncated toward zero; |p / size| >= 32767 or NaN: dropped and counted
  one per voxel  the point of LOWEST input index; survivors in ascending input index
  time rule      q > t_last: T_end; else the first k with t_k < q && t_k+1 >= q; none (q <= t_0): segment 0, s as it comes out;
                 |t_k+1 - t_k| < 1e-6: T_k; one state: T_end
  interpolation  slerp (Eigen's, normalised) / lerp at s; the new point is T_end^-1 Ti p

Discrete decisions (keys, segments) are taken in float64, as the device takes them; the arithmetic runs in the caller's dtype, so
numpy.longdouble gives the extended-precision reference. Next to a point the model returns A, the sum of absolute values behind each
coordinate (for the bound K u A of tests/test_gpu_scan.py)."""
import numpy as np

import vmap_np as vm

LD, U = vm.LD, vm.U


# ---- one point per voxel
def subsample(pts, size):
    """(kept input indices ascending, n_skipped): a vectorised restatement (packed keys, first occurrence by a stable unique)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        q = pts / np.float64(size)
        valid = (np.abs(q) < 32767.0).all(axis=1)      # (NaN compares false)
    idx = np.nonzero(valid)[0]
    k = np.trunc(q[idx]).astype(np.int64) + 32768
    packed = (k[:, 0] << 32) | (k[:, 1] << 16) | k[:, 2]
    _, first = np.unique(packed, return_index=True)      # (index of the first occurrence of every key)
    return np.sort(idx[first]).astype(np.int32), int(len(pts) - len(idx))


def subsample_dict(pts, size):
    """The independent implementation: a dictionary of the first index per key, the reference's loop."""
    first, skipped = {}, 0
    for i, p in enumerate(np.asarray(pts, np.float64).reshape(-1, 3)):
        k = vm.point_key(p, size)
        if k is None:
            skipped += 1
        elif k not in first:
            first[k] = i
    return np.array(sorted(first.values()), np.int32), skipped


# ---- the time rule
def segment(t, q):
    """-1: the last state; else the segment index (bisection: the number of state times below q, minus one)."""
    t = np.asarray(t, np.float64)
    q = np.float64(q)
    if len(t) < 2 or q > t[-1]:
        return -1
    lo, hi = 0, len(t)
    while lo < hi:
        mid = (lo + hi) >> 1
        if t[mid] < q:
            lo = mid + 1
        else:
            hi = mid
    return 0 if lo == 0 else lo - 1


def segment_brute(t, q):
    """The reference's linear scan, with its two undefined spots defined as f4d defines them."""
    t = np.asarray(t, np.float64)
    q = np.float64(q)
    if len(t) == 1 or q > t[-1]:
        return -1
    for k in range(len(t) - 1):
        if t[k] < q and t[k + 1] >= q:
            return k
    return 0


def branch(t, q):
    """Which rule decided: 'single', 'behind', 'front' (q <= t_0), 'short' (|dt| < 1e-6), 'interp'."""
    t = np.asarray(t, np.float64)
    if len(t) == 1:
        return "single"
    k = segment(t, q)
    if k < 0:
        return "behind"
    if abs(t[k + 1] - t[k]) < 1e-6:
        return "short"
    return "front" if not t[0] < q else "interp"


def pose_at(t, poses, q, dt=np.float64, sums=False):
    """(segment, Ti [7]) in dtype dt; sums: also (A_t [3], rho): the absolute sums |p_k| |1 - s| + |p_k+1| |s| behind Ti's translation
    and |s0| + |s1| behind its quaternion (1 where a state is taken as it is; both grow with an extrapolation)."""
    t64 = np.asarray(t, np.float64)
    P = np.asarray(poses, np.float64).reshape(-1, 7).astype(dt)
    k = segment(t64, q)
    if k < 0 or abs(t64[k + 1] - t64[k]) < 1e-6:
        Ti = P[k if k >= 0 else -1].copy()
        return (k, Ti, np.abs(Ti[:3]).astype(np.float64), 1.0) if sums else (k, Ti)
    s = (dt(q) - dt(t64[k])) / (dt(t64[k + 1]) - dt(t64[k]))
    r = vm._slerp(P[k, 3:], s, P[k + 1, 3:], dt)
    r = r / np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3])
    Ti = np.concatenate([P[k, :3] * (dt(1) - s) + P[k + 1, :3] * s, r])
    if not sums:
        return k, Ti
    At = (np.abs(P[k, :3]) * abs(dt(1) - s) + np.abs(P[k + 1, :3]) * abs(s)).astype(np.float64)
    return k, Ti, At, float(abs(dt(1) - s) + abs(s))


def undistort_point(Te, Ti, p, dt=np.float64, At=None, rho=1.0):
    """(T_end^-1 Ti p, A): R_end^T ((R_i p + t_i) - t_end) and the absolute sums behind its coordinates,
    A = |R_end|^T (rho |R_i| |p| + A_t + |t_end|) with A_t and rho of pose_at (A_t = |t_i| when not given)."""
    Ri, Re = vm._qrot(Ti[3:], dt), vm._qrot(Te[3:], dt)
    p = np.asarray(p, dt)
    d = np.array([(Ri[a, 0] * p[0] + Ri[a, 1] * p[1] + Ri[a, 2] * p[2] + Ti[a]) - Te[a] for a in range(3)], dt)
    out = np.array([Re[0, a] * d[0] + Re[1, a] * d[1] + Re[2, a] * d[2] for a in range(3)], dt)
    Ad = rho * (np.abs(Ri) @ np.abs(p)) + (np.abs(Ti[:3]) if At is None else At) + np.abs(Te[:3])
    return out, (np.abs(Re).T @ Ad).astype(np.float64)


def undistort(pts, ts, t, poses, dt=np.float64):
    """dict(pts [n, 3] in dt, A [n, 3], seg [n])."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    Te = np.asarray(poses, np.float64).reshape(-1, 7)[-1].astype(dt)
    out, A, seg = np.zeros((len(pts), 3), dt), np.zeros((len(pts), 3)), np.zeros(len(pts), np.int32)
    for i in range(len(pts)):
        seg[i], Ti, At, rho = pose_at(t, poses, ts[i], dt, sums=True)
        out[i], A[i] = undistort_point(Te, Ti, pts[i], dt, At, rho)
    return dict(pts=out, A=A, seg=seg)


def til_point(til, p, dt=np.float64):
    til = np.asarray(til, np.float64).astype(dt)
    R = vm._qrot(til[3:], dt)
    p = np.asarray(p, dt)
    return np.array([R[a, 0] * p[0] + R[a, 1] * p[1] + R[a, 2] * p[2] + til[a] for a in range(3)], dt)


# ---- transformPoint + gridSampling
def world_points(ct, pb, pe, alpha, pts, dt=np.float64):
    pb, pe = np.asarray(pb, np.float64).astype(dt), np.asarray(pe, np.float64).astype(dt)
    return np.array([vm.world_point(ct, pb, pe, dt(alpha[i]) if ct else dt(0), np.asarray(pts[i], np.float64).astype(dt), dt) for i in range(len(pts))], dt).reshape(-1, 3)


def keypoints(ct, pb, pe, alpha, pts, size, world=None):
    """(kept indices, n_skipped, world points): one keypoint per voxel of the WORLD point (world: the points to key on, when the
    caller has them — the device's, bit for bit)."""
    w = world_points(ct, pb, pe, alpha, pts) if world is None else np.asarray(world, np.float64)
    kept, skipped = subsample(w, size)
    return kept, skipped, w
