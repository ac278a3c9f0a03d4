"""TEST INFRASTRUCTURE. The model of the frame observations (include/gfbe_obs.h, rules O1 .. O8), written from the reference's text:
PinholeCamera.cc:278-295, :450-510, :520-542, :646-662, feature_tracker.cpp:210-372, :797-847, :1006-1045, estimator.cpp:3927-3946.
numpy float64 and float32 arrays and scalars, one operation a statement, nothing fused. It is not pinned against the reference (nothing
of the reference's front end can be built without OpenCV and Eigen): DESIGN.md section 8.7b says so.

The functions ending in _scalar are second statements of O2, O3, O4 and O8: a walk over one point at a time on Python floats with
numpy.float32 casts, written separately (tests/test_obs_model.py compares the two bit for bit)."""
import math

import numpy as np

F, D = np.float32, np.float64
DEFAULTS = dict(depth_cam=1, match_tile=256)
NO_DEPTH = -2.4
NOBS = 11


# ---- O1
def camera(p8):
    fx, fy, cx, cy, k1, k2, p1, p2 = [D(v) for v in p8]
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, k1=k1, k2=k2, p1=p1, p2=p2, inv_K11=D(1.0) / fx, inv_K13=-cx / fx, inv_K22=D(1.0) / fy, inv_K23=-cy / fy,
                no_distortion=bool(k1 == 0.0 and k2 == 0.0 and p1 == 0.0 and p2 == 0.0))


# ---- O2
def distortion(c, x, y):
    x, y = np.asarray(x, D), np.asarray(y, D)
    mx2 = x * x
    my2 = y * y
    mxy = x * y
    rho2 = mx2 + my2
    rad = c["k1"] * rho2 + (c["k2"] * rho2) * rho2
    dx = (x * rad + (D(2.0) * c["p1"]) * mxy) + c["p2"] * (rho2 + D(2.0) * mx2)
    dy = (y * rad + (D(2.0) * c["p2"]) * mxy) + c["p1"] * (rho2 + D(2.0) * my2)
    return dx, dy


# ---- O3
def lift64(c, pts):
    """The undistorted normalised coordinates in double, before the cast (the property test needs them)."""
    pts = np.asarray(pts, F).reshape(-1, 2)
    mx_d = c["inv_K11"] * pts[:, 0].astype(D) + c["inv_K13"]
    my_d = c["inv_K22"] * pts[:, 1].astype(D) + c["inv_K23"]
    if c["no_distortion"]:
        return mx_d, my_d
    dx, dy = distortion(c, mx_d, my_d)
    mx_u, my_u = mx_d - dx, my_d - dy
    for _ in range(7):
        dx, dy = distortion(c, mx_u, my_u)
        mx_u, my_u = mx_d - dx, my_d - dy
    return mx_u, my_u


def lift(c, pts):
    """cur_un_pts [n, 2] float32."""
    x, y = lift64(c, pts)
    return np.stack([(x / D(1.0)).astype(F), (y / D(1.0)).astype(F)], 1).reshape(-1, 2)


def space_to_plane(c, x, y):
    """spaceToPlane of (x, y, 1) in double: (u, v)."""
    x, y = np.asarray(x, D), np.asarray(y, D)
    if not c["no_distortion"]:
        dx, dy = distortion(c, x, y)
        x, y = x + dx, y + dy
    return c["fx"] * x + c["cx"], c["fy"] * y + c["cy"]


# ---- O4
def velocity(un, prev_un, dt):
    return ((np.asarray(un, F) - np.asarray(prev_un, F)).astype(D) / D(dt)).astype(F)


# ---- O5
def c_round(v):
    """C's round of floats promoted to double: half away from zero."""
    v = np.asarray(v, F).astype(D)
    return np.copysign(np.floor(np.abs(v) + D(0.5)), v)


def depth_lookup(pts, depth):
    """(depth [n] float64, reads outside the image) on a uint16 image [rows, cols]."""
    pts = np.asarray(pts, F).reshape(-1, 2)
    rows, cols = depth.shape
    rx, ry = c_round(pts[:, 0]), c_round(pts[:, 1])
    inside = (rx >= 0) & (rx < cols) & (ry >= 0) & (ry < rows)
    raw = np.zeros(len(pts), np.int32)
    raw[inside] = depth[ry[inside].astype(np.int64), rx[inside].astype(np.int64)].astype(np.int32)
    return raw.astype(D) / D(1000), int((~inside).sum())


# ---- O3 .. O6 of one camera
EMPTY_PREV = (np.zeros(0, np.int32), np.zeros((0, 2), F))


def observe(cam8, pts, ids, prev=EMPTY_PREV, dt=1.0, depth=None):
    """prev: (ids ascending, un [n, 2]) of the previous call or EMPTY_PREV; depth: the uint16 image, or None (depth_cam == 0).
    Returns dict(ids, obs8 [n, 8], counters [4], prev=(ids, un) for the next call, order)."""
    c = camera(cam8)
    pts, ids = np.asarray(pts, F).reshape(-1, 2), np.asarray(ids, np.int32).reshape(-1)
    n = len(ids)
    order = np.argsort(ids, kind="stable")
    p, i_ = pts[order], ids[order]
    un = lift(c, p)
    vel = np.zeros((n, 2), F)
    pid, pun = prev
    q = np.searchsorted(pid, i_, side="left")
    known = np.zeros(n, bool)
    if len(pid):
        ok = q < len(pid)
        known[ok] = pid[q[ok]] == i_[ok]
    if known.any():
        vel[known] = velocity(un[known], pun[q[known]], dt)
    if depth is None:
        dep, outside = np.full(n, D(NO_DEPTH)), 0
    else:
        dep, outside = depth_lookup(p, np.asarray(depth, np.uint16))
    obs8 = np.zeros((n, 8), D)
    obs8[:, 0], obs8[:, 1], obs8[:, 2] = un[:, 0].astype(D), un[:, 1].astype(D), D(1.0)
    obs8[:, 3], obs8[:, 4] = p[:, 0].astype(D), p[:, 1].astype(D)
    obs8[:, 5], obs8[:, 6], obs8[:, 7] = vel[:, 0].astype(D), vel[:, 1].astype(D), dep
    dup = int(n > 1 and bool((np.diff(i_.astype(np.int64)) == 0).any()))
    return dict(ids=i_.copy(), obs8=obs8, counters=np.array([n, int(known.sum()), outside, dup], np.int32), prev=(i_.copy(), un.copy()), order=order)


def sort_ids(ids):
    """(order, duplicate flag) of O6."""
    ids = np.asarray(ids, np.int32).reshape(-1)
    order = np.argsort(ids, kind="stable")
    return order, int(len(ids) > 1 and bool((np.diff(ids[order].astype(np.int64)) == 0).any()))


# ---- O7
def remove_outliers(pts, ids, track_cnt, drop):
    ids = np.asarray(ids, np.int32)
    keep = ~np.isin(ids, np.asarray(drop, np.int32))
    return np.asarray(pts, F).reshape(-1, 2)[keep], ids[keep], np.asarray(track_cnt, np.int32)[keep]


# ---- O8
def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _mul(R, a):
    return [_dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], a[0], a[1], a[2]) for i in range(3)]


def _mul_t(R, a):
    return [_dot3(R[i], R[3 + i], R[6 + i], a[0], a[1], a[2]) for i in range(3)]


def chain_world(point0, depth, pose_start, tic_ric):
    """pts_w of the chain (three float64 scalars)."""
    point0, pose_start, tic_ric = np.asarray(point0, D), np.asarray(pose_start, D), np.asarray(tic_ric, D)
    tic, ric = tic_ric[:3], tic_ric[3:]
    s = [D(depth) * point0[0], D(depth) * point0[1], D(depth) * point0[2]]
    pj = [v + tic[i] for i, v in enumerate(_mul(ric, s))]
    return [v + pose_start[i] for i, v in enumerate(_mul(pose_start[3:], pj))]


def predict_one(c, point0, depth, pose_start, tic_ric, pose_next):
    """((float32 u, float32 v), finite)."""
    pose_next, tic_ric = np.asarray(pose_next, D), np.asarray(tic_ric, D)
    tic, ric = tic_ric[:3], tic_ric[3:]
    pw = chain_world(point0, depth, pose_start, tic_ric)
    with np.errstate(all="ignore"):
        pl = _mul_t(pose_next[3:], [pw[i] - pose_next[i] for i in range(3)])
        pc = _mul_t(ric, [pl[i] - tic[i] for i in range(3)])
        x, y = pc[0] / pc[2], pc[1] / pc[2]
        u, v = space_to_plane(c, x, y)
        u, v = F(u), F(v)
    return (u, v), bool(np.isfinite(u) and np.isfinite(v))


def predicts(depth, n_obs, start_frame, frame_count):
    return bool(depth > 0 and n_obs >= 2 and start_frame + n_obs - 1 == frame_count)


def predict(cam8, pts, ids, table, frame_count, poses, tic_ric, next_pose):
    """table: FeatureTables.download() of the camera's table (feature_id, start_frame, n_obs, obs8 [n, 11, 8], estimated_depth); poses
    [11, 12]. Returns (predict_pts [n, 2] float32 in held order, the number predicted)."""
    c = camera(cam8)
    pts = np.asarray(pts, F).reshape(-1, 2)
    poses = np.asarray(poses, D).reshape(NOBS, 12)
    out, count = pts.copy(), 0
    where = {int(f): k for k, f in enumerate(table["feature_id"])}
    for i, fid in enumerate(np.asarray(ids, np.int32)):
        k = where.get(int(fid))
        if k is None or not predicts(table["estimated_depth"][k], table["n_obs"][k], table["start_frame"][k], frame_count):
            continue
        (u, v), ok = predict_one(c, table["obs8"][k, 0, :3], table["estimated_depth"][k], poses[table["start_frame"][k]], tic_ric, next_pose)
        if ok:
            out[i] = (u, v)
            count += 1
    return out, count


# ---- the second statements: one point at a time on Python floats
def _f(v):
    return float(np.float32(v))


def distortion_scalar(p8, x, y):
    fx, fy, cx, cy, k1, k2, p1, p2 = [float(v) for v in p8]
    r2 = x * x + y * y
    radial = k1 * r2 + (k2 * r2) * r2
    ddx = (x * radial + (2.0 * p1) * (x * y)) + p2 * (r2 + 2.0 * (x * x))
    ddy = (y * radial + (2.0 * p2) * (x * y)) + p1 * (r2 + 2.0 * (y * y))
    return ddx, ddy


def lift_scalar(p8, u, v):
    """(float32 x, float32 y) of one pixel."""
    fx, fy, cx, cy, k1, k2, p1, p2 = [float(v_) for v_ in p8]
    xd = (1.0 / fx) * _f(u) + (-cx / fx)
    yd = (1.0 / fy) * _f(v) + (-cy / fy)
    xu, yu = xd, yd
    if not (k1 == 0.0 and k2 == 0.0 and p1 == 0.0 and p2 == 0.0):
        for k in range(8):
            ddx, ddy = distortion_scalar(p8, xd, yd) if k == 0 else distortion_scalar(p8, xu, yu)
            xu, yu = xd - ddx, yd - ddy
    return np.float32(xu), np.float32(yu)


def velocity_scalar(un, prev_un, dt):
    return np.float32(float(np.float32(un) - np.float32(prev_un)) / float(dt))


def predict_scalar(p8, point0, depth, pose_start, tic_ric, pose_next):
    fx, fy, cx, cy, k1, k2, p1, p2 = [float(v) for v in p8]
    P0, R0 = [float(v) for v in pose_start[:3]], [float(v) for v in pose_start[3:]]
    Pn, Rn = [float(v) for v in pose_next[:3]], [float(v) for v in pose_next[3:]]
    t, r = [float(v) for v in tic_ric[:3]], [float(v) for v in tic_ric[3:]]
    d = float(depth)
    s = [d * float(point0[0]), d * float(point0[1]), d * float(point0[2])]
    row = lambda M, i, a: (M[3 * i] * a[0] + M[3 * i + 1] * a[1]) + M[3 * i + 2] * a[2]
    col = lambda M, i, a: (M[i] * a[0] + M[3 + i] * a[1]) + M[6 + i] * a[2]
    pj = [row(r, i, s) + t[i] for i in range(3)]
    pw = [row(R0, i, pj) + P0[i] for i in range(3)]
    dl = [pw[i] - Pn[i] for i in range(3)]
    pl = [col(Rn, i, dl) for i in range(3)]
    dc = [pl[i] - t[i] for i in range(3)]
    pc = [col(r, i, dc) for i in range(3)]
    div = lambda a, b: a / b if b != 0.0 else (math.nan if a == 0.0 or math.isnan(a) else math.copysign(math.inf, a) * math.copysign(1.0, b))
    x, y = div(pc[0], pc[2]), div(pc[1], pc[2])
    if not (k1 == 0.0 and k2 == 0.0 and p1 == 0.0 and p2 == 0.0):
        ddx, ddy = distortion_scalar(p8, x, y)
        x, y = x + ddx, y + ddy
    with np.errstate(all="ignore"):
        u, v = np.float32(fx * x + cx), np.float32(fy * y + cy)
    return (u, v), bool(np.isfinite(u) and np.isfinite(v))
