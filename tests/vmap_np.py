"""Plain Python / numpy model of the voxel map of the LiDAR odometry and of the scan-to-map association (the checker of gfbe_vmap_*),
written from lio/src/liw/lio/lidarodom.cpp: addPointToMap / map_incremental (:1167-1266), lasermap_fov_segment (:1268-1284),
searchNeighbors (:1086-1165), computeNeighborhoodDistribution (:887-927), the loop body of addSurfCostFactor (:929-1071) and
checkLocalizability (:811-885). A dict of voxels, the sequential insert, the triple loop, a sorted k-nearest (ties by visit order).

Map points are float64 (what the device stores); the association runs in the caller's dtype, so numpy.longdouble gives the
extended-precision reference, with a 3 x 3 cyclic Jacobi eigensolver in that dtype. Next to the outputs the association returns the
absolute sums A_X behind them (for the bounds K_X u A_X of tests/test_gpu_vmap.py) and the relative margin of every discrete
decision it took."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53

DEFAULTS = dict(size_voxel_map=0.2, max_num_points_in_voxel=20, min_distance_points=0.05, max_distance=500.0, voxel_neighborhood=1,
                max_number_neighbors=20, min_number_neighbors=20, threshold_voxel_occupancy=1, num_closest_neighbors=1,
                max_dist_to_plane_icp=0.3, power_planarity=2.0, weight_alpha=0.9, weight_neighborhood=0.1, max_num_residuals=2000)


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o


def axis_key(p, size):
    """(short)(p / size), truncated toward zero; None when |p / size| >= 32767 (the reference's cast is undefined there)."""
    q = np.float64(p) / np.float64(size)
    if not abs(q) < 32767.0:
        return None
    return int(q)      # int() truncates toward zero


def point_key(p, size):
    k = tuple(axis_key(p[a], size) for a in range(3))
    return None if None in k else k


class Map:
    def __init__(self, capacity=1 << 16, **kw):
        self.opt, self.cap = options(**kw), capacity
        self.vox = {}            # key -> list of float64 points, insertion order
        self.skipped, self.overflow = 0, 0
        self.min_margin = np.inf      # of the min_distance_points test

    def add_points(self, pts, min_num_points=0):
        o = self.opt
        pts = np.asarray(pts, np.float64).reshape(-1, 3)
        keys = [point_key(p, o["size_voxel_map"]) for p in pts]
        self.skipped += sum(k is None for k in keys)
        fresh = {k for k in keys if k is not None and k not in self.vox} if min_num_points <= 0 else set()
        if len(self.vox) + len(fresh) > self.cap:      # the device's capacity rule: the add changes nothing
            self.overflow = 1
            return
        md2 = np.float64(o["min_distance_points"]) ** 2
        for p, k in zip(pts, keys):
            if k is None:
                continue
            blk = self.vox.get(k)
            if blk is None:
                if min_num_points <= 0:
                    self.vox[k] = [p.copy()]
                continue
            if len(blk) >= o["max_num_points_in_voxel"]:
                continue
            sq_min = np.float64(10 * o["size_voxel_map"] * o["size_voxel_map"])
            for q in blk:
                d = q - p
                sq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                if sq < sq_min:
                    sq_min = sq
            if md2 > 0:
                self.min_margin = min(self.min_margin, abs(float(sq_min) - float(md2)) / float(md2))
            if sq_min > md2 and (min_num_points <= 0 or len(blk) >= min_num_points):
                blk.append(p.copy())

    def erase_far(self, location):
        loc = np.asarray(location, np.float64)
        md2 = np.float64(self.opt["max_distance"]) ** 2
        for k in [k for k, blk in self.vox.items() if ((blk[0] - loc) ** 2)[0] + ((blk[0] - loc) ** 2)[1] + ((blk[0] - loc) ** 2)[2] > md2]:
            del self.vox[k]

    def size(self):
        return dict(n_voxels=len(self.vox), n_points=sum(len(b) for b in self.vox.values()), n_skipped=self.skipped, overflow=self.overflow)

    def download(self):
        ks = sorted(self.vox)
        pts = [p for k in ks for p in self.vox[k]]
        return dict(keys=np.array(ks, np.int16).reshape(-1, 3), counts=np.array([len(self.vox[k]) for k in ks], np.int32),
                    points=np.array(pts, np.float64).reshape(-1, 3))

    def all_points(self):
        return np.array([p for b in self.vox.values() for p in b], np.float64).reshape(-1, 3)


# ---- pose algebra in the caller's dtype (the operation order of the device's lio_world_point)
def _qrot(q, dt):
    x, y, z, w = q
    one, two = dt(1), dt(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dt)


def _slerp(a, t, b, dt):
    one = dt(1) - dt(2.220446049250313e-16)
    d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]
    if abs(d) >= one:
        s0, s1 = dt(1) - t, t
    else:
        th = np.arccos(abs(d))
        st = np.sin(th)
        s0, s1 = np.sin((dt(1) - t) * th) / st, np.sin(t * th) / st
    if d < 0:
        s1 = -s1
    return s0 * a + s1 * b


def world_point(ct, pb, pe, al, p, dt):
    qs, ts = pb[3:], pb[:3]
    if ct:
        s = _slerp(pb[3:], al, pe[3:], dt)
        qs = s / np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3])
        ts = pb[:3] * (dt(1) - al) + pe[:3] * al
    R = _qrot(qs, dt)
    return np.array([R[a, 0] * p[0] + R[a, 1] * p[1] + R[a, 2] * p[2] + ts[a] for a in range(3)], dt)


def eig3(cov6, dt):
    """Cyclic Jacobi on [xx xy xz yy yz zz]: (eigenvalues ascending, eigenvectors as columns) in dtype dt."""
    A = np.array([[cov6[0], cov6[1], cov6[2]], [cov6[1], cov6[3], cov6[4]], [cov6[2], cov6[4], cov6[5]]], dt)
    Q = np.eye(3, dtype=dt)
    tol = dt(0.0625) * np.finfo(dt).eps
    for _ in range(12 if dt is np.float64 else 20):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            o = 3 - p - q
            apq = A[p, q]
            if abs(apq) <= tol * np.sqrt(abs(A[p, p] * A[q, q])):
                A[p, q] = A[q, p] = 0
                continue
            rotated = True
            theta = (A[q, q] - A[p, p]) / (dt(2) * apq)
            t = (dt(1) if theta >= 0 else dt(-1)) / (abs(theta) + np.sqrt(theta * theta + dt(1)))
            c = dt(1) / np.sqrt(t * t + dt(1))
            s = t * c
            A[p, p] -= t * apq
            A[q, q] += t * apq
            A[p, q] = A[q, p] = 0
            aop, aoq = A[o, p], A[o, q]
            A[o, p] = A[p, o] = c * aop - s * aoq
            A[o, q] = A[q, o] = s * aop + c * aoq
            for a in range(3):
                qp, qq = Q[a, p], Q[a, q]
                Q[a, p], Q[a, q] = c * qp - s * qq, s * qp + c * qq
        if not rotated:
            break
    i = [0, 1, 2]
    if A[i[1], i[1]] < A[i[0], i[0]]:
        i[0], i[1] = i[1], i[0]
    if A[i[2], i[2]] < A[i[1], i[1]]:
        i[1], i[2] = i[2], i[1]
    if A[i[1], i[1]] < A[i[0], i[0]]:
        i[0], i[1] = i[1], i[0]
    return np.array([A[k, k] for k in i], dt), Q[:, i]


def moments(nb, dt):
    """Barycentre and covariance upper triangle [xx xy xz yy yz zz], summed in neighbour order."""
    b = np.zeros(3, dt)
    for p in nb:
        b = b + p
    b = b / dt(len(nb))
    c = np.zeros(6, dt)
    for p in nb:
        d = p - b
        c = c + np.array([d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]], dt)
    return b, c


def normal_a2d(cov6, dt):
    lam, V = eig3(cov6, dt)
    n = V[:, 0] / np.sqrt(V[0, 0] * V[0, 0] + V[1, 0] * V[1, 0] + V[2, 0] * V[2, 0])
    s1, s2, s3 = np.sqrt(abs(lam[2])), np.sqrt(abs(lam[1])), np.sqrt(abs(lam[0]))
    with np.errstate(invalid="ignore", divide="ignore"):
        a2d = (s2 - s3) / s1
    return n, a2d, lam


def weight(a2d, d0, o, dt):
    lw, ln = dt(abs(o["weight_alpha"])), dt(abs(o["weight_neighborhood"]))
    s = lw + ln
    lw, ln = lw / s, ln / s
    return lw * a2d ** dt(o["power_planarity"]) + ln * np.exp(-d0 / (dt(o["max_dist_to_plane_icp"]) * dt(o["min_number_neighbors"])))


def search(m, pw, v, thr, K, dt):
    """searchNeighbors: [(distance, visit index, (key, index in voxel))] of the K nearest, ascending by (distance, visit index); the
    relative gap of the closest pair of consecutive distances up to the cut."""
    key = point_key(np.asarray(pw, np.float64), m.opt["size_voxel_map"])
    if key is None:
        return [], np.inf
    cand, c = [], 0
    for kxx in range(key[0] - v, key[0] + v + 1):
        for kyy in range(key[1] - v, key[1] + v + 1):
            for kzz in range(key[2] - v, key[2] + v + 1):
                blk = m.vox.get((kxx, kyy, kzz))
                if blk is None or len(blk) < thr:
                    continue
                for i, q in enumerate(blk):
                    d = q.astype(dt) - pw
                    cand.append((np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), c, ((kxx, kyy, kzz), i)))
                    c += 1
    cand.sort(key=lambda e: (e[0], e[1]))
    gap = np.inf
    for i in range(min(K, len(cand) - 1)):
        gap = min(gap, float((cand[i + 1][0] - cand[i][0]) / cand[i + 1][0]))
    return cand[:K], gap


def associate(m, ct, raw_pts, alpha, pose_begin, pose_end=None, frame_init=False, dtype=np.float64):
    dt, o = dtype, m.opt
    raw_pts = np.asarray(raw_pts, np.float64).reshape(-1, 3)
    n = len(raw_pts)
    pb = np.asarray(pose_begin, np.float64).astype(dt)
    pe = np.asarray(pose_end if pose_end is not None else pose_begin, np.float64).astype(dt)
    v = 2 if frame_init else o["voxel_neighborhood"]
    thr = 1 if frame_init else o["threshold_voxel_occupancy"]
    K, ncn, maxd = o["max_number_neighbors"], o["num_closest_neighbors"], dt(o["max_dist_to_plane_icp"])
    out = dict(src=[], pts=[], normals=[], offsets=[], alpha=[], weights=[], A_normal=[], A_offset=[], A_weight=[], relgap_res=[],
               neighbor_count=np.zeros(n, np.int32), a2D=np.zeros(n, dt), A_a2D=np.zeros(n), relgap=np.full(n, np.inf), neighbors=[None] * n, visit=np.full((n, K), -1, np.int32), n_nan=0)
    margin = dict(tie=np.inf, plane=np.inf, flip=np.inf)
    total = 0
    for k in range(n):
        raw = raw_pts[k].astype(dt)
        al = dt(alpha[k]) if ct else dt(0)
        pw = world_point(ct, pb, pe, al, raw, dt)
        best, gap = search(m, pw, v, thr, K, dt)
        out["neighbor_count"][k] = len(best)
        out["neighbors"][k] = [e[2] for e in best]
        out["visit"][k, :len(best)] = [e[1] for e in best]
        if len(best) < o["min_number_neighbors"] or not best:
            continue
        margin["tie"] = min(margin["tie"], gap)
        nb = [m.vox[key][i].astype(dt) for _, _, (key, i) in best]
        _, cov = moments(nb, dt)
        nrm, a2d, lam = normal_a2d(cov, dt)
        if a2d != a2d:
            out["n_nan"] += 1
            continue
        dot = nrm[0] * (pb[0] - raw[0]) + nrm[1] * (pb[1] - raw[1]) + nrm[2] * (pb[2] - raw[2])
        margin["flip"] = min(margin["flip"], float(abs(dot) / np.sqrt(((pb[:3] - raw) ** 2).sum())))
        if dot < 0:
            nrm = -nrm
        d0 = best[0][0]
        w = weight(a2d, d0, o, dt)
        nv = nrm / np.sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2])
        # the absolute sums behind the entries (floats)
        nC = float(np.sqrt(cov[0] ** 2 + cov[3] ** 2 + cov[5] ** 2 + 2 * (cov[1] ** 2 + cov[2] ** 2 + cov[4] ** 2)))
        s1, s2, s3 = (np.float64(np.sqrt(abs(lam[2]))), np.float64(np.sqrt(abs(lam[1]))), np.float64(np.sqrt(abs(lam[0]))))
        relgap = float(lam[1] - lam[0]) / nC
        with np.errstate(divide="ignore", invalid="ignore"):
            A_a2d = nC * (1.0 / (s2 * s1) + 1.0 / (s3 * s1)) / 2 + float(a2d) * nC / (2 * s1 * s1) + float(a2d)
        pp, denom = float(o["power_planarity"]), float(o["max_dist_to_plane_icp"]) * o["min_number_neighbors"]
        lw = abs(o["weight_alpha"]) / (abs(o["weight_alpha"]) + abs(o["weight_neighborhood"]))
        e = float(np.exp(-d0 / dt(denom)))
        A_w = lw * (float(a2d) ** pp + pp * float(a2d) ** (pp - 1) * A_a2d) + (1 - lw) * e * (1 + (float(d0) + float(abs(raw).sum()) + float(abs(pw).sum())) / denom)
        out["a2D"][k], out["A_a2D"][k], out["relgap"][k] = a2d, A_a2d, relgap
        if ct:
            pt = raw_pts[k].copy()
        else:      # point_end = rotation.inverse() * point - rotation.inverse() * translation
            q = pb[3:]
            q2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
            Ri = _qrot(np.array([-q[0] / q2, -q[1] / q2, -q[2] / q2, q[3] / q2], dt), dt)
            pt = np.array([(Ri[a, 0] * pw[0] + Ri[a, 1] * pw[1] + Ri[a, 2] * pw[2]) - (Ri[a, 0] * pb[0] + Ri[a, 1] * pb[1] + Ri[a, 2] * pb[2]) for a in range(3)], dt)
        cut = False
        for i in range(min(ncn, len(nb))):
            q = nb[i]
            dist = abs((pw[0] - q[0]) * nrm[0] + (pw[1] - q[1]) * nrm[1] + (pw[2] - q[2]) * nrm[2])
            margin["plane"] = min(margin["plane"], float(abs(dist - maxd) / maxd))
            if dist >= maxd:
                continue
            total += 1
            out["src"].append(k)
            out["pts"].append(pt)
            out["normals"].append(nv)
            out["offsets"].append(-(nv[0] * q[0] + nv[1] * q[1] + nv[2] * q[2]))
            out["alpha"].append(al)
            out["weights"].append(w)
            out["A_normal"].append(1.0 / relgap)
            out["A_offset"].append(float(abs(nv * q).sum()) + float(abs(q).sum()) / relgap)
            out["A_weight"].append(A_w)
            out["relgap_res"].append(relgap)
            if total >= o["max_num_residuals"]:
                cut = True
                break
        if cut:
            out["reached"] = k + 1      # (the reference never looks at the keypoints behind the cut; the device's diagnostics cover them)
            break
    out.setdefault("reached", n)
    out["n_res"] = total
    out["src"] = np.array(out["src"], np.int32)
    for key, shape in (("pts", (-1, 3)), ("normals", (-1, 3)), ("offsets", (-1,)), ("alpha", (-1,)), ("weights", (-1,))):
        out[key] = np.array(out[key], dt).reshape(shape)
    for key in ("A_normal", "A_offset", "A_weight", "relgap_res"):
        out[key] = np.array(out[key], float)
    out["margin"] = margin
    return out


def localizability(normals, relgap_res=None, dtype=np.float64):
    """checkLocalizability: (sv descending, degenerate, A_sv) from N^T N summed in row order."""
    dt = dtype
    N = np.asarray(normals, dt).reshape(-1, 3)
    M = np.zeros(6, dt)
    for v in N:
        M = M + np.array([v[0] * v[0], v[0] * v[1], v[0] * v[2], v[1] * v[1], v[1] * v[2], v[2] * v[2]], dt)
    lam, _ = eig3(M, dt)
    sv = np.array([np.sqrt(abs(lam[2])), np.sqrt(abs(lam[1])), np.sqrt(abs(lam[0]))], dt)
    deg = len(N) <= 10 or (sv[0] + sv[2] + sv[1]) / dt(3) < 10 or sv[2] < 7
    pert = float(len(N)) + (float((2.0 / np.asarray(relgap_res, float)).sum()) if relgap_res is not None and len(N) else 0.0)
    with np.errstate(divide="ignore"):
        A_sv = pert / (2 * sv.astype(float))
    return sv, bool(deg), A_sv


def guaranteed_radius(pw, key, v, size):
    """Every map point nearer than this to pw lies in the (2v + 1)^3 voxels around `key` (truncation toward zero: the voxels of
    index 0 are twice as wide)."""
    r = np.inf
    for a in range(3):
        lo_k, hi_k = key[a] - v, key[a] + v
        lo = lo_k * size if lo_k > 0 else (lo_k - 1) * size
        hi = (hi_k + 1) * size if hi_k >= 0 else hi_k * size
        r = min(r, float(pw[a]) - lo, hi - float(pw[a]))
    return r
