"""The model of the dense RGB-D map (gfbe_dmap_*, include/gfbe.h section f3c): a plain sequential dictionary walk in keyframe and
list order, as addKeyFrame / updatePath of dense_map/src/pose_graph.cpp do it with the octree, for a dtype argument (float64: the
arithmetic of the device, operation for operation; longdouble: the extended-precision check of the cases), and a brute-force
O(n^2) radius filter. capped_by_sort is the independent restatement of the density cap (a stable sort by (key, index))."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
KEY_BITS = 21
DEFAULTS = dict(add_cap=3, rebuild_cap=5, resolution=0.01, origin=-10000.0, z_min=-0.5, z_max=2.0,
                ex_cam=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), filter_radius=0.8, filter_min_neighbors=10)


def rot(q, dt=np.float64):
    """qrot of gfbe_math.h (Eigen's toRotationMatrix) on a quaternion x y z w, in dtype dt."""
    x, y, z, w = [dt(v) for v in q]
    two = dt(2.0)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = dt(1.0)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]], dtype=dt)


def world(pose7, ex_cam, pts, dt=np.float64):
    """pw = R (R_ic p + t_ic) + P, products left to right per row: (pw [n, 3] in dt, A [n, 3] the absolute sum behind each coordinate)."""
    p = np.asarray(pts, np.float32).reshape(-1, 3).astype(dt)
    pose7, ex_cam = np.asarray(pose7, np.float64), np.asarray(ex_cam, np.float64)
    R, P, Ric, tic = rot(pose7[3:], dt), pose7[:3].astype(dt), rot(ex_cam[3:], dt), ex_cam[:3].astype(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.stack([((Ric[a, 0] * p[:, 0] + Ric[a, 1] * p[:, 1]) + Ric[a, 2] * p[:, 2]) + tic[a] for a in range(3)], 1)
        pw = np.stack([((R[a, 0] * c[:, 0] + R[a, 1] * c[:, 1]) + R[a, 2] * c[:, 2]) + P[a] for a in range(3)], 1)
        ca = np.abs(p.astype(np.float64)) @ np.abs(Ric.astype(np.float64)).T + np.abs(tic.astype(np.float64))
        A = ca @ np.abs(R.astype(np.float64)).T + np.abs(P.astype(np.float64))
    return pw, A


def to_float(pw):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(pw).astype(np.float32)


def axis_q(pf, origin, resolution, dt=np.float64):
    """((double)pf - origin) / resolution before the floor, in dt."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(pf, np.float32).astype(dt) - dt(origin)) / dt(resolution)


def keys(pf, origin, resolution, dt=np.float64):
    """(valid [n], key [n, 3] int64) of float points pf [n, 3]: floor per axis, valid for 0 <= key < 2^21 on every axis."""
    q = np.floor(axis_q(np.asarray(pf, np.float32).reshape(-1, 3), origin, resolution, dt))
    with np.errstate(invalid="ignore"):
        ok = ((q >= 0) & (q < 2 ** KEY_BITS)).all(1)
    k = np.zeros(q.shape, np.int64)
    k[ok] = q[ok].astype(np.int64)
    return ok, k


def pack(k):
    k = np.asarray(k, np.int64)
    return (k[..., 0] << (2 * KEY_BITS)) | (k[..., 1] << KEY_BITS) | k[..., 2]


def unpack(key):
    m = (1 << KEY_BITS) - 1
    return (int(key) >> (2 * KEY_BITS)) & m, (int(key) >> KEY_BITS) & m, int(key) & m


def gated(z, z_min, z_max):
    with np.errstate(invalid="ignore"):
        return (z > z_max) | (z < z_min)


def capped_walk(packed, counts, cap):
    """The sequential walk: candidate i is kept while its voxel holds fewer than cap points; counts (a dict) is raised. kept [m] bool."""
    kept = np.zeros(len(packed), bool)
    for i, k in enumerate(packed.tolist()):
        c = counts.get(k, 0)
        if c < cap:
            counts[k] = c + 1
            kept[i] = True
    return kept


def capped_by_sort(packed, counts, cap):
    """The same set without a walk: kept iff base + rank < cap, rank = the position among the call's candidates of the voxel in index
    order (a stable sort by key). counts is read, not changed."""
    packed = np.asarray(packed, np.int64)
    order = np.argsort(packed, kind="stable")
    sk = packed[order]
    first = np.r_[True, sk[1:] != sk[:-1]] if len(sk) else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(len(sk)), 0)) if len(sk) else np.zeros(0, int)
    rank = np.arange(len(sk)) - start
    base = np.array([counts.get(k, 0) for k in sk.tolist()], np.int64)
    kept = np.zeros(len(packed), bool)
    kept[order] = base + rank < cap
    return kept


def filter_brute(xyz, radius, min_neighbors, chunk=1024):
    """keep [n] uint8: more than min_neighbors points (the point itself counted) with (dx dx + dy dy) + dz dz <= radius radius, FP64
    differences and products on the float coordinates."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    r2 = np.float64(radius) * np.float64(radius)
    keep = np.zeros(len(p), np.uint8)
    for a in range(0, len(p), chunk):
        d = p[a:a + chunk, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        keep[a:a + chunk] = (d2 <= r2).sum(1) > min_neighbors
    return keep


class DenseMapModel:
    """The handle's state on the host. Every list is in the order the reference's loops produce."""

    def __init__(self, point_capacity=1 << 30, keyframe_capacity=1 << 30, dtype=np.float64, restate=False, **options):
        self.opt = dict(DEFAULTS, **options)
        self.dt, self.pcap, self.kcap = dtype, point_capacity, keyframe_capacity
        self.capped = capped_by_sort if restate else capped_walk
        self.restate = restate
        self.kf_pts, self.kf_rgb = [], []              # the keyframes' lists
        self.counts = {}                               # packed key -> points
        self.xyz, self.rgb = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)
        self.kf, self.src = np.zeros(0, np.int32), np.zeros(0, np.int32)
        self.n_skipped = self.n_gated = self.n_refused = 0
        self.last_kept = np.zeros(0, np.int64)

    @property
    def n_stored(self):
        return int(sum(len(p) for p in self.kf_pts))

    def _cap(self, packed, cap):
        kept = self.capped(packed, self.counts, cap)
        if self.restate:      # (capped_by_sort leaves the counts alone)
            for k in packed[kept].tolist():
                self.counts[k] = self.counts.get(k, 0) + 1
        return kept

    def _candidates(self, pose7, pts, gate):
        o = self.opt
        pw, _ = world(pose7, o["ex_cam"], pts, self.dt)
        g = gated(pw[:, 2], self.dt(o["z_min"]), self.dt(o["z_max"])) if gate else np.zeros(len(pw), bool)
        pf = to_float(pw)
        ok, k = keys(pf, o["origin"], o["resolution"], self.dt)
        return pf, g, ok & ~g, pack(k)

    def add_keyframe(self, pose7, pts, rgb):
        """Returns the kept input indices (ascending)."""
        pts, rgb = np.asarray(pts, np.float32).reshape(-1, 3), np.asarray(rgb, np.uint8).reshape(-1, 3)
        n = len(pts)
        room = self.pcap - self.n_stored
        if len(self.kf_pts) >= self.kcap or (room <= 0 and n > 0):
            self.n_refused += n      # refused whole, unexamined
            if len(self.kf_pts) < self.kcap:
                self._append_keyframe(pts[:0], rgb[:0], np.zeros((0, 3), np.float32))
            self.last_kept = np.zeros(0, np.int64)
            return self.last_kept
        pf, g, cand, packed = self._candidates(pose7, pts, True)
        self.n_gated += int(g.sum())
        self.n_skipped += int((~cand & ~g).sum())
        idx = np.flatnonzero(cand)
        # the capacity cut is made on the kept list: the walk runs on a copy of the counts, what fits raises the real ones
        kept = idx[self.capped(packed[idx], dict(self.counts), self.opt["add_cap"])]
        fit = kept[:max(room, 0)]
        self.n_refused += len(kept) - len(fit)
        for k in packed[fit].tolist():
            self.counts[k] = self.counts.get(k, 0) + 1
        self._append_keyframe(pts[fit], rgb[fit], pf[fit])
        self.last_kept = fit
        return fit

    def _append_keyframe(self, pts, rgb, pf):
        k, base = len(self.kf_pts), self.n_stored
        self.kf_pts.append(pts.copy()); self.kf_rgb.append(rgb.copy())
        self.xyz, self.rgb = np.vstack([self.xyz, pf]), np.vstack([self.rgb, rgb])
        self.kf = np.r_[self.kf, np.full(len(pts), k, np.int32)]
        self.src = np.r_[self.src, base + np.arange(len(pts), dtype=np.int32)]

    def rebuild(self, poses):
        poses = np.asarray(poses, np.float64).reshape(-1, 7)
        assert len(poses) == len(self.kf_pts)
        self.counts = {}
        pfs, cands, packs, kfs, rgbs = [], [], [], [], []
        for k, (pts, rgb) in enumerate(zip(self.kf_pts, self.kf_rgb)):
            pf, _, cand, packed = self._candidates(poses[k], pts, False)
            pfs.append(pf); cands.append(cand); packs.append(packed); kfs.append(np.full(len(pts), k, np.int32)); rgbs.append(rgb)
        cat = lambda v, shape, dt: np.concatenate(v) if v else np.zeros(shape, dt)      # noqa: E731
        pf, cand, packed = cat(pfs, (0, 3), np.float32), cat(cands, 0, bool), cat(packs, 0, np.int64)
        kf, rgb = cat(kfs, 0, np.int32), cat(rgbs, (0, 3), np.uint8)
        self.n_skipped += int((~cand).sum())
        idx = np.flatnonzero(cand)
        kept = idx[self._cap(packed[idx], self.opt["rebuild_cap"])]
        self.xyz, self.rgb, self.kf, self.src = pf[kept], rgb[kept], kf[kept], kept.astype(np.int32)
        return kept

    def filter(self):
        return filter_brute(self.xyz, self.opt["filter_radius"], self.opt["filter_min_neighbors"])

    def size(self):
        return dict(n_keyframes=len(self.kf_pts), n_stored=self.n_stored, n_cloud=len(self.xyz), n_voxels=sum(1 for c in self.counts.values() if c > 0),
                    n_skipped=self.n_skipped, n_gated=self.n_gated, n_refused=self.n_refused)

    def pool(self):
        if not self.kf_pts:
            return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)
        return np.concatenate(self.kf_pts), np.concatenate(self.kf_rgb)
