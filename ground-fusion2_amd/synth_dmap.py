"""Seeded RGB-D keyframes for the dense map (gfbe_dmap_*): a ground robot in a corridor of a few planes (floor, a wall ahead, a side
wall, a ceiling above the height gate), seen again and again. A keyframe's point list is what dense_map keeps per keyframe
(KeyFrame::point_rgbd): every depth_dist-th pixel inside the depth_boundary of a 640 x 480 image, back-projected to the camera
frame, float32 xyz and uint8 rgb. The robot dwells: `dwell` consecutive keyframes share a pose up to a millimetre, so voxels fill
past the caps of the insert (3) and of the rebuild (5)."""
import numpy as np


def _qmul(a, b):      # (x, y, z, w)
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def _qrot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _ypr(yaw, pitch, roll):
    q = _qmul(_qmul(np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2)]), np.array([0, np.sin(pitch / 2), 0, np.cos(pitch / 2)])),
              np.array([np.sin(roll / 2), 0, 0, np.cos(roll / 2)]))
    return q / np.linalg.norm(q)


class DenseScene:
    """Planes n . x = d in the world: the floor z = 0, a wall x = 7, a side wall y = 2.5, a ceiling z = 2.4 (above z_max = 2: gated)."""
    PLANES = (((0.0, 0.0, 1.0), 0.0), ((1.0, 0.0, 0.0), 7.0), ((0.0, 1.0, 0.0), 2.5), ((0.0, 0.0, 1.0), 2.4))
    FX = FY = 460.0
    CX, CY = 320.0, 240.0

    def __init__(self, seed=0, depth_dist=10, depth_boundary=10, max_depth=8.0, depth_noise=0.002):
        self.rng = np.random.default_rng(seed)
        self.max_depth, self.depth_noise = max_depth, depth_noise
        u = np.arange(depth_boundary, 640 - depth_boundary, depth_dist, dtype=float)
        v = np.arange(depth_boundary, 480 - depth_boundary, depth_dist, dtype=float)
        uu, vv = np.meshgrid(u, v, indexing="xy")
        self.rays = np.stack([(uu.ravel() - self.CX) / self.FX, (vv.ravel() - self.CY) / self.FY, np.ones(uu.size)], 1)      # (62 x 46 = 2852)
        # the camera looks along the body's x axis: camera z = body x, camera x = -body y, camera y = -body z
        R_ic = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
        w = 0.5 * np.sqrt(1.0 + np.trace(R_ic))
        q = np.array([(R_ic[2, 1] - R_ic[1, 2]) / (4 * w), (R_ic[0, 2] - R_ic[2, 0]) / (4 * w), (R_ic[1, 0] - R_ic[0, 1]) / (4 * w), w])
        self.ex_cam = np.concatenate([[0.08, 0.02, 0.25], q / np.linalg.norm(q)])

    def poses(self, n, dwell=6, step=0.04):
        """n body poses [t | q(x, y, z, w)]: the robot advances `step` metres every `dwell` keyframes and jitters by a millimetre between."""
        out = []
        for k in range(n):
            s = k // dwell
            t = np.array([step * s, 0.3 * np.sin(0.05 * s), 0.2]) + self.rng.normal(0, 1e-3, 3)
            q = _ypr(0.25 * np.sin(0.07 * s) + self.rng.normal(0, 1e-4), 0.02 * np.sin(0.11 * s), 0.015 * np.cos(0.13 * s))
            out.append(np.concatenate([t, q]))
        return np.array(out)

    def keyframe(self, pose):
        """(pts [m, 3] float32 camera frame, rgb [m, 3] uint8) of the pixels whose ray meets a plane within max_depth."""
        R, P = _qrot(pose[3:]), pose[:3]
        Ric, tic = _qrot(self.ex_cam[3:]), self.ex_cam[:3]
        o = R @ tic + P
        d = self.rays @ (R @ Ric).T
        best, which = np.full(len(d), np.inf), np.full(len(d), -1)
        for k, (nrm, off) in enumerate(self.PLANES):
            nrm = np.asarray(nrm)
            with np.errstate(divide="ignore", invalid="ignore"):
                lam = (off - nrm @ o) / (d @ nrm)
            hit = np.isfinite(lam) & (lam > 0.3) & (lam < best)
            best[hit], which[hit] = lam[hit], k
        ok = (which >= 0) & (best * np.linalg.norm(self.rays, axis=1) <= self.max_depth)
        lam = best[ok] * (1.0 + self.rng.normal(0, self.depth_noise, int(ok.sum())))
        pts = (self.rays[ok] * lam[:, None]).astype(np.float32)
        world = (pts.astype(float) @ (R @ Ric).T) + o
        rgb = np.stack([60 + 60 * which[ok], (world[:, 0] * 32).astype(np.int64) & 255, (world[:, 1] * 32).astype(np.int64) & 255], 1).astype(np.uint8)
        return pts, rgb

    def corrected(self, poses, yaw_drift=0.01, t_drift=(0.05, -0.03, 0.0)):
        """The poses after a loop closure: a yaw and a translation growing linearly along the trajectory (what optimize4DoF spreads)."""
        out = poses.copy()
        n = len(poses)
        for k in range(n):
            s = k / max(1, n - 1)
            qz = np.array([0, 0, np.sin(s * yaw_drift / 2), np.cos(s * yaw_drift / 2)])
            out[k, :3] = _qrot(qz) @ poses[k, :3] + s * np.asarray(t_drift)
            q = _qmul(qz, poses[k, 3:])
            out[k, 3:] = q / np.linalg.norm(q)
        return out
