"""Seeded LiDAR scenes for the voxel map (gfbe_vmap_*): a small room of six planes plus clutter, a short trajectory through it and scans
with per-point alpha times. A scan is given both ways the odometry uses it: world points (what map_incremental adds) and raw points
in the body frame with alpha in [0, 1] (what addSurfCostFactor associates under a begin and an end pose)."""
import numpy as np


def _qmul(a, b):      # (x, y, z, w)
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def _qrot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _slerp(a, t, b):
    d = float(a @ b)
    if abs(d) >= 1.0 - 2.220446049250313e-16:
        s0, s1 = 1.0 - t, t
    else:
        th = np.arccos(abs(d))
        s0, s1 = np.sin((1.0 - t) * th) / np.sin(th), np.sin(t * th) / np.sin(th)
    if d < 0:
        s1 = -s1
    q = s0 * a + s1 * b
    return q / np.linalg.norm(q)


def pose_at(pose_begin, pose_end, alpha):
    """(R, t) at slerp(alpha) / lerp(alpha) between two poses [t | q(x, y, z, w)]."""
    q = _slerp(pose_begin[3:], alpha, pose_end[3:])
    return _qrot(q), pose_begin[:3] * (1 - alpha) + pose_end[:3] * alpha


class Room:
    """A box room centred at `centre` with half extents `half`, sampled with `noise` metres of plane noise."""

    def __init__(self, seed=0, half=(1.0, 1.0, 0.75), centre=(0.3, -0.2, 0.4), noise=0.004):
        self.rng = np.random.default_rng(seed)
        self.half, self.centre, self.noise = np.asarray(half, float), np.asarray(centre, float), noise

    def surface(self, n, clutter=0.0):
        """n points on the six faces (area-weighted), a fraction `clutter` of them uniform inside the box instead."""
        rng, h = self.rng, self.half
        area = np.array([h[1] * h[2], h[1] * h[2], h[0] * h[2], h[0] * h[2], h[0] * h[1], h[0] * h[1]])
        face = rng.choice(6, size=n, p=area / area.sum())
        p = rng.uniform(-1, 1, (n, 3)) * h
        ax, sg = face // 2, np.where(face % 2 == 0, -1.0, 1.0)
        p[np.arange(n), ax] = sg * h[ax] + rng.normal(0, self.noise, n)
        inside = rng.random(n) < clutter
        p[inside] = rng.uniform(-0.8, 0.8, (int(inside.sum()), 3)) * h
        return p + self.centre

    def trajectory(self, n_poses):
        """n_poses body poses [t | q] drifting through the room with a slow yaw and a little roll."""
        out = []
        for k in range(n_poses):
            s = k / max(1, n_poses - 1)
            t = self.centre + np.array([-0.3 + 0.5 * s, 0.1 * np.sin(2.0 * s), 0.05 * s])
            yaw, roll = 0.3 * s, 0.04 * np.sin(3.0 * s)
            q = _qmul(np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2)]), np.array([np.sin(roll / 2), 0, 0, np.cos(roll / 2)]))
            out.append(np.concatenate([t, q / np.linalg.norm(q)]))
        return np.array(out)

    def scan(self, pose_begin, pose_end, n, clutter=0.0):
        """dict(world [n, 3], raw [n, 3], alpha [n]): raw = R(alpha)^T (world - t(alpha))."""
        world = self.surface(n, clutter)
        alpha = self.rng.uniform(0, 1, n)
        raw = np.empty_like(world)
        for i in range(n):
            R, t = pose_at(pose_begin, pose_end, alpha[i])
            raw[i] = R.T @ (world[i] - t)
        return dict(world=world, raw=raw, alpha=alpha)
