"""Synthetic line windows for gfbe_line_refine (the input FeatureManager::linefeature holds before onlyLineOpt()).

A window: 11 camera-rig poses moving forward with a slow yaw, the camera extrinsic of a forward-looking camera, and straight 3-D segments
in front of the rig. Each line is seen from its start frame on: in every frame two points of the segment (a random part of it, as a line
detector sees it) are projected to the normalised image plane and perturbed by pixel noise. The initial line_plucker is the true line
with perturbed endpoints, in the start frame's camera frame, at an arbitrary scale (a Plücker line is homogeneous).

Line kinds (window["kind"]):
  ok              eligible, consistent observations
  short / late / untriangulated   ineligible: n_obs < LINE_MIN_OBS, start_frame >= WINDOW_SIZE - 2, is_triangulation = 0
  behind          eligible, consistent, but the segment lies behind the cameras (removeLineOutlier: endpoint behind the camera)
  long            eligible, consistent, a segment running 20 m into depth (removeLineOutlier: endpoints more than 10 apart)
  outlier_obs     eligible, one observation displaced far off the line (removeLineOutlier: reprojection error above 3 / 500)
"""
import numpy as np

NFRAMES, WINDOW_SIZE, LINE_MIN_OBS = 11, 10, 5


def _quat_xyzw(R):
    w = np.sqrt(max(1e-300, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def _rotz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


# body x forward, z up; camera z forward (= body x), camera x = -body y, camera y = -body z, slightly tilted
R_BC = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]) @ np.array(
    [[1.0, 0.0, 0.0], [0.0, np.cos(0.05), -np.sin(0.05)], [0.0, np.sin(0.05), np.cos(0.05)]])
T_BC = np.array([0.1, 0.02, 0.05])


def line_window(seed=0, n_ok=40, n_short=3, n_late=3, n_untri=2, n_behind=1, n_long=1, n_outlier=1, noise=0.5 / 460.0,
                init_sigma=0.05, shuffle=True):
    """One line window as a dict of numpy arrays (the keys abi.LineWindowHolder takes) plus the truth: true_plucker [n][6] (start camera
    frame, unit scale) and kind [n]."""
    rng = np.random.default_rng(seed)
    Rs, Ps = [], []
    yaw0 = rng.uniform(-np.pi, np.pi)
    p0 = rng.normal(0, 5, 3)
    for i in range(NFRAMES):
        yaw = yaw0 + 0.01 * i + 0.003 * rng.normal()
        R = _rotz(yaw)
        Rs.append(R)
        Ps.append(p0 + R @ np.array([0.25 * i, 0.0, 0.0]) + rng.normal(0, 0.01, 3))
    pose = np.array([np.concatenate([Ps[i], _quat_xyzw(Rs[i])]) for i in range(NFRAMES)])
    ex_cam = np.concatenate([T_BC, _quat_xyzw(R_BC)])
    Rwc = [Rs[i] @ R_BC for i in range(NFRAMES)]
    twc = [Ps[i] + Rs[i] @ T_BC for i in range(NFRAMES)]
    fwd, left = Rs[0][:, 0], Rs[0][:, 1]
    up = np.array([0.0, 0.0, 1.0])

    kinds = (["ok"] * n_ok + ["short"] * n_short + ["late"] * n_late + ["untriangulated"] * n_untri + ["behind"] * n_behind
             + ["long"] * n_long + ["outlier_obs"] * n_outlier)
    if shuffle:
        kinds = [kinds[k] for k in rng.permutation(len(kinds))]
    start, nobs, obs, tri, plk, truth = [], [], [], [], [], []
    for kind in kinds:
        if kind == "late":
            s = int(rng.integers(WINDOW_SIZE - 2, NFRAMES - 1))
            k = int(rng.integers(1, NFRAMES - s + 1))
        elif kind == "short":
            s = int(rng.integers(0, WINDOW_SIZE - 2))
            k = int(rng.integers(1, LINE_MIN_OBS))
        else:
            s = int(rng.integers(0, NFRAMES - LINE_MIN_OBS + 1))
            k = int(rng.integers(LINE_MIN_OBS, NFRAMES - s + 1))
        # the segment in the world
        depth = rng.uniform(5.0, 12.0)
        c = Ps[0] + fwd * depth + left * rng.uniform(-3.0, 3.0) + up * rng.uniform(-1.0, 2.5)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        half = rng.uniform(0.5, 1.5)
        if kind == "behind":
            c = Ps[0] - fwd * rng.uniform(4.0, 8.0) + left * rng.uniform(-2.0, 2.0) + up * rng.uniform(-0.5, 1.5)
        if kind == "long":
            c = Ps[0] + fwd * 14.0 + left * rng.uniform(1.0, 2.0) + up * 0.5
            d = fwd + 0.05 * left
            d /= np.linalg.norm(d)
            half = 10.0
        A, B = c - half * d, c + half * d
        o = []
        for j in range(s, s + k):
            a, b = np.sort(rng.uniform(0.0, 1.0, 2))
            a, b = (0.05 * a, 0.95 + 0.05 * b) if kind == "long" else (0.3 * a, 0.7 + 0.3 * b)   # (a long part of the segment)
            pts = []
            for u in (a, b):
                pc = Rwc[j].T @ (A + u * (B - A) - twc[j])
                pts += [pc[0] / pc[2], pc[1] / pc[2]]
            o.append(np.array(pts) + rng.normal(0, noise, 4))
        if kind == "outlier_obs":
            j = int(rng.integers(1, k))
            nrm = np.array([o[j][1] - o[j][3], o[j][2] - o[j][0]])
            nrm /= np.linalg.norm(nrm)
            o[j] = o[j] + np.concatenate([nrm, nrm]) * 0.08
        # truth and initial guess in the start camera frame
        Ac, Bc = Rwc[s].T @ (A - twc[s]), Rwc[s].T @ (B - twc[s])
        v = Bc - Ac
        L = np.concatenate([np.cross(Ac, v), v])
        truth.append(L / np.linalg.norm(L))
        A0, B0 = Ac + rng.normal(0, init_sigma, 3), Bc + rng.normal(0, init_sigma, 3)
        v0 = B0 - A0
        plk.append(np.concatenate([np.cross(A0, v0), v0]) * rng.uniform(0.5, 2.0))
        start.append(s)
        nobs.append(k)
        obs += o
        tri.append(0 if kind == "untriangulated" else 1)
    return dict(start_frame=np.array(start, np.int32), n_obs=np.array(nobs, np.int32), obs=np.array(obs).reshape(-1, 4),
                is_triangulation=np.array(tri, np.uint8), line_plucker=np.array(plk), pose=pose, ex_cam=ex_cam,
                true_plucker=np.array(truth), kind=np.array(kinds))


def eligible(lw):
    return (lw["n_obs"] >= LINE_MIN_OBS) & (lw["start_frame"] < WINDOW_SIZE - 2) & (lw["is_triangulation"] != 0)


class LineStream:
    """Frame-by-frame line observations for the line tables (gfbe_ltab_*): a camera rig driving forward with a slow yaw past 3-D
    segments scattered along its route. Segment k has the line id k; it is observed in a frame when both its endpoints are in front of
    the camera, inside the field of view and nearer than `max_range`, and the frame lies inside the segment's own life span (a tracker
    that loses and never re-finds a line) — so ids appear and disappear. noise = 0 gives exact projections of the full segment;
    otherwise a random part of the segment is projected and perturbed by `noise` (normalised image units), as in line_window().

      pose7(g) -> [p | q(x, y, z, w)] of global frame g;  frame(g) -> (line_id [n] ascending int32, obs4 [n][4])
      endpoints(k) -> the two 3-D endpoints of segment k in the world;  ex_cam: [tic | q(ric)]
    """

    def __init__(self, seed=0, n_frames=40, n_segments=120, noise=0.5 / 460.0, step=0.4, max_range=14.0):
        rng = np.random.default_rng(seed)
        self.n_frames, self.noise, self.max_range = n_frames, noise, max_range
        self.ex_cam = np.concatenate([T_BC, _quat_xyzw(R_BC)])
        yaw0, p0 = rng.uniform(-np.pi, np.pi), rng.normal(0, 5, 3)
        self.R, self.P = [], []
        p = p0.copy()
        for g in range(n_frames):
            R = _rotz(yaw0 + 0.012 * g + 0.003 * rng.normal())
            p = p + R @ np.array([step, 0.0, 0.0]) + rng.normal(0, 0.01, 3)
            self.R.append(R)
            self.P.append(p.copy())
        self.A, self.B, self.life = [], [], []
        for k in range(n_segments):
            g = int(rng.integers(0, n_frames))                      # the frame the segment is placed ahead of
            fwd, left, up = self.R[g][:, 0], self.R[g][:, 1], np.array([0.0, 0.0, 1.0])
            c = self.P[g] + fwd * rng.uniform(4.0, 10.0) + left * rng.uniform(-3.0, 3.0) + up * rng.uniform(-1.0, 2.0)
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            half = rng.uniform(0.4, 1.2)
            self.A.append(c - half * d)
            self.B.append(c + half * d)
            on = int(rng.integers(0, n_frames))
            self.life.append((on if rng.random() < 0.5 else 0, n_frames if rng.random() < 0.6 else on + int(rng.integers(1, 14))))
        self._rng_seed = seed

    def pose7(self, g):
        return np.concatenate([self.P[g], _quat_xyzw(self.R[g])])

    def endpoints(self, k):
        return self.A[k], self.B[k]

    def frame(self, g):
        rng = np.random.default_rng([self._rng_seed, 7919, g])       # (a frame's observations do not depend on which frames were asked for before)
        Rwc, twc = self.R[g] @ R_BC, self.P[g] + self.R[g] @ T_BC
        ids, obs = [], []
        for k in range(len(self.A)):
            if not (self.life[k][0] <= g < self.life[k][1]):
                continue
            A, B = self.A[k], self.B[k]
            if self.noise > 0:
                a, b = np.sort(rng.uniform(0.0, 1.0, 2))
                a, b = 0.3 * a, 0.7 + 0.3 * b
                A, B = self.A[k] + a * (self.B[k] - self.A[k]), self.A[k] + b * (self.B[k] - self.A[k])
            pa, pb = Rwc.T @ (A - twc), Rwc.T @ (B - twc)
            if min(pa[2], pb[2]) < 0.5 or max(pa[2], pb[2]) > self.max_range:
                continue
            o = np.array([pa[0] / pa[2], pa[1] / pa[2], pb[0] / pb[2], pb[1] / pb[2]])
            if np.abs(o[[0, 2]]).max() > 1.0 or np.abs(o[[1, 3]]).max() > 0.8:
                continue
            if self.noise > 0:
                o = o + rng.normal(0, self.noise, 4)
            ids.append(k)
            obs.append(o)
        return np.array(ids, np.int32), np.array(obs, float).reshape(-1, 4)
