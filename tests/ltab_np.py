"""TEST INFRASTRUCTURE. FeatureManager::linefeature as a plain Python list — the checker of the device line tables (gfbe_ltab_*,
csrc/gfbe_ltab.hip). Statement by statement from the reference:
  addFeatureCheckParallaxwithline, line loop    estimator/feature_manager.cpp:149-170
  triangulateLine                               :1151-1262 (pi_from_ppp / pipi_plk: utility/line_geometry.cpp:115-130)
  removeBackShiftDepthline, line loop           :1499-1527 — applied ONCE per call: in the reference the loop sits inside the loop over
                                                the point features (a misplaced brace), which empties the list within a frame or two
  removeBackline / removeFrontline, line loops  :896-911, :958-975
  getLineFeatureCount                           :1013-1027
  onlyLineOpt + removeLineOutlier               line_np.refine
The floating-point work (triangulate, the shift) runs in a chosen dtype (float64 or numpy.longdouble) on values that carry their
ABSOLUTE SUM along: every product multiplies the absolute sums, every sum adds them, so that A(x) >= |x| is the sum of the absolute
values of all terms x was formed from. A correct FP64 evaluation of x differs from the exact one by a small multiple of u A(x).
"""
import numpy as np

import line_np as ln

WINDOW_SIZE, NFRAMES, LINE_MIN_OBS = 10, 11, 5
COS_GATE = 0.998


class E:
    """A value (array) with its absolute sum."""

    def __init__(self, v, a=None, dtype=None):
        self.v = np.asarray(v, dtype=dtype)
        self.a = np.abs(self.v) if a is None else np.asarray(a, dtype=self.v.dtype)

    def __add__(self, o):
        return E(self.v + o.v, self.a + o.a)

    def __sub__(self, o):
        return E(self.v - o.v, self.a + o.a)

    def __neg__(self):
        return E(-self.v, self.a)

    def __mul__(self, o):
        return E(self.v * o.v, self.a * o.a)

    def __matmul__(self, o):
        return E(self.v @ o.v, self.a @ o.a)

    def __getitem__(self, k):
        return E(self.v[k], self.a[k])

    @property
    def T(self):
        return E(self.v.T, self.a.T)


def cross(x, y):
    return E(np.cross(x.v, y.v), np.array([x.a[1] * y.a[2] + x.a[2] * y.a[1], x.a[2] * y.a[0] + x.a[0] * y.a[2], x.a[0] * y.a[1] + x.a[1] * y.a[0]]))


def dot(x, y):
    return E(x.v @ y.v, x.a @ y.a)


def cat(*parts):
    return E(np.concatenate([np.atleast_1d(p.v) for p in parts]), np.concatenate([np.atleast_1d(p.a) for p in parts]))


def pi_from_ppp(x1, x2, x3):
    return cat(cross(x1 - x3, x2 - x3), -dot(x3, cross(x1, x2)))


def pipi_plk(p1, p2):
    def dp(a, b):
        return p1[a] * p2[b] - p2[a] * p1[b]
    return cat(dp(0, 3), dp(1, 3), dp(2, 3), -dp(1, 2), dp(0, 2), -dp(0, 1))


def plk_to_pose(plk, R, t):
    Rv = R @ plk[3:]
    return cat(R @ plk[:3] + cross(t, Rv), Rv)


def _unit(x):
    return x.v / np.sqrt((x.v * x.v).sum())


class LineTable:
    """One linefeature list. A line: dict(id, start, obs [list of [4]], tri, plk [6] float64, plk_abs [6])."""

    def __init__(self, dtype=np.float64):
        self.lines, self.dtype = [], dtype

    # ---- addFeatureCheckParallaxwithline, line loop
    def add_frame(self, frame_count, ids, obs4):
        tracked = new = 0
        for lid, ob in zip(ids, np.asarray(obs4, float).reshape(-1, 4)):          # (std::map order: ascending ids)
            hit = [l for l in self.lines if l["id"] == int(lid)]
            if not hit:
                self.lines.append(dict(id=int(lid), start=int(frame_count), obs=[ob.copy()], tri=0, plk=np.zeros(6), plk_abs=np.zeros(6)))
                new += 1
            else:
                if hit[0]["start"] + len(hit[0]["obs"]) >= NFRAMES:
                    raise OverflowError("a line received an observation past frame WINDOW_SIZE")
                hit[0]["obs"].append(ob.copy())
                tracked += 1
        return [tracked, new]

    # ---- triangulateLine. poses [11][12] = [P | R row-major], tic_ric [12]. Returns the decisions' margins per visited line:
    #      (id, |min_cos_theta - 0.998|, second-smallest cos_theta - smallest (inf with one partner), triangulated)
    def triangulate(self, poses, tic_ric):
        dt = self.dtype
        poses, tic_ric = np.asarray(poses, float).reshape(NFRAMES, 12), np.asarray(tic_ric, float).reshape(12)
        Ps = [E(poses[f, :3], dtype=dt) for f in range(NFRAMES)]
        Rs = [E(poses[f, 3:].reshape(3, 3), dtype=dt) for f in range(NFRAMES)]
        tic, ric = E(tic_ric[:3], dtype=dt), E(tic_ric[3:].reshape(3, 3), dtype=dt)
        one = np.ones(1)
        margins = []
        for l in self.lines:
            m, s = len(l["obs"]), l["start"]
            if not (m >= LINE_MIN_OBS and s < WINDOW_SIZE - 2) or l["tri"]:
                continue
            t0, R0 = Ps[s] + Rs[s] @ tic, Rs[s] @ ric
            o = l["obs"][0]
            pii = pi_from_ppp(E(np.concatenate([o[:2], one]), dtype=dt), E(np.concatenate([o[2:], one]), dtype=dt), E(np.zeros(3), dtype=dt))
            ni = _unit(pii[:3])
            min_cos, pij, coss = 1.0, None, []
            for k in range(1, m):
                t1, R1 = Ps[s + k] + Rs[s + k] @ tic, Rs[s + k] @ ric
                t, R = R0.T @ (t1 - t0), R0.T @ R1
                o = l["obs"][k]
                p3, p4 = R @ E(np.concatenate([o[:2], one]), dtype=dt) + t, R @ E(np.concatenate([o[2:], one]), dtype=dt) + t
                pj = pi_from_ppp(p3, p4, t)
                c = float(ni @ _unit(pj[:3]))
                coss.append(c)
                if c < min_cos:
                    min_cos, pij = c, pj
            cs = sorted(coss)
            gap = cs[1] - cs[0] if len(cs) > 1 else np.inf
            done = not (min_cos > COS_GATE)
            margins.append((l["id"], abs(min_cos - COS_GATE), gap, done))
            if not done:
                continue
            plk = pipi_plk(pii, pij)
            l["plk"], l["plk_abs"], l["tri"] = plk.v, plk.a, 1
        return margins

    # ---- removeBackShiftDepthline, line loop — once. marg_pr / new_pr [12] = [P | R]: the camera poses of the removed and the new frame 0
    def remove_back_shift(self, marg_pr, new_pr):
        dt = self.dtype
        marg_pr, new_pr = np.asarray(marg_pr, float), np.asarray(new_pr, float)
        mP, mR = E(marg_pr[:3], dtype=dt), E(marg_pr[3:].reshape(3, 3), dtype=dt)
        nP, nR = E(new_pr[:3], dtype=dt), E(new_pr[3:].reshape(3, 3), dtype=dt)
        kept = []
        for l in self.lines:
            if l["start"] != 0:
                l["start"] -= 1
            else:
                l["obs"].pop(0)
                if len(l["obs"]) < 2:
                    continue
                moved = plk_to_pose(E(l["plk"], dtype=dt), nR.T @ mR, nR.T @ (mP - nP))
                l["plk"], l["plk_abs"] = moved.v, moved.a
            kept.append(l)
        self.lines = kept

    def remove_back(self):
        kept = []
        for l in self.lines:
            if l["start"] != 0:
                l["start"] -= 1
            else:
                l["obs"].pop(0)
                if len(l["obs"]) == 0:
                    continue
            kept.append(l)
        self.lines = kept

    def remove_front(self, frame_count):
        kept = []
        for l in self.lines:
            if l["start"] == frame_count:
                l["start"] -= 1
            else:
                j = WINDOW_SIZE - 1 - l["start"]
                if l["start"] + len(l["obs"]) - 1 >= frame_count - 1:
                    l["obs"].pop(j)
                    if len(l["obs"]) == 0:
                        continue
            kept.append(l)
        self.lines = kept

    def size(self):
        return len(self.lines)

    def line_count(self):
        return sum(1 for l in self.lines if len(l["obs"]) >= LINE_MIN_OBS and l["start"] < WINDOW_SIZE - 2 and l["tri"])

    # ---- the list as gfbe_ltab_download returns it
    def snapshot(self):
        n = len(self.lines)
        out = dict(line_id=np.array([l["id"] for l in self.lines], np.int32).reshape(n), start_frame=np.array([l["start"] for l in self.lines], np.int32).reshape(n),
                   n_obs=np.array([len(l["obs"]) for l in self.lines], np.int32).reshape(n), obs4=np.zeros((n, NFRAMES, 4)),
                   is_triangulation=np.array([l["tri"] for l in self.lines], np.uint8).reshape(n),
                   line_plucker=np.array([l["plk"] for l in self.lines], self.dtype).reshape(n, 6),
                   plucker_abs=np.array([l["plk_abs"] for l in self.lines], self.dtype).reshape(n, 6))
        for i, l in enumerate(self.lines):
            out["obs4"][i, :len(l["obs"])] = l["obs"]
        return out

    def load(self, tab):
        """Replaces the list by a snapshot (gfbe_ltab_upload)."""
        self.lines = []
        for i in range(len(tab["line_id"])):
            k = int(tab["n_obs"][i])
            plk = np.asarray(tab["line_plucker"][i], float).copy()
            self.lines.append(dict(id=int(tab["line_id"][i]), start=int(tab["start_frame"][i]), obs=[np.array(tab["obs4"][i, q], float) for q in range(k)],
                                   tri=int(tab["is_triangulation"][i]), plk=plk, plk_abs=np.abs(plk)))

    def line_window(self, pose7, ex_cam):
        """The gfbe_line_window of this list (line_np.refine's input)."""
        obs = [o for l in self.lines for o in l["obs"]]
        return dict(start_frame=np.array([l["start"] for l in self.lines], np.int32), n_obs=np.array([len(l["obs"]) for l in self.lines], np.int32),
                    obs=np.array(obs, float).reshape(-1, 4), is_triangulation=np.array([l["tri"] for l in self.lines], np.uint8),
                    line_plucker=np.array([np.asarray(l["plk"], float) for l in self.lines]).reshape(-1, 6),
                    pose=np.asarray(pose7, float).reshape(NFRAMES, 7), ex_cam=np.asarray(ex_cam, float))

    # ---- setLineOrth + the erasures of removeLineOutlier, from given results (the device's, or line_np.refine's)
    def apply_refine(self, plucker, keep):
        kept = []
        for l, p, k in zip(self.lines, np.asarray(plucker, float).reshape(-1, 6), keep):
            if not k:
                continue
            l["plk"], l["plk_abs"] = p.copy(), np.abs(p)
            kept.append(l)
        self.lines = kept

    def refine(self, pose7, ex_cam, **kw):
        lw = self.line_window(pose7, ex_cam)
        res = ln.refine(lw, **kw) if len(self.lines) else None
        if res is not None:
            self.apply_refine(res["plucker"], res["keep"])
        return res


def cam_pr(pose7, ex_cam):
    """[P | R] of the CAMERA of a rig pose [p | q]: what slideWindowOld hands removeBackShiftDepthline (R = Rs ric, P = Ps + Rs tic)."""
    R, Rbc = ln.quat_R(np.asarray(pose7, float)[3:]), ln.quat_R(np.asarray(ex_cam, float)[3:])
    return np.concatenate([np.asarray(pose7, float)[:3] + R @ np.asarray(ex_cam, float)[:3], (R @ Rbc).ravel()])
