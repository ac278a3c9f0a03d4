"""TEST INFRASTRUCTURE. An independent numpy statement of the line landmarks' first stage — the checker of csrc/gfbe_line.h and
gfbe_line_refine. Written from the reference's formulas, vectorised over observations and lines, and deliberately different in structure
from the HIP code:
  * the factor's Jacobians are formed as the reference chains them: (2 x 6) d e / d Lc, the 6 x 6 transforms invTbc / invTwc and the
    6 x 4 d Lw / d orth, as full matrices (the device folds the zero blocks away);
  * the Levenberg-Marquardt loop (Ceres 1.14's TrustRegionMinimizer + LevenbergMarquardtStrategy with Jacobi scaling, as
    onlyLineOpt leaves the options) stacks every line's 4 x 4 block and solves them with numpy's batched Cholesky; the model cost change
    is computed from J and r (-(J s) . (r + J s / 2)), not from the normal equations;
  * removeLineOutlier forms the 4 x 4 Plücker matrix Lc and the planes through the camera centre literally.
References (the spec): line_projection_factor.cpp:18-231, line_parameterization.cpp:10-95, line_geometry.cpp:56-200,
estimator.cpp:4264-4332, feature_manager.cpp:1068-1150, 1372-1460.
"""
import numpy as np

WINDOW_SIZE, NFRAMES, LINE_MIN_OBS = 10, 11, 5


def skew(v):
    v = np.asarray(v, float)
    z = np.zeros(v.shape[:-1])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def quat_R(q):
    """Eigen's toRotationMatrix of (x, y, z, w) — also for a quaternion that is not exactly unit."""
    q = np.asarray(q, float)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def theta_R(th):
    th = np.asarray(th, float)
    Rx = np.zeros(th.shape[:-1] + (3, 3)); Ry = Rx.copy(); Rz = Rx.copy()
    c, s = np.cos(th), np.sin(th)
    Rx[..., 0, 0] = 1; Rx[..., 1, 1] = c[..., 0]; Rx[..., 1, 2] = -s[..., 0]; Rx[..., 2, 1] = s[..., 0]; Rx[..., 2, 2] = c[..., 0]
    Ry[..., 1, 1] = 1; Ry[..., 0, 0] = c[..., 1]; Ry[..., 0, 2] = s[..., 1]; Ry[..., 2, 0] = -s[..., 1]; Ry[..., 2, 2] = c[..., 1]
    Rz[..., 2, 2] = 1; Rz[..., 0, 0] = c[..., 2]; Rz[..., 0, 1] = -s[..., 2]; Rz[..., 1, 0] = s[..., 2]; Rz[..., 1, 1] = c[..., 2]
    return Rz @ Ry @ Rx        # = the reference's explicit R(theta)


def orth_to_plk(o):
    o = np.asarray(o, float)
    R = theta_R(o[..., :3])
    return np.concatenate([np.cos(o[..., 3:4]) * R[..., :, 0], np.sin(o[..., 3:4]) * R[..., :, 1]], -1)


def _angles(R):
    return np.stack([np.arctan2(R[..., 2, 1], R[..., 2, 2]), np.arcsin(-R[..., 2, 0]), np.arctan2(R[..., 1, 0], R[..., 0, 0])], -1)


def plk_to_orth(p):
    p = np.asarray(p, float)
    n, v = p[..., :3], p[..., 3:]
    nn, vn = np.linalg.norm(n, axis=-1), np.linalg.norm(v, axis=-1)
    u1, u2 = n / nn[..., None], v / vn[..., None]
    R = np.stack([u1, u2, np.cross(u1, u2)], -1)
    return np.concatenate([_angles(R), np.arcsin(vn / np.hypot(nn, vn))[..., None]], -1)


def plk_to_pose(p, R, t):
    """plk_to_pose(plk, Rcw, tcw): nc = R n + [t]x R v, vc = R v."""
    p = np.asarray(p, float)
    Rv = np.einsum("...ij,...j->...i", R, p[..., 3:])
    return np.concatenate([np.einsum("...ij,...j->...i", R, p[..., :3]) + np.cross(t, Rv), Rv], -1)


def plk_from_pose(p, R, t):
    Rt = np.swapaxes(R, -1, -2)
    return plk_to_pose(p, Rt, -np.einsum("...ij,...j->...i", Rt, t))


def orth_plus(x, d):
    x, d = np.asarray(x, float), np.asarray(d, float)
    R = theta_R(x[..., :3])
    z = np.zeros(d.shape[:-1])
    o = np.ones(d.shape[:-1])
    c, s = np.cos(d[..., :3]), np.sin(d[..., :3])
    Rx = np.stack([np.stack([o, z, z], -1), np.stack([z, c[..., 0], -s[..., 0]], -1), np.stack([z, s[..., 0], c[..., 0]], -1)], -2)
    Ry = np.stack([np.stack([c[..., 1], z, s[..., 1]], -1), np.stack([z, o, z], -1), np.stack([-s[..., 1], z, c[..., 1]], -1)], -2)
    Rz = np.stack([np.stack([c[..., 2], -s[..., 2], z], -1), np.stack([s[..., 2], c[..., 2], z], -1), np.stack([z, z, o], -1)], -2)
    Rn = R @ Rx @ Ry @ Rz
    phi = np.arcsin(np.sin(x[..., 3]) * np.cos(d[..., 3]) + np.cos(x[..., 3]) * np.sin(d[..., 3]))   # (W dW)(1, 0)
    return np.concatenate([_angles(Rn), phi[..., None]], -1)


def pose_plus(p7, d6):
    """PoseLocalParameterization: p + dp, q * [dtheta / 2, 1] normalised."""
    p7, d6 = np.asarray(p7, float), np.asarray(d6, float)
    q = p7[3:]
    dq = np.array([d6[3] / 2, d6[4] / 2, d6[5] / 2, 1.0])
    x1, y1, z1, w1 = q
    x2, y2, z2, w2 = dq
    qn = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                   w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
    return np.concatenate([p7[:3] + d6[:3], qn / np.linalg.norm(qn)])


def factor(pose, ex, orth, obs, sqrt_info=400.0, jac=True):
    """lineProjectionFactor over m observations: pose [m][7], ex [7], orth [m][4], obs [m][4] -> r [m][2] (and Jp, Je [m][2][7],
    Jo [m][2][4])."""
    pose, orth, obs, ex = (np.atleast_2d(np.asarray(a, float)) for a in (pose, orth, obs, ex))
    ex = ex[0]
    Rwb, twb = quat_R(pose[:, 3:]), pose[:, :3]
    Rbc, tbc = quat_R(ex[3:]), ex[:3]
    lw = orth_to_plk(orth)
    lb = plk_from_pose(lw, Rwb, twb)
    lc = plk_from_pose(lb, np.broadcast_to(Rbc, Rwb.shape), np.broadcast_to(tbc, twb.shape))
    nc = lc[:, :3]
    ln = nc[:, 0] ** 2 + nc[:, 1] ** 2
    ls, lt = np.sqrt(ln), ln * np.sqrt(ln)
    e1 = obs[:, 0] * nc[:, 0] + obs[:, 1] * nc[:, 1] + nc[:, 2]
    e2 = obs[:, 2] * nc[:, 0] + obs[:, 3] * nc[:, 1] + nc[:, 2]
    r = sqrt_info * np.stack([e1 / ls, e2 / ls], -1)
    if not jac:
        return r
    m = len(pose)
    jel = sqrt_info * np.stack([np.stack([obs[:, 0] / ls - nc[:, 0] * e1 / lt, obs[:, 1] / ls - nc[:, 1] * e1 / lt, 1 / ls], -1),
                                np.stack([obs[:, 2] / ls - nc[:, 0] * e2 / lt, obs[:, 3] / ls - nc[:, 1] * e2 / lt, 1 / ls], -1)], -2)
    jeLc = np.concatenate([jel, np.zeros((m, 2, 3))], -1)                        # 2 x 6
    RbcT = np.broadcast_to(Rbc.T, (m, 3, 3))
    invTbc = np.zeros((m, 6, 6))
    invTbc[:, :3, :3] = RbcT; invTbc[:, :3, 3:] = -RbcT @ skew(np.broadcast_to(tbc, (m, 3))); invTbc[:, 3:, 3:] = RbcT
    nw, dw = lw[:, :3], lw[:, 3:]
    RwbT = np.swapaxes(Rwb, -1, -2)
    jLp = np.zeros((m, 6, 6))
    jLp[:, :3, :3] = RwbT @ skew(dw)
    jLp[:, :3, 3:] = skew(np.einsum("mij,mj->mi", RwbT, nw + np.einsum("mij,mj->mi", skew(dw), twb)))
    jLp[:, 3:, 3:] = skew(np.einsum("mij,mj->mi", RwbT, dw))
    Jp = np.zeros((m, 2, 7)); Jp[:, :, :6] = jeLc @ invTbc @ jLp
    nb, db = lb[:, :3], lb[:, 3:]
    jLe = np.zeros((m, 6, 6))
    jLe[:, :3, :3] = RbcT @ skew(db)
    jLe[:, :3, 3:] = skew(np.einsum("mij,mj->mi", RbcT, nb + np.einsum("mij,mj->mi", skew(db), np.broadcast_to(tbc, (m, 3)))))
    jLe[:, 3:, 3:] = skew(np.einsum("mij,mj->mi", RbcT, db))
    Je = np.zeros((m, 2, 7)); Je[:, :, :6] = jeLc @ jLe
    Rwc = Rwb @ Rbc
    twc = np.einsum("mij,j->mi", Rwb, tbc) + twb
    RwcT = np.swapaxes(Rwc, -1, -2)
    invTwc = np.zeros((m, 6, 6))
    invTwc[:, :3, :3] = RwcT; invTwc[:, :3, 3:] = -RwcT @ skew(twc); invTwc[:, 3:, 3:] = RwcT
    nn, vn = np.linalg.norm(nw, axis=-1), np.linalg.norm(dw, axis=-1)
    u1, u2 = nw / nn[:, None], dw / vn[:, None]
    u3 = np.cross(u1, u2)
    w0, w1 = nn / np.hypot(nn, vn), vn / np.hypot(nn, vn)
    jLo = np.zeros((m, 6, 4))
    jLo[:, 3:, 0] = w1[:, None] * u3
    jLo[:, :3, 1] = -w0[:, None] * u3
    jLo[:, :3, 2] = w0[:, None] * u2
    jLo[:, 3:, 2] = -w1[:, None] * u1
    jLo[:, :3, 3] = -w1[:, None] * u1
    jLo[:, 3:, 3] = w0[:, None] * u2
    Jo = jeLc @ invTwc @ jLo
    return r, Jp, Je, Jo


def cauchy(s, a=1.0):
    """CauchyLoss(a): (1/2 rho(s), sqrt(rho'(s)))."""
    b = a * a
    return 0.5 * b * np.log1p(s / b), np.sqrt(1.0 / (1.0 + s / b))


def eval_robust(pose, ex, orth, obs, sqrt_info=400.0, robustify=True):
    r, Jp, Je, Jo = factor(pose, ex, orth, obs, sqrt_info)
    s = (r ** 2).sum(-1)
    if not robustify:
        return dict(r=r, J_pose=Jp, J_ex=Je, J_orth=Jo, cost=float(0.5 * s.sum()))
    c, sr = cauchy(s)
    k = sr[:, None]
    return dict(r=r * k, J_pose=Jp * k[:, :, None], J_ex=Je * k[:, :, None], J_orth=Jo * k[:, :, None], cost=float(c.sum()))


def eligible(lw):
    return (np.asarray(lw["n_obs"]) >= LINE_MIN_OBS) & (np.asarray(lw["start_frame"]) < WINDOW_SIZE - 2) & (np.asarray(lw["is_triangulation"]) != 0)


def cam_poses(lw):
    pose, ex = np.asarray(lw["pose"], float), np.asarray(lw["ex_cam"], float)
    Rs, Rbc = quat_R(pose[:, 3:]), quat_R(ex[3:])
    return Rs @ Rbc, pose[:, :3] + Rs @ ex[:3]


def cull_reason(plk_c, obs_line, s, Rwc, twc):
    """removeLineOutlier for one line: None (kept), 'behind', 'far' or 'reprojection'."""
    nc, vc = plk_c[:3], plk_c[3:]
    Lc = np.zeros((4, 4))
    Lc[:3, :3] = skew(nc); Lc[:3, 3] = vc; Lc[3, :3] = -vc
    o = obs_line[0]
    p11, p21 = np.array([o[0], o[1], 1.0]), np.array([o[2], o[3], 1.0])
    ln = np.cross(p11, p21)[:2]
    ln = ln / np.linalg.norm(ln)
    p12, p22 = np.array([p11[0] + ln[0], p11[1] + ln[1], 1.0]), np.array([p21[0] + ln[0], p21[1] + ln[1], 1.0])
    cam = np.zeros(3)

    def pi_from_ppp(x1, x2, x3):
        return np.concatenate([np.cross(x1 - x3, x2 - x3), [-x3 @ np.cross(x1, x2)]])
    e1, e2 = Lc @ pi_from_ppp(cam, p11, p12), Lc @ pi_from_ppp(cam, p21, p22)
    e1, e2 = e1 / e1[3], e2 / e2[3]
    if e1[2] < 0 or e2[2] < 0:
        return "behind"
    if np.linalg.norm(e1 - e2) > 10:
        return "far"
    lw = plk_to_pose(plk_c, Rwc[s], twc[s])
    allerr = 0.0
    for k, ob in enumerate(obs_line):
        lc = plk_from_pose(lw, Rwc[s + k], twc[s + k])
        n = lc[:3] / np.linalg.norm(lc[:2])
        err = (abs(n @ [ob[0], ob[1], 1.0]) + abs(n @ [ob[2], ob[3], 1.0])) / 2.0
        allerr = max(allerr, err)
    return "reprojection" if allerr > 3.0 / 500.0 else None


def refine(lw, sqrt_info=400.0, cauchy_scale=1.0, max_num_iterations=8):
    """onlyLineOpt + removeLineOutlier of one window: dict(plucker, keep, reason [n], summary)."""
    sf, no = np.asarray(lw["start_frame"]), np.asarray(lw["n_obs"])
    obs = np.asarray(lw["obs"], float).reshape(-1, 4)
    plk_in = np.asarray(lw["line_plucker"], float).reshape(-1, 6)
    n = len(sf)
    off = np.concatenate([[0], np.cumsum(no)])
    el = np.flatnonzero(eligible(lw))
    Rwc, twc = cam_poses(lw)
    pose, ex = np.asarray(lw["pose"], float), np.asarray(lw["ex_cam"], float)
    out, keep, reason = plk_in.copy(), np.ones(n, bool), [None] * n
    if len(el) < 4:
        return dict(plucker=out, keep=keep, reason=reason,
                    summary=dict(status=0, iterations=0, num_successful=0, termination=5, cost_history=[0.0], accepted=[0]))
    # the observations of the eligible lines, stacked: owner line (0..L-1), frame
    own = np.concatenate([np.full(no[l], q) for q, l in enumerate(el)])
    frm = np.concatenate([sf[l] + np.arange(no[l]) for l in el])
    ob = np.concatenate([obs[off[l]:off[l + 1]] for l in el])
    L = len(el)
    x = plk_to_orth(plk_to_pose(plk_in[el], Rwc[sf[el]], twc[sf[el]]))

    def evaluate(xx, jac):
        res = factor(pose[frm], ex, xx[own], ob, sqrt_info, jac)
        r, Jo = (res[0], res[3]) if jac else (res, None)
        c, sr = cauchy((r ** 2).sum(-1), cauchy_scale)
        cost = c.sum()
        if not jac:
            return cost
        return cost, r * sr[:, None], Jo * sr[:, None, None]

    def linearise(xx):
        cost, r, J = evaluate(xx, True)
        H, g = np.zeros((L, 4, 4)), np.zeros((L, 4))
        np.add.at(H, own, np.einsum("mia,mib->mab", J, J))
        np.add.at(g, own, np.einsum("mia,mi->ma", J, r))
        gmax = np.abs(xx - orth_plus(xx, -g)).max()
        return cost, r, J, H, g, gmax

    cost, r, J, H, g, gmax = linearise(x)
    scale = 1.0 / (1.0 + np.sqrt(np.einsum("lii->li", H)))
    radius, decrease, x_norm = 1e4, 2.0, np.linalg.norm(x)
    sm = dict(status=1, iterations=0, num_successful=0, termination=0, initial_cost=cost, cost_history=[cost], accepted=[0])
    it, invalid, reuse, diag2 = 0, 0, False, None
    max_it = min(max_num_iterations, 15)
    while True:
        if it >= max_it:
            sm["termination"] = 0
            break
        if gmax <= 1e-10:
            sm["termination"], sm["status"] = 3, 0
            break
        if radius < 1e-32:
            sm["termination"] = 4
            break
        it += 1
        Js = J * scale[own][:, None, :]
        Hs = H * scale[:, :, None] * scale[:, None, :]
        if not reuse:
            diag2 = np.clip(np.einsum("lii->li", Hs), 1e-6, 1e32)
        A = Hs + np.einsum("li,ij->lij", diag2 / radius, np.eye(4))
        try:
            Lc = np.linalg.cholesky(A)
            y = -np.linalg.solve(np.swapaxes(Lc, -1, -2), np.linalg.solve(Lc, (scale * g)[..., None]))[..., 0]
            model_r = np.einsum("mia,ma->mi", Js, y[own])
            mc = -(model_r * (r + model_r / 2)).sum()
            ok = True
        except np.linalg.LinAlgError:
            ok = False
        if not ok or not (mc > 0):
            sm["accepted"].append(0); sm["cost_history"].append(cost)
            invalid += 1
            if invalid >= 5:
                sm["termination"], sm["status"] = 4, 2
                break
            radius /= decrease; decrease *= 2; reuse = True
            continue
        invalid = 0
        cand = orth_plus(x, scale * y)
        cand_cost = evaluate(cand, False)
        step = np.linalg.norm(cand - x)
        hist_at = len(sm["cost_history"])
        sm["cost_history"].append(cost); sm["accepted"].append(0)
        assert hist_at == it
        if step <= 1e-8 * (x_norm + 1e-8):
            sm["termination"], sm["status"] = 2, 0
            break
        change = cost - cand_cost
        if abs(change) <= 1e-6 * cost:
            sm["termination"], sm["status"] = 1, 0
            break
        rho = change / mc
        if rho > 1e-3:
            x, x_norm = cand, np.linalg.norm(cand)
            sm["accepted"][it], sm["cost_history"][it] = 1, cand_cost
            sm["num_successful"] += 1
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease, reuse = 2.0, False
            cost, r, J, H, g, gmax = linearise(x)
            cost = cand_cost
        else:
            radius /= decrease; decrease *= 2; reuse = True
    sm.update(iterations=it, final_cost=cost, final_radius=radius)
    out[el] = plk_from_pose(orth_to_plk(x), Rwc[sf[el]], twc[sf[el]])
    for l in el:
        reason[l] = cull_reason(out[l], obs[off[l]:off[l + 1]], sf[l], Rwc, twc)
        keep[l] = reason[l] is None
    return dict(plucker=out, keep=keep, reason=reason, summary=sm, x=x)


def sensitivity(lw, **kw):
    """How far this checker's own result moves when the input lines change by one part in 1e15 (the size of a rounding difference):
    (relative change of the final cost, per-line max |change| of the written-back Plücker lines). A window with a line that wanders
    far from its start inside the joint trust region (such lines end up culled) turns rounding into differences of up to ~1e-4; two
    correct implementations that sum in different orders can differ by that much there, and by no more than ~1e-12 elsewhere."""
    a = refine(lw, **kw)
    lw2 = dict(lw)
    lw2["line_plucker"] = np.asarray(lw["line_plucker"], float) * (1 + 1e-15)
    b = refine(lw2, **kw)
    fa, fb = a["summary"].get("final_cost", 0.0), b["summary"].get("final_cost", 0.0)
    return abs(fa - fb) / max(abs(fa), 1e-300), np.abs(a["plucker"] - b["plucker"]).max(1)
