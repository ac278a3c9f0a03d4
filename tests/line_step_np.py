"""TEST INFRASTRUCTURE. The numpy checker of gfbe_line_step / gfbe_ltab_step / gfbe_ltab_commit (csrc/gfbe_line_step.hip): the step half
of a joint trust-region iteration over a window's line blocks, in the dtype the caller asks for (FP64 restatement and numpy.longdouble
reference are the same code), built on tests/line_reduce_np.py. tests/test_line_step_host.py pins it against the dense joint system.

Conventions (include/gfbe.h): line columns unscaled, the block's metric d2_l = clamp(diag V_l, 1e-6, 1e32); with the records Vinv, bl, W, V
    y_l = Vinv (bl - W^T y_p),  v_l = bl / d2_l
    G2 = sum bl^2 / d2, N2 = sum d2 y_l^2, gy = bl . y_l, vHv = 2 v_l . W^T v_p + v_l^T V v_l,
    vHy = v_l . W^T y_p + y_l . W^T v_p + v_l^T V y_l, yHy = 2 y_l . W^T y_p + y_l^T V y_l, max |x_l - Plus(x_l, -bl)|_inf, |x_l|^2
total = rest + shares; the three-branch dogleg rule; delta_l = c1 v_l + c2 y_l, x_l' = Plus(x_l, delta_l); candidate poses = pose_plus;
plucker_cand in the candidate start camera; cost_cand = sum 1/2 rho_huber at the candidates.

The records are INPUTS of the step (the device's own, in the GPU test): the checker takes them as exact. Beside every array X it returns
A_X, the scale of its rounding error, first order: the absolute sum behind the entry plus the allowances of what it is formed from,
  a_wty = |W|^T |y_p|;  A_yl = |Vinv| (|bl| + a_wty);  A_vl = |v_l|
  A_gram   the shares' absolute sums with |y_l| + A_yl for y_l and a_wt* for W^T *; entry 6: (1 + |x| + |Plus|) / cos (see _orth_cond)
  A_total  |rest| + A_gram
  A_coef   |coef| + sum_k |d coef / d total_k| A_total_k, the derivative by central differences of the dogleg rule (held on its branch)
           in longdouble
  A_delta  A_c1 |v_l| + A_c2 |y_l| + |c1| |v_l| + |c2| (|y_l| + A_yl); the pose step likewise
  A_orth   cond (1 + |x'| + |A_delta|_1 + s_x): the Euler angles of a rotation product, read back through atan2 / asin; cond = 1 / cos of
           the middle angle (1 / cos phi for the fourth), s_x the same allowance for the line x_l itself (formed from the Plücker vector)
  A_pose   position |p| + A_step; quaternion 1 + |A_step(rotation)|_1 / 2
  A_plk    |R^T| (|n| + |t| x |v|) (1 + s_R) + s_o (1 + |t|_1) + a_t for the moment, |R^T| |v| (1 + s_R) + s_o for the direction, with
           s_o = |A_orth|_1, s_R / a_t the rotation / translation allowances of the candidate camera
  A_cost   cost + sum_obs rho' (|r_1| A_r1 + |r_2| A_r2), A_r through e / |l| from the plain absolute sums |R^T| (|n| + |t| x |v|) of the
           line in the observing camera - as the plain sums of tests/line_reduce_np.py, the errors of the factors themselves (the line's
           trigonometric parameters, the candidate poses) are not in it and show in r_cpu
K_X: the smallest power of two >= 4 r_cpu[X], r_cpu the worst |X_64 - X_ld| / (u A_X) of this checker in FP64 against itself in
longdouble over all cases (R_CPU below; tests/test_line_step_host.py asserts that they do not drift upwards): the headroom the K of
tests/line_reduce_np.py have over their r_cpu.
"""
import numpy as np

import line_np as ln
import line_reduce_np as lr

LD, UNIT = lr.LD, lr.UNIT
D = lr.NP_DIM
COST_INVALID = 1.7976931348623157e308
ARRAYS = ("gram", "total", "coef", "y_l", "v_l", "orth_cand", "plucker_cand", "pose_cand", "ex_cand", "cost_cand")
# worst FP64-vs-longdouble ratios of this checker per array over all cases, mu in {0, 1} and the three radii (measured on the CPU)
R_CPU = dict(gram=5.18, total=2.36, coef=2.03, y_l=1.68, v_l=0.99, orth_cand=1.37, plucker_cand=0.12, pose_cand=1.33, ex_cand=1.33,
             cost_cand=8.97e8, V=9668.0)
K = {k: float(2 ** int(np.ceil(np.log2(4 * r)))) for k, r in R_CPU.items()}


# ---- small pieces in the caller's dtype
def tri_to_full(Vlow):
    Vlow = np.asarray(Vlow)
    V = np.zeros(Vlow.shape[:-1] + (4, 4), Vlow.dtype)
    q = 0
    for i in range(4):
        for j in range(i + 1):
            V[..., i, j] = Vlow[..., q]
            V[..., j, i] = Vlow[..., q]
            q += 1
    return V


def full_to_tri(V):
    V = np.asarray(V)
    return np.stack([V[..., i, j] for i in range(4) for j in range(i + 1)], -1)


def orth_plus(x, d):
    """LineOrthParameterization::Plus in the arrays' dtype (line_np.orth_plus is FP64 only)."""
    R = lr._theta_R(x[..., :3])
    z, o = np.zeros(d.shape[:-1], x.dtype), np.ones(d.shape[:-1], x.dtype)
    c, s = np.cos(d[..., :3]), np.sin(d[..., :3])
    Rx = np.stack([np.stack([o, z, z], -1), np.stack([z, c[..., 0], -s[..., 0]], -1), np.stack([z, s[..., 0], c[..., 0]], -1)], -2)
    Ry = np.stack([np.stack([c[..., 1], z, s[..., 1]], -1), np.stack([z, o, z], -1), np.stack([-s[..., 1], z, c[..., 1]], -1)], -2)
    Rz = np.stack([np.stack([c[..., 2], -s[..., 2], z], -1), np.stack([s[..., 2], c[..., 2], z], -1), np.stack([z, z, o], -1)], -2)
    Rn = R @ Rx @ Ry @ Rz
    phi = np.arcsin(np.sin(x[..., 3]) * np.cos(d[..., 3]) + np.cos(x[..., 3]) * np.sin(d[..., 3]))
    return np.stack([np.arctan2(Rn[..., 2, 1], Rn[..., 2, 2]), np.arcsin(-Rn[..., 2, 0]), np.arctan2(Rn[..., 1, 0], Rn[..., 0, 0]), phi], -1)


def pose_plus(p7, d6):
    """PoseLocalParameterization::Plus as the device forms it: p + dp, normalise(q * normalise([dtheta / 2, 1]))."""
    dt = p7.dtype.type
    dq = np.concatenate([d6[..., 3:] / dt(2), np.ones(d6.shape[:-1] + (1,), p7.dtype)], -1)
    dq = dq / np.sqrt((dq * dq).sum(-1))[..., None]
    x1, y1, z1, w1 = (p7[..., 3 + k] for k in range(4))
    x2, y2, z2, w2 = (dq[..., k] for k in range(4))
    qn = np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                   w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)
    return np.concatenate([p7[..., :3] + d6[..., :3], qn / np.sqrt((qn * qn).sum(-1))[..., None]], -1)


def dogleg(T, radius, force=None):
    """The three-branch rule of k_step on the totals T: (coef [c1, c2, step_norm, model_change], branch, margin). force: hold the
    branch (for derivatives). margin: the smallest relative distance of a branch condition that was tested from its boundary."""
    dt = T.dtype.type
    G2, N2, gy, vHv, vHy, yHy = T[:6]
    radius = dt(radius)
    with np.errstate(all="ignore"):
        alpha = G2 / vHv
        g_norm, gn_norm = np.sqrt(G2), np.sqrt(N2)
        m0 = abs(gn_norm - radius) / radius if radius > 0 else dt(1)
        m1 = abs(g_norm * alpha - radius) / radius if radius > 0 else dt(1)
        branch = force if force is not None else (0 if gn_norm <= radius else (1 if g_norm * alpha >= radius else 2))
        if branch == 0:
            c1, c2, step_norm, margin = dt(0), dt(-1), gn_norm, m0
        elif branch == 1:
            c1, c2, step_norm, margin = -radius / g_norm, dt(0), radius, min(m0, m1)
        else:
            b_dot_a = alpha * gy
            a_sq = (alpha * g_norm) * (alpha * g_norm)
            bma = a_sq - dt(2) * b_dot_a + N2
            cc = b_dot_a - a_sq
            dd = np.sqrt(cc * cc + bma * (radius * radius - a_sq))
            beta = (dd - cc) / bma if cc <= 0 else (radius * radius - a_sq) / (dd + cc)
            c1, c2 = -alpha * (dt(1) - beta), -beta
            step_norm = np.sqrt(max(dt(0), c1 * c1 * G2 + dt(2) * c1 * c2 * gy + c2 * c2 * N2))
            margin = min(m0, m1)
        mc = -(c1 * G2 + c2 * gy) - dt(0.5) * (c1 * c1 * vHv + dt(2) * c1 * c2 * vHy + c2 * c2 * yHy)
    return np.array([c1, c2, step_norm, mc], T.dtype), branch, margin


def radii_for(T):
    """Three radii that take the three branches at the totals T (Gauss-Newton inside, Cauchy point outside, the dogleg between)."""
    T = np.asarray(T, LD)
    gn, cauchy = float(np.sqrt(T[1])), float(np.sqrt(T[0]) * T[0] / T[3])
    return [2.0 * gn, 0.5 * cauchy, float(np.sqrt(gn * cauchy))]


def _coef_scale(T, A_T, radius, branch, coef):
    Tl = np.asarray(T, LD)
    A = np.abs(np.asarray(coef, LD))
    for k in range(6):
        h = LD(1e-7) * max(abs(Tl[k]), LD(1e-300))
        up, dn = Tl.copy(), Tl.copy()
        up[k] += h
        dn[k] -= h
        dc = (dogleg(up, radius, branch)[0] - dogleg(dn, radius, branch)[0]) / (2 * h)
        A = A + np.abs(np.where(np.isfinite(dc), dc, 0)) * LD(A_T[k])
    return A


def _orth_cond(x):
    """1 / cos of the angle the orthonormal parameters are read back through: theta_1 for the three Euler angles, phi for the fourth."""
    c = np.abs(np.cos(x[..., [1, 1, 1, 3]]))
    return 1 / np.maximum(c, x.dtype.type(1e-300))


def _abscross(a, b):
    return np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1)


def _cams(pose, ex):
    Rs, Rbc = lr._quat_R(pose[:, 3:]), lr._quat_R(ex[3:])
    return Rs @ Rbc, pose[:, :3] + lr._mv(Rs, np.broadcast_to(ex[:3], (len(pose), 3)))


def line_blocks(lw, sqrt_info=400.0, width=1.0, dtype=np.float64):
    """Per entering line (solve mode, list order): x_l, V_l WITHOUT the mu term [n][4][4] and its absolute sum A_V."""
    sf, no = np.asarray(lw["start_frame"]), np.asarray(lw["n_obs"])
    obs = np.asarray(lw["obs"], dtype).reshape(-1, 4)
    off = np.concatenate([[0], np.cumsum(no)]).astype(int)
    pose, ex = np.asarray(lw["pose"], dtype).reshape(lr.NFRAMES, 7), np.asarray(lw["ex_cam"], dtype)
    Rwc, twc = _cams(pose, ex)
    el = np.flatnonzero(lr.entering(lw, lr.SOLVE))
    plk = np.asarray(lw["line_plucker"], dtype).reshape(-1, 6)
    x, V, A_V = np.zeros((len(el), 4), dtype), np.zeros((len(el), 4, 4), dtype), np.zeros((len(el), 4, 4), dtype)
    for q, l in enumerate(el):
        s, m = int(sf[l]), int(no[l])
        x[q] = lr.plk_to_orth(lr.plk_to_pose(plk[l], Rwc[s], twc[s]))
        fr = np.arange(s, s + m)
        Jo = lr.eval_huber(pose[fr], ex, np.broadcast_to(x[q], (m, 4)), obs[off[l]:off[l] + m], sqrt_info, width, dtype)[3]
        V[q], A_V[q] = np.einsum("kia,kib->ab", Jo, Jo), np.einsum("kia,kib->ab", np.abs(Jo), np.abs(Jo))
    return x, V, A_V


def records_of(red, V):
    """The records gfbe_line_reduce hands to the step, from lr.reduce's result and line_blocks' V (failed lines zeroed, as the device does)."""
    ok = (red["failed"] == 0)
    z = lambda a: np.where(ok.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0)       # noqa: E731
    return dict(Vinv=z(red["Vinv"]), bl=z(red["bl"]), W=z(red["W"]), V=z(full_to_tri(V)), failed=red["failed"].copy())


def step(lw, rec, y_p, v_p, rest, radius, sqrt_info=400.0, width=1.0, dtype=np.float64):
    """One window. rec: Vinv [n][4][4], bl [n][4], W [n][72][4], V [n][10], failed [n] of the entering lines. dict: gram, total, coef,
    invalid, branch, margin, y_l, v_l, orth_cand, plucker_cand, pose_cand, ex_cand, cost_cand, x (the lines), and A_<array>."""
    dt = np.dtype(dtype).type
    sf, no = np.asarray(lw["start_frame"]), np.asarray(lw["n_obs"])
    obs = np.asarray(lw["obs"], dtype).reshape(-1, 4)
    off = np.concatenate([[0], np.cumsum(no)]).astype(int)
    pose, ex = np.asarray(lw["pose"], dtype).reshape(lr.NFRAMES, 7), np.asarray(lw["ex_cam"], dtype)
    Rwc, twc = _cams(pose, ex)
    el = np.flatnonzero(lr.entering(lw, lr.SOLVE))
    n = len(el)
    s_l = sf[el].astype(int)
    plk_in = np.asarray(lw["line_plucker"], dtype).reshape(-1, 6)[el]
    x = lr.plk_to_orth(lr.plk_to_pose(plk_in, Rwc[s_l], twc[s_l])) if n else np.zeros((0, 4), dtype)
    ok = np.asarray(rec["failed"]).reshape(n) == 0
    W, Vinv = np.asarray(rec["W"], dtype).reshape(n, D, 4), np.asarray(rec["Vinv"], dtype).reshape(n, 4, 4)
    bl, V = np.asarray(rec["bl"], dtype).reshape(n, 4), tri_to_full(np.asarray(rec["V"], dtype).reshape(n, 10))
    yp, vp, rest = np.asarray(y_p, dtype).reshape(D), np.asarray(v_p, dtype).reshape(D), np.asarray(rest, dtype).reshape(8)
    aW, aV, abl = np.abs(W), np.abs(V), np.abs(bl)
    wty, wtv = np.einsum("npa,p->na", W, yp), np.einsum("npa,p->na", W, vp)
    a_wty, a_wtv = np.einsum("npa,p->na", aW, np.abs(yp)), np.einsum("npa,p->na", aW, np.abs(vp))
    d2 = np.clip(np.einsum("naa->na", V), dt(1e-6), dt(1e32))
    okc = ok[:, None]
    with np.errstate(all="ignore"):
        vl = np.where(okc, bl / d2, 0)
        yl = np.where(okc, np.einsum("nab,nb->na", Vinv, bl - wty), 0)
        A_yl = np.where(okc, np.einsum("nab,nb->na", np.abs(Vinv), abl + a_wty), 0)
    A_vl = np.abs(vl)
    ay = np.abs(yl) + A_yl                     # |y_l| with its allowance
    av = np.abs(vl)
    xm = orth_plus(x, -bl) if n else x
    g6 = np.abs(x - xm).max(-1) if n else np.zeros(0, dtype)
    A6 = ((1 + np.abs(x) + np.abs(xm)) * _orth_cond(xm)).max(-1) if n else np.zeros(0, dtype)
    sh = np.stack([(bl * bl / d2).sum(-1), (d2 * yl * yl).sum(-1), (bl * yl).sum(-1),
                   2 * (vl * wtv).sum(-1) + np.einsum("na,nab,nb->n", vl, V, vl),
                   (vl * wty).sum(-1) + (yl * wtv).sum(-1) + np.einsum("na,nab,nb->n", vl, V, yl),
                   2 * (yl * wty).sum(-1) + np.einsum("na,nab,nb->n", yl, V, yl), g6, (x * x).sum(-1)], -1) if n else np.zeros((0, 8), dtype)
    A_sh = np.stack([(bl * bl / d2).sum(-1), (d2 * (yl * yl + 2 * np.abs(yl) * A_yl)).sum(-1), (abl * ay).sum(-1),
                     2 * (av * a_wtv).sum(-1) + np.einsum("na,nab,nb->n", av, aV, av),
                     (av * a_wty).sum(-1) + (ay * a_wtv).sum(-1) + np.einsum("na,nab,nb->n", av, aV, ay),
                     2 * (ay * a_wty).sum(-1) + np.einsum("na,nab,nb->n", ay, aV, ay), A6, (x * x).sum(-1)], -1) if n else np.zeros((0, 8), dtype)
    sh, A_sh = sh[ok], A_sh[ok]
    gram, A_gram = np.zeros(8, dtype), np.zeros(8, dtype)
    if len(sh):
        gram, A_gram = sh.sum(0), A_sh.sum(0)
        gram[6], A_gram[6] = sh[:, 6].max(), A_sh[:, 6].max()
    total, A_total = rest + gram, np.abs(rest) + A_gram
    total[6], A_total[6] = max(rest[6], gram[6]), max(abs(rest[6]), A_gram[6])
    coef, branch, margin = dogleg(total, radius)
    invalid = not coef[3] > 0
    A_coef = _coef_scale(total, A_total, radius, branch, coef).astype(dtype)
    s_x = ((1 + np.abs(x)) * _orth_cond(x)).sum(-1) if n else np.zeros(0, dtype)
    out = dict(gram=gram, total=total, coef=coef, invalid=int(invalid), branch=branch, margin=float(margin), y_l=yl, v_l=vl, x=x,
               A_gram=A_gram, A_total=A_total, A_coef=A_coef, A_y_l=A_yl, A_v_l=A_vl)
    A_x = (1 + np.abs(x)) * _orth_cond(x) + s_x[:, None] if n else np.zeros((0, 4), dtype)
    if invalid:
        out.update(orth_cand=x.copy(), A_orth_cand=A_x, plucker_cand=plk_in.copy(), A_plucker_cand=np.zeros((n, 6), dtype),
                   pose_cand=pose.copy(), A_pose_cand=np.zeros((lr.NFRAMES, 7), dtype), ex_cand=ex.copy(), A_ex_cand=np.zeros(7, dtype),
                   cost_cand=dt(COST_INVALID), A_cost_cand=dt(0))
        return out
    c1, c2, A_c1, A_c2 = coef[0], coef[1], A_coef[0], A_coef[1]
    # candidate poses / extrinsic
    dp = c1 * vp + c2 * yp
    A_dp = A_c1 * np.abs(vp) + A_c2 * np.abs(yp) + np.abs(c1 * vp) + np.abs(c2 * yp)
    blocks = np.concatenate([pose, ex[None]], 0)
    cand = pose_plus(blocks, dp.reshape(12, 6))
    A_blocks = np.concatenate([np.abs(blocks[:, :3]) + A_dp.reshape(12, 6)[:, :3],
                               np.broadcast_to(1 + A_dp.reshape(12, 6)[:, 3:].sum(-1, keepdims=True) / 2, (12, 4))], -1)
    pose_c, ex_c = cand[:11], cand[11]
    # candidate lines
    dl = c1 * vl + c2 * yl
    A_dl = A_c1 * av + A_c2 * np.abs(yl) + abs(c1) * av + abs(c2) * ay
    xc = np.where(okc, orth_plus(x, dl), x) if n else x
    A_xc = np.where(okc, _orth_cond(xc) * (1 + np.abs(xc) + A_dl.sum(-1, keepdims=True) + s_x[:, None]), A_x) if n else A_x
    Rc, tc = _cams(pose_c, ex_c)
    s_Rf = 2 * (A_blocks[:11, 3:].sum(-1) + A_blocks[11, 3:].sum())            # rotation allowance of a frame's candidate camera
    a_tf = A_blocks[:11, :3].sum(-1) + np.abs(ex_c[:3]).sum() * s_Rf + A_blocks[11, :3].sum()
    lwc = lr.orth_to_plk(xc) if n else np.zeros((0, 6), dtype)
    s_o = A_xc.sum(-1)

    def in_camera(lines, frames, so, plain=False):
        """The lines in the cameras of `frames`: Plücker vector and its allowance."""
        R, t = Rc[frames], tc[frames]
        got = lr.plk_from_pose(lines, R, t)
        aRt = np.abs(np.swapaxes(R, -1, -2))
        absn = lr._mv(aRt, np.abs(lines[..., :3]) + _abscross(np.abs(t), np.abs(lines[..., 3:])))
        absv = lr._mv(aRt, np.abs(lines[..., 3:]))
        if plain:
            return got, np.concatenate([absn, absv], -1)
        sR, at = s_Rf[frames][:, None], a_tf[frames][:, None]
        A = np.concatenate([absn * (1 + sR) + so[:, None] * (1 + np.abs(t).sum(-1, keepdims=True)) + at, absv * (1 + sR) + so[:, None]], -1)
        return got, A
    if n:
        plk_c, A_plk = in_camera(lwc, s_l, s_o)
        plk_c, A_plk = np.where(okc, plk_c, plk_in), np.where(okc, A_plk, 0)
    else:
        plk_c, A_plk = np.zeros((0, 6), dtype), np.zeros((0, 6), dtype)
    # candidate cost over the observations of the non-failed entering lines
    li = np.concatenate([np.full(int(no[l]), q) for q, l in enumerate(el) if ok[q]] + [np.zeros(0, int)]).astype(int)
    fi = np.concatenate([np.arange(int(sf[l]), int(sf[l] + no[l])) for q, l in enumerate(el) if ok[q]] + [np.zeros(0, int)]).astype(int)
    oi = np.concatenate([np.arange(off[l], off[l + 1]) for q, l in enumerate(el) if ok[q]] + [np.zeros(0, int)]).astype(int)
    cost, A_cost = dt(0), dt(0)
    if len(li):
        lc, A_lc = in_camera(lwc[li], fi, s_o[li], plain=True)
        ob = obs[oi]
        si = dt(sqrt_info)
        ls = np.sqrt(lc[:, 0] ** 2 + lc[:, 1] ** 2)
        e = np.stack([ob[:, 0] * lc[:, 0] + ob[:, 1] * lc[:, 1] + lc[:, 2], ob[:, 2] * lc[:, 0] + ob[:, 3] * lc[:, 1] + lc[:, 2]], -1)
        a_e = np.stack([np.abs(ob[:, 0]) * A_lc[:, 0] + np.abs(ob[:, 1]) * A_lc[:, 1] + A_lc[:, 2],
                        np.abs(ob[:, 2]) * A_lc[:, 0] + np.abs(ob[:, 3]) * A_lc[:, 1] + A_lc[:, 2]], -1)
        A_ls = (np.abs(lc[:, 0]) * A_lc[:, 0] + np.abs(lc[:, 1]) * A_lc[:, 1]) / ls
        r = si * e / ls[:, None]
        A_r = si * (a_e / ls[:, None] + np.abs(e) * (A_ls / (ls * ls))[:, None])
        c, sr = lr.huber((r * r).sum(-1), width)
        cost = c.sum()
        A_cost = cost + (sr * sr * (np.abs(r) * A_r).sum(-1)).sum()
    out.update(orth_cand=xc, A_orth_cand=A_xc, plucker_cand=plk_c, A_plucker_cand=A_plk, pose_cand=pose_c, A_pose_cand=A_blocks[:11],
               ex_cand=ex_c, A_ex_cand=A_blocks[11], cost_cand=cost, A_cost_cand=A_cost)
    return out


def ratios(got, ref, arrays=ARRAYS):
    """Per array: (worst |got - ref| / (u A), entries that differ where A is zero)."""
    res = {}
    for k in arrays:
        x, y, a = np.asarray(got[k], LD), np.asarray(ref[k], LD), np.asarray(ref["A_" + k], LD)
        x, y, a = np.broadcast_arrays(x, y, a)
        nz = a > 0
        with np.errstate(all="ignore"):
            worst = float((np.abs(x - y)[nz] / (UNIT * a[nz])).max()) if nz.any() else 0.0
        res[k] = (worst, int((x[~nz] != y[~nz]).sum()))
    return res


# ---- the caller's side of a joint iteration: everything that is not a line block
def rest_of_window(seed, scale=1.0):
    """A seeded SPD 72 x 72 `rest of the window` P with its gradient q (FP64 values; the tests widen them). Its spectrum spans four
    decades: with a well-conditioned P the damped Gauss-Newton step at mu = 1 is shorter than the Cauchy step and the dogleg branch
    cannot be reached at any radius."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(0, 1, (D, D)))[0]
    P = (Q * np.logspace(-3, 1, D)) @ Q.T
    return scale * (P + P.T) / 2, np.sqrt(scale) * rng.normal(0, 1, D)


def solve(A, b):
    """Gaussian elimination with partial pivoting in the arrays' dtype (numpy.linalg has no extended precision)."""
    A, b = A.copy(), b.copy()
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:]
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, A.dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def caller_side(H, g, U, bp, P, q, mu, x_norm2=0.0, dtype=np.float64):
    """From the reduce's H, g, U, bp and the rest of the window (P, q): D_p^2 = clamp(diag(U + P)), y_p solving
    (H + P + mu D_p^2) y = g + q, v_p = (bp + q) / D_p^2 and the eight scalars of the 72 dims (entry 7: x_norm2, the caller's |x|^2)."""
    dt = np.dtype(dtype).type
    H, g, U, bp, P, q = (np.asarray(a, dtype) for a in (H, g, U, bp, P, q))
    A = U + P
    Dp2 = np.clip(np.diag(A), dt(1e-6), dt(1e32))
    y = solve(H + P + dt(mu) * np.diag(Dp2), g + q)
    gp = bp + q
    v = gp / Dp2
    rest = np.array([(gp * gp / Dp2).sum(), (Dp2 * y * y).sum(), gp @ y, v @ A @ v, v @ A @ y, y @ A @ y, np.abs(gp).max(), dt(x_norm2)], dtype)
    return y, v, rest, Dp2


# ---- a closed trust-region loop over lines + a quadratic on the 72 dims (ops: the numpy checker here, the device in the GPU test)
def _local(pose, ex, ref):
    """z(x) [72]: the 72 dims' coordinates relative to the reference blocks (p - p_ref, 2 vec(q_ref^-1 q)), and d z / d tangent."""
    blocks, z, J = np.concatenate([pose, ex[None]], 0), np.zeros(D), np.zeros((D, D))
    for b in range(12):
        x1, y1, z1, w1 = ref[b, 3:] * np.array([-1, -1, -1, 1])
        x2, y2, z2, w2 = blocks[b, 3:]
        dq = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2, w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2,
                       w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
        z[6 * b:6 * b + 3] = blocks[b, :3] - ref[b, :3]
        z[6 * b + 3:6 * b + 6] = 2 * dq[:3]
        J[6 * b:6 * b + 3, 6 * b:6 * b + 3] = np.eye(3)
        J[6 * b + 3:6 * b + 6, 6 * b + 3:6 * b + 6] = dq[3] * np.eye(3) + ln.skew(dq[:3])
    return z, J


class Quadratic:
    """cost_P(x) = 1/2 (z(x) - z*)^T P0 (z(x) - z*): at(pose, ex) returns the cost, its Gauss-Newton block P = J^T P0 J and its
    gradient J^T P0 (z - z*) (the sign of g = J^T r in (H + mu D^2) y = g; the step is -y) at the current blocks."""

    def __init__(self, P0, zstar, ref):
        self.P0, self.zstar, self.ref = P0, zstar, ref

    def at(self, pose, ex):
        z, J = _local(pose, ex, self.ref)
        e = z - self.zstar
        return 0.5 * e @ self.P0 @ e, J.T @ self.P0 @ J, J.T @ self.P0 @ e


class NumpyOps:
    """reduce / step / commit of the closed loop on the numpy checker (FP64), the line window held as a dict."""

    def __init__(self, lw, sqrt_info=400.0, width=1.0):
        self.lw, self.si, self.width = dict(lw), sqrt_info, width

    def reduce(self, mu):
        red = lr.reduce(self.lw, lr.SOLVE, self.si, self.width, mu)
        self.rec = records_of(red, line_blocks(self.lw, self.si, self.width)[1])
        return red

    def step(self, y, v, rest, radius):
        self.last = step(self.lw, self.rec, y, v, rest, radius, self.si, self.width)
        return self.last

    def commit(self, accept):
        if accept:
            el = np.flatnonzero(lr.entering(self.lw, lr.SOLVE))
            plk = np.array(self.lw["line_plucker"], float).reshape(-1, 6).copy()
            plk[el] = self.last["plucker_cand"]
            self.lw.update(line_plucker=plk, pose=self.last["pose_cand"].copy(), ex_cam=self.last["ex_cand"].copy())


def closed_loop(ops, quad, pose, ex, max_iterations=40, function_tolerance=1e-13, radius=1e4, mu=1e-8):
    """Each iteration: reduce, the 72-dim solve, the step, the accept test on the total cost, the radius / mu updates of k_accept
    (quality > 1e-3 accepts; < 0.25 halves the radius, > 0.75 widens it to 3 |step|; mu <- max(1e-8, mu / 5) on accept, radius / 2 on
    reject, mu x 10 on an invalid step). The gradient convention: g = J^T r as the reduce returns it, so the quadratic adds its own
    J^T P0 e. Returns dict(costs, accepted ('a' / 'r' / 'i' per iteration), iterations, pose, ex)."""
    pose, ex = np.array(pose, float), np.array(ex, float)
    trace, costs = "", []
    invalid_run = 0
    red = None
    for it in range(max_iterations):
        if red is None:
            red = ops.reduce(mu)
            cP, P, qg = quad.at(pose, ex)
            cost = float(red["cost"]) + cP
            if not costs:
                costs.append(cost)
            y, v, rest, _ = caller_side(red["H"], red["g"], red["U"], red["bp"], P, qg, mu)
        st = ops.step(y, v, rest, radius)
        if st["invalid"]:
            trace += "i"
            invalid_run += 1
            ops.commit(False)
            if invalid_run >= 5:
                break
            mu *= 10.0
            red = None
            continue
        invalid_run = 0
        cand = float(st["cost_cand"]) + quad.at(st["pose_cand"], st["ex_cand"])[0]
        change = cost - cand
        coef = st["coef"]
        if abs(change) <= function_tolerance * cost:
            ops.commit(False)
            break
        if change / coef[3] > 1e-3:
            trace += "a"
            quality = change / coef[3]
            ops.commit(True)
            pose, ex, cost = np.array(st["pose_cand"], float), np.array(st["ex_cand"], float), cand
            costs.append(cost)
            if quality < 0.25:
                radius *= 0.5
            if quality > 0.75:
                radius = max(radius, 3.0 * coef[2])
            mu = max(1e-8, 2.0 * mu / 10.0)
            red = None
        else:
            trace += "r"
            ops.commit(False)
            radius *= 0.5
            red = None      # (the records are dropped by the commit: reduce again at the same state)
    return dict(costs=costs, trace=trace, iterations=len(trace), pose=pose, ex=ex, cost=costs[-1])


# ---- the cases of tests/test_gpu_line_step.py: those of line_reduce_np plus the NaN-observation and sqrt_info = 0 windows, each at
#      mu = 0 and mu = 1 and at three radii, one per dogleg branch
MUS = (0.0, 1.0)


def case_names():
    return lr.case_names() + ["nan_obs", "sqrt_info_0"]


def build_case(name):
    if name == "nan_obs":
        return lr.nan_case()[0], dict(lr.REF)
    if name == "sqrt_info_0":
        return lr.build_case("default")[0], dict(lr.REF, sqrt_info=0.0)
    return lr.build_case(name)


def prepare(name, lw, red, rec, mu, sqrt_info, width):
    """The caller's side of a case from the reduce's outputs (FP64, the device's own in the GPU test): y_p, v_p, rest, the three radii
    and (P, q). P is seeded by the case's place in case_names() and scaled to the lines' pose block. The gradient is DESIGNED, not
    drawn: with Jacobi scaling and mu = 1 a random gradient leaves the damped Gauss-Newton step shorter than the Cauchy step, and then no
    radius reaches the dogleg branch. So bp + q = f D_p (e_top + e_bottom), the eigenvectors of the largest and the smallest eigenvalue of
    the Jacobi-scaled reduced matrix D_p^-1 (H + P) D_p^-1 (Cauchy step <= 2.83 f / lambda_top, Gauss-Newton step >= f / (1 + lambda_bottom)),
    with f = 100 max(1, |lines' gradient|) so that the lines' own gradient does not undo it. All of it from this checker alone."""
    H, g, U, bp = (np.asarray(red[k], float) for k in ("H", "g", "U", "bp"))
    dg = np.diag(U)
    scale = float(np.median(dg[dg > 0])) if (dg > 0).any() else 1e3
    P = rest_of_window(1000 + case_names().index(name), scale)[0]
    Dp = np.sqrt(np.clip(np.diag(U + P), 1e-6, 1e32))
    Hs = (H + P) / np.outer(Dp, Dp)
    E = np.linalg.eigh((Hs + Hs.T) / 2)[1]
    z72 = np.zeros(D)
    f = 100.0 * max(1.0, float(np.sqrt(step(lw, rec, z72, z72, np.zeros(8), 1.0, sqrt_info, width)["gram"][0])))
    q = f * Dp * (E[:, -1] + E[:, 0]) - bp
    x2 = float((np.asarray(lw["pose"], float) ** 2).sum() + (np.asarray(lw["ex_cam"], float) ** 2).sum())
    y, v, rest, _ = caller_side(H, g, U, bp, P, q, mu, x2)
    T = step(lw, rec, y, v, rest, 1.0, sqrt_info, width)["total"]
    return y, v, rest, radii_for(T), (P, q)
