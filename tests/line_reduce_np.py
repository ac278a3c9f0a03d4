"""TEST INFRASTRUCTURE. The numpy checker of gfbe_line_reduce / gfbe_ltab_reduce (csrc/gfbe_line_reduce.hip): the line loops of
optimizationwithLine() (estimator.cpp:4566-4598 solve, :4736-4771 MARGIN_OLD) linearised with respect to the poses, the camera extrinsic
and the lines, and the 4 x 4 line blocks eliminated. Written from the reference's formulas as tests/line_np.py states them (the factor's
Jacobians chained as full 6 x 6 transforms), but in the dtype the caller asks for, so that the same code is the FP64 restatement and the
numpy.longdouble reference; tests/test_line_reduce_host.py pins it against line_np.factor and central differences.

    U = sum Jp^T Jp, bp = sum Jp^T r;  per line V = sum Jl^T Jl, bl = sum Jl^T r, W = sum Jp^T Jl
    V' = V + mu diag(clamp(diag V, 1e-6, 1e32));  H = U - sum_l W V'^-1 W^T;  g = bp - sum_l W V'^-1 bl

on the 72 dims [pose 0 .. pose 10 (dp, dtheta) | ex_cam (dp, dtheta)], r and J after ceres::HuberLoss(width) and its corrector (rho'' <= 0:
both scaled by sqrt(rho')). A line whose V' has no Cholesky factor (a pivot not positive and finite) is left out of every sum.

Beside every array X the checker returns A_X, the scale of its rounding error:
  U, bp, V, bl, W, cost   the entry's absolute sum (sum over the observations of |J_a J_b| per residual row; cost: the sum itself)
  Vinv                    kappa_l |Vinv| A_V' |Vinv|         (first-order effect of the entries of V' on its inverse)
  H                       A_U + sum_l kappa_l A_W |Vinv| A_W^T
  g                       A_bp + sum_l kappa_l A_W |Vinv| A_bl
with kappa_l = |C|_inf |C^-1|_inf, C = D V' D, D = diag(V')^-1/2 (the Jacobi-scaled block), computed in the checker's dtype.

The cases of tests/test_gpu_line_reduce.py and the bound K live here so that the CPU suite can measure K and confirm that no case holds
a line that fails by rounding (test_line_reduce_host.py).

K. Measured on the CPU: this checker in plain FP64 against itself in numpy.longdouble over every case and both modes, worst
|X_64 - X_ld| / (u A_X) per array (R_CPU below; test_line_reduce_host.py asserts that they do not drift upwards). K = max(
normal_equations_np.K, 4 R_CPU[array]) rounded up to a power of two, per array; the factor 4 is for the device's other summation order (tiles,
chunks, frame sums) and nothing else.
"""
import numpy as np

import line_np as ln

LD = np.longdouble
UNIT = 2.0 ** -53
NP_DIM, NFRAMES, WINDOW_SIZE = 72, 11, 10
SOLVE, MARG_OLD = 0, 1
# worst FP64-vs-longdouble ratios of this checker per array over all cases and both modes (measured, see the module docstring)
R_CPU = dict(H=104.0, g=10.3, U=2533.0, bp=3257.0, cost=943.0, Vinv=44.4, bl=6846.0, W=93496.0)
# (Why a plain FP64 evaluation is thousands of u A off in W, bl, U, bp: the residual is a difference of terms 400 x the scene's size that
#  cancel to the pixel noise, and the Jacobians inherit the rounding of the line's trigonometric parameters — errors of the FACTORS, which
#  the absolute sums of their products do not see. H, g, Vinv are small because kappa, 1e7 .. 1e9 at mu = 0, is in their allowance.)
K_NORMAL_EQUATIONS = 1024.0          # normal_equations_np.K (that module needs the CPU oracle; the figure is repeated here)
K = {k: max(K_NORMAL_EQUATIONS, float(2 ** int(np.ceil(np.log2(4 * r))))) for k, r in R_CPU.items()}


def _skew(v):
    z = np.zeros(v.shape[:-1], v.dtype)
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def _quat_R(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def _mv(M, v):
    return (M * v[..., None, :]).sum(-1)


def _theta_R(th):
    s1, c1, s2, c2, s3, c3 = np.sin(th[..., 0]), np.cos(th[..., 0]), np.sin(th[..., 1]), np.cos(th[..., 1]), np.sin(th[..., 2]), np.cos(th[..., 2])
    return np.stack([np.stack([c2 * c3, s1 * s2 * c3 - c1 * s3, c1 * s2 * c3 + s1 * s3], -1),
                     np.stack([c2 * s3, s1 * s2 * s3 + c1 * c3, c1 * s2 * s3 - s1 * c3], -1),
                     np.stack([-s2, s1 * c2, c1 * c2], -1)], -2)


def orth_to_plk(o):
    R = _theta_R(o[..., :3])
    return np.concatenate([np.cos(o[..., 3:4]) * R[..., :, 0], np.sin(o[..., 3:4]) * R[..., :, 1]], -1)


def plk_to_orth(p):
    n, v = p[..., :3], p[..., 3:]
    nn, vn = np.sqrt((n * n).sum(-1)), np.sqrt((v * v).sum(-1))
    u1, u2 = n / nn[..., None], v / vn[..., None]
    u3 = np.cross(u1, u2)
    return np.stack([np.arctan2(u2[..., 2], u3[..., 2]), np.arcsin(-u1[..., 2]), np.arctan2(u1[..., 1], u1[..., 0]),
                     np.arcsin(vn / np.sqrt(nn * nn + vn * vn))], -1)


def plk_to_pose(p, R, t):
    Rv = _mv(R, p[..., 3:])
    return np.concatenate([_mv(R, p[..., :3]) + np.cross(t, Rv), Rv], -1)


def plk_from_pose(p, R, t):
    Rt = np.swapaxes(R, -1, -2)
    return plk_to_pose(p, Rt, -_mv(Rt, t))


def factor(pose, ex, orth, obs, sqrt_info=400.0, jac=True, dtype=np.float64):
    """lineProjectionFactor over m observations in `dtype` (line_projection_factor.cpp:18-231): r [m][2], Jp, Je [m][2][6], Jo [m][2][4]."""
    pose, orth, obs = (np.atleast_2d(np.asarray(a, dtype)) for a in (pose, orth, obs))
    ex, si = np.asarray(ex, dtype).reshape(7), dtype(sqrt_info)
    m = len(pose)
    Rwb, twb = _quat_R(pose[:, 3:]), pose[:, :3]
    Rbc, tbc = np.broadcast_to(_quat_R(ex[3:]), (m, 3, 3)), np.broadcast_to(ex[:3], (m, 3))
    lw = orth_to_plk(orth)
    lb = plk_from_pose(lw, Rwb, twb)
    lc = plk_from_pose(lb, Rbc, tbc)
    nc = lc[:, :3]
    l2 = nc[:, 0] ** 2 + nc[:, 1] ** 2
    ls, lt = np.sqrt(l2), l2 * np.sqrt(l2)
    e1 = obs[:, 0] * nc[:, 0] + obs[:, 1] * nc[:, 1] + nc[:, 2]
    e2 = obs[:, 2] * nc[:, 0] + obs[:, 3] * nc[:, 1] + nc[:, 2]
    r = si * np.stack([e1 / ls, e2 / ls], -1)
    if not jac:
        return r
    jel = si * np.stack([np.stack([obs[:, 0] / ls - nc[:, 0] * e1 / lt, obs[:, 1] / ls - nc[:, 1] * e1 / lt, 1 / ls], -1),
                         np.stack([obs[:, 2] / ls - nc[:, 0] * e2 / lt, obs[:, 3] / ls - nc[:, 1] * e2 / lt, 1 / ls], -1)], -2)
    jeLc = np.concatenate([jel, np.zeros((m, 2, 3), dtype)], -1)
    RbcT, RwbT = np.swapaxes(Rbc, -1, -2), np.swapaxes(Rwb, -1, -2)
    invTbc = np.zeros((m, 6, 6), dtype)
    invTbc[:, :3, :3] = RbcT; invTbc[:, :3, 3:] = -(RbcT @ _skew(tbc)); invTbc[:, 3:, 3:] = RbcT
    nw, dw = lw[:, :3], lw[:, 3:]
    jLp = np.zeros((m, 6, 6), dtype)
    jLp[:, :3, :3] = RwbT @ _skew(dw)
    jLp[:, :3, 3:] = _skew(_mv(RwbT, nw + _mv(_skew(dw), twb)))
    jLp[:, 3:, 3:] = _skew(_mv(RwbT, dw))
    Jp = jeLc @ invTbc @ jLp
    nb, db = lb[:, :3], lb[:, 3:]
    jLe = np.zeros((m, 6, 6), dtype)
    jLe[:, :3, :3] = RbcT @ _skew(db)
    jLe[:, :3, 3:] = _skew(_mv(RbcT, nb + _mv(_skew(db), tbc)))
    jLe[:, 3:, 3:] = _skew(_mv(RbcT, db))
    Je = jeLc @ jLe
    Rwc, twc = Rwb @ Rbc, _mv(Rwb, tbc) + twb
    RwcT = np.swapaxes(Rwc, -1, -2)
    invTwc = np.zeros((m, 6, 6), dtype)
    invTwc[:, :3, :3] = RwcT; invTwc[:, :3, 3:] = -(RwcT @ _skew(twc)); invTwc[:, 3:, 3:] = RwcT
    nn, vn = np.sqrt((nw * nw).sum(-1)), np.sqrt((dw * dw).sum(-1))
    u1, u2 = nw / nn[:, None], dw / vn[:, None]
    u3 = np.cross(u1, u2)
    wn = np.sqrt(nn * nn + vn * vn)
    w0, w1 = nn / wn, vn / wn
    jLo = np.zeros((m, 6, 4), dtype)
    jLo[:, 3:, 0] = w1[:, None] * u3
    jLo[:, :3, 1] = -w0[:, None] * u3
    jLo[:, :3, 2] = w0[:, None] * u2
    jLo[:, 3:, 2] = -w1[:, None] * u1
    jLo[:, :3, 3] = -w1[:, None] * u1
    jLo[:, 3:, 3] = w0[:, None] * u2
    Jo = jeLc @ invTwc @ jLo
    return r, Jp, Je, Jo


def huber(s, a=1.0):
    """ceres::HuberLoss(a): (1/2 rho(s), sqrt(rho'(s))); a <= 0: no loss. s > a^2: rho = 2 a sqrt(s) - a^2, rho' = a / sqrt(s)."""
    s = np.asarray(s)
    if not a > 0:
        return 0.5 * s, np.ones_like(s)
    a = s.dtype.type(a)
    out = s > a * a
    rt = np.sqrt(np.where(out, s, 1))
    return np.where(out, 0.5 * (2 * a * rt - a * a), 0.5 * s), np.where(out, np.sqrt(a / rt), np.ones_like(s))


def eval_huber(pose, ex, orth, obs, sqrt_info=400.0, width=1.0, dtype=np.float64):
    """The corrected factor: r, Jp, Je, Jo scaled by sqrt(rho'), and 1/2 rho per observation."""
    r, Jp, Je, Jo = factor(pose, ex, orth, obs, sqrt_info, True, dtype)
    c, sr = huber((r * r).sum(-1), width)
    return r * sr[:, None], Jp * sr[:, None, None], Je * sr[:, None, None], Jo * sr[:, None, None], c


def chol_inv4(A):
    """(inverse, ok) of a 4 x 4 block through its Cholesky factor in A's dtype; ok False: a pivot that is not positive and finite."""
    dt = A.dtype.type
    L = np.zeros((4, 4), A.dtype)
    for j in range(4):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not (d > 0 and np.isfinite(d)):
            return None, False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 4):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    M = np.zeros((4, 4), A.dtype)
    for j in range(4):
        M[j, j] = dt(1) / L[j, j]
        for i in range(j + 1, 4):
            M[i, j] = -(L[i, j:i] * M[j:i, j]).sum() / L[i, i]
    return M.T @ M, True


def entering(lw, mode):
    e = ln.eligible(lw)
    return e & (np.asarray(lw["start_frame"]) == 0) if mode == MARG_OLD else e


def reduce(lw, mode=SOLVE, sqrt_info=400.0, width=1.0, mu=0.0, dtype=np.float64):
    """One window. dict: H, g, U, bp, cost, n_eligible, n_failed; per entering line (list order) Vinv, Vp (V'), bl, W, failed, kappa;
    and the scales A_H, A_g, A_U, A_bp, A_cost, A_Vinv, A_bl, A_W."""
    dt = np.dtype(dtype).type
    sf, no = np.asarray(lw["start_frame"]), np.asarray(lw["n_obs"])
    obs = np.asarray(lw["obs"], dtype).reshape(-1, 4)
    off = np.concatenate([[0], np.cumsum(no)]).astype(int)
    pose, ex = np.asarray(lw["pose"], dtype).reshape(NFRAMES, 7), np.asarray(lw["ex_cam"], dtype)
    Rs, Rbc = _quat_R(pose[:, 3:]), _quat_R(ex[3:])
    Rwc, twc = Rs @ Rbc, pose[:, :3] + _mv(Rs, np.broadcast_to(ex[:3], (NFRAMES, 3)))
    el = np.flatnonzero(entering(lw, mode))
    n = len(el)
    k0 = 1 if mode == MARG_OLD else 0
    D = NP_DIM
    out = dict(n_eligible=n, Vinv=np.zeros((n, 4, 4), dtype), Vp=np.zeros((n, 4, 4), dtype), bl=np.zeros((n, 4), dtype),
               W=np.zeros((n, D, 4), dtype), failed=np.zeros(n, np.uint8), kappa=np.ones(n, dtype),
               A_Vinv=np.zeros((n, 4, 4), dtype), A_bl=np.zeros((n, 4), dtype), A_W=np.zeros((n, D, 4), dtype))
    U, bp, A_U, A_bp = np.zeros((D, D), dtype), np.zeros(D, dtype), np.zeros((D, D), dtype), np.zeros(D, dtype)
    S, sg, A_S, A_sg = np.zeros((D, D), dtype), np.zeros(D, dtype), np.zeros((D, D), dtype), np.zeros(D, dtype)
    cost = dt(0)
    plk = np.asarray(lw["line_plucker"], dtype).reshape(-1, 6)
    for q, l in enumerate(el):
        s, m = int(sf[l]), int(no[l])
        x = plk_to_orth(plk_to_pose(plk[l], Rwc[s], twc[s]))         # getLineOrthVector
        fr = np.arange(s + k0, s + m)
        r, Jp, Je, Jo, c = eval_huber(pose[fr], ex, np.broadcast_to(x, (len(fr), 4)), obs[off[l] + k0:off[l] + m], sqrt_info, width, dtype)
        # the 72 columns of every observation's Jacobian
        J = np.zeros((len(fr), 2, D), dtype)
        for k, f in enumerate(fr):
            J[k, :, 6 * f:6 * f + 6] = Jp[k]
        J[:, :, 66:] = Je
        aJ, aJo, ar = np.abs(J), np.abs(Jo), np.abs(r)
        V, A_V = np.einsum("kia,kib->ab", Jo, Jo), np.einsum("kia,kib->ab", aJo, aJo)
        dg = np.clip(np.diag(V), dt(1e-6), dt(1e32))
        Vp, A_Vp = V + dt(mu) * np.diag(dg), A_V + dt(mu) * np.diag(dg)
        Vinv, ok = chol_inv4(Vp)
        if not ok:
            out["failed"][q] = 1
            continue
        sc = 1 / np.sqrt(np.diag(Vp))
        C = Vp * sc[:, None] * sc[None, :]
        Cinv = chol_inv4(C)[0]
        kappa = np.abs(C).sum(1).max() * np.abs(Cinv).sum(1).max()
        W, A_W = np.einsum("kip,kia->pa", J, Jo), np.einsum("kip,kia->pa", aJ, aJo)
        bl, A_bl = np.einsum("kia,ki->a", Jo, r), np.einsum("kia,ki->a", aJo, ar)
        U += np.einsum("kip,kiq->pq", J, J); A_U += np.einsum("kip,kiq->pq", aJ, aJ)
        bp += np.einsum("kip,ki->p", J, r); A_bp += np.einsum("kip,ki->p", aJ, ar)
        cost += c.sum()
        aV = np.abs(Vinv)
        S += W @ Vinv @ W.T; A_S += kappa * (A_W @ aV @ A_W.T)
        sg += W @ Vinv @ bl; A_sg += kappa * (A_W @ aV @ A_bl)
        out["Vinv"][q], out["Vp"][q], out["bl"][q], out["W"][q], out["kappa"][q] = Vinv, Vp, bl, W, kappa
        out["A_Vinv"][q], out["A_bl"][q], out["A_W"][q] = kappa * (aV @ A_Vp @ aV), A_bl, A_W
    out.update(H=U - S, g=bp - sg, U=U, bp=bp, cost=cost, A_H=A_U + A_S, A_g=A_bp + A_sg, A_U=A_U, A_bp=A_bp, A_cost=cost,
               n_failed=int(out["failed"].sum()))
    return out


ARRAYS = ("H", "g", "U", "bp", "cost", "Vinv", "bl", "W")


def ratios(got, ref):
    """Per array: (worst |got - ref| / (u A), entries that are non-zero where A is zero)."""
    res = {}
    keep = ref["failed"] == 0
    for k in ARRAYS:
        x, y, a = np.asarray(got[k], LD), np.asarray(ref[k], LD), np.asarray(ref["A_" + k], LD)
        if k in ("Vinv", "bl", "W"):
            x, y, a = x[keep], y[keep], a[keep]
        nz = a > 0
        worst = float((np.abs(x - y)[nz] / (UNIT * a[nz])).max()) if nz.any() else 0.0
        res[k] = (worst, int((x[~nz] != 0).sum()))
    return res


# ---- the cases of tests/test_gpu_line_reduce.py: name -> (line window, dict(sqrt_info, width, mu))
def _window(seed, n_ok, **kw):
    z = dict(n_short=0, n_late=0, n_untri=0, n_behind=0, n_long=0, n_outlier=0)
    z.update(kw)
    from _gfbe_import import gf
    return gf.synth_line.line_window(seed=seed, n_ok=n_ok, **z)


def _with_obs_count(lw, k):
    """Every line keeps exactly k observations (k = 11: the line starts in frame 0 and is re-observed in every frame)."""
    from _gfbe_import import gf
    n = len(lw["n_obs"])
    if k == 11:
        base = gf.synth_line.line_window(seed=4242, n_ok=800, n_short=0, n_late=0, n_untri=0, n_behind=0, n_long=0, n_outlier=0)
        pick = np.flatnonzero((base["start_frame"] == 0) & (base["n_obs"] == 11))[:n]
        assert len(pick) >= 8
        return _take(base, pick)
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])]).astype(int)
    obs = np.concatenate([lw["obs"][off[i]:off[i] + k] for i in range(n)])
    out = dict(lw)
    out.update(n_obs=np.full(n, k, np.int32), obs=obs)
    return out


def _take(lw, idx):
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])]).astype(int)
    out = dict(lw)
    out.update(start_frame=lw["start_frame"][idx], n_obs=lw["n_obs"][idx], is_triangulation=lw["is_triangulation"][idx],
               line_plucker=lw["line_plucker"][idx], true_plucker=lw["true_plucker"][idx], kind=lw["kind"][idx],
               obs=np.concatenate([lw["obs"][off[i]:off[i + 1]] for i in idx]) if len(idx) else np.zeros((0, 4)))
    return out


REF = dict(sqrt_info=400.0, width=1.0, mu=0.0)


def case_names():
    return ["default", "no_eligible", "one_line", "lines_257", "lines_600", "obs_5", "obs_11", "all_start_0", "none_start_0",
            "huber_active", "mu_1e-4", "mu_1", "huber_off", "huber_inactive", "marg_300"]


def build_case(name):
    from _gfbe_import import gf
    par = dict(REF)
    if name == "default":
        lw = gf.synth_line.line_window(seed=21)
    elif name == "no_eligible":
        lw = gf.synth_line.line_window(seed=22, n_ok=0, n_short=5, n_late=4, n_untri=3, n_behind=0, n_long=0, n_outlier=0)
    elif name == "one_line":
        lw = gf.synth_line.line_window(seed=23, n_ok=1, n_short=3, n_late=2, n_untri=2, n_behind=0, n_long=0, n_outlier=0)
    elif name == "lines_257":
        lw = _window(24, 257)
    elif name == "lines_600":
        lw = _window(25, 600, n_short=20, n_late=20)
    elif name == "obs_5":
        lw = _with_obs_count(_window(26, 40), 5)
    elif name == "obs_11":
        lw = _with_obs_count(_window(27, 24), 11)
    elif name == "all_start_0":
        w = _window(28, 200)
        lw = _take(w, np.flatnonzero(w["start_frame"] == 0))
    elif name == "none_start_0":
        w = _window(29, 80)
        lw = _take(w, np.flatnonzero(w["start_frame"] != 0))
    elif name == "huber_active":
        lw = _window(30, 60)
        rng = np.random.default_rng(30)
        hit = rng.random(len(lw["obs"])) < 0.1
        lw["obs"] = lw["obs"] + hit[:, None] * rng.normal(0, 0.02, lw["obs"].shape)
    elif name in ("mu_1e-4", "mu_1"):
        lw = _window(31, 50)
        par["mu"] = 1e-4 if name == "mu_1e-4" else 1.0
    elif name == "huber_off":
        lw = _window(32, 50)
        par["width"] = 0.0
    elif name == "huber_inactive":
        # the unrefined lines of these windows leave ~90 % of the residuals OUTSIDE the width at sqrt_info = 400 (so every other case
        # runs mostly on the loss's outer branch, and huber_active only adds larger ones); here sqrt_info = 4 puts them inside
        lw = _window(34, 60)
        par["sqrt_info"] = 4.0
    elif name == "marg_300":
        # more than 256 lines that start in frame 0: MARG_OLD mode with more than one line per thread
        w = _window(35, 2300)
        lw = _take(w, np.flatnonzero(w["start_frame"] == 0))
        assert len(lw["n_obs"]) > 256
    else:
        raise KeyError(name)
    return lw, par


def nan_case():
    """(window with one line made un-eliminable by a NaN observation, the same window without that line, index among the entering lines)."""
    lw = _window(33, 30)
    el = np.flatnonzero(ln.eligible(lw) & (lw["start_frame"] == 0))      # (a line that enters in both modes)
    victim = int(el[len(el) // 2])
    off = np.concatenate([[0], np.cumsum(lw["n_obs"])]).astype(int)
    bad = dict(lw)
    bad["obs"] = lw["obs"].copy()
    bad["obs"][off[victim] + 2, 1] = np.nan
    without = _take(lw, np.array([i for i in range(len(lw["n_obs"])) if i != victim]))
    return bad, without, victim
