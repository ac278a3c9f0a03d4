"""TEST MODEL. The loop-closure pose graph of dense_map (PoseGraph::optimize4DoF, dense_map/src/pose_graph.cpp:529-705; factors
pose_graph.h:129-288) restated in numpy for a dtype argument (float64 / longdouble): the two 4-DoF factors with analytic tangent
Jacobians, the Huber corrector, and Ceres 1.14's Levenberg-Marquardt loop (Jacobi scaling, the statements and order of the f3
restatement). Two solve paths over ONE linearisation:

  dense — the normal equations assembled densely, an unblocked Cholesky (small graphs only);
  band  — the device's structure phase for phase (ground-fusion2_amd/csrc/gfbe_loopgraph.hip): four poses form a 16 x 16 super-block,
          the sequence edges give a block-tridiagonal T, a loop edge four sparse columns of U, H = T + U U^T; parallel block cyclic
          reduction over the super-blocks with the right-hand-side panel [-g | U] (every sweep: alpha = -A B^-1 of the neighbour at the
          stride, the blocks' inverses by Gauss-Jordan, symmetrised), then the capacitance system S = I + U^T Z by a block LDL^T in
          16-wide tiles and y = z_0 - Z S^-1 U^T z_0.

A pose is out of the problem when it is fixed or touches no edge with a free pose: zero columns, identity diagonal, zero gradient, no
part in the scaling, the norms or the step. An edge between two fixed poses is dropped (Ceres removes the residual block)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
MAX_LOOPS = 64
SB = 16


def options(**kw):
    o = dict(huber_delta=0.1, max_num_iterations=5, span=4, loop_yaw_div=10.0)
    o.update(kw)
    return o


def _pi(dt):
    return dt(4) * np.arctan(dt(1))


def normalize_angle(a):
    return np.where(a > 180, a - 360, np.where(a < -180, a + 360, a))


def ypr_to_R(yaw, pitch, roll, dt):
    """[E, 9]: YawPitchRollToRotationMatrix, and the same sums with every term's magnitude (for the bounds)."""
    y, p, r = yaw / dt(180) * _pi(dt), pitch / dt(180) * _pi(dt), roll / dt(180) * _pi(dt)
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    R = np.stack([cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr, sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr,
                  -sp, cp * sr, cp * cr], axis=-1)
    a = np.abs
    Rabs = np.stack([a(cy * cp), a(sy * cr) + a(cy * sp * sr), a(sy * sr) + a(cy * sp * cr), a(sy * cp), a(cy * cr) + a(sy * sp * sr),
                     a(cy * sr) + a(sy * sp * cr), a(sp), a(cp * sr), a(cp * cr)], axis=-1)
    ang = a(y) + a(p) + a(r)
    return R, Rabs + 2 * ang[..., None], ang      # (a factor cos / sin carries its argument's rounding, u |angle|, whatever its own size)


def factor(yaw_i, ti, yaw_j, tj, meas, yaw_w, dt):
    """Vectorised over edges: r [E, 4], J [E, 4, 8] (columns yaw_i t_i yaw_j t_j), and the absolute sums A_r, A_J behind them.
    yaw_w [E]: 1 (FourDOFError) or 1 / loop_yaw_div (FourDOFWeightError). wrap [E]: distance of the yaw difference from +-180."""
    yaw_i, yaw_j, ti, tj, meas, yaw_w = (np.asarray(v, dt) for v in (yaw_i, yaw_j, ti, tj, meas, yaw_w))
    E = len(yaw_i)
    R, Rabs, _ = ypr_to_R(yaw_i, meas[:, 4], meas[:, 5], dt)
    d = tj - ti
    dabs = np.abs(tj) + np.abs(ti)
    r, J = np.zeros((E, 4), dt), np.zeros((E, 4, 8), dt)
    Ar, AJ = np.zeros((E, 4)), np.zeros((E, 4, 8))
    for a in range(3):
        r[:, a] = (R[:, a] * d[:, 0] + R[:, 3 + a] * d[:, 1] + R[:, 6 + a] * d[:, 2]) - meas[:, a]
        Ar[:, a] = ((Rabs[:, a] * dabs[:, 0] + Rabs[:, 3 + a] * dabs[:, 1] + Rabs[:, 6 + a] * dabs[:, 2]).astype(np.float64)
                    + np.abs(meas[:, a]).astype(np.float64))
        J[:, a, 0] = (R[:, a] * d[:, 1] - R[:, 3 + a] * d[:, 0]) * (_pi(dt) / dt(180))
        AJ[:, a, 0] = (Rabs[:, a] * dabs[:, 1] + Rabs[:, 3 + a] * dabs[:, 0]).astype(np.float64) * float(np.pi / 180)
        for b in range(3):
            J[:, a, 1 + b] = -R[:, 3 * b + a]
            J[:, a, 5 + b] = R[:, 3 * b + a]
            AJ[:, a, 1 + b] = AJ[:, a, 5 + b] = Rabs[:, 3 * b + a].astype(np.float64)
    e = yaw_j - yaw_i - meas[:, 3]
    r[:, 3] = normalize_angle(e) * yaw_w
    Ar[:, 3] = ((np.abs(yaw_j) + np.abs(yaw_i) + np.abs(meas[:, 3])) * yaw_w).astype(np.float64)
    J[:, 3, 0], J[:, 3, 4] = -yaw_w, yaw_w
    AJ[:, 3, 0] = AJ[:, 3, 4] = yaw_w.astype(np.float64)
    wrap = np.abs(np.abs(e) - 180).astype(np.float64)
    return r, J, Ar, AJ, wrap


def huber_corrector(sq, delta, dt):
    """ceres::HuberLoss + Corrector for one residual block: (rho / 2, sqrt(rho'), residual scale, alpha / sq)."""
    b = dt(delta) * dt(delta)
    if sq > b:
        rr = np.sqrt(sq)
        rho0, rho1 = 2 * dt(delta) * rr - b, max(dt(1e-300), dt(delta) / rr)
        rho2 = -rho1 / (2 * sq)
    else:
        rho0, rho1, rho2 = sq, dt(1), dt(0)
    s = np.sqrt(rho1)
    if sq == 0 or rho2 <= 0:
        return rho0 / 2, s, s, dt(0)
    D = 1 + 2 * sq * rho2 / rho1
    alpha = 1 - np.sqrt(D)
    return rho0 / 2, s, s / (1 - alpha), alpha / sq


def eval_edges(yaw, t, edge_i, edge_j, kind, meas, opt, dt):
    """What gfbe_lc4_eval returns: r [E, 4], J [E, 4, 8], cost with the loss; and the absolute sums A_r, A_J, A_cost, the smallest
    distance of a yaw difference from the wrap and of a kind-1 block's squared norm from the Huber threshold (relative)."""
    yaw, t, meas = np.asarray(yaw, dt), np.asarray(t, dt).reshape(-1, 3), np.asarray(meas, dt).reshape(-1, 6)
    ei, ej, kind = np.asarray(edge_i, np.int64), np.asarray(edge_j, np.int64), np.asarray(kind, np.int64)
    yw = np.where(kind == 1, dt(1) / dt(opt["loop_yaw_div"]), dt(1)).astype(dt)
    if len(ei) == 0:
        return dict(r=np.zeros((0, 4), dt), J=np.zeros((0, 4, 8), dt), cost=dt(0), A_r=np.zeros((0, 4)), A_J=np.zeros((0, 4, 8)), A_cost=0.0,
                    cost_e=np.zeros(0, dt), wrap=np.inf, huber=np.inf)
    r, J, Ar, AJ, wrap = factor(yaw[ei], t[ei], yaw[ej], t[ej], meas, yw, dt)
    cost_e, A_cost, hub = np.zeros(len(ei), dt), 0.0, np.inf
    sq_all = (r * r).sum(axis=1)
    A_sq_all = 2 * (np.abs(r).astype(np.float64) * Ar).sum(axis=1) + sq_all.astype(np.float64)
    cost_e[:] = sq_all / 2
    A_cost = float(A_sq_all[kind == 0].sum() / 2)
    for e in np.nonzero(kind == 1)[0]:
        sq, A_sq = sq_all[e], float(A_sq_all[e])
        b = float(opt["huber_delta"]) ** 2
        hub = min(hub, abs(float(sq) - b) / max(A_sq, 1e-300))
        c, s1, rs, asn = huber_corrector(sq, opt["huber_delta"], dt)
        rel = A_sq / float(sq) if sq > b else 0.0      # (the scale sqrt(delta / |r|) inherits the relative bound of |r|^2)
        rj = r[e] @ J[e]
        AJ[e] = float(s1) * (AJ[e] + np.abs(J[e]).astype(np.float64) * rel)
        Ar[e] = float(rs) * (Ar[e] + np.abs(r[e]).astype(np.float64) * rel)
        J[e] = s1 * (J[e] - asn * np.outer(r[e], rj))
        r[e] = rs * r[e]
        cost_e[e] = c
        A_cost += A_sq * float(s1) ** 2 / 2 + float(c)
    cost = cost_e.sum()
    return dict(r=r, J=J, cost=cost, cost_e=cost_e, A_r=Ar, A_J=AJ, A_cost=A_cost + float(cost), wrap=float(wrap.min()), huber=hub)


def sequence_meas(ta, ypr_a, tb, ypr_b, dt):
    R, _, _ = ypr_to_R(np.asarray([ypr_a[0]], dt), np.asarray([ypr_a[1]], dt), np.asarray([ypr_a[2]], dt), dt)
    R = R[0]
    d = np.asarray(tb, dt) - np.asarray(ta, dt)
    m = [R[a] * d[0] + R[3 + a] * d[1] + R[6 + a] * d[2] for a in range(3)]
    return np.array(m + [dt(ypr_b[0]) - dt(ypr_a[0]), dt(ypr_a[1]), dt(ypr_a[2])], dt)


def plan(n, n_loop):
    """The plan of gfbe_loopgraph.h (lc4_plan) without the scratch offsets."""
    M = (n + 3) // 4
    sweeps = 0
    while (1 << sweeps) < M:
        sweeps += 1
    ncol = 1 + 4 * n_loop
    ntile = (ncol + SB - 1) // SB
    cap = 4 * n_loop
    return dict(M=M, rows=SB * M, pad_poses=4 * M - n, sweeps=sweeps, ncol=ncol, ntile=ntile, ld=SB * ntile, cap=cap,
                cap_ld=SB * ((cap + SB - 1) // SB) if cap else SB)


def build_graph(t, ypr, sequence, fixed, loop_i, loop_c, loop_meas, opt, dt=np.float64):
    """The edge list of optimize4DoF: sequence edges (i - k, i), k = 1 .. span, between poses of one sequence, their measurements formed
    from the input poses IN FP64 (they are data of the problem: both precisions solve the same graph), then the loop edges (c, i).
    Edges with two fixed ends are dropped; free[i] = not fixed and on a kept edge."""
    del dt
    t, ypr = np.asarray(t, np.float64).reshape(-1, 3), np.asarray(ypr, np.float64).reshape(-1, 3)
    n = len(t)
    fixed = np.asarray(fixed).astype(bool)
    ei, ej, kind, meas = [], [], [], []
    for i in range(n):
        for k in range(1, opt["span"] + 1):
            if i - k >= 0 and sequence[i] == sequence[i - k] and not (fixed[i] and fixed[i - k]):
                ei.append(i - k); ej.append(i); kind.append(0)
                meas.append(sequence_meas(t[i - k], ypr[i - k], t[i], ypr[i], np.float64))
    n_seq = len(ei)
    lm = np.asarray(loop_meas, np.float64).reshape(-1, 4)
    loop_on = []
    for l in range(len(loop_i)):
        c, i = int(loop_c[l]), int(loop_i[l])
        on = not (fixed[c] and fixed[i])
        loop_on.append(on)
        if on:
            ei.append(c); ej.append(i); kind.append(1)
            meas.append(np.array([lm[l, 0], lm[l, 1], lm[l, 2], lm[l, 3], ypr[c, 1], ypr[c, 2]]))
    free = np.zeros(n, bool)
    for a, b in zip(ei, ej):
        free[a] = free[b] = True
    free &= ~fixed
    return dict(n=n, edge_i=np.array(ei, np.int64), edge_j=np.array(ej, np.int64), kind=np.array(kind, np.int64),
                meas=np.array(meas, np.float64).reshape(-1, 6), n_seq=n_seq, free=free, loop_on=np.array(loop_on, bool), n_loop=len(loop_i))


def plus(yaw, t, d, dt):
    """AngleLocalParameterization on the yaw (one wrap), identity on t; d [n, 4]."""
    return normalize_angle(yaw + d[:, 0]).astype(dt), t + d[:, 1:]


def linearize(G, yaw, t, opt, dt):
    """cost, and the structure both solve paths share: the band of the sequence part in super-blocks (Hb, Ha = block (m, m - 1),
    Hc = block (m, m + 1)), the sequence gradient, and per loop edge its corrected Jacobian (four columns of U with 8 non-zeros each),
    rows, gradient and diagonal shares. Columns of a pose that is out of the problem are zero."""
    n, P = G["n"], plan(G["n"], 0)
    M = P["M"]
    ev = eval_edges(yaw, t, G["edge_i"], G["edge_j"], G["kind"], G["meas"], opt, dt)
    J, r = ev["J"].copy(), ev["r"]
    free = G["free"]
    for e in range(len(J)):
        if not free[G["edge_i"][e]]:
            J[e, :, 0:4] = 0
        if not free[G["edge_j"][e]]:
            J[e, :, 4:8] = 0
    Hb, Ha, Hc, g = np.zeros((M, SB, SB), dt), np.zeros((M, SB, SB), dt), np.zeros((M, SB, SB), dt), np.zeros(SB * M, dt)

    def add(pi, pj, blk):
        mi, mj, ri, rj = pi // 4, pj // 4, 4 * (pi % 4), 4 * (pj % 4)
        tgt = Hb if mi == mj else (Ha if mi == mj + 1 else Hc)
        assert abs(mi - mj) <= 1
        tgt[mi, ri:ri + 4, rj:rj + 4] += blk
    JtJ, Jtr = np.einsum("eqa,eqb->eab", J, J), np.einsum("eqa,eq->ea", J, r)
    for e in range(G["n_seq"]):
        a, b = int(G["edge_i"][e]), int(G["edge_j"][e])
        add(a, a, JtJ[e, 0:4, 0:4]); add(b, b, JtJ[e, 4:8, 4:8]); add(b, a, JtJ[e, 4:8, 0:4]); add(a, b, JtJ[e, 0:4, 4:8])
        g[4 * a:4 * a + 4] += Jtr[e, 0:4]
        g[4 * b:4 * b + 4] += Jtr[e, 4:8]
    L = len(J) - G["n_seq"]
    Uv, Urow = np.zeros((L, 4, 8), dt), np.zeros((L, 8), np.int64)
    gl, dl = np.zeros((L, 8), dt), np.zeros((L, 8), dt)
    for l in range(L):
        e = G["n_seq"] + l
        a, b = int(G["edge_i"][e]), int(G["edge_j"][e])
        Uv[l] = J[e]
        Urow[l] = list(range(4 * a, 4 * a + 4)) + list(range(4 * b, 4 * b + 4))
        gl[l] = J[e].T @ r[e]
        dl[l] = (J[e] * J[e]).sum(axis=0)
    g0, diag0 = g.copy(), np.array([Hb[m, k, k] for m in range(M) for k in range(SB)], dt)
    for l in range(L):
        for k in range(8):
            g0[Urow[l, k]] += gl[l, k]
            diag0[Urow[l, k]] += dl[l, k]
    active = np.zeros(SB * M, bool)
    active[:4 * n] = np.repeat(free, 4)
    return dict(cost=ev["cost"], A_cost=ev["A_cost"], wrap=ev["wrap"], huber=ev["huber"], Hb=Hb, Ha=Ha, Hc=Hc, Uv=Uv, Urow=Urow, g0=g0, diag0=diag0,
                active=active, M=M, L=L)


# ---- the two solve paths ------------------------------------------------------------------------------------------------------------
def gj_inverse(B, dt):
    """Inverse of a batch of SPD 16 x 16 blocks [M, 16, 16] by Gauss-Jordan without pivoting on [B | I], symmetrised; ok[m] = every
    pivot positive (and finite)."""
    M, k = B.shape[0], B.shape[1]
    W = np.concatenate([B.astype(dt), np.broadcast_to(np.eye(k, dtype=dt), (M, k, k))], axis=2).copy()
    ok = np.ones(M, bool)
    for c in range(k):
        p = W[:, c, c].copy()
        ok &= (p > 0) & np.isfinite(p.astype(np.float64))
        p = np.where(p > 0, p, dt(1))
        rowc = W[:, c, :] / p[:, None]
        f = W[:, :, c].copy()
        W = W - f[:, :, None] * rowc[:, None, :]
        W[:, c, :] = rowc
    X = W[:, :, k:]
    return (X + X.transpose(0, 2, 1)) / 2, ok


def chol_solve_dense(H, b, dt):
    """Unblocked Cholesky; None when a pivot is not positive."""
    n = len(b)
    A = H.astype(dt).copy()
    for c in range(n):
        p = A[c, c]
        if not (p > 0) or not np.isfinite(float(p)):
            return None
        A[c, c] = np.sqrt(p)
        A[c + 1:, c] /= A[c, c]
        A[c + 1:, c + 1:] -= np.outer(A[c + 1:, c], A[c + 1:, c])
    y = b.astype(dt).copy()
    for c in range(n):
        y[c] /= A[c, c]
        y[c + 1:] -= A[c + 1:, c] * y[c]
    for c in range(n - 1, -1, -1):
        y[c] /= A[c, c]
        y[:c] -= A[c, :c] * y[c]
    return y


def band_to_dense(B, A, C):
    M = len(B)
    H = np.zeros((SB * M, SB * M), B.dtype)
    for m in range(M):
        H[SB * m:SB * m + SB, SB * m:SB * m + SB] = B[m]
        if m > 0:
            H[SB * m:SB * m + SB, SB * (m - 1):SB * m] = A[m]
        if m + 1 < M:
            H[SB * m:SB * m + SB, SB * (m + 1):SB * (m + 2)] = C[m]
    return H


def pcr_solve(B, A, C, panel, dt):
    """Parallel block cyclic reduction: ceil(log2 M) sweeps, then Z = B^-1 panel block by block. Returns (Z, ok)."""
    M = len(B)
    Binv, ok = gj_inverse(B, dt)
    good = ok.all()
    s = 1
    while s < M:
        al, ga = np.zeros_like(B), np.zeros_like(B)
        al[s:] = -(A[s:] @ Binv[:-s])
        ga[:-s] = -(C[:-s] @ Binv[s:])
        B2, A2, C2, p2 = B.copy(), np.zeros_like(A), np.zeros_like(C), panel.copy()
        B2[s:] += al[s:] @ C[:-s]
        B2[:-s] += ga[:-s] @ A[s:]
        A2[s:] = al[s:] @ A[:-s]
        C2[:-s] = ga[:-s] @ C[s:]
        p2[s:] += al[s:] @ panel[:-s]
        p2[:-s] += ga[:-s] @ panel[s:]
        B, A, C, panel = B2, A2, C2, p2
        Binv, ok = gj_inverse(B, dt)
        good = good and ok.all()
        s *= 2
    return Binv @ panel, good


def cap_solve(S, v, dt):
    """Block LDL^T of the SPD capacitance matrix in 16-wide tiles (L_IP = S_IP D_P^-1, D_P inverted by gj_inverse), then the solve."""
    nt = len(S) // SB
    S = S.astype(dt).copy()
    Lb, Dinv = np.zeros_like(S), np.zeros((nt, SB, SB), dt)
    T = lambda i, j: (slice(SB * i, SB * i + SB), slice(SB * j, SB * j + SB))
    for P in range(nt):
        di, ok = gj_inverse(S[T(P, P)][None], dt)
        if not ok.all():
            return None
        Dinv[P] = di[0]
        for I in range(P + 1, nt):
            Lb[T(I, P)] = S[T(I, P)] @ Dinv[P]
        for I in range(P + 1, nt):
            for Jt in range(P + 1, I + 1):
                S[T(I, Jt)] = S[T(I, Jt)] - Lb[T(I, P)] @ S[T(Jt, P)].T
    w = v.astype(dt).copy()
    for P in range(nt):
        for I in range(P + 1, nt):
            w[SB * I:SB * I + SB] -= Lb[T(I, P)] @ w[SB * P:SB * P + SB]
    for P in range(nt):
        w[SB * P:SB * P + SB] = Dinv[P] @ w[SB * P:SB * P + SB]
    for P in range(nt - 1, -1, -1):
        for I in range(P + 1, nt):
            w[SB * P:SB * P + SB] -= Lb[T(I, P)].T @ w[SB * I:SB * I + SB]
    return w


def scaled_system(lin, scale, dt):
    """The Jacobi-scaled, unregularised pieces: band (Bs, As, Cs), Us values, gs."""
    M = lin["M"]
    sc = scale.reshape(M, SB)
    Bs = lin["Hb"] * sc[:, :, None] * sc[:, None, :]
    As, Cs = np.zeros_like(Bs), np.zeros_like(Bs)
    As[1:] = lin["Ha"][1:] * sc[1:, :, None] * sc[:-1, None, :]
    Cs[:-1] = lin["Hc"][:-1] * sc[:-1, :, None] * sc[1:, None, :]
    Us = lin["Uv"] * scale[lin["Urow"]][:, None, :] if lin["L"] else lin["Uv"]
    return Bs, As, Cs, Us, scale * lin["g0"]


def lm_step(lin, scale, diag2, radius, dt, path):
    """Solve (S H S + D / radius) y = -S g. Returns (y or None when a pivot was not positive, model cost change)."""
    M, L, act = lin["M"], lin["L"], lin["active"]
    Bs, As, Cs, Us, gs = scaled_system(lin, scale, dt)
    B = Bs.copy()
    lam = diag2 / radius
    for m in range(M):
        for k in range(SB):
            B[m, k, k] = Bs[m, k, k] + lam[SB * m + k] if act[SB * m + k] else dt(1)
    rhs = np.where(act, -gs, dt(0))
    ncol = 1 + 4 * L
    if path == "dense":
        H = band_to_dense(B, As, Cs)
        for l in range(L):
            for q in range(4):
                H[np.ix_(lin["Urow"][l], lin["Urow"][l])] += np.outer(Us[l, q], Us[l, q])
        y = chol_solve_dense(H, rhs, dt)
    else:
        panel = np.zeros((M, SB, ncol), dt)
        panel[:, :, 0] = rhs.reshape(M, SB)
        for l in range(L):
            for q in range(4):
                for k in range(8):
                    row = lin["Urow"][l, k]
                    panel[row // SB, row % SB, 1 + 4 * l + q] = Us[l, q, k]
        Z, ok = pcr_solve(B, As, Cs, panel, dt)
        Z = Z.reshape(SB * M, ncol)
        y = Z[:, 0].copy() if ok else None
        if ok and L:
            P = plan(4, L)
            S, v = np.eye(P["cap_ld"], dtype=dt), np.zeros(P["cap_ld"], dt)
            for l in range(L):
                for q in range(4):
                    a = 4 * l + q
                    for k in range(8):      # fixed order: the column's 8 non-zeros
                        S[a, :4 * L] += Us[l, q, k] * Z[lin["Urow"][l, k], 1:]
                        v[a] += Us[l, q, k] * Z[lin["Urow"][l, k], 0]
            w = cap_solve(S, v, dt)
            if w is None:
                y = None
            else:
                for b in range(4 * L):
                    y = y - Z[:, 1 + b] * w[b]
    if y is None:
        return None, dt(0)
    # model cost change -(gs . y + |J S y|^2 / 2), the unregularised system
    yb = y.reshape(M, SB)
    Ty = np.einsum("mij,mj->mi", Bs, yb)
    Ty[1:] += np.einsum("mij,mj->mi", As[1:], yb[:-1])
    Ty[:-1] += np.einsum("mij,mj->mi", Cs[:-1], yb[1:])
    yHy = (y * Ty.reshape(-1)).sum()
    for l in range(L):
        p = Us[l] @ y[lin["Urow"][l]]
        yHy = yHy + p @ p
    return y, -((gs * y).sum() + yHy / 2)


def kappa_estimate(lin, scale, diag2, radius):
    """lambda_max / lambda_min of the regularised scaled system (the system of the last accepted step) in FP64: its eigenvalues for up to
    1100 rows, 12 power and 12 inverse iterations beyond (estimates from below)."""
    rng = np.random.default_rng(0)
    act = lin["active"]
    fl = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == LD else v) for k, v in lin.items()}
    sc, d2 = scale.astype(np.float64), diag2.astype(np.float64)
    Bs, As, Cs, Us, _ = scaled_system(fl, sc, np.float64)
    M = fl["M"]

    def mv(x):
        xb = x.reshape(M, SB)
        o = np.einsum("mij,mj->mi", Bs, xb)
        o[1:] += np.einsum("mij,mj->mi", As[1:], xb[:-1])
        o[:-1] += np.einsum("mij,mj->mi", Cs[:-1], xb[1:])
        o = o.reshape(-1) + d2 / float(radius) * x
        for l in range(fl["L"]):
            o[fl["Urow"][l]] += Us[l].T @ (Us[l] @ x[fl["Urow"][l]])
        return np.where(act, o, 0.0)
    if not act.any():
        return 1.0
    if len(act) <= 1100:
        idx = np.nonzero(act)[0]
        ev = np.linalg.eigvalsh(np.stack([mv(np.eye(len(act))[k]) for k in idx])[:, idx])
        return float(ev[-1] / ev[0])
    x = np.where(act, rng.normal(size=len(act)), 0.0)
    for _ in range(12):
        x = mv(x / np.linalg.norm(x))
    lmax = np.linalg.norm(x)
    x = np.where(act, rng.normal(size=len(act)), 0.0)
    for _ in range(12):
        x = x / np.linalg.norm(x)
        fl2 = dict(fl, g0=-x / sc)      # lm_step solves ... y = -S g0 = x
        x, _ = lm_step(fl2, sc, d2, np.float64(radius), np.float64, "band")
        if x is None:
            return np.inf
    return float(lmax * np.linalg.norm(x))


def solve(t, ypr, sequence, fixed, loop_i, loop_c, loop_meas, opt=None, dt=np.float64, path="band"):
    """gfbe_lc4_solve. Returns dict(t, yaw, drift, iterations, accepted [list], termination, status, cost_history, initial_cost, final_cost,
    radius, trace, margins, A_cost [per history entry], kappa, delta_l1, A_pose)."""
    opt = opt or options()
    G = build_graph(t, ypr, sequence, fixed, loop_i, loop_c, loop_meas, opt)
    n = G["n"]
    x_t, x_yaw = np.asarray(t, dt).reshape(-1, 3).copy(), np.asarray(ypr, dt).reshape(-1, 3)[:, 0].copy()
    free = G["free"]
    lin = linearize(G, x_yaw, x_t, opt, dt)
    cost, A_cost = lin["cost"], lin["A_cost"]
    out = dict(initial_cost=cost, cost_history=[cost], A_cost=[A_cost], g_l1=[float(np.abs(lin["g0"]).sum())], accepted=[], trace=[], margins=[("wrap", lin["wrap"], 1.0), ("huber", lin["huber"], 1.0)],
               kappa=1.0, delta_l1=0.0)

    def xnorm(yaw, tt):
        return np.sqrt((yaw[free] * yaw[free]).sum() + (tt[free] * tt[free]).sum())
    radius, decrease, it, invalid, reuse, scale, diag2 = dt(1e4), dt(2), 0, 0, False, None, None
    x_norm, term, status, nsucc, last = xnorm(x_yaw, x_t), 0, 1, 0, None
    act = lin["active"]
    for _ in range(min(opt["max_num_iterations"], 15)):
        gmax = np.abs(np.where(act, lin["g0"], 0)).max() if act.any() else dt(0)
        if radius < dt(1e-32):
            term, status = (3, 0) if gmax <= dt(1e-10) else (4, status)
            break
        out["margins"].append(("gradient", abs(float(gmax) - 1e-10), 1.0))
        if gmax <= dt(1e-10):
            term, status = 3, 0
            break
        it += 1
        if scale is None:
            scale = np.where(act, dt(1) / (dt(1) + np.sqrt(np.where(act, lin["diag0"], 0))), dt(1)).astype(dt)
        if not reuse:
            diag2 = np.minimum(np.maximum(lin["diag0"] * scale * scale, dt(1e-6)), dt(1e32))
        y, mc = lm_step(lin, scale, diag2, radius, dt, path)
        out["margins"].append(("model", abs(float(mc)), float(cost)))
        if y is None or not (mc > 0):
            out["accepted"].append(0); out["cost_history"].append(cost); out["A_cost"].append(A_cost); out["g_l1"].append(float(np.abs(lin["g0"]).sum()))
            out["trace"].append(dict(it=it, valid=False))
            invalid += 1
            if invalid >= 5:
                term, status = 4, 2
                break
            radius, decrease, reuse = radius / decrease, decrease * 2, True
            continue
        invalid = 0
        d = (scale * y)[:4 * n].reshape(n, 4)
        c_yaw, c_t = plus(x_yaw, x_t, d, dt)
        out["margins"].append(("plus_wrap", float(np.abs(np.abs(x_yaw + d[:, 0]) - 180).min()), 1.0))
        dy, dtt = c_yaw - x_yaw, c_t - x_t
        step2 = (dy[free] * dy[free]).sum() + (dtt[free] * dtt[free]).sum()
        lin_c = linearize(G, c_yaw, c_t, opt, dt)
        out["margins"] += [("wrap", lin_c["wrap"], 1.0), ("huber", lin_c["huber"], 1.0)]
        out["margins"].append(("parameter", abs(float(np.sqrt(step2)) - 1e-8 * (float(x_norm) + 1e-8)), float(np.sqrt(step2))))
        if np.sqrt(step2) <= dt(1e-8) * (x_norm + dt(1e-8)):
            out["accepted"].append(0); out["cost_history"].append(cost); out["A_cost"].append(A_cost); out["g_l1"].append(float(np.abs(lin["g0"]).sum()))
            term, status = 2, 0
            break
        change = cost - lin_c["cost"]
        out["margins"].append(("function", abs(abs(float(change)) - 1e-6 * float(cost)), A_cost + lin_c["A_cost"]))
        if abs(change) <= dt(1e-6) * cost:
            out["accepted"].append(0); out["cost_history"].append(cost); out["A_cost"].append(A_cost); out["g_l1"].append(float(np.abs(lin["g0"]).sum()))
            term, status = 1, 0
            break
        rho = change / mc
        out["margins"].append(("quality", abs(float(rho) - 1e-3), (A_cost + lin_c["A_cost"]) / float(mc)))
        if rho > dt(1e-3):
            last = (lin, scale, diag2, radius)
            out["delta_l1"] += float(np.abs(d).sum())
            x_yaw, x_t, lin, cost, A_cost = c_yaw, c_t, lin_c, lin_c["cost"], lin_c["A_cost"]
            x_norm = xnorm(x_yaw, x_t)
            out["accepted"].append(1); nsucc += 1
            out["trace"].append(dict(it=it, valid=True, accepted=True, rho=float(rho)))
            radius = min(dt(1e16), radius / max(dt(1) / dt(3), 1 - (2 * rho - 1) ** 3))
            decrease, reuse = dt(2), False
        else:
            out["accepted"].append(0)
            out["trace"].append(dict(it=it, valid=True, accepted=False, rho=float(rho)))
            radius, decrease, reuse = radius / decrease, decrease * 2, True
        out["cost_history"].append(cost); out["A_cost"].append(A_cost); out["g_l1"].append(float(np.abs(lin["g0"]).sum()))
    if last is not None:
        out["kappa"] = kappa_estimate(*last)
    yd = x_yaw[n - 1] - dt(np.asarray(ypr, np.float64).reshape(-1, 3)[n - 1, 0])
    a = yd / dt(180) * _pi(dt)
    v = np.asarray(t, dt).reshape(-1, 3)[n - 1]
    rz = np.array([np.cos(a) * v[0] - np.sin(a) * v[1], np.sin(a) * v[0] + np.cos(a) * v[1], v[2]], dt)
    xinf = max(float(np.abs(x_t).max()), float(np.abs(x_yaw).max()))
    out.update(t=x_t, yaw=x_yaw, drift=np.concatenate([[yd], x_t[n - 1] - rz]), iterations=it, termination=term, status=status, num_successful=nsucc,
               final_cost=cost, radius=radius, A_pose=out["kappa"] * (out["delta_l1"] + xinf), graph=G)
    return out
