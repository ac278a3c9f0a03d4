"""TEST MODEL. The 6-DoF loop-closure pose graph of dense_map (PoseGraph::optimize6DoF, dense_map/src/pose_graph.cpp:707-873; the factor
RelativeRTError, pose_graph.h:290-352) restated in numpy for a dtype argument (float64 / longdouble): the factor with its analytic
tangent Jacobian, the Huber corrector, QuaternionParameterization::Plus and Ceres 1.14's Levenberg-Marquardt loop (Jacobi scaling, the
statements and order of tests/lc4_np.py, whose linear-algebra pieces are used as they are). Two solve paths over ONE linearisation:

  dense — the normal equations assembled densely, an unblocked Cholesky (small graphs only);
  band  — the device's structure phase for phase (ground-fusion2_amd/csrc/gfbe_loopgraph6.hip): a pose takes 8 rows (6 tangent
          dimensions [dq, t] and 2 identity rows), four poses form a 32 x 32 super-block, the sequence edges give a block-tridiagonal T,
          a loop edge six sparse columns of U with 12 non-zeros each, H = T + U U^T; parallel block cyclic reduction over the
          super-blocks with the right-hand-side panel [-g | U], then the capacitance system S = I + U^T Z (6 n_loop rows, rounded up
          to a 16-column tile) by a block LDL^T in 16-wide tiles and y = z_0 - Z S^-1 U^T z_0.

A pose is out of the problem when it is fixed or touches no edge with a free pose: zero columns, identity diagonal, zero gradient, no
part in the scaling, the norms or the step. An edge between two fixed poses is dropped (Ceres removes the residual block).

A_X, the absolute sum behind an entry X (the unit of every bound is u A_X): every sum of the formula with each term's magnitude —
the rotation matrix' entries 1 + 2 (y^2 + z^2), 2 (|x y| + |z w|), ...; the quaternion products with |a_k| |b_k| summed."""
import numpy as np

from lc4_np import LD, U, cap_solve, chol_solve_dense, gj_inverse, huber_corrector, pcr_solve      # noqa: F401 (generic in the block size)

MAX_LOOPS = 128
SB = 32          # rows of a super-block
PR = 8           # rows of a pose
TILE = 16
_IDX = np.array([[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]])
_SL = np.array([[1, -1, -1, -1], [1, 1, -1, 1], [1, 1, 1, -1], [1, -1, 1, 1]])      # L(a): a * b = L(a) b
_SR = np.array([[1, -1, -1, -1], [1, 1, 1, -1], [1, -1, 1, 1], [1, 1, -1, 1]])      # R(b): a * b = R(b) a


def options(**kw):
    o = dict(huber_delta=0.1, max_num_iterations=5, span=4, t_var=0.1, q_var=0.01)
    o.update(kw)
    return o


def qmul(a, b):
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def qmul_abs(a, b):
    """The four-term sums of qmul with every term's magnitude."""
    a, b = np.abs(a), np.abs(b)
    return np.stack([(a[..., _IDX[k]] * b).sum(axis=-1) for k in range(4)], axis=-1)


def qconj(a):
    return a * np.array([1, -1, -1, -1], a.dtype)


def quat_to_R(q, dt):
    """[E, 9] row-major R of the normalised quaternion (w, x, y, z), and the same sums with every term's magnitude."""
    q = np.asarray(q, dt)
    nn = np.sqrt((q * q).sum(axis=-1))
    w, x, y, z = (q[..., k] / nn for k in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=-1)
    a = np.abs
    RA = np.stack([1 + 2 * (y * y + z * z), 2 * (a(x * y) + a(z * w)), 2 * (a(x * z) + a(y * w)), 2 * (a(x * y) + a(z * w)), 1 + 2 * (x * x + z * z),
                   2 * (a(y * z) + a(x * w)), 2 * (a(x * z) + a(y * w)), 2 * (a(y * z) + a(x * w)), 1 + 2 * (x * x + y * y)], axis=-1)
    return R, RA.astype(np.float64)


def factor(qi, ti, qj, tj, meas, t_var, q_var, dt):
    """Vectorised over edges: r [E, 6], J [E, 6, 12] (columns dq_i t_i dq_j t_j), and the absolute sums A_r, A_J behind them."""
    qi, ti, qj, tj, meas = (np.asarray(v, dt) for v in (qi, ti, qj, tj, meas))
    t_var, q_var = dt(t_var), dt(q_var)
    E = len(qi)
    R, RA = quat_to_R(qi, dt)
    d = tj - ti
    dabs = (np.abs(tj) + np.abs(ti)).astype(np.float64)
    r, J = np.zeros((E, 6), dt), np.zeros((E, 6, 12), dt)
    Ar, AJ = np.zeros((E, 6)), np.zeros((E, 6, 12))
    tv, qv = float(t_var), float(q_var)
    dx = [[None, (-1, 2), (1, 1)], [(1, 2), None, (-1, 0)], [(-1, 1), (1, 0), None]]      # [d]_x: (sign, component)
    for a in range(3):
        r[:, a] = (R[:, a] * d[:, 0] + R[:, 3 + a] * d[:, 1] + R[:, 6 + a] * d[:, 2] - meas[:, a]) / t_var
        Ar[:, a] = (RA[:, a] * dabs[:, 0] + RA[:, 3 + a] * dabs[:, 1] + RA[:, 6 + a] * dabs[:, 2] + np.abs(meas[:, a]).astype(np.float64)) / tv
        for b in range(3):
            s, sa = dt(0), 0.0
            for k in range(3):
                if dx[k][b] is not None:
                    sg, comp = dx[k][b]
                    s = s + R[:, 3 * k + a] * (sg * d[:, comp])
                    sa = sa + RA[:, 3 * k + a] * dabs[:, comp]
            J[:, a, b] = 2 * s / t_var
            AJ[:, a, b] = 2 * sa / tv
            J[:, a, 3 + b] = -R[:, 3 * b + a] / t_var
            J[:, a, 9 + b] = R[:, 3 * b + a] / t_var
            AJ[:, a, 3 + b] = AJ[:, a, 9 + b] = RA[:, 3 * b + a] / tv
    A = qmul(qconj(meas[:, 3:]), qconj(qi))
    Aabs = qmul_abs(meas[:, 3:], qi)
    e = qmul(A, qj)
    eabs = qmul_abs(Aabs, qj).astype(np.float64)
    r[:, 3:] = 2 * e[:, 1:] / q_var
    Ar[:, 3:] = 2 * eabs[:, 1:] / qv
    qja = np.abs(qj)
    for a in range(3):
        for b in range(3):
            s, sa = dt(0), 0.0
            for k in range(4):
                s = s + (_SL[a + 1, k] * A[:, _IDX[a + 1, k]]) * (_SR[k, b + 1] * qj[:, _IDX[k, b + 1]])
                sa = sa + Aabs[:, _IDX[a + 1, k]] * qja[:, _IDX[k, b + 1]]
            J[:, 3 + a, 6 + b] = 2 * s / q_var
            J[:, 3 + a, b] = -2 * s / q_var
            AJ[:, 3 + a, 6 + b] = AJ[:, 3 + a, b] = 2 * sa.astype(np.float64) / qv
    return r, J, Ar, AJ


def eval_edges(q, t, edge_i, edge_j, kind, meas, opt, dt):
    """What gfbe_lc6_eval returns: r [E, 6], J [E, 6, 12], cost with the loss; and the absolute sums A_r, A_J, A_cost, and the smallest
    distance of a kind-1 block's squared norm from the Huber threshold (in units of its absolute sum)."""
    q, t, meas = np.asarray(q, dt).reshape(-1, 4), np.asarray(t, dt).reshape(-1, 3), np.asarray(meas, dt).reshape(-1, 7)
    ei, ej, kind = np.asarray(edge_i, np.int64), np.asarray(edge_j, np.int64), np.asarray(kind, np.int64)
    if len(ei) == 0:
        return dict(r=np.zeros((0, 6), dt), J=np.zeros((0, 6, 12), dt), cost=dt(0), A_r=np.zeros((0, 6)), A_J=np.zeros((0, 6, 12)), A_cost=0.0,
                    cost_e=np.zeros(0, dt), huber=np.inf)
    r, J, Ar, AJ = factor(q[ei], t[ei], q[ej], t[ej], meas, opt["t_var"], opt["q_var"], dt)
    cost_e, hub = np.zeros(len(ei), dt), np.inf
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
    return dict(r=r, J=J, cost=cost, cost_e=cost_e, A_r=Ar, A_J=AJ, A_cost=A_cost + float(cost), huber=hub)


def sequence_meas(ta, qa, tb, qb, dt):
    """[t(3) | q wxyz]: R(q_a)^T (t_b - t_a) through the rotation matrix, q_a^-1 q_b (the conjugate)."""
    R = quat_to_R(np.asarray([qa], dt), dt)[0][0]
    d = np.asarray(tb, dt) - np.asarray(ta, dt)
    m = [R[a] * d[0] + R[3 + a] * d[1] + R[6 + a] * d[2] for a in range(3)]
    return np.concatenate([np.array(m, dt), qmul(qconj(np.asarray(qa, dt)), np.asarray(qb, dt))])


def plan(n, n_loop):
    """The plan of gfbe_loopgraph6.h (lc6_plan) without the scratch offsets."""
    M = (n + 3) // 4
    sweeps = 0
    while (1 << sweeps) < M:
        sweeps += 1
    ncol = 1 + 6 * n_loop
    ntile = (ncol + TILE - 1) // TILE
    cap = 6 * n_loop
    return dict(M=M, rows=SB * M, pad_poses=4 * M - n, sweeps=sweeps, ncol=ncol, ntile=ntile, ld=TILE * ntile, cap=cap,
                cap_ld=TILE * ((cap + TILE - 1) // TILE) if cap else TILE)


def build_graph(t, q, sequence, fixed, loop_i, loop_c, loop_meas, opt):
    """The edge list of optimize6DoF: sequence edges (i - k, i), k = 1 .. span, between poses of one sequence, their measurements formed
    from the input poses IN FP64 (they are data of the problem: both precisions solve the same graph), then the loop edges (c, i).
    Edges with two fixed ends are dropped; free[i] = not fixed and on a kept edge."""
    t, q = np.asarray(t, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 4)
    n = len(t)
    fixed = np.asarray(fixed).astype(bool)
    ei, ej, kind, meas = [], [], [], []
    for i in range(n):
        for k in range(1, opt["span"] + 1):
            if i - k >= 0 and sequence[i] == sequence[i - k] and not (fixed[i] and fixed[i - k]):
                ei.append(i - k); ej.append(i); kind.append(0)
                meas.append(sequence_meas(t[i - k], q[i - k], t[i], q[i], np.float64))
    n_seq = len(ei)
    lm = np.asarray(loop_meas, np.float64).reshape(-1, 7)
    loop_on = []
    for l in range(len(loop_i)):
        c, i = int(loop_c[l]), int(loop_i[l])
        on = not (fixed[c] and fixed[i])
        loop_on.append(on)
        if on:
            ei.append(c); ej.append(i); kind.append(1)
            meas.append(lm[l])
    free = np.zeros(n, bool)
    for a, b in zip(ei, ej):
        free[a] = free[b] = True
    free &= ~fixed
    return dict(n=n, edge_i=np.array(ei, np.int64), edge_j=np.array(ej, np.int64), kind=np.array(kind, np.int64),
                meas=np.array(meas, np.float64).reshape(-1, 7), n_seq=n_seq, free=free, loop_on=np.array(loop_on, bool), n_loop=len(loop_i))


def plus(q, t, d, dt):
    """QuaternionParameterization::Plus on q (d = 0: q as it is), identity on t; d [n, 6] = dq dt. No renormalisation."""
    dq = d[:, :3]
    nrm = np.sqrt((dq * dq).sum(axis=1))
    pos = nrm > 0
    safe = np.where(pos, nrm, dt(1))
    sn = np.sin(safe) / safe
    dQ = np.concatenate([np.cos(safe)[:, None], sn[:, None] * dq], axis=1)
    return np.where(pos[:, None], qmul(dQ, q), q).astype(dt), t + d[:, 3:]


def _rows(p):
    return list(range(PR * p, PR * p + 6))


def linearize(G, q, t, opt, dt):
    """cost, and the structure both solve paths share: the band of the sequence part in super-blocks (Hb, Ha = block (m, m - 1),
    Hc = block (m, m + 1)), the sequence gradient, and per loop edge its corrected Jacobian (six columns of U with 12 non-zeros each),
    rows, gradient and diagonal shares. Columns of a pose that is out of the problem are zero."""
    n, P = G["n"], plan(G["n"], 0)
    M = P["M"]
    ev = eval_edges(q, t, G["edge_i"], G["edge_j"], G["kind"], G["meas"], opt, dt)
    J, r = ev["J"].copy(), ev["r"]
    free = G["free"]
    for e in range(len(J)):
        if not free[G["edge_i"][e]]:
            J[e, :, 0:6] = 0
        if not free[G["edge_j"][e]]:
            J[e, :, 6:12] = 0
    Hb, Ha, Hc, g = np.zeros((M, SB, SB), dt), np.zeros((M, SB, SB), dt), np.zeros((M, SB, SB), dt), np.zeros(SB * M, dt)

    def add(pi, pj, blk):
        mi, mj, ri, rj = pi // 4, pj // 4, PR * (pi % 4), PR * (pj % 4)
        tgt = Hb if mi == mj else (Ha if mi == mj + 1 else Hc)
        assert abs(mi - mj) <= 1
        tgt[mi, ri:ri + 6, rj:rj + 6] += blk
    JtJ, Jtr = np.einsum("eqa,eqb->eab", J, J), np.einsum("eqa,eq->ea", J, r)
    for e in range(G["n_seq"]):
        a, b = int(G["edge_i"][e]), int(G["edge_j"][e])
        add(a, a, JtJ[e, 0:6, 0:6]); add(b, b, JtJ[e, 6:12, 6:12]); add(b, a, JtJ[e, 6:12, 0:6]); add(a, b, JtJ[e, 0:6, 6:12])
        g[_rows(a)] += Jtr[e, 0:6]
        g[_rows(b)] += Jtr[e, 6:12]
    L = len(J) - G["n_seq"]
    Uv, Urow = np.zeros((L, 6, 12), dt), np.zeros((L, 12), np.int64)
    gl, dl = np.zeros((L, 12), dt), np.zeros((L, 12), dt)
    for l in range(L):
        e = G["n_seq"] + l
        a, b = int(G["edge_i"][e]), int(G["edge_j"][e])
        Uv[l] = J[e]
        Urow[l] = _rows(a) + _rows(b)
        gl[l] = J[e].T @ r[e]
        dl[l] = (J[e] * J[e]).sum(axis=0)
    g0, diag0 = g.copy(), np.array([Hb[m, k, k] for m in range(M) for k in range(SB)], dt)
    for l in range(L):
        for k in range(12):
            g0[Urow[l, k]] += gl[l, k]
            diag0[Urow[l, k]] += dl[l, k]
    active = np.zeros((4 * M, PR), bool)
    active[:n, :6] = free[:, None]
    return dict(cost=ev["cost"], A_cost=ev["A_cost"], huber=ev["huber"], Hb=Hb, Ha=Ha, Hc=Hc, Uv=Uv, Urow=Urow, g0=g0, diag0=diag0,
                active=active.reshape(-1), M=M, L=L)


# ---- the two solve paths ------------------------------------------------------------------------------------------------------------
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
    ncol = 1 + 6 * L
    if path == "dense":
        H = band_to_dense(B, As, Cs)
        for l in range(L):
            for q in range(6):
                H[np.ix_(lin["Urow"][l], lin["Urow"][l])] += np.outer(Us[l, q], Us[l, q])
        y = chol_solve_dense(H, rhs, dt)
    else:
        panel = np.zeros((M, SB, ncol), dt)
        panel[:, :, 0] = rhs.reshape(M, SB)
        for l in range(L):
            for q in range(6):
                for k in range(12):
                    row = lin["Urow"][l, k]
                    panel[row // SB, row % SB, 1 + 6 * l + q] = Us[l, q, k]
        Z, ok = pcr_solve(B, As, Cs, panel, dt)
        Z = Z.reshape(SB * M, ncol)
        y = Z[:, 0].copy() if ok else None
        if ok and L:
            P = plan(4, L)
            S, v = np.eye(P["cap_ld"], dtype=dt), np.zeros(P["cap_ld"], dt)
            for l in range(L):
                for q in range(6):
                    a = 6 * l + q
                    for k in range(12):      # fixed order: the column's 12 non-zeros
                        S[a, :6 * L] += Us[l, q, k] * Z[lin["Urow"][l, k], 1:]
                        v[a] += Us[l, q, k] * Z[lin["Urow"][l, k], 0]
            w = cap_solve(S, v, dt)
            if w is None:
                y = None
            else:
                y = y - Z[:, 1:] @ w[:6 * L]
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
    2200 rows, 12 power and 12 inverse iterations beyond (estimates from below)."""
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
    if len(act) <= 2200:
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


def drift_of(q_out, t_out, q_in, t_in, dt):
    """pose_graph.cpp:849-850 of the last keyframe: q_drift = q_out q_in^-1, t_drift = t_out - R(q_drift) t_in."""
    qd = qmul(np.asarray(q_out, dt), qconj(np.asarray(q_in, dt)))
    R = quat_to_R(qd[None], dt)[0][0].reshape(3, 3)
    return np.concatenate([qd, np.asarray(t_out, dt) - R @ np.asarray(t_in, dt)])


def solve(t, q, sequence, fixed, loop_i, loop_c, loop_meas, opt=None, dt=np.float64, path="band"):
    """gfbe_lc6_solve. Returns dict(t, q, drift, iterations, accepted [list], termination, status, cost_history, initial_cost, final_cost,
    radius, trace, margins, A_cost [per history entry], kappa, delta_l1, A_pose)."""
    opt = opt or options()
    G = build_graph(t, q, sequence, fixed, loop_i, loop_c, loop_meas, opt)
    n = G["n"]
    x_t, x_q = np.asarray(t, dt).reshape(-1, 3).copy(), np.asarray(q, dt).reshape(-1, 4).copy()
    free = G["free"]
    lin = linearize(G, x_q, x_t, opt, dt)
    cost, A_cost = lin["cost"], lin["A_cost"]
    out = dict(initial_cost=cost, cost_history=[cost], A_cost=[A_cost], g_l1=[float(np.abs(lin["g0"]).sum())], accepted=[], trace=[], margins=[("huber", lin["huber"], 1.0)],
               kappa=1.0, delta_l1=0.0)

    def xnorm(qq, tt):
        return np.sqrt((qq[free] * qq[free]).sum() + (tt[free] * tt[free]).sum())
    radius, decrease, it, invalid, reuse, scale, diag2 = dt(1e4), dt(2), 0, 0, False, None, None
    x_norm, term, status, nsucc, last = xnorm(x_q, x_t), 0, 1, 0, None
    act = lin["active"]

    def keep():
        out["cost_history"].append(cost); out["A_cost"].append(A_cost); out["g_l1"].append(float(np.abs(lin["g0"]).sum()))
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
            out["accepted"].append(0); keep()
            out["trace"].append(dict(it=it, valid=False))
            invalid += 1
            if invalid >= 5:
                term, status = 4, 2
                break
            radius, decrease, reuse = radius / decrease, decrease * 2, True
            continue
        invalid = 0
        d = (scale * y).reshape(-1, PR)[:n, :6]
        c_q, c_t = plus(x_q, x_t, d, dt)
        dq, dtt = c_q - x_q, c_t - x_t
        step2 = (dq[free] * dq[free]).sum() + (dtt[free] * dtt[free]).sum()
        lin_c = linearize(G, c_q, c_t, opt, dt)
        out["margins"].append(("huber", lin_c["huber"], 1.0))
        out["margins"].append(("parameter", abs(float(np.sqrt(step2)) - 1e-8 * (float(x_norm) + 1e-8)), float(np.sqrt(step2))))
        if np.sqrt(step2) <= dt(1e-8) * (x_norm + dt(1e-8)):
            out["accepted"].append(0); keep()
            term, status = 2, 0
            break
        change = cost - lin_c["cost"]
        out["margins"].append(("function", abs(abs(float(change)) - 1e-6 * float(cost)), A_cost + lin_c["A_cost"]))
        if abs(change) <= dt(1e-6) * cost:
            out["accepted"].append(0); keep()
            term, status = 1, 0
            break
        rho = change / mc
        out["margins"].append(("quality", abs(float(rho) - 1e-3), (A_cost + lin_c["A_cost"]) / float(mc)))
        if rho > dt(1e-3):
            last = (lin, scale, diag2, radius)
            out["delta_l1"] += float(np.abs(d).sum())
            x_q, x_t, lin, cost, A_cost = c_q, c_t, lin_c, lin_c["cost"], lin_c["A_cost"]
            x_norm = xnorm(x_q, x_t)
            out["accepted"].append(1); nsucc += 1
            out["trace"].append(dict(it=it, valid=True, accepted=True, rho=float(rho)))
            radius = min(dt(1e16), radius / max(dt(1) / dt(3), 1 - (2 * rho - 1) ** 3))
            decrease, reuse = dt(2), False
        else:
            out["accepted"].append(0)
            out["trace"].append(dict(it=it, valid=True, accepted=False, rho=float(rho)))
            radius, decrease, reuse = radius / decrease, decrease * 2, True
        keep()
    if last is not None:
        out["kappa"] = kappa_estimate(*last)
    q_in, t_in = np.asarray(q, np.float64).reshape(-1, 4)[n - 1], np.asarray(t, np.float64).reshape(-1, 3)[n - 1]
    xinf = max(float(np.abs(x_t).max()), float(np.abs(x_q).max()))
    out.update(t=x_t, q=x_q, drift=drift_of(x_q[n - 1], x_t[n - 1], q_in, t_in, dt), iterations=it, termination=term, status=status, num_successful=nsucc,
               final_cost=cost, radius=radius, A_pose=out["kappa"] * (out["delta_l1"] + xinf), graph=G)
    return out
