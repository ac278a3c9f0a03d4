"""The global_fusion pose graph in extended precision — the model tests/test_posegraph_model.py (CPU: the oracle) and
tests/test_gpu_posegraph_model.py (device) hold gfo_pg_* / gfbe_pg_* against — and the named graphs that reach every path of
csrc/gfbe_posegraph.hip. numpy.longdouble throughout; neither the product nor the oracle is imported. The same role as
preint_np.py and prior_np.py.

Model. Restated from Factors.h:26-114 and globalOpt.cpp:107-236 as include/gfbe.h section f3 describes them:
  residuals   RelativeRTError: t part = (rotate(conj(q_i) / |q_i|, t_j - t_i) - t_meas) / t_var, the rotation as the quaternion
              sandwich q v q* (QuaternionRotatePoint normalises its quaternion); q part = 2 vec(conj(q_meas) (conj(q_i) q_j)) / q_var,
              the products NOT normalised. TError (t - t_meas) / var under HuberLoss(delta) through the Corrector: cost rho / 2, residual
              and Jacobian rescaled by sqrt(rho') (Huber's rho'' <= 0: the Corrector's alpha is zero).
  plus        QuaternionParameterization::Plus, q <- [cos|d|, sin|d| / |d| d] q, identity on t; tangent [dq(3), dt(3)].
  jacobians   NOT the device's formulas: Romberg (Richardson-extrapolated central differences) of `residuals` through `plus`, steps
              2^-4 .. 2^-9 (powers of two: t +- h is exact), the scheme's own error estimated from its last two levels and asserted
              below JAC_ERR = 1e-13 of each block's scale by the CPU module.
  lm_system   block-tridiagonal H = J^T J (Hd, Ho = block (i + 1, i)), g = J^T r, the Jacobi scale 1 / (1 + sqrt(H_ii)), the
              Levenberg-Marquardt diagonal clamp(diag(S H S), 1e-6, 1e32) / radius, and the step from a dense longdouble LDL^T
              (6 n <= DENSE_MAX) or a longdouble block-tridiagonal recurrence (above); the CPU module cross-checks the two.
  solve       the trust-region loop with the rules of gfo_pg_solve / k_pg_decide (radius 1e4, five invalid steps, diag2 kept on a
              rejected step, gradient / parameter / function tolerance), with the margin of every decision.
  pcr_fp64    the device's METHOD in plain FP64 numpy: parallel block cyclic reduction with travelling explicit inverses
              (csrc/gfbe_posegraph.hip, the comment above k_pg_pcr). Its only purpose is to measure the method's rounding floor.

Scales (what "u * scale" means per block; every one a product or sum of the magnitudes of the operands of the block's formula):
  rel_r t part      (|t_j - t_i| + |t_meas|) / t_var            rel_r q part         2 |q_meas| |q_i| |q_j| / q_var
  rel_J (t, dq_i)   2 |t_j - t_i| / t_var                       rel_J (t, t_i / t_j) 1 / t_var
  rel_J (q, dq_i / dq_j)   2 |q_meas| |q_i| |q_j| / q_var       rel_J (t, dq_j), (q, t_i), (q, t_j): structural zeros, exact
  fix_r             |fix_r| of the fix (a fix exactly at the pose: scale 0, exact)
  cost              sum |r| scale over the relative residuals + sum rho over the fixes (>= 2 cost)

Cases (case(name); seeds fixed; sizes the smallest that still reach the path).
  factor cases, for eval: mixed (n = 33: rel_i shuffled, fixes unsorted, two fixes on pose 8, the fix of pose 12 far outside delta,
      the fix of pose 16 exactly at the pose), gaps (n = 65, no factor starts at 0, 31, 63), nonunit (|q| = 1 +- 1e-3, poses and
      measurements), near_pi (n = 9, rotation errors within 1e-3 of pi, measurement 3 given as -q), far (everything offset by
      1e4 m), single (n = 1, one fix), empty (n = 1, nothing).
  cost-only: cost4097, cost8200 (two and three segments of the device's reduction).
  solve cases: n1, n2, n3, n32, n33, n64, n65, n257, n1025 (a fix on every fifth pose, in shuffled order), one_fix (n = 65, one
      fix on the last pose), split (n = 65, factors 20 and 43 missing: three components, the middle one without a fix),
      huber (n = 64, the start thrown 3 m off: most fixes are outliers at the start).

Measured on the CPU by tests/test_posegraph_model.py (which asserts every figure, so that none can drift), never on the device:
  K_MEASURED: worst |FP64 statement - model| / (u scale) per block family over the factor cases (the cost: over the cost-only cases too), the larger of the
      oracle and of this module's own formulas evaluated in FP64:
          %(KM)s
      K_FACTOR = K_MARGIN (8) x the largest, rounded up to a power of two = %(K)g.
  STEP_FLOOR: per solve case, max(|oracle first step - model|, |pcr_fp64 step - model|), max over the 7 n pose entries (metres, and
      quaternion entries), x 1.25 and rounded up; the device's bound is STEP_MARGIN (16) x this (the up-to-11 reduction levels at
      n = 1025, each with a freshly inverted block where the recurrence factorises once). Measured (oracle, pcr_fp64): n1 (8.1e-17, 3.3e-17)
      n2 (1.2e-14, 2e-14)   n3 (9.1e-15, 8.6e-15)   n32 (1.1e-14, 4.3e-15)   n33 (9.8e-15, 3.2e-15)   n64 (5e-15, 6e-15)   n65 (6.3e-15, 5.6e-15)
      n257 (3.7e-15, 3.7e-15)   n1025 (1e-14, 6e-15)   one_fix (8.2e-15, 1.8e-14)   split (1.2e-14, 9.7e-15)   huber (2.6e-13, 5.6e-13). Stored:
          %(SF)s
  LOOP_FLOOR: per full-loop case (max_iterations = 15), what the oracle's own loop reaches against the model: (max |pose
      difference|, max |difference of a cost history entry| / initial cost), x 1.25 and rounded up (several of these graphs end on costs
      that are rounding, so the history is not compared entry-relative):
          %(LF)s
"""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
T_VAR, Q_VAR, DELTA = 0.1, 0.01, 1.0
OK, NO_CONVERGENCE, NUMERICAL_FAILURE, BAD_INPUT = 0, 1, 2, 3          # gfbe_status (include/gfbe.h); the test modules assert these against abi
JAC_ERR = 1e-13
DENSE_MAX = 400
MARGIN_MIN = 1e-6
FAMILIES = ("rel_r_t", "rel_r_q", "J_t_dqi", "J_t_t", "J_q_dq", "fix_r", "cost")

# ---- measured by tests/test_posegraph_model.py on the CPU (see the module docstring)
K_MARGIN, STEP_MARGIN = 8.0, 16.0
K_MEASURED = dict(rel_r_t=2.0, rel_r_q=1.7, J_t_dqi=2.0, J_t_t=1.3, J_q_dq=3.1, fix_r=1.3, cost=1.1)
K_FACTOR = 2.0 ** np.ceil(np.log2(K_MARGIN * max(K_MEASURED.values())))
STEP_FLOOR = dict(n1=1.1e-16, n2=2.5e-14, n3=1.2e-14, n32=1.5e-14, n33=1.3e-14, n64=7.6e-15, n65=7.9e-15, n257=4.7e-15, n1025=1.3e-14, one_fix=2.4e-14,
                  split=1.6e-14, huber=7e-13)
LOOP_FLOOR = dict(n1=(3.1e-17, 8.3e-17), n2=(1.7e-15, 4e-16), n3=(4e-16, 3.1e-16), n32=(7.5e-11, 1.4e-13), n33=(1.8e-12, 3.3e-14), n64=(6.7e-12, 1.5e-14),
                  n65=(9.9e-13, 1.1e-13), n257=(8.6e-15, 6.4e-16), one_fix=(3.7e-14, 1.2e-15), split=(6.1e-11, 1.4e-12), huber=(1.8e-11, 1.2e-15))

FACTOR_CASES = ("mixed", "gaps", "nonunit", "near_pi", "far", "single", "empty")
COST_CASES = ("cost4097", "cost8200")
SOLVE_SIZES = (1, 2, 3, 32, 33, 64, 65, 257, 1025)
VARIANTS = ("one_fix", "split", "huber")
SOLVE_CASES = tuple("n%d" % n for n in SOLVE_SIZES) + VARIANTS
LOOP_CASES = tuple("n%d" % n for n in SOLVE_SIZES if n <= 257) + VARIANTS


def require_extended_precision():
    import pytest
    if np.finfo(LD).nmant < 63:
        pytest.skip("numpy.longdouble has a %d-bit mantissa on this host: no extended-precision reference" % np.finfo(LD).nmant)


# ---------------------------------------------------------------------------------------------------------------- quaternions (w x y z)
def qmul(a, b):
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def qconj(a):
    return a * np.array([1, -1, -1, -1], a.dtype)


def _norm(v):
    return np.sqrt(np.sum(v * v, axis=-1))


def rotate(q, v):
    """ceres::QuaternionRotatePoint: q is normalised first, then q [0, v] q*."""
    qn = q / _norm(q)[..., None]
    p = np.concatenate([np.zeros_like(v[..., :1]), v], axis=-1)
    return qmul(qmul(qn, p), qconj(qn))[..., 1:]


def plus(x, d6):
    """QuaternionParameterization::Plus on q, identity on t; x [..., 7] = t q, d6 [..., 6] = dq dt."""
    dq = d6[..., :3]
    nrm = _norm(dq)
    pos = nrm > 0
    safe = np.where(pos, nrm, 1)
    sc = np.where(pos, np.sin(safe) / safe, 0)
    dQ = np.concatenate([np.where(pos, np.cos(nrm), 1)[..., None], sc[..., None] * dq], axis=-1)
    return np.concatenate([x[..., :3] + d6[..., 3:], qmul(dQ, np.broadcast_to(x[..., 3:], dQ.shape))], axis=-1)


# ---------------------------------------------------------------------------------------------------------------- factors
def rel_residual(pi, pj, meas, t_var, q_var):
    """RelativeRTError (Factors.h:61-99) of poses pi, pj [..., 7] and measurement [..., 7]."""
    iqw = qconj(pi[..., 3:])
    rt = (rotate(iqw, pj[..., :3] - pi[..., :3]) - meas[..., :3]) / t_var
    e = qmul(qconj(meas[..., 3:]), qmul(iqw, pj[..., 3:]))
    return np.concatenate([rt, 2 * e[..., 1:] / q_var], axis=-1)


def _arrays(g, pose, dtype):
    pose = np.asarray(g["pose"] if pose is None else pose, dtype).reshape(-1, 7)
    ri, fi = np.asarray(g["rel_i"], np.int64).reshape(-1), np.asarray(g["fix_i"], np.int64).reshape(-1)
    return pose, ri, np.asarray(g["rel_meas"], dtype).reshape(-1, 7), fi, np.asarray(g["fix_meas"], dtype).reshape(-1, 4)


def residuals(g, pose=None, dtype=LD):
    """Residuals (in the caller's factor order), cost and the scales of the module docstring. dtype = numpy.float64 turns the model
    into the vectorised FP64 statement the rounding floor is measured with."""
    pose, ri, rm, fi, fm = _arrays(g, pose, dtype)
    t_var, q_var, delta = dtype(T_VAR), dtype(Q_VAR), dtype(DELTA)
    pi, pj = pose[ri], pose[ri + 1]
    rel_r = rel_residual(pi, pj, rm, t_var, q_var)
    raw = (pose[fi, :3] - fm[:, :3]) / fm[:, 3:4]
    sq = np.sum(raw * raw, axis=-1)
    out = sq > delta * delta
    rr = np.sqrt(np.where(out, sq, 1))
    rho = np.where(out, 2 * delta * rr - delta * delta, sq)
    rho1 = np.where(out, delta / rr, 1)
    fix_r = np.sqrt(rho1)[:, None] * raw
    terms = np.concatenate([np.sum(rel_r * rel_r, axis=-1) / 2, rho / 2])
    total = np.sum(terms) if dtype is LD else np.cumsum(np.append(terms, 0))[-1]      # (FP64: one term after the other, the same on every host)
    d, qs = _norm(pj[:, :3] - pi[:, :3]), _norm(rm[:, 3:]) * _norm(pi[:, 3:]) * _norm(pj[:, 3:])
    s_t, s_q = (d + _norm(rm[:, :3])) / t_var, 2 * qs / q_var
    rel_scale = np.concatenate([np.repeat(s_t[:, None], 3, 1), np.repeat(s_q[:, None], 3, 1)], axis=1)
    J_scale = np.zeros((len(ri), 6, 12), dtype)
    J_scale[:, :3, 0:3] = (2 * d / t_var)[:, None, None]
    J_scale[:, :3, 3:6] = 1 / t_var
    J_scale[:, :3, 9:12] = 1 / t_var
    J_scale[:, 3:, 0:3] = s_q[:, None, None]
    J_scale[:, 3:, 6:9] = s_q[:, None, None]
    return dict(rel_r=rel_r, fix_r=fix_r, fix_raw=raw, rho1=rho1, outlier=out, terms=terms, cost=total, rel_scale=rel_scale,
                J_scale=J_scale, fix_scale=_norm(fix_r), cost_scale=np.sum(np.abs(rel_r) * rel_scale) + np.sum(rho))


ROMBERG_LEVELS, ROMBERG_H0 = 6, 2.0 ** -4


def _romberg(f):
    """d f(h) / dh at 0 from central differences at h = H0 / 2^l, Richardson-extrapolated; (value, |last two levels' difference|)."""
    T = []
    for l in range(ROMBERG_LEVELS):
        h = LD(ROMBERG_H0) / LD(2 ** l)
        T.append((f(h) - f(-h)) / (2 * h))
    for m in range(1, ROMBERG_LEVELS):
        prev = T
        T = [prev[l + 1] + (prev[l + 1] - prev[l]) / LD(4 ** m - 1) for l in range(len(prev) - 1)]
    return T[0], np.abs(T[0] - prev[1])


def jacobians(g, pose=None):
    """rel_J [m, 6, 12] (columns dq_i t_i dq_j t_j), the scheme's error estimate per entry, fix_J [k, 3, 3] (corrected, with respect to t)."""
    pose, ri, rm, fi, fm = _arrays(g, pose, LD)
    pi, pj = pose[ri], pose[ri + 1]
    J, E = np.zeros((len(ri), 6, 12), LD), np.zeros((len(ri), 6, 12), LD)
    for c in range(12):
        def f(h, c=c):
            d6 = np.zeros((len(ri), 6), LD)
            d6[:, c % 6] = h
            return rel_residual(plus(pi, d6), pj, rm, LD(T_VAR), LD(Q_VAR)) if c < 6 else rel_residual(pi, plus(pj, d6), rm, LD(T_VAR), LD(Q_VAR))
        J[:, :, c], E[:, :, c] = _romberg(f)
    res = residuals(g, pose)
    fix_J = np.zeros((len(fi), 3, 3), LD)
    h = LD(2.0 ** -4)
    for c in range(3):
        d6 = np.zeros((len(fi), 6), LD)
        d6[:, 3 + c] = h
        fix_J[:, :, c] = ((plus(pose[fi], d6)[:, :3] - fm[:, :3]) / fm[:, 3:4] - (plus(pose[fi], -d6)[:, :3] - fm[:, :3]) / fm[:, 3:4]) / (2 * h)
    fix_J *= np.sqrt(res["rho1"])[:, None, None]
    return J, E, fix_J


def linearise(g, pose=None):
    """Hd [n, 6, 6], Ho [n - 1, 6, 6] (block (i + 1, i)), grad [n, 6] and the residuals' dict."""
    pose, ri, rm, fi, fm = _arrays(g, pose, LD)
    n = len(pose)
    res = residuals(g, pose)
    J, E, fix_J = jacobians(g, pose)
    Hd, Ho, grad = np.zeros((n, 6, 6), LD), np.zeros((max(n - 1, 0), 6, 6), LD), np.zeros((n, 6), LD)
    for k, i in enumerate(ri):                      # (a sum per factor: duplicates, should a case ever carry them, add up as in the oracle)
        Ji, Jj, r = J[k, :, :6], J[k, :, 6:], res["rel_r"][k]
        Hd[i] += Ji.T @ Ji
        Hd[i + 1] += Jj.T @ Jj
        Ho[i] += Jj.T @ Ji
        grad[i] += Ji.T @ r
        grad[i + 1] += Jj.T @ r
    for k, i in enumerate(fi):
        Hd[i, 3:, 3:] += fix_J[k].T @ fix_J[k]
        grad[i, 3:] += fix_J[k].T @ res["fix_r"][k]
    return dict(Hd=Hd, Ho=Ho, g=grad, res=res, cost=res["cost"], J=J, J_err=E)


# ---------------------------------------------------------------------------------------------------------------- linear algebra
def ldlt_solve(A, b, band=None):
    """x with A x = b for a symmetric positive definite longdouble A (LDL^T on the assembled matrix, no pivoting); None when a pivot is
    not positive. band: the matrix is zero beyond that many sub-diagonals, and so is its factor: those entries are skipped."""
    A = np.array(A, LD)
    n = len(A)
    w = n if band is None else band
    z = np.array(b, LD).reshape(n, -1)
    D = np.zeros(n, LD)
    for k in range(n):
        D[k] = A[k, k]
        if not D[k] > 0 or not np.isfinite(D[k]):
            return None
        hi = min(n, k + 1 + w)
        col = A[k + 1:hi, k] / D[k]
        A[k + 1:hi, k + 1:hi] -= np.outer(col, A[k + 1:hi, k])
        A[k + 1:hi, k] = col
        z[k + 1:hi] -= col[:, None] * z[k]
    z /= D[:, None]
    for k in range(n - 1, 0, -1):
        lo = max(0, k - w)
        z[lo:k] -= A[k, lo:k, None] * z[k]
    return z.reshape(np.shape(b))


def dense_of(Bd, Bo):
    n = len(Bd)
    M = np.zeros((6 * n, 6 * n), LD)
    for i in range(n):
        M[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Bd[i]
        if i + 1 < n:
            M[6 * i + 6:6 * i + 12, 6 * i:6 * i + 6] = Bo[i]
            M[6 * i:6 * i + 6, 6 * i + 6:6 * i + 12] = Bo[i].T
    return M


def solve_dense(Bd, Bo, rhs):
    y = ldlt_solve(dense_of(Bd, Bo), rhs.reshape(-1), band=11)      # (block-tridiagonal with 6 x 6 blocks: 11 sub-diagonals)
    return None if y is None else y.reshape(-1, 6)


def solve_recurrence(Bd, Bo, rhs):
    """Block-tridiagonal elimination in longdouble: D_0 = B_0, W_i = Bo_{i-1} D_{i-1}^-1, D_i = B_i - W_i Bo_{i-1}^T, z_i = b_i - W_i z_{i-1};
    y_i = D_i^-1 (z_i - Bo_i^T y_{i+1})."""
    n = len(Bd)
    D, z = np.array(Bd, LD), np.array(rhs, LD)
    for i in range(1, n):
        X = ldlt_solve(D[i - 1], np.concatenate([Bo[i - 1].T, z[i - 1][:, None]], axis=1))      # D^-1 [Bo^T | z]
        if X is None:
            return None
        D[i] = D[i] - Bo[i - 1] @ X[:, :6]
        z[i] = z[i] - Bo[i - 1] @ X[:, 6]
    y = np.zeros((n, 6), LD)
    for i in range(n - 1, -1, -1):
        b = z[i] - (Bo[i].T @ y[i + 1] if i + 1 < n else 0)
        yi = ldlt_solve(D[i], b)
        if yi is None:
            return None
        y[i] = yi
    return y


def block_matvec(Bd, Bo, y):
    out = np.einsum("iab,ib->ia", Bd, y)
    if len(Bd) > 1:
        out[1:] += np.einsum("iab,ib->ia", Bo, y[:-1])
        out[:-1] += np.einsum("iba,ib->ia", Bo, y[1:])
    return out


def lm_system(g, radius, diag2=None, pose=None, scale=None, lin=None, solver=None):
    """The Levenberg-Marquardt system at `pose`: H (Hd, Ho), g, the Jacobi scale (computed here unless the loop's is passed), diag2 =
    clamp(diag(S H S), 1e-6, 1e32) (or the kept one), lm = diag2 / radius, the scaled blocks Bs, As, rhs = -S g, y and step = S y."""
    lin = lin or linearise(g, pose)
    Hd, Ho, grad = lin["Hd"], lin["Ho"], lin["g"]
    n = len(Hd)
    if scale is None:
        scale = 1 / (1 + np.sqrt(np.einsum("iaa->ia", Hd)))
    Bs = Hd * scale[:, :, None] * scale[:, None, :]
    As = Ho * scale[1:, :, None] * scale[:-1, None, :]
    rhs = -scale * grad
    if diag2 is None:
        diag2 = np.minimum(np.maximum(np.einsum("iaa->ia", Bs), LD(1e-6)), LD(1e32))
    lm = diag2 / LD(radius)
    Breg = Bs.copy()
    Breg[:, np.arange(6), np.arange(6)] += lm
    solver = solver or (solve_dense if 6 * n <= DENSE_MAX else solve_recurrence)
    y = solver(Breg, As, rhs)
    return dict(Hd=Hd, Ho=Ho, g=grad, scale=scale, diag2=diag2, lm=lm, Bs=Bs, As=As, Breg=Breg, rhs=rhs, y=y, step=None if y is None else scale * y)


def _rel(value, threshold):
    return float(abs(value - threshold) / threshold)


def solve(g, max_it=15):
    """The trust-region loop of gfo_pg_solve / k_pg_decide in longdouble. Returns iterations, accepted, termination, status,
    cost_history (entries 0 .. iterations, as abi.summary_to_dict lists them), pose, margins [(test, iteration, relative distance of the
    tested value from its threshold)] and `first`: the first iteration's candidate, its cost and whether it was tried."""
    max_it = min(int(max_it), 15)
    x = np.asarray(g["pose"], LD).reshape(-1, 7)
    lin = linearise(g, x)
    cost = lin["cost"]
    hist, acc, margins = [cost], [0], []
    scale = 1 / (1 + np.sqrt(np.einsum("iaa->ia", lin["Hd"])))
    radius, decrease = LD(1e4), LD(2)
    x_norm = np.sqrt(np.sum(x * x))
    invalid = it = 0
    diag2, first = None, None
    status, term = NO_CONVERGENCE, 0
    while True:
        if it >= max_it:
            break
        gmax = np.max(np.abs(lin["g"]))
        margins.append(("gradient", it, _rel(gmax, LD(1e-10))))
        if gmax <= LD(1e-10):
            term, status = 3, OK
            break
        if radius < LD(1e-32):
            term = 4
            break
        it += 1
        S = lm_system(g, radius, diag2, scale=scale, lin=lin)
        diag2, y = S["diag2"], S["y"]
        mc = LD(0)
        if y is not None:
            gy, yHy = np.sum(-S["rhs"] * y), np.sum(y * block_matvec(S["Bs"], S["As"], y))
            mc = -(gy + yHy / 2)
            margins.append(("model_change", it, float(abs(mc) / (abs(gy) + abs(yHy) / 2))))
        if y is None or not mc > 0:
            acc.append(0), hist.append(cost)
            invalid += 1
            if invalid >= 5:
                term, status = 4, NUMERICAL_FAILURE
                break
            radius, decrease = radius / decrease, decrease * 2          # diag2 is kept
            continue
        invalid = 0
        cand = plus(x, scale * y)
        step = np.sqrt(np.sum((cand - x) ** 2))
        cand_cost = residuals(g, cand)["cost"]
        if first is None and it == 1:
            first = dict(candidate=cand, cost=cand_cost)
        thr = LD(1e-8) * (x_norm + LD(1e-8))
        margins.append(("parameter", it, _rel(step, thr)))
        if step <= thr:
            acc.append(0), hist.append(cost)
            term, status = 2, OK
            break
        change = cost - cand_cost
        margins.append(("function", it, _rel(abs(change), LD(1e-6) * cost)))
        if abs(change) <= LD(1e-6) * cost:
            acc.append(0), hist.append(cost)
            term, status = 1, OK
            break
        rho = change / mc
        margins.append(("rho", it, float(abs(rho - LD(1e-3)) / max(abs(rho), LD(1e-3)))))
        if rho > LD(1e-3):
            x, cost, x_norm = cand, cand_cost, np.sqrt(np.sum(cand * cand))
            acc.append(1), hist.append(cost)
            radius = min(LD(1e16), radius / max(LD(1.0 / 3.0), 1 - (2 * rho - 1) ** 3))
            decrease, diag2 = LD(2), None
            lin = linearise(g, x)
        else:
            acc.append(0), hist.append(cost)
            radius, decrease = radius / decrease, decrease * 2
    return dict(iterations=it, accepted=acc, termination=term, status=status, cost_history=hist, pose=x, margins=margins, first=first,
                final_cost=cost, final_radius=radius)


# ---------------------------------------------------------------------------------------------------------------- the device's method, FP64
def _mm(A, B):
    """Stacked 6 x 6 products as sums of elementwise products in a fixed order (no BLAS: the same bits on every host)."""
    out = A[:, :, 0, None] * B[:, 0, None, :]
    for k in range(1, A.shape[2]):
        out = out + A[:, :, k, None] * B[:, k, None, :]
    return out


def _mv(A, v):
    return _mm(A, v[:, :, None])[:, :, 0]


def _chol_inverse64(B):
    """B^-1 [n, 6, 6] in FP64: Cholesky factor column by column, then forward and back substitution on the identity."""
    n = len(B)
    L, Z, X = np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    eye = np.eye(6)
    for c in range(6):
        d = B[:, c, c].copy()
        for k in range(c):
            d -= L[:, c, k] * L[:, c, k]
        L[:, c, c] = np.sqrt(d)
        for r in range(c + 1, 6):
            v = B[:, r, c].copy()
            for k in range(c):
                v -= L[:, r, k] * L[:, c, k]
            L[:, r, c] = v / L[:, c, c]
    for r in range(6):
        v = np.broadcast_to(eye[r], (n, 6)).copy()
        for k in range(r):
            v -= L[:, r, k, None] * Z[:, k, :]
        Z[:, r, :] = v / L[:, r, r, None]
    for r in range(5, -1, -1):
        v = Z[:, r, :].copy()
        for k in range(r + 1, 6):
            v -= L[:, k, r, None] * X[:, k, :]
        X[:, r, :] = v / L[:, r, r, None]
    return X


def pcr_fp64(Breg, As, rhs):
    """y of the block-tridiagonal system in FP64 by the device's method: A_i x_{i-1} + B_i x_i + C_i x_{i+1} = d_i with A_i = As_{i-1},
    C_i = As_i^T; ceil(log2 n) sweeps at stride s = 1, 2, 4, ...
        alpha = -A_i B_{i-s}^-1, gamma = -C_i B_{i+s}^-1
        B' = B + alpha C_{i-s} + gamma A_{i+s}; d' = d + alpha d_{i-s} + gamma d_{i+s}; A' = alpha A_{i-s}; C' = gamma C_{i+s}
    the explicit inverse of every new diagonal block formed once, at the end of the sweep that produces it; then y_i = B_i^-1 d_i."""
    B, d = np.asarray(Breg, np.float64).copy(), np.asarray(rhs, np.float64).copy()
    n = len(B)
    A, C = np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    if n > 1:
        A[1:] = np.asarray(As, np.float64)
        C[:-1] = np.asarray(As, np.float64).transpose(0, 2, 1)
    Binv = _chol_inverse64(B)
    idx = np.arange(n)
    s = 1
    while s < n:
        m, p = idx[idx >= s], idx[idx + s < n]
        B2, d2, A2, C2 = B.copy(), d.copy(), np.zeros_like(A), np.zeros_like(C)
        alpha, gamma = -_mm(A[m], Binv[m - s]), -_mm(C[p], Binv[p + s])
        B2[m] += _mm(alpha, C[m - s])
        d2[m] += _mv(alpha, d[m - s])
        A2[m] = _mm(alpha, A[m - s])
        B2[p] += _mm(gamma, A[p + s])
        d2[p] += _mv(gamma, d[p + s])
        C2[p] = _mm(gamma, C[p + s])
        A, B, C, d = A2, B2, C2, d2
        Binv = _chol_inverse64(B)
        s *= 2
    return _mv(Binv, d)


# ---------------------------------------------------------------------------------------------------------------- graphs
def _q_axis(axis, angle):
    q = np.zeros(np.shape(angle) + (4,))
    q[..., 0], q[..., 1 + axis] = np.cos(0.5 * np.asarray(angle)), np.sin(0.5 * np.asarray(angle))
    return q


def _unit(q):
    return q / _norm(q)[..., None]


def chain(n, seed, fix_every=5, shuffle_fixes=True):
    """n poses on a planar random walk (steps of 0.1 m, yaw random walk 0.05 rad, small pitch and roll), a RelativeRTError per
    consecutive pair (noise 2 mm, 0.5 mrad), a TError (sigma 0.5 m, var 0.5) on every fix_every-th pose, and a start that drifts away
    from the truth (random walks of 1 cm and 1 mrad per pose) as a dead-reckoned chain does. FP64 inputs, as the C ABI takes them."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    yaw = np.cumsum(rng.normal(0, 0.05, n)) - 0.0
    step = np.column_stack([0.1 * np.cos(yaw), 0.1 * np.sin(yaw), rng.normal(0, 0.002, n)])
    t = np.vstack([np.zeros((1, 3)), np.cumsum(step[1:], axis=0)])
    q = _unit(qmul(qmul(_q_axis(2, yaw), _q_axis(1, 0.01 * np.sin(0.01 * i))), _q_axis(0, 0.01 * np.cos(0.013 * i))))
    truth = np.hstack([t, q])
    rel_i = np.arange(n - 1, dtype=np.int32)
    mt = rotate(qconj(q[:-1]), t[1:] - t[:-1]) + rng.normal(0, 0.002, (n - 1, 3))
    mq = qmul(qmul(qconj(q[:-1]), q[1:]), np.hstack([np.ones((n - 1, 1)), 0.5 * rng.normal(0, 0.0005, (n - 1, 3))]))
    rel_meas = np.hstack([mt, _unit(mq)]).reshape(-1, 7)
    fix_i = np.arange(0, n, fix_every, dtype=np.int32)
    fix_meas = np.column_stack([t[fix_i] + rng.normal(0, 0.5, (len(fix_i), 3)), np.full(len(fix_i), 0.5)])
    if shuffle_fixes:
        perm = rng.permutation(len(fix_i))
        fix_i, fix_meas = fix_i[perm], fix_meas[perm]
    drift_t = np.cumsum(rng.normal(0, 0.01, (n, 3)), axis=0)
    drift_q = np.hstack([np.ones((n, 1)), 0.5 * np.cumsum(rng.normal(0, 0.001, (n, 3)), axis=0)])
    pose = np.hstack([t + drift_t, _unit(qmul(q, drift_q))])
    return dict(n=n, pose=pose, rel_i=rel_i, rel_meas=rel_meas, fix_i=fix_i, fix_meas=fix_meas, truth=truth)


def _drop_factors(g, starts):
    keep = ~np.isin(g["rel_i"], starts)
    g["rel_i"], g["rel_meas"] = g["rel_i"][keep], g["rel_meas"][keep]


def _keep_fixes(g, keep):
    g["fix_i"], g["fix_meas"] = g["fix_i"][keep], g["fix_meas"][keep]


@functools.lru_cache(maxsize=None)
def _case(name):
    rng = np.random.default_rng(4242)
    if name in ("single", "empty"):
        g = chain(1, 71)
        if name == "empty":
            _keep_fixes(g, np.zeros(1, bool))
        return g
    if name == "mixed":
        g = chain(33, 72, fix_every=4)
        perm = rng.permutation(32)
        g["rel_i"], g["rel_meas"] = g["rel_i"][perm], g["rel_meas"][perm]
        fi, fm = g["fix_i"], g["fix_meas"]
        fm[fi == 12, :3] = g["pose"][12, :3] + np.array([30.0, -20.0, 10.0])
        fm[fi == 16, :3] = g["pose"][16, :3]
        g["fix_i"] = np.concatenate([fi[:3], [8], fi[3:]]).astype(np.int32)              # the second fix of pose 8, away from the first
        g["fix_meas"] = np.vstack([fm[:3], [np.append(g["pose"][8, :3] + [0.2, -0.1, 0.05], 0.3)], fm[3:]])
        return g
    if name == "gaps":
        g = chain(65, 73)
        _drop_factors(g, [0, 31, 63])
        return g
    if name == "nonunit":
        g = chain(33, 74)
        g["pose"][:, 3:] *= (1 + 1e-3 * np.where(np.arange(33) % 2, 1.0, -1.0) * rng.uniform(0.5, 1.0, 33))[:, None]
        g["rel_meas"][:, 3:] *= (1 + 1e-3 * np.where(np.arange(32) % 3, -1.0, 1.0) * rng.uniform(0.5, 1.0, 32))[:, None]
        return g
    if name == "near_pi":
        g = chain(9, 75)
        ax = _unit(rng.normal(size=(8, 3)))
        ang = np.pi + rng.uniform(-1e-3, 1e-3, 8)
        turn = np.hstack([np.cos(0.5 * ang)[:, None], np.sin(0.5 * ang)[:, None] * ax])
        q = g["pose"][:, 3:]
        g["rel_meas"][:, 3:] = _unit(qmul(qmul(qconj(q[:-1]), q[1:]), turn))          # the error of the START is the turn's conjugate
        g["rel_meas"][3, 3:] *= -1
        return g
    if name == "far":
        g = chain(33, 76)
        off = np.array([1e4, -1e4, 1e4])
        g["pose"][:, :3] += off
        g["fix_meas"][:, :3] += off
        return g
    if name.startswith("cost"):
        return chain(int(name[4:]), 77, fix_every=10)
    if name == "one_fix":
        g = chain(65, 78)
        _keep_fixes(g, g["fix_i"] == 64)
        g["fix_i"] = np.array([64], np.int32)
        g["fix_meas"] = np.append(g["truth"][64, :3] + [0.3, -0.2, 0.1], 0.5).reshape(1, 4)
        return g
    if name == "split":
        g = chain(65, 79)
        _drop_factors(g, [20, 43])
        _keep_fixes(g, (g["fix_i"] <= 20) | (g["fix_i"] >= 44))
        return g
    if name == "huber":
        g = chain(64, 80)
        g["pose"][:, :3] += rng.normal(0, 3.0, (64, 3))
        return g
    if name[0] == "n" and name[1:].isdigit():
        return chain(int(name[1:]), 100 + int(name[1:]))
    raise KeyError(name)


def case(name):
    """A fresh copy of the named graph (see the module docstring)."""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _case(name).items()}


@functools.lru_cache(maxsize=None)
def reference_eval(name):
    g = case(name)
    res = residuals(g)
    J, E, _ = jacobians(g)
    return dict(res, rel_J=J, J_err=E)


@functools.lru_cache(maxsize=None)
def reference_solve(name, max_it):
    return solve(case(name), max_it)


# ---------------------------------------------------------------------------------------------------------------- comparison
def _ratio(got, ref, scale):
    """max |got - ref| / (u scale); where the scale is zero the value must be exactly the model's (inf otherwise)."""
    err = np.abs(np.asarray(got, LD) - ref)
    scale = np.broadcast_to(np.asarray(scale, LD), err.shape)
    zero = scale == 0
    r = np.where(zero, np.where(err == 0, 0.0, np.inf), err / (U * np.where(zero, 1, scale)))
    return float(np.max(r)) if r.size else 0.0


def compare_eval(got, ref):
    """Worst ratio per block family of an eval result (dict of rel_r, rel_J, fix_r, cost) against reference_eval's; rel_J is optional."""
    out = dict(rel_r_t=_ratio(got["rel_r"][:, :3], ref["rel_r"][:, :3], ref["rel_scale"][:, :3]),
               rel_r_q=_ratio(got["rel_r"][:, 3:], ref["rel_r"][:, 3:], ref["rel_scale"][:, 3:]),
               fix_r=_ratio(got["fix_r"], ref["fix_r"], ref["fix_scale"][:, None]),
               cost=_ratio(got["cost"], ref["cost"], ref["cost_scale"]))
    if got.get("rel_J") is not None:
        J, Jr, Js = np.asarray(got["rel_J"]).reshape(-1, 6, 12), ref["rel_J"], ref["J_scale"]
        out["J_t_dqi"] = _ratio(J[:, :3, 0:3], Jr[:, :3, 0:3], Js[:, :3, 0:3])
        out["J_t_t"] = max(_ratio(J[:, :3, 3:6], Jr[:, :3, 3:6], Js[:, :3, 3:6]), _ratio(J[:, :3, 9:12], Jr[:, :3, 9:12], Js[:, :3, 9:12]))
        out["J_q_dq"] = max(_ratio(J[:, 3:, 0:3], Jr[:, 3:, 0:3], Js[:, 3:, 0:3]), _ratio(J[:, 3:, 6:9], Jr[:, 3:, 6:9], Js[:, 3:, 6:9]))
        zeros = np.concatenate([J[:, :3, 6:9].ravel(), J[:, 3:, 3:6].ravel(), J[:, 3:, 9:12].ravel()])
        out["J_zeros"] = 0.0 if not zeros.any() else np.inf
    return out


def merge_ratios(worst, ratios):
    for k, v in ratios.items():
        worst[k] = max(worst.get(k, 0.0), v)
    return worst


def fp64_eval(g):
    """This module's own formulas evaluated in FP64: the vectorised statement whose rounding K_FACTOR is measured with."""
    res = residuals(g, dtype=np.float64)
    return dict(rel_r=res["rel_r"], fix_r=res["fix_r"], cost=float(res["cost"]), rel_J=None)


def check_first_costs(g, pose_out, cost_history, what=""):
    """cost_history[0] against the model's cost of the start and cost_history[1] against the model's cost of the point the call
    RETURNED (its accepted candidate), each within K_FACTOR u cost_scale. The second is not compared with the cost of the model's own
    candidate: the two candidates differ by the step's rounding (bounded separately, STEP_FLOOR), and the cost moves with it by
    gradient x difference, which is no rounding of the evaluation — the oracle itself is 400 x the bound K_FACTOR u cost_scale away from the
    model's candidate cost on n1 (8.1 x on n2, 2.4 x on n3, 7.4 x on huber; these candidates' costs are nearly zero or steep), and
    within 0.006 x the bound of the model's cost of the oracle's own candidate on every case."""
    for k, pose in ((0, None), (1, pose_out)):
        ref = residuals(g, pose)
        r = _ratio(cost_history[k], ref["cost"], ref["cost_scale"])
        assert r <= K_FACTOR, "%s cost_history[%d] is %.3g u cost_scale from the model's (bound %g)" % (what, k, r, K_FACTOR)


def _fmt(d):
    return "   ".join("%s %s" % (k, ("(%.3g, %.3g)" % tuple(v)) if isinstance(v, tuple) else "%.3g" % v) for k, v in d.items())


__doc__ = __doc__ % dict(KM=_fmt(K_MEASURED), K=K_FACTOR, SF=_fmt(STEP_FLOOR), LF=_fmt(LOOP_FLOOR))
