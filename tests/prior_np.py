"""The new prior of a marginalisation in extended precision — the reference tests/test_prior_reference.py (CPU) and
tests/test_gpu_prior.py (device) hold J0, r0 and the block table against — and the windows that reach every size at which
csrc/gfbe_marg.hip takes another path. No HIP; the same role as normal_equations_np.py and preint_np.py.

Model (reference_prior). The factors of the marginalisation set come from the oracle as per-factor blocks
(gfo_eval_factors, robustified; the GNSS blocks from gfo_gnss_eval) plus the incoming prior as one more residual block
(J0, prior_r). Their J^T J and J^T r are summed in numpy.longdouble into the un-reduced A, b (placement: numpy_marginalize_old of
tests/test_oracle_solver.py, extended to a prior with arbitrary blocks, to MARGIN_SECOND_NEW and to the GNSS blocks). The dropped
set is eliminated in longdouble: the frame-0 landmarks by scalar division (their block is diagonal), then the dense dropped dims
(15; 20 with GNSS; the 6 of pose 9 for MARGIN_SECOND_NEW) by a hand-written Cholesky. The reference takes a pseudo-inverse
thresholded at marg_eps instead: build_case asserts in FP64 that every eigenvalue of the dropped block exceeds marg_eps by a
factor >= 1e3, so inverse and pseudo-inverse coincide. Outputs: A_ref, b_ref, a_scale = max |A|, b_scale = max |b| of the
un-reduced system, the kept block table with the address shift applied, x0.

Reaching every size. The prior is an input of the window and the marginalisation keeps every block the incoming prior lists, so
a case takes the (regularised, see below) prior of a solved first window and grows it by extra blocks (grow_prior): per extra block a row block
[0.3 N(0, 1) | 3 I] under J0, r0 ~ N(0, 1), x0 = the window's own value of the block (so the block has not moved), and the
entries of the block table. n_out = base + sum of the extra blocks' local sizes, where base is what the plain prior gives in
the second window: 86 when a frame-0 landmark reaches pose 10, 80 when none does.

Cases (CASES; n_out asserted per case by tests/test_prior_reference.py). MARGIN_OLD:
  85 (base 80 + plane_R + plane_Z), 86 (the shipped block list, nothing added), 87   around the shipped size
  88 | 89                                                                            k_marg_ldlt<4> | <6>
  90 | 91                                                                            MARG_LDS_N: in-LDS divide & conquer | global QL
  132 | 133                                                                          k_marg_ldlt<6> | <8>
  176 | 177                                                                          LDLT_MAX_N: above it the eigen path whatever marg_sqrt
  gnss (first window with GNSS, 20 dense dropped dims), nowheel (first window without wheel: the smallest prior, 76)
MARGIN_SECOND_NEW: input 91 -> 85, input 96 -> 90. Every size of the list is reached; 177 uses all 32 block slots of the incoming and of the new prior.
Sizes that are no multiple of four (ragged 4 x 4 tiles of the divide & conquer's M8, odd leaves of its tear): 85, 86, 87, 89,
90, 91, 133, 177.

Discrete results. The number of rows the square root keeps depends on marg_eps, so a case is only admitted when the decision is
not a matter of rounding: no eigenvalue of A_ref (FP64 eigvalsh of the rounded model) and no pivot of numpy_pivoted_ldlt_sqrt
lies in [marg_eps / G, marg_eps G]. G follows from the rounding of A': the device and the oracle form A' in FP64 from numbers of
size a_scale, so an eigenvalue moves by up to ~64 u a_scale; G - 1 >= 64 u a_scale / marg_eps. The un-reduced information of
these windows reaches a_scale = 6.7e11 (the bias random walk of the inertial factor), asserted <= A_SCALE_MAX = 1e12:
G - 1 >= 7.1e5, G = 2^20, the excluded band is [9.5e-15, 1.05e-2].

What that condition means for the windows. 64 u a_scale = 5e-3 is far above marg_eps = 1e-8: an eigenvalue BELOW the band is
moved across the threshold by the rounding of A' just as one inside it, so only a prior whose spectrum lies entirely above the
band has a well-defined number of rows. The marginal of a plain first window is not of that kind, whatever the seed: it has
the four exact null directions of the gauge (position, yaw) and a ladder of weak directions (old_86 without regularisation:
eigenvalues of A_ref 7e-13, 8e-11, 6e-10, 1e-8, 6e-8, 3e-7, 9e-7, 1e-6, 5e-6, 1.4e-4, ...), and the FP64 constructions
disagree about it among themselves (rows kept: model 79, oracle eigen 77, oracle LDL^T 76, numpy 77). The cases therefore take
a REGULARISED prior as input: the solved first window's J0^T J0 + C_REG I (C_REG = 1), Cholesky-factored, with r0 such that
J0^T r0 is unchanged; first windows (gnss, nowheel) get the prior sqrt(C_REG) I on exactly the blocks their marginalisation set
touches anyway (n_out unchanged). Marginalisation is monotone, so every eigenvalue of A' along the regularised blocks is
>= C_REG, and every case has full rank n in both modes — which the CPU test asserts through the gap condition. The
thresholding of a rank-deficient prior at marg_eps is NOT pinned by these cases (it cannot be, exactly); it stays with
tests/test_gpu_parity.py::test_prior_square_root_modes and the check_prior calls against the oracle.
"""
import numpy as np

from _gfbe_import import gf
import normal_equations_np as ne

abi, synth = gf.abi, gf.synth

LD = np.longdouble
U = 2.0 ** -53
MARG_EPS = 1e-8
DROP_MARGIN = 1e3                 # every eigenvalue of the dropped block > DROP_MARGIN * marg_eps
A_SCALE_MAX = 1e12
G = 2.0 ** 20                     # >= 1 + 64 u A_SCALE_MAX / marg_eps = 7.1e5, rounded up to a power of two
C_REG = 1.0                       # the regulariser of the incoming prior (see the module docstring)
assert G - 1 >= 64 * U * A_SCALE_MAX / MARG_EPS
W = abi.WINDOW_SIZE
require_extended_precision = ne.require_extended_precision


# ---------------------------------------------------------------------------------------------------------------- FP64 square roots
def numpy_pivoted_ldlt_sqrt(Ap, bp, eps=1e-8, pivots=None):
    """Independent statement of the product's default square root: diagonally pivoted LDL^T with pivots > eps,
    written as successive Schur complements on index sets (no in-place elimination loops like the C++ ones). pivots: a list that
    receives every pivot looked at, the first rejected one included."""
    n = len(bp)
    M, rhs = 0.5 * (Ap + Ap.T), bp.copy()
    left = list(range(n))
    J0, r0 = np.zeros((n, n)), np.zeros(n)
    for k in range(n):
        dg = np.array([M[i, i] for i in left])
        p = left[int(np.argmax(dg))]
        if pivots is not None:
            pivots.append(float(M[p, p]))
        if not M[p, p] > eps:
            break
        d = M[p, p]
        col = np.zeros(n)
        col[left] = M[left, p] / d
        J0[k] = np.sqrt(d) * col
        r0[k] = rhs[p] / np.sqrt(d)
        left.remove(p)
        M[np.ix_(left, left)] -= d * np.outer(col[left], col[left])
        rhs[left] -= col[left] * (r0[k] * np.sqrt(d))
    return J0, r0


def numpy_eigen_sqrt(Ap, bp, eps=1e-8):
    """The reference's square root (marginalization_factor.cpp:281-302): A' = V S V^T, S thresholded at eps, rows by ascending
    eigenvalue: J0 = sqrt(S) V^T, r0 = sqrt(S^-1) V^T b'."""
    w, V = np.linalg.eigh(0.5 * (Ap + Ap.T))
    keep = w > eps
    S, Sinv = np.where(keep, w, 0.0), np.where(keep, 1.0 / np.where(keep, w, 1.0), 0.0)
    return np.sqrt(S)[:, None] * V.T, np.sqrt(Sinv) * (V.T @ bp)


# ---------------------------------------------------------------------------------------------------------------- the marginalisation set
def gnss_rows(oracle, snap, only_frame0=False):
    """[(r, J, [(block id, columns)])] of the GNSS residual blocks from the stand-alone evaluator (tests/test_gnss_solve_oracle.py
    pins this wiring against the oracle's linearisation)."""
    from test_gnss_solve_oracle import gnss_rows as rows
    return rows(oracle, snap, only_frame0)


def marg_rows(oracle, snap, flag):
    """The residual blocks of the marginalisation set as (r, J, [(block, local columns)]); a landmark is the block ("l", index)."""
    ev = oracle.eval_factors(snap, robustify=True)
    rows = []
    if flag == abi.MARGIN_OLD:
        for k, i in enumerate(np.asarray(snap.get("imu_frame", []), int)):
            if i == 0:
                rows.append((ev["imu_r"][k], ev["imu_J"][k], [(0, range(6)), (abi.BLK_SB0, range(9)), (1, range(6)), (abi.BLK_SB0 + 1, range(9))]))
        for k, i in enumerate(np.asarray(snap.get("wheel_frame", []), int)):
            if i == 0:
                rows.append((ev["wheel_r"][k], ev["wheel_J"][k], [(0, range(6)), (1, range(6)), (abi.BLK_EX_WHEEL, range(6)), (abi.BLK_SX, [0]), (abi.BLK_SY, [0]),
                                                                  (abi.BLK_SW, [0]), (abi.BLK_TD_WHEEL, [0])]))
        for k in np.where(np.asarray(snap["vis_imu_i"]) == 0)[0]:
            j, l = int(snap["vis_imu_j"][k]), int(snap["vis_feature_index"][k])
            rows.append((ev["vis_r"][k], ev["vis_J"][k], [(0, range(6)), (j, range(6)), (abi.BLK_EX_CAM, range(6)), (("l", l), [0]), (abi.BLK_TD, [0])]))
        if snap.get("gnss") is not None and snap["gnss"].get("ready", 1):
            rows += gnss_rows(oracle, snap, only_frame0=True)
    pr = snap.get("prior")
    if pr is not None and pr.get("valid", 1) and pr["n"] > 0:
        n = int(pr["n"])
        blocks = [(int(pr["block_id"][q]), range(abi.block_local_size(int(pr["block_id"][q])))) for q in np.argsort(pr["block_idx"])]
        rows.append((ev["prior_r"], np.asarray(pr["J0"]).reshape(n, n), blocks))
    return rows


def shifted_id(flag, b):
    """The address shift of the kept blocks (estimator.cpp:3561-3590, 3644-3687)."""
    is_dt, is_ddt = abi.BLK_RCV_DT0 <= b < abi.BLK_RCV_DDT0, b >= abi.BLK_RCV_DDT0
    if flag == abi.MARGIN_OLD:
        return b - 1 if (b < abi.BLK_EX_CAM or is_ddt) else (b - 4 if is_dt else b)
    if b in (abi.BLK_POSE0 + W, abi.BLK_SB0 + W, abi.BLK_RCV_DDT0 + W):
        return b - 1
    return b - 4 if (is_dt and b >= abi.BLK_RCV_DT0 + 4 * W) else b


def block_value(snap, b):
    """The parameter block b of the window's state (global size)."""
    gs = snap.get("gnss_state") or {}
    if b < abi.BLK_SB0:
        return np.asarray(snap["pose"], float)[b]
    if b < abi.BLK_EX_CAM:
        return np.asarray(snap["speed_bias"], float)[b - abi.BLK_SB0]
    if b >= abi.BLK_RCV_DDT0:
        return np.asarray(gs.get("rcv_ddt", np.zeros(abi.NFRAMES)), float)[b - abi.BLK_RCV_DDT0:b - abi.BLK_RCV_DDT0 + 1]
    if b >= abi.BLK_RCV_DT0:
        return np.asarray(gs.get("rcv_dt", np.zeros((abi.NFRAMES, 4))), float).ravel()[b - abi.BLK_RCV_DT0:b - abi.BLK_RCV_DT0 + 1]
    return np.atleast_1d(np.asarray({abi.BLK_EX_CAM: snap["ex_pose"], abi.BLK_EX_WHEEL: snap["ex_pose_wheel"], abi.BLK_SX: snap["ix_wheel"][0],
                                     abi.BLK_SY: snap["ix_wheel"][1], abi.BLK_SW: snap["ix_wheel"][2], abi.BLK_TD: snap["td"], abi.BLK_TD_WHEEL: snap["td_wheel"],
                                     abi.BLK_PLANE_R: snap.get("plane_R", [0.0, 0.0, 0.0, 1.0]), abi.BLK_PLANE_Z: snap.get("plane_Z", 0.0),
                                     abi.BLK_ANC_ECEF: gs.get("anc_ecef", np.zeros(3)), abi.BLK_YAW_ENU: gs.get("yaw_enu_local", 0.0)}[b], float))


def cholesky_ld(M):
    """Lower Cholesky factor of a small symmetric positive definite matrix, in the dtype of M (no LAPACK: longdouble has none)."""
    n = M.shape[0]
    L = np.zeros_like(M)
    for j in range(n):
        d = M[j, j] - (L[j, :j] * L[j, :j]).sum()
        assert d > 0, "dropped block is not positive definite"
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def forward_solve(L, B):
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def reduce_system(rows, snap, flag, dtype=LD):
    """Un-reduced A, b of the marginalisation set from its residual blocks, the dropped set eliminated, all in `dtype`. Returns a
    dict: A, b (n x n, n: the reduced system in the kept blocks' order), a_scale, b_scale, keep (old ids), the new block table
    block_id / block_size / block_idx, x0, n, and dropped_min_eig (FP64, smallest eigenvalue of the whole dropped block)."""
    touched = set()
    for _, _, blocks in rows:
        touched |= {b for b, _ in blocks if not isinstance(b, tuple)}
    lms = sorted({b[1] for _, _, blocks in rows for b, _ in blocks if isinstance(b, tuple)})
    if flag == abi.MARGIN_OLD:
        gn = snap.get("gnss") is not None and snap["gnss"].get("ready", 1)
        drop = [b for b in sorted(touched) if b in (0, abi.BLK_SB0) or (gn and (abi.BLK_RCV_DT0 <= b < abi.BLK_RCV_DT0 + 4 or b == abi.BLK_RCV_DDT0))]
    else:
        drop = [abi.BLK_POSE0 + W - 1]
        assert drop[0] in touched
    keep = [b for b in sorted(touched) if b not in drop]
    idx, pos = {}, 0
    for b in drop:
        idx[b] = pos
        pos += abi.block_local_size(b)
    md = pos
    for l in lms:
        idx[("l", l)] = pos
        pos += 1
    m = pos
    for b in keep:
        idx[b] = pos
        pos += abi.block_local_size(b)
    A, bb = np.zeros((pos, pos), dtype), np.zeros(pos, dtype)
    for r, J, blocks in rows:
        cols = np.concatenate([idx[b] + np.asarray(list(c)) for b, c in blocks])
        J, r = np.asarray(J, dtype), np.asarray(r, dtype)
        A[np.ix_(cols, cols)] += J.T @ J
        bb[cols] += J.T @ r
    a_scale, b_scale = float(np.abs(A).max()), float(np.abs(bb).max())
    Amm = np.asarray(A[:m, :m], float)
    dropped_min_eig = float(np.linalg.eigvalsh(0.5 * (Amm + Amm.T)).min())
    # the landmarks: a diagonal block, eliminated one by one
    Dl = A[md:m, md:m]
    assert not (Dl - np.diag(np.diag(Dl))).any(), "the landmark block is not diagonal"
    rest = np.r_[0:md, m:pos]
    S, s = A[np.ix_(rest, rest)].copy(), bb[rest].copy()
    for p in range(md, m):
        a, d = A[rest, p], A[p, p]
        S -= np.outer(a, a) / d
        s -= a * (bb[p] / d)
    # the dense dropped dims
    L = cholesky_ld(S[:md, :md])
    Y, z = forward_solve(L, S[:md, md:]), forward_solve(L, s[:md])
    Ap, bp = S[md:, md:] - Y.T @ Y, s[md:] - Y.T @ z
    sizes = [abi.block_global_size(b) for b in keep]
    lidx = np.r_[0, np.cumsum([abi.block_local_size(b) for b in keep])]
    return dict(A=Ap, b=bp, a_scale=a_scale, b_scale=b_scale, keep=keep, n=int(lidx[-1]), block_id=[shifted_id(flag, b) for b in keep], block_size=sizes,
                block_idx=lidx[:-1].tolist(), x0=np.concatenate([block_value(snap, b) for b in keep]), dropped_min_eig=dropped_min_eig, n_dropped=m)


def reference_prior(oracle, snap, flag):
    """The extended-precision model of the new prior of `snap` under `flag`, with the discrete counts of both square roots
    (FP64 on the rounded model) and the quantities of the gap condition."""
    ref = reduce_system(marg_rows(oracle, snap, flag), snap, flag, LD)
    A64, b64 = np.asarray(ref["A"], float), np.asarray(ref["b"], float)
    A64 = 0.5 * (A64 + A64.T)
    ref["eig"] = np.linalg.eigvalsh(A64)
    ref["pivots"] = []
    numpy_pivoted_ldlt_sqrt(A64, b64, MARG_EPS, ref["pivots"])
    ref["rank"] = {0: int((ref["eig"] > MARG_EPS).sum()), 1: int((np.asarray(ref["pivots"]) > MARG_EPS).sum())}
    return ref


def fp64_prior(oracle, snap, flag, mode):
    """The same construction in plain FP64 numpy: sums, Schur complement, then eigh with threshold (mode 0) or the pivoted LDL^T."""
    red = reduce_system(marg_rows(oracle, snap, flag), snap, flag, np.float64)
    J0, r0 = (numpy_eigen_sqrt if mode == 0 else numpy_pivoted_ldlt_sqrt)(red["A"], red["b"], MARG_EPS)
    return dict(valid=1, n=red["n"], block_id=np.array(red["block_id"]), block_size=np.array(red["block_size"]), block_idx=np.array(red["block_idx"]),
                x0=red["x0"], J0=J0, r0=r0)


def gap_violations(ref):
    """Eigenvalues of A_ref and LDL^T pivots inside [marg_eps / G, marg_eps G]: the discrete results would be a matter of rounding."""
    lo, hi = MARG_EPS / G, MARG_EPS * G
    return [float(x) for x in ref["eig"] if lo <= x <= hi], [float(x) for x in ref["pivots"] if lo <= x <= hi]


# ---------------------------------------------------------------------------------------------------------------- the checker
def check_prior(prior, ref, mode, label="", x0=None):
    """A prior (dict of abi.PriorHolder.to_dict) against the model. Exact: the block table, x0 (against `x0` when given: the device's
    own linearisation point has been compared by the caller), the number of non-zero rows, zero rows where S = 0, ascending S in
    eigen mode. Returns the ratios in units of u: rA, rb, and ro (eigen mode)."""
    n = ref["n"]
    assert prior is not None and prior["valid"] == 1 and prior["n"] == n, (label, prior and prior["n"], n)
    for k in ("block_id", "block_size", "block_idx"):
        assert np.asarray(prior[k]).tolist() == list(ref[k]), (label, k, np.asarray(prior[k]).tolist(), list(ref[k]))
    want_x0 = ref["x0"] if x0 is None else x0
    assert np.array_equal(prior["x0"], want_x0), (label, "x0", float(np.abs(prior["x0"] - want_x0).max()))
    J0, r0 = np.asarray(prior["J0"], float), np.asarray(prior["r0"], float)
    assert np.isfinite(J0).all() and np.isfinite(r0).all(), label
    nz = np.abs(J0).sum(axis=1) > 0
    assert int(nz.sum()) == ref["rank"][mode], (label, "rows kept", int(nz.sum()), ref["rank"][mode])
    assert not r0[~nz].any(), (label, "r0 of a dropped row")
    Jl, rl = np.asarray(J0, LD), np.asarray(r0, LD)
    out = {}
    errA = np.maximum(np.abs(Jl.T @ Jl - ref["A"]) - LD(MARG_EPS), 0)
    out["rA"] = float(errA.max() / (LD(U) * LD(ref["a_scale"])))
    # P: the projector on the row space of the square root under test (orthonormal basis by Householder QR of the kept rows)
    Q, _ = np.linalg.qr(J0[nz].T)
    Pb = np.asarray(Q, LD) @ (np.asarray(Q, LD).T @ ref["b"])
    out["rb"] = float(np.abs(Jl.T @ rl - Pb).max() / (LD(U) * LD(max(ref["b_scale"], 1e-2 * ref["a_scale"]))))
    if mode == 0:
        GG = np.asarray(Jl @ Jl.T, float)
        dg = np.diag(GG)
        out["ro"] = float(np.abs(GG - np.diag(dg)).max() / dg.max() / U)
        assert (np.diff(dg) >= -8 * U * dg[1:]).all(), (label, "S not ascending")
        assert not nz[:n - int(nz.sum())].any(), (label, "zero rows are not the first ones")
    else:
        assert nz[:int(nz.sum())].all(), (label, "the kept rows are not the first ones")
    return out


def pow2_at_least(x):
    return float(2.0 ** np.ceil(np.log2(x)))


# Largest ratio per quantity over every case, both square roots, the oracle's gfo_marginalize and the FP64 numpy statement, measured
# by tests/test_prior_reference.py (which asserts them so that they cannot drift); in units of u, see check_prior
R_CPU = dict(rA=80.0, rb=220.0, ro=8.0)            # measured 77.35, 213.7, 7.696: rounded up
K = {q: pow2_at_least(4.0 * v) for q, v in R_CPU.items()}      # the device bound: smallest power of two >= 4 r_cpu


# ---------------------------------------------------------------------------------------------------------------- the cases
EXTRA = {      # the extra blocks per case: ids in the numbering of the window that is marginalised
    0: [],
    1: [abi.BLK_YAW_ENU],
    2: [abi.BLK_YAW_ENU, abi.BLK_PLANE_Z],
    3: [abi.BLK_ANC_ECEF],
    4: [abi.BLK_PLANE_R],
    5: [abi.BLK_PLANE_R, abi.BLK_PLANE_Z],
    10: [abi.BLK_SB0 + 2, abi.BLK_YAW_ENU],
    46: [abi.BLK_SB0 + 2 + k for k in range(5)] + [abi.BLK_YAW_ENU],
    47: [abi.BLK_SB0 + 2 + k for k in range(5)] + [abi.BLK_YAW_ENU, abi.BLK_PLANE_Z],
    90: [abi.BLK_SB0 + 2 + k for k in range(9)] + [abi.BLK_PLANE_R, abi.BLK_PLANE_Z, abi.BLK_ANC_ECEF, abi.BLK_YAW_ENU],
    91: [abi.BLK_SB0 + 2 + k for k in range(9)] + [abi.BLK_PLANE_R, abi.BLK_PLANE_Z, abi.BLK_ANC_ECEF, abi.BLK_YAW_ENU, abi.BLK_RCV_DDT0 + 5],
}
SEED_86, SEED_80 = 45, 36          # scenarios whose second window keeps 86 / 80 dims of the plain prior (a frame-0 landmark reaches pose 10 / none does)
# name: (kind, scenario seed, base of the plain prior, extra dims, margin flag, n_out)
CASES = {
    "old_85": ("grown", SEED_80, 80, 5, abi.MARGIN_OLD, 85),
    "old_86": ("grown", SEED_86, 86, 0, abi.MARGIN_OLD, 86),
    "old_87": ("grown", SEED_86, 86, 1, abi.MARGIN_OLD, 87),
    "old_88": ("grown", SEED_86, 86, 2, abi.MARGIN_OLD, 88),
    "old_89": ("grown", SEED_86, 86, 3, abi.MARGIN_OLD, 89),
    "old_90": ("grown", SEED_86, 86, 4, abi.MARGIN_OLD, 90),
    "old_91": ("grown", SEED_86, 86, 5, abi.MARGIN_OLD, 91),
    "old_132": ("grown", SEED_86, 86, 46, abi.MARGIN_OLD, 132),
    "old_133": ("grown", SEED_86, 86, 47, abi.MARGIN_OLD, 133),
    "old_176": ("grown", SEED_86, 86, 90, abi.MARGIN_OLD, 176),
    "old_177": ("grown", SEED_86, 86, 91, abi.MARGIN_OLD, 177),
    "gnss": ("gnss", 87, None, 0, abi.MARGIN_OLD, 71),
    "nowheel": ("nowheel", 41, None, 0, abi.MARGIN_OLD, 76),
    "new_85": ("grown", SEED_86, 86, 5, abi.MARGIN_SECOND_NEW, 85),
    "new_90": ("grown", SEED_86, 86, 10, abi.MARGIN_SECOND_NEW, 90),
}
N_LANDMARKS = 80


def grow_prior(prior, snap, extra, seed):
    """`prior` with one more block per id in `extra`: rows [0.3 N(0, 1) | 3 I] under J0, r0 ~ N(0, 1), x0 = the block's value in snap."""
    rng = np.random.default_rng(seed)
    p = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in prior.items()}
    for b in extra:
        assert b not in p["block_id"].tolist()
        n, ls = int(p["n"]), abi.block_local_size(b)
        J = np.zeros((n + ls, n + ls))
        J[:n, :n] = p["J0"]
        J[n:, :n] = 0.3 * rng.normal(0, 1, (ls, n))
        J[n:, n:] = 3.0 * np.eye(ls)
        p["J0"], p["r0"] = J, np.r_[p["r0"], rng.normal(0, 1, ls)]
        p["x0"] = np.r_[p["x0"], block_value(snap, b)]
        p["block_id"], p["block_size"] = np.r_[p["block_id"], b].astype(np.int32), np.r_[p["block_size"], abi.block_global_size(b)].astype(np.int32)
        p["block_idx"] = np.r_[p["block_idx"], n].astype(np.int32)
        p["n"] = n + ls
    return p


def regularised(prior):
    """The prior with the information J0^T J0 + C_REG I and an unchanged J0^T r0, as an upper-triangular square root."""
    p = dict(prior)
    J0, r0 = np.asarray(prior["J0"], float), np.asarray(prior["r0"], float)
    R = np.linalg.cholesky(J0.T @ J0 + C_REG * np.eye(len(r0))).T
    p["J0"], p["r0"] = R, np.linalg.solve(R.T, J0.T @ r0)
    return p


def identity_prior(oracle, snap, flag, seed):
    """sqrt(C_REG) I, r0 ~ 0.1 N(0, 1), on the blocks the marginalisation set of a window without prior touches anyway."""
    touched = set()
    for _, _, blocks in marg_rows(oracle, dict(snap, prior=None), flag):
        touched |= {b for b, _ in blocks if not isinstance(b, tuple)}
    ids = sorted(touched)
    assert len(ids) <= abi.MAX_PRIOR_BLOCKS
    lidx = np.r_[0, np.cumsum([abi.block_local_size(b) for b in ids])]
    n = int(lidx[-1])
    return dict(valid=1, n=n, block_id=np.array(ids, np.int32), block_size=np.array([abi.block_global_size(b) for b in ids], np.int32),
                block_idx=lidx[:-1].astype(np.int32), x0=np.concatenate([block_value(snap, b) for b in ids]), J0=np.sqrt(C_REG) * np.eye(n),
                r0=0.1 * np.random.default_rng(seed).normal(0, 1, n))


def host_marg_bound(snap):
    """The size the host reserves for a window's new prior, and what marg_nmax is the batch maximum of (prior_out_bound in
    csrc/gfbe_upload.h, both margin flags): the incoming prior's n, or the local sizes of every block the prior lists or a factor of
    the MARGIN_OLD set can touch, poses 0 and speed-bias 0 left out. Windows without the ground-plane factor."""
    pr = snap.get("prior")
    pr = pr if (pr is not None and pr.get("valid", 1) and pr["n"] > 0) else None
    touched = {int(b) for b in pr["block_id"]} if pr else set()
    if 0 in np.asarray(snap.get("imu_frame", []), int):
        touched |= {0, abi.BLK_SB0, 1, abi.BLK_SB0 + 1}
    if 0 in np.asarray(snap.get("wheel_frame", []), int):
        touched |= {0, 1, abi.BLK_EX_WHEEL, abi.BLK_SX, abi.BLK_SY, abi.BLK_SW, abi.BLK_TD_WHEEL}
    if snap.get("gnss") is not None and snap["gnss"].get("ready", 1):
        touched |= {0, abi.BLK_SB0, 1, abi.BLK_SB0 + 1, abi.BLK_YAW_ENU, abi.BLK_ANC_ECEF, abi.BLK_RCV_DDT0 + 1} | {abi.BLK_RCV_DT0 + 4 + k for k in range(4)}
    assert snap.get("plane") is None
    for j in set(np.asarray(snap["vis_imu_j"])[np.asarray(snap["vis_imu_i"]) == 0].tolist()):
        touched |= {0, int(j), abi.BLK_EX_CAM, abi.BLK_TD}
    old = sum(abi.block_local_size(b) for b in touched if b not in (0, abi.BLK_SB0))
    return max(min(old, abi.DENSE_DIM), int(pr["n"]) if pr else 0)


# the MARGIN_OLD cases whose host bound stays within k_marg_ldlt<4>'s 88 dims: a batch of these alone keeps <6> and <8> unlaunched
# (old_85, gnss and nowheel have a smaller new prior but a 91-dim incoming one)
WITHIN_88 = ["old_86", "old_87", "old_88"]


_cache = {}


def build_case(name, oracle):
    """(window, margin flag) of a case; deterministic, cached per process."""
    if name in _cache:
        return _cache[name]
    kind, seed, base, extra, flag, n_out = CASES[name]
    if kind == "grown":
        key = ("second", seed)
        if key not in _cache:
            scn = synth.Scenario(seed=seed, n_landmarks=N_LANDMARKS, use_wheel=True)
            res = oracle.solve(scn.window(0), abi.MARGIN_OLD)
            assert res["prior"]["n"] == 86
            _cache[key] = (scn, res, regularised(res["prior"]))
        scn, res, reg = _cache[key]
        snap = scn.window(1, state=synth.shift_state_for_next_window(scn, res["state"], 1), prior=None)
        snap["prior"] = grow_prior(reg, snap, EXTRA[extra], 9000 + extra)
    else:
        if kind == "gnss":
            import gnss_window_cases as gw
            _, _, snap = gw.gnss_window(seed=seed, L=N_LANDMARKS, n_per_frame=6)
        else:
            snap = synth.Scenario(seed=seed, n_landmarks=N_LANDMARKS, use_wheel=False).window(0)
        snap["prior"] = identity_prior(oracle, snap, flag, 9500 + seed)
    _cache[name] = (snap, flag)
    return _cache[name]


_ref_cache = {}


def case_reference(name, oracle):
    """(window, flag, model) of a case; computed once per process and left unchanged."""
    if name not in _ref_cache:
        snap, flag = build_case(name, oracle)
        _ref_cache[name] = (snap, flag, reference_prior(oracle, snap, flag))
    return _ref_cache[name]
