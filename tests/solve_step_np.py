"""Checker of the reduced-system solve (csrc/gfbe_solve.hip: k_solve, k_solve_chain, k_solve_chain_tw, k_solve_chain_wide,
k_solve_big) by its BACKWARD error, in numpy.longdouble, on the system the device itself assembled. CPU only;
tests/test_solve_step_reference.py measures the constants on a plain FP64 solve and shows what the checker sees,
tests/test_gpu_solve_step.py applies it to the device.

The restated system (the one the four solve bodies build before they factorise), on the active dims, from H, g, E, eg, s and mu:

    Ht = s H s     D2 = clamp(s^2 H_aa, GF_MIN_DIAG, GF_MAX_DIAG)     Et = s E s  (zero outside the 73 visual dims)
    S  = Ht + mu D2 - Et                                              rhs = s g - s eg

mu is known a priori, GF_MIN_MU GF_MU_INC^k with k the number of injected retries. The active dims are those with H[a, a] != 0:
the assembly removes constant dims and dims no factor touches from H (tests/test_gpu_normal_equations.py holds those entries to
exactly 0.0), and every active dim has a positive diagonal.

Checks (each returns error / bound; u = 2^-53):
  y     normwise backward error (Rigal-Gaches) with ABSOLUTE sums in the denominator — Ht - Et cancels for well-observed poses and the
        device forms S in FP64 from both terms —
            eta = |S y - rhs|_inf / ( | |Ht| + mu D2 + |Et| |_inf |y|_inf + | |s g| + |s eg| |_inf )  <=  K_Y u
        and y exactly 0.0 on inactive dims.
  s     first iteration: 1 / (1 + sqrt(H_aa)), three correctly rounded operations: relative error <= 4 u; exactly 1.0 when inactive.
  v     (s g) / D2 from the device's own s, four roundings and the clamp: relative error <= 8 u; exactly 0.0 where g is 0.0.
        (libgfbe.so is built with -O3 -ffp-contract=off and without -ffast-math or any relaxed division / square root flag —
        backend.py: build_native; -munsafe-fp-atomics concerns atomics only —, so hipcc emits the correctly rounded FP64 division and
        square root sequences, no product is fused into a sum, and the two counts stand.)
  G2 = sum gt^2 / D2, N2 = sum D2 y^2, gy = sum gt y: any summation order of m terms with three roundings each stays within
        (m + 3) u sum |term|, m = ND. The references are formed in longdouble from the device's own s, v, y.
  vHv, vHy, yHy against v^T Ht v, v^T Ht y, y^T Ht y in longdouble. The device forms them by subtraction,
        vHv = vSv - mu vDv + vEv      vHy = v.rhs - mu vDy + vEy      yHy = |z|^2 - mu N2 + yEy,
        so the bound is K_S u A_X + B_X with A_X the sum of the absolute values of every term of the device's formula,
            A_vHv = |v|^T M |v| + mu vDv + |sv|^T |E| |sv|                      M = |Ht| + mu D2 + |Et|
            A_vHy = |v|^T M |y| + |v|^T (|s g| + |s eg|) + mu |v|^T D2 |y| + |sv|^T |E| |sy|
            A_yHy = |y|^T M |y| + mu N2 + |sy|^T |E| |sy|
        and B_X the part that is exact only for an exact y: with r = S y - rhs, |r|_inf <= K_Y u den (den: the denominator of eta),
        y^T S y - y^T rhs = y^T r, so B_yHy = K_Y u den |y|_1, B_vHy = K_Y u den |v|_1, B_vHv = 0.

The constants are measured, not chosen (test_solve_step_reference.py asserts them so that they cannot drift): ETA_CPU is the worst
eta / u over every case of tests/solve_step_cases.py of a plain FP64 solve of the same S (numpy.linalg.cholesky and two triangular
solves, judged by the same longdouble residual), K_Y = 16 ETA_CPU rounded up to a power of two; S_CPU the worst scalar ratio
(|X - X_ref| - B_X) / (u A_X) of the three formulas restated in FP64 numpy in the device's term grouping, K_S = 16 S_CPU rounded up,
with a floor of ND + 3. The margin of 16 is for what the device does differently from LAPACK: 16 x 16 tiles multiplied by explicitly
inverted triangular factors (error grows with the tile's own condition), matrix-core accumulation order, a Newton-refined v_rsq_f64."""
import numpy as np

import normal_equations_np as ne

LD = np.longdouble
U = ne.U
ND, NV = ne.ND, ne.NV
# gfbe_devutil.h: GF_MIN_MU, GF_MU_INC, GF_MIN_DIAG, GF_MAX_DIAG (the first and the last two are normal_equations_np's)
GF_MIN_MU, GF_MU_INC, GF_MIN_DIAG, GF_MAX_DIAG = ne.GF_MIN_MU, 10.0, ne.GF_MIN_DIAG, ne.GF_MAX_DIAG
TB = 16                                         # gfbe_solve.hip: tile side

# measured by tests/test_solve_step_reference.py over every case (which asserts them): plain FP64 solve, in units of u
ETA_CPU = 1.71
S_CPU = dict(vHv=3.06, vHy=3.06, yHy=3.06)
K_MARGIN = 16.0


def _pow2_up(x):
    return float(2.0 ** np.ceil(np.log2(x)))


K_Y = _pow2_up(K_MARGIN * ETA_CPU)
K_S = max(_pow2_up(K_MARGIN * max(S_CPU.values())), float(ND + 3))
S_TOL, V_TOL = 4.0, 8.0                          # relative error of s and v in units of u
SUM_TOL = float(ND + 3)                          # positive sums, in units of u sum |term|


def mu_of(retries=0):
    """GF_MIN_MU GF_MU_INC^retries as the retry loop forms it (mu *= GF_MU_INC): the device must report these bits."""
    mu = GF_MIN_MU
    for _ in range(retries):
        mu *= GF_MU_INC
    return mu


def active_mask(H):
    return np.diag(np.asarray(H, float)) != 0.0


def symmetrise(H):
    """The device holds the lower triangle."""
    L = np.tril(np.asarray(H))
    return L + np.tril(L, -1).T


def embed_E(E, eg, dtype):
    """E [73, 73], eg [73] -> ND x ND, ND (zero outside the visual dims)."""
    Ef, egf = np.zeros((ND, ND), dtype), np.zeros(ND, dtype)
    Ef[:NV, :NV] = np.asarray(E)[:NV, :NV]
    egf[:NV] = np.asarray(eg)[:NV]
    return Ef, egf


def first_scaling(H, act, dtype=float):
    """s = 1 / (1 + sqrt(H_aa)) on the active dims, 1 elsewhere."""
    d = np.asarray(np.diag(H), dtype)
    one = d.dtype.type(1)
    return np.where(act, one / (one + np.sqrt(np.where(act, d, one))), one)


def restate(H, g, E, eg, s, mu, act=None, dtype=LD):
    """The reduced system in `dtype` on ALL ND dims (rows / columns of inactive dims zero): dict with Ht, D2, Et, S, gt, seg, rhs, M, act.
    H: full symmetric ND x ND. E, eg: 73-sized or ND-sized."""
    H, g, s = np.asarray(H, dtype), np.asarray(g, dtype), np.asarray(s, dtype)
    act = active_mask(H) if act is None else np.asarray(act, bool)
    if np.asarray(E).shape[0] != ND:
        E, eg = embed_E(E, eg, dtype)
    E, eg = np.asarray(E, dtype), np.asarray(eg, dtype)
    on = act.astype(dtype)
    Ht = (s[:, None] * H) * s[None, :] * on[:, None] * on[None, :]
    D2 = np.clip(s * s * np.diag(H), dtype(GF_MIN_DIAG), dtype(GF_MAX_DIAG)) * on
    Et = (s[:, None] * E) * s[None, :] * on[:, None] * on[None, :]
    mu = dtype(mu)
    S = Ht + np.diag(mu * D2) - Et
    gt, seg = s * g * on, s * eg * on
    return dict(Ht=Ht, D2=D2, Et=Et, S=S, gt=gt, seg=seg, rhs=gt - seg, M=np.abs(Ht) + np.diag(mu * D2) + np.abs(Et), act=act, mu=mu, s=s, E=E)


def eta_den(sy, y):
    y = np.asarray(y, LD)
    return np.abs(sy["M"]).sum(axis=1).max() * np.abs(y).max() + (np.abs(sy["gt"]) + np.abs(sy["seg"])).max()


def eta_ratio(sy, y, K=None):
    """eta / (K u) of the step y (ND entries) on the longdouble system sy."""
    K = K_Y if K is None else K
    y = np.asarray(y, LD)
    if not np.isfinite(np.asarray(y, float)).all():
        return np.inf
    r = sy["S"] @ y - sy["rhs"]
    den = eta_den(sy, y)
    return float(np.abs(r).max() / den / (LD(K) * LD(U))) if den > 0 else 0.0


def s_ratio(H, s, act):
    """Largest relative error of the first iteration's s in units of S_TOL u; number of inactive dims whose s is not exactly 1.0."""
    ref = first_scaling(np.asarray(H, LD), act, LD)
    s = np.asarray(s, LD)
    rel = np.abs(s - ref)[act] / ref[act]
    return (float(rel.max() / (LD(S_TOL) * LD(U))) if act.any() else 0.0), int((np.asarray(s, float)[~act] != 1.0).sum())


def v_ratio(sy, v, g):
    """Largest relative error of v = (s g) / D2 in units of V_TOL u; number of entries that must be exactly 0.0 and are not."""
    act, v = sy["act"], np.asarray(v, LD)
    ref = np.zeros(ND, LD)
    ref[act] = sy["gt"][act] / sy["D2"][act]
    nz = act & (np.asarray(g, float) != 0.0)
    rel = np.abs(v - ref)[nz] / np.abs(ref[nz])
    return (float(rel.max() / (LD(V_TOL) * LD(U))) if nz.any() else 0.0), int((np.asarray(v, float)[~nz] != 0.0).sum())


def scalar_refs(sy, v, y):
    """References and bounds of the seven scalars from the system sy and the vectors v, y (longdouble):
    {name: (reference, K-scaled part A of the bound in units of u, additive part B)}. The K of A is SUM_TOL for the positive sums
    and K_S for the subtracted ones."""
    v, y = np.asarray(v, LD), np.asarray(y, LD)
    act, D2, gt, mu, M = sy["act"], sy["D2"], sy["gt"], sy["mu"], sy["M"]
    D2i = np.where(act, LD(1) / np.where(act, D2, LD(1)), LD(0))
    av, ay = np.abs(v), np.abs(y)
    asv, asy = np.abs(sy["s"] * v) * act, np.abs(sy["s"] * y) * act
    aE = np.abs(sy["E"])
    den = eta_den(sy, y)
    eb = LD(K_Y) * LD(U) * den
    vDv, N2 = (D2 * v * v).sum(), (D2 * y * y).sum()
    out = {
        "G2": ((gt * gt * D2i).sum(), (gt * gt * D2i).sum(), LD(0)),
        "N2": (N2, N2, LD(0)),
        "gy": ((gt * y).sum(), np.abs(gt * y).sum(), LD(0)),
        "vHv": (v @ sy["Ht"] @ v, av @ M @ av + mu * vDv + asv @ aE @ asv, LD(0)),
        "vHy": (v @ sy["Ht"] @ y, av @ M @ ay + av @ (np.abs(gt) + np.abs(sy["seg"])) + mu * (D2 * av * ay).sum() + asv @ aE @ asy, eb * av.sum()),
        "yHy": (y @ sy["Ht"] @ y, ay @ M @ ay + mu * N2 + asy @ aE @ asy, eb * ay.sum()),
    }
    return out


def scalar_ratios(sy, v, y, got, K_s=None):
    """got: dict with G2, N2, gy, vHv, vHy, yHy. Returns {name: |got - ref| / bound}; `raw`: {name: max(|got - ref| - B, 0) / (u A)}."""
    K_s = K_S if K_s is None else K_s
    refs = scalar_refs(sy, v, y)
    ratio, raw = {}, {}
    for k, (ref, A, B) in refs.items():
        K = SUM_TOL if k in ("G2", "N2", "gy") else K_s
        err = abs(LD(got[k]) - ref)
        if not np.isfinite(float(got[k])):
            ratio[k] = raw[k] = np.inf
            continue
        bound = LD(K) * LD(U) * A + B
        ratio[k] = float(err / bound) if bound > 0 else (0.0 if err == 0 else np.inf)
        raw[k] = float(max(err - B, LD(0)) / (LD(U) * A)) if A > 0 else (0.0 if err == 0 else np.inf)
    return ratio, raw


# ---------------------------------------------------------------------------------------------------------------- plain FP64 solve
def tri_solve(L, b, lower=True):
    """Triangular solve by substitution in the dtype of L (numpy has no trsv without scipy)."""
    n = len(b)
    x = np.array(b, L.dtype)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        if lower:
            x[i] = (x[i] - L[i, :i] @ x[:i]) / L[i, i]
        else:
            x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def fp64_solve(H, g, E, eg, mu, mutate=None):
    """The solve in plain FP64: s, S by the formula, numpy.linalg.cholesky, two triangular solves, and the scalars in the device's
    term grouping. `mutate`: one of the defects of test_solve_step_reference.py, injected into the SOLVE (never into the checker).
    Returns dict with act, s, v, y (ND entries each) and the scalars."""
    H, g = np.asarray(H, float), np.asarray(g, float)
    act = active_mask(H)
    s = first_scaling(H, act)
    Ef, egf = embed_E(E, eg, float) if np.asarray(E).shape[0] != ND else (np.asarray(E, float), np.asarray(eg, float))
    Es = Ef.copy()
    mu_s = mu
    if mutate == "mu_decade":
        mu_s = 10.0 * mu
    if mutate == "E_row":                    # one row and column of E zeroed (the visual dim with the largest diagonal)
        a = int(np.argmax(np.diag(Es)))
        Es[a, :] = 0.0
        Es[:, a] = 0.0
    sy = restate(H, g, Es, egf, s, mu_s, act, float)
    ix = np.where(act)[0]
    n = len(ix)
    S, rhs = sy["S"][np.ix_(ix, ix)], sy["rhs"][ix]
    if mutate == "sb_coupling":              # one speed-bias block solved without its coupling to the next one
        sb = [k for k in range(ne.NF - 1) if act[ne.T_SB(k)] and act[ne.T_SB(k + 1)]]
        k = sb[len(sb) // 2]
        pos = {a: q for q, a in enumerate(ix)}
        p0 = [pos[ne.T_SB(k) + q] for q in range(9)]
        p1 = [pos[ne.T_SB(k + 1) + q] for q in range(9)]
        S = S.copy()
        S[np.ix_(p0, p1)] = 0.0
        S[np.ix_(p1, p0)] = 0.0
    if mutate in ("E_row", "sb_coupling"):  # (the defective matrix need not be positive definite: a general solve of it)
        yv = np.linalg.solve(S, rhs)
        zz = rhs @ yv
    else:
        L = np.linalg.cholesky(S)
        z = tri_solve(L, rhs, True)
        if mutate == "tile_product":         # one 16-row block of the forward substitution without one off-diagonal tile's contribution:
            nt = (n + TB - 1) // TB          # the tile of the factor with the largest norm
            norm = {(I, J): np.linalg.norm(L[I * TB:(I + 1) * TB, J * TB:(J + 1) * TB]) for I in range(nt) for J in range(I)}
            I, J = max(norm, key=norm.get)
            z = np.array(rhs)
            for i in range(n):
                cols = np.arange(i)
                if i // TB == I:
                    cols = cols[cols // TB != J]
                z[i] = (z[i] - L[i, cols] @ z[cols]) / L[i, i]
        if mutate == "rhs_row":              # the right-hand side row taken from the previous tile row of the augmented factor
            z = np.r_[L[n - TB, :n - TB + 1], np.zeros(TB - 1)]
        yv = tri_solve(L, z, False)
        zz = z @ z
    y, v = np.zeros(ND), np.zeros(ND)
    y[ix] = yv
    v[ix] = sy["gt"][ix] / sy["D2"][ix]
    # the dogleg scalars as the device groups them (with the true mu and E: the mutations above are defects of the solve)
    sy = restate(H, g, Ef, egf, s, mu, act, float)
    D2, gt = sy["D2"], sy["gt"]
    sv, sY = s * v * act, s * y * act
    vDv, vDy, N2 = (D2 * v * v).sum(), (D2 * v * y).sum(), (D2 * y * y).sum()
    vEv, vEy, yEy = sv @ Ef @ sv, sv @ Ef @ sY, sY @ Ef @ sY
    vSv, vrhs = v @ sy["S"] @ v, v @ sy["rhs"]
    out = dict(act=act, s=s, v=v, y=y, mu=mu, G2=(gt[ix] * gt[ix] / D2[ix]).sum(), N2=N2, gy=gt @ y,
               vHv=vSv - mu * vDv + vEv, vHy=vrhs - mu * vDy + vEy, yHy=zz - mu * N2 + (0.0 if mutate == "no_yEy" else yEy))
    return out


def check_all(H, g, E, eg, s, v, y, scal, mu):
    """Every check on one window's data (H full symmetric). Returns (ratios: dict name -> error / bound, raw scalar ratios in u A,
    list of exact-value failures). eta is reported as `y`; eta / u is ratios['y'] * K_Y."""
    act = active_mask(H)
    sy = restate(H, g, E, eg, s, mu, act)
    ratios, exact = {}, []
    ratios["y"] = eta_ratio(sy, y)
    if (np.asarray(y, float)[~act] != 0.0).any():
        exact.append("y is not exactly 0.0 on %d inactive dims" % int((np.asarray(y, float)[~act] != 0.0).sum()))
    ratios["s"], n1 = s_ratio(H, s, act)
    if n1:
        exact.append("s is not exactly 1.0 on %d inactive dims" % n1)
    ratios["v"], n0 = v_ratio(sy, v, g)
    if n0:
        exact.append("v is not exactly 0.0 on %d dims where g is 0.0 or the dim is inactive" % n0)
    sr, raw = scalar_ratios(sy, v, y, scal)
    ratios.update(sr)
    return ratios, raw, exact
