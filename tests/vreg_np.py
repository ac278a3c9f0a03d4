"""numpy model of the scan-to-map registration loop (the checker of gfbe_vmap_register), written from the behaviour of
lidarodom::optimize (lio/src/liw/lio/lidarodom.cpp:534-748), the consistency factors of lidarFactor.cpp:125-219, the Plus of
poseParameterization.cpp:31-50 and the Ceres 1.14 trust-region rules stated in the header of oracle/gfo_posegraph.cpp. The association is
vmap_np.associate. Everything runs in the caller's dtype (float64, or numpy.longdouble for the extended-precision reference).

Next to its results every function returns the margin of each discrete decision it took (|value - threshold| and the magnitude the
rounding of `value` scales with) and the absolute sums A_X behind the continuous outputs, for the bounds K_X u A_X of
tests/test_gpu_vreg.py."""
import numpy as np

import vmap_np as vm

LD, U = vm.LD, vm.U
DEFAULTS = dict(max_num_iteration=10, lm_max_num_iterations=5, min_num_residuals=300, laser_point_cov=0.001, huber_delta=0.5,
                beta_location_consistency=1.0, beta_orientation_consistency=1.0, beta_small_velocity=0.0, thres_translation_norm=0.01,
                thres_orientation_norm=0.1)


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in o, k
        o[k] = v
    return o


def qmul(a, b):      # [x y z w]
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], a.dtype)


def plus(pose, d6, dt):
    """[t | q]: t + dt, q * deltaQ(dtheta), normalised."""
    h = d6[3:] / dt(2)
    dq = np.array([h[0], h[1], h[2], dt(1)], dt) / np.sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2] + dt(1))
    q = qmul(pose[3:], dq)
    q = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.concatenate([pose[:3] + d6[:3], q])


def _qbr(q, sgn, dt):
    x, y, z, w = q
    return np.array([[w, -sgn * z, sgn * y], [sgn * z, w, -sgn * x], [-sgn * y, sgn * x, w]], dt)


def row(ct, p, nv, off, w, al, sqrt_info, pb, pe, dt):
    """One point-to-plane factor as the device's lio_row evaluates it: (r, J [6 or 12], A_r = the absolute sum behind r)."""
    qs, ts = pb[3:], pb[:3]
    if ct:
        s = vm._slerp(pb[3:], al, pe[3:], dt)
        qs = s / np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + s[3] * s[3])
        ts = pb[:3] * (dt(1) - al) + pe[:3] * al
    R = vm._qrot(qs, dt)
    pw = R @ p + ts
    r = sqrt_info * w * (nv[0] * pw[0] + nv[1] * pw[1] + nv[2] * pw[2] + off)
    A_r = float(sqrt_info * w) * float(np.abs(nv) @ (np.abs(R) @ np.abs(p) + np.abs(ts)) + abs(off))
    nR = nv @ R
    jrs = -w * np.cross(nR, p)
    if not ct:
        return r, np.concatenate([sqrt_info * w * nv, sqrt_info * jrs]), A_r
    qbi = np.array([-pb[3], -pb[4], -pb[5], pb[6]], dt)
    rd = qmul(qbi, pe[3:])
    rds = vm._slerp(np.array([0, 0, 0, 1], dt), al, rd, dt)
    Rds = vm._qrot(rds, dt)
    T1 = _qbr(rds, +1, dt) @ _inv3(_qbr(rd, +1, dt))
    Jb = Rds.T @ (np.eye(3, dtype=dt) - al * T1)
    T2 = _qbr(rds, -1, dt) @ _inv3(_qbr(rd, -1, dt))
    Je = al * T2
    J = np.concatenate([sqrt_info * w * nv * (dt(1) - al), sqrt_info * (jrs @ Jb), sqrt_info * w * nv * al, sqrt_info * (jrs @ Je)])
    return r, J, A_r


def _inv3(A):
    c0, c1, c2 = A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1], A[1, 2] * A[2, 0] - A[1, 0] * A[2, 2], A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]
    det = A[0, 0] * c0 + A[0, 1] * c1 + A[0, 2] * c2
    return np.array([[c0, A[0, 2] * A[2, 1] - A[0, 1] * A[2, 2], A[0, 1] * A[1, 2] - A[0, 2] * A[1, 1]],
                     [c1, A[0, 0] * A[2, 2] - A[0, 2] * A[2, 0], A[0, 2] * A[1, 0] - A[0, 0] * A[1, 2]],
                     [c2, A[0, 1] * A[2, 0] - A[0, 0] * A[2, 1], A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]]], A.dtype) / det


def huber(r, J, delta, dt):
    """Ceres' Corrector for HuberLoss on a scalar residual: (r', J', rho / 2, outlier). rho'' <= 0: scaling by sqrt(rho') alone."""
    sq = r * r
    if delta > 0 and sq > delta * delta:
        rr = np.sqrt(sq)
        sr = np.sqrt(max(dt(1e-300), delta / rr))
        return r * sr, J * sr, dt(0.5) * (dt(2) * delta * rr - delta * delta), True
    return r, J, dt(0.5) * sq, False


def consistency(x, n_res, o, prev_t, prev_q, dt):
    """The three factors of the ct = 1 problem at x = [begin | end]: list of (r [3], J [3, 12])."""
    out = []
    cov = dt(o["laser_point_cov"])
    if o["beta_location_consistency"] > 0:
        w = np.sqrt(dt(n_res) * dt(o["beta_location_consistency"]) * cov)
        J = np.zeros((3, 12), dt)
        J[:, 0:3] = w * np.eye(3, dtype=dt)
        out.append((w * (x[0:3] - prev_t), J))
    if o["beta_orientation_consistency"] > 0:
        w = np.sqrt(dt(n_res) * dt(o["beta_orientation_consistency"]) * cov)
        p2 = prev_q @ prev_q
        qt = qmul(np.array([-prev_q[0], -prev_q[1], -prev_q[2], prev_q[3]], dt) / p2, x[3:7])
        J = np.zeros((3, 12), dt)
        J[:, 3:6] = w * np.array([[qt[3], -qt[2], qt[1]], [qt[2], qt[3], -qt[0]], [-qt[1], qt[0], qt[3]]], dt)
        out.append((dt(2) * qt[:3] * w, J))
    if o["beta_small_velocity"] > 0:
        w = np.sqrt(dt(n_res) * dt(o["beta_small_velocity"]) * cov)
        J = np.zeros((3, 12), dt)
        J[:, 0:3], J[:, 6:9] = w * np.eye(3, dtype=dt), -w * np.eye(3, dtype=dt)
        out.append((w * (x[0:3] - x[7:10]), J))
    return out


def linearize(ct, rows, x, n_res, o, prev_t, prev_q, dt):
    """H, g, cost of the robustified point-to-plane rows plus the consistency factors at x [14]; A_cost; per-row Huber margins."""
    dn = 12 if ct else 6
    H, g, cost, A_cost = np.zeros((dn, dn), dt), np.zeros(dn, dt), dt(0), 0.0
    sqrt_info, delta = dt(np.sqrt(1.0 / np.float64(o["laser_point_cov"]))), dt(o["huber_delta"])
    hub = []
    pb, pe = x[:7], x[7:]
    for k in range(n_res):
        r, J, A_r = row(ct, rows["pts"][k].astype(dt), rows["normals"][k].astype(dt), dt(rows["offsets"][k]), dt(rows["weights"][k]),
                        dt(rows["alpha"][k]) if ct else dt(0), sqrt_info, pb, pe, dt)
        if delta > 0:
            hub.append((abs(float(abs(r) - delta)), A_r))
        r2, J2, c, _out = huber(r, J, delta, dt)
        H += np.outer(J2, J2)
        g += J2 * r2
        cost += c
        A_cost += float(c) + float(min(abs(r), delta if delta > 0 else abs(r))) * A_r
    if ct:
        for r, J in consistency(x, n_res, o, prev_t, prev_q, dt):
            H += J.T @ J
            g += J.T @ r
            cost += dt(0.5) * (r @ r)
            A_cost += float(r @ r) + float(np.abs(r).sum() * np.abs(J).max() * (np.abs(x).max() + np.abs(prev_t).max() + 1))
    return H, g, cost, A_cost, hub


def chol_solve(A, b, dt):
    n = len(b)
    L = A.copy()
    for c in range(n):
        ds = L[c, c] - (L[c, :c] @ L[c, :c] if c else dt(0))
        if not ds > 0 or not np.isfinite(ds):
            return None
        L[c, c] = np.sqrt(ds)
        for a in range(c + 1, n):
            L[a, c] = (L[a, c] - (L[a, :c] @ L[c, :c] if c else dt(0))) / L[c, c]
    y = np.zeros(n, dt)
    for a in range(n):
        y[a] = (b[a] - L[a, :a] @ y[:a]) / L[a, a]
    for a in range(n - 1, -1, -1):
        y[a] = (y[a] - L[a + 1:, a] @ y[a + 1:]) / L[a, a]
    return y


def lm(evaluate, x, step, max_it, dt):
    """Ceres 1.14's trust-region loop with the Levenberg-Marquardt strategy on evaluate(x) -> (H, g, cost, A_cost), step(x, d) -> x'.
    Returns dict(x, iterations, accepted bits, termination, cost_initial, cost_final, failed, trace, margins, kappa, delta_l1)."""
    H, g, cost, A_cost = evaluate(x)
    out = dict(cost_initial=cost, A_cost_initial=A_cost, trace=[], margins=[], kappa=1.0, delta_l1=0.0)
    scale = dt(1) / (dt(1) + np.sqrt(np.diag(H)))
    radius, decrease, it, invalid, acc, reuse, diag2, term, failed = dt(1e4), dt(2), 0, 0, 0, False, None, None, False
    x_norm = np.sqrt(x @ x)
    while True:
        if it >= max_it:
            term = 0
            break
        gmax = np.abs(g).max()
        out["margins"].append(("gradient", abs(float(gmax) - 1e-10), float(gmax)))
        if gmax <= 1e-10:
            term = 3
            break
        if radius < 1e-32:
            term = 4
            break
        it += 1
        Ad = H * np.outer(scale, scale)
        rhs = -scale * g
        if not reuse:
            diag2 = np.minimum(np.maximum(np.diag(Ad), dt(1e-6)), dt(1e32))
        Areg = Ad + np.diag(diag2 / radius)
        y = chol_solve(Areg, rhs, dt)
        mc = dt(0)
        if y is not None:
            mc = -((-rhs) @ y + dt(0.5) * (y @ (Ad @ y)))
        if y is None or not mc > 0:
            out["trace"].append(dict(it=it, valid=False, accepted=False))
            invalid += 1
            if invalid >= 5:
                term, failed = 4, True
                break
            radius, decrease, reuse = radius / decrease, decrease * 2, True
            continue
        cand = step(x, scale * y)
        step2 = (cand - x) @ (cand - x)
        _, _, cand_cost, A_cand = evaluate(cand)
        if not np.isfinite(cand_cost):      # a candidate without a finite cost is an invalid step too
            out["trace"].append(dict(it=it, valid=False, accepted=False))
            invalid += 1
            if invalid >= 5:
                term, failed = 4, True
                break
            radius, decrease, reuse = radius / decrease, decrease * 2, True
            continue
        invalid = 0
        tol = 1e-8 * (float(x_norm) + 1e-8)
        out["margins"].append(("parameter", abs(float(np.sqrt(step2)) - tol), float(np.sqrt(step2))))
        if np.sqrt(step2) <= dt(1e-8) * (x_norm + dt(1e-8)):
            term = 2
            break
        change = cost - cand_cost
        out["margins"].append(("function", abs(abs(float(change)) - 1e-6 * float(cost)), A_cost + A_cand))
        if abs(change) <= dt(1e-6) * cost:
            term = 1
            break
        rho = change / mc
        out["margins"].append(("quality", abs(float(rho) - 1e-3), (A_cost + A_cand) / float(mc)))
        kappa = float(np.linalg.cond(Areg.astype(np.float64)))
        if rho > dt(1e-3):
            out["trace"].append(dict(it=it, valid=True, accepted=True, rho=float(rho), radius=float(radius)))
            out["kappa"], out["delta_l1"] = kappa, out["delta_l1"] + float(np.abs(scale * y).sum())
            x, cost, A_cost = cand, cand_cost, A_cand
            x_norm = np.sqrt(x @ x)
            acc |= 1 << (it - 1)
            tq = dt(2) * rho - dt(1)
            radius = min(dt(1e16), radius / max(dt(1) / dt(3), dt(1) - tq * tq * tq))
            decrease, reuse = dt(2), False
            H, g, _, _ = evaluate(x)
        else:
            out["trace"].append(dict(it=it, valid=True, accepted=False, rho=float(rho), radius=float(radius)))
            radius, decrease, reuse = radius / decrease, decrease * 2, True
    out.update(g_l1=float(np.abs(g).sum()), x=x, iterations=it, accepted=acc, termination=term, cost_final=cost, A_cost_final=A_cost, failed=failed, final_radius=float(radius))
    return out


def angle_deg(qa, qb, dt):
    """AngularDistance in degrees with the acos argument clamped to [-1, 1]; (angle, unclamped argument)."""
    tr = dt(0)
    for v in (vm._qrot(qa, dt) * vm._qrot(qb, dt)).reshape(9):      # (the device's order of the nine products)
        tr = tr + v
    arg = (tr - dt(1)) / dt(2)
    return np.arccos(min(dt(1), max(dt(-1), arg))) * dt(180) / (dt(4) * np.arctan(dt(1))), arg


def outer_iteration(m, ct, raw, alpha, x, o, prev_t=None, prev_q=None, frame_init=False, dtype=np.float64):
    """One outer iteration from x = [begin | end] (float64 values): associate, the inner solve, the exit test."""
    dt = dtype
    x = np.asarray(x, np.float64).astype(dt)
    prev_t = np.zeros(3, dt) if prev_t is None else np.asarray(prev_t, np.float64).astype(dt)
    prev_q = np.array([0, 0, 0, 1], dt) if prev_q is None else np.asarray(prev_q, np.float64).astype(dt)
    rows = vm.associate(m, ct, raw, alpha, x[:7], x[7:], frame_init, dt)
    n_res = rows["n_res"]
    out = dict(n_res=n_res, rows=rows, x=x, too_few=n_res < o["min_num_residuals"])
    if n_res == 0:
        return out
    np_ = 14 if ct else 7
    hub_all = []

    def evaluate(xa):
        xx = np.concatenate([xa, x[7:]]) if not ct else xa
        H, g, c, A, hub = linearize(ct, rows, xx, n_res, o, prev_t, prev_q, dt)
        hub_all.append(hub)
        return H, g, c, A

    def step(xa, d):
        return plus(xa, d, dt) if not ct else np.concatenate([plus(xa[:7], d[:6], dt), plus(xa[7:], d[6:], dt)])
    res = lm(evaluate, x[:np_].copy(), step, o["lm_max_num_iterations"], dt)
    x1 = np.concatenate([res["x"], x[7:]]) if not ct else res["x"]
    dtr, drot, args = dt(0), dt(0), []
    for h in range(2):
        a, b = x[7 * h:7 * h + 7], x1[7 * h:7 * h + 7]
        dtr += np.sqrt(((a[:3] - b[:3]) ** 2).sum())
        ang, arg = angle_deg(a[3:], b[3:], dt)
        drot, args = drot + ang, args + [float(arg)]
    # the absolute sums behind the outputs
    A_pose = res["kappa"] * (res["delta_l1"] + float(np.abs(x1).max()))
    res["A_cost_final"] += res["g_l1"] * A_pose      # (the final cost is taken at the final pose: its bound moves the cost by |g| A_pose)
    th = [max(float(np.sqrt(max(0.0, 2 * (1 - min(1.0, a))))), float(np.sqrt(8 * U))) for a in args]
    A_dr = float(180 / np.pi) * sum(2 * A_pose + 8 / t for t in th)
    A_dt = 2 * A_pose + float(np.abs(x).max() + np.abs(x1).max())
    res["margins"] += [("exit_trans", abs(float(dtr) - o["thres_translation_norm"]), A_dt), ("exit_rot", abs(float(drot) - o["thres_orientation_norm"]), A_dr)]
    first_hub = hub_all[0]
    out.update(x=x1, lm=res, diff_trans=dtr, diff_rot=drot, acos_args=args, A_pose=A_pose, A_dt=A_dt, A_dr=A_dr, hub=[h for hs in hub_all for h in hs],
               n_outliers_first=sum(1 for k in range(n_res) if _is_outlier(ct, rows, k, x, o, dt)) if o["huber_delta"] > 0 else 0, first_hub=first_hub,
               converged=bool(drot < dt(o["thres_orientation_norm"]) and dtr < dt(o["thres_translation_norm"])))
    return out


def _is_outlier(ct, rows, k, x, o, dt):
    r, _, _ = row(ct, rows["pts"][k].astype(dt), rows["normals"][k].astype(dt), dt(rows["offsets"][k]), dt(rows["weights"][k]),
                  dt(rows["alpha"][k]) if ct else dt(0), dt(np.sqrt(1.0 / np.float64(o["laser_point_cov"]))), x[:7], x[7:], dt)
    return abs(r) > o["huber_delta"]


def register(m, ct, raw, alpha, pose_begin, pose_end=None, o=None, prev_t=None, prev_q=None, frame_init=False, dtype=np.float64):
    """The whole loop: dict(x, outer_iterations, converged, too_few_residuals, no_residuals, failed, iterations = [outer_iteration results])."""
    o = o or options()
    x = np.concatenate([np.asarray(pose_begin, np.float64), np.asarray(pose_end if pose_end is not None else pose_begin, np.float64)])
    out = dict(iterations=[], converged=0, too_few_residuals=0, no_residuals=0, failed=False, outer_iterations=0)
    for k in range(o["max_num_iteration"]):
        it = outer_iteration(m, ct, raw, alpha, x, o, prev_t, prev_q, frame_init, dtype)
        out["iterations"].append(it)
        out["too_few_residuals"] |= int(it["too_few"])
        if it["n_res"] == 0:
            out["no_residuals"] = 1
            break
        x = np.asarray(it["x"], np.float64)      # (the device's poses are float64)
        out["outer_iterations"] = k + 1
        if it["lm"]["failed"]:
            out["failed"] = True
            break
        if it["converged"]:
            out["converged"] = 1
            break
    out["x"] = x
    rows = out["iterations"][-1]["rows"]
    sv, deg, A_sv = vm.localizability(rows["normals"], rows["relgap_res"], dtype)
    out.update(sv=sv, degenerate=int(deg), A_sv=A_sv)
    return out
