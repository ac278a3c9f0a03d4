"""The GNSS factors in extended precision: a numpy.longdouble statement of THE OPERATION THE DEVICE PERFORMS, gnss_psr_dopp_eval /
gnss_dt_ddt_res / gnss_ddt_smooth_res of ground-fusion2_amd/csrc/gfbe_gnss.h, with the absolute sums that go with every result and
the distance of every observation from every branch of that arithmetic. CPU only, HIP-free. tests/test_gnss_reference.py measures the
bounds below on the CPU; tests/test_gpu_gnss.py holds the device's gfbe_gnss_eval (and the oracle) to them, entry by entry.

This is not tests/gnss_cases.py: that file states the published formulas independently (latitude by iteration, unit vectors instead
of a rotation product) and checks the FORMULAS to 2e-6. This one follows gfbe_gnss.h operation by operation (the closed-form
ecef2geo, geo2rotation, azimuth / elevation, Saastamoinen x Niell, Klobuchar, both weights, both residuals, the 2 x 18 Jacobian with
the reference's omissions), with every constant the double the C code holds (GNSS_PI is the double, not an 80-bit pi), and checks the
ARITHMETIC. The same code runs in any floating type T: T = longdouble is the reference, T = float64 is a plain FP64 statement on
which the branch condition is checked and into which tests/test_gnss_reference.py injects its defects.

What is compared, with u = 2^-53, for every observation k:

    |r_dev[k, q]    - r[k, q]   | <= K_R u A_r[k, q]           q = pseudo-range, Doppler
    |J_dev[k, q, c] - J[k, q, c]| <= K_J u A_J[k, q, c]        c = the 18 columns P_i V_i P_j V_j rcv_dt rcv_ddt yaw anc
    |r_clk_dev      - r_clk     | <= K_CLK u A_clk             the 40 DtDdt and 10 DdtSmooth residuals

A_r = weight x the sum of the absolute values of the terms of psr_est - psr, respectively dopp_est + dopp lambda (the Sagnac terms
product by product, dv . u as sum |dv_i| |u_i|). A_J = the products that form the entry summed in absolute value (R = Ree Rel as
|Ree| |Rel|, the differences sp - P and sv - V as |sp| + |P| and |sv| + |V|: a line-of-sight component near zero is the difference of
two ECEF coordinates of 1e7 m; the yaw column's cancelling dot product at its full size), times 1 + 2 |cot el|: both weights are sin^2(asin(.)) of a
computed elevation, so a rounding of the elevation comes back 2 cot(el) times as large in the weight (15 times at 8 degrees). That is
conditioning and belongs in the scale (A_r carries it on the residual's own size: + 2 |cot el| |r|); K stays a statement about rounding. A_clk = 50 (|dt_j - dt_i| + 0.5 (|ddt_i| + |ddt_j|) dt),
respectively w |ddt_i - ddt_j| (a difference of two doubles is rounded once, relative to itself; the clock biases are 1e5 m). Where A is exactly zero (the pseudo-range row at the velocities and the clock drift, the Doppler
row at the clock bias and the anchor, the columns of a pose whose interpolation weight is exactly 0) both sides must hold exactly 0.

K is measured on the CPU, never on the device: the largest |X_fp64 - X_model| / (u A_X) over all cases of gnss_model_cases(), both
ionosphere settings, for the oracle's gfo_gnss_eval and for gfbe_gnss.h compiled for the host (tests/host_shim.cpp):

    r %(r)s   J %(J)s   clock residuals %(clk)s        (in units of u A_X; tests/test_gnss_reference.py asserts them)

K = 8 x that, rounded up to a power of two (the rule of normal_equations_np.K_MARGIN): K_R = %(K_R)s, K_J = %(K_J)s, K_CLK = %(K_CLK)s. The 8 is
for what the device may do differently: OCML's sin, cos, atan2, asin, pow and exp are not correctly rounded, and fused multiply-adds.

Branches. The arithmetic decides on el <= 0, the height limits of the troposphere (-100 m, 0, 1e4 m; -1e3 m for the ionosphere),
int(|lat| / 15) and the sign of lat, the clamps of phi (+-0.416), amp (0) and per (72000), |x| < 1.57, the floor of the local time,
the az < 0 wrap and the 1e-12 zenith test. branch_failures() takes every observation's signed distance from each of them, made
dimensionless (psr_dopp()["margins"]); a case may hold an observation only if FP64 and longdouble put it on the same side with BRANCH_ROOM to spare.
That is a condition on the cases, asserted for every observation on the CPU; no observation is ever left out of a comparison.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
WINDOW = 10

# the doubles of gfbe_gnss.h
LIGHT_SPEED, EARTH_OMG, ECCE_2, SEMI_MAJOR, PI, PSR_TO_DOPP = 2.99792458e8, 7.2921151467e-5, 6.69437999014e-3, 6378137.0, 3.14159265358979323846, 5.0
NIELL = ((1.2769934e-3, 1.2683230e-3, 1.2465397e-3, 1.2196049e-3, 1.2045996e-3), (2.9153695e-3, 2.9152299e-3, 2.9288445e-3, 2.9022565e-3, 2.9024912e-3),
         (62.610505e-3, 62.837393e-3, 63.721774e-3, 63.824265e-3, 64.258455e-3), (0.0, 1.2709626e-5, 2.6523662e-5, 3.4000452e-5, 4.1202191e-5),
         (0.0, 2.1414979e-5, 3.0160779e-5, 7.2562722e-5, 11.723375e-5), (0.0, 9.0128400e-5, 4.3497037e-5, 84.795348e-5, 170.37206e-5),
         (5.8021897e-4, 5.6794847e-4, 5.8118019e-4, 5.9727542e-4, 6.1641693e-4), (1.4275268e-3, 1.5138625e-3, 1.4572752e-3, 1.5007428e-3, 1.7599082e-3),
         (4.3472961e-2, 4.6729510e-2, 4.3908931e-2, 4.4626982e-2, 5.4736038e-2))

# Largest |X_fp64 - X_model| / (u A_X), measured by tests/test_gnss_reference.py (which asserts them) over gnss_model_cases()
K_MEASURED = dict(r=2.5, J=5.5, clk=0.6)
K_MARGIN = 8.0
K_R, K_J, K_CLK = 32.0, 64.0, 8.0           # K_MARGIN x K_MEASURED, rounded up to a power of two
BRANCH_ROOM = 1e-9                           # dimensionless distance every observation keeps from every branch (FP64 resolves 1e-16)
__doc__ = __doc__ % dict({k: "%.3g" % v for k, v in K_MEASURED.items()}, K_R="%g" % K_R, K_J="%g" % K_J, K_CLK="%g" % K_CLK)

DEFECTS = ("tgd_sign", "dp_uura_in_psr_weight", "sagnac_index", "pj_ratio", "yaw_no_sin", "clk_half")


def require_extended_precision():
    import pytest
    if np.finfo(LD).nmant < 63:
        pytest.skip("numpy.longdouble has a %d-bit mantissa on this host: no extended-precision reference" % np.finfo(LD).nmant)


# ---------------------------------------------------------------------------------------------------------------- gfbe_gnss.h in type T
def _ecef2geo(T, x):
    if x[0] == 0 and x[1] == 0:
        return np.zeros(3, T)
    e2, a = T(ECCE_2), T(SEMI_MAJOR)
    a2 = a * a
    b2 = a2 * (T(1) - e2)
    b, ep2 = np.sqrt(b2), (a2 - b2) / b2
    p = np.sqrt(x[0] * x[0] + x[1] * x[1])
    s1, s2 = x[2] * a, p * b
    h = np.sqrt(s1 * s1 + s2 * s2)
    st, ct = s1 / h, s2 / h
    s1 = x[2] + ep2 * b * st * st * st
    s2 = p - a * e2 * ct * ct * ct
    h = np.sqrt(s1 * s1 + s2 * s2)
    sl, cl = s1 / h, s2 / h
    lat = np.arctan(s1 / s2)
    N = a2 / np.sqrt(a2 * cl * cl + b2 * sl * sl)
    deg = T(180) / T(PI)
    return np.array([lat * deg, np.arctan2(x[1], x[0]) * deg, p / cl - N], T)


def _geo2rotation(T, lla):
    rad = T(PI) / T(180)
    lat, lon = lla[0] * rad, lla[1] * rad
    sl, cl, so, co = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
    return np.array([[-so, -sl * co, cl * co], [co, -sl * so, cl * so], [T(0), cl, sl]], T)


def _interpc(T, coef, lat):
    i = int(lat / T(15))
    if i < 1:
        return T(coef[0])
    if i > 4:
        return T(coef[4])
    return T(coef[i - 1]) * (T(1) - lat / T(15) + T(i)) + T(coef[i]) * (lat / T(15) - T(i))


def _mapf(T, el, a, b, c):
    s = np.sin(el)
    return (T(1) + a / (T(1) + b / (T(1) + c))) / (s + (a / (s + b / (s + c))))


def _trop(T, doy, lla, az, el, m):
    m["h_lo"], m["h_hi"], m["h_zero"], m["el"] = (lla[2] + 100) / 100, (T(1e4) - lla[2]) / T(1e4), lla[2] / 100, el
    if lla[2] < T(-100) or T(1e4) < lla[2] or el <= 0:
        return T(0)
    hgt = T(0) if lla[2] < 0 else lla[2]
    pres = T(1013.25) * np.power(T(1) - T(2.2557e-5) * hgt, T(5.2568))
    temp = T(15) - T(6.5e-3) * hgt + T(273.16)
    e = T(6.108) * T(0.7) * np.exp((T(17.15) * temp - T(4684)) / (temp - T(38.45)))
    zhd = T(0.0022768) * pres / (T(1) - T(0.00266) * np.cos(T(2) * lla[0] * (T(PI) / T(180))) - T(0.00028) * hgt / T(1e3))
    zwd = T(0.002277) * (T(1255) / temp + T(0.05)) * e
    lat = lla[0]
    y = (doy - T(28)) / T(365.25) + (T(0.5) if lat < 0 else T(0))
    cosy = np.cos(T(2) * T(PI) * y)
    m["lat_sign"] = lat / 90
    lat = abs(lat)
    q = lat / T(15)
    m["lat_cell"] = min(abs(q - T(b)) for b in (1, 2, 3, 4, 5)) * (1 if int(q) % 2 else -1)     # signed by the cell's parity: a crossing flips it
    ah = [_interpc(T, NIELL[i], lat) - _interpc(T, NIELL[i + 3], lat) * cosy for i in range(3)]
    aw = [_interpc(T, NIELL[i + 6], lat) for i in range(3)]
    dm = (T(1) / np.sin(el) - _mapf(T, el, T(2.53e-5), T(5.49e-3), T(1.14e-3))) * lla[2] / T(1e3)
    mapfw, mapfh = _mapf(T, el, aw[0], aw[1], aw[2]), _mapf(T, el, ah[0], ah[1], ah[2]) + dm
    return mapfh * zhd + mapfw * zwd


def _ion(T, tow, ion, lla, az, el, m):
    if ion is None:
        return T(0)
    m["h_ion"] = (lla[2] + 1000) / 1000
    if lla[2] < T(-1e3) or el <= 0:
        return T(0)
    pi = T(PI)
    psi = T(0.0137) / (el / pi + T(0.11)) - T(0.022)
    phi = lla[0] / T(180) + psi * np.cos(az)
    m["phi_hi"], m["phi_lo"] = phi - T(0.416), phi + T(0.416)
    if phi > T(0.416):
        phi = T(0.416)
    elif phi < T(-0.416):
        phi = T(-0.416)
    lam = lla[1] / T(180) + psi * np.sin(az) / np.cos(phi * pi)
    phi = phi + T(0.064) * np.cos((lam - T(1.617)) * pi)
    tt = T(43200) * lam + tow
    days = tt / T(86400)
    m["tt_floor"] = min(days - np.floor(days), np.floor(days) + 1 - days)
    tt = tt - np.floor(days) * T(86400)
    f0 = T(0.53) - el / pi
    f = T(1) + T(16) * f0 * f0 * f0
    i = [T(v) for v in ion]
    amp = i[0] + phi * (i[1] + phi * (i[2] + phi * i[3]))
    per = i[4] + phi * (i[5] + phi * (i[6] + phi * i[7]))
    m["amp"], m["per"] = amp / (abs(i[0]) + abs(i[1]) + abs(i[2]) + abs(i[3])), (per - T(72000)) / T(72000)
    amp = T(0) if amp < 0 else amp
    per = T(72000) if per < T(72000) else per
    x = T(2) * pi * (tt - T(50400)) / per
    m["x_day"] = T(1.57) - abs(x)
    return T(LIGHT_SPEED) * f * (T(5e-9) + amp * (T(1) + x * x * (T(-0.5) + x * x / T(24))) if abs(x) < T(1.57) else T(5e-9))


def psr_dopp(T, o, ion, Pi, Vi, Pj, Vj, rcv_dt, rcv_ddt, yaw, anc, defect=None):
    """gnss_psr_dopp_eval in floating type T. Returns dict r [2], A_r [2], J [2, 18], A_J [2, 18], margins {branch: signed distance},
    el. defect: one of DEFECTS, a deliberately wrong statement (tests/test_gnss_reference.py)."""
    f = lambda v: T(float(v))                                             # noqa: E731  every input is the double the ABI carries
    v3 = lambda v: np.array([f(q) for q in v], T)                          # noqa: E731
    Pi, Vi, Pj, Vj, anc = v3(Pi[:3]), v3(Vi[:3]), v3(Pj[:3]), v3(Vj[:3]), v3(anc)
    rcv_dt, rcv_ddt, yaw, ratio = f(rcv_dt), f(rcv_ddt), f(yaw), f(o["ratio"])
    one = T(1)
    lp, lv = ratio * Pi + (one - ratio) * Pj, ratio * Vi + (one - ratio) * Vj
    alp, alv = ratio * abs(Pi) + (one - ratio) * abs(Pj), ratio * abs(Vi) + (one - ratio) * abs(Vj)
    sy, cy = np.sin(yaw), np.cos(yaw)
    Rel = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], T)
    Ree = _geo2rotation(T, _ecef2geo(T, anc))
    R, aR = Ree @ Rel, abs(Ree) @ abs(Rel)
    P, V = R @ lp + anc, R @ lv
    sp, sv = v3(o["sv_pos"]), v3(o["sv_vel"])
    m = {}
    ion_delay, tro_delay, az, el = T(0), T(0), T(0), T(PI) / T(2)
    if P @ P > 0:
        lla = _ecef2geo(T, P)
        d0 = sp - P
        u0 = d0 / np.sqrt(d0 @ d0)
        enu = _geo2rotation(T, lla).T @ u0
        hor = np.sqrt(u0[0] * u0[0] + u0[1] * u0[1])
        m["zenith"] = (hor - T(1e-12)) / T(1e-12) if hor < 1e-6 else one
        az = T(0) if hor < T(1e-12) else np.arctan2(enu[0], enu[1])
        m["az_wrap"] = az
        if az < 0:
            az = az + T(2) * T(PI)
        el = np.arcsin(enu[2])
        tro_delay = _trop(T, f(o["doy"]), lla, az, el, m)
        ion_delay = _ion(T, f(o["tow"]), ion, lla, az, el, m)
    sin_el = np.sin(el)
    sin_el_2 = sin_el * sin_el
    pr_weight = sin_el_2 / f(o["dp_uura" if defect == "dp_uura_in_psr_weight" else "pr_uura"]) * T(10)
    dp_weight = sin_el_2 / f(o["dp_uura"]) * T(10) * T(PSR_TO_DOPP)
    d = sp - P
    rng = np.sqrt(d @ d)
    u = d / rng
    c, w_c = T(LIGHT_SPEED), T(EARTH_OMG)
    sag = (sp[0] * P[0] - sp[1] * P[0]) if defect == "sagnac_index" else (sp[0] * P[1] - sp[1] * P[0])
    psr_sagnac = w_c * sag / c
    tgd = -f(o["tgd"]) if defect == "tgd_sign" else f(o["tgd"])
    psr_est = rng + psr_sagnac + rcv_dt - f(o["svdt"]) * c + ion_delay + tro_delay + tgd * c
    r0 = (psr_est - f(o["psr"])) * pr_weight
    A0 = (rng + w_c * (abs(sp[0] * P[1]) + abs(sp[1] * P[0])) / c + abs(rcv_dt) + abs(f(o["svdt"]) * c) + abs(ion_delay) + abs(tro_delay)
          + abs(f(o["tgd"]) * c) + abs(f(o["psr"]))) * pr_weight
    dopp_sagnac = w_c / c * (sv[0] * P[1] + sp[0] * V[1] - sv[1] * P[0] - sp[1] * V[0])
    dv = sv - V
    dopp_est = dv @ u + dopp_sagnac + rcv_ddt - f(o["svddt"]) * c
    r1 = (dopp_est + f(o["dopp"]) * f(o["wavelength"])) * dp_weight
    A1 = (abs(dv) @ abs(u) + w_c / c * (abs(sv[0] * P[1]) + abs(sp[0] * V[1]) + abs(sv[1] * P[0]) + abs(sp[1] * V[0])) + abs(rcv_ddt)
          + abs(f(o["svddt"]) * c) + abs(f(o["dopp"]) * f(o["wavelength"]))) * dp_weight
    J, AJ = np.zeros((2, 18), T), np.zeros((2, 18), T)
    aP, aV = aR @ alp + abs(anc), aR @ alv
    ad, adv = abs(sp) + aP, abs(sv) + aV                                  # d = sp - P and dv = sv - V cancel: their terms, not their values
    au = ad / rng
    uR, auR = R.T @ u, aR.T @ au
    n2 = rng * rng
    n3 = n2 * rng
    w, aw = np.zeros(3, T), np.zeros(3, T)
    for j in range(3):
        for i in range(3):
            w[j] += dv[i] * -(((n2 if i == j else T(0)) - d[i] * d[j])) / n3
            aw[j] += adv[i] * ((n2 if i == j else T(0)) + ad[i] * ad[j]) / n3
    wR, awR = R.T @ w, aR.T @ aw
    rj = ratio if defect == "pj_ratio" else one - ratio
    J[0, 0:3], AJ[0, 0:3] = -uR * pr_weight * ratio, auR * pr_weight * ratio
    J[1, 0:3], AJ[1, 0:3] = wR * dp_weight * ratio, awR * dp_weight * ratio
    J[1, 3:6], AJ[1, 3:6] = -uR * dp_weight * ratio, auR * dp_weight * ratio
    J[0, 6:9], AJ[0, 6:9] = -uR * pr_weight * rj, auR * pr_weight * (one - ratio)
    J[1, 6:9], AJ[1, 6:9] = wR * dp_weight * rj, awR * dp_weight * (one - ratio)
    J[1, 9:12], AJ[1, 9:12] = -uR * dp_weight * rj, auR * dp_weight * (one - ratio)
    J[0, 15:18], AJ[0, 15:18] = -u * pr_weight, au * pr_weight
    J[0, 12], AJ[0, 12] = pr_weight, pr_weight
    J[1, 13], AJ[1, 13] = dp_weight, dp_weight
    s_ = T(0) if defect == "yaw_no_sin" else sy
    dp = Ree @ np.array([-s_ * lp[0] - cy * lp[1], cy * lp[0] - s_ * lp[1], 0], T)
    dvv = Ree @ np.array([-s_ * lv[0] - cy * lv[1], cy * lv[0] - s_ * lv[1], 0], T)
    adp = abs(Ree) @ np.array([abs(sy) * alp[0] + abs(cy) * alp[1], abs(cy) * alp[0] + abs(sy) * alp[1], 0], T)
    advv = abs(Ree) @ np.array([abs(sy) * alv[0] + abs(cy) * alv[1], abs(cy) * alv[0] + abs(sy) * alv[1], 0], T)
    J[0, 14], AJ[0, 14] = -(u @ dp) * pr_weight, (au @ adp) * pr_weight
    J[1, 14], AJ[1, 14] = -(u @ dvv) * dp_weight, (au @ advv) * dp_weight
    cond = T(2) * abs(np.cos(el) / np.sin(el))                             # the weights' conditioning on the elevation
    AJ *= one + cond
    A0, A1 = A0 + cond * abs(r0), A1 + cond * abs(r1)                      # (nothing for a metre-level residual; a residual of 1e7 m carries its weight's rounding)
    return dict(r=np.array([r0, r1], T), A_r=np.array([A0, A1], T), J=J, A_J=AJ, margins=m, el=el)


def dt_ddt(T, dt_i, dt_j, ddt_i, ddt_j, delta_t, defect=None):
    """gnss_dt_ddt_res and its absolute sum."""
    dt_i, dt_j, ddt_i, ddt_j, delta_t = (T(float(v)) for v in (dt_i, dt_j, ddt_i, ddt_j, delta_t))
    half = T(1.0 if defect == "clk_half" else 0.5)
    return (dt_j - dt_i - half * (ddt_i + ddt_j) * delta_t) * T(50), (abs(dt_j - dt_i) + T(0.5) * (abs(ddt_i) + abs(ddt_j)) * abs(delta_t)) * T(50)


def ddt_smooth(T, ddt_i, ddt_j, weight):
    """gnss_ddt_smooth_res and its absolute sum."""
    ddt_i, ddt_j, weight = (T(float(v)) for v in (ddt_i, ddt_j, weight))
    return (ddt_i - ddt_j) * weight, abs(ddt_i - ddt_j) * abs(weight)


def eval_case(c, T=LD, iono="case", defect=None):
    """What gfbe_gnss_eval returns for case c (a dict of gnss_cases.gnss_case), in type T, with the absolute sums: r, A_r [n, 2],
    J, A_J [n, 2, 18], r_dt_ddt, A_dt_ddt [4, 10], r_smooth, A_smooth [10], cost, A_cost (sum of r^2 / 2), cost_allow (the first-order
    effect of the residuals' own bounds on the cost, sum |r| K u A_r), margins (a list of dicts per observation), el [n]."""
    ion = c["iono"] if isinstance(iono, str) else iono
    n = len(c["obs"])
    out = dict(r=np.zeros((n, 2), T), A_r=np.zeros((n, 2), T), J=np.zeros((n, 2, 18), T), A_J=np.zeros((n, 2, 18), T), margins=[], el=np.zeros(n, T))
    for k, o in enumerate(c["obs"]):
        lo = o["lower_idx"]
        e = psr_dopp(T, o, ion, c["pose"][lo], c["speed_bias"][lo], c["pose"][lo + 1], c["speed_bias"][lo + 1], c["rcv_dt"][o["frame"], o["sys_idx"]],
                     c["rcv_ddt"][o["frame"]], c["yaw"], c["anc"], defect=defect)
        for key in ("r", "A_r", "J", "A_J", "el"):
            out[key][k] = e[key]
        out["margins"].append(e["margins"])
    rc, Ac, rs, As = np.zeros((4, WINDOW), T), np.zeros((4, WINDOW), T), np.zeros(WINDOW, T), np.zeros(WINDOW, T)
    for i in range(WINDOW):
        for s in range(4):
            rc[s, i], Ac[s, i] = dt_ddt(T, c["rcv_dt"][i, s], c["rcv_dt"][i + 1, s], c["rcv_ddt"][i], c["rcv_ddt"][i + 1], c["frame_dt"][i], defect=defect)
        rs[i], As[i] = ddt_smooth(T, c["rcv_ddt"][i], c["rcv_ddt"][i + 1], c["ddt_weight"])
    half = T(0.5)
    out.update(r_dt_ddt=rc, A_dt_ddt=Ac, r_smooth=rs, A_smooth=As)
    out["cost"] = half * (out["r"] ** 2).sum() + half * (rc ** 2).sum() + half * (rs ** 2).sum()
    out["A_cost"] = out["cost"]
    out["cost_allow"] = T(U) * (T(K_R) * (abs(out["r"]) * out["A_r"]).sum() + T(K_CLK) * ((abs(rc) * Ac).sum() + (abs(rs) * As).sum()))
    return out


# ---------------------------------------------------------------------------------------------------------------- the comparison
def _worst(name, X, Xref, A):
    """(largest |X - Xref| / (u A) over A > 0, its index, number of entries with A == 0 where X or Xref is not exactly 0)."""
    X, Xref, A = np.asarray(X, LD), np.asarray(Xref, LD), np.asarray(A, LD)
    if A.size == 0:
        return 0.0, (), 0
    pos = A > 0
    ratio = np.zeros(A.shape)
    ratio[pos] = (np.abs(X - Xref)[pos] / (LD(U) * A[pos])).astype(float)
    ratio[pos & ~np.isfinite(X.astype(float))] = np.inf
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    bad0 = ~pos & ((X != 0) | (Xref != 0))
    return float(ratio[worst]), tuple(int(q) for q in worst), int(bad0.sum())


def compare(got, ref, label=""):
    """got: what abi.gnss_eval returns (FP64); ref: eval_case(c, LD). Returns ({r, J, clk, cost: worst ratio in u A}, failures):
    an entry outside its bound K_R / K_J / K_CLK (the cost: (K_R + its number of terms) u A_cost + cost_allow) or a structural zero that is not 0.0.
    Every observation and every entry takes part."""
    ratios, fails = {}, []
    clk_got = np.r_[np.ravel(got["r_dt_ddt"]), np.ravel(got["r_smooth"])]
    clk_ref, clk_A = np.r_[np.ravel(ref["r_dt_ddt"]), np.ravel(ref["r_smooth"])], np.r_[np.ravel(ref["A_dt_ddt"]), np.ravel(ref["A_smooth"])]
    for name, X, Xref, A, K in (("r", got["r"], ref["r"], ref["A_r"], K_R), ("J", got["J"], ref["J"], ref["A_J"], K_J), ("clk", clk_got, clk_ref, clk_A, K_CLK)):
        assert np.shape(X) == np.shape(Xref), (name, np.shape(X), np.shape(Xref))
        ratios[name], at, n0 = _worst(name, X, Xref, A)
        if not ratios[name] <= K:
            fails.append("%s %s%s: got %.17g want %.17g scale %.3g ratio %.3g > K = %g" % (label, name, list(at), float(np.asarray(X)[at]),
                                                                                        float(np.asarray(Xref)[at]), float(np.asarray(A)[at]), ratios[name], K))
        if n0:
            fails.append("%s %d structural zeros of %s are not 0.0" % (label, n0, name))
    # the cost: a sum of 2 n + 50 halves of squares, each rounded (K_R covers that) and added one by one (at most u per addition,
    # relative to the sum of these non-negative terms), on top of what the residuals' own bounds let through to first order
    err, n_terms = abs(LD(got["cost"]) - ref["cost"]), np.size(ref["r"]) + 5 * WINDOW
    ratios["cost"] = float(err / (LD(U) * ref["A_cost"])) if ref["A_cost"] > 0 else float(err != 0) * np.inf
    if not err <= (K_R + n_terms) * LD(U) * ref["A_cost"] + ref["cost_allow"]:
        fails.append("%s cost: got %.17g want %.17g, %.3g u A_cost > K = %g + %d terms and the allowance of %.3g u A_cost" % (
            label, got["cost"], float(ref["cost"]), ratios["cost"], K_R, n_terms, float(ref["cost_allow"] / (LD(U) * ref["A_cost"]))))
    return ratios, fails


def branch_failures(c, iono="case", label=""):
    """The condition on a case: every observation on the same side of every branch in FP64 and in longdouble, at least BRANCH_ROOM
    from it in both. Returns the list of violations (empty for a usable case) and {branch: set of sides seen}."""
    a, b = eval_case(c, np.float64, iono)["margins"], eval_case(c, LD, iono)["margins"]
    fails, sides = [], {}
    for k, (ma, mb) in enumerate(zip(a, b)):
        if set(ma) != set(mb):
            fails.append("%s observation %d takes different paths: %s vs %s" % (label, k, sorted(ma), sorted(mb)))
            continue
        for name in ma:
            sides.setdefault(name, set()).add(bool(mb[name] > 0))
            if not (min(abs(float(ma[name])), abs(float(mb[name]))) >= BRANCH_ROOM and (ma[name] > 0) == (mb[name] > 0)):
                fails.append("%s observation %d is %.3g (FP64) / %.3g (longdouble) from branch %s" % (label, k, float(ma[name]), float(mb[name]), name))
    return fails, sides


# ---------------------------------------------------------------------------------------------------------------- the cases
def rebase(c, k, rng, iono="case"):
    """Give observation k of case c the measurement that leaves metre / decimetre-per-second noise at its present geometry."""
    o = c["obs"][k]
    o["psr"], o["dopp"] = 0.0, 0.0
    lo = o["lower_idx"]
    e = psr_dopp(LD, o, c["iono"] if isinstance(iono, str) else iono, c["pose"][lo], c["speed_bias"][lo], c["pose"][lo + 1], c["speed_bias"][lo + 1],
                 c["rcv_dt"][o["frame"], o["sys_idx"]], c["rcv_ddt"][o["frame"]], c["yaw"], c["anc"])
    o["psr"] = float(e["r"][0] / e["J"][0, 12]) + rng.normal(0, 2.0)
    o["dopp"] = -(float(e["r"][1] / e["J"][1, 13]) + rng.normal(0, 0.2)) / o["wavelength"]


def shaped_case(seed, n_obs, lat, lon, h, below_horizon=False):
    """n_obs observations (elevations 8 .. 88 degrees) of a window anchored at lat / lon / h: the first has ratio exactly 0, the second
    exactly 1, the constellations go round 0 1 2 3, frames and both lower_idx of inner frames as gnss_cases deals them; with
    below_horizon the last satellite stands at -0.2 rad (no atmosphere, a weight from the elevation all the same)."""
    import gnss_cases as gc
    c = gc.gnss_case(seed, n_per_frame=(n_obs + WINDOW) // (WINDOW + 1), lat=lat, lon=lon, h=h)
    rng = np.random.default_rng(seed + 1000)
    c["obs"] = [c["obs"][q] for q in sorted(rng.permutation(len(c["obs"]))[:n_obs])]
    assert len(c["obs"]) == n_obs
    for k, o in enumerate(c["obs"]):
        changed = o["sys_idx"] != k % 4
        o["sys_idx"] = k % 4
        if k < 2:
            o["ratio"], changed = float(k), True
        if below_horizon and k == n_obs - 1:
            e, n, u = gc.enu_axes(lat, lon)
            o["sv_pos"], changed = c["anc"] + 2.0e7 * (np.cos(-0.2) * n + np.sin(-0.2) * u), True
        if changed:
            rebase(c, k, rng)
    return c


# name: (seed, observations, latitude, longitude, height, a satellite below the horizon). Latitudes in every interval of the Niell table and
# outside both ends, a southern one (the half-year shift), 80 degrees (phi clamps at 0.416), heights -20 m and 900 m, and the observation
# counts at the edges of gfbe_gnss_eval's 128-thread grid with the 50 clock threads behind them.
MODEL_CASES = {
    "lat04_h-20_n1": (31, 1, 4.0, 100.0, -20.0, False),
    "lat22_n63": (32, 63, 22.3, 114.17, 30.0, True),
    "lat40_n64": (33, 64, 40.0, -75.0, 120.0, False),
    "lat52_n65": (34, 65, 52.0, 13.4, 35.0, True),
    "lat68_n127": (35, 127, 68.0, -20.0, 5.0, False),
    "lat80_n128": (36, 128, 80.0, 15.0, 10.0, False),
    "south34_h900_n129": (37, 129, -33.9, 151.2, 900.0, True),
}
# the cases tests/test_gpu_gnss.py had before this model: gnss_cases.gnss_case(seed, n_per_frame, lat, lon, h) as it comes (33, 88 and 440
# observations), and its single observation moved below the horizon WITHOUT a new measurement (a residual of 1e7)
PLAIN_CASES = {"plain_21": (21, 8, 22.3, 114.17, 30.0), "plain_22": (22, 3, -33.9, 151.2, 900.0), "plain_23": (23, 40, 68.0, -20.0, 5.0)}
_cases = {}


def horizon_edge_case():
    import gnss_cases as gc
    c = gc.gnss_case(24, n_per_frame=1)
    e, n, u = gc.enu_axes(22.3, 114.17)
    c["obs"][0]["sv_pos"] = c["anc"] + 2.0e7 * (np.cos(-0.2) * n + np.sin(-0.2) * u)
    return c


def gnss_model_cases():
    """{name: case}; deterministic, cached per process."""
    if not _cases:
        import gnss_cases as gc
        for name, args in MODEL_CASES.items():
            _cases[name] = shaped_case(*args)
        for name, (seed, per, lat, lon, h) in PLAIN_CASES.items():
            _cases[name] = gc.gnss_case(seed, n_per_frame=per, lat=lat, lon=lon, h=h)
        _cases["edge_24"] = horizon_edge_case()
        _cases["edge_24_clock_only"] = dict(_cases["edge_24"], obs=[])
    return _cases


_refs = {}


def case_reference(name, iono="case"):
    """eval_case(case, longdouble) of a model case, cached per process and left unchanged."""
    key = (name, isinstance(iono, str))
    if key not in _refs:
        _refs[key] = eval_case(gnss_model_cases()[name], LD, iono)
    return _refs[key]


class ShimLib:
    """tests/host_shim.cpp's shim_gnss_eval behind the argument list of <prefix>gnss_eval, so that abi.gnss_eval drives it (prefix
    "shim_"). It returns no cost: the adaptor sums it the way gfbe_gnss_eval does."""

    def __init__(self, lib):
        self.lib = lib

    @property
    def shim_gnss_eval(self):
        import ctypes as C
        f = self.lib.shim_gnss_eval

        class _Call:
            restype = argtypes = None

            def __call__(self, ctx, n, arr, io, st, g, fdt, w, r, J, rc, rs, cost):
                status = f(n, arr, io, st, g, fdt, C.c_double(w), r, J, rc, rs)
                t = 0.0
                for buf, cnt in ((r, 2 * n), (rc, 4 * WINDOW), (rs, WINDOW)):
                    for q in range(cnt):
                        t += 0.5 * buf[q] * buf[q]
                cost[0] = t
                return status
        return _Call()
