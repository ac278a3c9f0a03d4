"""Mid-point pre-integration of the IMU and wheel streams in extended precision — the model tests/test_gpu_preint.py holds
k_preint_imu / k_preint_wheel against, and tests/test_preint_reference.py holds synth.preintegrate_*_np (FP64 numpy) and the CPU
oracle (oracle/gfo_preint.cpp) against — together with the named intervals they are compared on and the block-by-block comparison.

Model: preintegrate_imu_ld / preintegrate_wheel_ld restate IntegrationBase::{midPointIntegration, propagate}
(integration_base.h:63-167) and WheelIntegrationBase::{midPointIntegration, propagate} (wheel_integration_base.h:67-178) in
numpy.longdouble (64-bit mantissa), with Sophus::rightJacobianSO3 (sophus_utils.hpp:155-184) including its epsilon branch, the
quaternion normalised after every sample, and Eigen's toRotationMatrix polynomial for the not-yet-normalised mid-point quaternion.
They return records in the layout of gfbe_imu_preint (467) and gfbe_wheel_preint (78). They do not call synth.preintegrate_*_np.

Cases (case_names(); make_case(kind, name, variant) -> samples [n, 7], first [6], lin [6] or [4]; variant 0 is the case itself, a
further variant the same case from another seed: other samples, another `first`, another `lin`). Unless stated otherwise: gyro
rates up to 3 rad/s on all three axes at once, specific force = gravity magnitude in a random direction plus up to 5 m/s^2, wheel
velocity 0.5 .. 2 m/s per axis, ba up to 0.5, bg up to 0.05, sx, sy, sw from [0.8, 1.25] and pairwise different, td non-zero, dt
5 ms +- 30 %%.
WELL-CONDITIONED INPUTS. The bound measures a block by the size of its RESULT (S). A block that is a difference of nearly equal terms
has a rounding error set by the terms: dp_dsx of a one-sample interval is 0.5 dt (Rd e1 v0x + Rr e1 v1x), and with v1x = -v0x to 1 %%
(1 draw in 300 of a velocity of random sign) the one-ulp rounding of Rr alone is 100 u S. That is a property of such an input,
in any FP64 evaluation, not of a kernel, so the generated intervals do not contain it: within an interval every component of the
wheel velocity keeps its sign and gravity its direction, as they do over the milliseconds an interval lasts. The gyro rates change
sign freely (their sums enter through exact additions).
  empty      0 samples                                   one, two   1 and 2 samples
  frame      20 samples                                  long       200 samples, rates 5 +- 1 rad/s per axis: more than a full turn
  dt_spread  12 samples, dt from 1e-4 to 0.1 s           still      gyro exactly zero (wheel) / exactly bg (IMU): un_gyr == 0
  near_eps   two samples with |un_gyr dt| = 1e-5 (1 +- 1e-6): either side of rightJacobianSO3's branch (|phi|^2 > 1e-10)
  ground     one synth.Scenario interval (the workload's regime), wheel lin non-unit
  unit_lin   lin = [1, 1, 1, 0] / zero biases

Comparison: compare_record(got, ref, n_samples, K), with u = 2^-53 and n = max(n_samples, 1). For every block,
    max |got - ref| over the block  <=  K u n S,       S = the largest magnitude of the reference in that block
  pass-through      linearized_ba / _bg (IMU); linearized_sx .. _td, linearized_vel, linearized_gyr, vel_1, gyr_1 (wheel): the same bits
  state             sum_dt, delta_p, delta_v as blocks; delta_q: four components, S = 1
  jacobian, IMU     per 3 x 3 block. COMPARED EXACTLY (the blocks F never fills, and what the identity blocks of F carry through):
                    rows 9..14 (== rows 9..14 of the identity), the zero blocks (R,P), (R,V), (R,BA), (V,P), and (P,P) == (V,V) == I
  jacobian, wheel   per 3 x 1 block of every column. COMPARED EXACTLY: rows 3..5 of the sx and sy columns (zero)
  covariance        per 3 x 3 block (a, b) with S = sqrt(max diag_a * max diag_b) of the reference; the record's covariance minus its
                    transpose within the same bound; IMU: the blocks (BA,BG), (BG,BA) exactly zero
  n_samples == 0    every double equals the initial record (identity jacobian / zero for the wheel, zero covariance, identity
                    quaternion, sum_dt = 0, pass-through fields)
No sampling, no whole-record norm. A failure names the interval, the block and its ratio to u n S.

K (measured on the CPU by tests/test_preint_reference.py, which asserts these figures so they cannot drift): largest
|fp64 - model| / (u n S) of synth.preintegrate_*_np over all cases and both kinds, per block family:
    %(MEASURED)s
K = K_MARGIN (8) x the largest, rounded up to a power of two = %(K)g. The margin covers what a kernel may do differently from the
numpy statement: another order of the 15-term sums, fused multiply-adds, another libm.
"""
import functools
import zlib

import numpy as np

from _gfbe_import import gf
from normal_equations_np import require_extended_precision  # noqa: F401  (re-exported: the tests call preint_np.require_...)

abi, synth = gf.abi, gf.synth

LD = np.longdouble
U = 2.0 ** -53
SOPHUS_EPS = 1e-10                     # Sophus::Constants<double>::epsilon(), GF_SOPHUS_EPS
IMU_NOISE = (synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W)
WHEEL_NOISE = (synth.VEL_N_WHEEL, synth.GYR_N_WHEEL)

# Largest |fp64 numpy - model| / (u n S) per block family over all cases (tests/test_preint_reference.py asserts them)
K_MEASURED = dict(state=1.2, jacobian=1.6, covariance=3.3, symmetry=1.1)
K_MARGIN = 8.0
K = 32.0                               # K_MARGIN x max(K_MEASURED) = 26.4, rounded up to a power of two
__doc__ = __doc__ % dict(MEASURED="   ".join("%s %.3g" % kv for kv in K_MEASURED.items()), K=K)

# record layouts (include/gfbe.h)
I_SUM_DT, I_DP, I_DQ, I_DV, I_BA, I_BG, I_JAC, I_COV = 0, 1, 4, 8, 11, 14, 17, 242
W_SUM_DT, W_DP, W_DQ, W_LIN, W_LVEL, W_LGYR, W_VEL1, W_GYR1, W_JAC, W_COV = 0, 1, 4, 8, 12, 15, 18, 21, 24, 42
IMU_BLOCKS = ("P", "R", "V", "BA", "BG")
WHEEL_BLOCKS = ("p", "theta")


# ------------------------------------------------------------------ the model
def _skew(v):
    z = LD(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], LD)


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], LD)


def _qrot(q):
    """Eigen's toRotationMatrix polynomial (q need not be unit: the mid-point quaternion is used before it is normalised)."""
    x, y, z, w = q
    one, two = LD(1), LD(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], LD)


def right_jacobian_so3_ld(phi):
    """Sophus::rightJacobianSO3, sophus_utils.hpp:155-184."""
    n2 = phi @ phi
    h = _skew(phi)
    h2 = h @ h
    J = np.eye(3, dtype=LD)
    if n2 > LD(SOPHUS_EPS):
        n = np.sqrt(n2)
        J = J - h * (LD(1) - np.cos(n)) / n2
        J = J + h2 * (n - np.sin(n)) / (n2 * n)
    else:
        J = J - h / LD(2)
        J = J + h2 / LD(6)
    return J


def _mid_quat(w, dt):
    return np.array([w[0] * dt / 2, w[1] * dt / 2, w[2] * dt / 2, LD(1)], LD)


def preintegrate_imu_ld(samples, first, lin, noise=IMU_NOISE):
    """samples [n, 7] = dt, acc, gyr; first = acc_0, gyr_0; lin = ba, bg. The 467 doubles of gfbe_imu_preint, in longdouble."""
    samples, first, lin = np.asarray(samples, LD).reshape(-1, 7), np.asarray(first, LD), np.asarray(lin, LD)
    acc_0, gyr_0, ba, bg = first[:3], first[3:], lin[:3], lin[3:]
    dp, dv, dq = np.zeros(3, LD), np.zeros(3, LD), np.array([0, 0, 0, 1], LD)
    jac, cov = np.eye(15, dtype=LD), np.zeros((15, 15), LD)
    an, gn, aw, gw = [LD(x) for x in noise]
    N = np.repeat(np.array([an * an, gn * gn, an * an, gn * gn, aw * aw, gw * gw], LD), 3)     # integration_base.h:30-36
    I3 = np.eye(3, dtype=LD)
    q4, h = LD(0.25), LD(0.5)
    sum_dt = LD(0)
    for row in samples:
        dt, acc_1, gyr_1 = row[0], row[1:4], row[4:7]
        Rd = _qrot(dq)                                               # :72-78
        un_acc_0 = Rd @ (acc_0 - ba)
        un_gyr = h * (gyr_0 + gyr_1) - bg
        rq = _qmul(dq, _mid_quat(un_gyr, dt))
        Rr = _qrot(rq)
        un_acc_1 = Rr @ (acc_1 - ba)
        un_acc = h * (un_acc_0 + un_acc_1)
        rp = dp + dv * dt + h * un_acc * dt * dt
        rv = dv + un_acc * dt
        Rw, Ra0, Ra1 = _skew(un_gyr), _skew(acc_0 - ba), _skew(acc_1 - ba)   # :84-97
        ImW = I3 - Rw * dt
        F = np.zeros((15, 15), LD)                                   # :99-114
        F[0:3, 0:3] = I3
        F[0:3, 3:6] = -q4 * Rd @ Ra0 * dt * dt - q4 * Rr @ Ra1 @ ImW * dt * dt
        F[0:3, 6:9] = I3 * dt
        F[0:3, 9:12] = -q4 * (Rd + Rr) * dt * dt
        F[0:3, 12:15] = -q4 * Rr @ Ra1 * dt * dt * -dt
        F[3:6, 3:6] = ImW
        F[3:6, 12:15] = -I3 * dt
        F[6:9, 3:6] = -h * Rd @ Ra0 * dt - h * Rr @ Ra1 @ ImW * dt
        F[6:9, 6:9] = I3
        F[6:9, 9:12] = -h * (Rd + Rr) * dt
        F[6:9, 12:15] = -h * Rr @ Ra1 * dt * -dt
        F[9:12, 9:12] = I3
        F[12:15, 12:15] = I3
        V = np.zeros((15, 18), LD)                                   # :117-129
        V[0:3, 0:3] = q4 * Rd * dt * dt
        V[0:3, 3:6] = q4 * -Rr @ Ra1 * dt * dt * h * dt
        V[0:3, 6:9] = q4 * Rr * dt * dt
        V[0:3, 9:12] = V[0:3, 3:6]
        V[3:6, 3:6] = h * I3 * dt
        V[3:6, 9:12] = h * I3 * dt
        V[6:9, 0:3] = h * Rd * dt
        V[6:9, 3:6] = h * -Rr @ Ra1 * dt * h * dt
        V[6:9, 6:9] = h * Rr * dt
        V[6:9, 9:12] = V[6:9, 3:6]
        V[9:12, 12:15] = I3 * dt
        V[12:15, 15:18] = I3 * dt
        jac = F @ jac                                                # :133-134
        cov = F @ cov @ F.T + (V * N) @ V.T
        dp, dv = rp, rv                                              # propagate, :157-165
        dq = rq / np.sqrt(rq @ rq)
        sum_dt = sum_dt + dt
        acc_0, gyr_0 = acc_1, gyr_1
    return np.concatenate([[sum_dt], dp, dq, dv, ba, bg, jac.ravel(), cov.ravel()]).astype(LD)


def preintegrate_wheel_ld(samples, first, lin, noise=WHEEL_NOISE):
    """samples [n, 7] = dt, vel, gyr; first = vel_0, gyr_0; lin = sx, sy, sw, td. The 78 doubles of gfbe_wheel_preint, in longdouble."""
    samples, first, lin = np.asarray(samples, LD).reshape(-1, 7), np.asarray(first, LD), np.asarray(lin, LD)
    vel_0, gyr_0 = first[:3], first[3:]
    sx, sy, sw = lin[0], lin[1], lin[2]
    sv = np.diag(np.array([sx, sy, LD(1)], LD))                      # :77
    dp, dq = np.zeros(3, LD), np.array([0, 0, 0, 1], LD)
    jac, cov = np.zeros((6, 3), LD), np.zeros((6, 6), LD)
    vn, gn = [LD(x) for x in noise]
    N = np.repeat(np.array([vn * vn, gn * gn, vn * vn, gn * gn], LD), 3)      # :32-36
    I1, I2 = np.diag(np.array([1, 0, 0], LD)), np.diag(np.array([0, 1, 0], LD))
    q4, h = LD(0.25), LD(0.5)
    sum_dt = LD(0)
    vel_1, gyr_1 = vel_0, gyr_0
    for row in samples:
        dt, vel_1, gyr_1 = row[0], row[1:4], row[4:7]
        Rd = _qrot(dq)                                               # :78-84
        un_vel_0 = Rd @ (sv @ vel_0)
        un_gyr = h * sw * (gyr_0 + gyr_1)
        ddq = _mid_quat(un_gyr, dt)
        rq = _qmul(dq, ddq)
        Rr = _qrot(rq)
        un_vel_1 = Rr @ (sv @ vel_1)
        rp = dp + h * (un_vel_0 + un_vel_1) * dt
        Rv0, Rv1, RddT = _skew(sv @ vel_0), _skew(sv @ vel_1), _qrot(ddq).T      # :95-112
        F = np.zeros((6, 6), LD)
        F[0:3, 0:3] = np.eye(3, dtype=LD)
        F[0:3, 3:6] = -h * dt * (Rd @ Rv0 + Rr @ Rv1 @ RddT)
        F[3:6, 3:6] = RddT
        Jr = right_jacobian_so3_ld(un_gyr * dt)                      # :115
        V = np.zeros((6, 12), LD)                                    # :117-123
        V[0:3, 0:3] = h * dt * Rd @ sv
        V[0:3, 3:6] = -q4 * dt * dt * Rr @ Rv1 @ Jr
        V[0:3, 6:9] = h * dt * Rr @ sv
        V[0:3, 9:12] = V[0:3, 3:6]
        V[3:6, 3:6] = h * Jr * sw * dt
        V[3:6, 9:12] = h * Jr * sw * dt
        jac[0:3, 0] = jac[0:3, 0] + h * (Rd @ (I1 @ vel_0) + Rr @ (I1 @ vel_1)) * dt          # :134-139
        jac[0:3, 1] = jac[0:3, 1] + h * (Rd @ (I2 @ vel_0) + Rr @ (I2 @ vel_1)) * dt
        last = jac[3:6, 2].copy()
        jac[3:6, 2] = last + Jr @ (h * (gyr_0 + gyr_1) * dt)
        jac[0:3, 2] = jac[0:3, 2] + h * (Rd @ (_skew(last) @ (sv @ vel_0)) + Rr @ (_skew(jac[3:6, 2]) @ (sv @ vel_1))) * dt
        cov = F @ cov @ F.T + (V * N) @ V.T                          # :142
        dp = rp                                                      # propagate, :167-176
        dq = rq / np.sqrt(rq @ rq)
        sum_dt = sum_dt + dt
        vel_0, gyr_0 = vel_1, gyr_1
    return np.concatenate([[sum_dt], dp, dq, lin, first[:3], first[3:], vel_1, gyr_1, jac.ravel(), cov.ravel()]).astype(LD)


def model(kind, samples, first, lin):
    return (preintegrate_imu_ld if kind == "imu" else preintegrate_wheel_ld)(samples, first, lin)


def fp64_numpy(kind, samples, first, lin):
    """synth's FP64 statement of the same recursion (the second opinion the rounding floor is measured on)."""
    samples, first, lin = np.asarray(samples, float).reshape(-1, 7), np.asarray(first, float), np.asarray(lin, float)
    if kind == "imu":
        return synth.preintegrate_imu_np(samples, first, lin[:3], lin[3:], IMU_NOISE)
    return synth.preintegrate_wheel_np(samples, first, lin, WHEEL_NOISE)


def run_capi(api, kind, intervals, lins):
    """intervals [(samples, first)], lins [n, 6] / [n, 4] through abi.CApi (the product or the oracle), one linearisation per interval."""
    lins = np.asarray(lins, float)
    if kind == "imu":
        return api.preintegrate_imu(intervals, lins[:, :3], lins[:, 3:], IMU_NOISE)
    return api.preintegrate_wheel(intervals, lins, WHEEL_NOISE)


# ------------------------------------------------------------------ the cases
CASES = ("empty", "one", "two", "frame", "long", "dt_spread", "still", "near_eps", "ground", "unit_lin")
N_SAMPLES = dict(empty=0, one=1, two=2, frame=20, long=200, dt_spread=12, still=10, near_eps=2, unit_lin=10)
G_NORM = synth.G_NORM


def case_names():
    return list(CASES)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _draw_lin(kind, rng):
    if kind == "imu":
        return np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.05, 0.05, 3)])
    while True:
        s = rng.uniform(0.8, 1.25, 3)
        if min(abs(s[0] - s[1]), abs(s[0] - s[2]), abs(s[1] - s[2])) > 0.02:
            break
    td = rng.uniform(1e-3, 2e-2) * rng.choice([-1.0, 1.0])
    return np.concatenate([s, [td]])


def _draw_rows(kind, rng, n, rate=3.0, rate_mean=0.0):
    """n + 1 rows [dt, acc | vel, gyr]: row 0 is `first` (its dt is unused). Gravity keeps its direction and the wheel velocity the
    sign of each component within an interval (see WELL-CONDITIONED INPUTS in the module docstring)."""
    rows = np.zeros((n + 1, 7))
    rows[:, 0] = 5e-3 * (1.0 + rng.uniform(-0.3, 0.3, n + 1))
    down, sign = G_NORM * _unit(rng), rng.choice([-1.0, 1.0], 3)
    for r in rows:
        if kind == "imu":
            r[1:4] = down + rng.uniform(0.0, 5.0) * _unit(rng)
        else:
            r[1:4] = sign * rng.uniform(0.5, 2.0, 3)
        r[4:7] = rate_mean + rng.uniform(-rate, rate, 3)
    return rows


@functools.lru_cache(maxsize=None)
def _scenario(seed):
    return synth.Scenario(seed=seed, n_landmarks=8, use_wheel=True)


@functools.lru_cache(maxsize=None)
def _make_case(kind, name, variant):
    rng = np.random.default_rng([zlib.crc32(("%s/%s" % (kind, name)).encode()), variant])
    lin = _draw_lin(kind, rng)
    if name == "ground":
        scn = _scenario(20250708 + variant // 11)
        samples, first = (scn.imu_raw if kind == "imu" else scn.wheel_raw)[variant % 11]
        if kind == "imu":
            lin = np.concatenate([scn.ba_est, scn.bg_est]) + (rng.normal(0, 1e-3, 6) if variant else 0.0)
        return np.array(samples, float), np.array(first, float), lin
    n = N_SAMPLES[name]
    if name == "long":
        sign = rng.choice([-1.0, 1.0], 3)
        rows = _draw_rows(kind, rng, n, rate=1.0, rate_mean=5.0 * sign)
    else:
        rows = _draw_rows(kind, rng, n)
    if name == "dt_spread":
        rows[1:, 0] = np.geomspace(1e-4, 0.1, n)
    if name == "unit_lin":
        lin = np.zeros(6) if kind == "imu" else np.array([1.0, 1.0, 1.0, 0.0])
    if name == "still":
        rows[:, 4:7] = lin[3:6] if kind == "imu" else 0.0
    if name == "near_eps":
        # |un_gyr dt| = 1e-5 (1 + 1e-6) for sample 1 and 1e-5 (1 - 1e-6) for sample 2, in generic directions
        sw = 1.0 if kind == "imu" else lin[2]
        bg = lin[3:6] if kind == "imu" else np.zeros(3)
        axis = _unit(rng)
        for s, f in ((1, 1.0 + 1e-6), (2, 1.0 - 1e-6)):
            d = _unit(rng)
            d = d if d @ axis > 0 else -d                                 # (the two steps do not undo each other: dq_dsw is their sum)
            mid = f * 1e-5 / (rows[s, 0] * sw) * d + bg                   # 0.5 (gyr_0 + gyr_1) the sample needs
            rows[s, 4:7] = 2.0 * mid - rows[s - 1, 4:7]
            if s == 1:
                rows[0, 4:7] = rows[1, 4:7] = mid
    return rows[1:].copy(), rows[0, 1:].copy(), lin


def make_case(kind, name, variant=0):
    """(samples [n, 7], first [6], lin [6] | [4]) of the named interval; copies, safe to modify."""
    s, f, l = _make_case(kind, name, int(variant))
    return s.copy(), f.copy(), l.copy()


@functools.lru_cache(maxsize=None)
def _reference(kind, name, variant):
    r = model(kind, *_make_case(kind, name, variant))
    r.setflags(write=False)
    return r


def reference(kind, name, variant=0):
    """The model's record of make_case(kind, name, variant): computed once, shared, read-only."""
    return _reference(kind, name, int(variant))


def rotation_angle(kind, name, variant=0):
    """sum |un_gyr| dt of a case (rad)."""
    samples, first, lin = _make_case(kind, name, variant)
    g = np.vstack([first[3:], samples[:, 4:7]])
    mid = 0.5 * (g[:-1] + g[1:])
    mid = mid - lin[3:6] if kind == "imu" else mid * lin[2]
    return float(np.sum(np.linalg.norm(mid, axis=1) * samples[:, 0]))


# ------------------------------------------------------------------ the comparison
def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


def compare_record(got, ref, n_samples, K, label=""):
    """got: a device / oracle / numpy record (FP64); ref: the model's (longdouble). Returns (ratios, fails): the worst ratio
    |got - ref| / (u n S) per block family (state, jacobian, covariance, symmetry) and one message per violated block."""
    got = np.asarray(got)
    ref = np.asarray(ref, LD)
    imu = got.size == abi.IMU_DOUBLES
    assert got.size == ref.size and got.size in (abi.IMU_DOUBLES, abi.WHEEL_DOUBLES), (got.size, ref.size)
    n = max(int(n_samples), 1)
    unit = LD(U) * n
    ratios = dict(state=0.0, jacobian=0.0, covariance=0.0, symmetry=0.0)
    fails = []
    ref64 = ref.astype(np.float64)
    if not np.all(np.isfinite(got)):
        return dict.fromkeys(ratios, float("inf")), ["%s non-finite entries at %s" % (label, np.flatnonzero(~np.isfinite(got))[:8].tolist())]

    def exact(block, a, b):
        if not _bits_equal(np.asarray(a) + 0.0, np.asarray(b) + 0.0):         # (+ 0.0: a zero is a zero whatever its sign)
            fails.append("%s %s: not bit-identical (largest difference %.3g)" % (label, block, float(np.max(np.abs(np.asarray(a, LD) - b)))))

    def bounded(family, block, a, r, S):
        dev = float(np.max(np.abs(np.asarray(a, LD) - r)))
        S = float(S)
        if S == 0.0:
            ratio = 0.0 if dev == 0.0 else float("inf")
        else:
            ratio = dev / (float(unit) * S)
        ratios[family] = max(ratios[family], ratio)
        if not ratio <= K:
            fails.append("%s %s: |got - ref| = %.3g is %.4g x u n S (n = %d, S = %.3g), bound %g" % (label, block, dev, ratio, n, S, K))

    if int(n_samples) == 0:
        exact("initial record (no samples)", got, ref64)
        return ratios, fails

    if imu:
        exact("linearized_ba", got[I_BA:I_BA + 3], ref64[I_BA:I_BA + 3])
        exact("linearized_bg", got[I_BG:I_BG + 3], ref64[I_BG:I_BG + 3])
        state = (("sum_dt", I_SUM_DT, 1), ("delta_p", I_DP, 3), ("delta_v", I_DV, 3))
        o_q, o_jac, o_cov, dim, ncol, names = I_DQ, I_JAC, I_COV, 15, 15, IMU_BLOCKS
    else:
        for nm, o, k in (("linearized_sx/sy/sw/td", W_LIN, 4), ("linearized_vel", W_LVEL, 3), ("linearized_gyr", W_LGYR, 3),
                         ("vel_1", W_VEL1, 3), ("gyr_1", W_GYR1, 3)):
            exact(nm, got[o:o + k], ref64[o:o + k])
        state = (("sum_dt", W_SUM_DT, 1), ("delta_p", W_DP, 3))
        o_q, o_jac, o_cov, dim, ncol, names = W_DQ, W_JAC, W_COV, 6, 3, WHEEL_BLOCKS
    for nm, o, k in state:
        bounded("state", nm, got[o:o + k], ref[o:o + k], np.max(np.abs(ref[o:o + k])))
    bounded("state", "delta_q", got[o_q:o_q + 4], ref[o_q:o_q + 4], 1.0)

    J, Jr = got[o_jac:o_jac + dim * ncol].reshape(dim, ncol), ref[o_jac:o_jac + dim * ncol].reshape(dim, ncol)
    if imu:
        zero_blocks = {(1, 0), (1, 2), (1, 3), (2, 0)}
        ident_blocks = {(0, 0), (2, 2)}
        exact("jacobian rows 9..14 (bias rows)", J[9:15], np.eye(15)[9:15])
        for a in range(3):
            for b in range(5):
                blk, rblk = J[3 * a:3 * a + 3, 3 * b:3 * b + 3], Jr[3 * a:3 * a + 3, 3 * b:3 * b + 3]
                nm = "jacobian (%s,%s)" % (names[a], names[b])
                if (a, b) in zero_blocks:
                    exact(nm + " == 0", blk, np.zeros((3, 3)))
                elif (a, b) in ident_blocks:
                    exact(nm + " == I", blk, np.eye(3))
                else:
                    bounded("jacobian", nm, blk, rblk, np.max(np.abs(rblk)))
    else:
        cols = ("sx", "sy", "sw")
        for b in range(3):
            for a in range(2):
                blk, rblk = J[3 * a:3 * a + 3, b], Jr[3 * a:3 * a + 3, b]
                nm = "jacobian d%s/d%s" % (names[a], cols[b])
                if a == 1 and b < 2:
                    exact(nm + " == 0", blk, np.zeros(3))
                else:
                    bounded("jacobian", nm, blk, rblk, np.max(np.abs(rblk)))

    P, Pr = got[o_cov:o_cov + dim * dim].reshape(dim, dim), ref[o_cov:o_cov + dim * dim].reshape(dim, dim)
    nb = dim // 3
    dmax = [np.max(np.abs(np.diag(Pr)[3 * a:3 * a + 3])) for a in range(nb)]
    for a in range(nb):
        for b in range(nb):
            sl = (slice(3 * a, 3 * a + 3), slice(3 * b, 3 * b + 3))
            nm = "covariance (%s,%s)" % (names[a], names[b])
            if imu and {a, b} == {3, 4}:
                exact(nm + " == 0", P[sl], np.zeros((3, 3)))
                continue
            S = np.sqrt(dmax[a] * dmax[b])
            bounded("covariance", nm, P[sl], Pr[sl], S)
            bounded("symmetry", nm + " minus its transpose", P[sl], P.T[sl].astype(LD), S)
    return ratios, fails


def merge_ratios(worst, ratios):
    for k, v in ratios.items():
        worst[k] = max(worst.get(k, 0.0), v)
    return worst
