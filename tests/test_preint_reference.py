"""CPU checks of the extended-precision pre-integration model (tests/preint_np.py) and of the intervals the GPU comparison runs on
(tests/test_gpu_preint.py).

Rounding floor. synth.preintegrate_imu_np / _wheel_np (plain FP64 numpy) against the longdouble model on every case, through
preint_np.compare_record: the worst |fp64 - model| / (u n S) per block family is the rounding floor of an FP64 evaluation of these
formulas (it includes (1 - cos n) / n^2 next to rightJacobianSO3's branch, case near_eps: the cancellation costs 1e-6 of Jr's
first-order term, which the outputs see only through Jr Jr^T and through Jr applied to its own axis, where that term drops out).
Measured (asserted below, so that it cannot drift):
    %(FLOOR)s
    per case, worst family:  one 3.3   two 1.5   frame 0.71   long 0.17   dt_spread 0.26   still 0.30   near_eps 1.6   ground 0.41
    unit_lin 0.52   (the ratio falls with n: the errors of successive samples do not add up in one direction)
preint_np.K = 8 x the largest, rounded up to a power of two = %(K)g: fixed here, from the CPU, before any device run.

Oracle. oracle/gfo_preint.cpp through the per-interval-lin wrappers of abi.CApi, all cases in one ragged call, under the same K.

The jacobian as a derivative (model alone). On frame-like intervals (20 samples, dt = 1 ms, smooth rates up to 1 rad/s) the nine
blocks the factors read — dp_dba, dp_dbg, dq_dbg, dv_dba, dv_dbg (imu_raw), dp_dsx, dp_dsy, dp_dsw, dq_dsw (wheel_raw) — against
central differences of the model's delta_p, delta_v and 2 vec(q(lin)^-1 q(lin +- h)) with h = 1e-6 in longdouble. The recursion is
first order in dt, so the agreement is not to rounding. Measured gap, max |difference quotient - block| / max |block|:
    %(GAPS)s
Asserted: 4 x these. dp_dba, dv_dba, dp_dsx and dp_dsy are exact derivatives of the recursion (delta_p and delta_v are linear in ba,
sx and sy, and the rotation does not depend on them): their gap is the rounding of the difference quotient itself, u_longdouble / h.
The blocks that go through the rotation (the bg and sw columns) are first order in dt = 1 ms: a few 1e-4 to 1e-3 of the block. Every
bound is far below the 0.1 of the block's scale that a wrong sign, a transposed block or a swapped column would cost, and no block
of the reference's formula turned out not to be the derivative it is used as.
"""
import numpy as np
import pytest

import preint_np as pn

LD = pn.LD
KINDS = ("imu", "wheel")
# max |difference quotient - block| / max |block| of the model, measured by test_jacobian_blocks_are_the_derivatives (which prints them)
DERIVATIVE_GAP = dict(dp_dba=8.1e-13, dp_dbg=4.8e-4, dq_dbg=3.7e-4, dv_dba=9.1e-13, dv_dbg=4.8e-4, dp_dsx=1.2e-13, dp_dsy=1.5e-12, dp_dsw=1.1e-3, dq_dsw=1.2e-3)
__doc__ = __doc__ % dict(FLOOR="   ".join("%s %.3g" % kv for kv in pn.K_MEASURED.items()), K=pn.K,
                         GAPS="   ".join("%s %.2g" % kv for kv in DERIVATIVE_GAP.items()))


@pytest.fixture(scope="module", autouse=True)
def _extended_precision():
    pn.require_extended_precision()


def test_bound_constants_follow_from_the_measurement():
    top = pn.K_MARGIN * max(pn.K_MEASURED.values())
    assert pn.K == 2.0 ** np.ceil(np.log2(top)) and pn.K_MARGIN == 8.0


@pytest.mark.parametrize("kind", KINDS)
def test_cases_are_what_their_names_say(kind):
    assert pn.case_names() == ["empty", "one", "two", "frame", "long", "dt_spread", "still", "near_eps", "ground", "unit_lin"]
    n = {name: len(pn.make_case(kind, name)[0]) for name in pn.case_names()}
    assert (n["empty"], n["one"], n["two"], n["frame"], n["long"], n["dt_spread"], n["near_eps"]) == (0, 1, 2, 20, 200, 12, 2)
    assert pn.rotation_angle(kind, "long") > 2 * np.pi
    s, f, lin = pn.make_case(kind, "dt_spread")
    assert s[0, 0] == 1e-4 and abs(s[-1, 0] - 0.1) < 1e-15
    s, f, lin = pn.make_case(kind, "frame")
    assert len(set(np.round(s[:, 0], 9))) == 20 and s[:, 0].min() >= 3.5e-3 and s[:, 0].max() <= 6.5e-3
    assert (np.abs(s[:, 4:7]).max(axis=0) > 1.5).all()                                  # all three axes at once
    if kind == "imu":
        assert np.abs(lin[:3]).max() > 0.05 and np.abs(lin[3:]).max() > 0.005
    else:
        assert 0.8 <= lin[:3].min() and lin[:3].max() <= 1.25 and lin[3] != 0.0
        assert min(abs(lin[0] - lin[1]), abs(lin[0] - lin[2]), abs(lin[1] - lin[2])) > 0.02
    # still: un_gyr is exactly zero, sample after sample
    s, f, lin = pn.make_case(kind, "still")
    g = np.vstack([f[3:], s[:, 4:7]])
    un_gyr = 0.5 * (g[:-1] + g[1:]) - lin[3:6] if kind == "imu" else 0.5 * lin[2] * (g[:-1] + g[1:])
    assert not un_gyr.any()
    q = pn.reference(kind, "still")[pn.I_DQ:pn.I_DQ + 4]
    assert q.tolist() == [0, 0, 0, 1]
    # near_eps: one sample either side of |phi|^2 > 1e-10, in FP64 as in the model
    s, f, lin = pn.make_case(kind, "near_eps")
    g = np.vstack([f[3:], s[:, 4:7]])
    for prec in (np.float64, LD):
        gg, dt, ll = g.astype(prec), s[:, 0].astype(prec), lin.astype(prec)
        mid = prec(0.5) * (gg[:-1] + gg[1:])
        phi = ((mid - ll[3:6]) if kind == "imu" else mid * ll[2]) * dt[:, None]
        n2 = np.sum(phi * phi, axis=1)
        assert n2[0] > prec(pn.SOPHUS_EPS) > n2[1] and abs(float(n2[0]) / 1e-10 - 1) < 1e-5 and abs(float(n2[1]) / 1e-10 - 1) < 1e-5
    # every variant has its own first and lin
    a, b = pn.make_case(kind, "frame", 0), pn.make_case(kind, "frame", 1)
    assert not np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])
    assert pn.make_case(kind, "unit_lin")[2].tolist() == ([0.0] * 6 if kind == "imu" else [1.0, 1.0, 1.0, 0.0])
    assert not np.allclose(pn.make_case("wheel", "ground")[2][:3], 1.0)


@pytest.mark.parametrize("name", pn.case_names())
@pytest.mark.parametrize("kind", KINDS)
def test_fp64_numpy_is_within_the_measured_floor(kind, name):
    """The measurement of K: synth's FP64 recursion against the model, block by block."""
    s, f, lin = pn.make_case(kind, name)
    ratios, fails = pn.compare_record(pn.fp64_numpy(kind, s, f, lin), pn.reference(kind, name), len(s), pn.K, "%s %s:" % (kind, name))
    print("%-5s %-9s n = %3d   " % (kind, name, len(s)) + "   ".join("%s %.3g" % kv for kv in ratios.items()))
    assert not fails, "\n".join(fails)
    for fam, r in ratios.items():
        assert r <= pn.K_MEASURED[fam], (fam, r)


def test_the_measured_floor_is_reached():
    """K_MEASURED is the measurement, not a loose cover of it: each family's figure is reached to within 15 %."""
    worst = {}
    for kind in KINDS:
        for name in pn.case_names():
            s, f, lin = pn.make_case(kind, name)
            pn.merge_ratios(worst, pn.compare_record(pn.fp64_numpy(kind, s, f, lin), pn.reference(kind, name), len(s), pn.K)[0])
    print("floor:", worst)
    for fam, r in worst.items():
        assert 0.85 * pn.K_MEASURED[fam] <= r <= pn.K_MEASURED[fam], (fam, r)


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_matches_the_model(oracle, kind):
    """gfo_preintegrate_* with one linearisation point per interval: every case in one ragged call, then each alone."""
    names = pn.case_names()
    cases = [pn.make_case(kind, name) for name in names]
    got = pn.run_capi(oracle, kind, [(s, f) for s, f, _ in cases], [lin for _, _, lin in cases])
    fails, worst = [], {}
    for k, name in enumerate(names):
        ratios, f = pn.compare_record(got[k], pn.reference(kind, name), len(cases[k][0]), pn.K, "%s %s (interval %d):" % (kind, name, k))
        fails += f
        pn.merge_ratios(worst, ratios)
        alone = pn.run_capi(oracle, kind, [cases[k][:2]], [cases[k][2]])
        assert np.array_equal(alone[0], got[k]), name
    print("oracle %s: worst ratios %s" % (kind, {k: round(v, 2) for k, v in worst.items()}))
    assert not fails, "\n".join(fails)


def test_one_dimensional_lin_keeps_its_meaning(oracle):
    """A 1-D linearisation point is the one of every interval (what every caller outside these tests passes)."""
    iv = [pn.make_case("imu", n)[:2] for n in ("frame", "two", "empty")]
    lin = pn.make_case("imu", "frame")[2]
    a = oracle.preintegrate_imu(iv, lin[:3], lin[3:], pn.IMU_NOISE)
    b = oracle.preintegrate_imu(iv, np.tile(lin[:3], (3, 1)), np.tile(lin[3:], (3, 1)), pn.IMU_NOISE)
    assert np.array_equal(a, b)
    iw = [pn.make_case("wheel", n)[:2] for n in ("frame", "two", "empty")]
    linw = pn.make_case("wheel", "frame")[2]
    assert np.array_equal(oracle.preintegrate_wheel(iw, linw, pn.WHEEL_NOISE), oracle.preintegrate_wheel(iw, np.tile(linw, (3, 1)), pn.WHEEL_NOISE))
    with pytest.raises(ValueError):
        oracle.preintegrate_wheel(iw, np.tile(linw, (2, 1)), pn.WHEEL_NOISE)
    with pytest.raises(ValueError):
        oracle.preintegrate_imu(iv, np.tile(lin[:3], (3, 1)), lin[3:], pn.IMU_NOISE)


def test_compare_record_sees_what_it_should():
    """The comparison itself: a swapped column, a transposed block, a stale pass-through, an asymmetric covariance and a non-initial
    empty record each fail, and the message names the block."""
    s, f, lin = pn.make_case("imu", "frame")
    ref = pn.reference("imu", "frame")
    good = np.asarray(ref, float)
    assert not pn.compare_record(good, ref, len(s), pn.K)[1]

    def fails_with(rec, word, n=len(s), r=ref):
        fails = pn.compare_record(rec, r, n, pn.K, "iv 7:")[1]
        assert fails and all(m.startswith("iv 7:") for m in fails) and any(word in m for m in fails), fails

    J = good[pn.I_JAC:pn.I_JAC + 225].reshape(15, 15)
    bad = good.copy(); Jb = bad[pn.I_JAC:pn.I_JAC + 225].reshape(15, 15); Jb[0:3, 12:15] = J[0:3, 12:15].T
    fails_with(bad, "jacobian (P,BG)")
    bad = good.copy(); Jb = bad[pn.I_JAC:pn.I_JAC + 225].reshape(15, 15); Jb[6:9, 9] = J[6:9, 10]; Jb[6:9, 10] = J[6:9, 9]
    fails_with(bad, "jacobian (V,BA)")
    bad = good.copy(); bad[pn.I_JAC + 9 * 15 + 3] = 1e-300
    fails_with(bad, "rows 9..14")
    bad = good.copy(); bad[pn.I_BG] = np.nextafter(bad[pn.I_BG], 1.0)
    fails_with(bad, "linearized_bg")
    bad = good.copy(); bad[pn.I_COV + 0 * 15 + 7] *= 1 + 1e-9
    fails_with(bad, "minus its transpose")
    bad = good.copy(); bad[pn.I_DQ + 3] += 100 * pn.K * pn.U
    fails_with(bad, "delta_q")
    e = np.asarray(pn.reference("wheel", "empty"), float)
    bad = e.copy(); bad[pn.W_COV] = 1e-300
    fails_with(bad, "initial record", 0, pn.reference("wheel", "empty"))
    w = np.asarray(pn.reference("wheel", "frame"), float)
    bad = w.copy(); Jw = bad[pn.W_JAC:pn.W_JAC + 18].reshape(6, 3); Jw[0:3, [0, 1]] = Jw[0:3, [1, 0]]
    fails_with(bad, "jacobian dp/dsx", 20, pn.reference("wheel", "frame"))


# ------------------------------------------------------------------ the jacobian as a derivative
def _smooth_interval(kind, seed):
    """20 samples at dt = 1 ms, smooth signals, rates up to 1 rad/s."""
    rng = np.random.default_rng(seed)
    t = np.arange(21) * 1e-3
    ph, fr = rng.uniform(0, 6.28, (2, 3)), rng.uniform(5.0, 30.0, (2, 3))
    gyr = rng.uniform(0.3, 1.0, 3) * np.sin(fr[0] * t[:, None] + ph[0])
    if kind == "imu":
        d = rng.normal(size=3)
        a = pn.G_NORM * d / np.linalg.norm(d) + 2.0 * np.sin(fr[1] * t[:, None] + ph[1])
        lin = np.concatenate([rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.02, 0.02, 3)])
    else:
        a = rng.uniform(0.5, 1.5, 3) * np.sin(fr[1] * t[:, None] + ph[1]) + rng.uniform(-1, 1, 3)
        lin = np.array([1.1, 0.9, 1.2, 0.004]) + np.concatenate([rng.uniform(-0.05, 0.05, 3), [0.0]])
    rows = np.hstack([np.full((21, 1), 1e-3), a, gyr])
    return rows[1:], rows[0, 1:], lin


def _qinv_mul_vec2(q0, q1):
    """2 vec(q0^-1 q1) for unit quaternions (x y z w)."""
    c = np.array([-q0[0], -q0[1], -q0[2], q0[3]], LD)
    return 2 * pn._qmul(c, q1)[:3]


def _difference_quotients(kind, samples, first, lin, cols, h=LD(1e-6)):
    """Central differences of delta_p, delta_q (as 2 vec(q^-1 q+-)) and delta_v (IMU) with respect to lin[cols]."""
    lin = np.asarray(lin, LD)
    q0 = pn.model(kind, samples, first, lin)[pn.I_DQ:pn.I_DQ + 4]
    out = {}
    for c in cols:
        lp, lm = lin.copy(), lin.copy()
        lp[c] += h
        lm[c] -= h
        rp, rm = pn.model(kind, samples, first, lp), pn.model(kind, samples, first, lm)
        d = dict(p=(rp[pn.I_DP:pn.I_DP + 3] - rm[pn.I_DP:pn.I_DP + 3]) / (2 * h),
                 q=(_qinv_mul_vec2(q0, rp[pn.I_DQ:pn.I_DQ + 4]) - _qinv_mul_vec2(q0, rm[pn.I_DQ:pn.I_DQ + 4])) / (2 * h))
        if kind == "imu":
            d["v"] = (rp[pn.I_DV:pn.I_DV + 3] - rm[pn.I_DV:pn.I_DV + 3]) / (2 * h)
        out[c] = d
    return out


def _derivative_gaps(seed):
    gaps = {}
    s, f, lin = _smooth_interval("imu", seed)
    rec = pn.model("imu", s, f, lin)
    J = rec[pn.I_JAC:pn.I_JAC + 225].reshape(15, 15)
    fd = _difference_quotients("imu", s, f, lin, range(6))
    for name, what, r0, c0 in (("dp_dba", "p", 0, 9), ("dp_dbg", "p", 0, 12), ("dq_dbg", "q", 3, 12), ("dv_dba", "v", 6, 9), ("dv_dbg", "v", 6, 12)):
        D = np.stack([fd[c0 - 9 + k][what] for k in range(3)], axis=1)          # lin = ba (cols 9..11 of the state), bg (12..14)
        blk = J[r0:r0 + 3, c0:c0 + 3]
        gaps[name] = float(np.max(np.abs(D - blk)) / np.max(np.abs(blk)))
    s, f, lin = _smooth_interval("wheel", seed)
    rec = pn.model("wheel", s, f, lin)
    Jw = rec[pn.W_JAC:pn.W_JAC + 18].reshape(6, 3)
    fd = _difference_quotients("wheel", s, f, lin, range(3))
    for name, what, r0, c in (("dp_dsx", "p", 0, 0), ("dp_dsy", "p", 0, 1), ("dp_dsw", "p", 0, 2), ("dq_dsw", "q", 3, 2)):
        blk = Jw[r0:r0 + 3, c]
        gaps[name] = float(np.max(np.abs(fd[c][what] - blk)) / np.max(np.abs(blk)))
    return gaps


def test_jacobian_blocks_are_the_derivatives():
    worst = {}
    for seed in (1, 2, 3):
        for k, v in _derivative_gaps(seed).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("derivative gaps:", "   ".join("%s %.3g" % kv for kv in worst.items()))
    for k, v in worst.items():
        assert 4 * DERIVATIVE_GAP[k] < 0.1
        assert v <= 4 * DERIVATIVE_GAP[k], (k, v)
