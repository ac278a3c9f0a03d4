"""k_preint_imu / k_preint_wheel (gfbe_preintegrate_imu / _wheel) against the extended-precision model of tests/preint_np.py, block by
block (preint_np.compare_record: pass-through fields bit-exact, every other block within K u n S of the model, structural zeros
and identities exact, the covariance symmetric), on the named intervals of that module — every one with its own `first` and its
own linearisation point:

  test_each_case_alone                       n_interval = 1, one launch per case
  test_ragged_batch_of_257                   every case at shuffled places of one call (257 workgroups; empty intervals first, last and
                                             twice in a row in the middle; at most 3 000 samples); the variant that also ran alone
                                             is bit-identical to that run
  test_all_intervals_empty                   offset = [0, 0, 0, 0]: three initial records
  test_small_call_right_behind_a_large_one   the scratch and its pinned mirror reused by a smaller call: the same bits as on a fresh context
  test_bad_offsets_and_missing_arrays_are_refused   the host check of preint_common: GFBE_BAD_INPUT with a text, outputs untouched

K = %(K)g comes from the CPU (tests/test_preint_reference.py: 8 x the rounding floor of the FP64 numpy statement), not from the device.

%(MEASURED)s
"""
import ctypes as C

import numpy as np
import pytest

import preint_np as pn
from _gfbe_import import gf

abi = gf.abi
pytestmark = pytest.mark.gpu
KINDS = ("imu", "wheel")

MEASURED = """Worst |got - model| / (u n S) per block family. NOT YET A DEVICE FIGURE: no MI355X could be had while this file was written, so the
rows below come from the two kernels' statements compiled for the host (the same gfbe_math.h / gfbe_factors.h functions in the same
order, serial loops for the lanes, no fused multiply-add — the build whose factor blocks test_gpu_parity.py finds bit-identical to
the device's). The device can differ from them through its sqrt, sin and cos only. Replace them with the device's own figures (run
this file with -s) at the next opportunity; a ratio above K is a finding to explain from the kernel's code, K does not move.
  launch shape               kind    state  jacobian  covariance  symmetry   worst case
  alone (n_interval = 1)     imu      1.1      1.1        3.3        1.5     one (covariance), two (symmetry)
  alone (n_interval = 1)     wheel    0.96     1.6        1.2        0.01    near_eps (jacobian)
  ragged call of 257         imu      2.9      3.3        5.2        2.6     one, two (the shortest intervals: n = 1, 2)
  ragged call of 257         wheel    1.7      7.9        5.8        0.04    one (dp_dsw: a cross product of nearly parallel vectors)
Sensitivity (each mutation of gfbe_preint.hip applied to that host statement once, numbers only, none committed; `old`: whether
test_gpu_parity.py::test_preintegration_matches_oracle, with its inputs and rtol = 1e-10, sees it):
  mutation                                     test_each_case_alone fails             intervals of the 257 failing     old
  lin + 6 * iv read as lin (IMU)               none (one interval: iv = 0)            imu 256                          no
  sv = diagm(lsy, lsx, 1)                      wheel: all but empty, unit_lin         wheel 222                        no
  lsw dropped from un_gyr (wheel)              wheel: all but empty, still, unit_lin  wheel 191                        no
  F / V fill loop bounded at 256 entries       imu: all but empty                     imu 253                          imu
  V columns 9..11 (IMU) left zero              imu: all but empty                     imu 253                          imu
  dt of sample s - 1 in F(3,3)                 imu: two, frame, long, dt_spread,      imu 159                          no
                                               near_eps, unit_lin (ground: one dt)
  qnormalize dropped                           both: all but empty, still             imu 222, wheel 222               both
(F / V fill bounded at 256: the host statement keeps the previous sample's V where the kernel would keep stale LDS.)"""
__doc__ = __doc__ % dict(K=pn.K, MEASURED=MEASURED)


@pytest.fixture(scope="module")
def be():
    pn.require_extended_precision()
    b = gf.Backend(device=0)
    yield b
    b.close()


def run(api, kind, cases):
    """cases: [(samples, first, lin)] -> records [n, 467 | 78] of ONE call."""
    return pn.run_capi(api, kind, [(s, f) for s, f, _ in cases], [lin for _, _, lin in cases])


def fmt(ratios):
    return "   ".join("%s %.3g" % kv for kv in ratios.items())


@pytest.mark.parametrize("name", pn.case_names())
@pytest.mark.parametrize("kind", KINDS)
def test_each_case_alone(be, kind, name):
    case = pn.make_case(kind, name)
    got = run(be, kind, [case])
    ratios, fails = pn.compare_record(got[0], pn.reference(kind, name), len(case[0]), pn.K, "%s %s alone:" % (kind, name))
    print("%-5s %-9s alone    n = %3d   %s" % (kind, name, len(case[0]), fmt(ratios)))
    assert not fails, "\n".join(fails)


def batch_of_257(kind):
    """(name, variant) per place: `empty` at 0, 128, 129 and 256 (four variants), `long` twice, the other eight cases in variants 0..31
    at shuffled places. Variant 0 of every case is in it once."""
    rest = [n for n in pn.case_names() if n not in ("empty", "long")]
    pool = [("long", 0), ("long", 1)] + [(n, v) for v in range(32) for n in rest]
    pool = pool[:253]
    order = np.random.default_rng(257).permutation(len(pool))
    places = [pool[q] for q in order]
    places = [("empty", 0)] + places[:127] + [("empty", 1), ("empty", 2)] + places[127:] + [("empty", 3)]
    assert len(places) == 257 and places[128][0] == places[129][0] == places[256][0] == "empty"
    return places


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_batch_of_257(be, kind):
    places = batch_of_257(kind)
    cases = [pn.make_case(kind, n, v) for n, v in places]
    assert sum(len(c[0]) for c in cases) <= 3000
    assert {n for n, v in places if v == 0} == set(pn.case_names())
    got = run(be, kind, cases)
    fails, worst = [], {}
    for k, (name, v) in enumerate(places):
        ratios, f = pn.compare_record(got[k], pn.reference(kind, name, v), len(cases[k][0]), pn.K,
                                      "%s interval %d of 257 (%s, variant %d):" % (kind, k, name, v))
        fails += f
        pn.merge_ratios(worst.setdefault(name, {}), ratios)
        if v == 0:                                   # the same inputs alone: the same bits at another place of another grid
            alone = run(be, kind, [cases[k]])
            if not np.array_equal(alone[0].view(np.int64), got[k].view(np.int64)):
                fails.append("%s interval %d (%s): differs from the same interval integrated alone at doubles %s" %
                             (kind, k, name, np.flatnonzero(alone[0] != got[k])[:8].tolist()))
    for name, r in worst.items():
        print("%-5s %-9s B = 257   %s" % (kind, name, fmt(r)))
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("kind", KINDS)
def test_all_intervals_empty(be, kind):
    cases = [pn.make_case(kind, "empty", v) for v in range(3)]
    got = run(be, kind, cases)                       # (raises unless the status is GFBE_OK)
    fails = []
    for k in range(3):
        fails += pn.compare_record(got[k], pn.reference(kind, "empty", k), 0, pn.K, "%s empty interval %d of 3:" % (kind, k))[1]
    assert not fails, "\n".join(fails)
    if kind == "wheel":                              # the initial wheel record carries `first` as linearized_* and as vel_1 / gyr_1
        for k in range(3):
            assert np.array_equal(got[k][pn.W_LVEL:pn.W_LVEL + 6], cases[k][1]) and np.array_equal(got[k][pn.W_VEL1:pn.W_VEL1 + 6], cases[k][1])


@pytest.mark.parametrize("kind", KINDS)
def test_small_call_right_behind_a_large_one(kind):
    pn.require_extended_precision()
    large = [pn.make_case(kind, n, v) for n, v in batch_of_257(kind)]
    small = [pn.make_case(kind, "frame", 40), pn.make_case(kind, "two", 40)]
    used, fresh = gf.Backend(device=0), gf.Backend(device=0)
    try:
        run(used, kind, large)
        behind = run(used, kind, small)
        alone = run(fresh, kind, small)
    finally:
        used.close()
        fresh.close()
    assert np.array_equal(behind.view(np.int64), alone.view(np.int64)), np.flatnonzero((behind != alone).ravel())[:8].tolist()
    fails = []
    for k, (name, c) in enumerate(zip(("frame", "two"), small)):
        fails += pn.compare_record(behind[k], pn.reference(kind, name, 40), len(c[0]), pn.K, "%s %s behind the batch of 257:" % (kind, name))[1]
    assert not fails, "\n".join(fails)


def raw_call(be, kind, n, offset, samples, first, lin, noise, out):
    """The C entry point with the arrays as given (None: a NULL pointer). Returns the status."""
    f = getattr(be.lib, "gfbe_preintegrate_" + kind)
    f.restype = abi.c_i
    ptr = lambda a: None if a is None else abi._pd(a)        # noqa: E731
    rec = C.POINTER(abi.ImuPreint if kind == "imu" else abi.WheelPreint)
    return f(be.ctx, n, None if offset is None else abi._pi(offset), ptr(samples), ptr(first), ptr(lin), ptr(noise),
             C.cast(out.ctypes.data, rec))


@pytest.mark.parametrize("kind", KINDS)
def test_bad_offsets_and_missing_arrays_are_refused(be, kind):
    """preint_common looks at every offset and every pointer on the host and returns before anything is copied or launched: the status
    is GFBE_BAD_INPUT, gfbe_last_error says why, `out` keeps its bytes — and the next good call on the context is right."""
    names = ("frame", "two", "one")
    cases = [pn.make_case(kind, n) for n in names]
    samples = np.ascontiguousarray(np.concatenate([c[0] for c in cases]))
    first = np.ascontiguousarray(np.array([c[1] for c in cases]))
    lin = np.ascontiguousarray(np.array([c[2] for c in cases]))
    noise = np.ascontiguousarray(np.array(pn.IMU_NOISE if kind == "imu" else pn.WHEEL_NOISE))
    good = np.array([0, 20, 22, 23], np.int32)
    width = abi.IMU_DOUBLES if kind == "imu" else abi.WHEEL_DOUBLES

    def refused(word, offset=good, samples=samples, first=first, lin=lin, noise=noise, n=3):
        out = np.full((3, width), 7.0)
        rc = raw_call(be, kind, n, offset, samples, first, lin, noise, out)
        assert rc == abi.BAD_INPUT, (word, rc)
        assert word in be._err(), (word, be._err())
        assert (out == 7.0).all(), word

    refused("negative", offset=np.array([-1, 20, 22, 23], np.int32))
    refused("must not decrease", offset=np.array([0, 20, 19, 23], np.int32))
    refused("must not decrease", offset=np.array([0, 20, 22, 21], np.int32))
    refused("must not decrease", offset=np.array([5, 0, 22, 23], np.int32))
    refused("NULL", first=None)
    refused("NULL", lin=None)
    refused("NULL", noise=None)
    refused("NULL", samples=None)
    refused("NULL", offset=None)
    refused("n_interval", n=0)
    out = np.zeros((3, width))
    assert raw_call(be, kind, 3, good, samples, first, lin, noise, out) == abi.OK
    fails = []
    for k, name in enumerate(names):
        fails += pn.compare_record(out[k], pn.reference(kind, name), len(cases[k][0]), pn.K, "%s %s after the refused calls:" % (kind, name))[1]
    assert not fails, "\n".join(fails)
    # no samples at all: a NULL samples array is then allowed
    out = np.full((2, width), 7.0)
    assert raw_call(be, kind, 2, np.zeros(3, np.int32), None, first, lin, noise, out) == abi.OK
    assert not pn.compare_record(out[1], pn.model(kind, np.zeros((0, 7)), first[1], lin[1]), 0, pn.K)[1]
