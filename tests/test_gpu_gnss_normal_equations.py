"""The GNSS, plane and anchor share of the assembled normal equations — H (all 246 rows, lower triangle) and g after one iteration,
read through gfbe_debug_vector — against the extended-precision reference of tests/normal_equations_np.py,
whose GNSS blocks come from the longdouble model of the factors (tests/gnss_np.py), entry by entry:

    |X_dev[i, j] - X_ref[i, j]| <= K u A_X[i, j]      (exactly 0.0 where A_X is zero; K = %(K)g, the bound of test_gpu_normal_equations.py)

plus, in g, the first-order allowance of the GNSS residuals' own rounding (sum |J| K_R u A_r; normal_equations_np._Acc.add_gnss) and,
where the IMU factors reach, theirs. This is what sits between the factor pins (tests/test_gpu_gnss.py) and the solve pins (which
take the H the device assembled): k_gnss's index maps gn_tan / gn_frames / gn_col, its closed-form clock chain, the staged and the
unstaged sums, 1 to 16 workgroups per window, sub 0 and the speculative pair sub 1 + sub 2, the GNSS work item of k_lin_small, and
plane_anchor_term in its three assembly variants. d.H is read after the dense solve: k_solve, k_solve_chain_wide (GNSS windows)
and k_solve_big (GNSS + plane: the dense part no longer fits the chain kernel) take H through a pointer to const and factor copies in
LDS / their own workspace, so H is as assembled (ground-fusion2_amd/csrc/gfbe_solve.hip: solve_chain_body, k_solve_big).

Windows (gnss_window_cases.NE_COUNTS, 60 landmarks each; observations per frame): 8 everywhere; none with the window ready (the clock
chain alone); one in the whole window; empty frames between full ones; everything in one frame; 256 / 257 (GN_ITEM_MAX_OBS) and
320 / 321 (GN_LDS_OBS) in total; one constellation; pose and speed-bias of frame 4 constant (structural zeros); the anchor; GNSS +
PlaneFactors + anchor; the lowspeed window (no GNSS dim in the program); PlaneFactors with free and with constant plane blocks; the
second window with its ~95-dim prior over GNSS blocks; pose 0 constant (88 and 257 observations). The windows with observations in
every frame have them in frame 10 and with both lower_idx in every inner frame (asserted on the CPU for n8, n257, n321; gaps has both
lower_idx in its occupied inner frames; clock_only, one_obs and one_frame cannot). That every observation keeps its distance from the branches of the factor arithmetic is asserted on the
CPU (tests/test_gnss_reference.py); none is left out. The entries the visual factors reach carry the allowance of the reference's own
visual blocks (normal_equations_np.VIS_BLOCK_TOL: a pose pair of these small windows can have ONE factor). The landmark elimination
term E, eg is no subject here — no GNSS, plane or anchor factor reaches it, and it is held on the windows of
tests/test_gpu_normal_equations.py —; it takes part in the bit-identity of a window with itself.

Launch shapes: alone (16 workgroups per window); a batch of 5 (12 workgroups: 7874 entries over 6144 threads, a partial second pass);
a batch of 33 with plain windows mixed in (one workgroup; the throughput assembly k_visasm with plane_anchor_term); the 321-observation
window next to staged ones (one workgroup for all, LDS capped at 320). A window that occurs twice in a batch is bit-identical to
itself. The second linearisation (max_num_iterations = 2 against the reference at the state downloaded after one iteration, in the two
windows whose pose 0 is constant) with speculative_linearization 1 (evaluation at the candidate in sub 1 — the work item of
k_lin_small up to 256 observations, a launch of k_gnss above —, sums in sub 2) and 0; the clock-by-clock entries, which only GNSS and
the prior reach, bit-equal between the two.

Measured on an MI355X (worst |X_dev - X_ref| / (u A_X) per array; g beyond its allowances):
%(MEASURED)s
"""
import numpy as np
import pytest

import gnss_window_cases as gw
import normal_equations_np as ne
from _gfbe_import import gf

abi = gf.abi
pytestmark = pytest.mark.gpu

MEASURED = """  launch shape                                    H       g      worst case
  alone (16 workgroups of k_gnss)              15.0    1.64     H: second   g: all_three
  B = 5 (12 workgroups, partial second pass)    5.5    0.64     H: gaps
  B = 33 (one workgroup; k_visasm)             15.0    1.64
  B = 4 with the 321-observation window         2.7    0.64
  second linearisation, spec 1 and 0 alike      0.0    0.0      (inside the state allowance everywhere; without it H 15706 / 11774, g 82 / 594
                                                                 u A in n8_hold0 / n257_hold0: inertial and wheel entries, 1e-12 of their scale)
(bound K = 1024; the GNSS share sits where a plain FP64 loop does, the figures are the visual and inertial entries'.) The allowance of
the visual blocks was introduced after three windows had left K in a pose pair with a single visual factor (anchor 4993, one_obs 1806,
second 1240 u A); the host build of the device's visual arithmetic differs from the oracle's blocks by the same amount on the CPU (what
it costs, and where it is zero: normal_equations_np.VIS_BLOCK_TOL).
Sensitivity (each built once, not committed), failing tests of the 25 here / of the 9 of tests/test_gpu_gnss_solve.py: gn_frames returning
hi = f 19 / 6; a group stride that skips the last partial pass 4 / 4 (here: n321 alone, B = 5, B = 33, the unstaged batch); sMeta without
the constellation bits 19 / 6 (both second-linearisation tests see the first and the third). tests/test_gpu_gnss.py (the stand-alone evaluator) sees none of them."""
__doc__ = __doc__ % dict(K=ne.K, MEASURED=MEASURED)
CLK0 = abi.block_tangent_offset(abi.BLK_RCV_DT0)


@pytest.fixture(scope="module")
def backends():
    ne.require_extended_precision()
    made = {}

    def get(spec=1, iters=1):
        if (spec, iters) not in made:
            o = abi.default_options()
            o.max_num_iterations = iters
            o.speculative_linearization = spec
            made[(spec, iters)] = gf.Backend(device=0, options=o)
        return made[(spec, iters)]
    yield get
    for b in made.values():
        b.close()


def check_window(batch, w, name, oracle, label, worst):
    snap, ev, ref = gw.ne_reference(name, oracle)
    got = ne.device_system(batch, w)
    ratios, fails = ne.compare_system(got, ref, ne.K, "%s, %s:" % (name, label), names=("H", "g"), vis_block_tol=ne.VIS_BLOCK_TOL)
    for k, r in ratios.items():
        worst[k] = max(worst.get(k, 0.0), r)
    print("%-18s %-14s " % (name, label) + "  ".join("%s %8.2f" % (k, r) for k, r in ratios.items()))
    return got, fails


def same_bits(a, b):
    return [k for k in ("H", "g", "E", "eg") if not np.array_equal(a[k][np.tril(np.ones(a[k].shape, bool))] if a[k].ndim == 2 else a[k],
                                                                    b[k][np.tril(np.ones(b[k].shape, bool))] if b[k].ndim == 2 else b[k])]


def run_batch(be, oracle, names, label):
    """Every window of the batch: the first occurrence of a case against the reference, a later one against the first, bit for bit."""
    snaps = [gw.ne_case(n, oracle) for n in names]
    b = be.batch_upload(snaps)
    fails, worst, first = [], {}, {}
    try:
        b.solve(abi.MARGIN_NONE)
        res = b.download()
        for w, n in enumerate(names):
            assert res[w]["summary"]["iterations"] == 1
            if n not in first:
                first[n], f = check_window(b, w, n, oracle, label, worst)
                fails += f
            else:
                fails += ["%s: %s differs between two places of the batch (%s)" % (n, k, label) for k in same_bits(ne.device_system(b, w), first[n])]
    finally:
        b.free()
    print("%s: worst ratios %s" % (label, {k: round(v, 2) for k, v in worst.items()}))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", gw.ne_case_names())
def test_one_window_alone(backends, oracle, name):
    """B = 1: 16 workgroups of k_gnss per window, the small-batch assembly."""
    run_batch(backends(), oracle, [name], "alone")


def test_batch_of_five(backends, oracle):
    """12 workgroups per window: the entry count is no multiple of the threads of one pass."""
    run_batch(backends(), oracle, ["n8", "n257", "gaps", "n8", "const_frame"], "B=5")


def test_throughput_batch(backends, oracle):
    """33 windows, GNSS, plane, anchor and plain ones mixed: one workgroup of k_gnss per window, plane_anchor_term in k_visasm."""
    kinds = ["n8", "plain", "all_three", "plane_free", "anchor", "one_obs", "plane_const", "clock_only", "lowspeed", "gaps", "n320", "second", "one_constellation",
             "const_frame", "one_frame"]
    run_batch(backends(), oracle, [kinds[i % len(kinds)] for i in range(33)], "B=33")


def test_batch_with_a_window_beyond_the_staging_limit(backends, oracle):
    """The 321-observation window sums from the global copy, the others of its batch from LDS sized for 320: one workgroup for all."""
    run_batch(backends(), oracle, ["n320", "n321", "n8", "n321"], "B=4 unstaged")


@pytest.mark.parametrize("name", ["n8_hold0", "n257_hold0"])
def test_second_linearisation(backends, oracle, name):
    """H and g of the SECOND linearisation against the reference at the state a one-iteration solve hands back, with
    speculative_linearization 1 (the GNSS factors evaluated at the candidate in sub 1 — by the work item of k_lin_small for n8_hold0, by
    a launch of k_gnss for n257_hold0, which is above GN_ITEM_MAX_OBS — and summed in sub 2) and 0 (sub 0 at the accepted state). Pose 0
    is constant in these windows, so the gauge fix behind the solve (k_reanchor) is the identity and the downloaded state is the
    linearised one up to its round trip, which normal_equations_np.state_tolerance states as a first-order allowance (measured on the
    CPU; gnss_window_cases.at_state gives the quaternions the sign the solve carried). The branch condition of the factor arithmetic
    holds for every observation at the new state too. Between the two settings the state after the first step is the same and the
    rcv_dt / rcv_ddt by rcv_dt / rcv_ddt entries, which the GNSS factors alone reach in a window without a prior, are bit-equal: sub 1 +
    sub 2 perform sub 0's operations in its order (gfbe_gnss_solve.hip)."""
    import gnss_np as gn
    snap = gw.ne_case(name, oracle)
    got, fails = {}, []
    for spec in (1, 0):
        one = backends(spec, 1).solve_batch([snap])[0]
        assert one["summary"]["iterations"] == 1 and list(one["summary"]["accepted"]) == [0, 1]          # the step was taken
        at1 = gw.at_state(snap, one)
        assert np.abs(at1["pose"][0] - np.asarray(snap["pose"], float)[0]).max() <= ne.STATE_ULPS_MEASURED * ne.U          # the gauge fix had nothing to do
        bf, _ = gn.branch_failures(ne.gnss_case_of(at1), at1["gnss"].get("iono"), name)
        assert not bf, "\n".join(bf)
        ref = ne.reference_normal_equations(at1, oracle.eval_factors(at1, robustify=True))
        b = backends(spec, 2).batch_upload([snap])
        try:
            b.solve(abi.MARGIN_NONE)
            assert b.download()[0]["summary"]["iterations"] == 2
            got[spec] = ne.device_system(b, 0)
        finally:
            b.free()
        ratios, f = ne.compare_system(got[spec], ref, ne.K, "%s, second linearisation, spec=%d:" % (name, spec), names=("H", "g"),
                                      vis_block_tol=ne.VIS_BLOCK_TOL, state_tol=ne.state_tolerance(snap))
        print("%-11s second linearisation spec=%d  " % (name, spec) + "  ".join("%s %8.2f" % kv for kv in ratios.items()))
        bare, _ = ne.compare_system(got[spec], ref, ne.K, names=("H", "g"), vis_block_tol=ne.VIS_BLOCK_TOL)
        print("%-11s   without the state allowance  " % name + "  ".join("%s %8.2f" % kv for kv in bare.items()))
        fails += f
        got[spec]["state"] = one["state"]
    assert not fails, "\n".join(fails)
    assert np.array_equal(got[0]["state"]["pose"], got[1]["state"]["pose"])
    assert np.array_equal(got[0]["state"]["gnss_state"]["rcv_dt"], got[1]["state"]["gnss_state"]["rcv_dt"])
    tri = np.tril(np.ones((ne.ND - CLK0, ne.ND - CLK0), bool))
    assert np.array_equal(got[0]["H"][CLK0:, CLK0:][tri], got[1]["H"][CLK0:, CLK0:][tri]) and np.abs(got[1]["H"][CLK0:, CLK0:][tri]).max() > 0
    assert np.array_equal(got[0]["g"][CLK0:], got[1]["g"][CLK0:]) and np.abs(got[1]["g"][CLK0:]).max() > 0
    first = gw.ne_reference(name, oracle)[2]          # and it IS a second linearisation: g has moved away from the first one's
    assert np.abs(got[1]["g"][CLK0:] - np.asarray(first["g"][CLK0:], float)).max() > 1e-3 * np.abs(np.asarray(first["g"][CLK0:], float)).max()
