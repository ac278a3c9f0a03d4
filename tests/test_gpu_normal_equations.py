"""The assembled normal equations of the FIRST linearisation — H (every row, lower triangle), g, the landmark-elimination term E
(all 73 rows) and its gradient share eg, read through gfbe_debug_vector after one iteration — against an extended-precision sum of
the oracle's per-factor blocks (tests/normal_equations_np.py), entry by entry:

    |X_dev[i, j] - X_ref[i, j]| <= K u A_X[i, j]      (A_X: the entry's absolute sum; exactly 0.0 where A_X is zero)

with the bound K the helper derives from the rounding of a plain FP64 loop (measured on the CPU, test_normal_equations_reference.py)
and the separate allowance of the entries the IMU factors reach. No sampling of rows, no max-norm fallback.

One window per case; landmarks per start frame 0..9:
  tile_edges      64, 65, 63, 1, 0, 128, 129, 0, 2, 1: a full tile, one over, one under, a single landmark, empty start frames inside
                  the groups of k_schur, start frames 8 and 9 (two- and one-factor tracks)
  chunk_edges     256, 257 and 513 in three start frames: the boundaries of k_vis_chunk's four-tile chunks and its sub-chunks
  one_group_s     everything in start frame s = 0 / 2 / 4 / 7: the other groups of k_schur take the empty path
  short_tracks    every track has ONE factor, start frames 0..9
  no_landmarks    no visual factor: E, eg exactly zero
  idle_landmarks  every third landmark constant, every fifth without a factor: weight zero
  full_columns    camera extrinsic and td free (the uncompressed row format), observation stamps that differ from td
  robust          5 %% of the observations displaced by 20 px: the Huber corrector is active
  partial         frame_count = 6
  prior_wheel_2k  the bench shape: 2 000 landmarks, wheel, prior
  soak_349        3 500 landmarks, LiDAR block, a third of the landmarks constant, a window that is still filling up

Launch shapes: every case alone (the small-batch kernels: k_lin_small, k_schur_visblock_small, k_assemble); all cases at shuffled
places of a batch of 33 (the throughput kernels: k_vis_chunk, k_schur, k_visasm, k_dense_tp, k_prior_tp; grids sized by the largest
window) and of a batch of 131 (two halves on two stream pairs); the batch of 33 also without the speculative linearisation. One
window with free camera extrinsic switches the whole batch to the uncompressed rows, so every batch runs twice: with full_columns
in it and without (the compressed D / x rows, the shipped configuration). A window that occurs twice in a batch is bit-identical to
itself.

Measured on an MI355X (worst ratio |X_dev - X_ref| / (u A_X) per array over all cases; bound K = %(K)g):
%(MEASURED)s
"""
import time

import numpy as np
import pytest

import normal_equations_np as ne
from _gfbe_import import gf

abi = gf.abi
pytestmark = pytest.mark.gpu

MEASURED = """  launch shape                          H       g       E      eg     worst case
  alone (small-batch kernels)        888    14.2    1023     424     H, g: full_columns   E: one_group_2   eg: robust
  B = 33 / 131, uncompressed rows    888    14.2     532     424     (the same with speculative_linearization = 0)
  B = 33 / 131, compressed rows      317     2.9    1020     424     E: one_group_2
  soak_349 in every shape            312     1.0      94      18
E of one_group_2 (200 landmarks, all in start frame 2) sits at the bound: about half of it is the compressed D / x row form (532 with
the uncompressed rows of the same kernels), the rest the per-factor blocks. A regrouping of k_schur's sums moves that figure by a
few units; it is a rounding property, not an error, but there is no room under K for a further loss of accuracy there.
Sensitivity (each built once, not committed): k_schur without the last tile of a group, the landmark weight without its clamp term,
the gather of E without one partial slot, the staging of Hpl without the tenth observing pose — each fails 12 to 19 of these 20
tests; test_gpu_parity.py's comparison of the two kernel sets with each other sees the first and the third only."""
__doc__ = __doc__ % dict(K=ne.K, MEASURED=MEASURED)


@pytest.fixture(scope="module")
def backends():
    ne.require_extended_precision()
    made = {}

    def get(spec=1):
        if spec not in made:
            o = abi.default_options()
            o.max_num_iterations = 1
            o.speculative_linearization = spec
            made[spec] = gf.Backend(device=0, options=o)
        return made[spec]
    yield get
    for b in made.values():
        b.close()


def check_window(batch, w, name, oracle, label, worst):
    snap, ev, ref = ne.case_reference(name, oracle)
    got = ne.device_system(batch, w)
    ratios, fails = ne.compare_system(got, ref, ne.K, "%s, %s:" % (name, label))
    for k, r in ratios.items():
        worst[k] = max(worst.get(k, 0.0), r)
    print("%-15s %-22s " % (name, label) + "  ".join("%s %8.2f" % (k, r) for k, r in ratios.items()))
    return got, fails


@pytest.mark.parametrize("name", ne.case_names())
def test_one_window_alone(backends, oracle, name):
    """B = 1: the small-batch kernel set."""
    snap = ne.build_case(name, oracle)
    b = backends().batch_upload([snap])
    try:
        b.solve(abi.MARGIN_NONE)
        assert b.download()[0]["summary"]["iterations"] == 1
        _, fails = check_window(b, 0, name, oracle, "alone", {})
    finally:
        b.free()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mix", ["all", "compressed"])
@pytest.mark.parametrize("B,spec", [(33, 1), (33, 0), (131, 1)])
def test_heterogeneous_batch(backends, oracle, B, spec, mix):
    """Every case at a shuffled place of one batch (throughput kernels); `compressed`: without the window whose free camera extrinsic
    switches the batch to the uncompressed rows."""
    names = [n for n in ne.case_names() if mix == "all" or n != "full_columns"]
    rng = np.random.default_rng(B + spec)
    order = np.concatenate([rng.permutation(len(names)) for _ in range(B // len(names) + 1)])[:B]
    snaps = [ne.build_case(names[q], oracle) for q in order]
    t0 = time.time()
    b = backends(spec).batch_upload(snaps)
    fails, worst, first = [], {}, {}
    try:
        b.solve(abi.MARGIN_NONE)
        res = b.download()
        for w, q in enumerate(order):
            assert res[w]["summary"]["iterations"] == 1
            if q not in first:                       # the first occurrence against the reference, every array in full
                got, f = check_window(b, w, names[q], oracle, "B=%d spec=%d %s" % (B, spec, mix), worst)
                fails += f
                first[q] = got
            elif sum(1 for p in order[:w] if p == q) == 1:      # the second one against the first: the same bits at another place
                again = ne.device_system(b, w)
                for k in ("H", "g", "E", "eg"):
                    tri = np.tril(np.ones(again[k].shape, bool)) if k in ("H", "E") else np.ones(again[k].shape, bool)
                    if not np.array_equal(again[k][tri], first[q][k][tri]):
                        fails.append("%s: %s differs between places %d and %d of the batch" % (names[q], k, list(order).index(q), w))
    finally:
        b.free()
    print("B=%d spec=%d %s: worst ratios %s  (%.1f s)" % (B, spec, mix, {k: round(v, 2) for k, v in worst.items()}, time.time() - t0))
    assert len(first) == len(names)
    assert not fails, "\n".join(fails)
