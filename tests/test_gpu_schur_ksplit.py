"""k_schur's form for throughput batches with constant extrinsic / td (schur_body<true>: the twelve-double prefetch of compressed
rows, the k-steps behind a tile's last landmark skipped): E and eg of the first linearisation of batches of 32 windows — the smallest
batch on the throughput path — against the extended-precision sum of tests/normal_equations_np.py, at the bound K = %(K)g of
tests/test_gpu_normal_equations.py.

What can go wrong there shows at the edges of a tile and of a start-frame group, so the three windows (70 .. 140 landmarks of
synth.Scenario, shaped by normal_equations_np.shaped_window) hold, and `test_layout` checks on the CPU that they do:
  tiles with 1, 4, 5, 63 and 64 occupied rows (one row of a k-step, a whole k-step, one row into the next, the last row missing, full)
  tracks of 3 and of 10 factors (one block of the panel, all five)
  a start-frame group {0, 1}, {2}, {3, 4, 5}, {6 .. 10} without landmarks and one with a single tile, in every window
  constant landmarks (weight zero: rows of zeros inside a tile)
and the batch runs once more with gfbe_options.test_fail_chol_iter = 1: after the invalid step the windows' weights were formed with
another mu than the one k_schur multiplies with (WinCtl::sw_mu != mu), E is rebuilt at 10 mu0 and compared at that mu.
Determinism: two runs of the batch agree bit for bit, and a window gives the same bits among 31 others as in a batch of 32 copies.

Measured on an MI355X (worst |X_dev - X_ref| / (u A_X); at mu0 / after the invalid step):
  rows_64_5_4_1   E 422 / 422   eg  69 /  68
  rows_63_65_5    E 445 / 444   eg  60 /  61
  constant        E 434 / 432   eg 110 / 111
"""
import numpy as np
import pytest

import normal_equations_np as ne
from _gfbe_import import gf

abi, synth = gf.abi, gf.synth
pytestmark = pytest.mark.gpu
__doc__ = __doc__ % dict(K=ne.K)

B = 32
GROUPS = ((0, 1), (2,), (3, 4, 5), (6, 7, 8, 9, 10))
# {(start frame, factors): landmarks}
WINDOWS = {
    "rows_64_5_4_1": {(0, 10): 12, (0, 3): 52, (1, 9): 2, (1, 3): 3, (4, 6): 2, (4, 3): 2, (7, 3): 1},            # 74 landmarks
    "rows_63_65_5": {(0, 10): 12, (0, 3): 51, (2, 8): 10, (2, 3): 55, (6, 4): 2, (6, 3): 3},                      # 133
    "constant": {(0, 10): 10, (0, 5): 30, (3, 7): 30, (5, 3): 10, (8, 2): 10, (9, 1): 10},                        # 100, every third constant
}
_snaps = {}


def window(name):
    if name not in _snaps:
        counts = WINDOWS[name]
        scn = synth.Scenario(seed=8100 + list(WINDOWS).index(name), n_landmarks=4000, use_wheel=True)
        snap = ne.shaped_window(scn, 0, counts)
        if name == "constant":
            snap["feature_const"] = (np.arange(len(snap["para_feature"])) % 3 == 0).astype(np.uint8)
        _snaps[name] = snap
    return _snaps[name]


def tile_rows(per_start):
    """Occupied rows of every landmark tile: a start frame's landmarks fill tiles of 64."""
    return [min(64, n - q) for n in per_start for q in range(0, n, 64)]


def test_layout():
    rows, lengths, empty, single = set(), set(), 0, 0
    for name in WINDOWS:
        snap = window(name)
        assert 70 <= len(snap["para_feature"]) <= 140
        counts = ne.layout_counts(snap)
        assert counts == WINDOWS[name]
        per = ne.per_start_frame(counts)
        rows |= set(tile_rows(per))
        lengths |= {m for (_, m) in counts}
        tiles = [len(tile_rows([per[s] for s in g])) for g in GROUPS]
        empty += 0 in tiles
        single += 1 in tiles
    assert {1, 4, 5, 63, 64} <= rows, rows
    assert {3, 10} <= lengths
    assert empty == len(WINDOWS) and single == len(WINDOWS)
    assert window("constant")["feature_const"].any()


def schur_term(batch, w):
    E = np.array([batch.debug_vector(2000 + r, w)[:ne.NV] for r in range(ne.NV)])
    return dict(E=E, eg=batch.debug_vector(2000 + ne.NV, w)[:ne.NV].copy())


def run(backend, snaps, read):
    b = backend.batch_upload(snaps)
    try:
        b.solve(abi.MARGIN_NONE)
        assert all(r["summary"]["iterations"] == 1 for r in b.download())
        return {w: schur_term(b, w) for w in read}
    finally:
        b.free()


def same_bits(a, b):
    tri = np.tril(np.ones(a["E"].shape, bool))
    return np.array_equal(a["E"][tri], b["E"][tri]) and np.array_equal(a["eg"], b["eg"])


@pytest.fixture(scope="module")
def backends():
    ne.require_extended_precision()
    made = {}

    def get(fail=0):
        if fail not in made:
            o = abi.default_options()
            o.max_num_iterations = 1
            if fail:
                o.test_fail_chol_iter, o.test_fail_chol_count = 1, 1
            made[fail] = gf.Backend(device=0, options=o)
        return made[fail]
    yield get
    for b in made.values():
        b.close()


@pytest.fixture(scope="module")
def mixed(backends):
    """The batch of 32 — the three windows in turn — solved once: (names by place, E and eg of the first three places and of place 3 + q)."""
    names = [list(WINDOWS)[w % len(WINDOWS)] for w in range(B)]
    return names, run(backends(), [window(n) for n in names], range(2 * len(WINDOWS)))


@pytest.mark.parametrize("fail", [0, 1])
def test_against_extended_precision(backends, mixed, oracle, fail):
    names, got = mixed if not fail else (mixed[0], run(backends(1), [window(n) for n in mixed[0]], range(len(WINDOWS))))
    fails = []
    for w in range(len(WINDOWS)):
        snap = window(names[w])
        ev = oracle.eval_factors(snap, robustify=True)
        ref = ne.reference_system(snap, ev, mu=ne.GF_MIN_MU * (10.0 if fail else 1.0))
        ratios, f = ne.compare_system(got[w], ref, ne.K, "%s%s:" % (names[w], ", after an invalid step" if fail else ""), names=("E", "eg"))
        print("%-14s fail=%d  E %8.2f  eg %8.2f" % (names[w], fail, ratios["E"], ratios["eg"]))
        fails += f
    assert not fails, "\n".join(fails)


def test_same_bits_run_to_run_and_place_to_place(backends, mixed):
    names, got = mixed
    again = run(backends(), [window(n) for n in names], range(len(WINDOWS)))
    for w in range(len(WINDOWS)):
        assert same_bits(got[w], again[w]), "%s: two runs differ" % names[w]
        assert same_bits(got[w], got[w + len(WINDOWS)]), "%s: places %d and %d of the batch differ" % (names[w], w, w + len(WINDOWS))


@pytest.mark.parametrize("k", range(len(WINDOWS)))
def test_alone_in_a_batch_of_copies(backends, mixed, k):
    names, got = mixed
    alone = run(backends(), [window(names[k])] * B, (0, B - 1))
    assert same_bits(alone[0], got[k]), "%s: among 31 others and in a batch of 32 copies differ" % names[k]
    assert same_bits(alone[0], alone[B - 1])
