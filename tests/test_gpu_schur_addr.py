"""The addresses of k_schur's lean form (k_schur_lean: a wave's row bases formed on the scalar unit, one 32-bit byte offset of the lane's
slot per tile, the start frame of a tile from the group's boundaries held in scalar registers): H, g, E and eg of the first linearisation
of a batch of 32 windows — the smallest batch on the throughput path — against the extended-precision sum of
tests/normal_equations_np.py, at the bound K = %(K)g of tests/test_gpu_normal_equations.py, built like tests/test_gpu_schur_steps.py.

What the new addressing and the new start-frame lookup can get wrong is decided by where a window's start frames begin and end, so the
five windows (%(lo)d .. %(hi)d landmarks of synth.Scenario, shaped by normal_equations_np.shaped_window) hold these edges, and
`test_layout` checks on the CPU that they do (groups of start frames {0, 1}, {2}, {3, 4, 5}, {6 .. 10}):
  a group whose first, whose middle and whose last start frame has no landmark while the group has some (consecutive equal entries of
    sf_tile_begin; {0, 1} has no middle, the last frame of {6 .. 10} that can hold a landmark is 9)
  a group that is empty, in a window whose other groups are not
  a window with one tile in all
  start frame 9, where the last observation step clamps every row index to 0 and the waves 2 and 3 have no live block (start frame 10
    cannot hold a landmark with a factor — an observation in a later frame does not exist — and the C ABI files a landmark without
    factors under start frame 0: the clamp max(NF - 2 - s, 0) at s = 10 has no input that reaches it)
  start frame 0 with and without the tenth observer
  windows with different tile counts in one batch (the prefetch past a window's last tile is clamped, never staged)
  the largest window last in the batch: the last tile's lanes carry the largest offsets the batch has
  a tile with fewer than 64 occupied rows at the end of a start frame, followed by another start frame of the same group
`test_packed_layout` checks the same boundaries on the packed descriptors (csrc/gfbe_upload.h through the host shim of
tests/test_upload_host.py).
The batch runs once more with gfbe_options.test_fail_chol_iter = 1 (E and eg rebuilt at 10 mu0 from weights formed at the staging).
Determinism: two runs of the batch agree bit for bit, and a window gives the same bits among 31 others as in a batch of 32 copies.

Measured on an MI355X (worst |X_dev - X_ref| / (u A_X); E and eg at mu0 / after the invalid step):
%(measured)s
"""
import numpy as np
import pytest

import normal_equations_np as ne
import test_upload_host as uh
from _gfbe_import import gf
from test_upload_host import shim      # noqa: F401  (the fixture that builds the upload's host half)

abi, synth = gf.abi, gf.synth
gpu = pytest.mark.gpu

MEASURED = """  first_empty     H 396   g 0.30   E 220 / 220   eg  26 /  26
  middle_empty    H 173   g 0.20   E 243 / 243   eg  45 /  45
  last_empty      H 171   g 0.90   E 361 / 362   eg  38 /  38
  one_tile        H 1.6   g 0.37   E 987 / 988   eg 196 / 196
  largest         H 207   g 0.47   E 288 / 289   eg  23 /  22
(the parent commit gives the same bits for all five windows, with and without the invalid step; one_tile — seven landmarks with one factor
 each, nothing else in the sum — comes closest to the bound, under either library)"""

B = 32
GROUPS = ((0, 1), (2,), (3, 4, 5), (6, 7, 8, 9, 10))
LAST_FRAME_WITH_FACTORS = 9
# {(start frame, factors): landmarks}; a start frame's landmarks fill tiles of 64, longest track first
WINDOWS = {
    # the first start frame of every group with several is empty; start frame 1 ends in a tile of six rows, start frame 4 in one of one
    # (the last group: 6 and 9 empty, 7 and 8 not)
    "first_empty": {(1, 9): 30, (1, 4): 40, (2, 8): 10, (4, 6): 30, (4, 2): 35, (5, 5): 10, (7, 3): 5, (8, 2): 3},
    # the middle start frames are empty, the group {2} is empty, start frame 0 has a tenth observer
    "middle_empty": {(0, 10): 5, (0, 3): 20, (1, 5): 10, (3, 7): 10, (5, 5): 10, (6, 4): 10, (9, 1): 4},
    # the last start frames are empty and so is the group {6 .. 10}; start frame 0 has no tenth observer and ends in a tile of four rows
    "last_empty": {(0, 9): 8, (0, 2): 60, (2, 8): 3, (3, 7): 5, (4, 1): 70},
    # one tile in all, of start frame 9: three groups are empty
    "one_tile": {(9, 1): 7},
    # every start frame, full tiles next to ragged ones: the window with the most tiles, placed last
    "largest": {(0, 10): 66, (0, 5): 30, (1, 9): 64, (2, 8): 70, (3, 7): 64, (4, 6): 10, (5, 5): 66, (6, 4): 64, (7, 3): 10, (8, 2): 5, (9, 1): 64},
}
CYCLE = [n for n in WINDOWS if n != "largest"]
NAMES = [CYCLE[w % len(CYCLE)] for w in range(B - 1)] + ["largest"]       # by place in the batch
READ = list(range(len(CYCLE))) + [B - 1]                                  # the places compared against the reference: every window once
SIZES = [sum(c.values()) for c in WINDOWS.values()]
__doc__ = __doc__ % dict(K=ne.K, lo=min(SIZES), hi=max(SIZES), measured=MEASURED)
_snaps, _refs = {}, {}


def window(name):
    if name not in _snaps:
        scn = synth.Scenario(seed=8300 + list(WINDOWS).index(name), n_landmarks=12000, use_wheel=True)
        _snaps[name] = ne.shaped_window(scn, 0, WINDOWS[name])
    return _snaps[name]


def reference(name, oracle, mu_factor):
    """The extended-precision system of a window (computed once) with the Schur term at mu_factor x the first iteration's mu."""
    if name not in _refs:
        snap = window(name)
        _refs[name] = ne.reference_normal_equations(snap, oracle.eval_factors(snap, robustify=True))
    ref = dict(_refs[name])
    ref["E"], ref["eg"], ref["A_E"], ref["A_eg"] = ne.schur_reference(ref["Hll"], ref["gl"], ref["Hpl"], ne.GF_MIN_MU * mu_factor, True, ref["idle"],
                                                                       ref["A_Hpl"], ref["A_gl"])
    return ref


# ---- the layout, restated ------------------------------------------------------------------------------------------------------------
def tiles_of(counts):
    """The landmark tiles of a window in the device's order: [(start frame, track lengths of the occupied rows, longest first)]."""
    out = []
    for s in range(ne.NF):
        rows = [m for m in range(10, 0, -1) for _ in range(counts.get((s, m), 0))]
        out += [(s, rows[q:q + 64]) for q in range(0, len(rows), 64)]
    return out


def sf_tile_begin_of(counts):
    t = [s for s, _ in tiles_of(counts)]
    return [sum(1 for x in t if x < s) for s in range(ne.NF + 1)]


def edges_of(counts):
    """What one window shows, per group of start frames: which of its start frames hold no landmark while the group holds some."""
    sf = sf_tile_begin_of(counts)
    empty = [sf[s + 1] == sf[s] for s in range(ne.NF)]
    out = []
    for fr in GROUPS:
        fr = [s for s in fr if s <= LAST_FRAME_WITH_FACTORS]
        e = set()
        if all(empty[s] for s in fr):
            e.add("group")
        else:
            if empty[fr[0]] and len(fr) > 1:
                e.add("first")
            if empty[fr[-1]] and len(fr) > 1:
                e.add("last")
            if any(empty[s] for s in fr[1:-1]):
                e.add("middle")
        out.append(e)
    return out


def test_layout():
    E = {}
    for name in WINDOWS:
        assert ne.layout_counts(window(name)) == WINDOWS[name]
        E[name] = edges_of(WINDOWS[name])
    for g, fr in enumerate(GROUPS):
        seen = set().union(*(E[n][g] for n in WINDOWS))
        want = {"group"} | ({"first", "last"} if len(fr) > 1 else set()) | ({"middle"} if len(fr) > 2 else set())
        assert seen == want, (g, seen)
    # an empty group beside groups that are not; consecutive equal entries of sf_tile_begin inside a group that has tiles
    assert any("group" in e and any(not x for x in E[n]) for n in WINDOWS for e in E[n])
    tiles = {n: tiles_of(WINDOWS[n]) for n in WINDOWS}
    assert len(tiles["one_tile"]) == 1 and tiles["one_tile"][0][0] == 9
    assert any(s == 9 for n in WINDOWS for s, _ in tiles[n]) and all(s <= LAST_FRAME_WITH_FACTORS for n in WINDOWS for s, _ in tiles[n])
    tenth = {rows[0] == 10 for n in WINDOWS for s, rows in tiles[n] if s == 0}
    assert tenth == {True, False}
    assert len({len(t) for t in tiles.values()}) >= 4
    assert NAMES[-1] == "largest" and len(NAMES) == B and all(len(tiles["largest"]) > len(tiles[n]) for n in CYCLE)
    assert {s for s, _ in tiles["largest"]} == set(range(LAST_FRAME_WITH_FACTORS + 1))
    # a ragged tile at the end of a start frame with another start frame of the SAME group behind it, in every group with several
    ragged = set()
    for t in tiles.values():
        for (s, rows), (s2, _) in zip(t, t[1:]):
            if len(rows) < 64 and s2 != s:
                ragged |= {g for g, fr in enumerate(GROUPS) if s in fr and s2 in fr}
    assert ragged == {0, 2, 3}, ragged
    assert any(len(rows) == 64 for t in tiles.values() for _, rows in t)


def test_packed_layout(shim):
    """The same boundaries on the packed descriptors: sf_tile_begin of every window as restated above, the windows' slots back to back
    in the order of the batch, the largest window's tiles the last of the batch."""
    p = uh.Packed(shim, [window(n) for n in NAMES])
    try:
        assert p.status == abi.OK, p.err
        assert p.info["schur_groups"] == 4 and not p.info["vis_full"] and 8 * p.info["tot_lm"] < 2 ** 32      # the lean form
        off = 0
        for w, name in enumerate(NAMES):
            sc, ds = p.scan(w), p.desc(w)
            assert sc["sf_tile_begin"].tolist() == sf_tile_begin_of(WINDOWS[name]), name
            assert ds["lm_off"] == off and sc["slots"] == 64 * len(tiles_of(WINDOWS[name]))
            off += sc["slots"]
        assert off == p.info["tot_lm"] and p.desc(B - 1)["lm_off"] + p.scan(B - 1)["slots"] == p.info["tot_lm"]
        assert p.info["max_tiles"] == len(tiles_of(WINDOWS["largest"]))
    finally:
        p.close()


# ---- the device ------------------------------------------------------------------------------------------------------------------------
def run(backend, snaps, read, full=False):
    b = backend.batch_upload(snaps)
    try:
        b.solve(abi.MARGIN_NONE)
        assert all(r["summary"]["iterations"] == 1 for r in b.download())
        if full:
            return {w: ne.device_system(b, w) for w in read}
        return {w: dict(E=np.array([b.debug_vector(2000 + r, w)[:ne.NV] for r in range(ne.NV)]), eg=b.debug_vector(2000 + ne.NV, w)[:ne.NV].copy())
                for w in read}
    finally:
        b.free()


def same_bits(a, b):
    for k in a:
        tri = np.tril(np.ones(a[k].shape, bool)) if a[k].ndim == 2 else np.ones(a[k].shape, bool)
        if not np.array_equal(a[k][tri], b[k][tri]):
            return False
    return True


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
    """The batch of 32 — the four small windows in turn, the largest last — solved once: H, g, E and eg of every window's first place, of
    the second place of the four, and of the last place."""
    return run(backends(), [window(n) for n in NAMES], READ + [w + len(CYCLE) for w in range(len(CYCLE))], full=True)


@gpu
@pytest.mark.parametrize("fail", [0, 1])
def test_against_extended_precision(backends, mixed, oracle, fail):
    got = mixed if not fail else run(backends(1), [window(n) for n in NAMES], READ)
    fails = []
    for w in READ:
        ref = reference(NAMES[w], oracle, 10.0 if fail else 1.0)
        ratios, f = ne.compare_system(got[w], ref, ne.K, "%s%s:" % (NAMES[w], ", after an invalid step" if fail else ""),
                                      names=("E", "eg") if fail else ("H", "g", "E", "eg"))
        print("%-14s fail=%d  %s" % (NAMES[w], fail, "  ".join("%s %8.2f" % kv for kv in ratios.items())))
        fails += f
    assert not fails, "\n".join(fails)


@gpu
def test_same_bits_run_to_run_and_place_to_place(backends, mixed):
    again = run(backends(), [window(n) for n in NAMES], READ, full=True)
    for w in READ:
        assert same_bits(mixed[w], again[w]), "%s: two runs differ" % NAMES[w]
    for w in range(len(CYCLE)):
        assert same_bits(mixed[w], mixed[w + len(CYCLE)]), "%s: places %d and %d of the batch differ" % (NAMES[w], w, w + len(CYCLE))


@gpu
@pytest.mark.parametrize("k", range(len(READ)))
def test_alone_in_a_batch_of_copies(backends, mixed, k):
    w = READ[k]
    alone = run(backends(), [window(NAMES[w])] * B, (0, B - 1))
    assert same_bits(alone[0], {q: mixed[w][q] for q in ("E", "eg")}), "%s: among 31 others and in a batch of 32 copies differ" % NAMES[w]
    assert same_bits(alone[0], alone[B - 1])
