"""What the two matrix-core kernels of a throughput batch skip (schur_body<true>: the observation steps a tile never ran are not
staged, zeros are written only where a chunk of the tile reads, every 16-row chunk multiplies up to its own last 16-column block;
k_vis_chunk: the k-steps behind the last lane with a factor): H, g, E and eg of the first linearisation of batches of 32 windows — the
smallest batch on the throughput path — against the extended-precision sum of tests/normal_equations_np.py, at the bound K = %(K)g of
tests/test_gpu_normal_equations.py, built like tests/test_gpu_schur_ksplit.py.

The skipped work is decided per tile from the track lengths of its rows, so the four windows (%(lo)d .. %(hi)d landmarks of
synth.Scenario, shaped by normal_equations_np.shaped_window) hold the edges of those decisions, and `test_layout` checks on the CPU,
per start-frame group {0, 1}, {2}, {3, 4, 5}, {6 .. 10}, that they do (m0: the observation steps a tile ran = the track length of its
first landmark; a start frame s allots 10 - s):
  m0 equal to what the start frame allots, one below, two or more below, and 1
  m0 = 3, 6, 9 where the group's start frames allot as many (9: {0, 1} only; 6: not {6 .. 10}): with the steps dealt k = part - 1 + 3 u,
    a part then has zero (m0 = 1), one, two and three live blocks
  start frame 0 with and without a tenth observer
  the track length dropping exactly at rows 15/16, 16/17, 31/32 and 47/48 of a tile, each time across a 16-column boundary of the
    compact panel (a chunk's last block then differs from the tile's)
  a tile whose four 16-row chunks all end in different blocks (the group {6 .. 10} only has blocks 0 and 1: two there)
  a start frame changing inside a group directly after a wider tile (stale columns in front of the start block) and directly after
    a narrower one (stale columns behind what that tile wrote); the group {2} has one start frame
  observation steps of k_vis_chunk whose last lane with a factor is 0, 3, 4, 15, 16 and 63
  constant landmarks inside the active prefix
and that the packed layout is sorted the way the chunks' blocks are taken from (a tile's valid rows first, longest track first).
The batch runs once more with gfbe_options.test_fail_chol_iter = 1 (E and eg rebuilt at 10 mu0 from weights formed with another mu).
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

MEASURED = """  steps_1_4_5     H 198   g 0.23   E 470 / 469   eg 109 / 108
  chunks          H 205   g 0.81   E 298 / 298   eg  31 /  31
  drop_17         H 357   g 1.02   E 362 / 366   eg  45 /  46
  six_and_three   H 865   g 0.45   E 283 / 282   eg  82 /  82
(the parent commit gives the same bits for all four windows)"""

B = 32
GROUPS = ((0, 1), (2,), (3, 4, 5), (6, 7, 8, 9, 10))
# {(start frame, factors): landmarks}; a start frame's landmarks fill tiles of 64, longest track first
WINDOWS = {
    # one, four and five rows ahead of the rest, then a tile of single factors; the next start frame follows that narrow tile
    "steps_1_4_5": {(0, 10): 1, (0, 9): 3, (0, 8): 1, (0, 1): 64, (1, 8): 20,
                    (2, 8): 1, (2, 7): 3, (2, 6): 1, (2, 1): 64,
                    (3, 7): 1, (3, 6): 3, (3, 5): 1, (3, 1): 64, (4, 5): 20,
                    (6, 4): 1, (6, 3): 3, (6, 2): 28, (6, 1): 37, (7, 2): 20},
    # four chunks of sixteen rows, each ending in another block; the next start frame follows that wide tile. Every third landmark constant
    "chunks": {(0, 10): 16, (0, 9): 16, (0, 6): 16, (0, 4): 16, (1, 3): 30,
               (2, 8): 16, (2, 6): 16, (2, 4): 16, (2, 1): 16,
               (3, 7): 16, (3, 6): 16, (3, 4): 16, (3, 1): 16, (4, 3): 30,
               (6, 4): 16, (6, 3): 16, (6, 2): 16, (6, 1): 16, (7, 1): 30},
    # seventeen long rows: the second chunk's first row is long, the others are not
    "drop_17": {(0, 9): 17, (0, 6): 47, (1, 9): 17, (1, 4): 47, (2, 7): 17, (2, 5): 47, (3, 6): 17, (3, 4): 47, (6, 3): 17, (6, 1): 47},
    # tiles of six and of three steps, the drop at row 16 of the last group, start frames 5, 8 and 9
    "six_and_three": {(0, 6): 40, (1, 6): 64, (1, 3): 10, (2, 6): 64, (2, 3): 10, (3, 3): 40, (5, 5): 10,
                      (6, 2): 16, (6, 1): 48, (7, 3): 1, (7, 2): 3, (7, 1): 1, (8, 2): 5, (9, 1): 5},
}
SIZES = [sum(c.values()) for c in WINDOWS.values()]
__doc__ = __doc__ % dict(K=ne.K, lo=min(SIZES), hi=max(SIZES), measured=MEASURED)
_snaps, _refs = {}, {}


def window(name):
    if name not in _snaps:
        scn = synth.Scenario(seed=8200 + list(WINDOWS).index(name), n_landmarks=12000, use_wheel=True)
        snap = ne.shaped_window(scn, 0, WINDOWS[name])
        if name == "chunks":
            snap["feature_const"] = (np.arange(len(snap["para_feature"])) % 3 == 0).astype(np.uint8)
        _snaps[name] = snap
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
def group_of(s):
    return next(g for g, fr in enumerate(GROUPS) if s in fr)


def last_block(s, m):
    """Last 16-column block of the compact panel a row of start frame s with m factors reaches: gradient column, then the poses from the
    group's first start frame on."""
    return (6 * (s - GROUPS[group_of(s)][0] + m + 1)) >> 4


def tiles_of(counts):
    """The landmark tiles of a window in the device's order: [(start frame, track lengths of the occupied rows, longest first)]."""
    out = []
    for s in range(ne.NF):
        rows = [m for m in range(10, 0, -1) for _ in range(counts.get((s, m), 0))]
        out += [(s, rows[q:q + 64]) for q in range(0, len(rows), 64)]
    return out


def edges_of(all_tiles):
    """Per start-frame group, what its tiles show (see the module's docstring)."""
    E = [dict(below=set(), m0=set(), tenth=set(), drops=set(), chunk_blocks=0, after=set(), last_lane=set()) for _ in GROUPS]
    for tiles in all_tiles:
        for q, (s, rows) in enumerate(tiles):
            e, m0 = E[group_of(s)], rows[0]
            e["m0"].add(m0)
            e["below"].add(min(10 - s - m0, 2))
            if s == 0:
                e["tenth"].add(m0 == 10)
            for r in (16, 17, 32, 48):
                if len(rows) > r and rows[r - 1] > rows[r] and last_block(s, rows[r - 1]) > last_block(s, rows[r]):
                    e["drops"].add(r)
            e["chunk_blocks"] = max(e["chunk_blocks"], len({last_block(s, rows[c]) for c in range(0, len(rows), 16)}))
            if q > 0 and tiles[q - 1][0] != s and group_of(tiles[q - 1][0]) == group_of(s):
                f = GROUPS[group_of(s)][0]
                before, now = 6 * (tiles[q - 1][0] - f + tiles[q - 1][1][0] + 1), 6 * (s - f + m0 + 1)      # last non-zero column
                e["after"].add("wider" if before > now else "narrower" if before < now else "equal")
            e["last_lane"] |= {sum(m > k for m in rows) - 1 for k in range(m0)}
    return E


def test_layout():
    all_tiles = []
    for name in WINDOWS:
        snap = window(name)
        assert ne.layout_counts(snap) == WINDOWS[name]
        all_tiles.append(tiles_of(WINDOWS[name]))
    for g, e in enumerate(edges_of(all_tiles)):
        allot = 10 - GROUPS[g][0]
        assert e["below"] == {0, 1, 2} and 1 in e["m0"], (g, e)
        assert {m for m in (3, 6, 9) if m <= allot} <= e["m0"], (g, e)
        assert e["drops"] == {16, 17, 32, 48}, (g, e)
        assert e["chunk_blocks"] == (4 if g < 3 else 2), (g, e)
        assert g == 1 or {"wider", "narrower"} <= e["after"], (g, e)
        assert {0, 3, 4, 15, 16, 63} <= e["last_lane"], (g, e)
    assert edges_of(all_tiles)[0]["tenth"] == {True, False}
    # constant landmarks inside the active prefix: in front of a free landmark of the same tile with as many factors
    snap = window("chunks")
    fi = np.asarray(snap["vis_feature_index"], int)
    m, s = np.bincount(fi, minlength=len(snap["para_feature"])), np.zeros(len(snap["para_feature"]), int)
    s[fi] = np.asarray(snap["vis_imu_i"], int)
    inside = 0
    for s0 in range(ne.NF):
        rows = np.asarray(snap["feature_const"], bool)[np.lexsort((-m, s))][np.sort(s) == s0]      # (stable: ties in ABI order)
        inside += sum(bool(t[:-1].any() and not t[np.argmax(t):].all()) for t in (rows[q:q + 64] for q in range(0, len(rows), 64)))
    assert inside >= len(GROUPS), inside


def test_packed_order(shim):
    """The order the chunks' last blocks rely on, on the packed layout itself (csrc/gfbe_upload.h through the host shim of
    tests/test_upload_host.py): in every tile the valid rows come first and their track lengths never increase."""
    p = uh.Packed(shim, [window(n) for n in WINDOWS])
    try:
        assert p.status == abi.OK, p.err
        lm_info = p.array("lm_info", np.int32, p.info["tot_lm"]).copy()
        tiles = 0
        for w, name in enumerate(WINDOWS):
            sc, o = p.scan(w), p.desc(w)["lm_off"]
            assert [t for t in tiles_of(WINDOWS[name])] == [
                (int(lm_info[o + 64 * q] & 0xff), [int(x >> 8) & 0xff for x in lm_info[o + 64 * q:o + 64 * q + 64] if (x >> 24) & 1]) for q in range(sc["n_tiles"])]
            for q in range(sc["n_tiles"]):
                info = lm_info[o + 64 * q:o + 64 * q + 64]
                valid, m = (info >> 24) & 1, (info >> 8) & 0xff
                assert valid[0] and (np.diff(valid) <= 0).all() and (np.diff(np.where(valid, m, 0)) <= 0).all(), (name, q)
                const = ((info >> 16) & 1).astype(bool)
                tiles += bool((const[:-1] & (valid[1:] == 1) & (m[1:] == m[:-1]) & ~const[1:]).any())
        assert tiles > 0, "no constant landmark in front of a free one with as many factors"
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
    """The batch of 32 — the four windows in turn — solved once: (names by place, H, g, E and eg of the first eight places)."""
    names = [list(WINDOWS)[w % len(WINDOWS)] for w in range(B)]
    return names, run(backends(), [window(n) for n in names], range(2 * len(WINDOWS)), full=True)


@gpu
@pytest.mark.parametrize("fail", [0, 1])
def test_against_extended_precision(backends, mixed, oracle, fail):
    names, got = mixed if not fail else (mixed[0], run(backends(1), [window(n) for n in mixed[0]], range(len(WINDOWS))))
    fails = []
    for w in range(len(WINDOWS)):
        ref = reference(names[w], oracle, 10.0 if fail else 1.0)
        ratios, f = ne.compare_system(got[w], ref, ne.K, "%s%s:" % (names[w], ", after an invalid step" if fail else ""),
                                      names=("E", "eg") if fail else ("H", "g", "E", "eg"))
        print("%-14s fail=%d  %s" % (names[w], fail, "  ".join("%s %8.2f" % kv for kv in ratios.items())))
        fails += f
    assert not fails, "\n".join(fails)


@gpu
def test_same_bits_run_to_run_and_place_to_place(backends, mixed):
    names, got = mixed
    again = run(backends(), [window(n) for n in names], range(len(WINDOWS)), full=True)
    for w in range(len(WINDOWS)):
        assert same_bits(got[w], again[w]), "%s: two runs differ" % names[w]
        assert same_bits(got[w], got[w + len(WINDOWS)]), "%s: places %d and %d of the batch differ" % (names[w], w, w + len(WINDOWS))


@gpu
@pytest.mark.parametrize("k", range(len(WINDOWS)))
def test_alone_in_a_batch_of_copies(backends, mixed, k):
    names, got = mixed
    alone = run(backends(), [window(names[k])] * B, (0, B - 1))
    assert same_bits(alone[0], {q: got[k][q] for q in ("E", "eg")}), "%s: among 31 others and in a batch of 32 copies differ" % names[k]
    assert same_bits(alone[0], alone[B - 1])
