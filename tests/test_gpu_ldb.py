"""gfbe_ldb_* on the device against the FP64 model (tests/ldb_np.py) over tests/ldb_cases.py. Every output is compared for equality:
word ids, the float64 bits of BoW values and scores, the result order, loop_index, the counts, and every output of the descriptor
search. The margins of the cases are checked on the CPU (tests/test_ldb_model.py: K = 32 from r_cpu = 6.80); here nothing is a tolerance,
because every rule is an integer operation or one FP64 operation in a stated order. Measured on the MI355X: every comparison of the 42
tests holds (the whole file runs in 2.1 s; the largest case, 301 detecting adds, 0.55 s)."""
import ctypes as C

import numpy as np
import pytest

from _gfbe_import import gf
import ldb_cases as lc
import ldb_np as ln

pytestmark = pytest.mark.gpu
abi = gf.abi
TREES = lc.trees()
SMALL = lc.small_sequences()
MATCH = lc.match_cases()
TRANSFORM = lc.transform_cases()
_MODELS = {}


@pytest.fixture(scope="module")
def be():
    b = gf.Backend(device=0)
    yield b
    b.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _sequence(name):
    if name == "main":
        voc, kfs = lc.main_sequence()
        return voc, kfs, {}
    if name == "tie":
        voc, kfs = lc.tie_sequence()
        return voc, kfs, {}
    tname, kfs, opt = SMALL[name]
    return TREES[tname], kfs, opt


def _model(name):
    """The model's run of a sequence: computed once, shared by the tests and left unchanged."""
    if name not in _MODELS:
        voc, kfs, opt = _sequence(name)
        db = ln.Database(voc, **opt)
        _MODELS[name] = (voc, kfs, opt, db, [db.add_keyframe(*kf) for kf in kfs])
    return _MODELS[name]


def _same_step(got, want):
    assert got["index"] == want["index"] and got["loop_index"] == want["loop_index"]
    assert np.array_equal(got["result_id"], want["result_id"]) and np.array_equal(_bits(got["result_score"]), _bits(want["result_score"]))


def _same_entry(got, want):
    assert np.array_equal(got["bow_word"], want["bow_word"]) and np.array_equal(_bits(got["bow_value"]), _bits(want["bow_value"]))
    for k in ("desc", "pts", "pts_norm"):
        assert np.array_equal(got[k], want[k]), k


def _same_match(got, want):
    for k in ("status", "best_index", "best_dist", "n_matched", "matched_src", "matched_pt", "matched_pt_norm"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name", list(TRANSFORM))
def test_transform_against_the_model(be, name):
    """Every tree (k = 3 L = 2, k = 10 L = 3, 256 children at the root, k = 1, the unbalanced one, the twin descriptors, stopped words,
    TF weighting), n = 0, 1, 63, 64, 65, 257 and the cap of 4096, nine words with hundreds of copies each, and the word met seven times
    whose repeated sum is not 7 w."""
    tname, desc = TRANSFORM[name]
    words, ids, vals = ln.Vocab(TREES[tname]).transform(desc)
    db = be.loop_database(TREES[tname], 4, 8192)
    try:
        got = db.transform(desc)
        assert np.array_equal(got["word"], words) and np.array_equal(got["bow_word"], ids) and np.array_equal(_bits(got["bow_value"]), _bits(vals))
        assert db.size() == dict(n_keyframes=0, n_descriptors=0, n_bow=0, n_refused=0)
    finally:
        db.close()


@pytest.mark.parametrize("name", ["main", "tie"] + list(SMALL))
def test_sequence_against_the_model(be, name):
    """A detecting add at every step. main: every database size 0 .. 300 (both max_id quirks at 49 and below, frame_index > 50), keyframes of
    0, 1, 63, 64, 65, 257 and 4096 descriptors, no common word, exactly one result, revisits. tie: two identical keyframes, the lower id
    first. quirk: result 0 not the lowest id, a lower id below 0.015. The other trees; max_results 16 and 1."""
    voc, kfs, opt, model, outs = _model(name)
    db = be.loop_database(voc, len(kfs), sum(len(k[0]) for k in kfs) + 1, **opt)
    try:
        for kf, want in zip(kfs, outs):
            _same_step(db.add_keyframe(*kf), want)
        assert db.size() == model.size()
        for e in sorted({0, 1, 2, 3, len(kfs) // 2, len(kfs) - 1} & set(range(len(kfs)))):
            _same_entry(db.entry(e), model.entries[e])
    finally:
        db.close()


def test_add_without_detection_gives_the_same_database(be):
    """addKeyFrameIntoVoc for the first 60 keyframes of the main sequence (no query, no result), then detecting adds: the results of the
    model, whose database does not depend on how its entries were added."""
    voc, kfs, opt, model, outs = _model("main")
    db = be.loop_database(voc, 128, 1 << 15)
    try:
        for i, kf in enumerate(kfs[:60]):
            got = db.add_keyframe(*kf, detect_loop=False)
            assert got["index"] == i and got["loop_index"] == -1 and len(got["result_id"]) == 0
        for kf, want in zip(kfs[60:80], outs[60:80]):
            _same_step(db.add_keyframe(*kf), want)
        _same_entry(db.entry(30), model.entries[30])      # (the keyframe of 4096 descriptors)
    finally:
        db.close()


@pytest.mark.parametrize("name", list(lc.refusal_cases()))
def test_refused_keyframes_leave_the_handle_unchanged(be, name):
    kcap, dcap, ns, accepted = lc.refusal_cases()[name]
    rng = np.random.default_rng(5)
    kfs = [lc.keyframe(TREES["k3L2"], rng, n) for n in ns]
    model = ln.Database(TREES["k3L2"], kcap=kcap, dcap=dcap, query_gap=1, min_loop_frame=0)
    db = be.loop_database(TREES["k3L2"], kcap, dcap, query_gap=1, min_loop_frame=0)
    try:
        for kf, ok in zip(kfs, accepted):
            before = (db.size(), [db.entry(e) for e in range(model.size()["n_keyframes"])])
            want = model.add_keyframe(*kf)
            got = db.add_keyframe(*kf)
            _same_step(got, want)
            assert (got["index"] >= 0) == bool(ok)
            assert db.size() == model.size()
            if not ok:      # size but for the refusal count, and the pools
                assert dict(before[0], n_refused=before[0]["n_refused"] + 1) == db.size()
                for e, ent in enumerate(before[1]):
                    _same_entry(db.entry(e), ent)
        assert db.size()["n_refused"] == accepted.count(0)
        for e in range(model.size()["n_keyframes"]):
            _same_entry(db.entry(e), model.entries[e])
        if model.entries and len(model.entries[0]["desc"]):
            _same_match(db.match(0, kfs[0][0]), model.match(0, kfs[0][0]))
    finally:
        db.close()


def test_same_bits_alone_and_after_a_larger_database(be):
    """The quirk sequence, a transform and a match on a fresh handle; then the same after a larger database (60 keyframes of the main
    sequence, one of 4096 descriptors) lived and died on the context, and on that larger handle's own scratch: the same bits."""
    voc, kfs, opt, model, outs = _model("quirk")
    old, win = MATCH["old63_win300"]

    def run(db):
        steps = [db.add_keyframe(*kf) for kf in kfs]
        return steps, db.transform(kfs[3][0]), db.match(2, win)
    db = be.loop_database(voc, 64, 1 << 15, **opt)
    try:
        alone = run(db)
    finally:
        db.close()
    big = be.loop_database(voc, 64, 1 << 15)
    try:
        for kf in lc.main_sequence()[1][:60]:
            big.add_keyframe(*kf)
        t_big = big.transform(kfs[3][0])      # (after a 4096-descriptor vector went through the same scratch)
    finally:
        big.close()
    db = be.loop_database(voc, 64, 1 << 15, **opt)
    try:
        after = run(db)
    finally:
        db.close()
    for a, b, want in zip(alone[0], after[0], outs):
        _same_step(a, want)
        _same_step(b, want)
    for t in (alone[1], after[1], t_big):
        for k in ("word", "bow_word"):
            assert np.array_equal(t[k], alone[1][k])
        assert np.array_equal(_bits(t["bow_value"]), _bits(alone[1]["bow_value"]))
    _same_match(alone[2], after[2])
    _same_match(alone[2], model.match(2, win))


@pytest.mark.parametrize("name", list(MATCH))
def test_match_against_the_model(be, name):
    """n_window 0, 1, 65, 300 against keyframes of 0, 1, 63, 64, 65, 1025 descriptors: best distances of exactly 79 (a match) and 80 (none),
    an identical descriptor, two equal old descriptors (the first wins), a best match in the last tile, window descriptors 128 and 200
    bits from everything (index -1, distance 128)."""
    old, win = MATCH[name]
    pts = np.arange(2.0 * len(old), dtype=np.float32).reshape(-1, 2)
    db = be.loop_database(TREES["k3L2"], 4, 4096)
    try:
        db.add_keyframe(lc.rand_desc(np.random.default_rng(3), 7), np.zeros((7, 2)), np.zeros((7, 2)), detect_loop=False)
        assert db.add_keyframe(old, pts, -pts, detect_loop=False)["index"] == 1
        _same_match(db.match(1, win), ln.search(win, old, pts, -pts))
    finally:
        db.close()


def test_match_with_other_thresholds(be):
    old, win = MATCH["old64_win65"]
    pts = np.arange(2.0 * len(old), dtype=np.float32).reshape(-1, 2)
    for start, mx in ((80, 80), (128, 79), (257, 200), (1, 80)):
        db = be.loop_database(TREES["k3L2"], 4, 4096, match_start=start, match_max=mx)
        try:
            db.add_keyframe(old, pts, -pts, detect_loop=False)
            _same_match(db.match(0, win), ln.search(win, old, pts, -pts, dict(ln.DEFAULTS, match_start=start, match_max=mx)))
        finally:
            db.close()


def test_match_against_a_keyframe_added_before_and_after_300_others(be):
    voc, kfs, opt, model, outs = _model("main")
    old, win = MATCH["old1025_win300"]
    pts = np.arange(2.0 * len(old), dtype=np.float32).reshape(-1, 2)
    want = ln.search(win, old, pts, -pts)
    db = be.loop_database(voc, 400, 1 << 16)
    try:
        db.add_keyframe(old, pts, -pts, detect_loop=False)
        for kf in kfs[:300]:
            db.add_keyframe(*kf, detect_loop=False)
        assert db.add_keyframe(old, pts, -pts, detect_loop=False)["index"] == 301
        _same_match(db.match(0, win), want)
        _same_match(db.match(301, win), want)
        _same_match(db.match(10, win), ln.search(win, kfs[9][0], kfs[9][1], kfs[9][2]))
    finally:
        db.close()


def test_bad_input_paths_leave_the_handle_untouched(be):
    voc = TREES["k3L2"]
    rng = np.random.default_rng(9)
    with pytest.raises(gf.BackendError):
        be.loop_database(dict(voc, scoring=1))
    with pytest.raises(gf.BackendError):
        be.loop_database(dict(voc, parent_id=np.where(np.arange(len(voc["parent_id"])) == 3, 9, voc["parent_id"])))
    with pytest.raises(gf.BackendError):
        be.loop_database(voc, max_results=17)
    db = be.loop_database(voc, 8, 1024, max_keyframe_descriptors=64)
    try:
        kf = lc.keyframe(voc, rng, 20)
        db.add_keyframe(*kf)
        size, ent = db.size(), db.entry(0)
        big = lc.keyframe(voc, rng, 65)
        rc, _ = db.add_keyframe_raw(*big)
        assert rc == abi.BAD_INPUT and b"max_keyframe_descriptors" in be.lib.gfbe_last_error(be.ctx)
        f = db._f
        PI, PU64, PF = C.POINTER(abi.c_i), abi.PU64, abi.PF
        d, p, n = kf[0], kf[1], abi.c_i(-7)
        u64, pf = d.ctypes.data_as(PU64), p.ctypes.data_as(PF)
        assert f("add_keyframe")(be.ctx, db.h, -1, u64, pf, pf, 1, C.byref(n), None, None, None, None) == abi.BAD_INPUT
        assert f("add_keyframe")(be.ctx, db.h, 20, None, pf, pf, 1, C.byref(n), None, None, None, None) == abi.BAD_INPUT
        assert f("add_keyframe")(be.ctx, db.h, 20, u64, None, pf, 0, C.byref(n), None, None, None, None) == abi.BAD_INPUT
        assert f("transform")(be.ctx, db.h, 65, big[0].ctypes.data_as(PU64), None, C.byref(n), None, None) == abi.BAD_INPUT
        assert f("transform")(be.ctx, db.h, 5, None, None, C.byref(n), None, None) == abi.BAD_INPUT
        for old_index in (-1, 1, 99):
            assert db.match_raw(old_index, d)[0] == abi.BAD_INPUT and b"held keyframe" in be.lib.gfbe_last_error(be.ctx)
        assert f("match")(be.ctx, db.h, 0, -1, u64, None, None, None, C.byref(n), None, None, None) == abi.BAD_INPUT
        assert f("match")(be.ctx, db.h, 0, 5, None, None, None, None, C.byref(n), None, None, None) == abi.BAD_INPUT
        for e in (-1, 1):
            assert f("download_entry")(be.ctx, db.h, e, C.byref(n), None, None, C.byref(n), None, None, None) == abi.BAD_INPUT
        assert n.value == -7 and db.size() == size
        _same_entry(db.entry(0), ent)
        other = gf.Backend(device=0)
        try:
            assert f("size")(other.ctx, db.h, None) == abi.BAD_INPUT      # a handle of another context
        finally:
            other.close()
        assert db.add_keyframe(*lc.keyframe(voc, rng, 64))["index"] == 1      # the cap itself is accepted, and the handle still works
    finally:
        db.close()
