"""The loop database without a GPU: the model (tests/ldb_np.py: the reference's walk) against its independent restatement and against
hand cases; the margins of the cases (tests/ldb_cases.py) against the model run in longdouble; the host build of
ground-fusion2_amd/csrc/gfbe_ldb.h (a plain C++ compiler, tests/ldb_host_shim.cpp) against the model bit for bit; the vocabulary check,
one rejection per rule; the same header under the address and undefined-behaviour sanitizers in a program of its own
(tests/ldb_host_main.cpp); and the C ABI's contract without a device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from _gfbe_import import gf
import ldb_cases as lc
import ldb_np as ln

abi = gf.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
HDR = os.path.join(ROOT, "ground-fusion2_amd", "csrc", "gfbe_ldb.h")
PD, PI, PU64, PU8 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
TREES = lc.trees()
_RUNS = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run_sequence(voc, kfs, dt=np.float64, forward=False, **opt):
    db = ln.Database(voc, dt=dt, **opt)
    return db, [db.add_keyframe(*kf, forward=forward) for kf in kfs]


def main_run(dt=np.float64):
    """The model's run of the main sequence: computed once per type and left unchanged."""
    if dt not in _RUNS:
        voc, kfs = lc.main_sequence()
        _RUNS[dt] = (kfs,) + run_sequence(voc, kfs, dt)
    return _RUNS[dt]


# ---- hand cases

def _tiny():
    """Root with two leaves: node 1 = all zeros (word 0, weight 2), node 2 = all ones (word 1, weight 0.5)."""
    return dict(k=2, L=1, scoring=0, weighting=0, node_id=[1, 2], parent_id=[0, 0], weight=[2.0, 0.5],
                descriptor=np.array([[0] * 4, [2 ** 64 - 1] * 4], np.uint64), word_id=[0, 1], word_node=[1, 2])


def test_hand_descent_and_bow_vector():
    v = ln.Vocab(_tiny())
    zero, ones = np.zeros(4, np.uint64), np.full(4, 2 ** 64 - 1, np.uint64)
    half = np.array([2 ** 64 - 1, 2 ** 64 - 1, 0, 0], np.uint64)          # 128 from both: the first child wins the tie
    assert v.descend(zero) == (0, 2.0) and v.descend(ones) == (1, 0.5) and v.descend(half) == (0, 2.0)
    assert ln.hamming(zero, np.array([ones, half, zero])).tolist() == [256, 128, 0]
    words, ids, vals = v.transform(np.array([zero, ones, half, ones]))      # word 0 twice (4.0), word 1 twice (1.0); norm 5
    assert words.tolist() == [0, 1, 0, 1] and ids.tolist() == [0, 1] and vals.tolist() == [4.0 / 5.0, 1.0 / 5.0]
    assert v.transform(np.zeros((0, 4), np.uint64))[1].tolist() == []


def test_hand_query_and_decision():
    db = ln.Database(_tiny(), query_gap=2, min_loop_frame=2)
    zero, ones = np.zeros((1, 4), np.uint64), np.full((1, 4), 2 ** 64 - 1, np.uint64)
    p = np.zeros((1, 2), np.float32)
    assert db.add_keyframe(zero, p, p)["result_id"].tolist() == []                       # empty database
    out = db.add_keyframe(ones, p, p)                                                    # no word in common with entry 0: absent, not 0
    assert out["result_id"].tolist() == [] and out["loop_index"] == -1
    out = db.add_keyframe(np.concatenate([zero, ones]), np.zeros((2, 2)), np.zeros((2, 2)))      # q = (0.8, 0.2); max_id = 0: entry 1 only
    assert out["result_id"].tolist() == [1] and out["result_score"].tolist() == [-((abs(0.2 - 1.0) - 0.2) - 1.0) / 2.0]
    out = db.add_keyframe(zero, p, p)                                                    # max_id = 1: entries 0 and 2 (the previous one)
    assert out["result_id"].tolist() == [0, 2] and out["result_score"].tolist() == [1.0, 0.8]
    assert out["find_loop"] and out["loop_index"] == 0
    # the decision walk on its own: one result is no loop; result 0's id is taken unconditionally; a lower id needs a score above 0.015
    assert ln.decide([3], [0.9], 60) == (False, -1)
    assert ln.decide([7, 3], [0.9, 0.02], 60) == (True, 3) and ln.decide([7, 3, 1], [0.9, 0.02, 0.015], 60) == (True, 3)
    assert ln.decide([7, 9, 1], [0.9, 0.02, 0.001], 60) == (True, 7) and ln.decide([7, 9], [0.9, 0.02], 50) == (True, -1)
    assert ln.decide([7, 9], [0.05, 0.02], 60) == (False, -1) and ln.decide([7, 9], [0.9, 0.015], 60) == (False, -1)


def test_hand_search():
    old = np.array([[0] * 4, [1, 0, 0, 0], [0] * 4], np.uint64)
    pts = np.arange(6, dtype=np.float32).reshape(3, 2)
    win = np.array([[0] * 4, [3, 0, 0, 0], [2 ** 64 - 2, 2 ** 64 - 1, 1, 0], [2 ** 64 - 1, 2 ** 64 - 2, 0, 0]], np.uint64)
    out = ln.search(win, old, pts, pts + 10)
    assert out["best_index"].tolist() == [0, 1, -1, 1] and out["best_dist"].tolist() == [0, 1, 128, 126] and out["status"].tolist() == [1, 1, 0, 0]
    assert out["matched_src"].tolist() == [0, 1] and out["matched_pt"].tolist() == [[0, 1], [2, 3]] and out["matched_pt_norm"].tolist() == [[10, 11], [12, 13]]


# ---- the cases hold what they are for, and the model agrees with its restatement

def test_repeated_sum_differs_from_the_product():
    (desc, _, _), w = lc.repeated_word_keyframe(TREES["k10L3"])
    wt = TREES["k10L3"]["weight"][TREES["k10L3"]["word_node"][w] - 1]
    words, ids, vals = ln.Vocab(TREES["k10L3"]).transform(desc)
    assert (words == w).sum() == 7
    raw = np.float64(wt)
    for _ in range(6):
        raw = raw + np.float64(wt)
    assert raw != 7.0 * wt                                   # otherwise the case proves nothing
    prod = [7.0 * wt if i == w else TREES["k10L3"]["weight"][TREES["k10L3"]["word_node"][i] - 1] for i in ids]
    assert not np.array_equal(_bits(vals), _bits(np.array(prod) / np.sum(prod)))      # and the difference reaches the vector


def test_main_sequence_holds_its_cases():
    kfs, db, outs = main_run()
    assert [len(kfs[i][0]) for i in (2, 3, 7, 8, 9, 20, 30)] == [0, 1, 63, 64, 65, 257, lc.CAP]
    assert len(outs) == 301 and [o["index"] for o in outs] == list(range(301))
    assert len(outs[0]["result_id"]) == 0 and len(outs[1]["result_id"]) == 1                  # sizes 0 and 1: exactly one result is no loop
    assert not outs[1]["find_loop"] and len(outs[6]["result_id"]) == 0 and len(outs[3]["result_id"]) == 0      # no common word; an empty previous keyframe
    assert all(len(outs[i]["result_id"]) <= 1 for i in range(49)) and len(outs[49]["result_id"]) == 4           # max_id < -1, then == -1: everyone
    assert outs[49]["find_loop"] and outs[49]["loop_index"] == -1 and outs[50]["result_id"].tolist() == [49]   # max_id = 0: the previous one only
    assert outs[51]["loop_index"] >= 0 and set(outs[51]["result_id"]) <= {0, 50} and set(outs[52]["result_id"]) <= {0, 1, 51}
    assert outs[52]["loop_index"] != outs[52]["result_id"][0] >= 0                             # result 0's id is not the lowest
    for i, j in ((70, 5), (75, 12), (120, 15), (180, 100), (299, 150), (300, 9)):              # the revisits are found
        assert outs[i]["result_id"][0] == j and outs[i]["result_score"][0] > 0.3 and outs[i]["find_loop"]
    assert db.size() == dict(n_keyframes=301, n_descriptors=sum(len(k[0]) for k in kfs), n_bow=sum(len(e["bow_word"]) for e in db.entries), n_refused=0)


def test_small_sequences_hold_their_cases():
    name, kfs, opt = lc.small_sequences()["quirk"]
    _, outs = run_sequence(TREES[name], kfs, **opt)
    for i in (8, 11):      # a lower id whose score is below 0.015 does not replace result 0's successor
        o = outs[i]
        assert o["loop_index"] > min(o["result_id"]) and o["result_score"][list(o["result_id"]).index(min(o["result_id"]))] < 0.015 and o["loop_index"] != o["result_id"][0]
    name, kfs, opt = lc.small_sequences()["sixteen_results"]
    _, outs = run_sequence(TREES[name], kfs, **opt)
    assert len(outs[-1]["result_id"]) == 16 and len(outs[10]["result_id"]) == 10
    voc, kfs = lc.tie_sequence()
    _, outs = run_sequence(voc, kfs)
    o = outs[100]
    assert o["result_id"][:2].tolist() == [10, 11] and _bits(o["result_score"][:1]) == _bits(o["result_score"][1:2])      # equal raw scores: the lower id first


@pytest.mark.parametrize("name", ["main", "tie"] + list(lc.small_sequences()))
def test_model_against_its_restatement_queries(name):
    """The inverted-file walk and the forward-list merge give the same ids, the same score bits and the same decision at every step."""
    if name == "main":
        (voc, kfs), opt = lc.main_sequence(), {}
        a = main_run()[2]
    else:
        if name == "tie":
            (voc, kfs), opt = lc.tie_sequence(), {}
        else:
            tname, kfs, opt = lc.small_sequences()[name]
            voc = TREES[tname]
        a = run_sequence(voc, kfs, **opt)[1]
    b = run_sequence(voc, kfs, forward=True, **opt)[1]
    for x, y in zip(a, b):
        assert np.array_equal(x["result_id"], y["result_id"]) and np.array_equal(_bits(x["result_score"]), _bits(y["result_score"]))
        assert (x["loop_index"], x["find_loop"], x["index"]) == (y["loop_index"], y["find_loop"], y["index"])


def _match_model(old, win, vectorised=False):
    pts = np.arange(2.0 * len(old), dtype=np.float32).reshape(-1, 2)
    return (ln.search_matrix if vectorised else ln.search)(win, old, pts, -pts)


@pytest.mark.parametrize("name", list(lc.match_cases()))
def test_model_against_its_restatement_matches(name):
    old, win = lc.match_cases()[name]
    a, b = _match_model(old, win), _match_model(old, win, True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    if len(old) >= 63 and len(win) >= 65:      # the planted descriptors: 79 matches, 80 does not; identical; the first of two equal; the last tile
        assert a["best_dist"][:5].tolist() == [79, 80, 0, 9, 30] and a["status"][:5].tolist() == [1, 0, 1, 1, 1]
        assert a["best_index"][:5].tolist() == [5, 6, 7, 17, len(old) - 1] and a["best_index"][64] == len(old) - 2 and a["status"][64] == 1
    assert (a["best_dist"][a["best_index"] == -1] == 128).all() and (a["best_dist"][a["best_index"] >= 0] < 128).all()
    if len(old) == 0:
        assert (a["best_index"] == -1).all() and a["n_matched"] == 0
    if name == "far":
        assert a["best_index"].tolist() == [-1, -1, 0] and a["best_dist"].tolist() == [128, 128, 127] and a["n_matched"] == 0


def test_refusals_of_the_model():
    for name, (kcap, dcap, ns, accepted) in lc.refusal_cases().items():
        rng = np.random.default_rng(5)
        db = ln.Database(TREES["k3L2"], kcap=kcap, dcap=dcap)
        got = [db.add_keyframe(*lc.keyframe(TREES["k3L2"], rng, n))["index"] for n in ns]
        assert [g >= 0 for g in got] == [bool(a) for a in accepted], name
        assert db.size()["n_refused"] == accepted.count(0) and db.size()["n_keyframes"] == accepted.count(1)


# ---- the margins of the cases: FP64 against longdouble

MARGIN_CASES = ["main"] + [n for n in lc.small_sequences() if n != "k1"]      # (k = 1 has one word: every score is 1.0, a tie case like tie_sequence)


def _margins(name):
    """(r_cpu, closest gap / (u A)) of one sequence; asserts that FP64 and longdouble take every decision alike."""
    if name == "main":
        (_, db, a), (_, dbl, b), o = main_run(), main_run(np.longdouble), ln.DEFAULTS
    else:
        tname, kfs, opt = lc.small_sequences()[name]
        (db, a), (dbl, b), o = run_sequence(TREES[tname], kfs, **opt), run_sequence(TREES[tname], kfs, np.longdouble, **opt), dict(ln.DEFAULTS, **opt)
    r_cpu, closest = 0.0, np.inf
    for i, (x, y) in enumerate(zip(a, b)):
        ey = dbl.entries[i]
        assert np.array_equal(db.entries[i]["bow_word"], ey["bow_word"]) and set(x["pairs"]) == set(y["pairs"])
        A = {}
        for e in y["pairs"]:
            _, ia, ib = np.intersect1d(ey["bow_word"], dbl.entries[e]["bow_word"], assume_unique=True, return_indices=True)
            q, d = ey["bow_value"][ia], dbl.entries[e]["bow_value"][ib]
            A[e] = float((np.abs(q - d) + np.abs(q) + np.abs(d)).sum())
            r_cpu = max(r_cpu, float(abs(np.longdouble(x["pairs"][e]) - y["pairs"][e])) / (lc.U * A[e]))
        top = sorted(y["pairs"].items(), key=lambda kv: (kv[1], kv[0]))[:o["max_results"] + 1]
        assert [e for e, _ in top] == [e for e, _ in sorted(x["pairs"].items(), key=lambda kv: (kv[1], kv[0]))[:len(top)]]
        for (e0, r0), (e1, r1) in zip(top, top[1:]):
            closest = min(closest, float(r1 - r0) / (lc.U * (A[e0] + A[e1])))
        for e, r in top[:o["max_results"]]:
            for thr in (o["score_first"], o["score_other"]):
                closest = min(closest, float(abs(-r / 2 - thr)) * 2 / (lc.U * A[e]))
        assert (x["loop_index"], x["find_loop"]) == (y["loop_index"], y["find_loop"]) and np.array_equal(x["result_id"], y["result_id"])
    return r_cpu, closest


def test_margin_of_the_cases():
    """Every decision of every sequence but the tie cases (tie_sequence; k1, whose one word makes every score 1.0) is the same in FP64
    and in longdouble, with room: word ids, the ranking of the top max_results + 1 and the side of both thresholds. r_cpu = the worst
    |FP64 - longdouble| / (u A) over all raw scores, A = the sum of |q - d| + |q| + |d| over an entry's common words, u = 2^-53; K = the
    smallest power of two >= 4 r_cpu; every compared pair of raw scores and every threshold is at least K u A away. Measured: r_cpu = 6.80 (main;
    6.70 on sixteen_results, 0.6 .. 3.0 on the small trees: the values carry the rounding of their repeated sums and of the norm, and a score
    adds a term per common word), K = 32; the smallest gap of all cases is 2.9e11 u A (sixteen_results)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("longdouble is no wider than double here")
    got = {name: _margins(name) for name in MARGIN_CASES}
    r_cpu, closest = max(r for r, _ in got.values()), min(c for _, c in got.values())
    print("r_cpu %.3f K %g closest gap / (u A) %.3g" % (r_cpu, lc.K_SCORE, closest), {k: (round(r, 2), float("%.3g" % c)) for k, (r, c) in got.items()})
    assert lc.K_SCORE == 2.0 ** np.ceil(np.log2(4 * r_cpu)), r_cpu
    assert closest >= lc.K_SCORE, closest


# ---- the host build of gfbe_ldb.h

def _cxx(src, out, extra):
    if not CXX:
        pytest.fail("no C++ compiler: gfbe_ldb.h cannot be built for the host")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in (src, HDR)):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([CXX, "-O2", "-std=c++17", "-Wall", "-ffp-contract=off"] + extra + ["-o", out, src], check=True)
    return out


VOC_ARGS = [C.c_int] * 5 + [PI, PI, PD, PU64, C.c_int, PI, PI]


@pytest.fixture(scope="module")
def shim():
    lib = C.CDLL(_cxx(os.path.join(ROOT, "tests", "ldb_host_shim.cpp"), os.path.join(BUILD, "ldb_host_shim.so"), ["-fPIC", "-shared"]))
    lib.shim_ldb_validate.argtypes = VOC_ARGS
    lib.shim_ldb_vocab_error.restype, lib.shim_ldb_vocab_error.argtypes = C.c_char_p, [C.c_int]
    lib.shim_ldb_create.restype, lib.shim_ldb_create.argtypes = C.c_void_p, VOC_ARGS
    lib.shim_ldb_destroy.restype, lib.shim_ldb_destroy.argtypes = None, [C.c_void_p]
    lib.shim_ldb_hamming.argtypes = [PU64, PU64]
    lib.shim_ldb_repeated_sum.restype, lib.shim_ldb_repeated_sum.argtypes = C.c_double, [C.c_double, C.c_int]
    lib.shim_ldb_fits.argtypes = [C.c_longlong] * 5
    lib.shim_ldb_step.argtypes = [C.c_void_p, PU64, C.c_int, C.c_int]
    lib.shim_ldb_transform.argtypes = [C.c_void_p, C.c_int, PU64, PI, PI, PD]
    lib.shim_ldb_add.argtypes = [C.c_void_p, C.c_int, PU64, C.c_int, C.POINTER(C.c_int), PD, C.POINTER(C.c_int), PI, PD]
    lib.shim_ldb_match.argtypes = [C.c_void_p, C.c_int, C.c_int, PU64, C.c_int, C.c_int, PU8, PI, PI, PI]
    lib.shim_ldb_decide.argtypes = [C.c_int, PI, PD, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int)]
    return lib


def _voc_args(voc):
    h = abi.LdbVocabHolder(voc)
    return h, (h.c.k, h.c.L, h.c.scoring, h.c.weighting, h.c.n_nodes, h.c.node_id, h.c.parent_id, h.c.weight, h.c.descriptor, h.c.n_words, h.c.word_id, h.c.word_node)


class HostDb:
    def __init__(self, shim, voc):
        self.shim = shim
        self.holder, args = _voc_args(voc)
        self.h = shim.shim_ldb_create(*args)
        assert self.h

    def close(self):
        self.shim.shim_ldb_destroy(self.h)

    def transform(self, desc):
        d = np.ascontiguousarray(desc, np.uint64).reshape(-1, 4)
        word, bw, bv = np.zeros(len(d), np.int32), np.zeros(len(d), np.int32), np.zeros(len(d))
        n = self.shim.shim_ldb_transform(self.h, len(d), d.ctypes.data_as(PU64), word.ctypes.data_as(PI), bw.ctypes.data_as(PI), bv.ctypes.data_as(PD))
        return word, bw[:n], bv[:n]

    def add(self, desc, detect=True, **opt):
        o = dict(ln.DEFAULTS, **opt)
        d = np.ascontiguousarray(desc, np.uint64).reshape(-1, 4)
        io, thr = (C.c_int * 3)(o["max_results"], o["query_gap"], o["min_loop_frame"]), (C.c_double * 2)(o["score_first"], o["score_other"])
        nr, rid, rs = C.c_int(-1), np.zeros(16, np.int32), np.zeros(16)
        loop = self.shim.shim_ldb_add(self.h, len(d), d.ctypes.data_as(PU64), int(detect), io, thr, C.byref(nr), rid.ctypes.data_as(PI), rs.ctypes.data_as(PD))
        return loop, rid[:nr.value], rs[:nr.value]

    def match(self, old_index, win):
        w = np.ascontiguousarray(win, np.uint64).reshape(-1, 4)
        st, bi, bd, src = np.zeros(len(w), np.uint8), np.zeros(len(w), np.int32), np.zeros(len(w), np.int32), np.zeros(len(w), np.int32)
        m = self.shim.shim_ldb_match(self.h, old_index, len(w), w.ctypes.data_as(PU64), 128, 80, st.ctypes.data_as(PU8), bi.ctypes.data_as(PI), bd.ctypes.data_as(PI),
                                     src.ctypes.data_as(PI))
        return dict(status=st, best_index=bi, best_dist=bd, n_matched=m, matched_src=src[:m])


@pytest.mark.parametrize("name", list(lc.transform_cases()))
def test_host_transform_against_the_model(shim, name):
    tname, desc = lc.transform_cases()[name]
    words, ids, vals = ln.Vocab(TREES[tname]).transform(desc)
    h = HostDb(shim, TREES[tname])
    try:
        w, bw, bv = h.transform(desc)
        assert np.array_equal(w, words) and np.array_equal(bw, ids) and np.array_equal(_bits(bv), _bits(vals))
        v = ln.Vocab(TREES[tname])
        for f in desc[:20]:      # a step's key is the same however many walkers share the children (1, the kernel's 16, 64)
            keys = [shim.shim_ldb_step(h.h, np.ascontiguousarray(f).ctypes.data_as(PU64), 0, n) for n in (1, 16, 64)]
            d = ln.hamming(f, v.desc[v.children[0]])
            assert keys[0] == keys[1] == keys[2] == (int(d.min()) << 8 | int(d.argmin()))
    finally:
        h.close()


@pytest.mark.parametrize("name", ["main", "tie"] + list(lc.small_sequences()))
def test_host_walk_against_the_model(shim, name):
    if name == "main":
        (voc, kfs), opt = lc.main_sequence(), {}
        outs = main_run()[2]
    else:
        if name == "tie":
            (voc, kfs), opt = lc.tie_sequence(), {}
        else:
            tname, kfs, opt = lc.small_sequences()[name]
            voc = TREES[tname]
        outs = run_sequence(voc, kfs, **opt)[1]
    h = HostDb(shim, voc)
    try:
        for kf, o in zip(kfs, outs):
            loop, rid, rs = h.add(kf[0], **opt)
            assert loop == o["loop_index"] and np.array_equal(rid, o["result_id"]) and np.array_equal(_bits(rs), _bits(o["result_score"]))
    finally:
        h.close()


def test_host_match_and_small_functions(shim):
    h = HostDb(shim, TREES["k3L2"])
    try:
        for k, (name, (old, win)) in enumerate(lc.match_cases().items()):
            h.add(old, detect=False)
            got, want = h.match(k, win), _match_model(old, win)
            for key in got:
                assert np.array_equal(got[key], want[key]), (name, key)
    finally:
        h.close()
    a, b = lc.rand_desc(np.random.default_rng(1), 50), lc.rand_desc(np.random.default_rng(2), 50)
    for x, y in zip(a, b):
        assert shim.shim_ldb_hamming(x.ctypes.data_as(PU64), y.ctypes.data_as(PU64)) == ln.hamming(x, y[None])[0]
    for w in (0.1, 1.0 / 3.0, 7.77, 2.0):
        for c in (1, 2, 6, 7, 100):
            s = np.float64(w)
            for _ in range(c - 1):
                s = s + np.float64(w)
            assert shim.shim_ldb_repeated_sum(w, c) == s
    assert shim.shim_ldb_fits(2, 3, 90, 100, 10) == 1 and shim.shim_ldb_fits(3, 3, 0, 100, 0) == 0 and shim.shim_ldb_fits(0, 3, 91, 100, 10) == 0
    for ids, sc, fi in (([7, 3], [0.9, 0.02], 60), ([7, 9, 1], [0.9, 0.02, 0.001], 60), ([7, 9], [0.9, 0.02], 50), ([3], [0.9], 60), ([], [], 60)):
        found = C.c_int(-1)
        i, s = np.array(ids, np.int32), np.array(sc, np.float64)
        loop = shim.shim_ldb_decide(len(ids), i.ctypes.data_as(PI), s.ctypes.data_as(PD), fi, 0.05, 0.015, 50, C.byref(found))
        assert (bool(found.value), loop) == ln.decide(ids, sc, fi)


def _broken(**kw):
    v = {k: (np.array(x).copy() if not np.isscalar(x) else x) for k, x in TREES["unbalanced"].items()}
    for k, (i, x) in kw.items():
        v[k][i] = x
    return v


def test_vocabulary_validation_one_rejection_per_rule(shim):
    def code(voc):
        holder, args = _voc_args(voc)
        return shim.shim_ldb_validate(*args)
    for name, voc in TREES.items():
        assert code(voc) == 0, name
    assert code(dict(TREES["k3L2"], scoring=1)) == 1 and code(dict(TREES["k3L2"], weighting=2)) == 1 and code(dict(TREES["k3L2"], weighting=3)) == 1      # not L1 + TF-IDF / TF
    assert code(dict(TREES["k3L2"], k=0)) == 2 and code(dict(TREES["k3L2"], L=17)) == 2 and code(dict(TREES["k3L2"], k=lc.MAX_CHILDREN + 1)) == 2
    assert code(_broken(node_id=(5, 5))) == 3 and code(_broken(node_id=(5, 0))) == 3 and code(_broken(node_id=(5, 21))) == 3      # twice; outside 1 .. n
    assert code(_broken(parent_id=(3, 9))) == 4 and code(_broken(parent_id=(3, 4))) == 4 and code(_broken(parent_id=(3, -1))) == 4   # a later node; itself; none
    assert code(_broken(weight=(2, -0.5))) == 5 and code(_broken(weight=(2, np.nan))) == 5 and code(_broken(weight=(2, np.inf))) == 5
    wide = lc.balanced(lc.MAX_CHILDREN + 1, 1, 1)
    assert code(dict(wide, k=lc.MAX_CHILDREN)) == 6                                                                                  # 257 children
    assert code(lc.balanced(1, 17, 1)) in (2, 7) and code(dict(lc.balanced(1, 17, 1), L=16)) == 7                                    # 17 levels
    assert code(_broken(word_node=(0, 2))) == 8 and code(_broken(word_id=(1, 0))) == 8 and code(_broken(word_id=(1, 99))) == 8      # a word on an inner node; twice; outside
    v = dict(TREES["unbalanced"])
    v["word_id"], v["word_node"] = v["word_id"][:-1], v["word_node"][:-1]
    assert code(v) == 9                                                                                                              # a leaf without a word
    for c in range(1, 10):
        assert shim.shim_ldb_vocab_error(c)


def test_sanitized_stand_alone_program():
    """gfbe_ldb.h's host functions under -fsanitize=address,undefined in a program of its own (never on code loaded into Python)."""
    exe = _cxx(os.path.join(ROOT, "tests", "ldb_host_main.cpp"), os.path.join(BUILD, "ldb_host_main"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the C ABI without a device

def test_c_abi_without_a_device():
    gf.build_native()
    lib = C.CDLL(gf.lib_path())
    new = [s for s in gf.backend.EXPORTS if s.startswith("gfbe_ldb_")]
    assert len(new) == 8
    for s in new:
        assert hasattr(lib, s), s
        getattr(lib, s).restype = None if s in ("gfbe_ldb_destroy", "gfbe_ldb_default_options") else abi.c_i
    lib.gfbe_create.restype = abi.c_i
    lib.gfbe_last_error.restype = C.c_char_p
    lib.gfbe_ldb_create.argtypes = [C.c_void_p, C.POINTER(abi.LdbVocab), abi.c_i, C.c_int64, C.POINTER(abi.LdbOptions), C.POINTER(C.c_void_p)]
    o = abi.ldb_default_options(lib)
    assert o.struct_size == C.sizeof(abi.LdbOptions) == 48 and C.sizeof(abi.LdbVocab) == 72
    assert (o.max_results, o.query_gap, o.min_loop_frame, o.max_keyframe_descriptors, o.match_start, o.match_max) == (4, 50, 50, 4096, 128, 80)
    assert (o.score_first, o.score_other, o.reserved) == (0.05, 0.015, 0)
    ctx = C.c_void_p()
    assert lib.gfbe_create(C.byref(ctx), -1, None) == abi.OK
    voc = abi.LdbVocabHolder(TREES["k3L2"])
    out = C.c_void_p(0xDEAD)
    assert lib.gfbe_ldb_create(ctx, C.byref(voc.c), 16, 1024, C.byref(o), C.byref(out)) == abi.NO_DEVICE and not out.value
    assert b"no CPU fallback" in lib.gfbe_last_error(ctx)
    assert lib.gfbe_ldb_create(ctx, C.byref(voc.c), 16, 1024, None, C.byref(out)) == abi.NO_DEVICE

    def bad(**kw):
        b = abi.ldb_default_options(lib)
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    for b in (bad(struct_size=44), bad(struct_size=0), bad(max_results=0), bad(max_results=17), bad(query_gap=-1), bad(min_loop_frame=-1), bad(max_keyframe_descriptors=0),
              bad(max_keyframe_descriptors=4097), bad(match_start=0), bad(match_start=258), bad(match_max=-1), bad(score_first=float("nan")), bad(score_other=float("inf"))):
        out = C.c_void_p(0xDEAD)
        assert lib.gfbe_ldb_create(ctx, C.byref(voc.c), 16, 1024, C.byref(b), C.byref(out)) == abi.BAD_INPUT and not out.value
        assert lib.gfbe_last_error(ctx)
    for kc, dc in ((0, 1024), (-1, 1024), ((1 << 24) + 1, 1024), (16, 0), (16, (1 << 26) + 1)):
        assert lib.gfbe_ldb_create(ctx, C.byref(voc.c), kc, dc, C.byref(o), C.byref(out)) == abi.BAD_INPUT, (kc, dc)
    broken = abi.LdbVocabHolder(dict(TREES["k3L2"], scoring=1))
    assert lib.gfbe_ldb_create(ctx, C.byref(broken.c), 16, 1024, C.byref(o), C.byref(out)) == abi.BAD_INPUT and b"L1" in lib.gfbe_last_error(ctx)
    assert lib.gfbe_ldb_create(ctx, None, 16, 1024, C.byref(o), C.byref(out)) == abi.BAD_INPUT
    assert lib.gfbe_ldb_create(ctx, C.byref(voc.c), 16, 1024, C.byref(o), None) == abi.BAD_INPUT and lib.gfbe_ldb_create(None, C.byref(voc.c), 16, 1024, C.byref(o), C.byref(out)) == abi.BAD_INPUT
    # every other entry point: GFBE_NO_DEVICE, nothing written
    d, p = np.zeros((2, 4), np.uint64), np.zeros((2, 2), np.float32)
    n, counts, word = abi.c_i(-7), (abi.c_i * 4)(*[-7] * 4), np.full(2, -7, np.int32)
    u64, pf, pi = lambda a: a.ctypes.data_as(PU64), lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(PI)
    assert lib.gfbe_ldb_transform(ctx, None, 2, u64(d), pi(word), C.byref(n), None, None) == abi.NO_DEVICE
    assert lib.gfbe_ldb_add_keyframe(ctx, None, 2, u64(d), pf(p), pf(p), 1, C.byref(n), C.byref(n), C.byref(n), None, None) == abi.NO_DEVICE
    assert lib.gfbe_ldb_match(ctx, None, 0, 2, u64(d), None, pi(word), None, C.byref(n), None, None, None) == abi.NO_DEVICE
    assert lib.gfbe_ldb_size(ctx, None, counts) == abi.NO_DEVICE
    assert lib.gfbe_ldb_download_entry(ctx, None, 0, C.byref(n), None, None, C.byref(n), None, None, None) == abi.NO_DEVICE
    assert n.value == -7 and list(counts) == [-7] * 4 and word.tolist() == [-7, -7]
    lib.gfbe_ldb_destroy(ctx, None)
    lib.gfbe_destroy(ctx)
