#!/usr/bin/env python3
"""Times the loop database host to host (numpy arrays in, numpy arrays out, the one device wait inside) on a synthetic k = 10, L = 6
vocabulary (1 111 110 nodes, 10^6 words; a child's descriptor is its parent's with about 64 bits flipped):

  gfbe_ldb_add_keyframe with detection at 100, 1 000 and 5 000 held keyframes of about 1 000 descriptors (the database grows by one per
  call, 16 calls per row), gfbe_ldb_transform of the same keyframe beside it (rules 1 and 2 alone, its own wait), and
  gfbe_ldb_match of 150 window descriptors against a keyframe of 1 000 and of 1 000 against one of 4 000.

After a warm-up the rows are run alternately `--reps` times each: median and max - min of the repetitions. Beside every row the host
build of ground-fusion2_amd/csrc/gfbe_ldb.h (tests/ldb_host_shim.cpp, g++ -O2) doing the same walk on one core, median of 3. That figure
says how far a one-thread walk of this code is from the device; it says nothing about DBoW2, which cannot be built here (no boost, no
OpenCV), and whose inverted file visits only the rows of the query's words where this walk merges every eligible entry's list.
The split of an add into "transform" and "the rest" (query, selection, store) is by difference of two host-to-host times, not a
profile. Writes profiles/ldb_bench.txt.

    python tools/diag_ldb_bench.py [--reps 15] [--no-host] [--out profiles/ldb_bench.txt]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _gfbe_import import gf      # noqa: E402

PU64, PI, PD, PU8 = C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)


def rand64(rng, shape):
    return rng.integers(0, 1 << 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64)


def tree(k, L, rng):
    """The vocabulary dict of a full k-ary tree of L levels in level order; (r1 & r2) flips a quarter of the bits per level."""
    level = rand64(rng, (1, 4))
    ids, parents, descs, first = [], [], [], 0
    for _ in range(L):
        n = len(level) * k
        child = np.repeat(level, k, 0) ^ (rand64(rng, (n, 4)) & rand64(rng, (n, 4)))
        ids.append(np.arange(first + 1, first + n + 1))
        parents.append(np.repeat(np.arange(first + 1 - len(level), first + 1) if first else np.zeros(1, np.int64), k))
        descs.append(child)
        first += n
        level = child
    n_leaf = len(level)
    node_id = np.concatenate(ids).astype(np.int32)
    return dict(k=k, L=L, scoring=0, weighting=0, node_id=node_id, parent_id=np.concatenate(parents).astype(np.int32), weight=rng.uniform(0.3, 9.0, len(node_id)),
                descriptor=np.concatenate(descs), word_id=np.arange(n_leaf, dtype=np.int32), word_node=ids[-1].astype(np.int32)), level


def keyframe(rng, leaves, n):
    d = leaves[rng.integers(0, len(leaves), n)] ^ (rand64(rng, (n, 4)) & rand64(rng, (n, 4)) & rand64(rng, (n, 4)) & rand64(rng, (n, 4)))
    p = rng.uniform(0, 640, (n, 2)).astype(np.float32)
    return np.ascontiguousarray(d), p, (p / 460).astype(np.float32)


def host_shim():
    out = os.path.join(ROOT, "tests", "_build", "ldb_host_shim.so")
    src = os.path.join(ROOT, "tests", "ldb_host_shim.cpp")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.shim_ldb_create.restype = C.c_void_p
    lib.shim_ldb_create.argtypes = [C.c_int] * 5 + [PI, PI, PD, PU64, C.c_int, PI, PI]
    lib.shim_ldb_add.argtypes = [C.c_void_p, C.c_int, PU64, C.c_int, C.POINTER(C.c_int), PD, C.POINTER(C.c_int), PI, PD]
    lib.shim_ldb_match.argtypes = [C.c_void_p, C.c_int, C.c_int, PU64, C.c_int, C.c_int, PU8, PI, PI, PI]
    lib.shim_ldb_destroy.argtypes = [C.c_void_p]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--sizes", default="100,1000,5000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldb_bench.txt"))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    rng = np.random.default_rng(1)
    voc, leaves = tree(10, 6, rng)
    holder = gf.abi.LdbVocabHolder(voc)
    be = gf.Backend(device=0)
    pool = [keyframe(rng, leaves, int(rng.integers(900, 1100))) for _ in range(200)]      # the held keyframes cycle through these
    probes = [keyframe(rng, leaves, 1000) for _ in range(a.reps + 1)]
    dbs = {}
    for H in sizes:
        db = be.loop_database(holder, H + a.reps + 8, (H + a.reps + 8) * 1100)
        for i in range(H):
            db.add_keyframe(*pool[i % len(pool)], detect_loop=False)
        dbs[H] = db
    mdb = be.loop_database(holder, 4, 8192)
    old1k, old4k = keyframe(rng, leaves, 1000), keyframe(rng, leaves, 4000)
    mdb.add_keyframe(*old1k, detect_loop=False)
    mdb.add_keyframe(*old4k, detect_loop=False)
    win150 = old1k[0][rng.integers(0, 1000, 150)] ^ (rand64(rng, (150, 4)) & rand64(rng, (150, 4)) & rand64(rng, (150, 4)))
    win1k = old4k[0][rng.integers(0, 4000, 1000)] ^ (rand64(rng, (1000, 4)) & rand64(rng, (1000, 4)) & rand64(rng, (1000, 4)))
    rows = [("add_keyframe+detect", H) for H in sizes] + [("transform", H) for H in sizes] + [("match 150 x 1000", 0), ("match 1000 x 4000", 1)]

    def run(row, rep):
        what, arg = row
        if what == "add_keyframe+detect":
            return dbs[arg].add_keyframe(*probes[rep])
        if what == "transform":
            return dbs[arg].transform(probes[rep][0])
        return mdb.match(arg, win150 if arg == 0 else win1k)
    info = {}
    for row in rows:      # warm-up
        info[row] = run(row, a.reps)
    times = {row: [] for row in rows}
    for rep in range(a.reps):
        for row in rows:
            t0 = time.perf_counter()
            run(row, rep)
            times[row].append((time.perf_counter() - t0) * 1e3)
    host = {row: float("nan") for row in rows}
    if not a.no_host:
        lib = host_shim()
        c = holder.c
        io, thr = (C.c_int * 3)(4, 50, 50), (C.c_double * 2)(0.05, 0.015)
        nr, rid, rs = C.c_int(), np.zeros(16, np.int32), np.zeros(16)

        def hadd(h, kf, detect):
            t0 = time.perf_counter()
            lib.shim_ldb_add(h, len(kf[0]), kf[0].ctypes.data_as(PU64), detect, io, thr, C.byref(nr), rid.ctypes.data_as(PI), rs.ctypes.data_as(PD))
            return (time.perf_counter() - t0) * 1e3
        h = lib.shim_ldb_create(c.k, c.L, c.scoring, c.weighting, c.n_nodes, c.node_id, c.parent_id, c.weight, c.descriptor, c.n_words, c.word_id, c.word_node)
        held = 0
        for H in sorted(sizes):      # one host database grows through the sizes
            while held < H:
                hadd(h, pool[held % len(pool)], 0)
                held += 1
            host[("add_keyframe+detect", H)] = float(np.median([hadd(h, probes[r], 1) for r in range(3)]))
            held += 3
            host[("transform", H)] = float(np.median([hadd(h, probes[r], 0) for r in range(3)]))      # (transform and append, no query)
            held += 3
        lib.shim_ldb_destroy(h)
        h = lib.shim_ldb_create(c.k, c.L, c.scoring, c.weighting, c.n_nodes, c.node_id, c.parent_id, c.weight, c.descriptor, c.n_words, c.word_id, c.word_node)
        hadd(h, old1k, 0)
        hadd(h, old4k, 0)
        for row, win in ((("match 150 x 1000", 0), win150), (("match 1000 x 4000", 1), win1k)):
            st, bi, bd, src = np.zeros(len(win), np.uint8), np.zeros(len(win), np.int32), np.zeros(len(win), np.int32), np.zeros(len(win), np.int32)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                lib.shim_ldb_match(h, row[1], len(win), np.ascontiguousarray(win).ctypes.data_as(PU64), 128, 80, st.ctypes.data_as(PU8), bi.ctypes.data_as(PI),
                                   bd.ctypes.data_as(PI), src.ctypes.data_as(PI))
                ts.append((time.perf_counter() - t0) * 1e3)
            host[row] = float(np.median(ts))
        lib.shim_ldb_destroy(h)
    lines = ["gfbe_ldb_* host to host on a k = 10, L = 6 vocabulary, keyframes of about 1 000 descriptors, %d alternating repetitions after a warm-up (ms: median, max - min)" % a.reps,
             "%22s %8s %12s %10s %18s  %s" % ("call", "held", "median ms", "spread ms", "one core host ms", "note")]
    for row in rows:
        what, arg = row
        out = info[row]
        if what == "add_keyframe+detect":
            note = "results %d, best score %.3f" % (len(out["result_id"]), out["result_score"][0] if len(out["result_id"]) else 0.0)
        elif what == "transform":
            note = "%d words of %d descriptors" % (len(out["bow_word"]), len(out["word"]))
        else:
            note = "%d matched" % out["n_matched"]
        lines.append("%22s %8s %12.3f %10.3f %18.3f  %s" % (what, arg if what[0] != "m" else "-", float(np.median(times[row])), max(times[row]) - min(times[row]), host[row], note))
    for H in sizes:
        lines.append("add - transform at %d held: %.3f ms (query, selection, store; by difference of two host-to-host medians, not a profile)"
                     % (H, float(np.median(times[("add_keyframe+detect", H)])) - float(np.median(times[("transform", H)]))))
    lines.append("one core host: the host build of gfbe_ldb.h (g++ -O2) doing the same walk, median of 3; the transform row's host figure is transform + append.")
    lines.append("It is not DBoW2, which cannot be built here; DBoW2's inverted file visits only the rows of the query's words.")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
