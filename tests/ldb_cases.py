"""Seeded synthetic vocabularies, keyframes, databases and match cases of the loop database (tests/test_ldb_model.py on the CPU,
tests/test_gpu_ldb.py on the device). Nothing depends on a vocabulary file. A revisit is an earlier keyframe with a few bits of its
descriptors flipped. K_SCORE is the margin of the cases: measured and checked by tests/test_ldb_model.py."""
import numpy as np

import ldb_np as ln

MAX_CHILDREN, CAP = 256, 4096
K_SCORE = 32.0     # the smallest power of two >= 4 r_cpu, r_cpu = 6.80 (test_ldb_model.test_margin_of_the_cases)
U = 2.0 ** -53


def rand_desc(rng, n):
    return rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)


def flip(rng, d, nbits):
    """descriptor d [4] with exactly nbits distinct bits flipped."""
    out = np.array(d, np.uint64).copy()
    for b in rng.choice(256, nbits, replace=False):
        out[int(b) // 64] ^= np.uint64(1) << np.uint64(int(b) % 64)
    return out


def tree_from_parents(parents, rng, k, L, zero_words=(), weighting=0):
    """A vocabulary dict from the parent of every node in file order (ids 1 .. n ascending); leaves get the word ids in file order."""
    n = len(parents)
    has_child = np.zeros(n + 1, bool)
    has_child[np.array(parents)] = True
    leaves = [i for i in range(1, n + 1) if not has_child[i]]
    weight = rng.uniform(0.3, 9.0, n)
    for w in zero_words:
        weight[leaves[w] - 1] = 0.0
    desc = np.zeros((n + 1, 4), np.uint64)      # a child's descriptor is its parent's with 48 bits flipped: a leaf's own descriptor finds it
    desc[0] = rand_desc(rng, 1)[0]
    for i, p in enumerate(parents):
        desc[i + 1] = flip(rng, desc[p], 48)
    return dict(k=k, L=L, scoring=0, weighting=weighting, node_id=np.arange(1, n + 1, dtype=np.int32), parent_id=np.array(parents, np.int32), weight=weight,
                descriptor=desc[1:].copy(), word_id=np.arange(len(leaves), dtype=np.int32), word_node=np.array(leaves, np.int32))


def balanced(k, L, seed, **kw):
    parents, level = [], [0]
    for _ in range(L):
        nxt = []
        for p in level:
            for _ in range(k):
                parents.append(p)
                nxt.append(len(parents))
        level = nxt
    return tree_from_parents(parents, np.random.default_rng(seed), k, L, **kw)


def trees():
    t = {"k3L2": balanced(3, 2, 11), "k10L3": balanced(10, 3, 12), "wide_root": balanced(MAX_CHILDREN, 1, 13), "k1": balanced(1, 3, 14),
         "stopped": balanced(3, 2, 15, zero_words=(0, 4, 8)), "tf": balanced(3, 2, 16, weighting=1)}
    # unbalanced: node 1 is a leaf at level 1 beside the depth-3 subtrees of 2 and 3; node 5 has two children, node 4 one (k = 3)
    t["unbalanced"] = tree_from_parents([0, 0, 0, 2, 2, 2, 3, 3, 4, 5, 5, 6, 6, 6, 7, 7, 7, 8, 8, 8], np.random.default_rng(17), 3, 3)
    # twins: nodes 1 and 2 (siblings under the root) and leaves 4 and 5 (under node 1) carry one descriptor each pair: the first wins
    tw = balanced(3, 2, 18)
    tw["descriptor"][1] = tw["descriptor"][0]
    tw["descriptor"][4] = tw["descriptor"][3]
    t["twins"] = tw
    return t


def leaf_desc(voc):
    return voc["descriptor"][np.array(voc["word_node"]) - 1]


def keyframe(voc, rng, n, nflip=12):
    """n descriptors near random leaves of the tree, with keypoints."""
    ld = leaf_desc(voc)
    pick = rng.integers(0, len(ld), n)
    desc = np.array([flip(rng, ld[p], int(rng.integers(0, nflip + 1))) for p in pick], np.uint64).reshape(n, 4)
    pts = rng.uniform(0, 640, (n, 2)).astype(np.float32)
    return desc, pts, ((pts - 320) / 460).astype(np.float32)


def revisit(rng, kf, nbits=3, keep=1.0):
    desc, pts, ptsn = kf
    sel = np.flatnonzero(rng.uniform(size=len(desc)) < keep)
    d = np.array([flip(rng, desc[i], int(rng.integers(0, nbits + 1))) for i in sel], np.uint64).reshape(len(sel), 4)
    return d, pts[sel], ptsn[sel]


def repeated_word_keyframe(voc, copies=7):
    """`copies` exact copies of the descriptor of a leaf whose repeated sum differs from copies * w, beside five other leaves."""
    ld, wt, model = leaf_desc(voc), voc["weight"][np.array(voc["word_node"]) - 1], ln.Vocab(voc)
    for w in range(len(ld)):
        if wt[w] > 0 and model.descend(ld[w])[0] == w:
            s = np.float64(wt[w])
            for _ in range(copies - 1):
                s = s + np.float64(wt[w])
            if s != np.float64(copies) * np.float64(wt[w]):
                desc = np.concatenate([np.repeat(ld[w][None], copies, 0), ld[(w + 1 + np.arange(5)) % len(ld)]])
                pts = np.arange(2.0 * len(desc), dtype=np.float32).reshape(-1, 2)
                return (desc, pts, pts / 500), w
    raise AssertionError("no leaf whose repeated sum differs from the product")


def transform_cases():
    """(tree name, descriptors) pairs for gfbe_ldb_transform: every tree, the sizes around the wave and the workgroup, the cap."""
    t, out = trees(), {}
    for name, voc in t.items():
        rng = np.random.default_rng(100 + len(name))
        out["%s_n65" % name] = (name, keyframe(voc, rng, 65)[0])
    rng = np.random.default_rng(7)
    for n in (0, 1, 63, 64, 257, CAP):
        out["k10L3_n%d" % n] = ("k10L3", keyframe(t["k10L3"], rng, n)[0])
    out["k3L2_cap"] = ("k3L2", keyframe(t["k3L2"], rng, CAP)[0])      # nine words, hundreds of copies each
    out["repeated"] = ("k10L3", repeated_word_keyframe(t["k10L3"])[0][0])
    return out


def main_sequence(n_kf=301, seed=21):
    """301 keyframes on k10L3: a detecting add at every database size 0 .. 300. Sizes 0, 1, 63, 64, 65, 257 and the cap occur; revisits of
    keyframes far back (loops), a pair with no common word, an empty keyframe, a keyframe of one repeated word."""
    voc = trees()["k10L3"]
    rng = np.random.default_rng(seed)
    ld = leaf_desc(voc)
    kfs = []
    special = {2: 0, 3: 1, 7: 63, 8: 64, 9: 65, 20: 257, 30: CAP}
    loops = {70: 5, 75: 12, 90: 71, 120: 15, 121: 16, 122: 120, 180: 100, 200: 40, 250: 41, 251: 7, 299: 150, 300: 9}
    for i in range(n_kf):
        if i in loops:
            kf = revisit(rng, kfs[loops[i]], keep=0.9 if i % 2 else 0.6)
        elif i == 40:
            kf = repeated_word_keyframe(voc)[0]
        elif i == 5:      # leaves under the root's first child only, exact
            kf = (ld[:40].copy(), np.ones((40, 2), np.float32), np.ones((40, 2), np.float32))
        elif i == 6:      # leaves under the root's sixth child only: no word in common with keyframe 5
            kf = (ld[500:540].copy(), np.ones((40, 2), np.float32), np.ones((40, 2), np.float32))
        else:
            kf = keyframe(voc, rng, special.get(i, int(rng.integers(40, 70))))
        kfs.append(kf)
    return voc, kfs


def tie_sequence(seed=22):
    """Keyframes 10 and 11 are identical; keyframe 100 revisits them: two equal raw scores, the lower id first."""
    voc = trees()["k3L2"]
    rng = np.random.default_rng(seed)
    kfs = [keyframe(voc, rng, 20) for _ in range(101)]
    kfs[11] = kfs[10]
    kfs[100] = revisit(rng, kfs[10])
    return voc, kfs


def small_sequences():
    """name -> (tree name, keyframes, options): short databases on the other trees, and the option edges."""
    t, out = trees(), {}
    for name in ("k3L2", "wide_root", "k1", "unbalanced", "twins", "stopped", "tf"):
        rng = np.random.default_rng(300 + len(name))
        kfs = [keyframe(t[name], rng, int(rng.integers(1, 30))) for _ in range(8)]
        kfs.append(revisit(rng, kfs[1]))
        out[name] = (name, kfs, dict(query_gap=3, min_loop_frame=3))
    # the walk's quirk (pose_graph.cpp:505): at steps 8 and 11 result 0 is not the lowest id, and the lowest id of all scores below 0.015
    rng = np.random.default_rng(431)
    kfs = [keyframe(t["k10L3"], rng, int(rng.integers(30, 60))) for _ in range(12)]
    out["quirk"] = ("k10L3", kfs + [revisit(rng, kfs[-1])], dict(query_gap=4, min_loop_frame=4))
    rng = np.random.default_rng(41)
    kfs = [keyframe(t["k10L3"], rng, 50) for _ in range(24)] + [revisit(rng, kfs[0]), revisit(rng, kfs[3])]
    out["sixteen_results"] = ("k10L3", kfs, dict(query_gap=1, min_loop_frame=0, max_results=16, score_first=0.0, score_other=0.0))
    out["one_result_max"] = ("k10L3", kfs, dict(query_gap=1, min_loop_frame=0, max_results=1))
    return out


def refusal_cases():
    """name -> (kcap, dcap, [n of every keyframe], [accepted?])."""
    return {"keyframes": (3, 1000, [10, 10, 10, 10, 5], [1, 1, 1, 0, 0]), "descriptors": (10, 100, [65, 65, 35, 1, 0], [1, 0, 1, 0, 1])}


def match_cases(seed=31):
    """name -> (old descriptors, window descriptors). Random descriptors are about 128 +- 8 apart, so the planted ones decide: exact
    distances 79 and 80, an identical descriptor, two equal old descriptors (the first wins), a window descriptor 200 bits from all."""
    rng = np.random.default_rng(seed)
    out = {}
    for n_old, n_win in ((0, 65), (1, 1), (63, 300), (64, 65), (65, 0), (1025, 300)):
        old, win = rand_desc(rng, n_old), rand_desc(rng, n_win)
        if n_old >= 63 and n_win >= 65:
            old[40] = old[17]                                # equal best distances at two indices
            win[0] = flip(rng, old[5], 79)
            win[1] = flip(rng, old[6], 80)
            win[2] = old[7]
            win[3] = flip(rng, old[17], 9)
            win[4] = flip(rng, old[n_old - 1], 30)
            win[64] = flip(rng, old[n_old - 2], 78)
        out["old%d_win%d" % (n_old, n_win)] = (old, win)
    one = rand_desc(rng, 1)
    out["far"] = (one, np.array([flip(rng, one[0], 200), flip(rng, one[0], 128), flip(rng, one[0], 127)], np.uint64))
    return out
