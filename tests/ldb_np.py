"""The model of the loop database (gfbe_ldb_*): the reference's walk written plainly, with the floating type as an argument.

  descent       TemplatedVocabulary::transform(feature)   dense_map/src/ThirdParty/DBoW/TemplatedVocabulary.h:1217-1258
  BoW vector    transform(features), addWeight, normalize :1065-1121, BowVector.cpp:34-84
  query, add    queryL1 over the inverted file, add       TemplatedDatabase.h:656-723
  decision      detectLoop                                dense_map/src/pose_graph.cpp:476-511
  search        searchInAera / searchByBRIEFDes           dense_map/src/keyframe.cpp:194-244

and an independent restatement of the query (a merge of forward lists) and of the search (argmin over a distance matrix). A descriptor
is uint64 [4]; dt is np.float64 (the device's arithmetic) or np.longdouble (the check of the cases' margins)."""
import numpy as np

POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)
DEFAULTS = dict(max_results=4, query_gap=50, min_loop_frame=50, max_keyframe_descriptors=4096, match_start=128, match_max=80, score_first=0.05, score_other=0.015)


def hamming(f, B):
    """Hamming distances of descriptor f [4] to the rows of B [m, 4]."""
    x = np.bitwise_xor(np.ascontiguousarray(B, np.uint64).reshape(-1, 4), np.ascontiguousarray(f, np.uint64).reshape(1, 4))
    return POP8[x.view(np.uint8)].sum(1)


class Vocab:
    """loadBin's tree (:1509-1561): the children of a node are its nodes in file order."""

    def __init__(self, voc):
        n = len(voc["node_id"])
        self.children = [[] for _ in range(n + 1)]
        self.desc = np.zeros((n + 1, 4), np.uint64)
        self.weight = np.zeros(n + 1)
        self.word = np.full(n + 1, -1, np.int64)
        for i in range(n):
            nid, pid = int(voc["node_id"][i]), int(voc["parent_id"][i])
            self.children[pid].append(nid)
            self.desc[nid] = voc["descriptor"][i]
            self.weight[nid] = voc["weight"][i]
        for w, nid in zip(voc["word_id"], voc["word_node"]):
            self.word[int(nid)] = int(w)
        self.n_words = len(voc["word_id"])

    def descend(self, f):
        """(word id, weight) of one descriptor: a later child wins only with a strictly smaller distance; the walk ends at a leaf."""
        node = 0
        while True:
            kids = self.children[node]
            d = hamming(f, self.desc[kids])
            best, best_d = kids[0], d[0]
            for j in range(1, len(kids)):
                if d[j] < best_d:
                    best, best_d = kids[j], d[j]
            node = best
            if not self.children[node]:
                return int(self.word[node]), float(self.weight[node])

    def transform(self, descs, dt=np.float64):
        """words [n] of every descriptor, and the BoW vector (ascending word ids, values of type dt)."""
        words, v = [], {}
        for f in np.asarray(descs, np.uint64).reshape(-1, 4):
            w, wt = self.descend(f)
            words.append(w)
            if wt > 0:
                v[w] = v[w] + dt(wt) if w in v else dt(wt)      # addWeight: one addition per further copy
        ids = sorted(v)
        norm = dt(0.0)
        for w in ids:
            norm = norm + abs(v[w])
        if norm > 0:
            for w in ids:
                v[w] = v[w] / norm
        return np.array(words, np.int32), np.array(ids, np.int32), np.array([v[w] for w in ids], dt)


def decide(ids, scores, frame_index, o=DEFAULTS):
    """detectLoop's decision (pose_graph.cpp:476-511): (find_loop, loop_index)."""
    find_loop = False
    if len(ids) >= 1 and scores[0] > o["score_first"]:
        for i in range(1, len(ids)):
            if scores[i] > o["score_other"]:
                find_loop = True
    if find_loop and frame_index > o["min_loop_frame"]:
        min_index = -1
        for i in range(len(ids)):
            if min_index == -1 or (ids[i] < min_index and scores[i] > o["score_other"]):
                min_index = int(ids[i])
        return find_loop, min_index
    return find_loop, -1


class Database:
    """The database of detectLoop: the inverted file of TemplatedDatabase plus, per entry, what the handle keeps."""

    def __init__(self, voc, kcap=1 << 20, dcap=1 << 40, dt=np.float64, **opt):
        self.voc = voc if isinstance(voc, Vocab) else Vocab(voc)
        self.o, self.dt, self.kcap, self.dcap = dict(DEFAULTS, **opt), dt, kcap, dcap
        self.ifile = {}          # word -> [(entry, value)] in ascending entry id
        self.entries = []        # dict(bow_word, bow_value, desc, pts, pts_norm)
        self.n_desc = self.n_bow = self.n_refused = 0

    def size(self):
        return dict(n_keyframes=len(self.entries), n_descriptors=self.n_desc, n_bow=self.n_bow, n_refused=self.n_refused)

    def query_raw(self, ids, vals, max_id):
        """queryL1's walk (:656-697): {entry: raw score}, the rows visited word by word in ascending word id."""
        pairs = {}
        n_entries = len(self.entries)
        for w, q in zip(ids, vals):
            for e, d in self.ifile.get(int(w), ()):
                if e < max_id or max_id == -1 or e == n_entries - 1:
                    value = abs(q - d) - abs(q) - abs(d)
                    pairs[e] = pairs[e] + value if e in pairs else value
        return pairs

    def query_raw_forward(self, ids, vals, max_id):
        """The restatement: per entry the intersection of two ascending lists, the terms added in ascending word id."""
        pairs = {}
        n_entries = len(self.entries)
        for e, ent in enumerate(self.entries):
            if not (e < max_id or max_id == -1 or e == n_entries - 1):
                continue
            _, ia, ib = np.intersect1d(ids, ent["bow_word"], assume_unique=True, return_indices=True)
            if len(ia) == 0:
                continue
            q, d = vals[ia], ent["bow_value"][ib]
            terms = np.abs(q - d) - np.abs(q) - np.abs(d)
            acc = terms[0]
            for t in terms[1:]:
                acc = acc + t
            pairs[e] = acc
        return pairs

    def rank(self, pairs):
        """sorted by (raw, id), cut to max_results, the reported score -raw / 2."""
        order = sorted(pairs.items(), key=lambda kv: (kv[1], kv[0]))[:self.o["max_results"]]
        return np.array([e for e, _ in order], np.int32), np.array([-r / self.dt(2.0) for _, r in order], self.dt)

    def add_keyframe(self, desc, pts, pts_norm, detect_loop=True, forward=False):
        """dict(index, loop_index, find_loop, result_id, result_score, pairs); a keyframe that does not fit is refused whole."""
        desc = np.ascontiguousarray(desc, np.uint64).reshape(-1, 4)
        none = dict(index=-1, loop_index=-1, find_loop=False, result_id=np.zeros(0, np.int32), result_score=np.zeros(0, self.dt), pairs={})
        frame_index = len(self.entries)
        if frame_index >= self.kcap or self.n_desc + len(desc) > self.dcap:
            self.n_refused += 1
            return none
        _, ids, vals = self.voc.transform(desc, self.dt)
        out = dict(none, index=frame_index)
        if detect_loop:
            pairs = (self.query_raw_forward if forward else self.query_raw)(ids, vals, frame_index - self.o["query_gap"])
            rid, rs = self.rank(pairs)
            find_loop, loop_index = decide(rid, rs, frame_index, self.o)
            out.update(loop_index=loop_index, find_loop=find_loop, result_id=rid, result_score=rs, pairs=pairs)
        for w, v in zip(ids, vals):
            self.ifile.setdefault(int(w), []).append((frame_index, v))
        self.entries.append(dict(bow_word=ids, bow_value=vals, desc=desc.copy(), pts=np.array(pts, np.float32).reshape(-1, 2),
                                 pts_norm=np.array(pts_norm, np.float32).reshape(-1, 2)))
        self.n_desc += len(desc)
        self.n_bow += len(ids)
        return out

    def match(self, old_index, window, vectorised=False):
        e = self.entries[old_index]
        return (search_matrix if vectorised else search)(window, e["desc"], e["pts"], e["pts_norm"], self.o)


def _pack(status, bi, bd, pts, pts_norm):
    src = np.flatnonzero(status).astype(np.int32)
    return dict(status=status, best_index=bi, best_dist=bd, n_matched=len(src), matched_src=src,
                matched_pt=pts[bi[src]].reshape(-1, 2), matched_pt_norm=pts_norm[bi[src]].reshape(-1, 2))


def search(window, old, pts, pts_norm, o=DEFAULTS):
    """searchByBRIEFDes: the double loop of searchInAera, then reduceVector."""
    window, old = np.asarray(window, np.uint64).reshape(-1, 4), np.asarray(old, np.uint64).reshape(-1, 4)
    n = len(window)
    status, bi, bd = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        best, index = o["match_start"], -1
        d = hamming(window[i], old)
        for j in range(len(old)):
            if d[j] < best:
                best, index = int(d[j]), j
        bi[i], bd[i] = index, best
        status[i] = 1 if index != -1 and best < o["match_max"] else 0
    return _pack(status, bi, bd, pts, pts_norm)


def search_matrix(window, old, pts, pts_norm, o=DEFAULTS):
    """The restatement: the distance matrix, its first argmin per row, masked by the start distance."""
    window, old = np.asarray(window, np.uint64).reshape(-1, 4), np.asarray(old, np.uint64).reshape(-1, 4)
    n = len(window)
    if len(old) == 0 or n == 0:
        bi, bd = np.full(n, -1, np.int32), np.full(n, o["match_start"], np.int32)
    else:
        D = POP8[np.bitwise_xor(window[:, None, :], old[None, :, :]).view(np.uint8)].sum(2).astype(np.int32)
        bi = D.argmin(1).astype(np.int32)
        bd = D[np.arange(n), bi].astype(np.int32)
        miss = bd >= o["match_start"]
        bi[miss], bd[miss] = -1, o["match_start"]
    status = ((bi != -1) & (bd < o["match_max"])).astype(np.uint8)
    return _pack(status, bi, bd, pts, pts_norm)
