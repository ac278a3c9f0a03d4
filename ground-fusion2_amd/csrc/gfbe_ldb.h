// gfbe_ldb.h — the pieces of the loop database (gfbe_ldb.hip) that need no HIP header: under a plain C++ compiler they are ordinary
// inline functions, under hipcc the per-element ones are __host__ __device__ (tests/ldb_host_shim.cpp compiles them for the host).
//
//   descent of a descriptor, children in file order, strict <     dense_map/src/ThirdParty/DBoW/TemplatedVocabulary.h:1217-1258
//   BoW vector: repeated sums, L1 norm in ascending word id       :1065-1121, BowVector.cpp:34-84
//   queryL1: who takes part, the ordered score, -raw / 2          TemplatedDatabase.h:656-723
//   detectLoop: the decision and the walk for loop_index          dense_map/src/pose_graph.cpp:476-511
//   searchInAera: best = 128, strict <, status                    dense_map/src/keyframe.cpp:194-223
//
// Every operation is an integer operation or one IEEE FP64 addition, subtraction, fabs, comparison or division in the order written
// here; there is no multiply-add. The model tests/ldb_np.py reproduces every function bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define GF_LDB_HD __host__ __device__ inline
#else
#define GF_LDB_HD inline
#endif

namespace gfd {

constexpr int LDB_MAX_CHILDREN = 256;      // the child position is the low 8 bits of a descent key (GFBE_LDB_MAX_CHILDREN)
constexpr int LDB_MAX_DEPTH = 16;
constexpr int LDB_MAX_RESULTS = 16;
constexpr int LDB_MAX_KF_DESC = 4096;      // the BoW kernel sorts one keyframe's words in LDS: 16 KB of ids + 32 KB of values
constexpr int LDB_SUB = 16;                // lanes of a wave that share one descriptor's descent
constexpr int LDB_KEY_NONE = 0x7FFFFFFF;

// Hamming distance of two 256-bit descriptors (DVision BRIEF::distance, HammingDis of keyframe.cpp:571-576)
GF_LDB_HD int ldb_hamming(const uint64_t *a, const uint64_t *b) {
  int d = 0;
  for (int w = 0; w < 4; w++) {
#if defined(__HIP_DEVICE_COMPILE__)
    d += __popcll(a[w] ^ b[w]);
#else
    d += __builtin_popcountll(a[w] ^ b[w]);
#endif
  }
  return d;
}

// One descent step, the share of one walker: the smallest key (distance << 8 | position) over the children at positions first,
// first + stride, ... of a node whose children are child[0 .. count). The minimum over all walkers' keys is the reference's choice: the
// smallest distance, the lowest position among equals (a later child wins only with a strictly smaller distance, :1243).
GF_LDB_HD int ldb_step_key(const uint64_t *f, const uint64_t *node_desc, const int *child, int count, int first, int stride) {
  int best = LDB_KEY_NONE;
  for (int p = first; p < count; p += stride) {
    const int key = (ldb_hamming(f, node_desc + 4 * (size_t)child[p]) << 8) | p;
    if (key < best) best = key;
  }
  return best;
}

// the value of a word met c times: ((w + w) + w) + ..., c - 1 additions (BowVector::addWeight, once per descriptor)
GF_LDB_HD double ldb_repeated_sum(double w, int c) {
  double v = w;
  for (int a = 1; a < c; a++) v += w;
  return v;
}

// queryL1's term of a common word (TemplatedDatabase.h:681), left to right
GF_LDB_HD double ldb_term(double q, double d) { return (fabs(q - d) - fabs(q)) - fabs(d); }

// :679 — n_entries is the count before the query's keyframe is added
GF_LDB_HD bool ldb_eligible(int e, int max_id, int n_entries) { return e < max_id || max_id == -1 || e == n_entries - 1; }

// (raw, id) order of the results: ascending raw score, ties to the lower id (the stated deviation: std::sort leaves ties open)
GF_LDB_HD bool ldb_before(double ra, int ia, double rb, int ib) { return ra < rb || (ra == rb && ia < ib); }

// detectLoop's decision on the reported scores (pose_graph.cpp:476-511): returns loop_index, *find_loop as the reference sets it
GF_LDB_HD int ldb_decide(int n, const int *id, const double *score, int frame_index, double first_min, double other_min, int min_frame, int *find_loop) {
  int found = 0;
  if (n >= 1 && score[0] > first_min)
    for (int i = 1; i < n; i++)
      if (score[i] > other_min) found = 1;
  if (find_loop) *find_loop = found;
  if (!(found && frame_index > min_frame)) return -1;
  int min_index = -1;
  for (int i = 0; i < n; i++)
    if (min_index == -1 || (id[i] < min_index && score[i] > other_min)) min_index = id[i];
  return min_index;
}

// searchInAera's key: (distance << 32 | index); the minimum over the old descriptors whose distance is below `start` is the
// reference's (bestDist, bestIndex); nothing below `start` leaves ldb_match_none(start): distance = start, index = -1
GF_LDB_HD unsigned long long ldb_match_none(int start) { return ((unsigned long long)(unsigned)start << 32) | 0xFFFFFFFFull; }
GF_LDB_HD unsigned long long ldb_match_key(int dist, int index) { return ((unsigned long long)(unsigned)dist << 32) | (unsigned)index; }
GF_LDB_HD int ldb_match_status(unsigned long long key, int max_dist) { return (int)(unsigned)key != -1 && (int)(key >> 32) < max_dist; }

// the pool plan: a keyframe of n descriptors is taken iff a keyframe slot and n descriptor slots are left (a BoW vector has at most
// n words, and the word pool has descriptor_capacity slots, so it always fits)
GF_LDB_HD bool ldb_fits(long long n_kf, long long kcap, long long n_desc, long long dcap, long long n) { return n_kf < kcap && n_desc + n <= dcap; }

// ---- host side (plain inline functions: under hipcc they are host functions)

struct LdbVocabIn {
  int k, L, scoring, weighting, n_nodes;
  const int32_t *node_id, *parent_id;
  const double *weight;
  const uint64_t *descriptor;
  int n_words;
  const int32_t *word_id, *word_node;
};

// the tree as the kernels read it, indexed by node id (0 = the root)
struct LdbTree {
  std::vector<uint64_t> desc;       // [n_nodes + 1][4]
  std::vector<int> child_begin, child_count, child, word;      // [n + 1], [n + 1], [n] node ids in file order, [n + 1] word id or -1
  std::vector<double> weight;       // [n + 1]
  int n_words = 0;
};

enum { LDB_V_OK = 0, LDB_V_MODE, LDB_V_SHAPE, LDB_V_NODE_ID, LDB_V_PARENT, LDB_V_WEIGHT, LDB_V_CHILDREN, LDB_V_DEPTH, LDB_V_WORD, LDB_V_LEAF };

inline const char *ldb_vocab_error(int code) {
  switch (code) {
    case LDB_V_MODE: return "only L1 scoring (0) with TF-IDF (0) or TF (1) weighting is supported";
    case LDB_V_SHAPE: return "k outside 1 .. GFBE_LDB_MAX_CHILDREN, L outside 1 .. 16, no node, a negative count or a NULL array";
    case LDB_V_NODE_ID: return "a node id outside 1 .. n_nodes or defined twice";
    case LDB_V_PARENT: return "a parent that is neither the root nor an earlier-defined node";
    case LDB_V_WEIGHT: return "a weight that is not finite and non-negative";
    case LDB_V_CHILDREN: return "a node with more than GFBE_LDB_MAX_CHILDREN children";
    case LDB_V_DEPTH: return "a node deeper than 16 levels";
    case LDB_V_WORD: return "a word id outside 0 .. n_words - 1 or defined twice, or a word on a node that is no leaf or has a word already";
    case LDB_V_LEAF: return "a leaf without a word";
    default: return "";
  }
}

// loadBin's walk (TemplatedVocabulary.h:1509-1561) with every assumption it makes checked; fills *T when the vocabulary is sound
inline int ldb_plan_vocab(const LdbVocabIn &v, LdbTree *T) {
  if (v.scoring != 0 || (v.weighting != 0 && v.weighting != 1)) return LDB_V_MODE;
  if (v.k < 1 || v.k > LDB_MAX_CHILDREN || v.L < 1 || v.L > LDB_MAX_DEPTH || v.n_nodes < 1 || v.n_words < 1 || v.n_nodes > (1 << 28) || !v.node_id || !v.parent_id ||
      !v.weight || !v.descriptor || !v.word_id || !v.word_node)
    return LDB_V_SHAPE;
  const size_t N = (size_t)v.n_nodes + 1;
  std::vector<int> depth(N, -1), parent(N, 0), count(N, 0);
  depth[0] = 0;
  for (int i = 0; i < v.n_nodes; i++) {
    const int id = v.node_id[i], p = v.parent_id[i];
    if (id < 1 || id > v.n_nodes || depth[(size_t)id] >= 0) return LDB_V_NODE_ID;
    if (p < 0 || p > v.n_nodes || p == id || depth[(size_t)p] < 0) return LDB_V_PARENT;
    if (!(v.weight[i] >= 0.0) || !std::isfinite(v.weight[i])) return LDB_V_WEIGHT;
    if (++count[(size_t)p] > LDB_MAX_CHILDREN) return LDB_V_CHILDREN;
    if ((depth[(size_t)id] = depth[(size_t)p] + 1) > LDB_MAX_DEPTH) return LDB_V_DEPTH;
    parent[(size_t)id] = p;
  }
  std::vector<int> word(N, -1);
  std::vector<char> seen((size_t)v.n_words, 0);
  for (int i = 0; i < v.n_words; i++) {
    const int w = v.word_id[i], nd = v.word_node[i];
    if (w < 0 || w >= v.n_words || seen[(size_t)w] || nd < 1 || nd > v.n_nodes || count[(size_t)nd] != 0 || word[(size_t)nd] >= 0) return LDB_V_WORD;
    seen[(size_t)w] = 1;
    word[(size_t)nd] = w;
  }
  for (size_t id = 1; id < N; id++)
    if (count[id] == 0 && word[id] < 0) return LDB_V_LEAF;
  if (!T) return LDB_V_OK;
  T->n_words = v.n_words;
  T->desc.assign(4 * N, 0); T->weight.assign(N, 0.0); T->word = word;
  T->child_count = count; T->child_begin.assign(N, 0); T->child.assign((size_t)v.n_nodes, 0);
  int run = 0;
  for (size_t id = 0; id < N; id++) { T->child_begin[id] = run; run += count[id]; }
  std::vector<int> fill(N, 0);
  for (int i = 0; i < v.n_nodes; i++) {      // the children of a node are its nodes in file order (push_back, :1538)
    const size_t id = (size_t)v.node_id[i], p = (size_t)v.parent_id[i];
    T->child[(size_t)(T->child_begin[p] + fill[p]++)] = (int)id;
    T->weight[id] = v.weight[i];
    for (int w = 0; w < 4; w++) T->desc[4 * id + (size_t)w] = v.descriptor[4 * (size_t)i + (size_t)w];
  }
  return LDB_V_OK;
}

// ---- the same walk on one thread (the shim of the tests, and the one-core figure of tools/diag_ldb_bench.py)

// the leaf a descriptor falls into: its node id
inline int ldb_host_descend(const LdbTree &T, const uint64_t *f) {
  int node = 0;
  do {
    const int key = ldb_step_key(f, T.desc.data(), T.child.data() + T.child_begin[(size_t)node], T.child_count[(size_t)node], 0, 1);
    node = T.child[(size_t)(T.child_begin[(size_t)node] + (key & 255))];
  } while (T.child_count[(size_t)node] != 0);
  return node;
}

struct LdbBow { std::vector<int> word; std::vector<double> value; };

// transform (:1065-1121): the words of weight > 0 sorted, values by repeated sums per run, the L1 norm in ascending word id
inline void ldb_host_transform(const LdbTree &T, int n, const uint64_t *desc, int *word_out, LdbBow *v) {
  std::vector<std::pair<int, double>> met;
  for (int i = 0; i < n; i++) {
    const int node = ldb_host_descend(T, desc + 4 * (size_t)i), w = T.word[(size_t)node];
    if (word_out) word_out[i] = w;
    if (T.weight[(size_t)node] > 0.0) met.emplace_back(w, T.weight[(size_t)node]);
  }
  std::sort(met.begin(), met.end());
  v->word.clear(); v->value.clear();
  double norm = 0.0;
  for (size_t a = 0; a < met.size();) {
    size_t b = a;
    while (b < met.size() && met[b].first == met[a].first) b++;
    v->word.push_back(met[a].first);
    v->value.push_back(ldb_repeated_sum(met[a].second, (int)(b - a)));
    norm += fabs(v->value.back());
    a = b;
  }
  if (norm > 0.0)
    for (double &x : v->value) x /= norm;
}

// queryL1 over forward lists: per entry the merge of two ascending lists, the terms added in ascending word id from the first one;
// the results in (raw, id) order cut to max_results, the reported score -raw / 2. Returns the number of results.
inline int ldb_host_query(const std::vector<LdbBow> &db, const LdbBow &q, int max_id, int max_results, int *id, double *score) {
  const int E = (int)db.size();
  std::vector<double> raw;
  std::vector<int> ids;
  for (int e = 0; e < E; e++) {
    if (!ldb_eligible(e, max_id, E)) continue;
    const LdbBow &d = db[(size_t)e];
    size_t a = 0, b = 0;
    bool have = false;
    double acc = 0.0;
    while (a < q.word.size() && b < d.word.size()) {
      if (q.word[a] < d.word[b]) a++;
      else if (q.word[a] > d.word[b]) b++;
      else {
        const double t = ldb_term(q.value[a], d.value[b]);
        acc = have ? acc + t : t;
        have = true; a++; b++;
      }
    }
    if (have) { raw.push_back(acc); ids.push_back(e); }
  }
  int n = 0;
  std::vector<char> taken(raw.size(), 0);
  for (; n < max_results && n < (int)raw.size(); n++) {
    int best = -1;
    for (size_t j = 0; j < raw.size(); j++)
      if (!taken[j] && (best < 0 || ldb_before(raw[j], ids[j], raw[(size_t)best], ids[(size_t)best]))) best = (int)j;
    taken[(size_t)best] = 1;
    id[n] = ids[(size_t)best]; score[n] = -raw[(size_t)best] / 2.0;
  }
  return n;
}

// searchByBRIEFDes + reduceVector: best_index / best_dist / status per window descriptor, the compacted window indices; returns n_matched
inline int ldb_host_match(int n_old, const uint64_t *old_desc, int n_window, const uint64_t *win, int start, int max_dist, uint8_t *status, int *best_index,
                          int *best_dist, int *matched_src) {
  int m = 0;
  for (int i = 0; i < n_window; i++) {
    unsigned long long key = ldb_match_none(start);
    for (int j = 0; j < n_old; j++) {
      const int d = ldb_hamming(win + 4 * (size_t)i, old_desc + 4 * (size_t)j);
      if (d < (int)(key >> 32)) key = ldb_match_key(d, j);
    }
    best_index[i] = (int)(unsigned)key; best_dist[i] = (int)(key >> 32);
    status[i] = (uint8_t)ldb_match_status(key, max_dist);
    if (status[i]) matched_src[m++] = i;
  }
  return m;
}

}  // namespace gfd
