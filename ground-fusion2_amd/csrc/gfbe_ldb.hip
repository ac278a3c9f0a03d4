// gfbe_ldb.hip — the loop database of the loop-closure thread held on the device: the vocabulary tree, the keyframes' BoW vectors as
// forward lists, their descriptors and keypoints, the query with its decision, and the descriptor search against a held keyframe.
//
//   detectLoop          transform, query, add, decision     dense_map/src/pose_graph.cpp:432-512     gfbe_ldb_add_keyframe (detect_loop = 1)
//   addKeyFrameIntoVoc  add without a query                 :514-527                                 gfbe_ldb_add_keyframe (detect_loop = 0)
//   searchByBRIEFDes    searchInAera, reduceVector          dense_map/src/keyframe.cpp:194-244, 374-380   gfbe_ldb_match
//
// The rules and their order of operations are in gfbe_ldb.h and in section f3d of include/gfbe.h. Every sum whose order matters is
// done in that order: the repeated sum of a word by the one thread that owns the word, the norm by one lane walking the vector in LDS,
// an entry's score by one wave whose lanes fetch the terms of 64 entry words and then add the hits in ascending lane (= word) order.
// No FP64 atomics, no tree. A keyframe's size, its entry id and whether it fits are known to the host exactly (every accepted keyframe
// adds n descriptors), so a refusal costs no wait; the counts live in device memory (meta) all the same and the kernels read the
// bases from there. Workgroups communicate only across kernel boundaries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"
#include "gfbe_ldb.h"
#include "gfbe_handle.h"

using namespace gfd;

namespace {
enum { LM_NKF = 0, LM_NDESC, LM_NBOW, LM_NREFUSED, LM_QN, LM_META = 8 };
constexpr int LDB_THREADS = 256, LDB_BOW_THREADS = 1024, LDB_QUERY_BLOCKS = 512, LDB_MAX_WINDOW = 1 << 20;

struct LdbResult {      // what a detecting add and a transform bring back
  int n_results, loop_index, n_bow, pad;
  int id[LDB_MAX_RESULTS];
  double score[LDB_MAX_RESULTS];
};
struct LdbTreeDev {
  const uint64_t *desc; const int *child_begin, *child_count, *child, *word;
};
}  // namespace

struct gfbe_ldb : gfbe_handle {
  gfbe_ldb_options opt;
  int kcap = 0;
  long long dcap = 0;
  // the vocabulary, indexed by node id (0 = the root)
  uint64_t *t_desc = nullptr;
  int *t_child_begin = nullptr, *t_child_count = nullptr, *t_child = nullptr, *t_word = nullptr;
  double *t_word_weight = nullptr;      // [n_words] the weight of a word's leaf
  // the pools: forward lists, descriptors, keypoints; one row of ent per entry: bow begin, bow count, descriptor begin, count
  int *bow_word = nullptr; double *bow_val = nullptr;                      // [dcap]
  uint64_t *desc = nullptr; float *pts = nullptr, *ptsn = nullptr;        // [dcap][4], [dcap][2]
  long long *ent = nullptr;                                                // [kcap][4]
  // one call's scratch
  int *word_of = nullptr, *q_word = nullptr; double *q_val = nullptr;      // [max_keyframe_descriptors]
  double *raw = nullptr; int *has = nullptr;                               // [kcap]
  int *meta = nullptr;
  // exact host mirrors
  std::vector<long long> kf_begin; std::vector<int> kf_n;
  long long n_desc = 0;
};

namespace {

// Rule 1: LDB_SUB lanes per descriptor, lane c takes the children at positions c, c + 16, ...; the minimum of the packed keys is the
// reference's choice. Every loop is wave-uniform (the four descriptors of a wave walk until the last is at a leaf).
__global__ __launch_bounds__(LDB_THREADS) void k_ldb_descend(int n, const uint64_t *desc, LdbTreeDev T, int *word_of) {
  const int i = (blockIdx.x * LDB_THREADS + threadIdx.x) / LDB_SUB, sub = threadIdx.x & (LDB_SUB - 1);
  const bool live = i < n;
  uint64_t f[4] = {0, 0, 0, 0};
  if (live) for (int w = 0; w < 4; w++) f[w] = desc[4 * (size_t)i + w];
  int node = 0;
  bool done = !live;
  for (int level = 0; level < LDB_MAX_DEPTH && __any(!done); level++) {
    int key = LDB_KEY_NONE, begin = 0;
    if (!done) {
      begin = T.child_begin[node];
      key = ldb_step_key(f, T.desc, T.child + begin, T.child_count[node], sub, LDB_SUB);
    }
#pragma unroll
    for (int o = LDB_SUB / 2; o >= 1; o >>= 1) key = min(key, __shfl_xor(key, o, 64));
    if (!done) {
      node = T.child[begin + (key & 255)];
      done = T.child_count[node] == 0;
    }
  }
  if (live && sub == 0) word_of[i] = T.word[node];
}

// Rule 2 in one workgroup: the words of positive weight sorted in LDS (bitonic, stopped words as LDB_KEY_NONE at the end), run heads
// compacted in order, the repeated sum by the head's thread, the norm by thread 0 walking the values in ascending word id, the division.
__global__ __launch_bounds__(LDB_BOW_THREADS) void k_ldb_bow(int n, const int *word_of, const double *word_weight, int *q_word, double *q_val, int *meta, LdbResult *res) {
  __shared__ int s_w[LDB_MAX_KF_DESC];
  __shared__ double s_v[LDB_MAX_KF_DESC];
  __shared__ int lds[20];
  __shared__ double s_norm;
  const int t = threadIdx.x;
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = t; i < P; i += LDB_BOW_THREADS) {
    int w = LDB_KEY_NONE;
    if (i < n) { w = word_of[i]; if (!(word_weight[w] > 0.0)) w = LDB_KEY_NONE; }
    s_w[i] = w;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < P; i += LDB_BOW_THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const int a = s_w[i], b = s_w[l];
          if (((i & k) == 0) ? a > b : a < b) { s_w[i] = b; s_w[l] = a; }
        }
      }
      __syncthreads();
    }
  // every thread owns a contiguous chunk of the sorted list and counts its run heads
  const int chunk = (P + LDB_BOW_THREADS - 1) / LDB_BOW_THREADS, b0 = min(P, t * chunk), b1 = min(P, b0 + chunk);
  int heads = 0, total;
  for (int i = b0; i < b1; i++) heads += s_w[i] != LDB_KEY_NONE && (i == 0 || s_w[i] != s_w[i - 1]);
  int dst = block_exclusive_scan<LDB_BOW_THREADS>(heads, &total, lds);
  for (int i = b0; i < b1; i++) {
    const int w = s_w[i];
    if (w == LDB_KEY_NONE || (i > 0 && w == s_w[i - 1])) continue;
    int c = 1;
    while (i + c < P && s_w[i + c] == w) c++;
    q_word[dst] = w;
    s_v[dst] = ldb_repeated_sum(word_weight[w], c);
    dst++;
  }
  __syncthreads();
  if (t == 0) {
    double norm = 0.0;
    for (int a = 0; a < total; a++) norm += fabs(s_v[a]);
    s_norm = norm;
    meta[LM_QN] = total;
    if (res) res->n_bow = total;
  }
  __syncthreads();
  const double norm = s_norm;
  for (int a = t; a < total; a += LDB_BOW_THREADS) q_val[a] = norm > 0.0 ? s_v[a] / norm : s_v[a];
}

// Rule 3, the scores: the query vector in LDS, one wave per entry that takes part. The lanes look 64 entry words up in the query by
// binary search and form the terms; the hits are added in ascending lane order, which is ascending word id.
__global__ __launch_bounds__(LDB_THREADS) void k_ldb_query(const int *meta, int max_id, const int *q_word, const double *q_val, const long long *ent, const int *bow_word,
                                                           const double *bow_val, double *raw, int *has) {
  __shared__ int s_w[LDB_MAX_KF_DESC];
  __shared__ double s_v[LDB_MAX_KF_DESC];
  const int nq = meta[LM_QN], E = meta[LM_NKF];
  for (int a = threadIdx.x; a < nq; a += LDB_THREADS) { s_w[a] = q_word[a]; s_v[a] = q_val[a]; }
  __syncthreads();
  const int lane = threadIdx.x & 63, waves = LDB_THREADS / 64;
  for (int e = blockIdx.x * waves + (threadIdx.x >> 6); e < E; e += gridDim.x * waves) {
    double acc = 0.0;
    int have = 0;
    if (ldb_eligible(e, max_id, E)) {
      const long long b = ent[4 * (size_t)e];
      const int cnt = (int)ent[4 * (size_t)e + 1];
      for (int c0 = 0; c0 < cnt; c0 += 64) {
        double term = 0.0;
        int hit = 0;
        if (c0 + lane < cnt) {
          const int w = bow_word[b + c0 + lane];
          int lo = 0, hi = nq;
          while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_w[mid] < w) lo = mid + 1; else hi = mid; }
          if (lo < nq && s_w[lo] == w) { hit = 1; term = ldb_term(s_v[lo], bow_val[b + c0 + lane]); }
        }
        unsigned long long m = __ballot(hit);
        while (m) {
          const int l = __ffsll((long long)m) - 1;
          m &= m - 1;
          const double tl = __shfl(term, l, 64);
          acc = have ? acc + tl : tl;
          have = 1;
        }
      }
    }
    if (lane == 0) { raw[e] = acc; has[e] = have; }
  }
}

// Rule 3's selection and rule 4 in one workgroup: max_results rounds, each the minimum in (raw, id) order over the entries behind the
// round before; thread 0 reports -raw / 2 and walks the decision.
struct LdbDecide { int max_results, min_frame; double first_min, other_min; };
__global__ __launch_bounds__(LDB_BOW_THREADS) void k_ldb_select(const int *meta, const double *raw, const int *has, LdbDecide D, LdbResult *res) {
  __shared__ double s_r[LDB_BOW_THREADS / 64];
  __shared__ int s_i[LDB_BOW_THREADS / 64];
  __shared__ double s_pr;
  __shared__ int s_pi;
  const int E = meta[LM_NKF], t = threadIdx.x, lane = t & 63;
  int n = 0;
  double pr = 0.0;
  int pi = -1;      // the result of the round before; pi = -1: none yet
  for (int round = 0; round < D.max_results; round++) {
    double br = 0.0;
    int bi = -1;
    for (int e = t; e < E; e += LDB_BOW_THREADS) {
      if (!has[e]) continue;
      const double r = raw[e];
      if (pi >= 0 && !ldb_before(pr, pi, r, e)) continue;
      if (bi < 0 || ldb_before(r, e, br, bi)) { br = r; bi = e; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double r2 = __shfl_xor(br, o, 64);
      const int i2 = __shfl_xor(bi, o, 64);
      if (i2 >= 0 && (bi < 0 || ldb_before(r2, i2, br, bi))) { br = r2; bi = i2; }
    }
    if (lane == 0) { s_r[t >> 6] = br; s_i[t >> 6] = bi; }
    __syncthreads();
    if (t == 0) {
      for (int q = 1; q < LDB_BOW_THREADS / 64; q++)
        if (s_i[q] >= 0 && (bi < 0 || ldb_before(s_r[q], s_i[q], br, bi))) { br = s_r[q]; bi = s_i[q]; }
      s_pr = br; s_pi = bi;
      if (bi >= 0) { res->id[round] = bi; res->score[round] = -br / 2.0; }
    }
    __syncthreads();
    pr = s_pr; pi = s_pi;
    __syncthreads();
    if (pi < 0) break;
    n++;
  }
  if (t == 0) {
    res->n_results = n;
    res->loop_index = ldb_decide(n, res->id, res->score, E, D.first_min, D.other_min, D.min_frame, nullptr);
  }
}

// Rule 5: the keyframe's vector, descriptors and keypoints behind the pools' ends (k_ldb_commit moves the ends afterwards)
__global__ __launch_bounds__(LDB_THREADS) void k_ldb_store(const int *meta, int n, const uint64_t *d_in, const float *p_in, const float *pn_in, const int *q_word, const double *q_val,
                                                           uint64_t *desc, float *pts, float *ptsn, int *bow_word, double *bow_val) {
  const int i = blockIdx.x * LDB_THREADS + threadIdx.x;
  if (i < n) {
    const size_t d = (size_t)meta[LM_NDESC] + i;
    for (int w = 0; w < 4; w++) desc[4 * d + w] = d_in[4 * (size_t)i + w];
    for (int a = 0; a < 2; a++) { pts[2 * d + a] = p_in[2 * (size_t)i + a]; ptsn[2 * d + a] = pn_in[2 * (size_t)i + a]; }
  }
  if (i < meta[LM_QN]) {
    const size_t b = (size_t)meta[LM_NBOW] + i;
    bow_word[b] = q_word[i]; bow_val[b] = q_val[i];
  }
}
__global__ void k_ldb_commit(int *meta, int n, long long *ent) {
  if (threadIdx.x || blockIdx.x) return;
  const int k = meta[LM_NKF];
  ent[4 * (size_t)k] = meta[LM_NBOW]; ent[4 * (size_t)k + 1] = meta[LM_QN]; ent[4 * (size_t)k + 2] = meta[LM_NDESC]; ent[4 * (size_t)k + 3] = n;
  meta[LM_NKF] = k + 1; meta[LM_NBOW] += meta[LM_QN]; meta[LM_NDESC] += n;
}
__global__ void k_ldb_refuse(int *meta) {
  if (threadIdx.x == 0 && blockIdx.x == 0) meta[LM_NREFUSED]++;
}

// Rule 6: one wave per window descriptor, four per workgroup; the old keyframe's descriptors pass through LDS in tiles of 256, word-major
// so that the lanes read consecutive 8-byte words; every lane keeps the key (distance << 32 | index) over its stride, then a wave minimum.
__global__ __launch_bounds__(LDB_THREADS) void k_ldb_match(int n_window, const uint64_t *win, long long old_begin, int n_old, const uint64_t *desc, int start, int max_dist,
                                                           int *best_index, int *best_dist, int *flag, uint8_t *status) {
  __shared__ uint64_t tile[4][LDB_THREADS];
  const int lane = threadIdx.x & 63, i = blockIdx.x * (LDB_THREADS / 64) + (threadIdx.x >> 6);
  uint64_t f[4] = {0, 0, 0, 0};
  if (i < n_window) for (int w = 0; w < 4; w++) f[w] = win[4 * (size_t)i + w];
  unsigned long long key = ldb_match_none(start);
  for (int j0 = 0; j0 < n_old; j0 += LDB_THREADS) {
    __syncthreads();
    if (j0 + (int)threadIdx.x < n_old) for (int w = 0; w < 4; w++) tile[w][threadIdx.x] = desc[4 * ((size_t)old_begin + j0 + threadIdx.x) + w];
    __syncthreads();
    const int m = min(LDB_THREADS, n_old - j0);
    for (int j = lane; j < m; j += 64) {
      const int d = __popcll(f[0] ^ tile[0][j]) + __popcll(f[1] ^ tile[1][j]) + __popcll(f[2] ^ tile[2][j]) + __popcll(f[3] ^ tile[3][j]);
      if (d < start) key = min(key, ldb_match_key(d, j0 + j));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) key = min(key, (unsigned long long)__shfl_xor((long long)key, o, 64));
  if (i < n_window && lane == 0) {
    const int st = ldb_match_status(key, max_dist);
    best_index[i] = (int)(unsigned)key; best_dist[i] = (int)(key >> 32);
    flag[i] = st; status[i] = (uint8_t)st;
  }
}
// reduceVector in one workgroup: every thread a contiguous chunk of the flags, a scan over the threads, the survivors in ascending order
__global__ __launch_bounds__(LDB_BOW_THREADS) void k_ldb_compact(int n_window, const int *flag, const int *best_index, long long old_begin, const float *pts, const float *ptsn,
                                                                 int *n_matched, int *matched_src, float *matched_pt, float *matched_ptn) {
  __shared__ int lds[20];
  const int t = threadIdx.x, chunk = (n_window + LDB_BOW_THREADS - 1) / LDB_BOW_THREADS, b0 = min(n_window, t * chunk), b1 = min(n_window, b0 + chunk);
  int mine = 0, total;
  for (int i = b0; i < b1; i++) mine += flag[i];
  int dst = block_exclusive_scan<LDB_BOW_THREADS>(mine, &total, lds);
  for (int i = b0; i < b1; i++) {
    if (!flag[i]) continue;
    const size_t p = (size_t)old_begin + best_index[i];
    matched_src[dst] = i;
    for (int a = 0; a < 2; a++) { matched_pt[2 * (size_t)dst + a] = pts[2 * p + a]; matched_ptn[2 * (size_t)dst + a] = ptsn[2 * p + a]; }
    dst++;
  }
  if (t == 0) *n_matched = total;
}

const char *ldb_options_error(const gfbe_ldb_options *o) {
  if (o->struct_size != (int32_t)sizeof(gfbe_ldb_options)) return "gfbe_ldb_options.struct_size does not match this library (ABI mismatch)";
  if (o->max_results < 1 || o->max_results > LDB_MAX_RESULTS) return "max_results outside 1 .. 16";
  if (o->query_gap < 0 || o->min_loop_frame < 0) return "query_gap / min_loop_frame < 0";
  if (o->max_keyframe_descriptors < 1 || o->max_keyframe_descriptors > LDB_MAX_KF_DESC) return "max_keyframe_descriptors outside 1 .. 4096";
  if (o->match_start < 1 || o->match_start > 257 || o->match_max < 0) return "match_start outside 1 .. 257 or match_max < 0";
  if (!std::isfinite(o->score_first) || !std::isfinite(o->score_other)) return "score_first / score_other must be finite";
  return nullptr;
}
LdbTreeDev ldb_tree(const gfbe_ldb *m) { return LdbTreeDev{m->t_desc, m->t_child_begin, m->t_child_count, m->t_child, m->t_word}; }
int ldb_grid(long long n, int per) { return (int)((n + per - 1) / per); }

// rules 1 and 2 of n staged descriptors into q_word / q_val / meta[LM_QN]
void ldb_enqueue_transform(gfbe_ctx *c, gfbe_ldb *m, int n, const uint64_t *d_desc, LdbResult *res) {
  hipStream_t st = ctx_stream(c);
  if (n > 0) hipLaunchKernelGGL(k_ldb_descend, dim3(ldb_grid(n, LDB_THREADS / LDB_SUB)), dim3(LDB_THREADS), 0, st, n, d_desc, ldb_tree(m), m->word_of);
  hipLaunchKernelGGL(k_ldb_bow, dim3(1), dim3(LDB_BOW_THREADS), 0, st, n, (const int *)m->word_of, (const double *)m->t_word_weight, m->q_word, m->q_val, m->meta, res);
}

// rule 5's refusal: a keyframe that does not fit is refused whole and counted; nobody waits. True: the call is over with *rc.
bool ldb_add_refused(gfbe_ctx *c, gfbe_ldb *m, int n, int32_t *index_out, int32_t *loop_index, int32_t *n_results, gfbe_status *rc) {
  if (loop_index) *loop_index = -1;
  if (n_results) *n_results = 0;
  if (ldb_fits((long long)m->kf_n.size(), m->kcap, m->n_desc, m->dcap, n)) return false;
  hipLaunchKernelGGL(k_ldb_refuse, dim3(1), dim3(1), 0, ctx_stream(c), m->meta);
  *rc = hip_ok(c, hipGetLastError(), "hipGetLastError()") ? GFBE_OK : GFBE_DEVICE_ERROR;
  if (index_out) *index_out = -1;
  return true;
}

// The launch half of an add: rules 1 to 5 on n descriptors and keypoints that lie on the device (dd [n][4], dp / dpn [n][2]: in `sg`
// after gfbe_ldb_add_keyframe's upload half, or a producer's own lists, gfbe_kfd_add_keyframe). `sg` is the database's staging,
// opened by the caller and not yet flushed; the keyframe fits (ldb_add_refused).
gfbe_status ldb_add_launch(gfbe_ctx *c, gfbe_ldb *m, const char *who, int n, const uint64_t *dd, const float *dp, const float *dpn, int detect_loop, Staged &sg,
                           int32_t *index_out, int32_t *loop_index, int32_t *n_results, int32_t *result_id, double *result_score) {
  hipStream_t st = ctx_stream(c);
  const int frame_index = (int)m->kf_n.size();
  LdbResult hres;
  std::memset(&hres, 0, sizeof hres);
  LdbResult *dres = sg.up((const LdbResult *)nullptr, 1);
  if (!sg.ok) { ctx_set_error(c, (std::string(who) + ": staging allocation failed").c_str()); return GFBE_DEVICE_ERROR; }
  sg.flush();
  ldb_enqueue_transform(c, m, n, dd, nullptr);
  if (detect_loop) {
    // the query sees the database before this keyframe is added (db.query, then db.add: pose_graph.cpp:447-452)
    hipLaunchKernelGGL(k_ldb_query, dim3(std::max(1, std::min(LDB_QUERY_BLOCKS, ldb_grid(frame_index, LDB_THREADS / 64)))), dim3(LDB_THREADS), 0, st, (const int *)m->meta,
                       frame_index - m->opt.query_gap, (const int *)m->q_word, (const double *)m->q_val, (const long long *)m->ent, (const int *)m->bow_word,
                       (const double *)m->bow_val, m->raw, m->has);
    hipLaunchKernelGGL(k_ldb_select, dim3(1), dim3(LDB_BOW_THREADS), 0, st, (const int *)m->meta, (const double *)m->raw, (const int *)m->has,
                       LdbDecide{m->opt.max_results, m->opt.min_loop_frame, m->opt.score_first, m->opt.score_other}, dres);
    sg.down(&hres, (const LdbResult *)dres, 1);
  }
  if (n > 0)
    hipLaunchKernelGGL(k_ldb_store, dim3(ldb_grid(n, LDB_THREADS)), dim3(LDB_THREADS), 0, st, (const int *)m->meta, (int)n, dd, dp, dpn, (const int *)m->q_word,
                       (const double *)m->q_val, m->desc, m->pts, m->ptsn, m->bow_word, m->bow_val);
  hipLaunchKernelGGL(k_ldb_commit, dim3(1), dim3(1), 0, st, m->meta, (int)n, m->ent);
  sg.finish();      // detecting: the one wait, for the results; otherwise the slot's event
  m->kf_begin.push_back(m->n_desc); m->kf_n.push_back(n); m->n_desc += n;
  GFBE_CHECK(c, hipGetLastError());
  if (index_out) *index_out = frame_index;
  if (detect_loop) {
    if (loop_index) *loop_index = hres.loop_index;
    if (n_results) *n_results = hres.n_results;
    for (int a = 0; a < hres.n_results; a++) { if (result_id) result_id[a] = hres.id[a]; if (result_score) result_score[a] = hres.score[a]; }
  }
  return GFBE_OK;
}

// The launch half of a match: rule 6 of n_window descriptors on the device (dw [n_window][4]) against held keyframe old_index; `sg` as above.
gfbe_status ldb_match_launch(gfbe_ctx *c, gfbe_ldb *m, const char *who, int old_index, int n_window, const uint64_t *dw, Staged &sg, uint8_t *status, int32_t *best_index,
                             int32_t *best_dist, int32_t *n_matched, int32_t *matched_src, float *matched_pt, float *matched_pt_norm) {
  const size_t W = (size_t)n_window;
  int hn = 0;
  int *d_bi = sg.up((const int *)nullptr, W), *d_bd = sg.up((const int *)nullptr, W), *d_flag = sg.up((const int *)nullptr, W), *d_src = sg.up((const int *)nullptr, W);
  int *d_n = sg.up((const int *)nullptr, 1);
  uint8_t *d_st = sg.up((const uint8_t *)nullptr, W);
  float *d_pt = sg.up((const float *)nullptr, 2 * W), *d_ptn = sg.up((const float *)nullptr, 2 * W);
  if (!sg.ok) { ctx_set_error(c, (std::string(who) + ": staging allocation failed").c_str()); return GFBE_DEVICE_ERROR; }
  sg.flush();
  ldb_match_enqueue(c, m, old_index, n_window, dw, d_bi, d_bd, d_flag, d_st, d_n, d_src, d_pt, d_ptn);
  // the compacted outputs are copied whole (n_window rows): only the first n_matched are defined, the rest the caller never reads
  std::vector<int32_t> src_h(matched_src ? W : 0);
  std::vector<float> pt_h(matched_pt ? 2 * W : 0), ptn_h(matched_pt_norm ? 2 * W : 0);
  sg.down(&hn, (const int *)d_n, 1);
  sg.down(status, (const uint8_t *)d_st, W);
  sg.down(best_index, (const int32_t *)d_bi, W);
  sg.down(best_dist, (const int32_t *)d_bd, W);
  sg.down(src_h.data(), (const int32_t *)d_src, src_h.size());
  sg.down(pt_h.data(), (const float *)d_pt, pt_h.size());
  sg.down(ptn_h.data(), (const float *)d_ptn, ptn_h.size());
  sg.finish();      // the one wait
  if (matched_src) std::memcpy(matched_src, src_h.data(), sizeof(int32_t) * (size_t)hn);
  if (matched_pt) std::memcpy(matched_pt, pt_h.data(), sizeof(float) * 2 * (size_t)hn);
  if (matched_pt_norm) std::memcpy(matched_pt_norm, ptn_h.data(), sizeof(float) * 2 * (size_t)hn);
  GFBE_CHECK(c, hipGetLastError());
  if (n_matched) *n_matched = hn;
  return GFBE_OK;
}

}  // namespace

// ---- what gfbe_kfd.hip (include/gfbe_kfd.h) sees of the database: the two calls on lists that lie on the device (gfbe_device.h)
namespace gfd {
gfbe_status ldb_add_keyframe_device(gfbe_ctx *c, gfbe_ldb *m, const char *who, int n, const uint64_t *dd, const float *dp, const float *dpn, int detect_loop, int32_t *index_out,
                                    int32_t *loop_index, int32_t *n_results, int32_t *result_id, double *result_score) {
  gfbe_status rc = handle_ready(c, m, who, "loop database");
  if (rc != GFBE_OK) return rc;
  if (n < 0 || n > m->opt.max_keyframe_descriptors) return handle_bad(c, who, "n outside 0 .. max_keyframe_descriptors of the loop database");
  if (ldb_add_refused(c, m, n, index_out, loop_index, n_results, &rc)) return rc;
  Staged sg(c, m, 4096, /*defer=*/!detect_loop);
  return ldb_add_launch(c, m, who, n, dd, dp, dpn, detect_loop, sg, index_out, loop_index, n_results, result_id, result_score);
}
gfbe_status ldb_match_device(gfbe_ctx *c, gfbe_ldb *m, const char *who, int old_index, int n_window, const uint64_t *dw, uint8_t *status, int32_t *best_index, int32_t *best_dist,
                             int32_t *n_matched, int32_t *matched_src, float *matched_pt, float *matched_pt_norm) {
  const gfbe_status rc = ldb_match_check(c, m, who, old_index, n_window);
  if (rc != GFBE_OK) return rc;
  Staged sg(c, m, (size_t)n_window * 40 + 8192);
  return ldb_match_launch(c, m, who, old_index, n_window, dw, sg, status, best_index, best_dist, n_matched, matched_src, matched_pt, matched_pt_norm);
}
// ---- ... and gfbe_pnp.hip (include/gfbe_pnp.h): the checks of a match, and rule 6 + reduceVector enqueued on the context's stream into
// device buffers of n_window rows (at least one); nobody waits here
gfbe_status ldb_match_check(gfbe_ctx *c, gfbe_ldb *m, const char *who, int old_index, int n_window) {
  gfbe_status rc = handle_ready(c, m, who, "loop database");
  if (rc != GFBE_OK) return rc;
  if (old_index < 0 || old_index >= (int)m->kf_n.size()) return handle_bad(c, who, "old_index is not a held keyframe");
  if (n_window < 0 || n_window > LDB_MAX_WINDOW) return handle_bad(c, who, "n_window outside 0 .. 2^20");
  return GFBE_OK;
}
void ldb_match_enqueue(gfbe_ctx *c, gfbe_ldb *m, int old_index, int n_window, const uint64_t *dw, int *d_bi, int *d_bd, int *d_flag, uint8_t *d_st, int *d_n, int *d_src,
                       float *d_pt, float *d_ptn) {
  hipStream_t st = ctx_stream(c);
  const long long ob = m->kf_begin[(size_t)old_index];
  if (n_window > 0)
    hipLaunchKernelGGL(k_ldb_match, dim3(ldb_grid(n_window, LDB_THREADS / 64)), dim3(LDB_THREADS), 0, st, (int)n_window, dw, ob, m->kf_n[(size_t)old_index],
                       (const uint64_t *)m->desc, (int)m->opt.match_start, (int)m->opt.match_max, d_bi, d_bd, d_flag, d_st);
  hipLaunchKernelGGL(k_ldb_compact, dim3(1), dim3(LDB_BOW_THREADS), 0, st, (int)n_window, (const int *)d_flag, (const int *)d_bi, ob, (const float *)m->pts,
                     (const float *)m->ptsn, d_n, d_src, d_pt, d_ptn);
}
}  // namespace gfd

extern "C" {

void gfbe_ldb_default_options(gfbe_ldb_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = (int32_t)sizeof *o;
  o->max_results = 4; o->query_gap = 50; o->min_loop_frame = 50;
  o->max_keyframe_descriptors = LDB_MAX_KF_DESC;
  o->match_start = 128; o->match_max = 80;
  o->score_first = 0.05; o->score_other = 0.015;
}

void gfbe_ldb_destroy(gfbe_ctx *c, gfbe_ldb *m) {
  if (!m) return;
  m->release(c);
  delete m;
}

gfbe_status gfbe_ldb_create(gfbe_ctx *c, const gfbe_ldb_vocab *voc, int32_t keyframe_capacity, int64_t descriptor_capacity, const gfbe_ldb_options *opt, gfbe_ldb **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  gfbe_ldb_options o;
  if (opt) o = *opt; else gfbe_ldb_default_options(&o);
  if (const char *bad = ldb_options_error(&o)) { ctx_set_error(c, (std::string("gfbe_ldb_create: ") + bad).c_str()); return GFBE_BAD_INPUT; }
  if (!voc) { ctx_set_error(c, "gfbe_ldb_create: no vocabulary"); return GFBE_BAD_INPUT; }
  if (keyframe_capacity < 1 || keyframe_capacity > (1 << 24) || descriptor_capacity < 1 || descriptor_capacity > (1ll << 26)) {
    ctx_set_error(c, "gfbe_ldb_create: keyframe_capacity outside 1 .. 2^24 or descriptor_capacity outside 1 .. 2^26");
    return GFBE_BAD_INPUT;
  }
  LdbTree T;
  const LdbVocabIn vin{voc->k, voc->L, voc->scoring, voc->weighting, voc->n_nodes, voc->node_id, voc->parent_id, voc->weight, voc->descriptor, voc->n_words, voc->word_id, voc->word_node};
  if (const int bad = ldb_plan_vocab(vin, ctx_device(c) < 0 ? nullptr : &T)) { ctx_set_error(c, (std::string("gfbe_ldb_create: vocabulary: ") + ldb_vocab_error(bad)).c_str()); return GFBE_BAD_INPUT; }
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_ldb_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  gfbe_ldb *m = new gfbe_ldb();
  CreateGuard<gfbe_ldb> guard{c, m, gfbe_ldb_destroy};
  m->owner = c; m->opt = o; m->kcap = keyframe_capacity; m->dcap = descriptor_capacity;
  const size_t N = (size_t)voc->n_nodes + 1, K = (size_t)keyframe_capacity, D = (size_t)descriptor_capacity, Q = (size_t)o.max_keyframe_descriptors;
  hipStream_t st = ctx_stream(c);
  bool ok = m->alloc(&m->t_desc, 4 * N) && m->alloc(&m->t_child_begin, N) && m->alloc(&m->t_child_count, N) && m->alloc(&m->t_child, N) && m->alloc(&m->t_word, N) &&
            m->alloc(&m->t_word_weight, (size_t)T.n_words) && m->alloc(&m->bow_word, D) && m->alloc(&m->bow_val, D) && m->alloc(&m->desc, 4 * D) && m->alloc(&m->pts, 2 * D) &&
            m->alloc(&m->ptsn, 2 * D) && m->alloc(&m->ent, 4 * K) && m->alloc(&m->word_of, Q) && m->alloc(&m->q_word, Q) && m->alloc(&m->q_val, Q) && m->alloc(&m->raw, K) && m->alloc(&m->has, K) &&
            m->alloc(&m->meta, (size_t)LM_META);
  if (!ok) { ctx_set_error(c, "gfbe_ldb_create: device allocation failed"); return GFBE_DEVICE_ERROR; }
  std::vector<double> word_weight((size_t)T.n_words, 0.0);
  for (size_t id = 1; id < N; id++) if (T.word[id] >= 0) word_weight[(size_t)T.word[id]] = T.weight[id];
  GFBE_CHECK(c, hipMemcpyAsync(m->t_desc, T.desc.data(), sizeof(uint64_t) * 4 * N, hipMemcpyHostToDevice, st));
  GFBE_CHECK(c, hipMemcpyAsync(m->t_child_begin, T.child_begin.data(), sizeof(int) * N, hipMemcpyHostToDevice, st));
  GFBE_CHECK(c, hipMemcpyAsync(m->t_child_count, T.child_count.data(), sizeof(int) * N, hipMemcpyHostToDevice, st));
  GFBE_CHECK(c, hipMemcpyAsync(m->t_child, T.child.data(), sizeof(int) * (N - 1), hipMemcpyHostToDevice, st));
  GFBE_CHECK(c, hipMemcpyAsync(m->t_word, T.word.data(), sizeof(int) * N, hipMemcpyHostToDevice, st));
  GFBE_CHECK(c, hipMemcpyAsync(m->t_word_weight, word_weight.data(), sizeof(double) * (size_t)T.n_words, hipMemcpyHostToDevice, st));
  if (!m->make_staging(c, "gfbe_ldb_create", 1 << 16, true)) return GFBE_DEVICE_ERROR;
  GFBE_CHECK(c, hipStreamSynchronize(st));      // (the host vectors of the tree leave scope)
  guard.armed = false;
  *out = m;
  return GFBE_OK;
}

gfbe_status gfbe_ldb_transform(gfbe_ctx *c, gfbe_ldb *m, int32_t n, const uint64_t *desc, int32_t *word_out, int32_t *n_bow, int32_t *bow_word, double *bow_value) {
  gfbe_status rc = handle_ready(c, m, "gfbe_ldb_transform");
  if (rc != GFBE_OK) return rc;
  if (n < 0 || n > m->opt.max_keyframe_descriptors || (n > 0 && !desc)) { ctx_set_error(c, "gfbe_ldb_transform: n outside 0 .. max_keyframe_descriptors or desc NULL"); return GFBE_BAD_INPUT; }
  const size_t N = (size_t)n;
  LdbResult hres;
  std::memset(&hres, 0, sizeof hres);
  {
    Staged sg(c, m, N * 32 + 4096);
    const uint64_t *dd = sg.up(desc, 4 * N);
    LdbResult *dres = sg.up((const LdbResult *)nullptr, 1);
    if (!sg.ok) { ctx_set_error(c, "gfbe_ldb_transform: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    ldb_enqueue_transform(c, m, n, dd, dres);
    sg.down(&hres, (const LdbResult *)dres, 1);
    sg.down(word_out, (const int32_t *)m->word_of, N);
    sg.finish();
  }
  GFBE_CHECK(c, hipGetLastError());
  if (n_bow) *n_bow = hres.n_bow;
  hipStream_t st = ctx_stream(c);
  if (hres.n_bow > 0 && bow_word) GFBE_CHECK(c, hipMemcpyAsync(bow_word, m->q_word, sizeof(int) * (size_t)hres.n_bow, hipMemcpyDeviceToHost, st));
  if (hres.n_bow > 0 && bow_value) GFBE_CHECK(c, hipMemcpyAsync(bow_value, m->q_val, sizeof(double) * (size_t)hres.n_bow, hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  return GFBE_OK;
}

gfbe_status gfbe_ldb_add_keyframe(gfbe_ctx *c, gfbe_ldb *m, int32_t n, const uint64_t *desc, const float *pts, const float *pts_norm, int32_t detect_loop, int32_t *index_out,
                                  int32_t *loop_index, int32_t *n_results, int32_t *result_id, double *result_score) {
  gfbe_status rc = handle_ready(c, m, "gfbe_ldb_add_keyframe");
  if (rc != GFBE_OK) return rc;
  if (n < 0 || n > m->opt.max_keyframe_descriptors || (n > 0 && (!desc || !pts || !pts_norm))) {
    ctx_set_error(c, "gfbe_ldb_add_keyframe: n outside 0 .. max_keyframe_descriptors or a NULL input array");
    return GFBE_BAD_INPUT;
  }
  if (ldb_add_refused(c, m, n, index_out, loop_index, n_results, &rc)) return rc;
  // the upload half: the keyframe goes into the staging chunk (detecting) or a slot of the ring
  const size_t N = (size_t)n;
  Staged sg(c, m, N * 48 + 4096, /*defer=*/!detect_loop);
  const uint64_t *dd = sg.up(desc, 4 * N);
  const float *dp = sg.up(pts, 2 * N), *dpn = sg.up(pts_norm, 2 * N);
  return ldb_add_launch(c, m, "gfbe_ldb_add_keyframe", n, dd, dp, dpn, detect_loop, sg, index_out, loop_index, n_results, result_id, result_score);
}

gfbe_status gfbe_ldb_match(gfbe_ctx *c, gfbe_ldb *m, int32_t old_index, int32_t n_window, const uint64_t *window_desc, uint8_t *status, int32_t *best_index, int32_t *best_dist,
                           int32_t *n_matched, int32_t *matched_src, float *matched_pt, float *matched_pt_norm) {
  gfbe_status rc = handle_ready(c, m, "gfbe_ldb_match");
  if (rc != GFBE_OK) return rc;
  if (old_index < 0 || old_index >= (int)m->kf_n.size()) { ctx_set_error(c, "gfbe_ldb_match: old_index is not a held keyframe"); return GFBE_BAD_INPUT; }
  if (n_window < 0 || n_window > LDB_MAX_WINDOW || (n_window > 0 && !window_desc)) { ctx_set_error(c, "gfbe_ldb_match: n_window outside 0 .. 2^20 or window_desc NULL"); return GFBE_BAD_INPUT; }
  const size_t W = (size_t)n_window;
  Staged sg(c, m, W * 72 + 8192);
  const uint64_t *dw = sg.up(window_desc, 4 * W);
  return ldb_match_launch(c, m, "gfbe_ldb_match", old_index, n_window, dw, sg, status, best_index, best_dist, n_matched, matched_src, matched_pt, matched_pt_norm);
}

gfbe_status gfbe_ldb_size(gfbe_ctx *c, gfbe_ldb *m, int32_t *counts) {
  gfbe_status rc = handle_ready(c, m, "gfbe_ldb_size");
  if (rc != GFBE_OK) return rc;
  int h[LM_META];
  GFBE_CHECK(c, hipMemcpyAsync(h, m->meta, sizeof h, hipMemcpyDeviceToHost, ctx_stream(c)));
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  if (counts) for (int a = 0; a < GFBE_LDB_N_COUNTS; a++) counts[a] = h[a];
  return GFBE_OK;
}

gfbe_status gfbe_ldb_download_entry(gfbe_ctx *c, gfbe_ldb *m, int32_t e, int32_t *n_bow, int32_t *bow_word, double *bow_value, int32_t *n_desc, uint64_t *desc, float *pts,
                                    float *pts_norm) {
  gfbe_status rc = handle_ready(c, m, "gfbe_ldb_download_entry");
  if (rc != GFBE_OK) return rc;
  if (e < 0 || e >= (int)m->kf_n.size()) { ctx_set_error(c, "gfbe_ldb_download_entry: no such entry"); return GFBE_BAD_INPUT; }
  hipStream_t st = ctx_stream(c);
  long long row[4];
  GFBE_CHECK(c, hipMemcpyAsync(row, m->ent + 4 * (size_t)e, sizeof row, hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  const size_t nb = (size_t)row[1], nd = (size_t)row[3];
  if (n_bow) *n_bow = (int32_t)nb;
  if (n_desc) *n_desc = (int32_t)nd;
  if (nb && bow_word) GFBE_CHECK(c, hipMemcpyAsync(bow_word, m->bow_word + row[0], sizeof(int) * nb, hipMemcpyDeviceToHost, st));
  if (nb && bow_value) GFBE_CHECK(c, hipMemcpyAsync(bow_value, m->bow_val + row[0], sizeof(double) * nb, hipMemcpyDeviceToHost, st));
  if (nd && desc) GFBE_CHECK(c, hipMemcpyAsync(desc, m->desc + 4 * row[2], sizeof(uint64_t) * 4 * nd, hipMemcpyDeviceToHost, st));
  if (nd && pts) GFBE_CHECK(c, hipMemcpyAsync(pts, m->pts + 2 * row[2], sizeof(float) * 2 * nd, hipMemcpyDeviceToHost, st));
  if (nd && pts_norm) GFBE_CHECK(c, hipMemcpyAsync(pts_norm, m->ptsn + 2 * row[2], sizeof(float) * 2 * nd, hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  return GFBE_OK;
}

}  // extern "C"
