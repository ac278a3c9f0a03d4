// gfbe_pnp.hip — the loop verification of the loop-closure thread on the device: P3P RANSAC on the matched pairs of a loop candidate, the
// refit on the inliers, loop_info and its acceptance test, for a batch of problems; and findConnection's chain from the window descriptors
// to the decision behind one host wait.
//
//   KeyFrame::PnPRANSAC (cv::solvePnPRansac)           dense_map/src/keyframe.cpp:273-329                   k_pnp_hyp, k_pnp_score, k_pnp_finish
//   findConnection's loop_info and test                :479-565                                             k_pnp_finish, pnp_decide on the host
//   searchByBRIEFDes + reduceVector + the gather       :194-244, 374-380, 497-510                           gfd::ldb_match_enqueue, k_pnp_gather
//
// The rules are in gfbe_pnp.h and include/gfbe_pnp.h; every statement is the header's function, compiled here for the device.
// k_pnp_hyp: one lane per (problem, hypothesis) draws the sample (V2) and solves the P3P (V3); branchy scalar FP64, everything in
// registers. k_pnp_score: a workgroup of four waves per four hypotheses of a problem; the problem's points pass through LDS in tiles of
// 512 as double; a wave owns a hypothesis with its up to four poses, its lanes stride the tile, counts are ballots and popcounts (V4).
// k_pnp_finish: one wave per problem; the packed-key maximum over the counts by shuffles (V5), the winner's mask and its inlier list in
// LDS by ballots, the lane-strided sums and the butterfly of V6 with every lane solving the same 6 x 6 system, V7 without its atan2.
// k_pnp_gather: the window's points by matched_src and the problem's offsets from the match count on the device. Integers only in
// every count, no atomics, no scratch; no result depends on the order workgroups ran in or on what an allocation held before.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gfbe_pnp.h"
#include "gfbe_device.h"
#include "gfbe_pnp.h"
#include "gfbe_handle.h"

using namespace gfd;

static_assert(sizeof(gfbe_pnp_options) == 56, "the layout of include/gfbe_pnp.h");

struct gfbe_pnp : gfbe_handle {
  gfbe_pnp_options opt;
  // one call's scratch: [max_problems][iterations] rows
  int *sample = nullptr, *nsol = nullptr, *hcount = nullptr;      // [.][3], [.], [.][4]
  double *hpose = nullptr;                                        // [.][4][12]
};

namespace {
constexpr int PNP_TILE = 512, PNP_SCORE_THREADS = 256;
constexpr int PI_NINL = 0, PI_H = 1, PI_S = 2, PI_FLAG = 3;      // ires [B][4]

struct PnpDev {
  const int *off;                          // [B + 1], on the device
  const float *p3, *pn;                    // [n][3], [n][2]
  const double *pose_cur, *tic_qic;        // [B][12]
  int *sample, *nsol, *hcount;
  double *hpose;
  uint8_t *status;                         // [n]
  double *res;                             // [B][PNP_RES]
  int *ires;                               // [B][4]
  PnpParams P;
};

// ---- V2, V3 -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pnp_hyp(PnpDev A) {
  const int b = blockIdx.y, h = blockIdx.x * 64 + threadIdx.x;
  if (h >= A.P.iterations) return;
  const int o = A.off[b], n = A.off[b + 1] - o;
  const size_t row = (size_t)b * (size_t)A.P.iterations + (size_t)h;
  double *sol = A.hpose + 48 * row;
  int idx[3] = {-1, -1, -1}, ns = 0;
  if (n > A.P.min_loop_num && pnp_sample(A.P.seed, h, n, idx) == 3) {
    double X[9], uv[6];
#pragma unroll
    for (int m = 0; m < 3; m++) {
      const size_t p = (size_t)o + (size_t)idx[m];
#pragma unroll
      for (int a = 0; a < 3; a++) X[3 * m + a] = (double)A.p3[3 * p + a];
#pragma unroll
      for (int a = 0; a < 2; a++) uv[2 * m + a] = (double)A.pn[2 * p + a];
    }
    ns = pnp_p3p(X, uv, sol);
  }
  for (int a = 12 * ns; a < 48; a++) sol[a] = 0.0;
  A.sample[3 * row] = idx[0]; A.sample[3 * row + 1] = idx[1]; A.sample[3 * row + 2] = idx[2];
  A.nsol[row] = ns;
}

// ---- V4 ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNP_SCORE_THREADS) void k_pnp_score(PnpDev A) {
  __shared__ double s_pt[5][PNP_TILE];
  const int b = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int h = __builtin_amdgcn_readfirstlane(blockIdx.x * (PNP_SCORE_THREADS / 64) + (t >> 6));
  const int o = A.off[b], n = A.off[b + 1] - o;
  const bool mine = h < A.P.iterations;
  const size_t row = (size_t)b * (size_t)A.P.iterations + (size_t)(mine ? h : 0);
  const int ns = mine && n > A.P.min_loop_num ? A.nsol[row] : 0;
  const double *sol = A.hpose + 48 * row;
  int count[4] = {0, 0, 0, 0};
  const int n_run = n > A.P.min_loop_num ? n : 0;      // (uniform over the workgroup)
  for (int i0 = 0; i0 < n_run; i0 += PNP_TILE) {
    __syncthreads();
    for (int e = t; e < PNP_TILE; e += PNP_SCORE_THREADS) {
      const int i = i0 + e;
      if (i < n) {
        const size_t p = (size_t)o + (size_t)i;
        s_pt[0][e] = (double)A.p3[3 * p]; s_pt[1][e] = (double)A.p3[3 * p + 1]; s_pt[2][e] = (double)A.p3[3 * p + 2];
        s_pt[3][e] = (double)A.pn[2 * p]; s_pt[4][e] = (double)A.pn[2 * p + 1];
      }
    }
    __syncthreads();
    const int m = min(PNP_TILE, n - i0);
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if (s >= ns) continue;      // (wave-uniform)
      double pose[12];
#pragma unroll
      for (int a = 0; a < 12; a++) pose[a] = sol[12 * s + a];
      for (int e0 = 0; e0 < m; e0 += 64) {
        const int e = e0 + lane;
        const bool in = e < m && pnp_inlier(pose, s_pt[0][e < m ? e : 0], s_pt[1][e < m ? e : 0], s_pt[2][e < m ? e : 0], s_pt[3][e < m ? e : 0], s_pt[4][e < m ? e : 0], A.P.thr2);
        count[s] += __popcll(__ballot(in));
      }
    }
  }
  if (mine && lane == 0) {
#pragma unroll
    for (int s = 0; s < 4; s++) A.hcount[4 * row + s] = s < ns ? count[s] : 0;
  }
}

// ---- V5, V6, V7 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pnp_finish(PnpDev A) {
  __shared__ int s_list[PNP_MAX_POINTS];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int o = A.off[b], n = A.off[b + 1] - o, H = A.P.iterations;
  const size_t row0 = (size_t)b * (size_t)H;
  unsigned long long key = 0;
  if (n > A.P.min_loop_num)
    for (int e = lane; e < 4 * H; e += 64) {
      const int h = e >> 2, s = e & 3;
      if (s < A.nsol[row0 + h]) { const unsigned long long k = pnp_key(A.hcount[4 * (row0 + h) + s], h, s); key = k > key ? k : key; }
    }
#pragma unroll
  for (int f = 32; f >= 1; f >>= 1) { const unsigned long long k = (unsigned long long)__shfl_xor((long long)key, f, 64); key = k > key ? k : key; }
  double *res = A.res + (size_t)PNP_RES * (size_t)b;
  int *ires = A.ires + 4 * (size_t)b;
  if (key == 0) {      // V1 without PnP, or no solution anywhere (wave-uniform)
    for (int i = lane; i < n; i += 64) A.status[(size_t)o + i] = 0;
    if (lane < PNP_RES) res[lane] = 0.0;
    if (lane == 0) { ires[PI_NINL] = 0; ires[PI_H] = -1; ires[PI_S] = -1; ires[PI_FLAG] = 0; }
    return;
  }
  const int slot = pnp_key_slot(key), cnt = pnp_key_count(key);
  double pose[12];
#pragma unroll
  for (int a = 0; a < 12; a++) pose[a] = A.hpose[48 * (row0 + (size_t)(slot >> 2)) + 12 * (size_t)(slot & 3) + a];
  // the winner's mask, and its inliers in ascending point index
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    bool in = false;
    if (i < n) {
      const size_t p = (size_t)o + (size_t)i;
      in = pnp_inlier(pose, (double)A.p3[3 * p], (double)A.p3[3 * p + 1], (double)A.p3[3 * p + 2], (double)A.pn[2 * p], (double)A.pn[2 * p + 1], A.P.thr2);
      A.status[p] = in ? 1 : 0;
    }
    const unsigned long long m = __ballot(in);
    if (in) s_list[base + __popcll(m & ((1ull << lane) - 1ull))] = i;
    base += __popcll(m);
  }
  __syncthreads();
  double q[4];
  pnp_rot_to_quat(pose + 3, q);
  int flag = 0;
  for (int it = 0; it < A.P.refine_iterations; it++) {
    double acc[27];
#pragma unroll
    for (int e = 0; e < 27; e++) acc[e] = 0.0;
    for (int r = lane; r < base; r += 64) {
      const size_t p = (size_t)o + (size_t)s_list[r];
      pnp_accumulate(pose, (double)A.p3[3 * p], (double)A.p3[3 * p + 1], (double)A.p3[3 * p + 2], (double)A.pn[2 * p], (double)A.pn[2 * p + 1], acc);
    }
#pragma unroll
    for (int f = 32; f >= 1; f >>= 1) {
#pragma unroll
      for (int e = 0; e < 27; e++) acc[e] = acc[e] + __shfl_xor(acc[e], f, 64);
    }
    double d[6];
    if (!pnp_solve6(acc, d)) { flag = 1; break; }      // (every lane holds the same sums: wave-uniform)
    pnp_update(d, q, pose);
  }
  if (lane == 0) {
    pnp_relative(pose, A.pose_cur + 12 * (size_t)b, A.tic_qic + 12 * (size_t)b, res);
    ires[PI_NINL] = cnt; ires[PI_H] = slot >> 2; ires[PI_S] = slot & 3; ires[PI_FLAG] = flag;
  }
}

// ---- findConnection's gather: point_3d of the window by matched_src, and the one problem's offsets from the count on the device ------------
__global__ __launch_bounds__(256) void k_pnp_gather(int n_window, const int *n_matched, const int *matched_src, const float *p3_window, float *p3, int *off) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = min(max(*n_matched, 0), n_window);
  if (i == 0) { off[0] = 0; off[1] = n; }
  if (i >= n) return;
  const int s = matched_src[i];
  if (s < 0 || s >= n_window) { p3[3 * (size_t)i] = p3[3 * (size_t)i + 1] = p3[3 * (size_t)i + 2] = 0.f; return; }      // (cannot happen: reduceVector lists window rows)
  for (int a = 0; a < 3; a++) p3[3 * (size_t)i + a] = p3_window[3 * (size_t)s + a];
}

const char *pnp_options_error(const gfbe_pnp_options *o) {
  if (o->struct_size != (int32_t)sizeof(gfbe_pnp_options)) return "gfbe_pnp_options.struct_size does not match this library (ABI mismatch)";
  if (o->max_problems < 1 || o->max_problems > 4096) return "max_problems outside 1 .. 4096";
  if (o->max_points < 1 || o->max_points > PNP_MAX_POINTS) return "max_points outside 1 .. 4096";
  if (o->iterations < 1 || o->iterations > PNP_MAX_ITER) return "iterations outside 1 .. 1024";
  if (o->refine_iterations < 0 || o->refine_iterations > PNP_MAX_REFINE) return "refine_iterations outside 0 .. 20";
  if (o->min_loop_num < 0) return "min_loop_num < 0";
  if (!std::isfinite(o->reproj_threshold) || !(o->reproj_threshold > 0.0)) return "reproj_threshold must be finite and > 0";
  if (!std::isfinite(o->max_yaw_deg) || !std::isfinite(o->max_translation)) return "max_yaw_deg / max_translation must be finite";
  return nullptr;
}
PnpParams pnp_params(const gfbe_pnp_options &o) {
  PnpParams P;
  P.iterations = o.iterations; P.refine_iterations = o.refine_iterations; P.min_loop_num = o.min_loop_num; P.pad = 0; P.seed = o.seed;
  P.thr2 = o.reproj_threshold * o.reproj_threshold;
  return P;
}
int pnp_grid(long long n, int per) { return (int)std::max<long long>(1, (n + per - 1) / per); }
// V2 .. V7 of B problems whose arguments lie on the device
void pnp_enqueue(gfbe_ctx *c, const PnpDev &A, int B) {
  hipStream_t st = ctx_stream(c);
  hipLaunchKernelGGL(k_pnp_hyp, dim3(pnp_grid(A.P.iterations, 64), B), dim3(64), 0, st, A);
  hipLaunchKernelGGL(k_pnp_score, dim3(pnp_grid(A.P.iterations, PNP_SCORE_THREADS / 64), B), dim3(PNP_SCORE_THREADS), 0, st, A);
  hipLaunchKernelGGL(k_pnp_finish, dim3(B), dim3(64), 0, st, A);
}
// V7's yaw and V8 of problem b from what came back
void pnp_finish_host(const gfbe_pnp_options &o, size_t b, const double *res, const int *ires, const double *pose_cur, int32_t *n_inliers, int32_t *has_loop, double *loop_info,
                     double *pnp_pose, int32_t *best, int32_t *refine_flag) {
  double info[8];
  const int has = pnp_decide(res, pose_cur, ires[PI_NINL], o.min_loop_num, o.max_yaw_deg, o.max_translation, info);      // (no winner: 0 inliers, zeros)
  if (n_inliers) n_inliers[b] = ires[PI_NINL];
  if (has_loop) has_loop[b] = has;
  if (loop_info) std::memcpy(loop_info + 8 * b, info, sizeof info);
  if (pnp_pose) std::memcpy(pnp_pose + 12 * b, res + 7, sizeof(double) * 12);
  if (best) { best[2 * b] = ires[PI_H]; best[2 * b + 1] = ires[PI_S]; }
  if (refine_flag) refine_flag[b] = ires[PI_FLAG];
}

// the chain of findConnection on n_window window descriptors that lie on the device (dw); `sg` is the handle's staging, opened by the
// caller with dw's upload in it (or nothing) and not yet flushed
gfbe_status pnp_connect(gfbe_ctx *c, gfbe_pnp *m, const char *who, Staged &sg, gfbe_ldb *db, int old_index, int n_window, const uint64_t *dw, const float *point_3d,
                        const double *pose_cur, const double *tic_qic, int32_t *n_matched, int32_t *matched_src, float *matched_pt, float *matched_pt_norm, uint8_t *status_pnp,
                        int32_t *n_inliers, int32_t *has_loop, double *loop_info, double *pnp_pose, int32_t *best, int32_t *refine_flag) {
  const size_t W = (size_t)n_window;
  const float *d_p3w = sg.up(point_3d, 3 * W);
  const double *d_pc = sg.up(pose_cur, 12), *d_tq = sg.up(tic_qic, 12);
  int *d_bi = sg.up((const int *)nullptr, W), *d_bd = sg.up((const int *)nullptr, W), *d_flag = sg.up((const int *)nullptr, W), *d_src = sg.up((const int *)nullptr, W);
  int *d_n = sg.up((const int *)nullptr, 1), *d_off = sg.up((const int *)nullptr, 2), *d_ires = sg.up((const int *)nullptr, 4);
  uint8_t *d_st = sg.up((const uint8_t *)nullptr, W), *d_stp = sg.up((const uint8_t *)nullptr, W);
  float *d_pt = sg.up((const float *)nullptr, 2 * W), *d_ptn = sg.up((const float *)nullptr, 2 * W), *d_p3 = sg.up((const float *)nullptr, 3 * W);
  double *d_res = sg.up((const double *)nullptr, PNP_RES);
  if (!sg.ok) { ctx_set_error(c, (std::string(who) + ": staging allocation failed").c_str()); return GFBE_DEVICE_ERROR; }
  sg.flush();
  ldb_match_enqueue(c, db, old_index, n_window, dw, d_bi, d_bd, d_flag, d_st, d_n, d_src, d_pt, d_ptn);
  hipLaunchKernelGGL(k_pnp_gather, dim3(pnp_grid(n_window, 256)), dim3(256), 0, ctx_stream(c), n_window, (const int *)d_n, (const int *)d_src, d_p3w, d_p3, d_off);
  PnpDev A;
  std::memset(&A, 0, sizeof A);
  A.off = d_off; A.p3 = d_p3; A.pn = d_ptn; A.pose_cur = d_pc; A.tic_qic = d_tq; A.sample = m->sample; A.nsol = m->nsol; A.hcount = m->hcount; A.hpose = m->hpose;
  A.status = d_stp; A.res = d_res; A.ires = d_ires; A.P = pnp_params(m->opt);
  pnp_enqueue(c, A, 1);
  // the compacted outputs are copied whole (n_window rows): only the first n_matched are defined, the rest the caller never reads
  int hn = 0, ires[4] = {0, -1, -1, 0};
  double res[PNP_RES] = {};
  std::vector<int32_t> src_h(matched_src ? W : 0);
  std::vector<float> pt_h(matched_pt ? 2 * W : 0), ptn_h(matched_pt_norm ? 2 * W : 0);
  std::vector<uint8_t> stp_h(status_pnp ? W : 0);
  sg.down(&hn, (const int *)d_n, 1);
  sg.down(ires, (const int *)d_ires, 4);
  sg.down(res, (const double *)d_res, PNP_RES);
  sg.down(src_h.data(), (const int32_t *)d_src, src_h.size());
  sg.down(pt_h.data(), (const float *)d_pt, pt_h.size());
  sg.down(ptn_h.data(), (const float *)d_ptn, ptn_h.size());
  sg.down(stp_h.data(), (const uint8_t *)d_stp, stp_h.size());
  sg.finish();      // the one wait
  GFBE_CHECK(c, hipGetLastError());
  hn = std::max(0, std::min(hn, n_window));
  if (matched_src) std::memcpy(matched_src, src_h.data(), sizeof(int32_t) * (size_t)hn);
  if (matched_pt) std::memcpy(matched_pt, pt_h.data(), sizeof(float) * 2 * (size_t)hn);
  if (matched_pt_norm) std::memcpy(matched_pt_norm, ptn_h.data(), sizeof(float) * 2 * (size_t)hn);
  if (status_pnp) std::memcpy(status_pnp, stp_h.data(), (size_t)hn);
  if (n_matched) *n_matched = hn;
  pnp_finish_host(m->opt, 0, res, ires, pose_cur, n_inliers, has_loop, loop_info, pnp_pose, best, refine_flag);
  return GFBE_OK;
}
size_t pnp_connect_bytes(int n_window) { return (size_t)n_window * 96 + 20 * 256 + 8192; }      // (90 bytes a window row, 18 blocks rounded to 256)

}  // namespace

extern "C" {

void gfbe_pnp_default_options(gfbe_pnp_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = (int32_t)sizeof *o;
  o->max_problems = 64; o->max_points = 4096; o->iterations = 100; o->refine_iterations = 5; o->min_loop_num = 25; o->seed = 0;
  o->reproj_threshold = 10.0 / 460.0; o->max_yaw_deg = 30.0; o->max_translation = 20.0;
}

void gfbe_pnp_destroy(gfbe_ctx *c, gfbe_pnp *m) {
  if (!m) return;
  m->release(c);
  delete m;
}

gfbe_status gfbe_pnp_create(gfbe_ctx *c, const gfbe_pnp_options *opt, gfbe_pnp **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  gfbe_pnp_options o;
  if (opt) o = *opt; else gfbe_pnp_default_options(&o);
  if (const char *bad = pnp_options_error(&o)) return handle_bad(c, "gfbe_pnp_create", bad);
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_pnp_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  gfbe_pnp *m = new gfbe_pnp();
  CreateGuard<gfbe_pnp> guard{c, m, gfbe_pnp_destroy};
  m->owner = c; m->opt = o;
  const size_t rows = (size_t)o.max_problems * (size_t)o.iterations;
  if (!(m->alloc(&m->sample, 3 * rows) && m->alloc(&m->nsol, rows) && m->alloc(&m->hcount, 4 * rows) && m->alloc(&m->hpose, 48 * rows))) {
    ctx_set_error(c, "gfbe_pnp_create: device allocation failed");
    return GFBE_DEVICE_ERROR;
  }
  if (!m->make_staging(c, "gfbe_pnp_create", 1 << 18, false)) return GFBE_DEVICE_ERROR;
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  guard.armed = false;
  *out = m;
  return GFBE_OK;
}

gfbe_status gfbe_pnp_verify(gfbe_ctx *c, gfbe_pnp *m, int32_t n_problems, const int32_t *offset, const float *point_3d, const float *pt_norm, const double *pose_cur,
                            const double *tic_qic, uint8_t *status, int32_t *n_inliers, int32_t *has_loop, double *loop_info, double *pnp_pose, int32_t *best, int32_t *refine_flag,
                            int32_t *sample_idx, int32_t *n_solutions, double *hyp_pose, int32_t *hyp_count) {
  const char *who = "gfbe_pnp_verify";
  gfbe_status rc = handle_ready(c, m, who);
  if (rc != GFBE_OK) return rc;
  if (n_problems < 0 || n_problems > m->opt.max_problems) return handle_bad(c, who, "n_problems outside 0 .. max_problems");
  if (n_problems == 0) return GFBE_OK;
  if (!offset || offset[0] != 0) return handle_bad(c, who, "offsets that do not ascend from 0");
  const size_t B = (size_t)n_problems;
  for (size_t b = 0; b < B; b++) {
    if (offset[b + 1] < offset[b]) return handle_bad(c, who, "offsets that do not ascend from 0");
    if (offset[b + 1] - offset[b] > m->opt.max_points) return handle_bad(c, who, "a problem has more points than max_points");
  }
  const size_t n = (size_t)offset[B], H = (size_t)m->opt.iterations;
  if ((n > 0 && (!point_3d || !pt_norm)) || !pose_cur || !tic_qic) return handle_bad(c, who, "point_3d, pt_norm, pose_cur or tic_qic NULL");
  std::vector<double> res(PNP_RES * B);
  std::vector<int> ires(4 * B);
  {
    Staged sg(c, m, n * 21 + B * (4 + 192 + 8 * PNP_RES + 16) + 16 * 256 + 8192);
    PnpDev A;
    std::memset(&A, 0, sizeof A);
    A.off = sg.up((const int *)offset, B + 1); A.p3 = sg.up(point_3d, 3 * n); A.pn = sg.up(pt_norm, 2 * n); A.pose_cur = sg.up(pose_cur, 12 * B); A.tic_qic = sg.up(tic_qic, 12 * B);
    A.status = sg.up((const uint8_t *)nullptr, n); A.res = sg.up((const double *)nullptr, PNP_RES * B); A.ires = sg.up((const int *)nullptr, 4 * B);
    A.sample = m->sample; A.nsol = m->nsol; A.hcount = m->hcount; A.hpose = m->hpose; A.P = pnp_params(m->opt);
    if (!sg.ok) { ctx_set_error(c, "gfbe_pnp_verify: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    pnp_enqueue(c, A, n_problems);
    sg.down(status, (const uint8_t *)A.status, n);
    sg.down(res.data(), (const double *)A.res, PNP_RES * B);
    sg.down(ires.data(), (const int *)A.ires, 4 * B);
    sg.down(sample_idx, (const int32_t *)m->sample, 3 * H * B);
    sg.down(n_solutions, (const int32_t *)m->nsol, H * B);
    sg.down(hyp_pose, (const double *)m->hpose, 48 * H * B);
    sg.down(hyp_count, (const int32_t *)m->hcount, 4 * H * B);
    sg.finish();      // the one wait
    GFBE_CHECK(c, hipGetLastError());
  }
  for (size_t b = 0; b < B; b++)
    pnp_finish_host(m->opt, b, res.data() + PNP_RES * b, ires.data() + 4 * b, pose_cur + 12 * b, n_inliers, has_loop, loop_info, pnp_pose, best, refine_flag);
  return GFBE_OK;
}

gfbe_status gfbe_pnp_find_connection(gfbe_ctx *c, gfbe_pnp *m, gfbe_ldb *db, int32_t old_index, int32_t n_window, const uint64_t *window_desc, const float *point_3d,
                                     const double *pose_cur, const double *tic_qic, int32_t *n_matched, int32_t *matched_src, float *matched_pt, float *matched_pt_norm,
                                     uint8_t *status_pnp, int32_t *n_inliers, int32_t *has_loop, double *loop_info, double *pnp_pose, int32_t *best, int32_t *refine_flag) {
  const char *who = "gfbe_pnp_find_connection";
  gfbe_status rc = handle_ready(c, m, who);
  if (rc != GFBE_OK) return rc;
  if (!db) return handle_bad(c, who, "loop database NULL");
  if ((rc = ldb_match_check(c, db, who, old_index, n_window)) != GFBE_OK) return rc;
  if (n_window > m->opt.max_points) return handle_bad(c, who, "n_window above max_points");
  if ((n_window > 0 && (!window_desc || !point_3d)) || !pose_cur || !tic_qic) return handle_bad(c, who, "window_desc, point_3d, pose_cur or tic_qic NULL");
  Staged sg(c, m, pnp_connect_bytes(n_window));
  const uint64_t *dw = sg.up(window_desc, 4 * (size_t)n_window);
  return pnp_connect(c, m, who, sg, db, old_index, n_window, dw, point_3d, pose_cur, tic_qic, n_matched, matched_src, matched_pt, matched_pt_norm, status_pnp, n_inliers, has_loop,
                     loop_info, pnp_pose, best, refine_flag);
}

gfbe_status gfbe_pnp_find_connection_kfd(gfbe_ctx *c, gfbe_pnp *m, gfbe_kfd *kfd, int32_t camera, gfbe_ldb *db, int32_t old_index, const float *point_3d, const double *pose_cur,
                                         const double *tic_qic, int32_t *n_matched, int32_t *matched_src, float *matched_pt, float *matched_pt_norm, uint8_t *status_pnp,
                                         int32_t *n_inliers, int32_t *has_loop, double *loop_info, double *pnp_pose, int32_t *best, int32_t *refine_flag) {
  const char *who = "gfbe_pnp_find_connection_kfd";
  gfbe_status rc = handle_ready(c, m, who);
  if (rc != GFBE_OK) return rc;
  if (!kfd || !db) return handle_bad(c, who, "describer or loop database NULL");
  int n_window = 0;
  const uint64_t *dw = nullptr;
  if ((rc = kfd_window_desc(c, kfd, who, camera, &n_window, &dw)) != GFBE_OK) return rc;
  if ((rc = ldb_match_check(c, db, who, old_index, n_window)) != GFBE_OK) return rc;
  if (n_window > m->opt.max_points) return handle_bad(c, who, "the camera's window has more points than max_points");
  if ((n_window > 0 && !point_3d) || !pose_cur || !tic_qic) return handle_bad(c, who, "point_3d, pose_cur or tic_qic NULL");
  Staged sg(c, m, pnp_connect_bytes(n_window));
  return pnp_connect(c, m, who, sg, db, old_index, n_window, dw, point_3d, pose_cur, tic_qic, n_matched, matched_src, matched_pt, matched_pt_norm, status_pnp, n_inliers, has_loop,
                     loop_info, pnp_pose, best, refine_flag);
}

}  // extern "C"
