// gfbe_ltab.hip — device-resident line feature tables: the FeatureManager line operations a `use_line` frame runs around
// optimizationwithLine(), one table per window, W tables per launch (the line counterpart of gfbe_ftab.hip).
//
//   addFeatureCheckParallaxwithline (line loop)   estimator/feature_manager.cpp:149-170
//   triangulateLine :1151-1262  (pi_from_ppp / pipi_plk: utility/line_geometry.cpp:115-130)
//   removeBackShiftDepthline (line loop) :1499-1527, removeBackline (line loop) :896-911, removeFrontline (line loop) :958-975
//   getLineFeatureCount :1013-1027
//   onlyLineOpt + removeLineOutlier: k_line_refine<true> (gfbe_line.hip) reading the tables in place, then the erasure below
//
// A table is the reference's std::list<lineFeaturePerId> in insertion order, stored SoA with a fixed row of WINDOW_SIZE + 1
// observation slots [x1 y1 x2 y2] per line, is_triangulation and line_plucker[6] (zeros until triangulated). Erasing keeps the order
// with the scheme of k_ftab_erase: every thread owns a contiguous chunk of the list, a block-wide exclusive scan of the per-chunk
// survivor counts gives each chunk its destination, and the survivors are copied (with their edits) into the other half of a
// ping-pong buffer. Integer / byte work plus a few dozen flops per line: HBM- and latency-bound, no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"
#include "gfbe_line.h"
#include "gfbe_line_batch.h"
#include "gfbe_handle.h"

using namespace gfd;

namespace {

constexpr int NOBS = LT_NOBS;   // observation slots per line
constexpr int OW = 4;           // x1 y1 x2 y2
constexpr int LT_THREADS = 1024;

enum { OP_BACK_SHIFT = 0, OP_BACK = 1, OP_FRONT = 2, OP_REFINE = 3 };

__device__ __forceinline__ mat3 ldm(const double *p) { mat3 R; for (int q = 0; q < 9; q++) R.m[q] = p[q]; return R; }

// ---- erasing operations: decide per line and scan (one workgroup per table), then copy the survivors into the other half (one
//      thread per (line, observation slot), any number of workgroups)
__global__ __launch_bounds__(LT_THREADS) void k_ltab_erase(LtabDev T, int cur, int op, const int *iarg) {
  const int w = blockIdx.x, t = threadIdx.x;
  __shared__ int lds[20];
  const int n = T.count[w];
  const size_t base = (size_t)w * T.F;
  const int *start = T.start[cur] + base, *nobs = T.nobs[cur] + base;
  int *keep = T.keep + base;
  const int chunk = (n + LT_THREADS - 1) / LT_THREADS, f0 = t * chunk, f1 = min(n, f0 + chunk);
  int survivors = 0;
  for (int f = f0; f < f1; f++) {
    // keep[f]: 0 erased; 1 kept, start unchanged; 2 kept, start - 1; 3 + j kept, observation j erased
    int k = 1;
    if (op == OP_BACK_SHIFT || op == OP_BACK) {
      if (start[f] != 0) k = 2;
      else {
        const int left = nobs[f] - 1;
        k = (op == OP_BACK ? left == 0 : left < 2) ? 0 : 3;
      }
    } else if (op == OP_FRONT) {
      const int fc = iarg[w];
      if (start[f] == fc) k = 2;
      else if (start[f] + nobs[f] - 1 < fc - 1) k = 1;
      else k = (nobs[f] - 1 == 0) ? 0 : 3 + (GFBE_WINDOW_SIZE - 1 - start[f]);
    } else {      // OP_REFINE: the keep flags of removeLineOutlier
      k = T.rkeep[base + f] ? 1 : 0;
    }
    keep[f] = k;
    survivors += k != 0;
  }
  int total;
  int dst = block_exclusive_scan<LT_THREADS>(survivors, &total, lds);
  int *dsti = T.dst + base;
  for (int f = f0; f < f1; f++) dsti[f] = keep[f] ? dst++ : -1;
  if (t == 0) { T.cnt_scratch[w] = n; T.count[w] = total; }
}
// argA / argB: marg_PR / new_PR [W][12] of OP_BACK_SHIFT
__global__ __launch_bounds__(256) void k_ltab_erase_copy(LtabDev T, int cur, int op, const double *argA, const double *argB) {
  const int w = blockIdx.y;
  const int n = T.cnt_scratch[w];            // lines before the operation
  const int g = blockIdx.x * 256 + threadIdx.x, f = g / NOBS, q = g - f * NOBS;
  if (f >= n) return;
  const size_t base = (size_t)w * T.F;
  const int k = T.keep[base + f], dst = T.dst[base + f];
  if (k == 0) return;
  const int o = 1 - cur;
  const int drop = k >= 3 ? k - 3 : -1, m = T.nobs[cur][base + f];
  if (q == 0) {
    T.id[o][base + dst] = T.id[cur][base + f]; T.tri[o][base + dst] = T.tri[cur][base + f];
    T.start[o][base + dst] = k == 2 ? T.start[cur][base + f] - 1 : T.start[cur][base + f];
    T.nobs[o][base + dst] = drop >= 0 ? m - 1 : m;
    const double *pin = (op == OP_REFINE ? T.plk_out : T.plk[cur]) + (base + f) * 6;
    double *pout = T.plk[o] + (base + dst) * 6;
    if (op == OP_BACK_SHIFT && k >= 3) {      // plk_to_pose(line_plucker, new_R^T marg_R, new_R^T (marg_P - new_P)), triangulated or not
      const double *mP = argA + 12 * w, *nP = argB + 12 * w;
      const mat3 nR = ldm(nP + 3);
      double moved[6];
      line_plk_to_pose(pin, tmul(nR, ldm(mP + 3)), tmv(nR, sub(ld3(mP), ld3(nP))), moved);
      for (int a = 0; a < 6; a++) pout[a] = moved[a];
    } else {
      for (int a = 0; a < 6; a++) pout[a] = pin[a];
    }
  }
  // output slot q <- source slot q (+ 1 behind the erased observation); slots past the track are zero
  const int sq = (drop >= 0 && q >= drop) ? q + 1 : q;
  const bool live = sq < m && sq < NOBS;
  const double *src = T.obs[cur] + ((base + f) * NOBS + (live ? sq : 0)) * OW;
  double *d4 = T.obs[o] + ((base + dst) * NOBS + q) * OW;
#pragma unroll
  for (int c = 0; c < OW; c++) d4[c] = live ? src[c] : 0.0;
}

// ---- addFeatureCheckParallaxwithline, line loop. find_if over the list for every incoming line: ids are unique inside a table, so
//      at most one list entry matches (the tiling of k_ftab_match)
#define LT_MATCH_TILE 256
__global__ __launch_bounds__(64) void k_ltab_match(LtabDev T, int cur, const int *offset, const int *lid, int *match) {
  const int w = blockIdx.z, j0 = offset[w], m = offset[w + 1] - j0, a = blockIdx.x * 64 + threadIdx.x;
  const int n = T.count[w], f0 = blockIdx.y * LT_MATCH_TILE, nt = min(n - f0, LT_MATCH_TILE);
  if ((int)blockIdx.x * 64 >= m || nt <= 0) return;       // (workgroup-uniform)
  __shared__ int s_id[LT_MATCH_TILE];
  const int *id = T.id[cur] + (size_t)w * T.F + f0;
  for (int f = threadIdx.x; f < nt; f += 64) s_id[f] = id[f];
  __syncthreads();
  if (a >= m) return;
  const int want = lid[j0 + a];
  int hit = -1;
  for (int f = nt - 1; f >= 0; f--) hit = s_id[f] == want ? f : hit;
  if (hit >= 0) match[j0 + a] = f0 + hit;
}
__global__ __launch_bounds__(LT_THREADS) void k_ltab_add(LtabDev T, int cur, const int *frame_count, const int *offset, const int *lid,
                                                         const double *obs4, const int *match, int *counters) {
  const int w = blockIdx.x, t = threadIdx.x;
  __shared__ int lds[20];
  __shared__ int s_cnt[2];
  const int n = T.count[w], fc = frame_count[w];
  const size_t base = (size_t)w * T.F;
  int *id = T.id[cur] + base, *start = T.start[cur] + base, *nobs = T.nobs[cur] + base;
  unsigned char *tri = T.tri[cur] + base;
  double *plk = T.plk[cur] + base * 6, *obs = T.obs[cur] + base * NOBS * OW;
  const int j0 = offset[w], m = offset[w + 1] - j0;
  if (t < 2) s_cnt[t] = 0;
  __syncthreads();
  const int chunk = (m + LT_THREADS - 1) / LT_THREADS, a0 = t * chunk, a1 = min(m, a0 + chunk);
  int fresh = 0;
  for (int a = a0; a < a1; a++) fresh += match[j0 + a] < 0;
  int total_new;
  int dst = n + block_exclusive_scan<LT_THREADS>(fresh, &total_new, lds);
  if (n + total_new > T.F) { if (t == 0) atomicOr(&T.err[w], 1); total_new = 0; }
  int tracked = 0;
  for (int a = a0; a < a1; a++) {
    const int hit = match[j0 + a];
    const double *src = obs4 + (size_t)(j0 + a) * OW;
    if (hit >= 0) {
      const int k = nobs[hit];
      tracked++;
      if (start[hit] + k >= NOBS) { atomicOr(&T.err[w], 2); continue; }      // (no frame WINDOW_SIZE + 1 to observe it in)
      for (int c = 0; c < OW; c++) obs[((size_t)hit * NOBS + k) * OW + c] = src[c];
      nobs[hit] = k + 1;
    } else if (total_new > 0) {      // lineFeaturePerId(feature_id, frame_count): not triangulated, line_plucker zero
      id[dst] = lid[j0 + a]; start[dst] = fc; nobs[dst] = 1; tri[dst] = 0;
      for (int c = 0; c < 6; c++) plk[(size_t)dst * 6 + c] = 0.0;
      for (int q = 0; q < NOBS; q++) for (int c = 0; c < OW; c++) obs[((size_t)dst * NOBS + q) * OW + c] = q == 0 ? src[c] : 0.0;
      dst++;
    }
  }
  atomicAdd(&s_cnt[0], tracked); atomicAdd(&s_cnt[1], fresh);
  __syncthreads();
  if (t == 0) { T.count[w] = n + total_new; counters[2 * w] = s_cnt[0]; counters[2 * w + 1] = s_cnt[1]; }
}

// ---- triangulateLine: one thread per line (at most WINDOW_SIZE partner planes each)
// pi_from_ppp(x1, x2, x3) = [(x1 - x3) x (x2 - x3) | -x3 . (x1 x x2)]
__device__ __forceinline__ void pi_from_ppp(const vec3 &x1, const vec3 &x2, const vec3 &x3, double *pi) {
  const vec3 c = lcross(sub(x1, x3), sub(x2, x3));
  pi[0] = c[0]; pi[1] = c[1]; pi[2] = c[2];
  pi[3] = -dot3(x3, lcross(x1, x2));
}
__device__ __forceinline__ vec3 unit3(const double *p) { const double nn = lnorm3(ld3(p)); return mk3(p[0] / nn, p[1] / nn, p[2] / nn); }

__global__ __launch_bounds__(256) void k_ltab_triangulate(LtabDev T, int cur, const double *poses, const double *tic_ric) {
  const int w = blockIdx.y;
  const int n = T.count[w];
  const size_t base = (size_t)w * T.F;
  const double *PR = poses + 132 * (size_t)w, *tic = tic_ric + 12 * (size_t)w;
  __shared__ LineRT Cw[NOBS];        // the camera pose of every window frame: R_f ric, P_f + R_f tic
  if (threadIdx.x < NOBS) {
    const mat3 Rf = ldm(PR + 12 * threadIdx.x + 3);
    Cw[threadIdx.x].R = mul(Rf, ldm(tic + 3));
    Cw[threadIdx.x].t = add(ld3(PR + 12 * threadIdx.x), mv(Rf, ld3(tic)));
  }
  __syncthreads();
  for (int f = blockIdx.x * blockDim.x + threadIdx.x; f < n; f += gridDim.x * blockDim.x) {
    const int m = T.nobs[cur][base + f], s = T.start[cur][base + f];
    if (!(m >= 5 && s < GFBE_WINDOW_SIZE - 2) || T.tri[cur][base + f]) continue;      // LINE_MIN_OBS
    const double *ob = T.obs[cur] + (base + f) * NOBS * OW;
    const mat3 R0 = Cw[s].R;
    const vec3 t0 = Cw[s].t;
    double pii[4], pij[4] = {0.0, 0.0, 0.0, 0.0};
    pi_from_ppp(mk3(ob[0], ob[1], 1.0), mk3(ob[2], ob[3], 1.0), mk3(0.0, 0.0, 0.0), pii);
    const vec3 ni = unit3(pii);
    double min_cos_theta = 1.0;
    for (int k = 1; k < m; k++) {
      const vec3 tt = tmv(R0, sub(Cw[s + k].t, t0));      // tij
      const mat3 R = tmul(R0, Cw[s + k].R);               // Rij
      const vec3 p3 = add(mv(R, mk3(ob[4 * k], ob[4 * k + 1], 1.0)), tt), p4 = add(mv(R, mk3(ob[4 * k + 2], ob[4 * k + 3], 1.0)), tt);
      double pj[4];
      pi_from_ppp(p3, p4, tt, pj);
      const double cos_theta = dot3(ni, unit3(pj));
      if (cos_theta < min_cos_theta) {        // (the reference recomputes the winner's plane from the stored obsj, Rij, tij: the same values)
        min_cos_theta = cos_theta;
        for (int a = 0; a < 4; a++) pij[a] = pj[a];
      }
    }
    if (min_cos_theta > 0.998) continue;
    // pipi_plk: dp = pi1 pi2^T - pi2 pi1^T; plk = [dp03 dp13 dp23 | -dp12 dp02 -dp01], not normalised
    auto dp = [&](int a, int b) { return pii[a] * pij[b] - pij[a] * pii[b]; };
    double *plk = T.plk[cur] + (base + f) * 6;
    plk[0] = dp(0, 3); plk[1] = dp(1, 3); plk[2] = dp(2, 3); plk[3] = -dp(1, 2); plk[4] = dp(0, 2); plk[5] = -dp(0, 1);
    T.tri[cur][base + f] = 1;
  }
}

// getLineFeatureCount: lines the line-only refinement and the window solve take
__global__ __launch_bounds__(256) void k_ltab_line_count(LtabDev T, int cur, int *count_out) {
  const int w = blockIdx.x;
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const size_t base = (size_t)w * T.F;
  int mine = 0;
  for (int f = threadIdx.x; f < T.count[w]; f += 256)
    mine += T.nobs[cur][base + f] >= 5 && T.start[cur][base + f] < GFBE_WINDOW_SIZE - 2 && T.tri[cur][base + f];
  atomicAdd(&s_cnt, mine);
  __syncthreads();
  if (threadIdx.x == 0) count_out[w] = s_cnt;
}

gfbe_status lt_ready(gfbe_ctx *c, gfbe_ltab *t) { return t ? handle_device(c, t, "gfbe_ltab") : GFBE_BAD_INPUT; }
// the survivor scan and the copy into the other half; the halves swap
void lt_erase_launch(gfbe_ctx *c, gfbe_ltab *t, int op, const int *iarg, const double *da, const double *db) {
  const int W = t->d.W;
  hipLaunchKernelGGL(k_ltab_erase, dim3(W), dim3(LT_THREADS), 0, ctx_stream(c), t->d, t->cur, op, iarg);
  hipLaunchKernelGGL(k_ltab_erase_copy, dim3((unsigned)(((size_t)t->d.F * NOBS + 255) / 256), W), dim3(256), 0, ctx_stream(c), t->d, t->cur, op, da, db);
  t->cur = 1 - t->cur;
}
gfbe_status lt_erase(gfbe_ctx *c, gfbe_ltab *t, int op, const double *a, const double *b, const int32_t *iarg) {
  gfbe_status st = lt_ready(c, t);
  if (st != GFBE_OK) return st;
  const int W = t->d.W;
  t->gen++;      // (records of a reduce before this operation no longer describe the tables: gfbe_ltab_step refuses them)
  {
    Staged s(c, t, (size_t)W * 256 + 8 * 256, /*defer=*/true);
    double *da = a ? s.up(a, 12 * (size_t)W) : nullptr, *db = b ? s.up(b, 12 * (size_t)W) : nullptr;
    int *di = iarg ? s.up(iarg, W) : nullptr;
    if (!s.ok) { ctx_set_error(c, "line table operation: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    s.flush();
    lt_erase_launch(c, t, op, di, da, db);
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

}  // namespace

extern "C" {

gfbe_status gfbe_ltab_create(gfbe_ctx *c, int32_t n_tables, int32_t cap, gfbe_ltab **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  if (n_tables < 1 || cap < 1 || cap > 16384) return GFBE_BAD_INPUT;
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_ltab_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  gfbe_ltab *t = new gfbe_ltab();
  // (a failed allocation leaves nothing behind: the table built so far is destroyed and *out stays null)
  CreateGuard<gfbe_ltab> guard{c, t, gfbe_ltab_destroy};
  t->owner = c;
  LtabDev &d = t->d;
  d.W = n_tables; d.F = cap;
  const size_t N = (size_t)n_tables * cap;
#define LA(p, n) if (!t->alloc(&p, n)) return GFBE_DEVICE_ERROR
  LA(d.count, n_tables); LA(d.err, n_tables); LA(d.cnt_scratch, n_tables); LA(d.keep, N); LA(d.dst, N);
  LA(d.row, N * line_refine_row_doubles()); LA(d.plk_out, N * 6); LA(d.rkeep, N);
  for (int b = 0; b < 2; b++) {
    LA(d.id[b], N); LA(d.start[b], N); LA(d.nobs[b], N); LA(d.tri[b], N); LA(d.plk[b], N * 6); LA(d.obs[b], N * NOBS * OW);
  }
#undef LA
  if (!t->make_staging(c, "gfbe_ltab_create", (size_t)n_tables * (sizeof(gfbe_summary) + 1024), true)) return GFBE_DEVICE_ERROR;
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  guard.armed = false;
  *out = t;
  return GFBE_OK;
}

void gfbe_ltab_destroy(gfbe_ctx *c, gfbe_ltab *t) {
  if (!t) return;
  t->release(c);
  for (const DevBuf *b : {&t->reduce_buf, &t->rec_buf, &t->step_buf})
    if (b->d) (void)hipFree(b->d);
  delete t;
}

gfbe_status gfbe_ltab_add_frame(gfbe_ctx *c, gfbe_ltab *t, const int32_t *frame_count, const int32_t *offset, const int32_t *line_id,
                                const double *obs4, int32_t *counters) {
  gfbe_status st = lt_ready(c, t);
  if (st != GFBE_OK) return st;
  if (!frame_count || !offset) return GFBE_BAD_INPUT;
  const int W = t->d.W, M = offset[W];
  if (offset[0] != 0 || M < 0 || (M > 0 && (!line_id || !obs4))) return GFBE_BAD_INPUT;
  for (int w = 0; w < W; w++) {
    if (offset[w + 1] < offset[w]) return GFBE_BAD_INPUT;
    for (int k = offset[w] + 1; k < offset[w + 1]; k++)
      if (line_id[k] <= line_id[k - 1]) { ctx_set_error(c, "gfbe_ltab_add_frame: line ids of a table must be strictly ascending"); return GFBE_BAD_INPUT; }
  }
  std::vector<int> err(W, 0);
  t->gen++;
  {
    Staged s(c, t, (size_t)M * (OW * 8 + 8) + (size_t)W * 64 + 16 * 256);
    int *dfc = s.up(frame_count, W), *doff = s.up(offset, W + 1), *dlid = s.up(line_id, M);
    double *dobs = s.up(obs4, (size_t)M * OW);
    int *dmatch = s.up<int>(nullptr, M), *dcnt = s.up<int>(nullptr, 2 * (size_t)W), *derr = s.up<int>(nullptr, W);
    if (!s.ok) { ctx_set_error(c, "gfbe_ltab_add_frame: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    s.flush();
    int mmax = 1;
    for (int w = 0; w < W; w++) mmax = std::max(mmax, offset[w + 1] - offset[w]);
    (void)hipMemsetAsync(dmatch, 0xFF, sizeof(int) * (size_t)std::max(M, 1), ctx_stream(c));     // -1: not in the list
    hipLaunchKernelGGL(k_ltab_match, dim3((mmax + 63) / 64, (t->d.F + LT_MATCH_TILE - 1) / LT_MATCH_TILE, W), dim3(64), 0, ctx_stream(c), t->d, t->cur, doff, dlid, dmatch);
    hipLaunchKernelGGL(k_ltab_add, dim3(W), dim3(LT_THREADS), 0, ctx_stream(c), t->d, t->cur, dfc, doff, dlid, dobs, dmatch, dcnt);
    // the tables' sticky error flags (only this operation raises them) travel back with the results: one copy, one wait
    (void)hipMemcpyAsync(derr, t->d.err, sizeof(int) * W, hipMemcpyDeviceToDevice, ctx_stream(c));
    s.down(counters, dcnt, 2 * (size_t)W); s.down(err.data(), derr, W);
  }
  GFBE_CHECK(c, hipGetLastError());
  for (int w = 0; w < W; w++)
    if (err[w]) { ctx_set_error(c, err[w] & 1 ? "line table capacity exceeded" : "a line received more than WINDOW_SIZE + 1 observations"); return GFBE_BAD_INPUT; }
  return GFBE_OK;
}

gfbe_status gfbe_ltab_triangulate(gfbe_ctx *c, gfbe_ltab *t, const double *poses, const double *tic_ric) {
  gfbe_status st = lt_ready(c, t);
  if (st != GFBE_OK) return st;
  if (!poses || !tic_ric) return GFBE_BAD_INPUT;
  const int W = t->d.W;
  t->gen++;
  {
    Staged s(c, t, (size_t)W * 144 * 8 + 8 * 256, /*defer=*/true);
    double *dp = s.up(poses, 132 * (size_t)W), *de = s.up(tic_ric, 12 * (size_t)W);
    if (!s.ok) { ctx_set_error(c, "line table operation: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    s.flush();
    hipLaunchKernelGGL(k_ltab_triangulate, dim3((t->d.F + 255) / 256, W), dim3(256), 0, ctx_stream(c), t->d, t->cur, dp, de);
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_ltab_remove_back_shift(gfbe_ctx *c, gfbe_ltab *t, const double *marg_PR, const double *new_PR) {
  if (!marg_PR || !new_PR) return GFBE_BAD_INPUT;
  return lt_erase(c, t, OP_BACK_SHIFT, marg_PR, new_PR, nullptr);
}
gfbe_status gfbe_ltab_remove_back(gfbe_ctx *c, gfbe_ltab *t) { return lt_erase(c, t, OP_BACK, nullptr, nullptr, nullptr); }
gfbe_status gfbe_ltab_remove_front(gfbe_ctx *c, gfbe_ltab *t, const int32_t *frame_count) {
  if (!frame_count) return GFBE_BAD_INPUT;
  return lt_erase(c, t, OP_FRONT, nullptr, nullptr, frame_count);
}

gfbe_status gfbe_ltab_refine(gfbe_ctx *c, gfbe_ltab *t, const double *pose7, const double *ex_cam, double sqrt_info, double cauchy_scale,
                             int32_t max_num_iterations, gfbe_summary *summary) {
  gfbe_status st = lt_ready(c, t);
  if (st != GFBE_OK) return st;
  if (!pose7 || !ex_cam || !summary || !(cauchy_scale > 0.0) || max_num_iterations < 0) return GFBE_BAD_INPUT;
  const int W = t->d.W;
  std::vector<gfbe_summary> h_sum(W);
  t->gen++;
  {
    Staged s(c, t, (size_t)W * (84 * 8 + sizeof(gfbe_summary)) + 8 * 256);
    double *dp = s.up(pose7, 77 * (size_t)W), *de = s.up(ex_cam, 7 * (size_t)W);
    gfbe_summary *dsum = s.up<gfbe_summary>(nullptr, W);
    if (!s.ok) { ctx_set_error(c, "gfbe_ltab_refine: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    s.flush();
    launch_line_refine_tables(ltab_line_list(*t, dp, de), W, sqrt_info, cauchy_scale, max_num_iterations, t->d.row, t->d.plk_out, t->d.rkeep, dsum, ctx_stream(c));
    // setLineOrth + the erasures of removeLineOutlier, in place: refined lines written back, culled lines erased in order
    lt_erase_launch(c, t, OP_REFINE, nullptr, nullptr, nullptr);
    s.down(h_sum.data(), dsum, W);
  }
  GFBE_CHECK(c, hipGetLastError());
  int worst = GFBE_OK;
  for (int w = 0; w < W; w++) worst = std::max(worst, (int)h_sum[w].status);
  std::memcpy(summary, h_sum.data(), sizeof(gfbe_summary) * (size_t)W);
  return (gfbe_status)worst;
}

gfbe_status gfbe_ltab_size(gfbe_ctx *c, gfbe_ltab *t, int32_t *n) {
  gfbe_status st = lt_ready(c, t);
  if (st != GFBE_OK) return st;
  if (!n) return GFBE_BAD_INPUT;
  GFBE_CHECK(c, hipMemcpyAsync(t->stage_h, t->d.count, sizeof(int) * t->d.W, hipMemcpyDeviceToHost, ctx_stream(c)));   // (through the pinned mirror)
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  std::memcpy(n, t->stage_h, sizeof(int) * t->d.W);
  return GFBE_OK;
}

gfbe_status gfbe_ltab_line_count(gfbe_ctx *c, gfbe_ltab *t, int32_t *count) {
  gfbe_status st = lt_ready(c, t);
  if (st != GFBE_OK) return st;
  if (!count) return GFBE_BAD_INPUT;
  const int W = t->d.W;
  {
    Staged s(c, t, (size_t)W * 4 + 4 * 256);
    int *dcnt = s.up<int>(nullptr, W);
    if (!s.ok) { ctx_set_error(c, "line table operation: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    hipLaunchKernelGGL(k_ltab_line_count, dim3(W), dim3(256), 0, ctx_stream(c), t->d, t->cur, dcnt);
    s.down(count, dcnt, W);
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_ltab_download(gfbe_ctx *c, gfbe_ltab *t, int32_t w, int32_t *id, int32_t *start, int32_t *nobs, double *obs4,
                               uint8_t *tri, double *plk) {
  gfbe_status st = lt_ready(c, t);
  if (st != GFBE_OK) return st;
  if (w < 0 || w >= t->d.W) return GFBE_BAD_INPUT;
  hipStream_t s = ctx_stream(c);
  GFBE_CHECK(c, hipMemcpyAsync(t->stage_h, t->d.count + w, sizeof(int), hipMemcpyDeviceToHost, s));
  GFBE_CHECK(c, hipStreamSynchronize(s));
  const int n = *(const int *)t->stage_h;
  const size_t base = (size_t)w * t->d.F;
  const int b = t->cur;
#define DN(h, dptr, cnt) if (h && n) GFBE_CHECK(c, hipMemcpyAsync(h, dptr, sizeof(*h) * (cnt), hipMemcpyDeviceToHost, s))
  DN(id, t->d.id[b] + base, (size_t)n); DN(start, t->d.start[b] + base, (size_t)n); DN(nobs, t->d.nobs[b] + base, (size_t)n);
  DN(tri, t->d.tri[b] + base, (size_t)n); DN(plk, t->d.plk[b] + base * 6, (size_t)n * 6);
  DN(obs4, t->d.obs[b] + base * NOBS * OW, (size_t)n * NOBS * OW);
#undef DN
  GFBE_CHECK(c, hipStreamSynchronize(s));
  return GFBE_OK;
}

gfbe_status gfbe_ltab_upload(gfbe_ctx *c, gfbe_ltab *t, int32_t w, int32_t n, const int32_t *id, const int32_t *start, const int32_t *nobs,
                             const double *obs4, const uint8_t *tri, const double *plk) {
  gfbe_status st = lt_ready(c, t);
  if (st != GFBE_OK) return st;
  if (w < 0 || w >= t->d.W || n < 0 || n > t->d.F || (n > 0 && (!id || !start || !nobs || !obs4 || !tri || !plk))) return GFBE_BAD_INPUT;
  for (int i = 0; i < n; i++)
    if (start[i] < 0 || nobs[i] < 1 || start[i] + nobs[i] > NOBS) { ctx_set_error(c, "gfbe_ltab_upload: a line's observations must lie in frames 0 .. WINDOW_SIZE"); return GFBE_BAD_INPUT; }
  const size_t base = (size_t)w * t->d.F;
  const int b = t->cur;
  t->gen++;
  {
    // one staged copy up, then device-to-device into the table's arrays; observation rows past n_obs are stored as zeros
    const size_t N = (size_t)std::max(n, 1);
    Staged s(c, t, N * (3 * 4 + 1 + 6 * 8 + NOBS * OW * 8) + 8 * 256);
    int *dn = s.up(&n, 1), *did = s.up(id, n), *dst = s.up(start, n), *dno = s.up(nobs, n);
    uint8_t *dtri = s.up(tri, n);
    double *dplk = s.up(plk, (size_t)n * 6);
    double *dobs = s.up<double>(nullptr, (size_t)n * NOBS * OW);
    if (!s.ok) { ctx_set_error(c, "gfbe_ltab_upload: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    if (n) {
      double *ho = (double *)(s.bh + ((char *)dobs - s.bd));
      for (int i = 0; i < n; i++)
        for (int q = 0; q < NOBS; q++)
          for (int a = 0; a < OW; a++) ho[((size_t)i * NOBS + q) * OW + a] = q < nobs[i] ? obs4[((size_t)i * NOBS + q) * OW + a] : 0.0;
      s.ulo = std::min(s.ulo, (size_t)((char *)dobs - s.bd));
      s.uhi = std::max(s.uhi, (size_t)((char *)dobs - s.bd) + sizeof(double) * (size_t)n * NOBS * OW);
    }
    s.flush();
    hipStream_t q = ctx_stream(c);
#define UP(dptr, src, cnt) if (n) GFBE_CHECK(c, hipMemcpyAsync(dptr, src, sizeof(*src) * (cnt), hipMemcpyDeviceToDevice, q))
    UP(t->d.id[b] + base, did, (size_t)n); UP(t->d.start[b] + base, dst, (size_t)n); UP(t->d.nobs[b] + base, dno, (size_t)n);
    UP(t->d.tri[b] + base, dtri, (size_t)n); UP(t->d.plk[b] + base * 6, dplk, (size_t)n * 6);
    UP(t->d.obs[b] + base * NOBS * OW, dobs, (size_t)n * NOBS * OW);
#undef UP
    GFBE_CHECK(c, hipMemcpyAsync(t->d.count + w, dn, sizeof(int), hipMemcpyDeviceToDevice, q));
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

}  // extern "C"
