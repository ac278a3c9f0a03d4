// gfbe_line_reduce.hip — reduced normal equations of a window's line factors: the line loops of optimizationwithLine()
// (estimator/estimator.cpp:4566-4598 solve, :4736-4771 MARGIN_OLD), linearised with respect to the poses, the camera extrinsic and the
// lines, the 4 x 4 line blocks eliminated (include/gfbe.h: gfbe_line_reduce / gfbe_ltab_reduce):
//
//     H = U - sum_l W_l V'_l^-1 W_l^T,  g = bp - sum_l W_l V'_l^-1 bl      on the 72 dims [pose 0 .. pose 10 | ex_cam]
//
// Shape: ONE WORKGROUP PER WINDOW AT A TIME (a workgroup walks windows blockIdx.x, blockIdx.x + gridDim.x, ...; its scratch slab is
// its own, so a window's bits do not depend on the batch). Per window:
//   rank    the eligible lines in list order (block scan), rank -> line
//   lines   a thread owns eligible lines t, t + 256, ...: line_reduce_line (gfbe_line.h) — every observation's factor with all three
//           Jacobians, V_l, bl, the 6 x 4 blocks of W_l, the 4 x 4 Cholesky and V'^-1 — into the line's scratch row
//   chunks  RC_CHUNK lines at a time are staged in LDS as Y = W V'^-1 and W, [line][k][80 rows] (leading dimension 80 = 16 mod 32
//           doubles: the two 16-lane halves of a ds_read_b64 lane group land on disjoint banks, no conflict per matrix-core operand);
//           ONE LINE IS ONE K = 4 SLICE of v_mfma_f64_16x16x4_f64: the 15 lower 16 x 16 tiles of sum_l Y_l W_l^T are spread over the
//           four waves and accumulated in registers over all chunks, in line order. U and bp are block-sparse: 11 frames x 90 entries
//           (pose-pose 21, pose-extrinsic 36, extrinsic-extrinsic 21, bp 6 + 6), a thread owns up to four of them and sums the
//           chunk's observation records from LDS in line order; threads 0..71 sum their row of sum_l Y_l bl.
//   finish  tiles and frame sums through LDS; H, U written from the lower triangle and mirrored (symmetric bit for bit)
// No atomics, no grid barrier; FP64 throughout. A failed line (no Cholesky factor) is staged as zeros and skipped in U, bp, cost.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"
#include "gfbe_line.h"
#include "gfbe_tabstage.h"

using namespace gfd;

namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));

enum { RC_THREADS = 256, RC_WAVES = 4, RC_CHUNK = 8, RC_LD = 80, RC_NP = LINE_NP, RC_NT = 15, RC_TASKS = GFBE_NFRAMES * 90,
       RC_TPT = (RC_TASKS + RC_THREADS - 1) / RC_THREADS, RC_MAX_GRID = 256,
       RC_STAGE = 2 * RC_CHUNK * 4 * RC_LD,        // doubles: Y and W of a chunk; reused for the 15 tiles + the frame sums at the end
       RC_WROW = RC_NP * 4, RC_JROW = GFBE_NFRAMES * LINE_JREC };
static_assert(RC_NT * 256 + RC_TASKS <= RC_STAGE, "the finish phase reuses the chunk staging area");

struct ReduceBatch {
  // the lines, as LineBatch of gfbe_line.hip: host-fed CSR or the tables in place
  const int *line_off, *obs_off;       // host-fed
  const int *count, *nobs;             // table-fed
  int F;
  const int *start;
  const unsigned char *tri;
  const double *plk_in, *obs, *pose, *ex;
  double sqrt_info, huber, mu;
  int mode, n_windows, slab_lines;     // slab_lines: line slots of one workgroup's scratch slab
  const int *rec_off;                  // [n_windows] first record slot of a window (prefix of the line counts)
  // scratch, per workgroup slab [gridDim.x][slab_lines]
  int *lineof;
  double *Wrow, *Jrec, *Vinv, *bl, *Vl;       // (Vl: the lower triangle of V_l, the step side's record)
  unsigned char *failed;
  // outputs (null: not wanted)
  double *H, *g, *U, *bp, *cost, *ms;
  int *n_elig, *n_failed;
  double *oVinv, *obl, *oW, *oV;
  unsigned char *ofailed;
};

// the lines that enter: the predicate of gfbe_line_refine (gfbe_line.h), and in MARG_OLD mode only those that start in frame 0
template <bool TAB>
__device__ __forceinline__ bool rb_eligible(const ReduceBatch &P, int l) {
  return line_eligible<TAB>(P, l) && (P.mode == GFBE_LINE_REDUCE_SOLVE || P.start[l] == 0);
}

// offsets of the two products of frame-sum entry e (0..89) in an observation record [r(2) | Jp(2 x 6) | Je(2 x 6)]:
// value = rec[a] rec[b] + rec[a2] rec[b2]
__device__ void rc_decode(int e, int *a, int *a2, int *b, int *b2) {
  auto tri = [](int q, int *i, int *j) { int r = 0; while ((r + 1) * (r + 2) / 2 <= q) r++; *i = r; *j = q - r * (r + 1) / 2; };
  int i, j;
  if (e < 21) { tri(e, &i, &j); *a = 2 + i; *a2 = 8 + i; *b = 2 + j; *b2 = 8 + j; }
  else if (e < 57) { i = (e - 21) / 6; j = (e - 21) % 6; *a = 2 + i; *a2 = 8 + i; *b = 14 + j; *b2 = 20 + j; }
  else if (e < 78) { tri(e - 57, &i, &j); *a = 14 + i; *a2 = 20 + i; *b = 14 + j; *b2 = 20 + j; }
  else if (e < 84) { i = e - 78; *a = 2 + i; *a2 = 8 + i; *b = 0; *b2 = 1; }
  else { i = e - 84; *a = 14 + i; *a2 = 20 + i; *b = 0; *b2 = 1; }
}

// fixed-order sum of two per-thread values over the workgroup (wave shuffle tree, then the waves in order); every thread gets both
__device__ void rc_reduce2(double v0, double v1, double (*sh)[RC_WAVES], double *out) {
  const int t = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { v0 += __shfl_down(v0, o, 64); v1 += __shfl_down(v1, o, 64); }
  if ((t & 63) == 0) { sh[0][t >> 6] = v0; sh[1][t >> 6] = v1; }
  __syncthreads();
  double a = 0.0, b = 0.0;
  for (int q = 0; q < RC_WAVES; q++) { a += sh[0][q]; b += sh[1][q]; }
  out[0] = a; out[1] = b;
  __syncthreads();
}

template <bool TAB>
__global__ __launch_bounds__(RC_THREADS) void k_line_reduce(ReduceBatch P) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4;
  __shared__ LineRT Bs[GFBE_NFRAMES], Cw[GFBE_NFRAMES];
  __shared__ LineRT Ex;
  __shared__ double stage[RC_STAGE];
  __shared__ double sJ[RC_CHUNK * RC_JROW];
  __shared__ double sbl[RC_CHUNK][4];
  __shared__ int smeta[RC_CHUNK][3];           // start, first observation, observations (0: the line is not in the sums)
  __shared__ double sh[2][RC_WAVES];
  __shared__ int scan_lds[20];
  double *sY = stage, *sW = stage + RC_CHUNK * 4 * RC_LD;
  const size_t slab = (size_t)blockIdx.x * P.slab_lines;
  int *lineof = P.lineof + slab;
  double *Wrow = P.Wrow + slab * RC_WROW, *Jrec = P.Jrec + slab * RC_JROW, *Vinv = P.Vinv + slab * 16, *bl = P.bl + slab * 4;
  double *Vl = P.Vl + slab * 10;
  unsigned char *failed = P.failed + slab;
  // the frame-sum entries of this thread
  int tf[RC_TPT], ta[RC_TPT], ta2[RC_TPT], tb[RC_TPT], tb2[RC_TPT];
#pragma unroll
  for (int q = 0; q < RC_TPT; q++) {
    const int task = t + q * RC_THREADS;
    tf[q] = task < RC_TASKS ? task / 90 : -1;
    rc_decode(task < RC_TASKS ? task % 90 : 0, &ta[q], &ta2[q], &tb[q], &tb2[q]);
  }
  // the tiles of this wave: tile index ti = wave + 4 q over the lower triangle (I >= J) of the 5 x 5 tile grid
  int tI[4], tJ[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int ti = wave + RC_WAVES * q;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= ti) I++;
    tI[q] = I; tJ[q] = ti - I * (I + 1) / 2;
  }
  const int k0 = P.mode == GFBE_LINE_REDUCE_MARG_OLD ? 1 : 0;

  for (int w = blockIdx.x; w < P.n_windows; w += gridDim.x) {
    const uint64_t t_start = P.ms ? wall_clock64() : 0;      // (the clock is read only when ms_kernel is asked for)
    uint64_t t_mfma = 0;
    const int l0 = TAB ? w * P.F : P.line_off[w], l1 = TAB ? l0 + P.count[w] : P.line_off[w + 1];
    __syncthreads();                               // (the previous window's readers of LDS are done)
    if (t < GFBE_NFRAMES) Bs[t] = line_make_pose(P.pose + (size_t)w * 77 + 7 * t);
    if (t == GFBE_NFRAMES) Ex = line_make_pose(P.ex + (size_t)w * 7);
    for (int q = t; q < RC_STAGE; q += RC_THREADS) stage[q] = 0.0;      // (rows 72..79 of every operand stay zero)
    __syncthreads();
    if (t < GFBE_NFRAMES) { Cw[t].R = mul(Bs[t].R, Ex.R); Cw[t].t = add(Bs[t].t, mv(Bs[t].R, Ex.t)); }   // Rwc = Rs ric, twc = Ps + Rs tic
    // ---- rank: eligible lines in list order
    int n_elig = 0;
    for (int c0 = l0; c0 < l1; c0 += RC_THREADS) {
      const int l = c0 + t;
      const int e = (l < l1 && rb_eligible<TAB>(P, l)) ? 1 : 0;
      int total;
      const int ex = block_exclusive_scan<RC_THREADS>(e, &total, scan_lds);
      if (e) lineof[n_elig + ex] = l;
      n_elig += total;
    }
    __threadfence();
    __syncthreads();
    // ---- lines
    double csum = 0.0, nfail = 0.0;
    for (int q = t; q < n_elig; q += RC_THREADS) {
      const int l = lineof[q], s = P.start[l];
      double lw[6], x[4], c;
      line_plk_to_pose(P.plk_in + 6 * (size_t)l, Cw[s].R, Cw[s].t, lw);     // para_LineFeature = plk_to_orth(plk_to_pose(line_plucker, Rwc, twc))
      line_plk_to_orth(lw, x);
      const bool ok = line_reduce_line(Bs, Ex, x, s, k0, line_nobs<TAB>(P, l), line_obs<TAB>(P, l), P.sqrt_info, P.huber, P.mu,
                                       Wrow + (size_t)q * RC_WROW, Jrec + (size_t)q * RC_JROW, Vinv + (size_t)q * 16, bl + (size_t)q * 4, &c,
                                       Vl + (size_t)q * 10);
      failed[q] = ok ? 0 : 1;
      if (ok) csum += c; else nfail += 1.0;
    }
    __threadfence();
    double red[2];
    rc_reduce2(csum, nfail, sh, red);
    // ---- chunks
    dbl4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = dbl4{0.0, 0.0, 0.0, 0.0};
    double usum[RC_TPT], gsum = 0.0;
#pragma unroll
    for (int q = 0; q < RC_TPT; q++) usum[q] = 0.0;
    for (int q0 = 0; q0 < n_elig; q0 += RC_CHUNK) {
      const int nc = min(RC_CHUNK, n_elig - q0);
      if (t < RC_CHUNK) {
        const bool in = t < nc && !failed[q0 + t];
        const int l = in ? lineof[q0 + t] : 0;
        smeta[t][0] = in ? P.start[l] : 0; smeta[t][1] = k0; smeta[t][2] = in ? line_nobs<TAB>(P, l) : 0;
      }
      if (t < RC_CHUNK * 4) {
        const int c = t >> 2;
        sbl[c][t & 3] = (c < nc && !failed[q0 + c]) ? bl[(size_t)(q0 + c) * 4 + (t & 3)] : 0.0;
      }
      for (int i = t; i < RC_CHUNK * RC_NP; i += RC_THREADS) {
        const int c = i / RC_NP, row = i % RC_NP;
        double wv[4] = {0.0, 0.0, 0.0, 0.0}, yv[4] = {0.0, 0.0, 0.0, 0.0};
        if (c < nc && !failed[q0 + c]) {
          const double *wp = Wrow + (size_t)(q0 + c) * RC_WROW + 4 * row;
          for (int a = 0; a < 4; a++) wv[a] = wp[a];
          line_Y_row(wv, Vinv + (size_t)(q0 + c) * 16, yv);
        }
        for (int a = 0; a < 4; a++) { sW[(c * 4 + a) * RC_LD + row] = wv[a]; sY[(c * 4 + a) * RC_LD + row] = yv[a]; }
      }
      for (int i = t; i < nc * RC_JROW; i += RC_THREADS) sJ[i] = Jrec[(size_t)q0 * RC_JROW + i];
      __syncthreads();
      // the contraction: one line = one K = 4 slice
      const uint64_t m0 = P.ms ? wall_clock64() : 0;
      for (int c = 0; c < nc; c++) {
        if (smeta[c][2] == 0) continue;              // (a failed line: zeros; block-uniform)
        const double *yc = sY + (c * 4 + lk) * RC_LD + lr, *wc = sW + (c * 4 + lk) * RC_LD + lr;
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (wave + RC_WAVES * q < RC_NT) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(yc[16 * tI[q]], wc[16 * tJ[q]], acc[q], 0, 0, 0);
      }
      if (P.ms) t_mfma += wall_clock64() - m0;
      // U, bp: the frame sums
#pragma unroll
      for (int q = 0; q < RC_TPT; q++) {
        if (tf[q] < 0) continue;
        for (int c = 0; c < nc; c++) {
          const int k = tf[q] - smeta[c][0];
          if (k < smeta[c][1] || k >= smeta[c][2]) continue;
          const double *rec = sJ + c * RC_JROW + k * LINE_JREC;
          usum[q] += rec[ta[q]] * rec[tb[q]] + rec[ta2[q]] * rec[tb2[q]];
        }
      }
      if (t < RC_NP)
        for (int c = 0; c < nc; c++) {
          if (smeta[c][2] == 0) continue;
          double s = 0.0;
          for (int a = 0; a < 4; a++) s += sY[(c * 4 + a) * RC_LD + t] * sbl[c][a];
          gsum += s;
        }
      __syncthreads();
    }
    // ---- finish: tiles and frame sums through LDS
    double *sS = stage, *sR = stage + RC_NT * 256;
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (wave + RC_WAVES * q < RC_NT)
        for (int i = 0; i < 4; i++) sS[(wave + RC_WAVES * q) * 256 + (lk + 4 * i) * 16 + lr] = acc[q][i];     // D: row lk + 4 i, column lr
#pragma unroll
    for (int q = 0; q < RC_TPT; q++)
      if (tf[q] >= 0) sR[t + q * RC_THREADS] = usum[q];
    __syncthreads();
    auto tri_at = [](int a, int b) { return a * (a + 1) / 2 + b; };
    auto U_at = [&](int hi, int lo) -> double {        // hi >= lo
      if (hi < 66) return hi / 6 == lo / 6 ? sR[(hi / 6) * 90 + tri_at(hi % 6, lo % 6)] : 0.0;
      if (lo < 66) return sR[(lo / 6) * 90 + 21 + (lo % 6) * 6 + (hi - 66)];
      double s = 0.0;
      for (int f = 0; f < GFBE_NFRAMES; f++) s += sR[f * 90 + 57 + tri_at(hi - 66, lo - 66)];
      return s;
    };
    for (int idx = t; idx < RC_NP * RC_NP; idx += RC_THREADS) {
      const int i = idx / RC_NP, j = idx % RC_NP, hi = max(i, j), lo = min(i, j);
      const double u = U_at(hi, lo);
      const int I = hi >> 4, J = lo >> 4;
      const double s = sS[(I * (I + 1) / 2 + J) * 256 + (hi & 15) * 16 + (lo & 15)];
      if (P.U) P.U[(size_t)w * RC_NP * RC_NP + idx] = u;
      if (P.H) P.H[(size_t)w * RC_NP * RC_NP + idx] = u - s;
    }
    if (t < RC_NP) {
      double b = 0.0;
      if (t < 66) b = sR[(t / 6) * 90 + 78 + t % 6];
      else for (int f = 0; f < GFBE_NFRAMES; f++) b += sR[f * 90 + 84 + (t - 66)];
      if (P.bp) P.bp[(size_t)w * RC_NP + t] = b;
      if (P.g) P.g[(size_t)w * RC_NP + t] = b - gsum;
    }
    // the per-line records
    const size_t ro = (size_t)P.rec_off[w];
    if (P.oVinv) for (int i = t; i < n_elig * 16; i += RC_THREADS) P.oVinv[ro * 16 + i] = failed[i >> 4] ? 0.0 : Vinv[i];
    if (P.obl) for (int i = t; i < n_elig * 4; i += RC_THREADS) P.obl[ro * 4 + i] = failed[i >> 2] ? 0.0 : bl[i];
    if (P.oW) for (int i = t; i < n_elig * RC_WROW; i += RC_THREADS) P.oW[ro * RC_WROW + i] = failed[i / RC_WROW] ? 0.0 : Wrow[i];
    if (P.oV) for (int i = t; i < n_elig * 10; i += RC_THREADS) P.oV[ro * 10 + i] = failed[i / 10] ? 0.0 : Vl[i];
    if (P.ofailed) for (int i = t; i < n_elig; i += RC_THREADS) P.ofailed[ro + i] = failed[i];
    if (t == 0) {
      if (P.cost) P.cost[w] = red[0];
      if (P.n_elig) P.n_elig[w] = n_elig;
      if (P.n_failed) P.n_failed[w] = (int)red[1];
      if (P.ms) { P.ms[2 * w] = (double)(wall_clock64() - t_start) * 1e-5; P.ms[2 * w + 1] = (double)t_mfma * 1e-5; }   // (100 MHz device wall clock)
    }
    __threadfence();                               // (the slab is written again by the next window of this workgroup)
  }
}

#define RD_CHECK(c, call)                                                                                      \
  do {                                                                                                         \
    hipError_t e_ = (call);                                                                                    \
    if (e_ != hipSuccess) { ctx_set_error(c, (std::string(#call) + ": " + hipGetErrorString(e_)).c_str()); st = GFBE_DEVICE_ERROR; goto done; } \
  } while (0)

bool reduce_args_ok(gfbe_ctx *c, const char *who, int32_t mode, double mu, const gfbe_line_reduced *out) {
  // (both sizes of the structure are admitted: a caller built before the member V existed sees no change)
  if (!out || (out->struct_size != (int32_t)sizeof(gfbe_line_reduced) && out->struct_size != GFBE_LINE_REDUCED_SIZE_V0)) { ctx_set_error(c, (std::string(who) + ": gfbe_line_reduced ABI mismatch").c_str()); return false; }
  if (mode != GFBE_LINE_REDUCE_SOLVE && mode != GFBE_LINE_REDUCE_MARG_OLD) return false;
  return mu >= 0.0 && std::isfinite(mu);
}
// the caller's structure at the library's size (V = NULL for the smaller one)
gfbe_line_reduced reduced_full(const gfbe_line_reduced *out) {
  gfbe_line_reduced r{};
  std::memcpy(&r, out, (size_t)out->struct_size);
  if (out->struct_size == GFBE_LINE_REDUCED_SIZE_V0) r.V = nullptr;
  return r;
}

// Launch and hand-over shared by the two entry points. P: the line inputs on the device; nlines [W]: lines per window (the record
// slots). h_pose / h_ex (table-fed): the poses on the host, copied into the call's allocation. cache (table-fed): the table handle's
// scratch allocation, kept between calls and grown on demand — a per-frame caller pays no hipMalloc / hipFree; without it the
// allocation lives for the call (the host-fed entry point, as gfbe_line_refine). keep (table-fed, solve mode, gfbe_ltab_keep_records on):
// the per-line records are written into the store on the table handle instead of the call's allocation — the same values from the same
// kernel, so the call's outputs keep their bits — and stay there for gfbe_ltab_step.
struct ReduceCache { char **d; size_t *cap; };
template <bool TAB>
gfbe_status reduce_run(gfbe_ctx *c, ReduceBatch P, int W, const std::vector<int> &nlines, const gfbe_line_reduced *out, const double *h_pose,
                       const double *h_ex, ReduceCache cache, gfbe_ltab *keep = nullptr) {
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  std::vector<int> rec_off(W + 1, 0);
  int maxl = 0;
  for (int w = 0; w < W; w++) { rec_off[w + 1] = rec_off[w] + nlines[w]; maxl = std::max(maxl, nlines[w]); }
  const size_t N = (size_t)rec_off[W], n72 = (size_t)W * RC_NP, n5k = n72 * RC_NP;
  const int grid = std::min(W, (int)RC_MAX_GRID);
  const size_t slab_lines = (size_t)maxl + RC_CHUNK, S = (size_t)grid * slab_lines;
  auto up8 = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const bool rec = out->Vinv || out->bl || out->W || out->failed || out->V;
  char *d = nullptr;
  std::vector<double> hH, hU, hg, hbp, hcost, hms, hV, hb, hW, hVl;
  std::vector<int> hne(W), hnf(W);
  std::vector<unsigned char> hf;
  // the layout of the call's one device allocation: laid out once from a null base for its size, then from the allocation
  int *d_rec = nullptr;
  auto layout = [&](char *p) -> size_t {
    char *const p0 = p;
    auto take = [&](size_t bytes) { char *q = p; p += up8(bytes); return q; };
    d_rec = (int *)take(sizeof(int) * (W + 1));
    P.rec_off = d_rec;
    if (h_pose) { P.pose = (double *)take(8 * 77 * (size_t)W); P.ex = (double *)take(8 * 7 * (size_t)W); }
    P.lineof = (int *)take(sizeof(int) * S);
    P.Wrow = (double *)take(8 * S * RC_WROW); P.Jrec = (double *)take(8 * S * RC_JROW);
    P.Vinv = (double *)take(8 * S * 16); P.bl = (double *)take(8 * S * 4); P.Vl = (double *)take(8 * S * 10); P.failed = (unsigned char *)take(S);
    P.H = out->H ? (double *)take(8 * n5k) : nullptr; P.U = out->U ? (double *)take(8 * n5k) : nullptr;
    P.g = (double *)take(8 * n72); P.bp = (double *)take(8 * n72);
    P.cost = (double *)take(8 * (size_t)W); P.ms = out->ms_kernel ? (double *)take(16 * (size_t)W) : nullptr;
    P.n_elig = (int *)take(4 * (size_t)W); P.n_failed = (int *)take(4 * (size_t)W);
    if (rec && !keep) {
      P.oVinv = out->Vinv ? (double *)take(8 * N * 16) : nullptr; P.obl = out->bl ? (double *)take(8 * N * 4) : nullptr;
      P.oW = out->W ? (double *)take(8 * N * RC_WROW) : nullptr; P.oV = out->V ? (double *)take(8 * N * 10) : nullptr;
      P.ofailed = (unsigned char *)take(N + 1);
    }
    return (size_t)(p - p0);
  };
  // the store on the table handle: rec_off, then every record array at full size
  int *k_off = nullptr;
  auto keep_layout = [&](char *p) -> size_t {
    char *const p0 = p;
    auto take = [&](size_t bytes) { char *q = p; p += up8(bytes); return q; };
    k_off = (int *)take(sizeof(int) * (W + 1));
    P.oVinv = (double *)take(8 * N * 16); P.obl = (double *)take(8 * N * 4); P.oW = (double *)take(8 * N * RC_WROW);
    P.oV = (double *)take(8 * N * 10); P.ofailed = (unsigned char *)take(N + 1);
    return (size_t)(p - p0);
  };
  {
    const size_t need = layout(nullptr);
    if (cache.d && *cache.cap >= need) {
      d = *cache.d;
    } else {
      if (cache.d && *cache.d) { RD_CHECK(c, hipStreamSynchronize(s)); (void)hipFree(*cache.d); *cache.d = nullptr; *cache.cap = 0; }
      RD_CHECK(c, hipMalloc((void **)&d, need));
      if (cache.d) { *cache.d = d; *cache.cap = need; }
    }
    (void)layout(d);
    if (keep) {
      keep->rec_valid = false; keep->cand_valid = false;
      const size_t kneed = keep_layout(nullptr);
      if (keep->rec_cap < kneed) {
        RD_CHECK(c, hipStreamSynchronize(s));
        if (keep->rec_d) { (void)hipFree(keep->rec_d); keep->rec_d = nullptr; keep->rec_cap = 0; }
        RD_CHECK(c, hipMalloc((void **)&keep->rec_d, kneed));
        keep->rec_cap = kneed;
      }
      (void)keep_layout(keep->rec_d);
      RD_CHECK(c, hipMemcpyAsync(k_off, rec_off.data(), sizeof(int) * (W + 1), hipMemcpyHostToDevice, s));
    }
    P.n_windows = W; P.slab_lines = (int)slab_lines;
    if (h_pose) {
      RD_CHECK(c, hipMemcpyAsync((void *)P.pose, h_pose, 8 * 77 * (size_t)W, hipMemcpyHostToDevice, s));
      RD_CHECK(c, hipMemcpyAsync((void *)P.ex, h_ex, 8 * 7 * (size_t)W, hipMemcpyHostToDevice, s));
    }
    RD_CHECK(c, hipMemcpyAsync(d_rec, rec_off.data(), sizeof(int) * (W + 1), hipMemcpyHostToDevice, s));
  }
  hipLaunchKernelGGL(k_line_reduce<TAB>, dim3(grid), dim3(RC_THREADS), 0, s, P);
  RD_CHECK(c, hipGetLastError());
#define RD_DOWN(vec, dptr, n) do { vec.resize(std::max<size_t>(n, 1)); if (n) RD_CHECK(c, hipMemcpyAsync(vec.data(), dptr, sizeof(vec[0]) * (n), hipMemcpyDeviceToHost, s)); } while (0)
  if (out->H) RD_DOWN(hH, P.H, n5k);
  if (out->U) RD_DOWN(hU, P.U, n5k);
  if (out->g) RD_DOWN(hg, P.g, n72);
  if (out->bp) RD_DOWN(hbp, P.bp, n72);
  if (out->cost) RD_DOWN(hcost, P.cost, (size_t)W);
  if (out->ms_kernel) RD_DOWN(hms, P.ms, 2 * (size_t)W);
  RD_DOWN(hne, P.n_elig, (size_t)W);
  RD_DOWN(hnf, P.n_failed, (size_t)W);
  if (out->Vinv) RD_DOWN(hV, P.oVinv, N * 16);
  if (out->bl) RD_DOWN(hb, P.obl, N * 4);
  if (out->W) RD_DOWN(hW, P.oW, N * RC_WROW);
  if (out->failed) RD_DOWN(hf, P.ofailed, N);
  if (out->V) RD_DOWN(hVl, P.oV, N * 10);
#undef RD_DOWN
  RD_CHECK(c, hipStreamSynchronize(s));
  // (outputs are written only once the whole call has succeeded)
  if (out->H) std::memcpy(out->H, hH.data(), 8 * n5k);
  if (out->U) std::memcpy(out->U, hU.data(), 8 * n5k);
  if (out->g) std::memcpy(out->g, hg.data(), 8 * n72);
  if (out->bp) std::memcpy(out->bp, hbp.data(), 8 * n72);
  if (out->cost) std::memcpy(out->cost, hcost.data(), 8 * (size_t)W);
  if (out->ms_kernel) std::memcpy(out->ms_kernel, hms.data(), 16 * (size_t)W);
  if (out->n_eligible) std::memcpy(out->n_eligible, hne.data(), 4 * (size_t)W);
  if (out->n_failed) std::memcpy(out->n_failed, hnf.data(), 4 * (size_t)W);
  if (rec) {       // the records of a window's eligible lines, concatenated
    size_t o = 0;
    for (int w = 0; w < W; w++) {
      const size_t n = (size_t)hne[w], from = (size_t)rec_off[w];
      if (out->Vinv && n) std::memcpy(out->Vinv + o * 16, hV.data() + from * 16, 8 * n * 16);
      if (out->bl && n) std::memcpy(out->bl + o * 4, hb.data() + from * 4, 8 * n * 4);
      if (out->W && n) std::memcpy(out->W + o * RC_WROW, hW.data() + from * RC_WROW, 8 * n * RC_WROW);
      if (out->failed && n) std::memcpy(out->failed + o, hf.data() + from, n);
      if (out->V && n) std::memcpy(out->V + o * 10, hVl.data() + from * 10, 8 * n * 10);
      o += n;
    }
  }
  if (keep) {
    keep->rec_Vinv = P.oVinv; keep->rec_bl = P.obl; keep->rec_W = P.oW; keep->rec_V = P.oV; keep->rec_failed = P.ofailed; keep->rec_off_d = k_off;
    keep->rec_off = rec_off; keep->rec_ne.assign(hne.begin(), hne.end());
    keep->rec_pose.assign(h_pose, h_pose + 77 * (size_t)W);
    keep->rec_pose.insert(keep->rec_pose.end(), h_ex, h_ex + 7 * (size_t)W);
    keep->rec_mu = P.mu; keep->rec_gen = keep->gen; keep->rec_valid = true;
  }
done:
  if (d && !cache.d) (void)hipFree(d);
  return st;
}

}  // namespace

extern "C" gfbe_status gfbe_line_reduce(gfbe_ctx *c, int32_t n_windows, const gfbe_line_window *const *win, int32_t mode, double sqrt_info,
                                        double huber_width, double mu, gfbe_line_reduced *out) {
  if (!c || n_windows < 0 || (n_windows > 0 && !win)) return GFBE_BAD_INPUT;
  if (!reduce_args_ok(c, "gfbe_line_reduce", mode, mu, out)) return GFBE_BAD_INPUT;
  const gfbe_line_reduced full = reduced_full(out);
  // the windows: sizes, frames and pointers (the checks of gfbe_line_refine; observation VALUES are not looked at)
  std::vector<int> line_off(n_windows + 1, 0), nlines(n_windows, 0);
  size_t n_obs_total = 0;
  for (int w = 0; w < n_windows; w++) {
    const gfbe_line_window *L = win[w];
    if (!L || L->struct_size != (int32_t)sizeof(gfbe_line_window)) { ctx_set_error(c, "gfbe_line_reduce: gfbe_line_window ABI mismatch"); return GFBE_BAD_INPUT; }
    if (L->n_lines < 0 || (L->n_lines > 0 && (!L->start_frame || !L->n_obs || !L->is_triangulation || !L->line_plucker))) return GFBE_BAD_INPUT;
    size_t no = 0;
    for (int i = 0; i < L->n_lines; i++) {
      const int s = L->start_frame[i], k = L->n_obs[i];
      if (s < 0 || k < 0 || s + k > GFBE_NFRAMES) { ctx_set_error(c, "gfbe_line_reduce: a line's observations run past the window"); return GFBE_BAD_INPUT; }
      no += (size_t)k;
    }
    if (no > 0 && !L->obs) return GFBE_BAD_INPUT;
    if ((size_t)line_off[w] + (size_t)L->n_lines > (size_t)INT32_MAX / 512 || n_obs_total + no > (size_t)INT32_MAX / 8) return GFBE_BAD_INPUT;
    line_off[w + 1] = line_off[w] + L->n_lines;
    nlines[w] = L->n_lines;
    n_obs_total += no;
  }
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_line_reduce: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (n_windows == 0) return GFBE_OK;
  const int n_lines = line_off[n_windows];
  // pack as gfbe_line_refine does: ints (line_off, obs_off, start), doubles (plucker, obs, poses, extrinsics), the triangulation flags
  std::vector<int> ints((size_t)n_windows + 1 + 2 * (size_t)n_lines + 1);
  int *h_line_off = ints.data(), *h_obs_off = h_line_off + n_windows + 1, *h_start = h_obs_off + n_lines + 1;
  std::vector<double> dbl((size_t)6 * n_lines + 4 * n_obs_total + 84 * (size_t)n_windows);
  double *h_plk = dbl.data(), *h_obs = h_plk + 6 * (size_t)n_lines, *h_pose = h_obs + 4 * n_obs_total, *h_ex = h_pose + 77 * (size_t)n_windows;
  std::vector<unsigned char> h_tri(std::max(n_lines, 1));
  {
    size_t o = 0;
    for (int w = 0; w < n_windows; w++) {
      const gfbe_line_window *L = win[w];
      h_line_off[w] = line_off[w];
      std::memcpy(h_pose + 77 * (size_t)w, L->pose, sizeof(double) * 77);
      std::memcpy(h_ex + 7 * (size_t)w, L->ex_cam, sizeof(double) * 7);
      size_t lo = 0;
      for (int i = 0; i < L->n_lines; i++) {
        const int l = line_off[w] + i;
        h_obs_off[l] = (int)o; h_start[l] = L->start_frame[i]; h_tri[l] = L->is_triangulation[i] ? 1 : 0;
        std::memcpy(h_plk + 6 * (size_t)l, L->line_plucker + 6 * (size_t)i, sizeof(double) * 6);
        if (L->n_obs[i] > 0) std::memcpy(h_obs + 4 * o, L->obs + 4 * lo, sizeof(double) * 4 * L->n_obs[i]);
        o += L->n_obs[i]; lo += L->n_obs[i];
      }
    }
    h_line_off[n_windows] = n_lines;
    h_obs_off[n_lines] = (int)o;
  }
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  char *d = nullptr;
  const size_t b_int = sizeof(int) * ints.size(), b_dbl = sizeof(double) * dbl.size(), b_tri = h_tri.size();
  auto up8 = [](size_t b) { return (b + 255) & ~(size_t)255; };
  ReduceBatch P{};
  RD_CHECK(c, hipMalloc((void **)&d, up8(b_int) + up8(b_dbl) + up8(b_tri)));
  {
    int *d_int = (int *)d;
    double *d_dbl = (double *)(d + up8(b_int));
    unsigned char *d_tri = (unsigned char *)(d + up8(b_int) + up8(b_dbl));
    P.line_off = d_int; P.obs_off = d_int + (h_obs_off - h_line_off); P.start = d_int + (h_start - h_line_off);
    P.plk_in = d_dbl; P.obs = d_dbl + (h_obs - h_plk); P.pose = d_dbl + (h_pose - h_plk); P.ex = d_dbl + (h_ex - h_plk);
    P.tri = d_tri;
    P.sqrt_info = sqrt_info; P.huber = huber_width; P.mu = mu; P.mode = mode;
    RD_CHECK(c, hipMemcpyAsync(d_int, ints.data(), b_int, hipMemcpyHostToDevice, s));
    RD_CHECK(c, hipMemcpyAsync(d_dbl, dbl.data(), b_dbl, hipMemcpyHostToDevice, s));
    RD_CHECK(c, hipMemcpyAsync(d_tri, h_tri.data(), b_tri, hipMemcpyHostToDevice, s));
  }
  st = reduce_run<false>(c, P, n_windows, nlines, &full, nullptr, nullptr, ReduceCache{nullptr, nullptr});     // (synchronises the stream: the packed host buffers stay alive until then)
done:
  if (d) { (void)hipStreamSynchronize(s); (void)hipFree(d); }
  return st;
}

extern "C" gfbe_status gfbe_ltab_reduce(gfbe_ctx *c, gfbe_ltab *t, int32_t mode, const double *pose7, const double *ex_cam, double sqrt_info,
                                        double huber_width, double mu, gfbe_line_reduced *out) {
  if (!c) return GFBE_BAD_INPUT;
  if (!reduce_args_ok(c, "gfbe_ltab_reduce", mode, mu, out)) return GFBE_BAD_INPUT;
  const gfbe_line_reduced full = reduced_full(out);
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_ltab_reduce: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (!t || !pose7 || !ex_cam) return GFBE_BAD_INPUT;
  const int W = t->d.W, b = t->cur;
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  std::vector<int> nlines(W);
  ReduceBatch P{};
  // the tables' sizes (the record slots and the scratch slab) come down first: the one wait of the call besides the results'
  RD_CHECK(c, hipMemcpyAsync(nlines.data(), t->d.count, sizeof(int) * W, hipMemcpyDeviceToHost, s));
  RD_CHECK(c, hipStreamSynchronize(s));
  P.count = t->d.count; P.nobs = t->d.nobs[b]; P.F = t->d.F; P.start = t->d.start[b]; P.tri = t->d.tri[b]; P.plk_in = t->d.plk[b];
  P.obs = t->d.obs[b];
  P.sqrt_info = sqrt_info; P.huber = huber_width; P.mu = mu; P.mode = mode;
  st = reduce_run<true>(c, P, W, nlines, &full, pose7, ex_cam, ReduceCache{&t->reduce_d, &t->reduce_cap},
                        t->keep_records && mode == GFBE_LINE_REDUCE_SOLVE ? t : nullptr);
done:
  return st;
}
