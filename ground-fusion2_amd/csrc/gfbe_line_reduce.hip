// gfbe_line_reduce.hip — reduced normal equations of a window's line factors: the line loops of optimizationwithLine()
// (estimator/estimator.cpp:4566-4598 solve, :4736-4771 MARGIN_OLD), linearised with respect to the poses, the camera extrinsic and the
// lines, the 4 x 4 line blocks eliminated (include/gfbe.h: gfbe_line_reduce / gfbe_ltab_reduce):
//
//     H = U - sum_l W_l V'_l^-1 W_l^T,  g = bp - sum_l W_l V'_l^-1 bl      on the 72 dims [pose 0 .. pose 10 | ex_cam]
//
// Shape: ONE WORKGROUP PER WINDOW AT A TIME (a workgroup walks windows blockIdx.x, blockIdx.x + gridDim.x, ...; its scratch slab is
// its own, so a window's bits do not depend on the batch). Per window:
//   rank    the eligible lines in list order (line_rank, gfbe_line.h), rank -> line
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
#include "gfbe_line_batch.h"

using namespace gfd;

namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));

enum { RC_THREADS = 256, RC_WAVES = 4, RC_CHUNK = 8, RC_LD = 80, RC_NP = LINE_NP, RC_NT = 15, RC_TASKS = GFBE_NFRAMES * 90,
       RC_TPT = (RC_TASKS + RC_THREADS - 1) / RC_THREADS, RC_MAX_GRID = 256,
       RC_STAGE = 2 * RC_CHUNK * 4 * RC_LD,        // doubles: Y and W of a chunk; reused for the 15 tiles + the frame sums at the end
       RC_WROW = RC_NP * 4, RC_JROW = GFBE_NFRAMES * LINE_JREC };
static_assert(RC_NT * 256 + RC_TASKS <= RC_STAGE, "the finish phase reuses the chunk staging area");

struct ReduceBatch {
  LineList L;                          // the lines: host-fed CSR or the tables in place (gfbe_line.h)
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

// the lines that enter: line_eligible (gfbe_line.h), and in MARG_OLD mode only those that start in frame 0
template <bool TAB>
__device__ __forceinline__ bool rb_eligible(const ReduceBatch &P, int l) {
  return line_eligible<TAB>(P.L, l) && (P.mode == GFBE_LINE_REDUCE_SOLVE || P.L.start[l] == 0);
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

template <bool TAB>
__global__ __launch_bounds__(RC_THREADS) void k_line_reduce(ReduceBatch P) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4;
  const LineList &L = P.L;
  __shared__ LineRT Bs[GFBE_NFRAMES], Cw[GFBE_NFRAMES];
  __shared__ LineRT Ex;
  __shared__ double stage[RC_STAGE];
  __shared__ double sJ[RC_CHUNK * RC_JROW];
  __shared__ double sbl[RC_CHUNK][4];
  __shared__ int smeta[RC_CHUNK][3];           // start, first observation, observations (0: the line is not in the sums)
  __shared__ double sh[2 * RC_WAVES];
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
    int l0, l1;
    line_range<TAB>(L, w, &l0, &l1);
    __syncthreads();                               // (the previous window's readers of LDS are done)
    line_stage_poses(L, w, Bs, &Ex);
    for (int q = t; q < RC_STAGE; q += RC_THREADS) stage[q] = 0.0;      // (rows 72..79 of every operand stay zero)
    __syncthreads();
    line_stage_cameras(Bs, Ex, Cw);
    // ---- rank: eligible lines in list order
    const int n_elig = line_rank<RC_THREADS>(l0, l1, [&](int l) { return rb_eligible<TAB>(P, l); }, lineof, scan_lds);
    __threadfence();
    __syncthreads();
    // ---- lines
    double csum = 0.0, nfail = 0.0;
    for (int q = t; q < n_elig; q += RC_THREADS) {
      const int l = lineof[q], s = L.start[l];
      double lw[6], x[4], c;
      line_plk_to_pose(L.plk_in + 6 * (size_t)l, Cw[s].R, Cw[s].t, lw);     // para_LineFeature = plk_to_orth(plk_to_pose(line_plucker, Rwc, twc))
      line_plk_to_orth(lw, x);
      const bool ok = line_reduce_line(Bs, Ex, x, s, k0, line_nobs<TAB>(L, l), line_obs<TAB>(L, l), P.sqrt_info, P.huber, P.mu,
                                       Wrow + (size_t)q * RC_WROW, Jrec + (size_t)q * RC_JROW, Vinv + (size_t)q * 16, bl + (size_t)q * 4, &c,
                                       Vl + (size_t)q * 10);
      failed[q] = ok ? 0 : 1;
      if (ok) csum += c; else nfail += 1.0;
    }
    __threadfence();
    double red[2] = {csum, nfail};                 // the window's cost and failure count: fixed-order sums (line_block_reduce, gfbe_line.h)
    line_block_reduce<2, RC_WAVES>(red, 0u, sh);
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
        smeta[t][0] = in ? L.start[l] : 0; smeta[t][1] = k0; smeta[t][2] = in ? line_nobs<TAB>(L, l) : 0;
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
// slots). h_pose / h_ex (table-fed): the poses on the host, copied into the call's allocation. kept (table-fed): the table handle's
// scratch allocation, kept between calls and grown on demand — a per-frame caller pays no hipMalloc / hipFree; without it the
// allocation lives for the call (the host-fed entry point, as gfbe_line_refine). keep (table-fed, solve mode, gfbe_ltab_keep_records on):
// the per-line records are written into the store on the table handle instead of the call's allocation — the same values from the same
// kernel, so the call's outputs keep their bits — and stay there for gfbe_ltab_step.
template <bool TAB>
gfbe_status reduce_run(gfbe_ctx *c, ReduceBatch P, int W, const std::vector<int> &nlines, const gfbe_line_reduced *out, const double *h_pose,
                       const double *h_ex, DevBuf *kept, gfbe_ltab *keep = nullptr) {
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  std::vector<int> rec_off(W + 1, 0);
  int maxl = 0;
  for (int w = 0; w < W; w++) { rec_off[w + 1] = rec_off[w] + nlines[w]; maxl = std::max(maxl, nlines[w]); }
  const size_t N = (size_t)rec_off[W], n72 = (size_t)W * RC_NP, n5k = n72 * RC_NP;
  const int grid = std::min(W, (int)RC_MAX_GRID);
  const size_t slab_lines = (size_t)maxl + RC_CHUNK, S = (size_t)grid * slab_lines;
  const bool rec = out->Vinv || out->bl || out->W || out->failed || out->V;
  DevBuf own, &buf = kept ? *kept : own;
  std::vector<double> hH, hU, hg, hbp, hcost, hms, hV, hb, hW, hVl;
  std::vector<int> hne(W), hnf(W);
  std::vector<unsigned char> hf;
  // the call's one device allocation
  int *d_rec = nullptr;
  auto layout = [&](char *base) {
    Arena a(base);
    d_rec = a.take<int>(W + 1);
    P.rec_off = d_rec;
    if (h_pose) { P.L.pose = a.take<double>(77 * (size_t)W); P.L.ex = a.take<double>(7 * (size_t)W); }
    P.lineof = a.take<int>(S);
    P.Wrow = a.take<double>(S * RC_WROW); P.Jrec = a.take<double>(S * RC_JROW);
    P.Vinv = a.take<double>(S * 16); P.bl = a.take<double>(S * 4); P.Vl = a.take<double>(S * 10); P.failed = a.take<unsigned char>(S);
    P.H = out->H ? a.take<double>(n5k) : nullptr; P.U = out->U ? a.take<double>(n5k) : nullptr;
    P.g = a.take<double>(n72); P.bp = a.take<double>(n72);
    P.cost = a.take<double>(W); P.ms = out->ms_kernel ? a.take<double>(2 * (size_t)W) : nullptr;
    P.n_elig = a.take<int>(W); P.n_failed = a.take<int>(W);
    if (rec && !keep) {
      P.oVinv = out->Vinv ? a.take<double>(N * 16) : nullptr; P.obl = out->bl ? a.take<double>(N * 4) : nullptr;
      P.oW = out->W ? a.take<double>(N * RC_WROW) : nullptr; P.oV = out->V ? a.take<double>(N * 10) : nullptr;
      P.ofailed = a.take<unsigned char>(N + 1);
    }
    return a.off;
  };
  // the store on the table handle: rec_off, then every record array at full size
  int *k_off = nullptr;
  auto keep_layout = [&](char *base) {
    Arena a(base);
    k_off = a.take<int>(W + 1);
    P.oVinv = a.take<double>(N * 16); P.obl = a.take<double>(N * 4); P.oW = a.take<double>(N * RC_WROW);
    P.oV = a.take<double>(N * 10); P.ofailed = a.take<unsigned char>(N + 1);
    return a.off;
  };
  GFBE_CHECK_DONE(c, lay_out(s, buf, layout));
  if (keep) {
    keep->rec_valid = false; keep->cand_valid = false;
    GFBE_CHECK_DONE(c, lay_out(s, keep->rec_buf, keep_layout));
    GFBE_CHECK_DONE(c, hipMemcpyAsync(k_off, rec_off.data(), sizeof(int) * (W + 1), hipMemcpyHostToDevice, s));
  }
  P.n_windows = W; P.slab_lines = (int)slab_lines;
  if (h_pose) {
    GFBE_CHECK_DONE(c, hipMemcpyAsync((void *)P.L.pose, h_pose, 8 * 77 * (size_t)W, hipMemcpyHostToDevice, s));
    GFBE_CHECK_DONE(c, hipMemcpyAsync((void *)P.L.ex, h_ex, 8 * 7 * (size_t)W, hipMemcpyHostToDevice, s));
  }
  GFBE_CHECK_DONE(c, hipMemcpyAsync(d_rec, rec_off.data(), sizeof(int) * (W + 1), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_line_reduce<TAB>, dim3(grid), dim3(RC_THREADS), 0, s, P);
  GFBE_CHECK_DONE(c, hipGetLastError());
  if (out->H) GFBE_CHECK_DONE(c, download(hH, P.H, n5k, s));
  if (out->U) GFBE_CHECK_DONE(c, download(hU, P.U, n5k, s));
  if (out->g) GFBE_CHECK_DONE(c, download(hg, P.g, n72, s));
  if (out->bp) GFBE_CHECK_DONE(c, download(hbp, P.bp, n72, s));
  if (out->cost) GFBE_CHECK_DONE(c, download(hcost, P.cost, (size_t)W, s));
  if (out->ms_kernel) GFBE_CHECK_DONE(c, download(hms, P.ms, 2 * (size_t)W, s));
  GFBE_CHECK_DONE(c, download(hne, P.n_elig, (size_t)W, s));
  GFBE_CHECK_DONE(c, download(hnf, P.n_failed, (size_t)W, s));
  if (out->Vinv) GFBE_CHECK_DONE(c, download(hV, P.oVinv, N * 16, s));
  if (out->bl) GFBE_CHECK_DONE(c, download(hb, P.obl, N * 4, s));
  if (out->W) GFBE_CHECK_DONE(c, download(hW, P.oW, N * RC_WROW, s));
  if (out->failed) GFBE_CHECK_DONE(c, download(hf, P.ofailed, N, s));
  if (out->V) GFBE_CHECK_DONE(c, download(hVl, P.oV, N * 10, s));
  GFBE_CHECK_DONE(c, hipStreamSynchronize(s));
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
  if (own.d) (void)hipFree(own.d);
  return st;
}

}  // namespace

extern "C" gfbe_status gfbe_line_reduce(gfbe_ctx *c, int32_t n_windows, const gfbe_line_window *const *win, int32_t mode, double sqrt_info,
                                        double huber_width, double mu, gfbe_line_reduced *out) {
  if (!c || n_windows < 0 || (n_windows > 0 && !win)) return GFBE_BAD_INPUT;
  if (!reduce_args_ok(c, "gfbe_line_reduce", mode, mu, out)) return GFBE_BAD_INPUT;
  const gfbe_line_reduced full = reduced_full(out);
  LineWindows B;
  if (!check_line_windows(c, "gfbe_line_reduce", n_windows, win, (size_t)INT32_MAX / 512, B)) return GFBE_BAD_INPUT;
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_line_reduce: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (n_windows == 0) return GFBE_OK;
  std::vector<int> nlines(n_windows);
  for (int w = 0; w < n_windows; w++) nlines[w] = B.line_off[w + 1] - B.line_off[w];
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  LineUpload U;
  ReduceBatch P{};
  GFBE_CHECK_DONE(c, upload_line_windows(s, n_windows, win, B, 0, U));
  P.L = U.L; P.sqrt_info = sqrt_info; P.huber = huber_width; P.mu = mu; P.mode = mode;
  st = reduce_run<false>(c, P, n_windows, nlines, &full, nullptr, nullptr, nullptr);     // (synchronises the stream: the packed host buffers stay alive until then)
done:
  if (U.d) { (void)hipStreamSynchronize(s); (void)hipFree(U.d); }
  return st;
}

extern "C" gfbe_status gfbe_ltab_reduce(gfbe_ctx *c, gfbe_ltab *t, int32_t mode, const double *pose7, const double *ex_cam, double sqrt_info,
                                        double huber_width, double mu, gfbe_line_reduced *out) {
  if (!c) return GFBE_BAD_INPUT;
  if (!reduce_args_ok(c, "gfbe_ltab_reduce", mode, mu, out)) return GFBE_BAD_INPUT;
  const gfbe_line_reduced full = reduced_full(out);
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_ltab_reduce: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (!t || !pose7 || !ex_cam) return GFBE_BAD_INPUT;
  const int W = t->d.W;
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  std::vector<int> nlines(W);
  ReduceBatch P{};
  // the tables' sizes (the record slots and the scratch slab) come down first: the one wait of the call besides the results'
  GFBE_CHECK_DONE(c, hipMemcpyAsync(nlines.data(), t->d.count, sizeof(int) * W, hipMemcpyDeviceToHost, s));
  GFBE_CHECK_DONE(c, hipStreamSynchronize(s));
  P.L = ltab_line_list(*t, nullptr, nullptr);      // (reduce_run copies the poses up)
  P.sqrt_info = sqrt_info; P.huber = huber_width; P.mu = mu; P.mode = mode;
  st = reduce_run<true>(c, P, W, nlines, &full, pose7, ex_cam, &t->reduce_buf,
                        t->keep_records && mode == GFBE_LINE_REDUCE_SOLVE ? t : nullptr);
done:
  return st;
}
