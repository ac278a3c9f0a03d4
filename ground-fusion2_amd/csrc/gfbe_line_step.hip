// gfbe_line_step.hip — the step half of a joint trust-region iteration over a window's line blocks (include/gfbe.h: gfbe_line_step,
// gfbe_ltab_keep_records / gfbe_ltab_step / gfbe_ltab_commit): back-substitution, the line blocks' shares of the
// dogleg scalars, the step, the candidate lines / poses and the candidate line cost, and the commit of an accepted candidate into the
// line tables. The model is the scalar landmark code of the window solve (k_lm_step's shares, k_step's three-branch rule restated in
// line_dogleg, k_candidate), generalised to 4-dimensional blocks in the coordinates of gfbe_line_reduce (gfbe_line.h).
//
// Shape: ONE WORKGROUP PER WINDOW AT A TIME (a workgroup walks windows blockIdx.x, blockIdx.x + gridDim.x, ...); thread t owns the
// entering lines t, t + 256, ... Per window:
//   rank     the entering lines in list order (line_rank, gfbe_line.h: the rank k_line_reduce takes): record q belongs to the q-th of them
//   phase 1  y_p, v_p staged in LDS; a thread streams its line's W (288 doubles) ONCE for both W^T y_p and W^T v_p, forms y_l, v_l and
//            the eight shares (line_step_shares); vector ALU work: the right-hand side is two columns wide, a 16-wide matrix-core tile
//            would be 7/8 padding. The shares go through line_block_reduce (gfbe_line.h: wave shuffle tree, then the waves
//            in order through LDS); every thread adds `rest` and takes the same dogleg branch from the broadcast totals
//   phase 2  threads 0..11 form the candidate poses / extrinsic with the device's pose_plus; a thread forms its lines' candidates and
//            their cost (line_factor without Jacobians + line_huber) and the candidate Plücker vector in the candidate start camera
// No atomics, no grid barrier; FP64 throughout; a window's bits do not depend on the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"
#include "gfbe_factors.h"
#include "gfbe_line.h"
#include "gfbe_line_batch.h"
#include "gfbe_tabstage.h"

using namespace gfd;

namespace {

enum { LS_THREADS = 256, LS_WAVES = 4, LS_NP = LINE_NP, LS_WROW = LINE_NP * 4, LS_MAX_GRID = 1024 };
#define LS_COST_INVALID 1.7976931348623157e308

struct StepBatch {
  LineList L;                          // the lines: host-fed CSR or the tables in place (gfbe_line.h)
  double sqrt_info, huber;
  int n_windows;
  const int *rec_off;                  // [n_windows + 1] first record slot of a window
  // the records of the reduce, per slot
  const double *Vinv, *bl, *W, *V;
  const unsigned char *failed;
  // per window: the caller's directions and scalars
  const double *yp, *vp, *rest, *radius;
  // per record slot
  int *lineof;
  double *yl, *vl, *xc, *plkc;
  // per window
  double *gram, *total, *coef, *pose_c, *ex_c, *cost, *ms;
  unsigned char *invalid;
  int *n_elig;
};

template <bool TAB>
__global__ __launch_bounds__(LS_THREADS) void k_line_step(StepBatch P) {
  const int t = threadIdx.x;
  const LineList &L = P.L;
  __shared__ LineRT Bs[GFBE_NFRAMES], Cw[GFBE_NFRAMES], Bc[GFBE_NFRAMES], Cc[GFBE_NFRAMES];
  __shared__ LineRT Ex, Exc;
  __shared__ double syp[LS_NP], svp[LS_NP];
  __shared__ double sh[8 * LS_WAVES];
  __shared__ int scan_lds[20];
  for (int w = blockIdx.x; w < P.n_windows; w += gridDim.x) {
    const uint64_t t_start = P.ms ? wall_clock64() : 0;
    int l0, l1;
    line_range<TAB>(L, w, &l0, &l1);
    const size_t ro = (size_t)P.rec_off[w];
    const int cap = P.rec_off[w + 1] - P.rec_off[w];       // record slots of this window: nothing is written past them
    const double *pose = L.pose + (size_t)w * 77, *ex = L.ex + (size_t)w * 7;
    __syncthreads();                               // (the previous window's readers of LDS are done)
    line_stage_poses(L, w, Bs, &Ex);
    if (t >= 64 && t < 64 + LS_NP) { syp[t - 64] = P.yp[(size_t)w * LS_NP + t - 64]; svp[t - 64] = P.vp[(size_t)w * LS_NP + t - 64]; }
    __syncthreads();
    line_stage_cameras(Bs, Ex, Cw);
    // ---- rank: the entering lines in list order (the predicate of gfbe_line_reduce in solve mode)
    int *lineof = P.lineof + ro;
    const int n_elig = line_rank<LS_THREADS>(l0, l1, [&](int l) { return line_eligible<TAB>(L, l); }, lineof, scan_lds, cap);
    __threadfence();
    __syncthreads();
    // ---- phase 1: back-substitution and the shares
    double p[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = t; q < n_elig; q += LS_THREADS) {
      const size_t slot = ro + q;
      const int l = lineof[q], s = L.start[l];
      double lw[6], x[4], yl[4] = {0.0, 0.0, 0.0, 0.0}, vl[4] = {0.0, 0.0, 0.0, 0.0};
      line_plk_to_pose(L.plk_in + 6 * (size_t)l, Cw[s].R, Cw[s].t, lw);     // getLineOrthVector, as the reduce formed it
      line_plk_to_orth(lw, x);
      if (!P.failed[slot]) {
        double sp[8];
        line_step_shares(P.W + slot * LS_WROW, P.Vinv + slot * 16, P.bl + slot * 4, P.V + slot * 10, syp, svp, x, yl, vl, sp);
#pragma unroll
        for (int k = 0; k < 8; k++) p[k] = (k == 6) ? fmax(p[k], sp[k]) : p[k] + sp[k];
      }
      for (int a = 0; a < 4; a++) { P.yl[slot * 4 + a] = yl[a]; P.vl[slot * 4 + a] = vl[a]; P.xc[slot * 4 + a] = x[a]; }
    }
    line_block_reduce<8, LS_WAVES>(p, 1u << 6, sh);      // (fixed order; entry 6 is a maximum)
    double tot[8], coef[4];
    const double *rest = P.rest + (size_t)w * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) tot[k] = (k == 6) ? fmax(rest[k], p[k]) : rest[k] + p[k];
    line_dogleg(tot, P.radius[w], coef);
    const bool invalid = !(coef[3] > 0.0);         // TrustRegionMinimizer::HandleInvalidStep: the caller raises mu and reduces again
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < 8; k++) { P.gram[(size_t)w * 8 + k] = p[k]; P.total[(size_t)w * 8 + k] = tot[k]; }
#pragma unroll
      for (int k = 0; k < 4; k++) P.coef[(size_t)w * 4 + k] = coef[k];
    }
    // ---- phase 2: the candidates and their cost
    double csum = 0.0;
    if (invalid) {                                 // no candidate is formed: every candidate array holds its input
      if (t < GFBE_NFRAMES) for (int a = 0; a < 7; a++) P.pose_c[(size_t)w * 77 + 7 * t + a] = pose[7 * t + a];
      if (t == GFBE_NFRAMES) for (int a = 0; a < 7; a++) P.ex_c[(size_t)w * 7 + a] = ex[a];
      for (int q = t; q < n_elig; q += LS_THREADS) {
        const int l = lineof[q];
        for (int a = 0; a < 6; a++) P.plkc[(ro + q) * 6 + a] = L.plk_in[6 * (size_t)l + a];
      }
    } else {
      if (t <= GFBE_NFRAMES) {                     // candidate poses / extrinsic = pose_plus(., c1 v_p + c2 y_p)
        const double *src = t < GFBE_NFRAMES ? pose + 7 * t : ex;
        double d6[6], y7[7];
        for (int k = 0; k < 6; k++) d6[k] = coef[0] * svp[6 * t + k] + coef[1] * syp[6 * t + k];
        pose_plus(src, d6, nullptr, y7);
        double *dst = t < GFBE_NFRAMES ? P.pose_c + (size_t)w * 77 + 7 * t : P.ex_c + (size_t)w * 7;
        for (int a = 0; a < 7; a++) dst[a] = y7[a];
        if (t < GFBE_NFRAMES) Bc[t] = line_make_pose(y7); else Exc = line_make_pose(y7);
      }
      __syncthreads();
      line_stage_cameras(Bc, Exc, Cc);
      __syncthreads();
      for (int q = t; q < n_elig; q += LS_THREADS) {
        const size_t slot = ro + q;
        const int l = lineof[q], s = L.start[l];
        if (P.failed[slot]) {                      // a failed line takes part in nothing: its candidate is its input, bit for bit
          for (int a = 0; a < 6; a++) P.plkc[slot * 6 + a] = L.plk_in[6 * (size_t)l + a];
          continue;
        }
        double x[4], yl[4], vl[4], xc[4], plk[6];
        for (int a = 0; a < 4; a++) { x[a] = P.xc[slot * 4 + a]; yl[a] = P.yl[slot * 4 + a]; vl[a] = P.vl[slot * 4 + a]; }   // (this thread's own stores)
        csum += line_step_candidate(Bc, Exc, Cc[s], x, yl, vl, coef[0], coef[1], s, line_nobs<TAB>(L, l), line_obs<TAB>(L, l), P.sqrt_info,
                                    P.huber, xc, plk);
        for (int a = 0; a < 4; a++) P.xc[slot * 4 + a] = xc[a];
        for (int a = 0; a < 6; a++) P.plkc[slot * 6 + a] = plk[a];
      }
    }
    double c1[1] = {csum};
    line_block_reduce<1, LS_WAVES>(c1, 0u, sh);
    if (t == 0) {
      P.cost[w] = invalid ? LS_COST_INVALID : c1[0];
      P.invalid[w] = invalid ? 1 : 0;
      P.n_elig[w] = n_elig;
      if (P.ms) P.ms[w] = (double)(wall_clock64() - t_start) * 1e-5;      // (100 MHz device wall clock)
    }
  }
}

// gfbe_ltab_commit: the tables with accept != 0 take the candidate Plücker vectors of their entering, non-failed lines
__global__ __launch_bounds__(256) void k_line_commit(double *plk, const unsigned char *accept, const int *rec_off, const int *ne, const int *lineof,
                                                     const unsigned char *failed, const double *plkc) {
  const int w = blockIdx.x;
  if (!accept[w]) return;
  const size_t ro = (size_t)rec_off[w];
  const int n = min(ne[w], rec_off[w + 1] - rec_off[w]);
  for (int i = threadIdx.x; i < n * 6; i += 256) {
    const int q = i / 6, a = i - 6 * q;
    if (failed[ro + q]) continue;
    plk[6 * (size_t)lineof[ro + q] + a] = plkc[(ro + q) * 6 + a];
  }
}

bool all_finite(const double *p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}
bool stepped_ok(gfbe_ctx *c, const char *who, const gfbe_line_stepped *out) {
  if (!out || out->struct_size != (int32_t)sizeof(gfbe_line_stepped)) { ctx_set_error(c, (std::string(who) + ": gfbe_line_stepped ABI mismatch").c_str()); return false; }
  return true;
}
// y_p, v_p [W][72], rest [W][8], radius [W]
bool step_inputs_ok(gfbe_ctx *c, const char *who, int W, const double *yp, const double *vp, const double *rest, const double *radius) {
  if (W == 0) return true;
  if (!yp || !vp || !rest || !radius) return false;
  if (!all_finite(yp, (size_t)W * LS_NP) || !all_finite(vp, (size_t)W * LS_NP) || !all_finite(rest, (size_t)W * 8)) {
    ctx_set_error(c, (std::string(who) + ": y_p, v_p and rest must be finite").c_str());
    return false;
  }
  for (int w = 0; w < W; w++)
    if (!(radius[w] >= 0.0) || !std::isfinite(radius[w])) { ctx_set_error(c, (std::string(who) + ": radius must be finite and not negative").c_str()); return false; }
  return true;
}

// Launch and hand-over shared by the two entry points. P: the line inputs and the records on the device; rec_off [W + 1]: the record
// slots; ne [W]: the entering lines of a window (what the reduce reported). h_pose / h_ex, d_rec_off (table-fed): the poses on the host,
// copied into the call's allocation, and the slots already on the device. kept (table-fed): the allocation stays on the table handle —
// it holds the candidates gfbe_ltab_commit reads.
template <bool TAB>
gfbe_status step_run(gfbe_ctx *c, StepBatch P, int W, const std::vector<int> &rec_off, const std::vector<int> &ne, const double *yp,
                     const double *vp, const double *rest, const double *radius, const double *h_pose, const double *h_ex,
                     const int *d_rec_off, gfbe_line_stepped *out, DevBuf *kept, StepBatch *laid = nullptr) {
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  const size_t N = (size_t)rec_off[W], nw = (size_t)W;
  const int grid = std::min(W, (int)LS_MAX_GRID);
  DevBuf own, &buf = kept ? *kept : own;
  double *d_yp = nullptr, *d_vp = nullptr, *d_rest = nullptr, *d_radius = nullptr, *d_pose = nullptr, *d_ex = nullptr;
  int *d_off = nullptr;
  std::vector<double> hgram, htotal, hcoef, hyl, hvl, hxc, hplk, hpose, hex, hcost, hms;
  std::vector<unsigned char> hinv;
  auto layout = [&](char *base) {
    Arena a(base);
    d_yp = a.take<double>(nw * LS_NP); d_vp = a.take<double>(nw * LS_NP); d_rest = a.take<double>(nw * 8); d_radius = a.take<double>(nw);
    if (h_pose) { d_pose = a.take<double>(77 * nw); d_ex = a.take<double>(7 * nw); }
    if (!d_rec_off) d_off = a.take<int>(nw + 1);
    P.lineof = a.take<int>(N + 1);
    P.yl = a.take<double>(N * 4); P.vl = a.take<double>(N * 4); P.xc = a.take<double>(N * 4); P.plkc = a.take<double>(N * 6);
    P.gram = a.take<double>(nw * 8); P.total = a.take<double>(nw * 8); P.coef = a.take<double>(nw * 4);
    P.pose_c = a.take<double>(nw * 77); P.ex_c = a.take<double>(nw * 7); P.cost = a.take<double>(nw);
    P.ms = out->ms_kernel ? a.take<double>(nw) : nullptr;
    P.invalid = a.take<unsigned char>(nw); P.n_elig = a.take<int>(nw);
    return a.off;
  };
  GFBE_CHECK_DONE(c, lay_out(s, buf, layout));
  P.n_windows = W; P.yp = d_yp; P.vp = d_vp; P.rest = d_rest; P.radius = d_radius;
  GFBE_CHECK_DONE(c, hipMemcpyAsync(d_yp, yp, 8 * nw * LS_NP, hipMemcpyHostToDevice, s));
  GFBE_CHECK_DONE(c, hipMemcpyAsync(d_vp, vp, 8 * nw * LS_NP, hipMemcpyHostToDevice, s));
  GFBE_CHECK_DONE(c, hipMemcpyAsync(d_rest, rest, 8 * nw * 8, hipMemcpyHostToDevice, s));
  GFBE_CHECK_DONE(c, hipMemcpyAsync(d_radius, radius, 8 * nw, hipMemcpyHostToDevice, s));
  if (h_pose) {
    P.L.pose = d_pose; P.L.ex = d_ex;
    GFBE_CHECK_DONE(c, hipMemcpyAsync(d_pose, h_pose, 8 * 77 * nw, hipMemcpyHostToDevice, s));
    GFBE_CHECK_DONE(c, hipMemcpyAsync(d_ex, h_ex, 8 * 7 * nw, hipMemcpyHostToDevice, s));
  }
  if (d_rec_off) P.rec_off = d_rec_off;
  else { P.rec_off = d_off; GFBE_CHECK_DONE(c, hipMemcpyAsync(d_off, rec_off.data(), sizeof(int) * (nw + 1), hipMemcpyHostToDevice, s)); }
  if (laid) *laid = P;
  hipLaunchKernelGGL(k_line_step<TAB>, dim3(grid), dim3(LS_THREADS), 0, s, P);
  GFBE_CHECK_DONE(c, hipGetLastError());
  if (out->gram) GFBE_CHECK_DONE(c, download(hgram, P.gram, nw * 8, s));
  if (out->total) GFBE_CHECK_DONE(c, download(htotal, P.total, nw * 8, s));
  if (out->coef) GFBE_CHECK_DONE(c, download(hcoef, P.coef, nw * 4, s));
  if (out->invalid) GFBE_CHECK_DONE(c, download(hinv, P.invalid, nw, s));
  if (out->y_l) GFBE_CHECK_DONE(c, download(hyl, P.yl, N * 4, s));
  if (out->v_l) GFBE_CHECK_DONE(c, download(hvl, P.vl, N * 4, s));
  if (out->orth_cand) GFBE_CHECK_DONE(c, download(hxc, P.xc, N * 4, s));
  if (out->plucker_cand) GFBE_CHECK_DONE(c, download(hplk, P.plkc, N * 6, s));
  if (out->pose_cand) GFBE_CHECK_DONE(c, download(hpose, P.pose_c, nw * 77, s));
  if (out->ex_cand) GFBE_CHECK_DONE(c, download(hex, P.ex_c, nw * 7, s));
  if (out->cost_cand) GFBE_CHECK_DONE(c, download(hcost, P.cost, nw, s));
  if (out->ms_kernel) GFBE_CHECK_DONE(c, download(hms, P.ms, nw, s));
  GFBE_CHECK_DONE(c, hipStreamSynchronize(s));
  // (outputs are written only once the whole call has succeeded)
  if (out->gram) std::memcpy(out->gram, hgram.data(), 8 * nw * 8);
  if (out->total) std::memcpy(out->total, htotal.data(), 8 * nw * 8);
  if (out->coef) std::memcpy(out->coef, hcoef.data(), 8 * nw * 4);
  if (out->invalid) std::memcpy(out->invalid, hinv.data(), nw);
  if (out->pose_cand) std::memcpy(out->pose_cand, hpose.data(), 8 * nw * 77);
  if (out->ex_cand) std::memcpy(out->ex_cand, hex.data(), 8 * nw * 7);
  if (out->cost_cand) std::memcpy(out->cost_cand, hcost.data(), 8 * nw);
  if (out->ms_kernel) std::memcpy(out->ms_kernel, hms.data(), 8 * nw);
  {       // the per-line arrays of a window's entering lines, concatenated
    size_t o = 0;
    for (int w = 0; w < W; w++) {
      const size_t n = (size_t)ne[w], from = (size_t)rec_off[w];
      if (out->y_l && n) std::memcpy(out->y_l + o * 4, hyl.data() + from * 4, 8 * n * 4);
      if (out->v_l && n) std::memcpy(out->v_l + o * 4, hvl.data() + from * 4, 8 * n * 4);
      if (out->orth_cand && n) std::memcpy(out->orth_cand + o * 4, hxc.data() + from * 4, 8 * n * 4);
      if (out->plucker_cand && n) std::memcpy(out->plucker_cand + o * 6, hplk.data() + from * 6, 8 * n * 6);
      o += n;
    }
  }
done:
  if (own.d) { (void)hipStreamSynchronize(s); (void)hipFree(own.d); }
  return st;
}

}  // namespace

extern "C" gfbe_status gfbe_line_step(gfbe_ctx *c, int32_t n_windows, const gfbe_line_window *const *win, const gfbe_line_reduced *rec,
                                      double sqrt_info, double huber_width, double mu, const double *y_p, const double *v_p, const double *rest,
                                      const double *radius, gfbe_line_stepped *out) {
  if (!c || n_windows < 0 || (n_windows > 0 && !win)) return GFBE_BAD_INPUT;
  if (!stepped_ok(c, "gfbe_line_step", out)) return GFBE_BAD_INPUT;
  if (!rec || rec->struct_size != (int32_t)sizeof(gfbe_line_reduced)) {      // (the size without V has no V: a missing record array)
    ctx_set_error(c, "gfbe_line_step: gfbe_line_reduced ABI mismatch (the records need the member V)");
    return GFBE_BAD_INPUT;
  }
  if (!(mu >= 0.0) || !std::isfinite(mu)) return GFBE_BAD_INPUT;
  if (n_windows > 0 && (!rec->Vinv || !rec->bl || !rec->W || !rec->V || !rec->failed || !rec->n_eligible)) {
    ctx_set_error(c, "gfbe_line_step: the records Vinv, bl, W, V, failed and n_eligible are all required");
    return GFBE_BAD_INPUT;
  }
  if (!step_inputs_ok(c, "gfbe_line_step", n_windows, y_p, v_p, rest, radius)) return GFBE_BAD_INPUT;
  // the windows, and the records must be these windows' own
  LineWindows B;
  if (!check_line_windows(c, "gfbe_line_step", n_windows, win, (size_t)INT32_MAX / 512, B)) return GFBE_BAD_INPUT;
  std::vector<int> rec_off(n_windows + 1, 0);
  for (int w = 0; w < n_windows; w++) {
    if (rec->n_eligible[w] != B.entering[w]) { ctx_set_error(c, "gfbe_line_step: n_eligible is not the window's count of entering lines"); return GFBE_BAD_INPUT; }
    rec_off[w + 1] = rec_off[w] + B.entering[w];
  }
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_line_step: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (n_windows == 0) return GFBE_OK;
  const size_t N = (size_t)rec_off[n_windows];
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  LineUpload U;
  StepBatch P{};
  // the records, behind the packed windows in the call's one allocation
  auto layout = [&](char *base) {
    Arena a(base);
    P.Vinv = a.take<double>(N * 16); P.bl = a.take<double>(N * 4); P.W = a.take<double>(N * LS_WROW); P.V = a.take<double>(N * 10);
    P.failed = a.take<unsigned char>(N + 1);
    return a.off;
  };
  GFBE_CHECK_DONE(c, upload_line_windows(s, n_windows, win, B, layout(nullptr), U));
  (void)layout(U.extra);
  P.L = U.L; P.sqrt_info = sqrt_info; P.huber = huber_width;
  if (N) {
    GFBE_CHECK_DONE(c, hipMemcpyAsync((void *)P.Vinv, rec->Vinv, 8 * N * 16, hipMemcpyHostToDevice, s));
    GFBE_CHECK_DONE(c, hipMemcpyAsync((void *)P.bl, rec->bl, 8 * N * 4, hipMemcpyHostToDevice, s));
    GFBE_CHECK_DONE(c, hipMemcpyAsync((void *)P.W, rec->W, 8 * N * LS_WROW, hipMemcpyHostToDevice, s));
    GFBE_CHECK_DONE(c, hipMemcpyAsync((void *)P.V, rec->V, 8 * N * 10, hipMemcpyHostToDevice, s));
    GFBE_CHECK_DONE(c, hipMemcpyAsync((void *)P.failed, rec->failed, N, hipMemcpyHostToDevice, s));
  }
  st = step_run<false>(c, P, n_windows, rec_off, B.entering, y_p, v_p, rest, radius, nullptr, nullptr, nullptr, out, nullptr);   // (synchronises the stream)
done:
  if (U.d) { (void)hipStreamSynchronize(s); (void)hipFree(U.d); }
  return st;
}

extern "C" gfbe_status gfbe_ltab_keep_records(gfbe_ctx *c, gfbe_ltab *t, int32_t on) {
  if (!c) return GFBE_BAD_INPUT;
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_ltab_keep_records: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (!t) return GFBE_BAD_INPUT;
  t->keep_records = on != 0;
  if (!t->keep_records) { t->rec_valid = false; t->cand_valid = false; }
  return GFBE_OK;
}

extern "C" gfbe_status gfbe_ltab_step(gfbe_ctx *c, gfbe_ltab *t, const double *pose7, const double *ex_cam, double sqrt_info, double huber_width,
                                      const double *y_p, const double *v_p, const double *rest, const double *radius, gfbe_line_stepped *out) {
  if (!c) return GFBE_BAD_INPUT;
  if (!stepped_ok(c, "gfbe_ltab_step", out)) return GFBE_BAD_INPUT;
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_ltab_step: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (!t || !pose7 || !ex_cam) return GFBE_BAD_INPUT;
  const int W = t->d.W;
  if (!step_inputs_ok(c, "gfbe_ltab_step", W, y_p, v_p, rest, radius)) return GFBE_BAD_INPUT;
  if (!t->keep_records || !t->rec_valid) { ctx_set_error(c, "gfbe_ltab_step: no records are held (gfbe_ltab_keep_records, then gfbe_ltab_reduce in solve mode)"); return GFBE_BAD_INPUT; }
  if (t->rec_gen != t->gen) { ctx_set_error(c, "gfbe_ltab_step: the tables have changed since the reduce that wrote the records"); return GFBE_BAD_INPUT; }
  if (std::memcmp(t->rec_pose.data(), pose7, 8 * 77 * (size_t)W) != 0 || std::memcmp(t->rec_pose.data() + 77 * (size_t)W, ex_cam, 8 * 7 * (size_t)W) != 0) {
    ctx_set_error(c, "gfbe_ltab_step: pose7 / ex_cam differ from the reduce's");
    return GFBE_BAD_INPUT;
  }
  t->cand_valid = false;
  StepBatch P{};
  P.L = ltab_line_list(*t, nullptr, nullptr);      // (step_run copies the poses up)
  P.Vinv = t->rec_Vinv; P.bl = t->rec_bl; P.W = t->rec_W; P.V = t->rec_V; P.failed = t->rec_failed;
  P.sqrt_info = sqrt_info; P.huber = huber_width;
  StepBatch laid{};
  const gfbe_status st = step_run<true>(c, P, W, t->rec_off, t->rec_ne, y_p, v_p, rest, radius, pose7, ex_cam, t->rec_off_d, out,
                                        &t->step_buf, &laid);
  if (st != GFBE_OK) return st;
  // the candidates stay in the handle's allocation for gfbe_ltab_commit
  t->cand_lineof = laid.lineof; t->cand_plk = laid.plkc; t->cand_ne = laid.n_elig;
  t->cand_valid = true;
  return GFBE_OK;
}

extern "C" gfbe_status gfbe_ltab_commit(gfbe_ctx *c, gfbe_ltab *t, const uint8_t *accept) {
  if (!c) return GFBE_BAD_INPUT;
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_ltab_commit: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (!t || !accept) return GFBE_BAD_INPUT;
  if (!t->cand_valid || !t->rec_valid || t->rec_gen != t->gen) { ctx_set_error(c, "gfbe_ltab_commit: no candidates are held (gfbe_ltab_step first)"); return GFBE_BAD_INPUT; }
  const int W = t->d.W;
  {
    Staged s(c, t, (size_t)W + 8 * 256, /*defer=*/true);
    unsigned char *da = s.up(accept, (size_t)W);
    if (!s.ok) { ctx_set_error(c, "gfbe_ltab_commit: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    s.flush();
    hipLaunchKernelGGL(k_line_commit, dim3(W), dim3(256), 0, ctx_stream(c), t->d.plk[t->cur], da, t->rec_off_d, t->cand_ne, t->cand_lineof,
                       t->rec_failed, t->cand_plk);
  }
  t->gen++;
  t->rec_valid = false; t->cand_valid = false;
  if (hipGetLastError() != hipSuccess) { ctx_set_error(c, "gfbe_ltab_commit: launch failed"); return GFBE_DEVICE_ERROR; }
  return GFBE_OK;
}
