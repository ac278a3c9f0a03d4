// gfbe_line_step.hip — the step half of a joint trust-region iteration over a window's line blocks (include/gfbe.h: gfbe_line_step,
// gfbe_ltab_keep_records / gfbe_ltab_step / gfbe_ltab_commit): back-substitution, the line blocks' shares of the
// dogleg scalars, the step, the candidate lines / poses and the candidate line cost, and the commit of an accepted candidate into the
// line tables. The model is the scalar landmark code of the window solve (k_lm_step's shares, k_step's three-branch rule restated in
// line_dogleg, k_candidate), generalised to 4-dimensional blocks in the coordinates of gfbe_line_reduce (gfbe_line.h).
//
// Shape: ONE WORKGROUP PER WINDOW AT A TIME (a workgroup walks windows blockIdx.x, blockIdx.x + gridDim.x, ...); thread t owns the
// entering lines t, t + 256, ... Per window:
//   rank     the entering lines in list order (block scan), as k_line_reduce ranks them: record q belongs to the q-th of them
//   phase 1  y_p, v_p staged in LDS; a thread streams its line's W (288 doubles) ONCE for both W^T y_p and W^T v_p, forms y_l, v_l and
//            the eight shares (line_step_shares); vector ALU work: the right-hand side is two columns wide, a 16-wide matrix-core tile
//            would be 7/8 padding. The shares go through the fixed-order reduction of k_line_refine (wave shuffle tree, then the waves
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
#include "gfbe_tabstage.h"

using namespace gfd;

namespace {

enum { LS_THREADS = 256, LS_WAVES = 4, LS_NP = LINE_NP, LS_WROW = LINE_NP * 4, LS_MAX_GRID = 1024 };
#define LS_COST_INVALID 1.7976931348623157e308

struct StepBatch {
  // the lines, as ReduceBatch of gfbe_line_reduce.hip: host-fed CSR or the tables in place
  const int *line_off, *obs_off;       // host-fed
  const int *count, *nobs;             // table-fed
  int F;
  const int *start;
  const unsigned char *tri;
  const double *plk_in, *obs, *pose, *ex;
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

// fixed-order reduction of eight per-thread values over the workgroup (wave shuffle tree, then the waves in order); entry 6 is a
// maximum, the others are sums; every thread gets all eight
__device__ void ls_reduce8(double *v, double (*sh)[LS_WAVES]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const double u = __shfl_down(v[k], o, 64);
      v[k] = (k == 6) ? fmax(v[k], u) : v[k] + u;
    }
  if ((t & 63) == 0)
    for (int k = 0; k < 8; k++) sh[k][t >> 6] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; k++) {
    double a = 0.0;
    for (int q = 0; q < LS_WAVES; q++) a = (k == 6) ? fmax(a, sh[k][q]) : a + sh[k][q];
    v[k] = a;
  }
  __syncthreads();
}

template <bool TAB>
__global__ __launch_bounds__(LS_THREADS) void k_line_step(StepBatch P) {
  const int t = threadIdx.x;
  __shared__ LineRT Bs[GFBE_NFRAMES], Cw[GFBE_NFRAMES], Bc[GFBE_NFRAMES], Cc[GFBE_NFRAMES];
  __shared__ LineRT Ex, Exc;
  __shared__ double syp[LS_NP], svp[LS_NP];
  __shared__ double sh[8][LS_WAVES];
  __shared__ int scan_lds[20];
  for (int w = blockIdx.x; w < P.n_windows; w += gridDim.x) {
    const uint64_t t_start = P.ms ? wall_clock64() : 0;
    const int l0 = TAB ? w * P.F : P.line_off[w], l1 = TAB ? l0 + P.count[w] : P.line_off[w + 1];
    const size_t ro = (size_t)P.rec_off[w];
    const int cap = P.rec_off[w + 1] - P.rec_off[w];       // record slots of this window: nothing is written past them
    const double *pose = P.pose + (size_t)w * 77, *ex = P.ex + (size_t)w * 7;
    __syncthreads();                               // (the previous window's readers of LDS are done)
    if (t < GFBE_NFRAMES) Bs[t] = line_make_pose(pose + 7 * t);
    if (t == GFBE_NFRAMES) Ex = line_make_pose(ex);
    if (t >= 64 && t < 64 + LS_NP) { syp[t - 64] = P.yp[(size_t)w * LS_NP + t - 64]; svp[t - 64] = P.vp[(size_t)w * LS_NP + t - 64]; }
    __syncthreads();
    if (t < GFBE_NFRAMES) { Cw[t].R = mul(Bs[t].R, Ex.R); Cw[t].t = add(Bs[t].t, mv(Bs[t].R, Ex.t)); }   // Rwc = Rs ric, twc = Ps + Rs tic
    // ---- rank: the entering lines in list order (the predicate of gfbe_line_reduce in solve mode)
    int *lineof = P.lineof + ro;
    int n_elig = 0;
    for (int c0 = l0; c0 < l1; c0 += LS_THREADS) {
      const int l = c0 + t;
      const int e = (l < l1 && line_eligible<TAB>(P, l)) ? 1 : 0;
      int total;
      const int at = n_elig + block_exclusive_scan<LS_THREADS>(e, &total, scan_lds);
      if (e && at < cap) lineof[at] = l;
      n_elig += total;
    }
    n_elig = min(n_elig, cap);
    __threadfence();
    __syncthreads();
    // ---- phase 1: back-substitution and the shares
    double p[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = t; q < n_elig; q += LS_THREADS) {
      const size_t slot = ro + q;
      const int l = lineof[q], s = P.start[l];
      double lw[6], x[4], yl[4] = {0.0, 0.0, 0.0, 0.0}, vl[4] = {0.0, 0.0, 0.0, 0.0};
      line_plk_to_pose(P.plk_in + 6 * (size_t)l, Cw[s].R, Cw[s].t, lw);     // getLineOrthVector, as the reduce formed it
      line_plk_to_orth(lw, x);
      if (!P.failed[slot]) {
        double sp[8];
        line_step_shares(P.W + slot * LS_WROW, P.Vinv + slot * 16, P.bl + slot * 4, P.V + slot * 10, syp, svp, x, yl, vl, sp);
#pragma unroll
        for (int k = 0; k < 8; k++) p[k] = (k == 6) ? fmax(p[k], sp[k]) : p[k] + sp[k];
      }
      for (int a = 0; a < 4; a++) { P.yl[slot * 4 + a] = yl[a]; P.vl[slot * 4 + a] = vl[a]; P.xc[slot * 4 + a] = x[a]; }
    }
    ls_reduce8(p, sh);
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
        for (int a = 0; a < 6; a++) P.plkc[(ro + q) * 6 + a] = P.plk_in[6 * (size_t)l + a];
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
      if (t < GFBE_NFRAMES) { Cc[t].R = mul(Bc[t].R, Exc.R); Cc[t].t = add(Bc[t].t, mv(Bc[t].R, Exc.t)); }
      __syncthreads();
      for (int q = t; q < n_elig; q += LS_THREADS) {
        const size_t slot = ro + q;
        const int l = lineof[q], s = P.start[l];
        if (P.failed[slot]) {                      // a failed line takes part in nothing: its candidate is its input, bit for bit
          for (int a = 0; a < 6; a++) P.plkc[slot * 6 + a] = P.plk_in[6 * (size_t)l + a];
          continue;
        }
        double x[4], yl[4], vl[4], xc[4], plk[6];
        for (int a = 0; a < 4; a++) { x[a] = P.xc[slot * 4 + a]; yl[a] = P.yl[slot * 4 + a]; vl[a] = P.vl[slot * 4 + a]; }   // (this thread's own stores)
        csum += line_step_candidate(Bc, Exc, Cc[s], x, yl, vl, coef[0], coef[1], s, line_nobs<TAB>(P, l), line_obs<TAB>(P, l), P.sqrt_info,
                                    P.huber, xc, plk);
        for (int a = 0; a < 4; a++) P.xc[slot * 4 + a] = xc[a];
        for (int a = 0; a < 6; a++) P.plkc[slot * 6 + a] = plk[a];
      }
    }
    double c8[8] = {csum, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    ls_reduce8(c8, sh);
    if (t == 0) {
      P.cost[w] = invalid ? LS_COST_INVALID : c8[0];
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

#define LS_CHECK(c, call)                                                                                      \
  do {                                                                                                         \
    hipError_t e_ = (call);                                                                                    \
    if (e_ != hipSuccess) { ctx_set_error(c, (std::string(#call) + ": " + hipGetErrorString(e_)).c_str()); st = GFBE_DEVICE_ERROR; goto done; } \
  } while (0)

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
// copied into the call's allocation, and the slots already on the device. cache (table-fed): the allocation stays on the table handle —
// it holds the candidates gfbe_ltab_commit reads.
struct StepCache { char **d; size_t *cap; };
template <bool TAB>
gfbe_status step_run(gfbe_ctx *c, StepBatch P, int W, const std::vector<int> &rec_off, const std::vector<int> &ne, const double *yp,
                     const double *vp, const double *rest, const double *radius, const double *h_pose, const double *h_ex,
                     const int *d_rec_off, gfbe_line_stepped *out, StepCache cache, StepBatch *laid = nullptr) {
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  const size_t N = (size_t)rec_off[W], nw = (size_t)W;
  const int grid = std::min(W, (int)LS_MAX_GRID);
  auto up8 = [](size_t b) { return (b + 255) & ~(size_t)255; };
  char *d = nullptr;
  double *d_yp = nullptr, *d_vp = nullptr, *d_rest = nullptr, *d_radius = nullptr, *d_pose = nullptr, *d_ex = nullptr;
  int *d_off = nullptr;
  std::vector<double> hgram, htotal, hcoef, hyl, hvl, hxc, hplk, hpose, hex, hcost, hms;
  std::vector<unsigned char> hinv;
  auto layout = [&](char *p) -> size_t {
    char *const p0 = p;
    auto take = [&](size_t bytes) { char *q = p; p += up8(bytes); return q; };
    d_yp = (double *)take(8 * nw * LS_NP); d_vp = (double *)take(8 * nw * LS_NP); d_rest = (double *)take(8 * nw * 8); d_radius = (double *)take(8 * nw);
    if (h_pose) { d_pose = (double *)take(8 * 77 * nw); d_ex = (double *)take(8 * 7 * nw); }
    if (!d_rec_off) d_off = (int *)take(sizeof(int) * (nw + 1));
    P.lineof = (int *)take(sizeof(int) * (N + 1));
    P.yl = (double *)take(8 * N * 4); P.vl = (double *)take(8 * N * 4); P.xc = (double *)take(8 * N * 4); P.plkc = (double *)take(8 * N * 6);
    P.gram = (double *)take(8 * nw * 8); P.total = (double *)take(8 * nw * 8); P.coef = (double *)take(8 * nw * 4);
    P.pose_c = (double *)take(8 * nw * 77); P.ex_c = (double *)take(8 * nw * 7); P.cost = (double *)take(8 * nw);
    P.ms = out->ms_kernel ? (double *)take(8 * nw) : nullptr;
    P.invalid = (unsigned char *)take(nw); P.n_elig = (int *)take(sizeof(int) * nw);
    return (size_t)(p - p0);
  };
  {
    const size_t need = layout(nullptr);
    if (cache.d && *cache.cap >= need) {
      d = *cache.d;
    } else {
      if (cache.d && *cache.d) { LS_CHECK(c, hipStreamSynchronize(s)); (void)hipFree(*cache.d); *cache.d = nullptr; *cache.cap = 0; }
      LS_CHECK(c, hipMalloc((void **)&d, need));
      if (cache.d) { *cache.d = d; *cache.cap = need; }
    }
    (void)layout(d);
    P.n_windows = W; P.yp = d_yp; P.vp = d_vp; P.rest = d_rest; P.radius = d_radius;
    LS_CHECK(c, hipMemcpyAsync(d_yp, yp, 8 * nw * LS_NP, hipMemcpyHostToDevice, s));
    LS_CHECK(c, hipMemcpyAsync(d_vp, vp, 8 * nw * LS_NP, hipMemcpyHostToDevice, s));
    LS_CHECK(c, hipMemcpyAsync(d_rest, rest, 8 * nw * 8, hipMemcpyHostToDevice, s));
    LS_CHECK(c, hipMemcpyAsync(d_radius, radius, 8 * nw, hipMemcpyHostToDevice, s));
    if (h_pose) {
      P.pose = d_pose; P.ex = d_ex;
      LS_CHECK(c, hipMemcpyAsync(d_pose, h_pose, 8 * 77 * nw, hipMemcpyHostToDevice, s));
      LS_CHECK(c, hipMemcpyAsync(d_ex, h_ex, 8 * 7 * nw, hipMemcpyHostToDevice, s));
    }
    if (d_rec_off) P.rec_off = d_rec_off;
    else { P.rec_off = d_off; LS_CHECK(c, hipMemcpyAsync(d_off, rec_off.data(), sizeof(int) * (nw + 1), hipMemcpyHostToDevice, s)); }
    if (laid) *laid = P;
  }
  hipLaunchKernelGGL(k_line_step<TAB>, dim3(grid), dim3(LS_THREADS), 0, s, P);
  LS_CHECK(c, hipGetLastError());
#define LS_DOWN(vec, dptr, n) do { vec.resize(std::max<size_t>(n, 1)); if (n) LS_CHECK(c, hipMemcpyAsync(vec.data(), dptr, sizeof(vec[0]) * (n), hipMemcpyDeviceToHost, s)); } while (0)
  if (out->gram) LS_DOWN(hgram, P.gram, nw * 8);
  if (out->total) LS_DOWN(htotal, P.total, nw * 8);
  if (out->coef) LS_DOWN(hcoef, P.coef, nw * 4);
  if (out->invalid) LS_DOWN(hinv, P.invalid, nw);
  if (out->y_l) LS_DOWN(hyl, P.yl, N * 4);
  if (out->v_l) LS_DOWN(hvl, P.vl, N * 4);
  if (out->orth_cand) LS_DOWN(hxc, P.xc, N * 4);
  if (out->plucker_cand) LS_DOWN(hplk, P.plkc, N * 6);
  if (out->pose_cand) LS_DOWN(hpose, P.pose_c, nw * 77);
  if (out->ex_cand) LS_DOWN(hex, P.ex_c, nw * 7);
  if (out->cost_cand) LS_DOWN(hcost, P.cost, nw);
  if (out->ms_kernel) LS_DOWN(hms, P.ms, nw);
#undef LS_DOWN
  LS_CHECK(c, hipStreamSynchronize(s));
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
  if (d && !cache.d) { (void)hipStreamSynchronize(s); (void)hipFree(d); }
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
  // the windows: the checks of gfbe_line_reduce, and the records must be these windows' own
  std::vector<int> line_off(n_windows + 1, 0), rec_off(n_windows + 1, 0), ne(n_windows, 0);
  size_t n_obs_total = 0;
  for (int w = 0; w < n_windows; w++) {
    const gfbe_line_window *L = win[w];
    if (!L || L->struct_size != (int32_t)sizeof(gfbe_line_window)) { ctx_set_error(c, "gfbe_line_step: gfbe_line_window ABI mismatch"); return GFBE_BAD_INPUT; }
    if (L->n_lines < 0 || (L->n_lines > 0 && (!L->start_frame || !L->n_obs || !L->is_triangulation || !L->line_plucker))) return GFBE_BAD_INPUT;
    size_t no = 0;
    int entering = 0;
    for (int i = 0; i < L->n_lines; i++) {
      const int s = L->start_frame[i], k = L->n_obs[i];
      if (s < 0 || k < 0 || s + k > GFBE_NFRAMES) { ctx_set_error(c, "gfbe_line_step: a line's observations run past the window"); return GFBE_BAD_INPUT; }
      no += (size_t)k;
      entering += (k >= 5 && s < GFBE_WINDOW_SIZE - 2 && L->is_triangulation[i]) ? 1 : 0;
    }
    if (no > 0 && !L->obs) return GFBE_BAD_INPUT;
    if (rec->n_eligible[w] != entering) { ctx_set_error(c, "gfbe_line_step: n_eligible is not the window's count of entering lines"); return GFBE_BAD_INPUT; }
    if ((size_t)line_off[w] + (size_t)L->n_lines > (size_t)INT32_MAX / 512 || n_obs_total + no > (size_t)INT32_MAX / 8) return GFBE_BAD_INPUT;
    line_off[w + 1] = line_off[w] + L->n_lines;
    rec_off[w + 1] = rec_off[w] + entering;
    ne[w] = entering;
    n_obs_total += no;
  }
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_line_step: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (n_windows == 0) return GFBE_OK;
  const int n_lines = line_off[n_windows];
  const size_t N = (size_t)rec_off[n_windows];
  // pack as gfbe_line_reduce does: ints (line_off, obs_off, start), doubles (plucker, obs, poses, extrinsics), the triangulation flags
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
  auto up8 = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_int = sizeof(int) * ints.size(), b_dbl = sizeof(double) * dbl.size(), b_tri = h_tri.size();
  const size_t b_rec[5] = {8 * N * 16, 8 * N * 4, 8 * N * LS_WROW, 8 * N * 10, N + 1};
  StepBatch P{};
  {
    size_t need = up8(b_int) + up8(b_dbl) + up8(b_tri);
    for (size_t b : b_rec) need += up8(b);
    LS_CHECK(c, hipMalloc((void **)&d, need));
    char *p = d;
    auto take = [&](size_t bytes) { char *q = p; p += up8(bytes); return q; };
    int *d_int = (int *)take(b_int);
    double *d_dbl = (double *)take(b_dbl);
    unsigned char *d_tri = (unsigned char *)take(b_tri);
    double *d_Vinv = (double *)take(b_rec[0]), *d_bl = (double *)take(b_rec[1]), *d_W = (double *)take(b_rec[2]), *d_V = (double *)take(b_rec[3]);
    unsigned char *d_failed = (unsigned char *)take(b_rec[4]);
    P.line_off = d_int; P.obs_off = d_int + (h_obs_off - h_line_off); P.start = d_int + (h_start - h_line_off);
    P.plk_in = d_dbl; P.obs = d_dbl + (h_obs - h_plk); P.pose = d_dbl + (h_pose - h_plk); P.ex = d_dbl + (h_ex - h_plk);
    P.tri = d_tri;
    P.Vinv = d_Vinv; P.bl = d_bl; P.W = d_W; P.V = d_V; P.failed = d_failed;
    P.sqrt_info = sqrt_info; P.huber = huber_width;
    LS_CHECK(c, hipMemcpyAsync(d_int, ints.data(), b_int, hipMemcpyHostToDevice, s));
    LS_CHECK(c, hipMemcpyAsync(d_dbl, dbl.data(), b_dbl, hipMemcpyHostToDevice, s));
    LS_CHECK(c, hipMemcpyAsync(d_tri, h_tri.data(), b_tri, hipMemcpyHostToDevice, s));
    if (N) {
      LS_CHECK(c, hipMemcpyAsync(d_Vinv, rec->Vinv, b_rec[0], hipMemcpyHostToDevice, s));
      LS_CHECK(c, hipMemcpyAsync(d_bl, rec->bl, b_rec[1], hipMemcpyHostToDevice, s));
      LS_CHECK(c, hipMemcpyAsync(d_W, rec->W, b_rec[2], hipMemcpyHostToDevice, s));
      LS_CHECK(c, hipMemcpyAsync(d_V, rec->V, b_rec[3], hipMemcpyHostToDevice, s));
      LS_CHECK(c, hipMemcpyAsync(d_failed, rec->failed, N, hipMemcpyHostToDevice, s));
    }
  }
  st = step_run<false>(c, P, n_windows, rec_off, ne, y_p, v_p, rest, radius, nullptr, nullptr, nullptr, out, StepCache{nullptr, nullptr});   // (synchronises the stream)
done:
  if (d) { (void)hipStreamSynchronize(s); (void)hipFree(d); }
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
  const int W = t->d.W, b = t->cur;
  if (!step_inputs_ok(c, "gfbe_ltab_step", W, y_p, v_p, rest, radius)) return GFBE_BAD_INPUT;
  if (!t->keep_records || !t->rec_valid) { ctx_set_error(c, "gfbe_ltab_step: no records are held (gfbe_ltab_keep_records, then gfbe_ltab_reduce in solve mode)"); return GFBE_BAD_INPUT; }
  if (t->rec_gen != t->gen) { ctx_set_error(c, "gfbe_ltab_step: the tables have changed since the reduce that wrote the records"); return GFBE_BAD_INPUT; }
  if (std::memcmp(t->rec_pose.data(), pose7, 8 * 77 * (size_t)W) != 0 || std::memcmp(t->rec_pose.data() + 77 * (size_t)W, ex_cam, 8 * 7 * (size_t)W) != 0) {
    ctx_set_error(c, "gfbe_ltab_step: pose7 / ex_cam differ from the reduce's");
    return GFBE_BAD_INPUT;
  }
  t->cand_valid = false;
  StepBatch P{};
  P.count = t->d.count; P.nobs = t->d.nobs[b]; P.F = t->d.F; P.start = t->d.start[b]; P.tri = t->d.tri[b]; P.plk_in = t->d.plk[b];
  P.obs = t->d.obs[b];
  P.Vinv = t->rec_Vinv; P.bl = t->rec_bl; P.W = t->rec_W; P.V = t->rec_V; P.failed = t->rec_failed;
  P.sqrt_info = sqrt_info; P.huber = huber_width;
  StepBatch laid{};
  const gfbe_status st = step_run<true>(c, P, W, t->rec_off, t->rec_ne, y_p, v_p, rest, radius, pose7, ex_cam, t->rec_off_d, out,
                                        StepCache{&t->step_d, &t->step_cap}, &laid);
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
