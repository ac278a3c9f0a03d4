// gfbe_line.hip — line landmarks on the device: stand-alone evaluation of the line projection factor, and the line-only refinement
// that runs on every frame of a `use_line` deployment (estimator.cpp:1426-1438), as one batched call:
//
//   Estimator::onlyLineOpt                       estimator/estimator.cpp:4264-4332
//   FeatureManager::getLineOrthVector / setLineOrth   estimator/feature_manager.cpp:1068-1125 (orth <-> Plücker on entry and exit)
//   FeatureManager::removeLineOutlier            estimator/feature_manager.cpp:1372-1460 (with reprojection_error :1126-1150)
//
// Solver: ceres::Solve with Ceres 1.14's defaults as onlyLineOpt leaves them — Levenberg-Marquardt trust region, Jacobi scaling,
// max_num_iterations = NUM_ITERATIONS — with every pose and the camera extrinsic constant and CauchyLoss(1.0) on each observation. The
// LM conventions are those of the pose graph's restatement (gfbe_posegraph.hip, oracle/gfo_posegraph.cpp): Jacobi scaling fixed at
// iteration 0, diagonal clamp(diag, 1e-6, 1e32) / radius (kept on a rejected step), initial radius 1e4, the radius / decrease-factor
// update, min_relative_decrease 1e-3, function / gradient / parameter tolerances 1e-6 / 1e-10 / 1e-8; the gradient max-norm is
// |x - Plus(x, -g)|_inf through the line Plus, as Ceres takes it. With the poses constant the normal equations are block-diagonal:
// one 4 x 4 block per line.
//
// Shape: ONE WORKGROUP PER WINDOW runs the whole loop in one launch. Lines are spread over the threads (line t, t + 256, ...); each
// line's linearisation (4 x 4 J^T J, J^T r), scaling, LM diagonal and parameters live in a per-line scratch row; the per-window sums
// (cost, model cost change, |step|^2, |x|^2, gradient max-norm, the factorisation failure flag) go through a fixed-order reduction
// (wave shuffle tree, then the waves in order through LDS). Every thread holds the loop's scalars and takes the same decisions from
// the broadcast sums. No grid barrier, no atomics, nothing shared between windows: a window's outputs are bit-reproducible and do not
// depend on the batch around it. FP64 vector ALU only (4 x 4 blocks leave the matrix cores nothing to do).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"
#include "gfbe_line.h"
#include "gfbe_line_batch.h"

using namespace gfd;

namespace {

enum { LR_THREADS = 256, LR_WAVES = LR_THREADS / 64, LR_ROW = 40 };
// per-line scratch row (LR_ROW doubles): x [0, 4), candidate [4, 8), H [8, 24), g [24, 28), Jacobi scale [28, 32), LM diagonal [32, 36)
enum { LX = 0, LC = 4, LH = 8, LG = 24, LS = 28, LD = 32 };

__global__ __launch_bounds__(256) void k_line_eval(int n, const double *pose, const double *ex, const double *orth, const double *obs,
                                                   double sqrt_info, int robust, double *r, double *Jp, double *Je, double *Jo,
                                                   double *cost_part) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const LineRT B = line_make_pose(pose + 7 * (size_t)k), E = line_make_pose(ex);
  double res[2], jp[14], je[14], jo[8];
  line_factor<true>(B, E, orth + 4 * (size_t)k, obs + 4 * (size_t)k, sqrt_info, res, jp, je, jo);
  const double s = res[0] * res[0] + res[1] * res[1];
  double c;
  if (robust) {
    double sr;
    c = line_cauchy(s, 1.0, &sr);
    res[0] *= sr; res[1] *= sr;
    for (int q = 0; q < 14; q++) { jp[q] *= sr; je[q] *= sr; }
    for (int q = 0; q < 8; q++) jo[q] *= sr;
  } else {
    c = 0.5 * s;
  }
  if (r) for (int q = 0; q < 2; q++) r[2 * (size_t)k + q] = res[q];
  if (Jp) for (int q = 0; q < 14; q++) Jp[14 * (size_t)k + q] = jp[q];
  if (Je) for (int q = 0; q < 14; q++) Je[14 * (size_t)k + q] = je[q];
  if (Jo) for (int q = 0; q < 8; q++) Jo[8 * (size_t)k + q] = jo[q];
  cost_part[k] = c;       // summed in factor order on the host
}

// the lines of a batch of windows (host-fed or the tables in place: LineList, gfbe_line.h), the loop's parameters, scratch and outputs
struct LineBatch {
  LineList L;
  double sqrt_info, cauchy;
  int max_it;
  double *row;                  // [n_lines][LR_ROW]
  double *plk_out;              // [n_lines][6]
  unsigned char *keep;          // [n_lines]
  gfbe_summary *sum;            // [n_windows]
};

// cost of line l at x; with H, g: its Cauchy-corrected normal-equation block and gradient
template <bool LIN, bool TAB>
__device__ double line_lin(const LineBatch &P, int l, const double *x, const LineRT *Bs, const LineRT &Ex, double *H, double *g) {
  const LineList &L = P.L;
  double cost = 0.0;
  if (LIN) { for (int q = 0; q < 16; q++) H[q] = 0.0; for (int q = 0; q < 4; q++) g[q] = 0.0; }
  const int s = L.start[l], m = line_nobs<TAB>(L, l);
  const double *ob = line_obs<TAB>(L, l);
  for (int k = 0; k < m; k++) {
    double r[2], Jo[8];
    line_factor<LIN>(Bs[s + k], Ex, x, ob + 4 * k, P.sqrt_info, r, nullptr, nullptr, LIN ? Jo : nullptr);
    double sr;
    cost += line_cauchy(r[0] * r[0] + r[1] * r[1], P.cauchy, &sr);
    if (LIN) {
      r[0] *= sr; r[1] *= sr;
      for (int q = 0; q < 8; q++) Jo[q] *= sr;
      for (int a = 0; a < 4; a++) {
        g[a] += Jo[a] * r[0] + Jo[4 + a] * r[1];
        for (int b = 0; b < 4; b++) H[4 * a + b] += Jo[a] * Jo[b] + Jo[4 + a] * Jo[4 + b];
      }
    }
  }
  return cost;
}

// |x - Plus(x, -g)|_inf of one line
__device__ double line_grad_norm(const double *x, const double *g) {
  const double mg[4] = {-g[0], -g[1], -g[2], -g[3]};
  double xp[4], m = 0.0;
  line_orth_plus(x, mg, xp);
  for (int a = 0; a < 4; a++) m = fmax(m, fabs(x[a] - xp[a]));
  return m;
}

// 4 x 4 SPD solve A y = b by Cholesky; false if a pivot is not positive (or not a number)
__device__ bool chol4_solve(double *A, const double *b, double *y) {
  double L[16];
  for (int q = 0; q < 16; q++) L[q] = 0.0;
  for (int j = 0; j < 4; j++) {
    double d = A[5 * j];
    for (int k = 0; k < j; k++) d -= L[4 * j + k] * L[4 * j + k];
    if (!(d > 0.0)) return false;
    const double ljj = sqrt(d);
    L[5 * j] = ljj;
    for (int i = j + 1; i < 4; i++) {
      double s = A[4 * i + j];
      for (int k = 0; k < j; k++) s -= L[4 * i + k] * L[4 * j + k];
      L[4 * i + j] = s / ljj;
    }
  }
  double z[4];
  for (int i = 0; i < 4; i++) { double s = b[i]; for (int k = 0; k < i; k++) s -= L[4 * i + k] * z[k]; z[i] = s / L[5 * i]; }
  for (int i = 3; i >= 0; i--) { double s = z[i]; for (int k = i + 1; k < 4; k++) s -= L[4 * k + i] * y[k]; y[i] = s / L[5 * i]; }
  return true;
}

template <bool TAB>
__global__ __launch_bounds__(LR_THREADS) void k_line_refine(LineBatch P) {
  const int w = blockIdx.x, t = threadIdx.x;
  const LineList &L = P.L;
  __shared__ LineRT Bs[GFBE_NFRAMES], Cw[GFBE_NFRAMES];
  __shared__ LineRT Ex;
  __shared__ double sh[4 * LR_WAVES];
  // the per-window sums: four per-thread values through the fixed-order reduction (line_block_reduce, gfbe_line.h), entry 0 by max
  // when max0; every thread gets the results in red[4]
  double red[4];
  auto reduce4 = [&](double v0, double v1, double v2, double v3, bool max0) {
    red[0] = v0; red[1] = v1; red[2] = v2; red[3] = v3;
    line_block_reduce<4, LR_WAVES>(red, max0 ? 1u : 0u, sh);
  };
  int l0, l1;
  line_range<TAB>(L, w, &l0, &l1);
  const uint64_t t_start = wall_clock64();
  line_stage_poses(L, w, Bs, &Ex);
  __syncthreads();
  line_stage_cameras(Bs, Ex, Cw);
  // eligibility count
  double ne = 0.0;
  for (int l = l0 + t; l < l1; l += LR_THREADS) ne += line_eligible<TAB>(L, l) ? 1.0 : 0.0;
  reduce4(0.0, ne, 0.0, 0.0, false);
  const int n_elig = (int)red[1];
  // the loop's scalars live in every thread (the same values everywhere); its per-iteration record in LDS, written by thread 0
  __shared__ double hist[16];
  __shared__ unsigned char acc[16];
  int status = GFBE_OK, termination = 0, num_successful = 0;
  auto record = [&](int i, int a, double v) { if (t == 0) { hist[i] = v; acc[i] = (unsigned char)a; } };
  if (n_elig < 4) {      // `if (feature_index < 3) return;` — nothing solved, nothing written back, removeLineOutlier not called
    for (int l = l0 + t; l < l1; l += LR_THREADS) {
      for (int a = 0; a < 6; a++) P.plk_out[6 * (size_t)l + a] = L.plk_in[6 * (size_t)l + a];
      P.keep[l] = 1;
    }
    if (t == 0) { gfbe_summary sm{}; sm.status = GFBE_OK; sm.termination = 5; P.sum[w] = sm; }
    return;
  }
  // entry: para_LineFeature = plk_to_orth(plk_to_pose(line_plucker, Rwc, twc)) of the start frame; the first linearisation
  double c = 0.0, x2 = 0.0, gm = 0.0;
  for (int l = l0 + t; l < l1; l += LR_THREADS) {
    if (!line_eligible<TAB>(L, l)) continue;
    double *row = P.row + (size_t)l * LR_ROW, lw[6];
    const int s = L.start[l];
    line_plk_to_pose(L.plk_in + 6 * (size_t)l, Cw[s].R, Cw[s].t, lw);
    line_plk_to_orth(lw, row + LX);
    c += line_lin<true, TAB>(P, l, row + LX, Bs, Ex, row + LH, row + LG);
    for (int a = 0; a < 4; a++) { x2 += row[LX + a] * row[LX + a]; row[LS + a] = 1.0 / (1.0 + sqrt(row[LH + 5 * a])); }
    gm = fmax(gm, line_grad_norm(row + LX, row + LG));
  }
  reduce4(gm, c, x2, 0.0, true);
  double cost = red[1], gmax = red[0], x_norm = sqrt(red[2]), radius = 1e4, decrease = 2.0;
  const double initial_cost = cost;
  if (t < 16) { hist[t] = 0.0; acc[t] = 0; }
  __syncthreads();
  record(0, 0, cost);
  status = GFBE_NO_CONVERGENCE;
  int it = 0, invalid = 0;
  bool reuse = false;
  while (true) {
    if (it >= P.max_it) { termination = 0; break; }
    if (gmax <= 1e-10) { termination = 3; status = GFBE_OK; break; }
    if (radius < 1e-32) { termination = 4; break; }
    it++;
    // every line: scaled system, LM diagonal, 4 x 4 solve, model cost change, candidate
    double fail = 0.0, mc = 0.0, st2 = 0.0, cx2 = 0.0;
    for (int l = l0 + t; l < l1; l += LR_THREADS) {
      if (!line_eligible<TAB>(L, l)) continue;
      double *row = P.row + (size_t)l * LR_ROW;
      double Hs[16], A[16], rhs[4], y[4];
      for (int a = 0; a < 4; a++) {
        for (int b = 0; b < 4; b++) Hs[4 * a + b] = row[LH + 4 * a + b] * row[LS + a] * row[LS + b];
        rhs[a] = -row[LS + a] * row[LG + a];
      }
      if (!reuse) for (int a = 0; a < 4; a++) row[LD + a] = fmin(fmax(Hs[5 * a], 1e-6), 1e32);
      for (int q = 0; q < 16; q++) A[q] = Hs[q];
      for (int a = 0; a < 4; a++) A[5 * a] += row[LD + a] / radius;
      if (!chol4_solve(A, rhs, y)) { fail = 1.0; continue; }
      double gy = 0.0, yHy = 0.0;
      for (int a = 0; a < 4; a++) {
        double s = 0.0;
        for (int b = 0; b < 4; b++) s += Hs[4 * a + b] * y[b];
        gy += -rhs[a] * y[a]; yHy += y[a] * s;
      }
      mc += -(gy + 0.5 * yHy);
      double d[4];
      for (int a = 0; a < 4; a++) d[a] = row[LS + a] * y[a];
      line_orth_plus(row + LX, d, row + LC);
      for (int a = 0; a < 4; a++) { const double df = row[LC + a] - row[LX + a]; st2 += df * df; cx2 += row[LC + a] * row[LC + a]; }
    }
    reduce4(fail, mc, st2, cx2, true);
    const double model_change = red[1], step2 = red[2], cand_x2 = red[3];
    if (red[0] != 0.0 || !(model_change > 0.0)) {      // invalid step
      record(it, 0, cost);
      if (++invalid >= 5) { termination = 4; status = GFBE_NUMERICAL_FAILURE; break; }
      radius /= decrease; decrease *= 2; reuse = true;
      continue;
    }
    invalid = 0;
    double cc = 0.0;
    for (int l = l0 + t; l < l1; l += LR_THREADS)
      if (line_eligible<TAB>(L, l)) cc += line_lin<false, TAB>(P, l, P.row + (size_t)l * LR_ROW + LC, Bs, Ex, nullptr, nullptr);
    reduce4(0.0, cc, 0.0, 0.0, false);
    const double cand_cost = red[1];
    record(it, 0, cost);
    if (sqrt(step2) <= 1e-8 * (x_norm + 1e-8)) { termination = 2; status = GFBE_OK; break; }
    const double change = cost - cand_cost;
    if (fabs(change) <= 1e-6 * cost) { termination = 1; status = GFBE_OK; break; }
    const double rho = change / model_change;
    if (rho > 1e-3) {
      cost = cand_cost; x_norm = sqrt(cand_x2);
      record(it, 1, cost); num_successful++;
      radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * rho - 1.0, 3.0)));
      decrease = 2.0; reuse = false;
      double g2 = 0.0;
      for (int l = l0 + t; l < l1; l += LR_THREADS) {
        if (!line_eligible<TAB>(L, l)) continue;
        double *row = P.row + (size_t)l * LR_ROW;
        for (int a = 0; a < 4; a++) row[LX + a] = row[LC + a];
        (void)line_lin<true, TAB>(P, l, row + LX, Bs, Ex, row + LH, row + LG);
        g2 = fmax(g2, line_grad_norm(row + LX, row + LG));
      }
      reduce4(g2, 0.0, 0.0, 0.0, true);
      gmax = red[0];
    } else {
      record(it, 0, cost);
      radius /= decrease; decrease *= 2; reuse = true;
    }
  }
  // exit: setLineOrth (line_plucker = plk_from_pose(orth_to_plk(orth), Rwc, twc)), then removeLineOutlier on the written-back lines
  for (int l = l0 + t; l < l1; l += LR_THREADS) {
    double *out = P.plk_out + 6 * (size_t)l;
    if (!line_eligible<TAB>(L, l)) {
      for (int a = 0; a < 6; a++) out[a] = L.plk_in[6 * (size_t)l + a];
      P.keep[l] = 1;
      continue;
    }
    const int s = L.start[l], m = line_nobs<TAB>(L, l);
    const double *ob = line_obs<TAB>(L, l);
    double lw[6];
    line_orth_to_plk(P.row + (size_t)l * LR_ROW + LX, lw);
    line_plk_from_pose(lw, Cw[s].R, Cw[s].t, out);
    unsigned char keep = 1;
    if (line_endpoints_bad(out, ob)) {
      keep = 0;
    } else {
      line_plk_to_pose(out, Cw[s].R, Cw[s].t, lw);
      double allerr = 0.0;
      for (int k = 0; k < m; k++) {
        const double err = line_reprojection_error(ob + 4 * k, Cw[s + k].R, Cw[s + k].t, lw);
        if (allerr < err) allerr = err;
      }
      if (allerr > 3.0 / 500.0) keep = 0;
    }
    P.keep[l] = keep;
  }
  if (t == 0) {
    gfbe_summary sm{};
    sm.status = status; sm.termination = termination; sm.num_successful = num_successful;
    sm.iterations = it; sm.initial_cost = initial_cost; sm.final_cost = cost; sm.final_radius = radius;
    for (int q = 0; q < 16; q++) { sm.cost_history[q] = hist[q]; sm.accepted[q] = acc[q]; }
    sm.ms_solve = (double)(wall_clock64() - t_start) * 1e-5;      // (100 MHz device wall clock)
    P.sum[w] = sm;
  }
}

}  // namespace

namespace gfd {
size_t line_refine_row_doubles() { return LR_ROW; }
void launch_line_refine_tables(const LineList &L, int n_tables, double sqrt_info, double cauchy, int max_it, double *row, double *plk_out,
                               unsigned char *keep, gfbe_summary *sum, hipStream_t s) {
  LineBatch P{};
  P.L = L; P.sqrt_info = sqrt_info; P.cauchy = cauchy; P.max_it = std::min(max_it, 15);
  P.row = row; P.plk_out = plk_out; P.keep = keep; P.sum = sum;
  hipLaunchKernelGGL(k_line_refine<true>, dim3(n_tables), dim3(LR_THREADS), 0, s, P);
}
}  // namespace gfd

extern "C" gfbe_status gfbe_line_eval(gfbe_ctx *c, int32_t n, const double *pose, const double *ex_cam, const double *orth, const double *obs,
                                      double sqrt_info, int32_t robustify, double *r, double *J_pose, double *J_ex, double *J_orth,
                                      double *cost) {
  if (!c || n < 0 || (n > 0 && (!pose || !orth || !obs)) || !ex_cam) return GFBE_BAD_INPUT;
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_line_eval: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (n == 0) { if (cost) *cost = 0.0; return GFBE_OK; }
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  double *d = nullptr;
  const size_t np = (size_t)7 * n, no = (size_t)4 * n, nr = (size_t)2 * n, nj = (size_t)14 * n, nk = (size_t)8 * n;
  double *dpose, *dex, *dorth, *dobs, *dr, *djp, *dje, *djo, *dc;
  std::vector<double> hc(n);
  GFBE_CHECK_DONE(c, hipMalloc((void **)&d, sizeof(double) * (np + 7 + 2 * no + nr + 2 * nj + nk + n)));
  dpose = d; dex = dpose + np; dorth = dex + 7; dobs = dorth + no; dr = dobs + no; djp = dr + nr; dje = djp + nj; djo = dje + nj; dc = djo + nk;
  GFBE_CHECK_DONE(c, hipMemcpyAsync(dpose, pose, sizeof(double) * np, hipMemcpyHostToDevice, s));
  GFBE_CHECK_DONE(c, hipMemcpyAsync(dex, ex_cam, sizeof(double) * 7, hipMemcpyHostToDevice, s));
  GFBE_CHECK_DONE(c, hipMemcpyAsync(dorth, orth, sizeof(double) * no, hipMemcpyHostToDevice, s));
  GFBE_CHECK_DONE(c, hipMemcpyAsync(dobs, obs, sizeof(double) * no, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_line_eval, dim3((n + 255) / 256), dim3(256), 0, s, n, dpose, dex, dorth, dobs, sqrt_info, robustify ? 1 : 0,
                     r ? dr : nullptr, J_pose ? djp : nullptr, J_ex ? dje : nullptr, J_orth ? djo : nullptr, dc);
  GFBE_CHECK_DONE(c, hipGetLastError());
  GFBE_CHECK_DONE(c, hipMemcpyAsync(hc.data(), dc, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  GFBE_CHECK_DONE(c, hipStreamSynchronize(s));
  // (outputs are written only once the whole evaluation has succeeded)
  if (r) GFBE_CHECK_DONE(c, hipMemcpy(r, dr, sizeof(double) * nr, hipMemcpyDeviceToHost));
  if (J_pose) GFBE_CHECK_DONE(c, hipMemcpy(J_pose, djp, sizeof(double) * nj, hipMemcpyDeviceToHost));
  if (J_ex) GFBE_CHECK_DONE(c, hipMemcpy(J_ex, dje, sizeof(double) * nj, hipMemcpyDeviceToHost));
  if (J_orth) GFBE_CHECK_DONE(c, hipMemcpy(J_orth, djo, sizeof(double) * nk, hipMemcpyDeviceToHost));
  if (cost) { double tot = 0.0; for (int k = 0; k < n; k++) tot += hc[k]; *cost = tot; }
done:
  if (d) (void)hipFree(d);
  return st;
}

extern "C" gfbe_status gfbe_line_refine(gfbe_ctx *c, int32_t n_windows, const gfbe_line_window *const *win, double sqrt_info,
                                        double cauchy_scale, int32_t max_num_iterations, double *plucker_out, uint8_t *keep_out,
                                        gfbe_summary *summary) {
  if (!c || n_windows < 0 || (n_windows > 0 && (!win || !summary)) || !(cauchy_scale > 0.0) || max_num_iterations < 0) return GFBE_BAD_INPUT;
  LineWindows B;
  if (!check_line_windows(c, "gfbe_line_refine", n_windows, win, (size_t)INT32_MAX / 64, B)) return GFBE_BAD_INPUT;
  const int n_lines = B.n_lines();
  if (n_lines > 0 && (!plucker_out || !keep_out)) return GFBE_BAD_INPUT;
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_line_refine: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (n_windows == 0) return GFBE_OK;
  hipStream_t s = ctx_stream(c);
  gfbe_status st = GFBE_OK;
  const size_t b_out = sizeof(double) * 6 * (size_t)n_lines, b_sum = sizeof(gfbe_summary) * (size_t)n_windows;
  std::vector<double> h_out((size_t)6 * n_lines);
  std::vector<unsigned char> h_keep(std::max(n_lines, 1));
  std::vector<gfbe_summary> h_sum(n_windows);
  LineUpload U;
  LineBatch P{};
  // the kernel's scratch rows and outputs, behind the packed windows in the call's one allocation
  auto layout = [&](char *base) {
    Arena a(base);
    P.row = a.take<double>((size_t)LR_ROW * n_lines); P.plk_out = a.take<double>((size_t)6 * n_lines);
    P.sum = a.take<gfbe_summary>(n_windows); P.keep = a.take<unsigned char>(std::max(n_lines, 1));
    return a.off;
  };
  GFBE_CHECK_DONE(c, upload_line_windows(s, n_windows, win, B, layout(nullptr), U));
  (void)layout(U.extra);
  P.L = U.L; P.sqrt_info = sqrt_info; P.cauchy = cauchy_scale; P.max_it = std::min<int>(max_num_iterations, 15);
  hipLaunchKernelGGL(k_line_refine<false>, dim3(n_windows), dim3(LR_THREADS), 0, s, P);
  GFBE_CHECK_DONE(c, hipGetLastError());
  if (n_lines) {
    GFBE_CHECK_DONE(c, hipMemcpyAsync(h_out.data(), P.plk_out, b_out, hipMemcpyDeviceToHost, s));
    GFBE_CHECK_DONE(c, hipMemcpyAsync(h_keep.data(), P.keep, (size_t)n_lines, hipMemcpyDeviceToHost, s));
  }
  GFBE_CHECK_DONE(c, hipMemcpyAsync(h_sum.data(), P.sum, b_sum, hipMemcpyDeviceToHost, s));
  GFBE_CHECK_DONE(c, hipStreamSynchronize(s));
  {
    int worst = GFBE_OK;
    for (int w = 0; w < n_windows; w++) worst = std::max(worst, (int)h_sum[w].status);
    if (n_lines) { std::memcpy(plucker_out, h_out.data(), b_out); std::memcpy(keep_out, h_keep.data(), (size_t)n_lines); }
    std::memcpy(summary, h_sum.data(), b_sum);
    st = (gfbe_status)worst;
  }
done:
  if (U.d) (void)hipFree(U.d);
  return st;
}
