// gfbe_vreg.hip — the scan-to-map registration loop of the LiDAR odometry on the device: what consumes the rows of the association
// (gfbe_vmap.hip) where they are produced.
//
//   lidarodom::optimize, the ICP loop         lio/src/liw/lio/lidarodom.cpp:534-748
//   Location / Rotation / SmallVelocity       lio/src/liw/lidarFactor.cpp:125-219
//   RotationParameterization::Plus            lio/src/liw/poseParameterization.cpp:31-50
//
// The loop lives in one VrState in device memory: the poses, the LM state of the inner solve, the per-iteration trace and a `done`
// flag. The host uploads the arguments once, enqueues max_num_iteration x (k_vm_assoc, k_vm_compact, k_vr_begin,
// (lm_max_num_iterations + 1) x (k_vr_lin, k_vr_step)) and k_vm_local, and waits once. Every kernel returns at once when `done` is
// set or its inner solve has terminated; nothing waits on another workgroup, so the sequence cannot hang.
//
// k_vr_lin: one thread per residual at the pose VrState.xe (the current pose, or the candidate of the step in flight): lio_row (the
// body k_lio runs), the Huber corrector (rho'' <= 0: r and J scaled by sqrt(rho')), J^T J, J^T r and the cost accumulated in
// registers per workgroup and reduced in a fixed order into one partial per workgroup. Linearising at the candidate gives its cost
// and, when the step is accepted, the next iteration's normal equations in the same pass.
// k_vr_step: one wave. Lanes add the partials in workgroup order; lane 0 adds the consistency factors, decides on the candidate
// (Ceres 1.14's rules as oracle/gfo_posegraph.cpp states them), solves the next scaled, regularised system by a Cholesky in LDS,
// forms the next candidate and, when the inner solve ends, runs the outer exit test and writes the trace.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "gfbe_device.h"
#include "gfbe_lio_pose.h"
#include "gfbe_tabstage.h"
#include "gfbe_vmap_impl.h"

using namespace gfd;

namespace {

constexpr int VR_THREADS = 256;      // workgroup width of k_vr_lin (tests/vreg_cases.py cuts rows at 255 / 256 / 257)
constexpr int VR_MAXG = 32;          // partials per linearisation
constexpr int VR_MAXIT = 32;

struct VrOpt {
  int ct, K, L, min_res;
  double sqrt_info, huber, cov, b_loc, b_rot, b_vel, thr_t, thr_r;
  double prev_t[3], prev_q[4];
};

struct VrState {
  int done, k, failed, overflow, no_res, too_few, converged, nres;
  int active, phase, it, invalid, reuse, acc_bits, pad0, pad1;
  double x[14], x0[14], xe[14];      // current poses [begin | end], the poses at the head of the outer iteration, the evaluation point
  double H[144], g[12], scale[12], diag2[12];
  double cost, radius, decrease, x_norm, model_change, step2;
  double local[4];                   // sv [3] | degenerate (k_vm_local)
  int s_nres[VR_MAXIT], s_it[VR_MAXIT], s_acc[VR_MAXIT], s_term[VR_MAXIT];
  double s_c0[VR_MAXIT], s_c1[VR_MAXIT], s_dt[VR_MAXIT], s_dr[VR_MAXIT], s_trace[VR_MAXIT][14];
};

template <int CT> struct VrDim { static constexpr int DN = CT ? 12 : 6, NP = CT ? 14 : 7, PART = DN * (DN + 1) / 2 + DN + 1; };

// head of an outer iteration: the residual count of the association just made, the fresh LM state
__global__ void k_vr_begin(VrState *S, const int *meta, VrOpt O) {
  if (threadIdx.x != 0 || S->done) return;
  if (meta[M_OVER]) { S->overflow = 1; S->done = 1; return; }
  const int n = meta[M_NRES], k = S->k;
  S->s_nres[k] = n; S->nres = n;
  if (n < O.min_res) S->too_few = 1;
  if (n == 0) { S->no_res = 1; S->done = 1; return; }
  S->active = 1; S->phase = 0; S->it = 0; S->invalid = 0; S->reuse = 0; S->acc_bits = 0;
  S->radius = 1e4; S->decrease = 2.0;
  for (int i = 0; i < 14; i++) { S->x0[i] = S->x[i]; S->xe[i] = S->x[i]; }
}

template <int CT>
__global__ __launch_bounds__(VR_THREADS) void k_vr_lin(const VrState *S, const int *meta, const double *pts, const double *normals, const double *offsets,
                                                       const double *alpha, const double *weights, VrOpt O, double *part) {
  constexpr int DN = VrDim<CT>::DN, PART = VrDim<CT>::PART, TRI = DN * (DN + 1) / 2;
  if (S->done || !S->active) return;      // (grid-uniform)
  const int t = threadIdx.x, n = meta[M_NRES];
  double acc[PART];
#pragma unroll
  for (int q = 0; q < PART; q++) acc[q] = 0.0;
  const double *pb = S->xe, *pe = S->xe + 7;
  const Qx qb = {pb[3], pb[4], pb[5], pb[6]};
  const Qx qe = {pe[3], pe[4], pe[5], pe[6]};
  const double hb = O.huber * O.huber;
  for (int k = blockIdx.x * VR_THREADS + t; k < n; k += gridDim.x * VR_THREADS) {
    double Jk[DN], rk, al = 0.0;
    if (CT) al = alpha[k];
    lio_row<CT>(pts + 3 * (size_t)k, normals + 3 * (size_t)k, offsets[k], weights[k], al, O.sqrt_info, qb, qe, pb, pe, Jk, &rk);
    const double sq = rk * rk;
    double rho0 = sq;
    if (O.huber > 0.0 && sq > hb) {      // HuberLoss + Corrector: rho'' <= 0, so residual and Jacobian are scaled by sqrt(rho') alone
      const double rr = sqrt(sq), sr = sqrt(fmax(1e-300, O.huber / rr));
      rho0 = 2.0 * O.huber * rr - hb;
      rk *= sr;
#pragma unroll
      for (int a = 0; a < DN; a++) Jk[a] *= sr;
    }
    int e = 0;
#pragma unroll
    for (int a = 0; a < DN; a++)
#pragma unroll
      for (int b = 0; b <= a; b++) acc[e++] += Jk[a] * Jk[b];
#pragma unroll
    for (int a = 0; a < DN; a++) acc[TRI + a] += Jk[a] * rk;
    acc[TRI + DN] += 0.5 * rho0;
  }
  // fixed-order reduction: 64-lane butterflies, then the waves through LDS (the scheme of k_lio)
  __shared__ double red[VR_THREADS / 64][PART];
#pragma unroll
  for (int q = 0; q < PART; q++) {
    double v = acc[q];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((t & 63) == 0) red[t >> 6][q] = v;
  }
  __syncthreads();
  if (t < PART) {
    double v = 0.0;
    for (int wv = 0; wv < VR_THREADS / 64; wv++) v += red[wv][t];
    part[(size_t)blockIdx.x * PART + t] = v;
  }
}

__device__ __forceinline__ void vr_plus(const double *x, const double *d6, double *out) {      // t + dt; q * deltaQ(dtheta), normalised
  for (int a = 0; a < 3; a++) out[a] = x[a] + d6[a];
  const double hx = d6[3] / 2.0, hy = d6[4] / 2.0, hz = d6[5] / 2.0;
  const double dn = sqrt(hx * hx + hy * hy + hz * hz + 1.0);
  const Qx dq = {hx / dn, hy / dn, hz / dn, 1.0 / dn};
  const Qx q = qmulx({x[3], x[4], x[5], x[6]}, dq);
  const double qn = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  out[3] = q.x / qn; out[4] = q.y / qn; out[5] = q.z / qn; out[6] = q.w / qn;
}
// AngularDistance in degrees, the acos argument clamped to [-1, 1]
__device__ __forceinline__ double vr_angle(const double *qa, const double *qb) {
  double Ra[9], Rb[9];
  qrotx({qa[0], qa[1], qa[2], qa[3]}, Ra);
  qrotx({qb[0], qb[1], qb[2], qb[3]}, Rb);
  double tr = 0.0;
  for (int i = 0; i < 9; i++) tr += Ra[i] * Rb[i];
  const double arg = fmin(1.0, fmax(-1.0, (tr - 1.0) / 2.0));
  return acos(arg) * 180.0 / 3.14159265358979323846;
}

template <int CT>
__global__ __launch_bounds__(64) void k_vr_step(VrState *S, const double *part, int G, VrOpt O) {
  constexpr int DN = VrDim<CT>::DN, NP = VrDim<CT>::NP, PART = VrDim<CT>::PART, TRI = DN * (DN + 1) / 2;
  if (S->done || !S->active) return;      // (uniform)
  __shared__ double sp[PART], sH[DN * DN], sg[DN], Hc[DN * DN], gc[DN], Ad[DN * DN], Lm[DN * DN], rhs[DN], y[DN], scale[DN], diag2[DN];
  const int lane = threadIdx.x;
  for (int q = lane; q < PART; q += 64) {      // the partials in workgroup order
    double v = 0.0;
    for (int b = 0; b < G; b++) v += part[(size_t)b * PART + q];
    sp[q] = v;
  }
  for (int q = lane; q < DN * DN; q += 64) sH[q] = S->H[q];
  if (lane < DN) { sg[lane] = S->g[lane]; scale[lane] = S->scale[lane]; diag2[lane] = S->diag2[lane]; }
  __syncthreads();
  if (lane != 0) return;
  { int e = 0; for (int a = 0; a < DN; a++) for (int b = 0; b <= a; b++, e++) { Hc[a * DN + b] = sp[e]; Hc[b * DN + a] = sp[e]; } }
  for (int a = 0; a < DN; a++) gc[a] = sp[TRI + a];
  double cc = sp[TRI + DN];
  double x[14], xe[14];
  for (int i = 0; i < 14; i++) { x[i] = S->x[i]; xe[i] = S->xe[i]; }
  const int nres = S->nres;
  if (CT) {      // the consistency factors at xe, weight sqrt(n_res * beta * laser_point_cov), no loss
    if (O.b_loc > 0.0) {
      const double w = sqrt((double)nres * O.b_loc * O.cov);
      for (int a = 0; a < 3; a++) { const double r = w * (xe[a] - O.prev_t[a]); Hc[a * DN + a] += w * w; gc[a] += w * r; cc += 0.5 * r * r; }
    }
    if (O.b_rot > 0.0) {
      const double w = sqrt((double)nres * O.b_rot * O.cov);
      const double p2 = O.prev_q[0] * O.prev_q[0] + O.prev_q[1] * O.prev_q[1] + O.prev_q[2] * O.prev_q[2] + O.prev_q[3] * O.prev_q[3];
      const Qx qi = {-O.prev_q[0] / p2, -O.prev_q[1] / p2, -O.prev_q[2] / p2, O.prev_q[3] / p2};
      const Qx qt = qmulx(qi, {xe[3], xe[4], xe[5], xe[6]});
      const double r[3] = {2.0 * qt.x * w, 2.0 * qt.y * w, 2.0 * qt.z * w};
      const double J[9] = {w * qt.w, w * -qt.z, w * qt.y, w * qt.z, w * qt.w, w * -qt.x, w * -qt.y, w * qt.x, w * qt.w};      // w (q_w I + [q_v]x)
      for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) { double s = 0.0; for (int m = 0; m < 3; m++) s += J[3 * m + a] * J[3 * m + b]; Hc[(3 + a) * DN + 3 + b] += s; }
        double s = 0.0;
        for (int m = 0; m < 3; m++) s += J[3 * m + a] * r[m];
        gc[3 + a] += s;
        cc += 0.5 * r[a] * r[a];
      }
    }
    if (O.b_vel > 0.0) {
      const double w = sqrt((double)nres * O.b_vel * O.cov);
      for (int a = 0; a < 3; a++) {
        const double r = w * (xe[a] - xe[7 + a]);
        Hc[a * DN + a] += w * w; Hc[(6 + a) * DN + 6 + a] += w * w; Hc[a * DN + 6 + a] -= w * w; Hc[(6 + a) * DN + a] -= w * w;
        gc[a] += w * r; gc[6 + a] -= w * r; cc += 0.5 * r * r;
      }
    }
  }
  const int k = S->k;
  int it = S->it, invalid = S->invalid, reuse = S->reuse, acc_bits = S->acc_bits, term = -1, failed = 0;
  double cost = S->cost, radius = S->radius, decrease = S->decrease, x_norm = S->x_norm;
  auto take = [&]() { for (int q = 0; q < DN * DN; q++) sH[q] = Hc[q]; for (int a = 0; a < DN; a++) sg[a] = gc[a]; cost = cc; };
  auto norm_x = [&]() { double s = 0.0; for (int i = 0; i < NP; i++) s += x[i] * x[i]; return sqrt(s); };
  if (S->phase == 0) {      // the first linearisation of this inner solve
    take();
    S->s_c0[k] = cost;
    for (int a = 0; a < DN; a++) scale[a] = 1.0 / (1.0 + sqrt(sH[a * DN + a]));
    x_norm = norm_x();
  } else if (!isfinite(cc)) {      // a candidate without a finite cost is an invalid step, counted like a failed factorisation
    if (++invalid >= 5) { term = 4; failed = 1; }
    else { radius /= decrease; decrease *= 2.0; reuse = 1; }
  } else {                  // the candidate's cost is in: tolerances, step quality, radius
    invalid = 0;
    if (sqrt(S->step2) <= 1e-8 * (x_norm + 1e-8)) term = 2;
    else {
      const double change = cost - cc;
      if (fabs(change) <= 1e-6 * cost) term = 1;
      else {
        const double rho = change / S->model_change;
        if (rho > 1e-3) {
          for (int i = 0; i < 14; i++) x[i] = xe[i];
          take();
          x_norm = norm_x();
          acc_bits |= 1 << (it - 1);
          const double tq = 2.0 * rho - 1.0;
          radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - tq * tq * tq));
          decrease = 2.0; reuse = 0;
        } else { radius /= decrease; decrease *= 2.0; reuse = 1; }
      }
    }
  }
  bool pending = false;
  while (term < 0) {
    if (it >= O.L) { term = 0; break; }
    double gmax = 0.0;
    for (int a = 0; a < DN; a++) gmax = fmax(gmax, fabs(sg[a]));
    if (gmax <= 1e-10) { term = 3; break; }
    if (radius < 1e-32) { term = 4; break; }
    it++;
    for (int a = 0; a < DN; a++) {
      for (int b = 0; b < DN; b++) Ad[a * DN + b] = sH[a * DN + b] * scale[a] * scale[b];
      rhs[a] = -scale[a] * sg[a];
    }
    if (!reuse) for (int a = 0; a < DN; a++) diag2[a] = fmin(fmax(Ad[a * DN + a], 1e-6), 1e32);
    for (int q = 0; q < DN * DN; q++) Lm[q] = Ad[q];
    for (int a = 0; a < DN; a++) Lm[a * DN + a] += diag2[a] / radius;
    bool ok = true;
    for (int c = 0; c < DN && ok; c++) {      // Cholesky in place (lower)
      double ds = Lm[c * DN + c];
      for (int q = 0; q < c; q++) ds -= Lm[c * DN + q] * Lm[c * DN + q];
      if (!(ds > 0.0) || !isfinite(ds)) { ok = false; break; }
      const double lcc = sqrt(ds);
      Lm[c * DN + c] = lcc;
      for (int a = c + 1; a < DN; a++) { double s = Lm[a * DN + c]; for (int q = 0; q < c; q++) s -= Lm[a * DN + q] * Lm[c * DN + q]; Lm[a * DN + c] = s / lcc; }
    }
    double mc = 0.0;
    if (ok) {
      for (int a = 0; a < DN; a++) { double s = rhs[a]; for (int q = 0; q < a; q++) s -= Lm[a * DN + q] * y[q]; y[a] = s / Lm[a * DN + a]; }
      for (int a = DN - 1; a >= 0; a--) { double s = y[a]; for (int q = a + 1; q < DN; q++) s -= Lm[q * DN + a] * y[q]; y[a] = s / Lm[a * DN + a]; }
      double gy = 0.0, yHy = 0.0;
      for (int a = 0; a < DN; a++) {
        double s = 0.0;
        for (int b = 0; b < DN; b++) s += Ad[a * DN + b] * y[b];
        gy += -rhs[a] * y[a]; yHy += y[a] * s;
      }
      mc = -(gy + 0.5 * yHy);
    }
    if (!ok || !(mc > 0.0)) {      // an invalid step: a failed factorisation counts as a rejection
      if (++invalid >= 5) { term = 4; failed = 1; break; }
      radius /= decrease; decrease *= 2.0; reuse = 1;
      continue;
    }
    double d[12];
    for (int a = 0; a < DN; a++) d[a] = scale[a] * y[a];
    for (int i = 0; i < 14; i++) xe[i] = x[i];
    vr_plus(x, d, xe);
    if (CT) vr_plus(x + 7, d + 6, xe + 7);
    double s2 = 0.0;
    for (int i = 0; i < NP; i++) { const double df = xe[i] - x[i]; s2 += df * df; }
    S->step2 = s2; S->model_change = mc;
    pending = true;
    break;
  }
  // state back
  for (int q = 0; q < DN * DN; q++) S->H[q] = sH[q];
  for (int a = 0; a < DN; a++) { S->g[a] = sg[a]; S->scale[a] = scale[a]; S->diag2[a] = diag2[a]; }
  for (int i = 0; i < 14; i++) { S->x[i] = x[i]; S->xe[i] = xe[i]; }
  S->it = it; S->invalid = invalid; S->reuse = reuse; S->acc_bits = acc_bits; S->phase = 1;
  S->cost = cost; S->radius = radius; S->decrease = decrease; S->x_norm = x_norm;
  if (pending) return;
  // the inner solve has ended: the summary of this outer iteration, the exit test, the trace
  S->active = 0;
  S->s_it[k] = it; S->s_acc[k] = acc_bits; S->s_term[k] = term; S->s_c1[k] = cost;
  const double *x0 = S->x0;
  double dtr = 0.0, drot = 0.0;
  for (int h = 0; h < 2; h++) {
    const double *a = x0 + 7 * h, *b = x + 7 * h;
    dtr += sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
    drot += vr_angle(a + 3, b + 3);
  }
  S->s_dt[k] = dtr; S->s_dr[k] = drot;
  for (int i = 0; i < 14; i++) S->s_trace[k][i] = x[i];
  S->k = k + 1;
  if (failed) { S->failed = 1; S->done = 1; }
  else if (drot < O.thr_r && dtr < O.thr_t) { S->converged = 1; S->done = 1; }
  else if (k + 1 >= O.K) S->done = 1;
}

bool vr_options_ok(const gfbe_vreg_options *o) {
  return o->struct_size == (int32_t)sizeof(gfbe_vreg_options) && o->max_num_iteration >= 1 && o->max_num_iteration <= VR_MAXIT && o->lm_max_num_iterations >= 0 &&
         o->lm_max_num_iterations <= 16 && o->min_num_residuals >= 0 && o->laser_point_cov > 0.0 && std::isfinite(o->laser_point_cov) && std::isfinite(o->huber_delta) &&
         std::isfinite(o->beta_location_consistency) && std::isfinite(o->beta_orientation_consistency) && std::isfinite(o->beta_small_velocity) &&
         std::isfinite(o->thres_translation_norm) && std::isfinite(o->thres_orientation_norm);
}

}  // namespace

extern "C" {

void gfbe_vreg_default_options(gfbe_vreg_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = (int32_t)sizeof(gfbe_vreg_options);
  o->max_num_iteration = 10; o->lm_max_num_iterations = 5; o->min_num_residuals = 300; o->laser_point_cov = 0.001; o->huber_delta = 0.5;
  o->beta_location_consistency = 1.0; o->beta_orientation_consistency = 1.0; o->beta_small_velocity = 0.0;
  o->thres_translation_norm = 0.01; o->thres_orientation_norm = 0.1;
}

// what both fronts check before they stage anything: the context, the options, the map
static gfbe_status vr_front(gfbe_ctx *c, gfbe_vmap *m, const gfbe_vreg_options *opt, gfbe_vreg_options *o) {
  if (!c) return GFBE_BAD_INPUT;
  if (opt) { if (opt->struct_size != (int32_t)sizeof(gfbe_vreg_options)) return GFBE_BAD_INPUT; *o = *opt; }
  else gfbe_vreg_default_options(o);
  if (ctx_device(c) < 0) return GFBE_NO_DEVICE;
  if (!m) return GFBE_BAD_INPUT;
  if (!vr_options_ok(o)) { ctx_set_error(c, "gfbe_vmap_register: an option is outside its admitted range"); return GFBE_BAD_INPUT; }
  return GFBE_OK;
}

// The body: the loop on n keypoints already on the device (draw [n][3], dal [n]; n known to the host). sg: the map's staging chunk
// with whatever the front put into it, not yet flushed; the state and the partials go behind it, one copy up, one wait.
static gfbe_status vr_run(gfbe_ctx *c, gfbe_vmap *m, const gfbe_vreg_options &o, int ct, int n, Staged &sg, const double *draw, const double *dal,
                          const double *pose_begin, const double *pose_end, const double *prev_translation, const double *prev_rotation, int32_t frame_init,
                          double *pose_begin_out, double *pose_end_out, gfbe_vreg_summary *summary) {
  hipStream_t s = ctx_stream(c);
  m->assoc_valid = false;
  VrOpt O;
  O.ct = ct; O.K = o.max_num_iteration; O.L = o.lm_max_num_iterations; O.min_res = o.min_num_residuals;
  O.sqrt_info = std::sqrt(1.0 / o.laser_point_cov); O.huber = o.huber_delta; O.cov = o.laser_point_cov;
  O.b_loc = o.beta_location_consistency; O.b_rot = o.beta_orientation_consistency; O.b_vel = o.beta_small_velocity;
  O.thr_t = o.thres_translation_norm; O.thr_r = o.thres_orientation_norm;
  for (int a = 0; a < 3; a++) O.prev_t[a] = prev_translation ? prev_translation[a] : 0.0;
  for (int a = 0; a < 4; a++) O.prev_q[a] = prev_rotation ? prev_rotation[a] : (a == 3 ? 1.0 : 0.0);
  // grids by the bound of the residual count (the count itself is known only on the device)
  const long long bound = std::max<long long>(1, std::min<long long>((long long)n * m->opt.num_closest_neighbors, m->opt.max_num_residuals));
  const int G = (int)std::min<long long>(VR_MAXG, (bound + VR_THREADS - 1) / VR_THREADS);
  VrState hs;
  std::memset(&hs, 0, sizeof hs);
  std::memcpy(hs.x, pose_begin, sizeof(double) * 7);
  std::memcpy(hs.x + 7, pose_end ? pose_end : pose_begin, sizeof(double) * 7);
  gfbe_status st = GFBE_OK;
  {
    VrState *dS = sg.up(&hs, 1);
    double *dpart = sg.up<double>(nullptr, (size_t)VR_MAXG * VrDim<1>::PART);
    if (!sg.ok) { ctx_set_error(c, "gfbe_vmap_register: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    for (int k = 0; k < O.K && st == GFBE_OK; k++) {
      st = vmap_enqueue_assoc(c, m, ct, n, draw, dal, dS->x, dS->x + 7, frame_init, &dS->done);
      if (st != GFBE_OK) break;
      hipLaunchKernelGGL(k_vr_begin, dim3(1), dim3(1), 0, s, dS, (const int *)m->meta, O);
      for (int i = 0; i <= O.L; i++) {
        if (ct) {
          hipLaunchKernelGGL(k_vr_lin<1>, dim3(G), dim3(VR_THREADS), 0, s, dS, (const int *)m->meta, m->res_pts, m->res_nrm, m->res_off, m->res_al, m->res_w, O, dpart);
          hipLaunchKernelGGL(k_vr_step<1>, dim3(1), dim3(64), 0, s, dS, dpart, G, O);
        } else {
          hipLaunchKernelGGL(k_vr_lin<0>, dim3(G), dim3(VR_THREADS), 0, s, dS, (const int *)m->meta, m->res_pts, m->res_nrm, m->res_off, m->res_al, m->res_w, O, dpart);
          hipLaunchKernelGGL(k_vr_step<0>, dim3(1), dim3(64), 0, s, dS, dpart, G, O);
        }
      }
    }
    if (st == GFBE_OK) {
      vmap_enqueue_local(c, m, dS->local);
      sg.down(&hs, (const VrState *)dS, 1);
    }
    sg.finish();      // the one host wait
  }
  if (st != GFBE_OK) return st;
  if (hipGetLastError() != hipSuccess) { ctx_set_error(c, "gfbe_vmap_register: launch failed"); return GFBE_DEVICE_ERROR; }
  if (hs.overflow) { ctx_set_error(c, "voxel map capacity exceeded"); return GFBE_BAD_INPUT; }
  m->n_res = hs.nres; m->assoc_ct = ct; m->assoc_gen = m->gen; m->assoc_valid = true;
  std::memcpy(pose_begin_out, hs.x, sizeof(double) * 7);
  if (pose_end_out) std::memcpy(pose_end_out, hs.x + 7, sizeof(double) * 7);
  if (summary) {
    std::memset(summary, 0, sizeof(*summary));
    summary->outer_iterations = hs.k; summary->converged = hs.converged; summary->too_few_residuals = hs.too_few; summary->no_residuals = hs.no_res;
    summary->degenerate = hs.local[3] != 0.0;
    for (int a = 0; a < 3; a++) summary->sv[a] = hs.local[a];
    for (int k = 0; k < VR_MAXIT; k++) {
      summary->n_res[k] = hs.s_nres[k]; summary->lm_iterations[k] = hs.s_it[k]; summary->lm_accepted[k] = hs.s_acc[k]; summary->lm_termination[k] = hs.s_term[k];
      summary->cost_initial[k] = hs.s_c0[k]; summary->cost_final[k] = hs.s_c1[k]; summary->diff_trans[k] = hs.s_dt[k]; summary->diff_rot[k] = hs.s_dr[k];
      std::memcpy(summary->pose_trace[k], hs.s_trace[k], sizeof(double) * 14);
    }
  }
  if (hs.failed) { ctx_set_error(c, "gfbe_vmap_register: the inner solve produced no usable step"); return GFBE_NUMERICAL_FAILURE; }
  return GFBE_OK;
}

// the staging front of the host-fed call: the keypoints go up with the state
gfbe_status gfbe_vmap_register(gfbe_ctx *c, gfbe_vmap *m, const gfbe_vreg_options *opt, int32_t ct, int32_t n, const double *raw_pts, const double *alpha,
                               const double *pose_begin, const double *pose_end, const double *prev_translation, const double *prev_rotation, int32_t frame_init,
                               double *pose_begin_out, double *pose_end_out, gfbe_vreg_summary *summary) {
  gfbe_vreg_options o;
  const gfbe_status st = vr_front(c, m, opt, &o);
  if (st != GFBE_OK) return st;
  if (n < 0 || !pose_begin || !pose_begin_out || (n > 0 && !raw_pts) || (ct && (!pose_end || !pose_end_out || (n > 0 && !alpha)))) return GFBE_BAD_INPUT;
  ct = ct ? 1 : 0;
  const size_t N = (size_t)std::max(n, 1);
  Staged sg(c, m, N * 32 + sizeof(VrState) + sizeof(double) * VR_MAXG * VrDim<1>::PART + 8192);
  const double *draw = sg.up(raw_pts, 3 * (size_t)n), *dal = sg.up(ct ? alpha : nullptr, (size_t)n);
  return vr_run(c, m, o, ct, n, sg, draw, dal, pose_begin, pose_end, prev_translation, prev_rotation, frame_init, pose_begin_out, pose_end_out, summary);
}

// the same body on the KEYPOINTS of a scan handle: only the state goes up
gfbe_status gfbe_vmap_register_scan(gfbe_ctx *c, gfbe_vmap *m, const gfbe_vreg_options *opt, int32_t ct, gfbe_scan *scan, const double *pose_begin,
                                    const double *pose_end, const double *prev_translation, const double *prev_rotation, int32_t frame_init,
                                    double *pose_begin_out, double *pose_end_out, gfbe_vreg_summary *summary) {
  gfbe_vreg_options o;
  gfbe_status st = vr_front(c, m, opt, &o);
  if (st != GFBE_OK) return st;
  if (!scan || !pose_begin || !pose_begin_out || (ct && (!pose_end || !pose_end_out))) return GFBE_BAD_INPUT;
  ScanView sv;
  if ((st = scan_keypoints_view(c, scan, "gfbe_vmap_register_scan", &sv)) != GFBE_OK) return st;
  ct = ct ? 1 : 0;
  Staged sg(c, m, sizeof(VrState) + sizeof(double) * VR_MAXG * VrDim<1>::PART + 8192);
  return vr_run(c, m, o, ct, sv.n, sg, sv.pts, sv.alpha, pose_begin, pose_end, prev_translation, prev_rotation, frame_init, pose_begin_out, pose_end_out, summary);
}

}  // extern "C"
