// gfbe_gate.hip — the sensor gate for a batch of robots whose FeatureManager lists are the tables of a gfbe_ftab (gfbe_ftab.hip): the
// per-frame detectors of the reference and the wheel prediction of the newest frame, reading the tables in place.
//
//   the displacement test of processMeasurements, processIMU, processWheel     vins_estimator/src/estimator/estimator.cpp:681-705, :795-895    k_gate_interval
//   checkimu, checkimuexcited                                                 :2190-2280                                                      k_gate_interval
//   checkvisual / relativePose on getCorresponding(WithDepth)                  :2282-2335, :2118-2146, feature_manager.cpp:198-247             k_gate_pairs
//   systemstationary of processImage                                          :923-949                                                        k_gate_pairs, thread 0
//   the lists of getCorresponding(WithDepth)                                  feature_manager.cpp:198-247                                     k_gate_corres
//
// The rules are in gfbe_gate.h and include/gfbe_gate.h; every per-robot and per-feature statement is the header's function, compiled here
// for the device. k_gate_interval is serial per robot (a chain of dependent FP64 operations over the interval's samples): one lane per
// robot, 64 robots a workgroup, the samples read straight from global memory. It is latency-bound and is not there for throughput: its
// point is that the flags and the prediction are ready beside the tables behind the same wait. k_gate_pairs: one workgroup of 1024 per
// table on the current half of the ping-pong buffers; a thread walks its contiguous chunk of the list once, keeps the ten (count, sum)
// pairs in registers, the ten shuffle trees of a wave are interleaved and share one LDS round; thread 0 takes the decisions and, behind
// k_gate_interval on the same stream, G7. k_gate_corres: the order-preserving compaction of the erase kernels. No atomics, no scratch,
// no communication between workgroups inside a launch; the tables are never written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gfbe_gate.h"
#include "gfbe_device.h"
#include "gfbe_gate.h"
#include "gfbe_handle.h"

using namespace gfd;

static_assert(GATE_NL == GFBE_WINDOW_SIZE && GATE_NOBS == FT_NOBS && GATE_OW == FT_OW, "a row of the tables");
static_assert(GATE_F_ANOMALY == GFBE_GATE_WHEEL_ANOMALY && GATE_F_WHEEL == GFBE_GATE_WHEEL_STATIONARY && GATE_F_PREINT == GFBE_GATE_PREINT_STATIONARY &&
              GATE_F_VAR == GFBE_GATE_VAR_STATIONARY && GATE_F_EXCITED == GFBE_GATE_IMU_EXCITED && GATE_F_VISUAL == GFBE_GATE_VISUAL_STATIONARY &&
              GATE_F_IMU == GFBE_GATE_IMU_STATIONARY && GATE_F_SYSTEM == GFBE_GATE_SYSTEM_STATIONARY, "the header's bits");

struct gfbe_gate : gfbe_handle {
  gfbe_gate_options opt;
  int B = 0;
};

namespace {

// ---- G1 .. G4 -------------------------------------------------------------------------------------------------------------------------
struct GateIntervalArgs {
  int B;
  const int *frame_count, *imu_off, *wheel_off, *stationary_prev, *frames_off;      // wheel_* null with use_wheel == 0
  const double *imu, *imu_first, *wheel, *wheel_first, *pose, *vel_ba, *frames;
  double g_norm;
  double *res;      // [B][GATE_RES]
  int *iflags;      // [B] the bits of G3 and G4
};
__global__ __launch_bounds__(64) void k_gate_interval(GateParams G, GateIntervalArgs A) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= A.B) return;
  const int i0 = A.imu_off[b], ni = A.imu_off[b + 1] - i0, f0 = A.frames_off[b], M = A.frames_off[b + 1] - f0;
  const int w0 = G.use_wheel ? A.wheel_off[b] : 0, nw = G.use_wheel ? A.wheel_off[b + 1] - w0 : 0;
  const double *ws = G.use_wheel ? A.wheel + 7 * (size_t)w0 : nullptr, *wf = G.use_wheel ? A.wheel_first + 6 * (size_t)b : nullptr;
  double res[GATE_RES];
  A.iflags[b] = gate_interval(G, A.frame_count[b], A.imu + 7 * (size_t)i0, ni, A.imu_first + 6 * (size_t)b, ws, nw, wf,
                              A.pose + 12 * (size_t)b, A.vel_ba + 6 * (size_t)b, A.g_norm, A.stationary_prev[b], A.frames + 4 * (size_t)f0, M, res);
  for (int e = 0; e < GATE_RES; e++) A.res[GATE_RES * (size_t)b + e] = res[e];
}

// ---- G5 .. G7 -------------------------------------------------------------------------------------------------------------------------
struct GatePairsArgs {
  const int *iflags;      // [B] of k_gate_interval, or null: the table half alone
  int *count;             // [B][10]
  double *sum;            // [B][10]
  int *l_still, *l_init, *flags;      // [B]; flags null without iflags
};
__global__ __launch_bounds__(GATE_THREADS) void k_gate_pairs(FtabDev T, int cur, GateParams G, int mode, GatePairsArgs A) {
  __shared__ double s_sum[GATE_NL][GATE_THREADS / 64];
  __shared__ int s_cnt[GATE_NL][GATE_THREADS / 64];
  const int w = blockIdx.x, t = threadIdx.x;
  const int n = max(0, min(T.count[w], T.F));
  const size_t base = (size_t)w * T.F;
  const int *start = T.start[cur] + base, *nobs = T.nobs[cur] + base;
  const double *obs = T.obs[cur] + base * GATE_NOBS * GATE_OW;
  const int ch = (n + GATE_THREADS - 1) / GATE_THREADS, f0 = min(n, t * ch), f1 = min(n, f0 + ch);
  double sum[GATE_NL];
  int cnt[GATE_NL];
#pragma unroll
  for (int l = 0; l < GATE_NL; l++) { sum[l] = 0.0; cnt[l] = 0; }
  for (int f = f0; f < f1; f++) {
    const int s = start[f], nb = nobs[f];
    if (!gate_spans(s, nb, GATE_NL - 1, GATE_NL)) continue;      // (it spans to r from its start on)
    const double *row = obs + (size_t)f * GATE_NOBS * GATE_OW, *rp = row + (size_t)(GATE_NL - s) * GATE_OW;
    double rrow[GATE_OW];
#pragma unroll
    for (int q = 0; q < GATE_OW; q++) rrow[q] = rp[q];
#pragma unroll
    for (int l = 0; l < GATE_NL; l++) {
      if (l < s) continue;
      const double *lp = row + (size_t)(l - s) * GATE_OW;
      const double lrow[GATE_OW] = {lp[0], lp[1], lp[2], 0.0, 0.0, 0.0, 0.0, lp[7]};
      double a[3], b[3];
      if (gate_pair(G, mode, lrow, rrow, a, b)) { sum[l] = sum[l] + gate_term(mode, a, b); cnt[l]++; }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int l = 0; l < GATE_NL; l++) { sum[l] = sum[l] + __shfl_down(sum[l], o, 64); cnt[l] += __shfl_down(cnt[l], o, 64); }
  }
  if ((t & 63) == 0) {
#pragma unroll
    for (int l = 0; l < GATE_NL; l++) { s_sum[l][t >> 6] = sum[l]; s_cnt[l][t >> 6] = cnt[l]; }
  }
  __syncthreads();
  if (t != 0) return;
  int c[GATE_NL];
  double s[GATE_NL];
  for (int l = 0; l < GATE_NL; l++) {
    double a = 0.0;
    int k = 0;
    for (int q = 0; q < GATE_THREADS / 64; q++) { a = a + s_sum[l][q]; k += s_cnt[l][q]; }
    s[l] = a; c[l] = k;
    A.count[GATE_NL * (size_t)w + l] = k; A.sum[GATE_NL * (size_t)w + l] = a;
  }
  int ls, li;
  gate_decide(G, c, s, &ls, &li);
  A.l_still[w] = ls; A.l_init[w] = li;
  if (A.iflags) A.flags[w] = gate_system(A.iflags[w], ls);
}

// ---- G8 -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GATE_THREADS) void k_gate_corres(FtabDev T, int cur, GateParams G, int mode, const int *lv, const int *rv, const int *off, double *a3, double *b3,
                                                              int *count) {
  __shared__ int lds[20];
  const int w = blockIdx.x, t = threadIdx.x;
  const int n = max(0, min(T.count[w], T.F)), l = lv[w], r = rv[w], out = off[w], room = off[w + 1] - out;
  const size_t base = (size_t)w * T.F;
  const int *start = T.start[cur] + base, *nobs = T.nobs[cur] + base;
  const double *obs = T.obs[cur] + base * GATE_NOBS * GATE_OW;
  const int ch = (n + GATE_THREADS - 1) / GATE_THREADS, f0 = min(n, t * ch), f1 = min(n, f0 + ch);
  const bool ok = l >= 0 && l < r && r <= GATE_NL;      // (the host has checked it)
  int kept = 0, total;
  for (int f = f0; f < f1 && ok; f++) {
    const int s = start[f];
    if (!gate_spans(s, nobs[f], l, r)) continue;
    const double *row = obs + (size_t)f * GATE_NOBS * GATE_OW;
    double a[3], b[3];
    kept += gate_pair(G, mode, row + (size_t)(l - s) * GATE_OW, row + (size_t)(r - s) * GATE_OW, a, b) ? 1 : 0;
  }
  int dst = block_exclusive_scan<GATE_THREADS>(kept, &total, lds);
  for (int f = f0; f < f1 && ok; f++) {
    const int s = start[f];
    if (!gate_spans(s, nobs[f], l, r)) continue;
    const double *row = obs + (size_t)f * GATE_NOBS * GATE_OW;
    double a[3], b[3];
    if (!gate_pair(G, mode, row + (size_t)(l - s) * GATE_OW, row + (size_t)(r - s) * GATE_OW, a, b)) continue;
    if (dst < room) {
      const size_t p = 3 * ((size_t)out + (size_t)dst);
      for (int q = 0; q < 3; q++) { a3[p + q] = a[q]; b3[p + q] = b[q]; }
    }
    dst++;
  }
  if (t == 0) count[w] = total;
}

bool gate_fin(double v) { return std::isfinite(v); }
const char *gate_options_error(const gfbe_gate_options *o) {
  if (o->struct_size != (int32_t)sizeof(gfbe_gate_options)) return "gfbe_gate_options.struct_size does not match this library (ABI mismatch)";
  if (o->max_samples < 1 || o->max_samples > 65536) return "max_samples outside 1 .. 65536";
  if (o->max_frames < 1 || o->max_frames > 4096) return "max_frames outside 1 .. 4096";
  if (o->use_wheel < 0 || o->use_wheel > 1) return "use_wheel outside 0 .. 1";
  if (o->wdetect < 0 || o->wdetect > 1) return "wdetect outside 0 .. 1";
  if (o->depth_mode < 0 || o->depth_mode > 1) return "depth_mode outside 0 .. 1";
  if (o->min_pair_count < 0) return "min_pair_count < 0";
  if (!gate_fin(o->dis_threshold) || o->dis_threshold < 0.0) return "dis_threshold must be finite and >= 0";
  if (!gate_fin(o->wheel_still_norm) || o->wheel_still_norm < 0.0 || !gate_fin(o->preint_still_norm) || o->preint_still_norm < 0.0)
    return "wheel_still_norm / preint_still_norm must be finite and >= 0";
  if (!gate_fin(o->var_still) || !gate_fin(o->var_excited)) return "var_still / var_excited must be finite";
  if (!gate_fin(o->still_parallax_px) || !gate_fin(o->init_parallax_px)) return "still_parallax_px / init_parallax_px must be finite";
  if (!gate_fin(o->parallax_focal) || !(o->parallax_focal > 0.0)) return "parallax_focal must be finite and > 0";
  if (!gate_fin(o->depth_min) || !gate_fin(o->depth_max) || o->depth_max < o->depth_min) return "depth_min / depth_max must be finite and ordered";
  return nullptr;
}
GateParams gate_params(const gfbe_gate_options &o) {
  GateParams G;
  G.use_wheel = o.use_wheel; G.wdetect = o.wdetect; G.min_pair_count = o.min_pair_count; G.pad = 0;
  G.dis_threshold = o.dis_threshold; G.wheel_still_norm = o.wheel_still_norm; G.preint_still_norm = o.preint_still_norm; G.var_still = o.var_still;
  G.var_excited = o.var_excited; G.still_parallax_px = o.still_parallax_px; G.init_parallax_px = o.init_parallax_px; G.parallax_focal = o.parallax_focal;
  G.depth_min = o.depth_min; G.depth_max = o.depth_max;
  return G;
}
// offsets [B + 1] from 0, ascending, no list above `most` (most < 0: any length)
const char *gate_offsets_error(const int32_t *off, size_t B, int most) {
  if (off[0] != 0) return "offsets that do not ascend from 0";
  for (size_t b = 0; b < B; b++) {
    if (off[b + 1] < off[b]) return "offsets that do not ascend from 0";
    if (most >= 0 && off[b + 1] - off[b] > most) return "a list is longer than the handle's max_samples / max_frames";
  }
  return nullptr;
}
// the head of every call: the handle, then the tables it reads. Nothing is copied or launched before it has passed.
gfbe_status gate_ready(gfbe_ctx *c, gfbe_gate *m, gfbe_ftab *t, const char *who) {
  gfbe_status rc = handle_ready(c, m, who);
  if (rc != GFBE_OK) return rc;
  if (!t) return handle_bad(c, who, "ftab NULL");
  if (t->owner != c) return handle_bad(c, who, "the tables belong to another context");
  if (t->d.W != m->B) return handle_bad(c, who, "the table count is not the handle's n_robots");
  if (t->err_seen) return handle_bad(c, who, "a table's sticky error flag is set");
  return GFBE_OK;
}

}  // namespace

extern "C" {

void gfbe_gate_default_options(gfbe_gate_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = (int32_t)sizeof *o;
  o->max_samples = 256; o->max_frames = 64; o->use_wheel = 1; o->wdetect = 1; o->depth_mode = 1; o->min_pair_count = 20;
  o->dis_threshold = 0.02; o->wheel_still_norm = 0.001; o->preint_still_norm = 0.001; o->var_still = 0.1; o->var_excited = 0.35;
  o->still_parallax_px = 0.5; o->init_parallax_px = 30.0; o->parallax_focal = 460.0; o->depth_min = 0.1; o->depth_max = 10.0;
}

void gfbe_gate_destroy(gfbe_ctx *c, gfbe_gate *m) {
  if (!m) return;
  m->release(c);
  delete m;
}

gfbe_status gfbe_gate_create(gfbe_ctx *c, int32_t n_robots, const gfbe_gate_options *opt, gfbe_gate **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  gfbe_gate_options o;
  if (opt) o = *opt; else gfbe_gate_default_options(&o);
  if (const char *bad = gate_options_error(&o)) return handle_bad(c, "gfbe_gate_create", bad);
  if (n_robots < 1 || n_robots > 65536) return handle_bad(c, "gfbe_gate_create", "n_robots outside 1 .. 65536");
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_gate_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  gfbe_gate *m = new gfbe_gate();
  CreateGuard<gfbe_gate> guard{c, m, gfbe_gate_destroy};
  m->owner = c; m->opt = o; m->B = n_robots;
  // (the smallest chunk; a call stages 0.7 KiB a robot plus its samples and frames and grows the chunk when it needs to)
  if (!m->make_staging(c, "gfbe_gate_create", 0, false)) return GFBE_DEVICE_ERROR;
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  guard.armed = false;
  *out = m;
  return GFBE_OK;
}

gfbe_status gfbe_gate_frame(gfbe_ctx *c, gfbe_gate *m, gfbe_ftab *t, const int32_t *frame_count, const int32_t *imu_offset, const double *imu_samples, const double *imu_first,
                            const int32_t *wheel_offset, const double *wheel_samples, const double *wheel_first, const double *pose, const double *vel_ba, double g_norm,
                            const int32_t *stationary_prev, const int32_t *frames_offset, const double *frames, int32_t *flags, int32_t *l_still, int32_t *l_init,
                            int32_t *pair_count, double *pair_sum, double *dP_imu, double *dP_wheel, double *dis, double *var, double *pose_out, double *vel_out) {
  const char *who = "gfbe_gate_frame";
  gfbe_status rc = gate_ready(c, m, t, who);
  if (rc != GFBE_OK) return rc;
  const size_t B = (size_t)m->B;
  const bool wheel = m->opt.use_wheel != 0;
  if (!frame_count || !imu_offset || !imu_first || !pose || !vel_ba || !stationary_prev || !frames_offset)
    return handle_bad(c, who, "frame_count, imu_offset, imu_first, pose, vel_ba, stationary_prev or frames_offset NULL");
  if (wheel && (!wheel_offset || !wheel_first)) return handle_bad(c, who, "use_wheel == 1 needs wheel_offset and wheel_first");
  if (const char *bad = gate_offsets_error(imu_offset, B, m->opt.max_samples)) return handle_bad(c, who, bad);
  if (wheel)
    if (const char *bad = gate_offsets_error(wheel_offset, B, m->opt.max_samples)) return handle_bad(c, who, bad);
  if (const char *bad = gate_offsets_error(frames_offset, B, m->opt.max_frames)) return handle_bad(c, who, bad);
  const size_t nI = (size_t)imu_offset[B], nW = wheel ? (size_t)wheel_offset[B] : 0, nF = (size_t)frames_offset[B];
  if ((nI > 0 && !imu_samples) || (nW > 0 && !wheel_samples) || (nF > 0 && !frames)) return handle_bad(c, who, "imu_samples, wheel_samples or frames NULL");
  if ((rc = ftab_ready(c, t)) != GFBE_OK) return rc;
  std::vector<double> res(GATE_RES * B);
  {
    Staged sg(c, m, (nI + nW) * 56 + nF * 32 + B * (8 * (GATE_RES + 12 + 6 + 12 + GATE_NL) + 4 * (10 + GATE_NL)) + 24 * 256 + 8192);
    GateIntervalArgs A;
    std::memset(&A, 0, sizeof A);
    A.B = m->B; A.g_norm = g_norm;
    A.frame_count = sg.up((const int *)frame_count, B); A.imu_off = sg.up((const int *)imu_offset, B + 1); A.stationary_prev = sg.up((const int *)stationary_prev, B);
    A.frames_off = sg.up((const int *)frames_offset, B + 1);
    A.imu = sg.up(imu_samples, 7 * nI); A.imu_first = sg.up(imu_first, 6 * B); A.pose = sg.up(pose, 12 * B); A.vel_ba = sg.up(vel_ba, 6 * B); A.frames = sg.up(frames, 4 * nF);
    if (wheel) { A.wheel_off = sg.up((const int *)wheel_offset, B + 1); A.wheel = sg.up(wheel_samples, 7 * nW); A.wheel_first = sg.up(wheel_first, 6 * B); }
    A.res = sg.up((const double *)nullptr, GATE_RES * B);
    A.iflags = sg.up((const int *)nullptr, B);
    GatePairsArgs P;
    P.iflags = A.iflags; P.count = sg.up((const int *)nullptr, GATE_NL * B); P.sum = sg.up((const double *)nullptr, GATE_NL * B);
    P.l_still = sg.up((const int *)nullptr, B); P.l_init = sg.up((const int *)nullptr, B); P.flags = sg.up((const int *)nullptr, B);
    if (!sg.ok) { ctx_set_error(c, "gfbe_gate_frame: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    const GateParams G = gate_params(m->opt);
    hipLaunchKernelGGL(k_gate_interval, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, ctx_stream(c), G, A);
    hipLaunchKernelGGL(k_gate_pairs, dim3((unsigned)B), dim3(GATE_THREADS), 0, ctx_stream(c), t->d, t->cur, G, (int)m->opt.depth_mode, P);
    sg.down(res.data(), (const double *)A.res, GATE_RES * B);
    sg.down(flags, (const int32_t *)P.flags, B); sg.down(l_still, (const int32_t *)P.l_still, B); sg.down(l_init, (const int32_t *)P.l_init, B);
    sg.down(pair_count, (const int32_t *)P.count, GATE_NL * B); sg.down(pair_sum, (const double *)P.sum, GATE_NL * B);
    sg.finish();      // the one wait
    GFBE_CHECK(c, hipGetLastError());
  }
  for (size_t b = 0; b < B; b++) {
    const double *r = res.data() + GATE_RES * b;
    if (dP_imu) std::memcpy(dP_imu + 3 * b, r + GATE_R_DPI, sizeof(double) * 3);
    if (dP_wheel) std::memcpy(dP_wheel + 3 * b, r + GATE_R_DPW, sizeof(double) * 3);
    if (dis) dis[b] = r[GATE_R_DIS];
    if (var) var[b] = r[GATE_R_VAR];
    if (pose_out) std::memcpy(pose_out + 12 * b, r + GATE_R_POSE, sizeof(double) * 12);
    if (vel_out) std::memcpy(vel_out + 3 * b, r + GATE_R_VEL, sizeof(double) * 3);
  }
  return GFBE_OK;
}

gfbe_status gfbe_gate_pair_stats(gfbe_ctx *c, gfbe_gate *m, gfbe_ftab *t, int32_t mode, int32_t *pair_count, double *pair_sum, int32_t *l_still, int32_t *l_init) {
  const char *who = "gfbe_gate_pair_stats";
  gfbe_status rc = gate_ready(c, m, t, who);
  if (rc != GFBE_OK) return rc;
  if (mode < 0 || mode > 1) return handle_bad(c, who, "mode outside 0 .. 1");
  if ((rc = ftab_ready(c, t)) != GFBE_OK) return rc;
  const size_t B = (size_t)m->B;
  Staged sg(c, m, B * (12 * GATE_NL + 8) + 4 * 256 + 8192);
  GatePairsArgs P;
  P.iflags = nullptr; P.flags = nullptr;
  P.count = sg.up((const int *)nullptr, GATE_NL * B); P.sum = sg.up((const double *)nullptr, GATE_NL * B);
  P.l_still = sg.up((const int *)nullptr, B); P.l_init = sg.up((const int *)nullptr, B);
  if (!sg.ok) { ctx_set_error(c, "gfbe_gate_pair_stats: staging allocation failed"); return GFBE_DEVICE_ERROR; }
  hipLaunchKernelGGL(k_gate_pairs, dim3((unsigned)B), dim3(GATE_THREADS), 0, ctx_stream(c), t->d, t->cur, gate_params(m->opt), (int)mode, P);
  sg.down(pair_count, (const int32_t *)P.count, GATE_NL * B); sg.down(pair_sum, (const double *)P.sum, GATE_NL * B);
  sg.down(l_still, (const int32_t *)P.l_still, B); sg.down(l_init, (const int32_t *)P.l_init, B);
  sg.finish();      // the one wait
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_gate_corresponding(gfbe_ctx *c, gfbe_gate *m, gfbe_ftab *t, int32_t mode, const int32_t *l, const int32_t *r, const int32_t *offset, double *a, double *b,
                                    int32_t *count) {
  const char *who = "gfbe_gate_corresponding";
  gfbe_status rc = gate_ready(c, m, t, who);
  if (rc != GFBE_OK) return rc;
  if (mode < 0 || mode > 1) return handle_bad(c, who, "mode outside 0 .. 1");
  if (!l || !r || !offset) return handle_bad(c, who, "l, r or offset NULL");
  const size_t B = (size_t)m->B;
  if (const char *bad = gate_offsets_error(offset, B, -1)) return handle_bad(c, who, bad);
  for (size_t q = 0; q < B; q++)
    if (!(l[q] >= 0 && l[q] < r[q] && r[q] <= GATE_NL)) return handle_bad(c, who, "l / r outside 0 <= l < r <= WINDOW_SIZE");
  const size_t n = (size_t)offset[B];
  if (n > 0 && (!a || !b)) return handle_bad(c, who, "a or b NULL");
  if ((rc = ftab_ready(c, t)) != GFBE_OK) return rc;
  // a and b come back through vectors of the call: on too little room nothing but count is written
  std::vector<double> ah(3 * n), bh(3 * n);
  std::vector<int32_t> cnt(B, 0);
  {
    Staged sg(c, m, n * 48 + B * 16 + 8 * 256 + 8192);
    const int *d_l = sg.up((const int *)l, B), *d_r = sg.up((const int *)r, B), *d_off = sg.up((const int *)offset, B + 1);
    double *d_a = sg.up((const double *)nullptr, 3 * n), *d_b = sg.up((const double *)nullptr, 3 * n);
    int *d_cnt = sg.up((const int *)nullptr, B);
    if (!sg.ok) { ctx_set_error(c, "gfbe_gate_corresponding: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    hipLaunchKernelGGL(k_gate_corres, dim3((unsigned)B), dim3(GATE_THREADS), 0, ctx_stream(c), t->d, t->cur, gate_params(m->opt), (int)mode, d_l, d_r, d_off, d_a, d_b, d_cnt);
    sg.down(cnt.data(), (const int32_t *)d_cnt, B);
    sg.down(ah.data(), (const double *)d_a, 3 * n); sg.down(bh.data(), (const double *)d_b, 3 * n);
    sg.finish();      // the one wait
    GFBE_CHECK(c, hipGetLastError());
  }
  if (count) std::memcpy(count, cnt.data(), sizeof(int32_t) * B);
  for (size_t q = 0; q < B; q++)
    if (cnt[q] > offset[q + 1] - offset[q]) return handle_bad(c, who, "a table has more pairs than room (count is written)");
  // (rows past a table's count are not the caller's to read: only the pairs are copied)
  for (size_t q = 0; q < B; q++) {
    const size_t o = 3 * (size_t)offset[q], k = 3 * (size_t)std::max(cnt[q], 0);
    if (k) { std::memcpy(a + o, ah.data() + o, sizeof(double) * k); std::memcpy(b + o, bh.data() + o, sizeof(double) * k); }
  }
  return GFBE_OK;
}

}  // extern "C"
