// gfbe_gate.h — the rules of the sensor gate (gfbe_gate.hip) that need no HIP header: under a plain C++ compiler they are ordinary inline
// functions, under hipcc the per-robot and per-feature ones are __host__ __device__ (tests/gate_host_shim.cpp compiles them for the host).
// The rules G1 .. G8 are stated in include/gfbe_gate.h; citations are to
//
//   Estimator::processMeasurements, the displacement test          vins_estimator/src/estimator/estimator.cpp:681-705
//   Estimator::processIMU, processWheel                            :795-836, :837-895
//   Estimator::processImage, checkimu, checkimuexcited, checkvisual  :923-949, :2190-2335
//   FeatureManager::getCorresponding, getCorrespondingWithDepth    vins_estimator/src/estimator/feature_manager.cpp:198-247
//
// Everything here is FP64 + - * /, sqrt and comparisons, every expression written once and compiled without contraction. The model
// tests/gate_np.py reproduces every function bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GF_GATE_HD __host__ __device__ inline
#else
#define GF_GATE_HD inline
#endif

namespace gfd {

constexpr int GATE_NL = 10;               // pairs of a table: l = 0 .. WINDOW_SIZE - 1 against r = WINDOW_SIZE
constexpr int GATE_NOBS = GATE_NL + 1;    // observation slots of a feature (FT_NOBS)
constexpr int GATE_OW = 8;                // doubles of an observation row (FT_OW): x y z u v vx vy depth
constexpr int GATE_THREADS = 1024;        // the workgroup of a table kernel: G5's sum order is stated on it
constexpr int GATE_RES = 23;              // doubles a robot's interval brings back: dP_imu, dP_wheel, dis, var, P, R, V
enum { GATE_R_DPI = 0, GATE_R_DPW = 3, GATE_R_DIS = 6, GATE_R_VAR = 7, GATE_R_POSE = 8, GATE_R_VEL = 20 };
// the flag bits (GFBE_GATE_* of include/gfbe_gate.h)
enum { GATE_F_ANOMALY = 1, GATE_F_WHEEL = 2, GATE_F_PREINT = 4, GATE_F_VAR = 8, GATE_F_EXCITED = 16, GATE_F_VISUAL = 32, GATE_F_IMU = 64, GATE_F_SYSTEM = 128 };

struct GateParams {                        // the options a kernel needs
  int use_wheel, wdetect, min_pair_count, pad;
  double dis_threshold, wheel_still_norm, preint_still_norm, var_still, var_excited, still_parallax_px, init_parallax_px, parallax_focal, depth_min, depth_max;
};

GF_GATE_HD double gate_dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
GF_GATE_HD double gate_norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }
// row-major 3 x 3 times a vector
GF_GATE_HD void gate_rot(const double *R, double x, double y, double z, double *o) {
  o[0] = gate_dot3(R[0], R[1], R[2], x, y, z); o[1] = gate_dot3(R[3], R[4], R[5], x, y, z); o[2] = gate_dot3(R[6], R[7], R[8], x, y, z);
}

// ---- G1 (estimator.cpp:811-833): R and V stay, both accelerations turn by the same R ---------------------------------------------------
GF_GATE_HD void gate_dp_imu(int frame_count, const double *imu, int n, const double *first, const double *R, const double *V, const double *ba, double g_norm, double *dP) {
  dP[0] = dP[1] = dP[2] = 0.0;
  if (frame_count == 0) return;
  double a0x = first[0], a0y = first[1], a0z = first[2];
  for (int k = 0; k < n; k++) {
    const double *s = imu + 7 * (size_t)k;
    const double dt = s[0];
    double u0[3], u1[3];
    gate_rot(R, a0x - ba[0], a0y - ba[1], a0z - ba[2], u0);
    gate_rot(R, s[1] - ba[0], s[2] - ba[1], s[3] - ba[2], u1);
    u0[2] = u0[2] - g_norm; u1[2] = u1[2] - g_norm;      // (g = (0, 0, g_norm): x - 0.0 is x)
    const double h = (0.5 * dt) * dt;
    for (int a = 0; a < 3; a++) dP[a] = (dP[a] + dt * V[a]) + h * (0.5 * (u0[a] + u1[a]));
    a0x = s[1]; a0y = s[2]; a0z = s[3];
  }
}

// ---- G2 (estimator.cpp:850-891, utility.h:23-35, Eigen's toRotationMatrix written out): P [3], R [9], V [3] are updated in place ----------
GF_GATE_HD void gate_delta_rot(double tx_, double ty_, double tz_, double *M) {      // M(normalize(1, theta / 2))
  const double hx = tx_ / 2.0, hy = ty_ / 2.0, hz = tz_ / 2.0;
  const double nrm = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
  const double w = 1.0 / nrm, x = hx / nrm, y = hy / nrm, z = hz / nrm;
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  M[0] = 1.0 - (tyy + tzz); M[1] = txy - twz; M[2] = txz + twy;
  M[3] = txy + twz; M[4] = 1.0 - (txx + tzz); M[5] = tyz - twx;
  M[6] = txz - twy; M[7] = tyz + twx; M[8] = 1.0 - (txx + tyy);
}
GF_GATE_HD void gate_wheel(int frame_count, const double *wheel, int n, const double *first, int stationary, double *P, double *R, double *V, double *dPw) {
  dPw[0] = dPw[1] = dPw[2] = 0.0;
  if (frame_count == 0) return;
  double v0x = first[0], v0y = first[1], v0z = first[2], g0x = first[3], g0y = first[4], g0z = first[5];
  for (int k = 0; k < n; k++) {
    const double *s = wheel + 7 * (size_t)k;
    const double dt = s[0];
    const double ux = 0.5 * (g0x + s[4]), uy = 0.5 * (g0y + s[5]), uz = 0.5 * (g0z + s[6]);
    double uv0[3];
    gate_rot(R, v0x, v0y, v0z, uv0);      // (the R from before the update)
    if (!stationary) {
      double M[9], Rn[9], Rv[3];
      gate_delta_rot(ux * dt, uy * dt, uz * dt, M);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rn[3 * i + j] = gate_dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], M[j], M[3 + j], M[6 + j]);
      for (int e = 0; e < 9; e++) R[e] = Rn[e];
      gate_rot(R, s[1], s[2], s[3], Rv);
      for (int a = 0; a < 3; a++) { V[a] = 0.5 * (Rv[a] + uv0[a]); P[a] = P[a] + dt * V[a]; }
    } else {
      V[0] = V[1] = V[2] = 0.0;
    }
    dPw[0] = dPw[0] - dt * V[1];
    dPw[1] = dPw[1] + dt * V[0];
    dPw[2] = dPw[2] - dt * V[2];
    v0x = s[1]; v0y = s[2]; v0z = s[3]; g0x = s[4]; g0y = s[5]; g0z = s[6];
  }
}

// ---- G4 (estimator.cpp:2234-2280, :2190-2232): frames [M][4] = delta_v, sum_dt in map order; no guard, a NaN comes back as the one quiet NaN
// any NaN -> 0x7FF8000000000000, on the bits: a floating-point select between two NaNs is the compiler's to simplify
GF_GATE_HD double gate_one_nan(double v) {
  uint64_t u;
  __builtin_memcpy(&u, &v, sizeof u);
  if ((u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) u = 0x7FF8000000000000ull;
  __builtin_memcpy(&v, &u, sizeof u);
  return v;
}
GF_GATE_HD double gate_var(const double *frames, int M) {
  const double den = (double)(M - 1);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int f = 1; f < M; f++) {
    const double *q = frames + 4 * (size_t)f;
    sx = sx + q[0] / q[3]; sy = sy + q[1] / q[3]; sz = sz + q[2] / q[3];
  }
  const double ax = sx / den, ay = sy / den, az = sz / den;
  double var = 0.0;
  for (int f = 1; f < M; f++) {
    const double *q = frames + 4 * (size_t)f;
    const double dx = q[0] / q[3] - ax, dy = q[1] / q[3] - ay, dz = q[2] / q[3] - az;
    var = var + ((dx * dx + dy * dy) + dz * dz);
  }
  return gate_one_nan(sqrt(var / den));
}

// ---- G1 .. G4 of one robot: res [GATE_RES]; returns the flag bits of G3 and G4 ---------------------------------------------------------------
GF_GATE_HD int gate_interval(const GateParams &G, int frame_count, const double *imu, int n_imu, const double *imu_first, const double *wheel, int n_wheel,
                             const double *wheel_first, const double *pose, const double *vel_ba, double g_norm, int stationary_prev, const double *frames, int M, double *res) {
  double P[3], R[9], V[3], dPi[3], dPw[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < 3; a++) { P[a] = pose[a]; V[a] = vel_ba[a]; }
  for (int e = 0; e < 9; e++) R[e] = pose[3 + e];
  gate_dp_imu(frame_count, imu, n_imu, imu_first, R, V, vel_ba + 3, g_norm, dPi);
  if (G.use_wheel) gate_wheel(frame_count, wheel, n_wheel, wheel_first, stationary_prev, P, R, V, dPw);
  const double dis = gate_norm3(dPw[0] - dPi[0], dPw[1] - dPi[1], dPw[2] - dPi[2]);
  const double var = gate_var(frames, M);
  int flags = 0;
  if (G.use_wheel) {
    if (G.wdetect && dis > G.dis_threshold) flags |= GATE_F_ANOMALY;
    if (gate_norm3(dPw[0], dPw[1], dPw[2]) < G.wheel_still_norm) flags |= GATE_F_WHEEL;
    if (gate_norm3(dPi[0], dPi[1], dPi[2]) < G.preint_still_norm) flags |= GATE_F_PREINT;
  }
  if (var < G.var_still) flags |= GATE_F_VAR;
  if (!(var < G.var_excited)) flags |= GATE_F_EXCITED;
  for (int a = 0; a < 3; a++) { res[GATE_R_DPI + a] = dPi[a]; res[GATE_R_DPW + a] = dPw[a]; res[GATE_R_POSE + a] = P[a]; res[GATE_R_VEL + a] = V[a]; }
  for (int e = 0; e < 9; e++) res[GATE_R_POSE + 3 + e] = R[e];
  res[GATE_R_DIS] = dis; res[GATE_R_VAR] = var;
  return flags;
}

// ---- G5, G8: one feature in one pair. lrow / rrow: its observation rows of frames l and r. False: the depth test of mode 1 drops it. ---------
GF_GATE_HD bool gate_spans(int start, int nobs, int l, int r) { return start >= 0 && nobs <= GATE_NOBS && start <= l && start + nobs - 1 >= r; }
GF_GATE_HD bool gate_depth_ok(const GateParams &G, double d) { return !(d < G.depth_min || d > G.depth_max); }
GF_GATE_HD bool gate_pair(const GateParams &G, int mode, const double *lrow, const double *rrow, double *a, double *b) {
  if (mode == 0) {
    for (int q = 0; q < 3; q++) { a[q] = lrow[q]; b[q] = rrow[q]; }
    return true;
  }
  const double dl = lrow[7], dr = rrow[7];
  if (!gate_depth_ok(G, dl) || !gate_depth_ok(G, dr)) return false;
  for (int q = 0; q < 3; q++) { a[q] = lrow[q] * dl; b[q] = rrow[q] * dr; }
  return true;
}
GF_GATE_HD double gate_term(int mode, const double *a, const double *b) {
  double du, dv;
  if (mode == 0) { du = a[0] - b[0]; dv = a[1] - b[1]; }
  else { du = a[0] / a[2] - b[0] / b[2]; dv = a[1] / a[2] - b[1] / b[2]; }
  return sqrt(du * du + dv * dv);
}

// ---- G6, G7 ----------------------------------------------------------------------------------------------------------------------------------
GF_GATE_HD void gate_decide(const GateParams &G, const int *count, const double *sum, int *l_still, int *l_init) {
  int ls = -1, li = -1;
  for (int l = 0; l < GATE_NL; l++) {
    if (!(count[l] > G.min_pair_count)) continue;
    const double px = sum[l] / (double)count[l] * G.parallax_focal;
    if (ls < 0 && px < G.still_parallax_px) ls = l;
    if (li < 0 && px > G.init_parallax_px) li = l;
  }
  *l_still = ls; *l_init = li;
}
GF_GATE_HD int gate_system(int flags, int l_still) {
  int f = flags & (GATE_F_ANOMALY | GATE_F_WHEEL | GATE_F_PREINT | GATE_F_VAR | GATE_F_EXCITED);
  const bool wheel = (f & GATE_F_WHEEL) != 0, visual = l_still >= 0, imu = (f & GATE_F_VAR) != 0 && (f & GATE_F_PREINT) != 0;
  if (visual) f |= GATE_F_VISUAL;
  if (imu) f |= GATE_F_IMU;
  if ((imu && wheel) || (visual && wheel) || (imu && visual)) f |= GATE_F_SYSTEM;
  return f;
}

// ---- the table half on the host, in the device's sum order (G5): thread t of 1024 owns the chunk [t ch, (t + 1) ch), ch = ceil(n / 1024); the
//      64 partials of a wave go through s += shfl_down(s, o), o = 32 .. 1 (lane 0 keeps the wave's sum), the 16 wave sums are added in order.
//      start / nobs [n], obs [n][11][8] of one table; count / sum [10]. For the host build of the tests and the host leg of the benchmark.
inline void gate_pairs_host(const GateParams &G, int mode, int n, const int *start, const int *nobs, const double *obs, int *count, double *sum) {
  const int ch = (n + GATE_THREADS - 1) / GATE_THREADS;
  for (int l = 0; l < GATE_NL; l++) {
    double wave[GATE_THREADS / 64];
    int cnt = 0;
    for (int w = 0; w < GATE_THREADS / 64; w++) {
      double lane[64];
      for (int q = 0; q < 64; q++) {
        const int t = 64 * w + q;
        const long long f0 = (long long)t * ch, f1 = f0 + ch < n ? f0 + ch : n;
        double s = 0.0;
        for (long long f = f0; f < f1; f++) {
          if (!gate_spans(start[f], nobs[f], l, GATE_NL)) continue;
          const double *row = obs + (size_t)f * GATE_NOBS * GATE_OW;
          double a[3], b[3];
          if (!gate_pair(G, mode, row + (size_t)(l - start[f]) * GATE_OW, row + (size_t)(GATE_NL - start[f]) * GATE_OW, a, b)) continue;
          s = s + gate_term(mode, a, b);
          cnt++;
        }
        lane[q] = s;
      }
      for (int o = 32; o >= 1; o >>= 1)
        for (int q = 0; q < o; q++) lane[q] = lane[q] + lane[q + o];
      wave[w] = lane[0];
    }
    double s = 0.0;
    for (int w = 0; w < GATE_THREADS / 64; w++) s = s + wave[w];
    count[l] = cnt; sum[l] = s;
  }
}
// gfbe_gate_frame on the host, one robot after the other: the tables packed (table b at rows toff[b] .. toff[b + 1] of start / nobs / obs), the
// other arguments and the outputs as the entry point's (any output may be null; wheel_* null with use_wheel == 0)
inline void gate_frame_host(const GateParams &G, int mode, int B, const int *toff, const int *start, const int *nobs, const double *obs, const int *frame_count,
                            const int *imu_off, const double *imu, const double *imu_first, const int *wheel_off, const double *wheel, const double *wheel_first,
                            const double *pose, const double *vel_ba, double g_norm, const int *stationary_prev, const int *frames_off, const double *frames, int *flags,
                            int *l_still, int *l_init, int *pair_count, double *pair_sum, double *dP_imu, double *dP_wheel, double *dis, double *var, double *pose_out,
                            double *vel_out) {
  for (int b = 0; b < B; b++) {
    const size_t q = (size_t)b;
    double res[GATE_RES], sum[GATE_NL];
    int count[GATE_NL], ls, li;
    const int nw = G.use_wheel ? wheel_off[b + 1] - wheel_off[b] : 0;
    const int f = gate_interval(G, frame_count[b], imu + 7 * (size_t)imu_off[b], imu_off[b + 1] - imu_off[b], imu_first + 6 * q,
                                G.use_wheel ? wheel + 7 * (size_t)wheel_off[b] : nullptr, nw, G.use_wheel ? wheel_first + 6 * q : nullptr, pose + 12 * q, vel_ba + 6 * q, g_norm,
                                stationary_prev[b], frames + 4 * (size_t)frames_off[b], frames_off[b + 1] - frames_off[b], res);
    gate_pairs_host(G, mode, toff[b + 1] - toff[b], start + toff[b], nobs + toff[b], obs + (size_t)toff[b] * GATE_NOBS * GATE_OW, count, sum);
    gate_decide(G, count, sum, &ls, &li);
    if (flags) flags[b] = gate_system(f, ls);
    if (l_still) l_still[b] = ls;
    if (l_init) l_init[b] = li;
    for (int l = 0; l < GATE_NL; l++) { if (pair_count) pair_count[GATE_NL * q + l] = count[l]; if (pair_sum) pair_sum[GATE_NL * q + l] = sum[l]; }
    for (int a = 0; a < 3; a++) { if (dP_imu) dP_imu[3 * q + a] = res[GATE_R_DPI + a]; if (dP_wheel) dP_wheel[3 * q + a] = res[GATE_R_DPW + a]; if (vel_out) vel_out[3 * q + a] = res[GATE_R_VEL + a]; }
    if (dis) dis[b] = res[GATE_R_DIS];
    if (var) var[b] = res[GATE_R_VAR];
    if (pose_out) for (int e = 0; e < 12; e++) pose_out[12 * q + e] = res[GATE_R_POSE + e];
  }
}
// G8 of one table on the host: the pairs of (l, r) in list order; returns their number, writes at most `room`
inline int gate_corres_host(const GateParams &G, int mode, int n, const int *start, const int *nobs, const double *obs, int l, int r, int room, double *a3, double *b3) {
  int k = 0;
  for (int f = 0; f < n; f++) {
    if (!gate_spans(start[f], nobs[f], l, r)) continue;
    const double *row = obs + (size_t)f * GATE_NOBS * GATE_OW;
    double a[3], b[3];
    if (!gate_pair(G, mode, row + (size_t)(l - start[f]) * GATE_OW, row + (size_t)(r - start[f]) * GATE_OW, a, b)) continue;
    if (k < room)
      for (int q = 0; q < 3; q++) { a3[3 * (size_t)k + q] = a[q]; b3[3 * (size_t)k + q] = b[q]; }
    k++;
  }
  return k;
}

}  // namespace gfd
