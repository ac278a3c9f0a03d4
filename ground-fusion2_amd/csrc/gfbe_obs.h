// gfbe_obs.h — the rules of the frame observations (gfbe_obs.hip) that need no HIP header: under a plain C++ compiler they are ordinary
// inline functions, under hipcc the per-point ones are __host__ __device__ (tests/obs_host_shim.cpp compiles them for the host).
// The rules O1 .. O8 are stated in include/gfbe_obs.h; citations are to
//
//   PinholeCamera::liftProjective, spaceToPlane, distortion      camera_models/src/camera_models/PinholeCamera.cc:450-510, :520-542, :646-662
//   FeatureTracker::undistortedPts, ptsVelocity, trackImage      vins_estimator/src/featureTracker/feature_tracker.cpp:797-808, :810-847, :320-368
//   Estimator::predictPtsInNextFrame                             vins_estimator/src/estimator/estimator.cpp:3927-3946
//
// Every statement is double or single precision in the order written here. There is no multiply-add: the build has
// -ffp-contract=off. The model tests/obs_np.py reproduces every function bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gfbe_klt.h"

#define GF_OBS_HD GF_KLT_HD

namespace gfd {

constexpr int OBS_MAX_POINTS = 2048;      // GFBE_DET_MAX_POINTS: held points a camera
constexpr int OBS_OW = 8;                 // a row of O6

// ---- O1 ---------------------------------------------------------------------------------------------------------------------------
struct ObsCam {
  double fx, fy, cx, cy, k1, k2, p1, p2;
  double inv_K11, inv_K13, inv_K22, inv_K23;
  int no_distortion;
};
GF_OBS_HD ObsCam obs_camera(const double *p /* fx fy cx cy k1 k2 p1 p2 */) {
  ObsCam c;
  c.fx = p[0]; c.fy = p[1]; c.cx = p[2]; c.cy = p[3]; c.k1 = p[4]; c.k2 = p[5]; c.p1 = p[6]; c.p2 = p[7];
  c.inv_K11 = 1.0 / c.fx; c.inv_K13 = -c.cx / c.fx; c.inv_K22 = 1.0 / c.fy; c.inv_K23 = -c.cy / c.fy;
  c.no_distortion = (c.k1 == 0.0 && c.k2 == 0.0 && c.p1 == 0.0 && c.p2 == 0.0) ? 1 : 0;
  return c;
}
GF_OBS_HD bool obs_finite(double v) { return v - v == 0.0; }      // (neither an infinity nor a NaN)
GF_OBS_HD bool obs_camera_ok(const double *p) {
  for (int k = 0; k < 8; k++)
    if (!obs_finite(p[k])) return false;
  return p[0] != 0.0 && p[1] != 0.0;
}

// ---- O2 ---------------------------------------------------------------------------------------------------------------------------
GF_OBS_HD void obs_distortion(const ObsCam &c, double x, double y, double *dx, double *dy) {
  const double mx2 = x * x, my2 = y * y, mxy = x * y, rho2 = mx2 + my2;
  const double rad = c.k1 * rho2 + (c.k2 * rho2) * rho2;
  *dx = (x * rad + (2.0 * c.p1) * mxy) + c.p2 * (rho2 + 2.0 * mx2);
  *dy = (y * rad + (2.0 * c.p2) * mxy) + c.p1 * (rho2 + 2.0 * my2);
}

// ---- O3 ---------------------------------------------------------------------------------------------------------------------------
GF_OBS_HD void obs_lift(const ObsCam &c, float u, float v, float *unx, float *uny) {
  const double mx_d = c.inv_K11 * (double)u + c.inv_K13, my_d = c.inv_K22 * (double)v + c.inv_K23;
  double mx_u = mx_d, my_u = my_d;
  if (!c.no_distortion) {
    double dx, dy;
    obs_distortion(c, mx_d, my_d, &dx, &dy);
    mx_u = mx_d - dx; my_u = my_d - dy;
    for (int k = 0; k < 7; k++) {
      obs_distortion(c, mx_u, my_u, &dx, &dy);
      mx_u = mx_d - dx; my_u = my_d - dy;
    }
  }
  *unx = (float)(mx_u / 1.0); *uny = (float)(my_u / 1.0);
}

// ---- O4 ---------------------------------------------------------------------------------------------------------------------------
GF_OBS_HD float obs_velocity(float un, float prev_un, double dt) { return (float)((double)(un - prev_un) / dt); }
// the first entry of the ascending list that is >= id (the list's length when there is none)
GF_OBS_HD int obs_lower_bound(const int32_t *ids, int n, int32_t id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (ids[mid] < id) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- O5 ---------------------------------------------------------------------------------------------------------------------------
// C's round of the float promoted to double; *inside: the pixel exists
GF_OBS_HD void obs_depth_index(float u, float v, int cols, int rows, int *x, int *y, bool *inside) {
  const double rx = round((double)u), ry = round((double)v);
  *inside = rx >= 0.0 && rx < (double)cols && ry >= 0.0 && ry < (double)rows;      // (false for a NaN)
  *x = *inside ? (int)rx : 0; *y = *inside ? (int)ry : 0;
}
GF_OBS_HD double obs_depth_value(uint16_t raw) { return (double)(int)raw / 1000; }
GF_OBS_HD double obs_no_depth() { return -2.4; }

// ---- O6 ---------------------------------------------------------------------------------------------------------------------------
GF_OBS_HD void obs_row(float unx, float uny, float u, float v, float vx, float vy, double depth, double *row) {
  row[0] = (double)unx; row[1] = (double)uny; row[2] = 1.0; row[3] = (double)u; row[4] = (double)v; row[5] = (double)vx; row[6] = (double)vy; row[7] = depth;
}
// the order of the frame as one unsigned key: the id ascending, then the list index; smaller keys come first
GF_OBS_HD uint64_t obs_key(int32_t id, int index) { return ((uint64_t)((uint32_t)id ^ 0x80000000u) << 32) | (uint32_t)index; }
GF_OBS_HD int32_t obs_key_id(uint64_t k) { return (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u); }
GF_OBS_HD int obs_key_index(uint64_t k) { return (int)(uint32_t)k; }

// ---- O8 ---------------------------------------------------------------------------------------------------------------------------
GF_OBS_HD double obs_dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
// R a (R row-major) and R^T a
GF_OBS_HD void obs_mul(const double *R, const double *a, double *o) {
  for (int i = 0; i < 3; i++) o[i] = obs_dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], a[0], a[1], a[2]);
}
GF_OBS_HD void obs_mul_t(const double *R, const double *a, double *o) {
  for (int i = 0; i < 3; i++) o[i] = obs_dot3(R[i], R[3 + i], R[6 + i], a[0], a[1], a[2]);
}
GF_OBS_HD bool obs_predicts(double depth, int n_obs, int start_frame, int frame_count) { return depth > 0.0 && n_obs >= 2 && start_frame + n_obs - 1 == frame_count; }
// the chain; pose rows are [P(3) | R(9, row-major)], tic_ric = [tic(3) | ric(9)]. Returns whether both coordinates are finite.
GF_OBS_HD bool obs_predict(const ObsCam &c, const double *point0, double depth, const double *pose_start, const double *tic_ric, const double *pose_next, float *u, float *v) {
  const double *tic = tic_ric, *ric = tic_ric + 3;
  const double s[3] = {depth * point0[0], depth * point0[1], depth * point0[2]};
  double pj[3], pw[3], pl[3], pc[3], d[3];
  obs_mul(ric, s, pj);
  for (int i = 0; i < 3; i++) pj[i] = pj[i] + tic[i];
  obs_mul(pose_start + 3, pj, pw);
  for (int i = 0; i < 3; i++) pw[i] = pw[i] + pose_start[i];
  for (int i = 0; i < 3; i++) d[i] = pw[i] - pose_next[i];
  obs_mul_t(pose_next + 3, d, pl);
  for (int i = 0; i < 3; i++) d[i] = pl[i] - tic[i];
  obs_mul_t(ric, d, pc);
  const double x = pc[0] / pc[2], y = pc[1] / pc[2];
  double px = x, py = y;
  if (!c.no_distortion) {
    double dx, dy;
    obs_distortion(c, x, y, &dx, &dy);
    px = x + dx; py = y + dy;
  }
  *u = (float)(c.fx * px + c.cx); *v = (float)(c.fy * py + c.cy);
  return obs_finite((double)*u) && obs_finite((double)*v);
}

// ---- host side (the shim of the tests and the one-thread figure of tools/diag_obs_bench.py) --------------------------------------------
// the order of O6: order [n] = the list indices by ascending id (equal ids in list order). Returns whether two ids are equal.
inline bool obs_host_sort(int n, const int32_t *ids, int *order) {
  std::vector<uint64_t> keys((size_t)n);
  for (int i = 0; i < n; i++) keys[(size_t)i] = obs_key(ids[i], i);
  std::sort(keys.begin(), keys.end());
  bool dup = false;
  for (int i = 0; i < n; i++) {
    order[i] = obs_key_index(keys[(size_t)i]);
    dup = dup || (i > 0 && obs_key_id(keys[(size_t)i]) == obs_key_id(keys[(size_t)i - 1]));
  }
  return dup;
}
// O3 .. O6 of one camera on n held points. prev_ids / prev_un: the previous list, ascending in id (n_prev 0: none); depth: the uint16
// image or nullptr (every row -2.4). ids_out [n], obs8 [n][8] in ascending id, un_out [n][2] likewise (the next previous list);
// counters [4] as gfbe_obs_observe's.
inline void obs_host_observe(const double *cam8, int n, const float *pts, const int32_t *ids, int n_prev, const int32_t *prev_ids, const float *prev_un, double dt,
                             const uint16_t *depth, int cols, int rows, int32_t *ids_out, double *obs8, float *un_out, int32_t *counters) {
  const ObsCam c = obs_camera(cam8);
  std::vector<int> order((size_t)std::max(n, 1));
  const bool dup = obs_host_sort(n, ids, order.data());
  int found = 0, outside = 0;
  for (int j = 0; j < n; j++) {
    const int i = order[(size_t)j];
    const float u = pts[2 * i], v = pts[2 * i + 1];
    float unx, uny, vx = 0.f, vy = 0.f;
    obs_lift(c, u, v, &unx, &uny);
    const int q = obs_lower_bound(prev_ids, n_prev, ids[i]);
    if (q < n_prev && prev_ids[q] == ids[i]) {
      vx = obs_velocity(unx, prev_un[2 * q], dt); vy = obs_velocity(uny, prev_un[2 * q + 1], dt);
      found++;
    }
    double dep = obs_no_depth();
    if (depth) {
      int x, y;
      bool inside;
      obs_depth_index(u, v, cols, rows, &x, &y, &inside);
      dep = obs_depth_value(inside ? depth[(size_t)y * (size_t)cols + (size_t)x] : (uint16_t)0);
      outside += inside ? 0 : 1;
    }
    obs_row(unx, uny, u, v, vx, vy, dep, obs8 + (size_t)OBS_OW * (size_t)j);
    ids_out[j] = ids[i]; un_out[2 * j] = unx; un_out[2 * j + 1] = uny;
  }
  counters[0] = n; counters[1] = found; counters[2] = outside; counters[3] = dup ? 1 : 0;
}
// O8 of one camera: the table's lists (n_feat features; obs0 [n_feat][8] the first observation of each), the held points in held order
inline int obs_host_predict(const double *cam8, int n, const float *pts, const int32_t *ids, int n_feat, const int32_t *feature_id, const int32_t *start_frame,
                            const int32_t *n_obs, const double *depth, const double *obs0, int frame_count, const double *poses /* [11][12] */, const double *tic_ric,
                            const double *next_pose, float *predict_pts) {
  const ObsCam c = obs_camera(cam8);
  int predicted = 0;
  for (int i = 0; i < n; i++) {
    float u = pts[2 * i], v = pts[2 * i + 1];
    for (int f = 0; f < n_feat; f++) {
      if (feature_id[f] != ids[i]) continue;
      float pu, pv;
      if (obs_predicts(depth[f], n_obs[f], start_frame[f], frame_count) &&
          obs_predict(c, obs0 + (size_t)OBS_OW * (size_t)f, depth[f], poses + 12 * (size_t)start_frame[f], tic_ric, next_pose, &pu, &pv)) {
        u = pu; v = pv; predicted++;
      }
      break;
    }
    predict_pts[2 * i] = u; predict_pts[2 * i + 1] = v;
  }
  return predicted;
}

}  // namespace gfd
