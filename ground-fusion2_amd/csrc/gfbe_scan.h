// gfbe_scan.h — the per-point pieces of the device-resident LiDAR scan (gfbe_scan.hip), __host__ __device__ so that
// tests/scan_host_shim.cpp can compile them for the host: the segment search of PoseInterp, the interpolated pose, the motion
// compensation of one point and the lidar-to-IMU transform applied at upload.
//
//   PoseInterp                lio/src/common/math_utils.h:530-585
//   Undistort                 lio/src/liw/lio/lidarodom.cpp:1578-1600
//
// Poses are [t | q(x,y,z,w)] with unit quaternions, as everywhere in the LiDAR entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "gfbe_lio_pose.h"

namespace gfd {

constexpr int SC_MAX_STATES = 512;      // nominal states of one scan (staged in LDS: 512 x 8 doubles = 32 KB)

// The segment of PoseInterp for a point stamped q among n states with ascending times t: -1 = the last state (n == 1, or q behind
// the last time), else the first k with t[k] < q && t[k + 1] >= q; when there is none (q <= t[0], or q is NaN) segment 0.
__host__ __device__ inline int scan_segment(int n, const double *t, double q) {
  if (n < 2 || q > t[n - 1]) return -1;
  int lo = 0, hi = n;      // the first j with !(t[j] < q); q <= t[n - 1] keeps it below n
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] < q) lo = mid + 1; else hi = mid;
  }
  return lo == 0 ? 0 : lo - 1;
}

// Ti of a point stamped q: the last state, state k of a segment shorter than 1e-6 s, or slerp (normalised) / lerp at
// s = (q - t[k]) / (t[k + 1] - t[k]) as it comes out (s <= 0 in front of the first state: extrapolation). *seg = scan_segment.
__host__ __device__ inline void scan_pose_at(int n, const double *t, const double *pose, double q, int *seg, double *Ti) {
  const int k = scan_segment(n, t, q);
  *seg = k;
  if (k < 0) { for (int a = 0; a < 7; a++) Ti[a] = pose[7 * (n - 1) + a]; return; }
  const double *a = pose + 7 * k, *b = a + 7;
  const double dt = t[k + 1] - t[k];
  if (fabs(dt) < 1e-6) { for (int i = 0; i < 7; i++) Ti[i] = a[i]; return; }
  const double s = (q - t[k]) / dt;
  const Qx r = slerpx({a[3], a[4], a[5], a[6]}, s, {b[3], b[4], b[5], b[6]});
  const double nn = sqrt(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w);
  Ti[3] = r.x / nn; Ti[4] = r.y / nn; Ti[5] = r.z / nn; Ti[6] = r.w / nn;
  for (int i = 0; i < 3; i++) Ti[i] = a[i] * (1 - s) + b[i] * s;
}

// out = T_end^-1 Ti p = R_end^T ((R_i p + t_i) - t_end)
__host__ __device__ inline void scan_undistort_point(const double *Te, const double *Ti, const double *p, double *out) {
  double Ri[9], Re[9], d[3];
  qrotx({Ti[3], Ti[4], Ti[5], Ti[6]}, Ri);
  qrotx({Te[3], Te[4], Te[5], Te[6]}, Re);
  for (int a = 0; a < 3; a++) d[a] = (Ri[3 * a] * p[0] + Ri[3 * a + 1] * p[1] + Ri[3 * a + 2] * p[2] + Ti[a]) - Te[a];
  for (int a = 0; a < 3; a++) out[a] = Re[a] * d[0] + Re[3 + a] * d[1] + Re[6 + a] * d[2];
}

// out = T_IL p (the lidar point in the IMU frame)
__host__ __device__ inline void scan_til_point(const double *til, const double *p, double *out) {
  double R[9];
  qrotx({til[3], til[4], til[5], til[6]}, R);
  for (int a = 0; a < 3; a++) out[a] = R[3 * a] * p[0] + R[3 * a + 1] * p[1] + R[3 * a + 2] * p[2] + til[a];
}

}  // namespace gfd
