// gfbe_lio_pose.h — the pose algebra of the LiDAR point-to-plane factors shared by k_lio (gfbe_lio.hip) and the scan-to-map
// association (gfbe_vmap.hip): the quaternion helpers and the world point of a scan point, at the single pose (ct = 0) or at
// slerp(alpha) / lerp(alpha) between the begin and the end pose (ct = 1; lio/src/liw/lidarFactor.cpp:59-120).
#pragma once
#include <hip/hip_runtime.h>

namespace gfd {

struct Qx { double x, y, z, w; };
__device__ __forceinline__ Qx qmulx(Qx a, Qx b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
          a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
__device__ __forceinline__ void qrotx(Qx q, double R[9]) {
  const double x = q.x, y = q.y, z = q.z, w = q.w;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
__device__ __forceinline__ Qx slerpx(Qx a, double t, Qx b) {   // Eigen::QuaternionBase::slerp
  const double one = 1.0 - 2.220446049250313e-16;
  const double d = a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w, ad = fabs(d);
  double s0, s1;
  if (ad >= one) { s0 = 1.0 - t; s1 = t; }
  else { const double th = acos(ad), st = sin(th); s0 = sin((1.0 - t) * th) / st; s1 = sin(t * th) / st; }
  if (d < 0) s1 = -s1;
  return {s0 * a.x + s1 * b.x, s0 * a.y + s1 * b.y, s0 * a.z + s1 * b.z, s0 * a.w + s1 * b.w};
}
// R = rotation of the pose the point is taken at, pw = R p + t
__device__ __forceinline__ void lio_world_point(int ct, const Qx &qb, const Qx &qe, const double *pb, const double *pe, double al, const double *p,
                                                double *R, double *pw) {
  Qx qs = qb;
  double ts[3] = {pb[0], pb[1], pb[2]};
  if (ct) {
    const Qx s = slerpx(qb, al, qe);
    const double nn = sqrt(s.x * s.x + s.y * s.y + s.z * s.z + s.w * s.w);
    qs = {s.x / nn, s.y / nn, s.z / nn, s.w / nn};
    for (int a = 0; a < 3; a++) ts[a] = pb[a] * (1 - al) + pe[a] * al;
  }
  qrotx(qs, R);
  pw[0] = R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + ts[0];
  pw[1] = R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + ts[1];
  pw[2] = R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + ts[2];
}

}  // namespace gfd
