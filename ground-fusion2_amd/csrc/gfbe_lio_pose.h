// gfbe_lio_pose.h — the pose algebra of the LiDAR point-to-plane factors shared by k_lio (gfbe_lio.hip) and the scan-to-map
// association (gfbe_vmap.hip): the quaternion helpers and the world point of a scan point, at the single pose (ct = 0) or at
// slerp(alpha) / lerp(alpha) between the begin and the end pose (ct = 1; lio/src/liw/lidarFactor.cpp:59-120). The quaternion helpers and
// the world point are __host__ __device__: the scan handle's per-point pieces (gfbe_scan.h) compile for the host with them.
#pragma once
#include <hip/hip_runtime.h>

namespace gfd {

struct Qx { double x, y, z, w; };
__host__ __device__ __forceinline__ Qx qmulx(Qx a, Qx b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
          a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
__host__ __device__ __forceinline__ void qrotx(Qx q, double R[9]) {
  const double x = q.x, y = q.y, z = q.z, w = q.w;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
__host__ __device__ __forceinline__ Qx slerpx(Qx a, double t, Qx b) {   // Eigen::QuaternionBase::slerp
  const double one = 1.0 - 2.220446049250313e-16;
  const double d = a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w, ad = fabs(d);
  double s0, s1;
  if (ad >= one) { s0 = 1.0 - t; s1 = t; }
  else { const double th = acos(ad), st = sin(th); s0 = sin((1.0 - t) * th) / st; s1 = sin(t * th) / st; }
  if (d < 0) s1 = -s1;
  return {s0 * a.x + s1 * b.x, s0 * a.y + s1 * b.y, s0 * a.z + s1 * b.z, s0 * a.w + s1 * b.w};
}
// R = rotation of the pose the point is taken at, pw = R p + t
__host__ __device__ __forceinline__ void lio_world_point(int ct, const Qx &qb, const Qx &qe, const double *pb, const double *pe, double al, const double *p,
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
// the world point of scan point i into out [n][3] (the body of k_vm_world and of the scan handle's k_sc_world)
__device__ __forceinline__ void lio_world_store(int i, int ct, const double *raw, const double *alpha, const double *pb, const double *pe, double *out) {
  const Qx qb = {pb[3], pb[4], pb[5], pb[6]}, qe = {pe[3], pe[4], pe[5], pe[6]};
  double R[9], pw[3];
  lio_world_point(ct, qb, qe, pb, pe, ct ? alpha[i] : 0.0, raw + 3 * (size_t)i, R, pw);
  for (int a = 0; a < 3; a++) out[3 * (size_t)i + a] = pw[a];
}

__device__ __forceinline__ void q_br(Qx q, double sgn, double M[9]) {   // bottom-right 3x3 of Qleft (+1) / Qright (-1)
  M[0] = q.w; M[1] = -sgn * q.z; M[2] = sgn * q.y; M[3] = sgn * q.z; M[4] = q.w; M[5] = -sgn * q.x; M[6] = -sgn * q.y; M[7] = sgn * q.x; M[8] = q.w;
}
__device__ __forceinline__ void inv3(const double A[9], double B[9]) {
  const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
  const double det = A[0] * c0 + A[1] * c1 + A[2] * c2;
  B[0] = c0 / det; B[1] = (A[2] * A[7] - A[1] * A[8]) / det; B[2] = (A[1] * A[5] - A[2] * A[4]) / det;
  B[3] = c1 / det; B[4] = (A[0] * A[8] - A[2] * A[6]) / det; B[5] = (A[2] * A[3] - A[0] * A[5]) / det;
  B[6] = c2 / det; B[7] = (A[1] * A[6] - A[0] * A[7]) / det; B[8] = (A[0] * A[4] - A[1] * A[3]) / det;
}
__device__ __forceinline__ void mm3(const double *A, const double *B, double *C) {
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { double s = 0; for (int k = 0; k < 3; k++) s += A[3 * i + k] * B[3 * k + j]; C[3 * i + j] = s; }
}

// One point-to-plane row: the residual rk and its 1 x 6 (CT = 0) / 1 x 12 (CT = 1) tangent Jacobian Jk, as k_lio and the registration
// loop (gfbe_vreg.hip) evaluate it — one body, so that both give the same bits.
template <int CT>
__device__ __forceinline__ void lio_row(const double *p, const double *nv, double off, double wgt, double al, double sqrt_info, const Qx &qb, const Qx &qe,
                                        const double *pb, const double *pe, double *Jk, double *r_out) {
  double R[9], pw[3];
  lio_world_point(CT, qb, qe, pb, pe, al, p, R, pw);
  *r_out = sqrt_info * wgt * (nv[0] * pw[0] + nv[1] * pw[1] + nv[2] * pw[2] + off);
  const double nR[3] = {nv[0] * R[0] + nv[1] * R[3] + nv[2] * R[6], nv[0] * R[1] + nv[1] * R[4] + nv[2] * R[7], nv[0] * R[2] + nv[1] * R[5] + nv[2] * R[8]};
  const double jrs[3] = {-wgt * (nR[1] * p[2] - nR[2] * p[1]), -wgt * (nR[2] * p[0] - nR[0] * p[2]), -wgt * (nR[0] * p[1] - nR[1] * p[0])};
  if (!CT) {
    for (int a = 0; a < 3; a++) { Jk[a] = sqrt_info * wgt * nv[a]; Jk[3 + a] = sqrt_info * jrs[a]; }
  } else {
    const Qx qbi = {-qb.x, -qb.y, -qb.z, qb.w};
    const Qx rd = qmulx(qbi, qe);
    const Qx rds = slerpx({0, 0, 0, 1}, al, rd);
    double Rds[9], Ql_s[9], Ql_d[9], Qr_s[9], Qr_d[9], inv[9], T1[9], Jb[9], Je[9];
    qrotx(rds, Rds);
    q_br(rds, +1, Ql_s); q_br(rd, +1, Ql_d); q_br(rds, -1, Qr_s); q_br(rd, -1, Qr_d);
    inv3(Ql_d, inv); mm3(Ql_s, inv, T1);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double s = 0;
        for (int m = 0; m < 3; m++) s += Rds[3 * m + i] * (((m == j) ? 1.0 : 0.0) - al * T1[3 * m + j]);
        Jb[3 * i + j] = s;
      }
    inv3(Qr_d, inv); mm3(Qr_s, inv, T1);
    for (int q = 0; q < 9; q++) Je[q] = al * T1[q];
    for (int a = 0; a < 3; a++) {
      Jk[a] = sqrt_info * wgt * nv[a] * (1 - al);
      Jk[6 + a] = sqrt_info * wgt * nv[a] * al;
      Jk[3 + a] = sqrt_info * (jrs[0] * Jb[a] + jrs[1] * Jb[3 + a] + jrs[2] * Jb[6 + a]);
      Jk[9 + a] = sqrt_info * (jrs[0] * Je[a] + jrs[1] * Je[3 + a] + jrs[2] * Je[6 + a]);
    }
  }
}

}  // namespace gfd
