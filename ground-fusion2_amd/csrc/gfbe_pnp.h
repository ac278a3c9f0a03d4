// gfbe_pnp.h — the rules of the loop verification (gfbe_pnp.hip) that need no HIP header: under a plain C++ compiler they are ordinary
// inline functions, under hipcc the per-hypothesis and per-point ones are __host__ __device__ (tests/pnp_host_shim.cpp compiles them for
// the host). The rules V1 .. V8 are stated in include/gfbe_pnp.h; citations are to
//
//   KeyFrame::PnPRANSAC                                            dense_map/src/keyframe.cpp:273-329
//   KeyFrame::findConnection, the loop_info half                   dense_map/src/keyframe.cpp:479-565
//
// Everything here is FP64 + - * /, sqrt, fabs and comparisons, every expression written once and compiled without contraction; the two
// atan2 of V7 and the floor of normalizeAngle are taken on the host (pnp_decide). No array is indexed by a computed value: a choice among
// three is pnp_sel3, so that the device keeps everything in registers. The model tests/pnp_np.py reproduces every function bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define GF_PNP_HD __host__ __device__ inline
#else
#define GF_PNP_HD inline
#endif
#if defined(__clang__)
#define GF_PNP_UNROLL _Pragma("unroll")
#else
#define GF_PNP_UNROLL
#endif

namespace gfd {

constexpr int PNP_MAX_POINTS = 4096;      // points of a problem: the inlier list of V6 is 16 KB of LDS
constexpr int PNP_MAX_ITER = 1024;        // hypotheses of a problem: 4 h + s stays below 2^20 in V5's key
constexpr int PNP_DRAWS = 64;             // draws of a hypothesis (V2)
constexpr int PNP_MAX_REFINE = 20;
constexpr int PNP_BISECT = 100;           // halvings of V3's bracket
constexpr int PNP_RES = 19;               // doubles a problem brings back: relative_t, relative_q (w x y z), PnP_T_old, PnP_R_old

struct PnpParams {                         // the options a kernel needs
  int iterations, refine_iterations, min_loop_num, pad;
  uint64_t seed;
  double thr2;                             // reproj_threshold * reproj_threshold
};

GF_PNP_HD bool pnp_finite(double v) { return v - v == 0.0; }      // (neither an infinity nor a NaN)
GF_PNP_HD double pnp_sel3(int k, double a0, double a1, double a2) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }

// ---- V2 ---------------------------------------------------------------------------------------------------------------------------
GF_PNP_HD uint64_t pnp_hash(uint64_t seed, int h, int k) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(1 + 256 * h + k);
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// the sample of hypothesis h among n points: idx [3], -1 where unfilled; returns the accepted indices (3: a sample)
GF_PNP_HD int pnp_sample(uint64_t seed, int h, int n, int *idx) {
  int a = -1, b = -1, c = -1, got = 0;
  for (int k = 0; k < PNP_DRAWS; k++) {
    const int i = (int)(pnp_hash(seed, h, k) % (uint64_t)n);
    if (got < 3 && i != a && i != b && i != c) {
      if (got == 0) a = i; else if (got == 1) b = i; else c = i;
      got++;
    }
  }
  idx[0] = a; idx[1] = b; idx[2] = c;
  return got;
}

// ---- V3 ---------------------------------------------------------------------------------------------------------------------------
// the cofactors of a symmetric 3 x 3 matrix m = (m00 m01 m02 m11 m12 m22), in the same order
GF_PNP_HD void pnp_cof(const double *m, double *A) {
  A[0] = m[3] * m[5] - m[4] * m[4];
  A[1] = m[2] * m[4] - m[1] * m[5];
  A[2] = m[1] * m[4] - m[2] * m[3];
  A[3] = m[0] * m[5] - m[2] * m[2];
  A[4] = m[1] * m[2] - m[0] * m[4];
  A[5] = m[0] * m[3] - m[1] * m[1];
}
GF_PNP_HD double pnp_dot6(const double *A, const double *q) { return A[0] * q[0] + A[3] * q[3] + A[5] * q[5] + 2.0 * (A[1] * q[1] + A[2] * q[2] + A[4] * q[4]); }
GF_PNP_HD double pnp_cubic(double c0, double c1, double c2, double c3, double x) { return ((c3 * x + c2) * x + c1) * x + c0; }
// a real root of c0 + c1 x + c2 x^2 + c3 x^3 by PNP_BISECT halvings of [-r, r], r = 1 + max(|c0|, |c1|, |c2|) / |c3| (Cauchy's bound)
GF_PNP_HD double pnp_cubic_root(double c0, double c1, double c2, double c3) {
  double mx = fabs(c0);
  mx = fabs(c1) > mx ? fabs(c1) : mx;
  mx = fabs(c2) > mx ? fabs(c2) : mx;
  const double r = 1.0 + mx / fabs(c3);
  const bool up = c3 > 0.0;
  double lo = -r, hi = r;
  for (int k = 0; k < PNP_BISECT; k++) {
    const double mid = 0.5 * (lo + hi);
    const bool pos = pnp_cubic(c0, c1, c2, c3, mid) > 0.0;
    if (pos == up) hi = mid; else lo = mid;
  }
  return 0.5 * (lo + hi);
}
// what a sample's three world points fix before any solution: the edges, the degeneracy test, the inverse of [d12 d13 d12 x d13]
struct PnpTriad {
  double d12[3], d13[3], a12, a13, a23, r0[3], r1[3], r2[3];
  bool ok;
};
GF_PNP_HD void pnp_cross(const double *a, const double *b, double *c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
GF_PNP_HD double pnp_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
GF_PNP_HD PnpTriad pnp_triad(const double *X /* [3][3] */) {
  PnpTriad T;
  double d23[3], cr[3];
  for (int a = 0; a < 3; a++) { T.d12[a] = X[a] - X[3 + a]; T.d13[a] = X[a] - X[6 + a]; d23[a] = X[3 + a] - X[6 + a]; }
  T.a12 = pnp_dot(T.d12, T.d12); T.a13 = pnp_dot(T.d13, T.d13); T.a23 = pnp_dot(d23, d23);
  pnp_cross(T.d12, T.d13, cr);
  const double c2 = pnp_dot(cr, cr);
  // degenerate: two equal points or three on a line, |d12 x d13|^2 <= 1e-12 |d12|^2 |d13|^2 (false for a NaN as well)
  T.ok = c2 > 1e-12 * T.a12 * T.a13;
  double u[3], v[3];
  pnp_cross(T.d13, cr, u);
  pnp_cross(cr, T.d12, v);
  for (int a = 0; a < 3; a++) { T.r0[a] = u[a] / c2; T.r1[a] = v[a] / c2; T.r2[a] = cr[a] / c2; }
  return T;
}
// One solution: depths l [3] of the bearings y [3][3] -> pose12 = t then R row-major with Xc = R Xw + t; false: a non-finite entry
GF_PNP_HD bool pnp_pose_from_depths(const PnpTriad &T, const double *X0, const double *y, const double *l, double *pose12) {
  double Y0[3], e1[3], e2[3], e3[3];
  for (int a = 0; a < 3; a++) { Y0[a] = l[0] * y[a]; e1[a] = Y0[a] - l[1] * y[3 + a]; e2[a] = Y0[a] - l[2] * y[6 + a]; }
  pnp_cross(e1, e2, e3);
  double R[9], chk = 0.0;
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) { R[3 * a + b] = e1[a] * T.r0[b] + e2[a] * T.r1[b] + e3[a] * T.r2[b]; chk += R[3 * a + b]; }
  double t[3];
  for (int a = 0; a < 3; a++) { t[a] = Y0[a] - (R[3 * a] * X0[0] + R[3 * a + 1] * X0[1] + R[3 * a + 2] * X0[2]); chk += t[a]; }
  if (!pnp_finite(chk)) return false;
  for (int a = 0; a < 3; a++) pose12[a] = t[a];
  for (int a = 0; a < 9; a++) pose12[3 + a] = R[a];
  return true;
}
// The P3P of one sample: X [3][3] world points, uv [3][2] normalised observations. Up to four poses into out [4][12] (t, then R), in the
// order line 0 root +, line 0 root -, line 1 root +, line 1 root -; returns their number. The unused rows of `out` are not written.
//   depths l_i of the unit bearings y_i: l_i^2 + l_j^2 - 2 b_ij l_i l_j = a_ij with b_ij = y_i . y_j, a_ij = |X_i - X_j|^2.
//   D1 = M12 a23 - M23 a12 and D2 = M13 a23 - M23 a13 are two conics in (l_1 : l_2 : l_3); g with det(D1 + g D2) = 0 makes
//   D0 = D1 + g D2 a pair of lines, found from -adj(D0) = p p^T and D0 + [p]x = 2 m l^T; each line meets a conic in two points.
GF_PNP_HD int pnp_p3p(const double *X, const double *uv, double *out) {
  const PnpTriad T = pnp_triad(X);
  if (!T.ok) return 0;
  double y[9];
  for (int i = 0; i < 3; i++) {
    const double u = uv[2 * i], v = uv[2 * i + 1], nn = sqrt(u * u + v * v + 1.0);
    y[3 * i] = u / nn; y[3 * i + 1] = v / nn; y[3 * i + 2] = 1.0 / nn;
  }
  const double b12 = pnp_dot(y, y + 3), b13 = pnp_dot(y, y + 6), b23 = pnp_dot(y + 3, y + 6);
  const double a12 = T.a12, a13 = T.a13, a23 = T.a23;
  const double D1[6] = {a23, -(a23 * b12), 0.0, a23 - a12, a12 * b23, -a12};
  const double D2[6] = {a23, 0.0, -(a23 * b13), -a13, a13 * b23, a23 - a13};
  double A1[6], A2[6];
  pnp_cof(D1, A1);
  pnp_cof(D2, A2);
  const double c0 = D1[0] * A1[0] + D1[1] * A1[1] + D1[2] * A1[2], c3 = D2[0] * A2[0] + D2[1] * A2[1] + D2[2] * A2[2];
  const double c1 = pnp_dot6(A1, D2), c2 = pnp_dot6(A2, D1);
  const double g = pnp_cubic_root(c0, c1, c2, c3);
  if (!pnp_finite(g)) return 0;
  double D0[6], Bm[6];
  for (int a = 0; a < 6; a++) D0[a] = D1[a] + g * D2[a];
  pnp_cof(D0, Bm);
  for (int a = 0; a < 6; a++) Bm[a] = -Bm[a];
  int j = 0;
  double bjj = Bm[0];
  if (Bm[3] > bjj) { j = 1; bjj = Bm[3]; }
  if (Bm[5] > bjj) { j = 2; bjj = Bm[5]; }
  if (!(bjj > 0.0)) return 0;      // the lines are not real (or a NaN)
  const double sq = sqrt(bjj);
  const double p0 = pnp_sel3(j, Bm[0], Bm[1], Bm[2]) / sq, p1 = pnp_sel3(j, Bm[1], Bm[3], Bm[4]) / sq, p2 = pnp_sel3(j, Bm[2], Bm[4], Bm[5]) / sq;
  const double C00 = D0[0], C01 = D0[1] - p2, C02 = D0[2] + p1, C10 = D0[1] + p2, C11 = D0[3], C12 = D0[4] - p0, C20 = D0[2] - p1, C21 = D0[4] + p0, C22 = D0[5];
  // the entry of largest magnitude, the first in row-major order on a tie: its row is one line, its column the other
  int ra = 0, cb = 0;
  double big = fabs(C00);
  if (fabs(C01) > big) { big = fabs(C01); ra = 0; cb = 1; }
  if (fabs(C02) > big) { big = fabs(C02); ra = 0; cb = 2; }
  if (fabs(C10) > big) { big = fabs(C10); ra = 1; cb = 0; }
  if (fabs(C11) > big) { big = fabs(C11); ra = 1; cb = 1; }
  if (fabs(C12) > big) { big = fabs(C12); ra = 1; cb = 2; }
  if (fabs(C20) > big) { big = fabs(C20); ra = 2; cb = 0; }
  if (fabs(C21) > big) { big = fabs(C21); ra = 2; cb = 1; }
  if (fabs(C22) > big) { big = fabs(C22); ra = 2; cb = 2; }
  const double L[6] = {pnp_sel3(ra, C00, C10, C20), pnp_sel3(ra, C01, C11, C21), pnp_sel3(ra, C02, C12, C22),
                       pnp_sel3(cb, C00, C01, C02), pnp_sel3(cb, C10, C11, C12), pnp_sel3(cb, C20, C21, C22)};
  // the conic the lines are cut with: the one D0 is farther from
  const bool useD2 = fabs(g) <= 1.0;
  double Q[6];
  for (int a = 0; a < 6; a++) Q[a] = useD2 ? D2[a] : D1[a];
  int ns = 0;
  for (int line = 0; line < 2; line++) {
    const double L0 = L[3 * line], L1 = L[3 * line + 1], L2 = L[3 * line + 2];
    int k = 0;
    double lk = fabs(L0);
    if (fabs(L1) > lk) { k = 1; lk = fabs(L1); }
    if (fabs(L2) > lk) { k = 2; lk = fabs(L2); }
    if (!(lk > 0.0)) continue;
    // with i = k + 1 and j = k + 2 (cyclic): l_k = wi l_i + wj l_j on the line
    const double Lk = pnp_sel3(k, L0, L1, L2), wi = -pnp_sel3(k, L1, L2, L0) / Lk, wj = -pnp_sel3(k, L2, L0, L1) / Lk;
    const double Qkk = pnp_sel3(k, Q[0], Q[3], Q[5]), Qii = pnp_sel3(k, Q[3], Q[5], Q[0]), Qjj = pnp_sel3(k, Q[5], Q[0], Q[3]);
    const double Qki = pnp_sel3(k, Q[1], Q[4], Q[2]), Qkj = pnp_sel3(k, Q[2], Q[1], Q[4]), Qij = pnp_sel3(k, Q[4], Q[2], Q[1]);
    const double qa = Qkk * wi * wi + 2.0 * Qki * wi + Qii;
    const double qb = 2.0 * (Qkk * wi * wj + Qki * wj + Qkj * wi + Qij);
    const double qc = Qkk * wj * wj + 2.0 * Qkj * wj + Qjj;
    const double disc = qb * qb - 4.0 * qa * qc;
    if (!(disc >= 0.0)) continue;
    const double sd = sqrt(disc);
    for (int sign = 0; sign < 2; sign++) {
      const double tau = (sign == 0 ? -qb + sd : -qb - sd) / (2.0 * qa);      // l_i with l_j = 1
      const double lamk = wi * tau + wj;
      const double m0 = pnp_sel3(k, lamk, 1.0, tau), m1 = pnp_sel3(k, tau, lamk, 1.0), m2 = pnp_sel3(k, 1.0, tau, lamk);
      const double den = m0 * m0 + m1 * m1 - 2.0 * b12 * m0 * m1;
      const double sc = sqrt(a12 / den), s = m0 < 0.0 ? -sc : sc;
      const double l[3] = {s * m0, s * m1, s * m2};
      if (!(l[0] > 0.0 && l[1] > 0.0 && l[2] > 0.0)) continue;      // positive depths (false for a NaN)
      if (pnp_pose_from_depths(T, X, y, l, out + 12 * ns)) ns++;
    }
  }
  return ns;
}

// ---- V4 ---------------------------------------------------------------------------------------------------------------------------
// pose12 = t, then R row-major; X the world point, (u, v) its observation
GF_PNP_HD void pnp_transform(const double *pose12, double X0, double X1, double X2, double *xc) {
  xc[0] = pose12[3] * X0 + pose12[4] * X1 + pose12[5] * X2 + pose12[0];
  xc[1] = pose12[6] * X0 + pose12[7] * X1 + pose12[8] * X2 + pose12[1];
  xc[2] = pose12[9] * X0 + pose12[10] * X1 + pose12[11] * X2 + pose12[2];
}
GF_PNP_HD double pnp_error(const double *xc, double u, double v) {
  const double du = xc[0] / xc[2] - u, dv = xc[1] / xc[2] - v;
  return du * du + dv * dv;
}
GF_PNP_HD bool pnp_inlier(const double *pose12, double X0, double X1, double X2, double u, double v, double thr2) {
  double xc[3];
  pnp_transform(pose12, X0, X1, X2, xc);
  return xc[2] > 0.0 && pnp_error(xc, u, v) <= thr2;
}
// ---- V5 ---------------------------------------------------------------------------------------------------------------------------
// the larger key wins: the larger count, then the lower 4 h + s; 0 is "no solution"
GF_PNP_HD unsigned long long pnp_key(int count, int h, int s) { return (unsigned long long)count << 20 | (unsigned long long)(0xFFFFF - (4 * h + s)); }
GF_PNP_HD int pnp_key_count(unsigned long long key) { return (int)(key >> 20); }
GF_PNP_HD int pnp_key_slot(unsigned long long key) { return 0xFFFFF - (int)(key & 0xFFFFF); }

// ---- V6, V7: quaternions (w x y z) ----------------------------------------------------------------------------------------------------
// Eigen's Quaternion(Matrix3): the trace branch, else the largest diagonal entry (the first of equal ones)
GF_PNP_HD void pnp_rot_to_quat(const double *R, double *q) {
  const double tr = R[0] + R[4] + R[8];
  double w, x, y, z;      // (scalars: a store to q [i] with a computed i would put q into scratch on the device)
  if (tr > 0.0) {
    double s = sqrt(tr + 1.0);
    w = 0.5 * s;
    s = 0.5 / s;
    x = (R[7] - R[5]) * s; y = (R[2] - R[6]) * s; z = (R[3] - R[1]) * s;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > (i == 0 ? R[0] : R[4])) i = 2;
    if (i == 0) {
      double s = sqrt(R[0] - R[4] - R[8] + 1.0);
      x = 0.5 * s;
      s = 0.5 / s;
      w = (R[7] - R[5]) * s; y = (R[3] + R[1]) * s; z = (R[6] + R[2]) * s;
    } else if (i == 1) {
      double s = sqrt(R[4] - R[8] - R[0] + 1.0);
      y = 0.5 * s;
      s = 0.5 / s;
      w = (R[2] - R[6]) * s; z = (R[7] + R[5]) * s; x = (R[1] + R[3]) * s;
    } else {
      double s = sqrt(R[8] - R[0] - R[4] + 1.0);
      z = 0.5 * s;
      s = 0.5 / s;
      w = (R[3] - R[1]) * s; x = (R[2] + R[6]) * s; y = (R[5] + R[7]) * s;
    }
  }
  q[0] = w; q[1] = x; q[2] = y; q[3] = z;
}
GF_PNP_HD void pnp_quat_to_rot(const double *q, double *R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w); R[2] = 2.0 * (x * z + y * w);
  R[3] = 2.0 * (x * y + z * w); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
  R[6] = 2.0 * (x * z - y * w); R[7] = 2.0 * (y * z + x * w); R[8] = 1.0 - 2.0 * (x * x + y * y);
}
GF_PNP_HD void pnp_quat_normalize(double *q) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}
// a * b (Hamilton)
GF_PNP_HD void pnp_quat_mul(const double *a, const double *b, double *c) {
  c[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  c[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  c[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  c[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
// one inlier's share of the normal equations: acc [27] = the 21 upper-triangle entries of J^T J row by row, then J^T r
GF_PNP_HD void pnp_accumulate(const double *pose12, double X0, double X1, double X2, double u, double v, double *acc) {
  double xc[3];
  pnp_transform(pose12, X0, X1, X2, xc);
  const double iz = 1.0 / xc[2], px = xc[0] * iz, py = xc[1] * iz, ru = px - u, rv = py - v;
  const double gu2 = -(px * iz), gv2 = -(py * iz);      // d(u) / dXc = (iz, 0, gu2), d(v) / dXc = (0, iz, gv2)
  const double Ju[6] = {gu2 * xc[1], iz * xc[2] - gu2 * xc[0], -(iz * xc[1]), iz, 0.0, gu2};
  const double Jv[6] = {-(iz * xc[2]) + gv2 * xc[1], -(gv2 * xc[0]), iz * xc[0], 0.0, iz, gv2};
  int e = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) { acc[e] = acc[e] + (Ju[a] * Ju[b] + Jv[a] * Jv[b]); e++; }
  for (int a = 0; a < 6; a++) acc[21 + a] = acc[21 + a] + (Ju[a] * ru + Jv[a] * rv);
}
// (J^T J) d = -J^T r by L D L^T without pivoting; false: a pivot <= 0 or not finite (d is then undefined)
GF_PNP_HD bool pnp_solve6(const double *acc, double *d) {
  double Lm[36], Dg[6], yv[6];
  bool ok = true;
  GF_PNP_UNROLL
  for (int a = 0; a < 6; a++)
    GF_PNP_UNROLL
    for (int b = 0; b < 6; b++) Lm[6 * a + b] = 0.0;
  GF_PNP_UNROLL
  for (int jc = 0; jc < 6; jc++) {
    // entry (a, b), a <= b, of the upper triangle listed row by row sits at a * 6 - a (a - 1) / 2 + b - a
    double dj = acc[jc * 6 - jc * (jc - 1) / 2];
    GF_PNP_UNROLL
    for (int k = 0; k < jc; k++) dj = dj - Lm[6 * jc + k] * Lm[6 * jc + k] * Dg[k];
    if (!(dj > 0.0) || !pnp_finite(dj)) ok = false;
    Dg[jc] = dj;
    GF_PNP_UNROLL
    for (int i = jc + 1; i < 6; i++) {
      double s = acc[jc * 6 - jc * (jc - 1) / 2 + i - jc];
      GF_PNP_UNROLL
      for (int k = 0; k < jc; k++) s = s - Lm[6 * i + k] * Lm[6 * jc + k] * Dg[k];
      Lm[6 * i + jc] = s / dj;
    }
  }
  GF_PNP_UNROLL
  for (int i = 0; i < 6; i++) {
    double s = -acc[21 + i];
    GF_PNP_UNROLL
    for (int k = 0; k < i; k++) s = s - Lm[6 * i + k] * yv[k];
    yv[i] = s;
  }
  GF_PNP_UNROLL
  for (int i = 5; i >= 0; i--) {
    double s = yv[i] / Dg[i];
    GF_PNP_UNROLL
    for (int k = i + 1; k < 6; k++) s = s - Lm[6 * k + i] * d[k];
    d[i] = s;
  }
  return ok;
}
// the update of a step d = (dtheta, dt) on q (w x y z) and pose12 = t, R
GF_PNP_HD void pnp_update(const double *d, double *q, double *pose12) {
  double dq[4] = {1.0, 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]}, dR[9], qn[4];
  pnp_quat_normalize(dq);
  pnp_quat_mul(dq, q, qn);
  pnp_quat_normalize(qn);
  pnp_quat_to_rot(dq, dR);
  const double t0 = pose12[0], t1 = pose12[1], t2 = pose12[2];
  pose12[0] = dR[0] * t0 + dR[1] * t1 + dR[2] * t2 + d[3];
  pose12[1] = dR[3] * t0 + dR[4] * t1 + dR[5] * t2 + d[4];
  pose12[2] = dR[6] * t0 + dR[7] * t1 + dR[8] * t2 + d[5];
  for (int a = 0; a < 4; a++) q[a] = qn[a];
  pnp_quat_to_rot(q, pose12 + 3);
}
// ---- V7 without its two atan2: res [PNP_RES] = relative_t, relative_q (w x y z), PnP_T_old, PnP_R_old ------------------------------------
GF_PNP_HD void pnp_relative(const double *pose12, const double *pose_cur, const double *tic_qic, double *res) {
  const double *R = pose12 + 3, *t = pose12, *Pc = pose_cur, *Rc = pose_cur + 3, *tic = tic_qic, *qic = tic_qic + 3;
  double Tw[3], PR[9], PT[3], dd[3], Rr[9];
  for (int a = 0; a < 3; a++) Tw[a] = R[a] * -t[0] + R[3 + a] * -t[1] + R[6 + a] * -t[2];                                     // R^T (-t)
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) PR[3 * a + b] = R[a] * qic[3 * b] + R[3 + a] * qic[3 * b + 1] + R[6 + a] * qic[3 * b + 2];      // R^T qic^T
  for (int a = 0; a < 3; a++) PT[a] = Tw[a] - (PR[3 * a] * tic[0] + PR[3 * a + 1] * tic[1] + PR[3 * a + 2] * tic[2]);
  for (int a = 0; a < 3; a++) dd[a] = Pc[a] - PT[a];
  for (int a = 0; a < 3; a++) res[a] = PR[a] * dd[0] + PR[3 + a] * dd[1] + PR[6 + a] * dd[2];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) Rr[3 * a + b] = PR[a] * Rc[b] + PR[3 + a] * Rc[3 + b] + PR[6 + a] * Rc[6 + b];
  pnp_rot_to_quat(Rr, res + 3);
  for (int a = 0; a < 3; a++) res[7 + a] = PT[a];
  for (int a = 0; a < 9; a++) res[10 + a] = PR[a];
}

// ---- V7's yaw and V8, on the host ------------------------------------------------------------------------------------------------------
inline double pnp_yaw_deg(double r10, double r00) { return atan2(r10, r00) / M_PI * 180.0; }
inline double pnp_normalize_angle(double a) {      // utility.h:140-148
  const double two_pi = 2.0 * 180;
  if (a > 0) return a - two_pi * floor((a + 180.0) / two_pi);
  return a + two_pi * floor((-a + 180.0) / two_pi);
}
// res of pnp_relative and the winner's count -> loop_info [8] (zeros unless has_loop), returns has_loop
inline int pnp_decide(const double *res, const double *pose_cur, int n_inliers, int min_loop_num, double max_yaw_deg, double max_translation, double *loop_info) {
  for (int a = 0; a < 8; a++) loop_info[a] = 0.0;
  if (!(n_inliers > min_loop_num)) return 0;
  const double yaw = pnp_normalize_angle(pnp_yaw_deg(pose_cur[6], pose_cur[3]) - pnp_yaw_deg(res[13], res[10]));
  const double tn = sqrt(res[0] * res[0] + res[1] * res[1] + res[2] * res[2]);
  if (!(fabs(yaw) < max_yaw_deg && tn < max_translation)) return 0;
  for (int a = 0; a < 7; a++) loop_info[a] = res[a];
  loop_info[7] = yaw;
  return 1;
}

// ---- host side: one problem on one thread (the shim of the tests and the host column of tools/diag_pnp_bench.py) --------------------------
struct PnpHostOut {
  int n_inliers = 0, has_loop = 0, best_h = -1, best_s = -1, refine_flag = 0;
  double loop_info[8] = {}, res[PNP_RES] = {};
};
// diagnostics (any may be null): sample_idx [H][3], n_solutions [H], hyp_pose [H][4][12], hyp_count [H][4]
inline PnpHostOut pnp_host_problem(const PnpParams &P, double max_yaw_deg, double max_translation, int n, const float *point_3d, const float *pt_norm, const double *pose_cur,
                                   const double *tic_qic, uint8_t *status, int32_t *sample_idx, int32_t *n_solutions, double *hyp_pose, int32_t *hyp_count) {
  PnpHostOut o;
  const int H = P.iterations;
  for (int i = 0; i < n; i++) if (status) status[i] = 0;
  for (int h = 0; h < H; h++) {
    if (sample_idx) for (int a = 0; a < 3; a++) sample_idx[3 * h + a] = -1;
    if (n_solutions) n_solutions[h] = 0;
    if (hyp_pose) for (int a = 0; a < 48; a++) hyp_pose[48 * (size_t)h + a] = 0.0;
    if (hyp_count) for (int a = 0; a < 4; a++) hyp_count[4 * h + a] = 0;
  }
  if (n <= P.min_loop_num) return o;
  std::vector<double> Xd(3 * (size_t)n), Ud(2 * (size_t)n);
  for (size_t a = 0; a < 3 * (size_t)n; a++) Xd[a] = (double)point_3d[a];
  for (size_t a = 0; a < 2 * (size_t)n; a++) Ud[a] = (double)pt_norm[a];
  unsigned long long best = 0;
  double best_pose[12] = {};
  for (int h = 0; h < H; h++) {
    int idx[3];
    double sol[48] = {};
    int ns = 0;
    if (pnp_sample(P.seed, h, n, idx) == 3) {
      double X[9], uv[6];
      for (int m = 0; m < 3; m++) {
        for (int a = 0; a < 3; a++) X[3 * m + a] = Xd[3 * (size_t)idx[m] + a];
        for (int a = 0; a < 2; a++) uv[2 * m + a] = Ud[2 * (size_t)idx[m] + a];
      }
      ns = pnp_p3p(X, uv, sol);
    }
    for (int a = 12 * ns; a < 48; a++) sol[a] = 0.0;
    if (sample_idx) for (int a = 0; a < 3; a++) sample_idx[3 * h + a] = idx[a];
    if (n_solutions) n_solutions[h] = ns;
    if (hyp_pose) for (int a = 0; a < 48; a++) hyp_pose[48 * (size_t)h + a] = sol[a];
    for (int s = 0; s < ns; s++) {
      int count = 0;
      for (int i = 0; i < n; i++) count += pnp_inlier(sol + 12 * s, Xd[3 * (size_t)i], Xd[3 * (size_t)i + 1], Xd[3 * (size_t)i + 2], Ud[2 * (size_t)i], Ud[2 * (size_t)i + 1], P.thr2) ? 1 : 0;
      if (hyp_count) hyp_count[4 * h + s] = count;
      const unsigned long long key = pnp_key(count, h, s);
      if (key > best) { best = key; for (int a = 0; a < 12; a++) best_pose[a] = sol[12 * s + a]; }
    }
  }
  if (best == 0) return o;
  o.n_inliers = pnp_key_count(best); o.best_h = pnp_key_slot(best) / 4; o.best_s = pnp_key_slot(best) % 4;
  std::vector<int> inl;
  for (int i = 0; i < n; i++) {
    const bool in = pnp_inlier(best_pose, Xd[3 * (size_t)i], Xd[3 * (size_t)i + 1], Xd[3 * (size_t)i + 2], Ud[2 * (size_t)i], Ud[2 * (size_t)i + 1], P.thr2);
    if (status) status[i] = in ? 1 : 0;
    if (in) inl.push_back(i);
  }
  // V6: lane l of 64 sums the inliers l, l + 64, ...; then the butterfly s = s + shfl_xor(s, off), off = 32 .. 1
  double pose[12], q[4];
  for (int a = 0; a < 12; a++) pose[a] = best_pose[a];
  pnp_rot_to_quat(pose + 3, q);
  for (int it = 0; it < P.refine_iterations; it++) {
    std::vector<double> lane(64 * 27, 0.0), nxt(64 * 27);
    for (size_t r = 0; r < inl.size(); r++) {
      const size_t i = (size_t)inl[r];
      pnp_accumulate(pose, Xd[3 * i], Xd[3 * i + 1], Xd[3 * i + 2], Ud[2 * i], Ud[2 * i + 1], &lane[27 * (r % 64)]);
    }
    for (int off = 32; off >= 1; off >>= 1) {
      for (int l = 0; l < 64; l++)
        for (int e = 0; e < 27; e++) nxt[27 * l + e] = lane[27 * l + e] + lane[27 * (l ^ off) + e];
      lane.swap(nxt);
    }
    double d[6];
    if (!pnp_solve6(lane.data(), d)) { o.refine_flag = 1; break; }
    pnp_update(d, q, pose);
  }
  pnp_relative(pose, pose_cur, tic_qic, o.res);
  o.has_loop = pnp_decide(o.res, pose_cur, o.n_inliers, P.min_loop_num, max_yaw_deg, max_translation, o.loop_info);
  return o;
}

}  // namespace gfd
