// gfbe_line.h — line landmarks: the orthonormal line representation, the line projection factor and the culling test, as
// __host__ __device__ functions used by csrc/gfbe_line.hip (and compiled for the host by tests/line_host_shim.cpp); the line list of a
// batch (LineList) and the kernel-side pieces gfbe_line.hip, gfbe_line_reduce.hip and gfbe_line_step.hip share: the accessors, a
// window's prologue, the rank of the entering lines and the fixed-order workgroup reduction.
// Reference semantics:
//   plk_to_orth / orth_to_plk / plk_to_pose / plk_from_pose   utility/line_geometry.cpp:56-113, 181-200
//   lineProjectionFactor::Evaluate                            factor/line_projection_factor.cpp:18-231
//   LineOrthParameterization::Plus                            factor/line_parameterization.cpp:10-95 (ComputeJacobian = I)
//   ceres::CauchyLoss + the corrector of the residual block   (rho'' < 0: r and J scaled by sqrt(rho'))
//   FeatureManager::removeLineOutlier / reprojection_error    estimator/feature_manager.cpp:1126-1150, 1372-1460
// Plücker lines are [n(3) | v(3)] (moment, direction); orthonormal lines [theta(3) | phi]. Poses are [p(3) | q(x, y, z, w)].
#pragma once
#include "gfbe_math.h"
#ifdef GFBE_NFRAMES      // (a kernel translation unit: line_rank scans with block_exclusive_scan)
#include "gfbe_tabstage.h"
#endif

namespace gfd {

GF_HD vec3 lcross(const vec3 &a, const vec3 &b) {
  return mk3(a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]);
}
GF_HD double lnorm3(const vec3 &a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// R(theta) = Rz(theta2) Ry(theta1) Rx(theta0), written out as the reference does (line_geometry.cpp:84-94)
GF_HD mat3 line_theta_rot(double t0, double t1, double t2) {
  const double s1 = sin(t0), c1 = cos(t0), s2 = sin(t1), c2 = cos(t1), s3 = sin(t2), c3 = cos(t2);
  mat3 R;
  R.m[0] = c2 * c3; R.m[1] = s1 * s2 * c3 - c1 * s3; R.m[2] = c1 * s2 * c3 + s1 * s3;
  R.m[3] = c2 * s3; R.m[4] = s1 * s2 * s3 + c1 * c3; R.m[5] = c1 * s2 * s3 - s1 * c3;
  R.m[6] = -s2;     R.m[7] = s1 * c2;                R.m[8] = c1 * c2;
  return R;
}

// orth -> Plücker: n = cos(phi) u1, v = sin(phi) u2 (u1, u2 the first two columns of R(theta))
GF_HD void line_orth_to_plk(const double *o, double *plk) {
  const mat3 R = line_theta_rot(o[0], o[1], o[2]);
  const double w1 = cos(o[3]), w2 = sin(o[3]);
  for (int a = 0; a < 3; a++) { plk[a] = w1 * R(a, 0); plk[3 + a] = w2 * R(a, 1); }
}

// Plücker -> orth (any scale of the line; the result describes the normalised line)
GF_HD void line_plk_to_orth(const double *plk, double *o) {
  const vec3 n = ld3(plk), v = ld3(plk + 3);
  const double nn = lnorm3(n), vn = lnorm3(v);
  const vec3 u1 = mk3(n[0] / nn, n[1] / nn, n[2] / nn), u2 = mk3(v[0] / vn, v[1] / vn, v[2] / vn);
  const vec3 u3 = lcross(u1, u2);
  o[0] = atan2(u2[2], u3[2]);
  o[1] = asin(-u1[2]);
  o[2] = atan2(u1[1], u1[0]);
  const double wn = sqrt(nn * nn + vn * vn);
  o[3] = asin(vn / wn);
}

// plk_to_pose(plk, Rcw, tcw): the line expressed in the frame that (Rcw, tcw) maps into
GF_HD void line_plk_to_pose(const double *plk, const mat3 &R, const vec3 &t, double *out) {
  const vec3 Rv = mv(R, ld3(plk + 3));
  const vec3 nc = add(mv(R, ld3(plk)), lcross(t, Rv));
  for (int a = 0; a < 3; a++) { out[a] = nc[a]; out[3 + a] = Rv[a]; }
}
// plk_from_pose(plk, Rcw, tcw) = plk_to_pose(plk, Rcw^T, -Rcw^T tcw)
GF_HD void line_plk_from_pose(const double *plk, const mat3 &R, const vec3 &t, double *out) {
  line_plk_to_pose(plk, transp(R), neg(tmv(R, t)), out);
}

// LineOrthParameterization::Plus: R <- R Rx(d0) Ry(d1) Rz(d2), W <- W W(d3), back to (theta, phi)
GF_HD void line_orth_plus(const double *x, const double *d, double *out) {
  const mat3 R0 = line_theta_rot(x[0], x[1], x[2]);
  const double cx = cos(d[0]), sx = sin(d[0]), cy = cos(d[1]), sy = sin(d[1]), cz = cos(d[2]), sz = sin(d[2]);
  mat3 Rx, Ry, Rz;
  Rx.m[0] = 1.0; Rx.m[1] = 0.0; Rx.m[2] = 0.0; Rx.m[3] = 0.0; Rx.m[4] = cx; Rx.m[5] = -sx; Rx.m[6] = 0.0; Rx.m[7] = sx; Rx.m[8] = cx;
  Ry.m[0] = cy; Ry.m[1] = 0.0; Ry.m[2] = sy; Ry.m[3] = 0.0; Ry.m[4] = 1.0; Ry.m[5] = 0.0; Ry.m[6] = -sy; Ry.m[7] = 0.0; Ry.m[8] = cy;
  Rz.m[0] = cz; Rz.m[1] = -sz; Rz.m[2] = 0.0; Rz.m[3] = sz; Rz.m[4] = cz; Rz.m[5] = 0.0; Rz.m[6] = 0.0; Rz.m[7] = 0.0; Rz.m[8] = 1.0;
  const mat3 R = mul(mul(mul(R0, Rx), Ry), Rz);
  const double w1 = cos(x[3]), w2 = sin(x[3]), c4 = cos(d[3]), s4 = sin(d[3]);
  const double W10 = w2 * c4 + w1 * s4;      // (W dW)(1, 0)
  out[0] = atan2(R(2, 1), R(2, 2));
  out[1] = asin(-R(2, 0));
  out[2] = atan2(R(1, 0), R(0, 0));
  out[3] = asin(W10);
}

// ceres::CauchyLoss(a) and the corrector of a 2-row residual block: cost = 1/2 rho(s); r, J scaled by sqrt(rho') (rho'' < 0 always)
GF_HD double line_cauchy(double s, double a, double *sqrt_rho1) {
  const double b = a * a, c = 1.0 / b;
  const double sum = 1.0 + s * c, inv = 1.0 / sum;
  *sqrt_rho1 = sqrt(fmax(2.2250738585072014e-308, inv));
  return 0.5 * (b * log(sum));
}

// lineProjectionFactor::Evaluate. Pose / extrinsic as rotation + translation (PoseRT-like), orth [4], obs [4] = the two endpoints on
// the normalised image plane. r [2]; if JAC: Jp, Je [2][7] (tangent columns dp(3) dtheta(3), the 7th zero), Jo [2][4].
struct LineRT { vec3 t; mat3 R; };
GF_HD LineRT line_make_pose(const double *p7) { LineRT o; o.t = ld3(p7); o.R = qrot(ldq(p7 + 3)); return o; }

template <bool JAC>
GF_HD void line_factor(const LineRT &B, const LineRT &E, const double *orth, const double *obs, double sqrt_info, double *r, double *Jp,
                       double *Je, double *Jo) {
  double lw[6], lb[6], lc[6];
  line_orth_to_plk(orth, lw);
  line_plk_from_pose(lw, B.R, B.t, lb);
  line_plk_from_pose(lb, E.R, E.t, lc);
  const double l_norm = lc[0] * lc[0] + lc[1] * lc[1];
  const double l_sqrt = sqrt(l_norm), l_tri = l_norm * l_sqrt;
  const double e1 = obs[0] * lc[0] + obs[1] * lc[1] + lc[2];
  const double e2 = obs[2] * lc[0] + obs[3] * lc[1] + lc[2];
  r[0] = sqrt_info * (e1 / l_sqrt);
  r[1] = sqrt_info * (e2 / l_sqrt);
  if (!JAC) return;
  // d e / d nc (2 x 3), sqrt_info applied; the direction part of line_c does not enter the residual
  double jel[6] = {obs[0] / l_sqrt - lc[0] * e1 / l_tri, obs[1] / l_sqrt - lc[1] * e1 / l_tri, 1.0 / l_sqrt,
                   obs[2] / l_sqrt - lc[0] * e2 / l_tri, obs[3] / l_sqrt - lc[1] * e2 / l_tri, 1.0 / l_sqrt};
  for (int q = 0; q < 6; q++) jel[q] = sqrt_info * jel[q];
  // J = jel * M for a 3 x 3 block M, into columns [c0, c0 + 3) of a row-major matrix with `ld` columns
  auto put = [&](double *J, int ld, int c0, const mat3 &M) {
    for (int i = 0; i < 2; i++)
      for (int b = 0; b < 3; b++) J[i * ld + c0 + b] = jel[3 * i] * M(0, b) + jel[3 * i + 1] * M(1, b) + jel[3 * i + 2] * M(2, b);
  };
  if (Jp) {   // top rows of invTbc * dLb/d(pose): Rbc^T [Rwb^T [dw]x | [Rwb^T (nw + [dw]x twb)]x] - Rbc^T [tbc]x [0 | [Rwb^T dw]x]
    const vec3 nw = ld3(lw), dw = ld3(lw + 3);
    const mat3 Mt = tmul(E.R, tmul(B.R, hat(dw)));
    const mat3 Mth = msub(tmul(E.R, hat(tmv(B.R, add(nw, lcross(dw, B.t))))), tmul(E.R, mul(hat(E.t), hat(tmv(B.R, dw)))));
    put(Jp, 7, 0, Mt); put(Jp, 7, 3, Mth);
    Jp[6] = 0.0; Jp[13] = 0.0;
  }
  if (Je) {
    const vec3 nb = ld3(lb), db = ld3(lb + 3);
    put(Je, 7, 0, tmul(E.R, hat(db))); put(Je, 7, 3, hat(tmv(E.R, add(nb, lcross(db, E.t)))));
    Je[6] = 0.0; Je[13] = 0.0;
  }
  if (Jo) {   // jel * [Rwc^T, -Rwc^T [twc]x] * dLw/d(orth)
    const mat3 Rwc = mul(B.R, E.R);
    const vec3 twc = add(mv(B.R, E.t), B.t);
    const vec3 nw = ld3(lw), vw = ld3(lw + 3);
    const double nn = lnorm3(nw), vn = lnorm3(vw);
    const vec3 u1 = mk3(nw[0] / nn, nw[1] / nn, nw[2] / nn), u2 = mk3(vw[0] / vn, vw[1] / vn, vw[2] / vn), u3 = lcross(u1, u2);
    const double wn = sqrt(nn * nn + vn * vn), w0 = nn / wn, w1 = vn / wn;
    // columns of dLw/d(orth): n part Ln, v part Lv (3 x 4 each)
    vec3 Ln[4], Lv[4];
    Ln[0] = mk3(0.0, 0.0, 0.0);  Lv[0] = scl(w1, u3);
    Ln[1] = scl(-w0, u3);        Lv[1] = mk3(0.0, 0.0, 0.0);
    Ln[2] = scl(w0, u2);         Lv[2] = scl(-w1, u1);
    Ln[3] = scl(-w1, u1);        Lv[3] = scl(w0, u2);
    const mat3 Tw = tmul(Rwc, hat(twc));      // Rwc^T [twc]x
    for (int k = 0; k < 4; k++) {
      const vec3 c = sub(tmv(Rwc, Ln[k]), mv(Tw, Lv[k]));
      for (int i = 0; i < 2; i++) Jo[i * 4 + k] = jel[3 * i] * c[0] + jel[3 * i + 1] * c[1] + jel[3 * i + 2] * c[2];
    }
  }
}

// ---- the line loops of optimizationwithLine (estimator.cpp:4566-4598, 4736-4771): per-line pieces of the reduced normal equations
//      (csrc/gfbe_line_reduce.hip; compiled for the host by tests/line_reduce_host_shim.cpp)
// ceres::HuberLoss(a): returns 1/2 rho(s), *sqrt_rho1 = sqrt(rho'(s)) (rho'' <= 0: the corrector scales r and J by it). a <= 0: no loss.
GF_HD double line_huber(double s, double a, double *sqrt_rho1) {
  const double b = a * a;
  if (a > 0.0 && s > b) {
    const double r = sqrt(s);
    *sqrt_rho1 = sqrt(fmax(2.2250738585072014e-308, a / r));
    return 0.5 * (2.0 * a * r - b);
  }
  *sqrt_rho1 = 1.0;
  return 0.5 * s;
}
// V' = V + mu diag(clamp(diag V, 1e-6, 1e32)); Vinv = V'^-1 through the Cholesky factor (lower triangle computed, mirrored: symmetric
// bit for bit). false: a pivot that is not positive and finite — Vinv is then not written.
GF_HD bool line_chol4_inv(const double *V, double mu, double *Vinv) {
  double L[16], M[16];
  for (int q = 0; q < 16; q++) { L[q] = 0.0; M[q] = 0.0; }
  for (int j = 0; j < 4; j++) {
    double d = V[5 * j] + mu * fmin(fmax(V[5 * j], 1e-6), 1e32);
    for (int k = 0; k < j; k++) d -= L[4 * j + k] * L[4 * j + k];
    if (!(d > 0.0 && d <= 1.7976931348623157e308)) return false;
    const double ljj = sqrt(d);
    L[5 * j] = ljj;
    for (int i = j + 1; i < 4; i++) {
      double s = V[4 * i + j];
      for (int k = 0; k < j; k++) s -= L[4 * i + k] * L[4 * j + k];
      L[4 * i + j] = s / ljj;
    }
  }
  for (int j = 0; j < 4; j++) {      // M = L^-1, column by column
    M[5 * j] = 1.0 / L[5 * j];
    for (int i = j + 1; i < 4; i++) {
      double s = 0.0;
      for (int k = j; k < i; k++) s -= L[4 * i + k] * M[4 * k + j];
      M[4 * i + j] = s / L[5 * i];
    }
  }
  for (int i = 0; i < 4; i++)        // Vinv = M^T M
    for (int j = 0; j <= i; j++) {
      double s = 0.0;
      for (int k = i; k < 4; k++) s += M[4 * k + i] * M[4 * k + j];
      Vinv[4 * i + j] = s; Vinv[4 * j + i] = s;
    }
  return true;
}
// One line with m observations in frames start .. start + m - 1, the first k0 of them skipped, at the world line `orth`:
//   Wrow [72][4]: W_l = sum Jp^T Jl (rows 6 f .. 6 f + 5 of an observing pose f, rows 66 .. 71 the extrinsic, zero elsewhere)
//   Jrec [m][LINE_JREC]: per observation r (2), Jp (2 x 6), Je (2 x 6) after the loss — what U and bp are summed from
//   V'^-1 [4][4], bl [4], cost = sum 1/2 rho.   Returns false when V' has no Cholesky factor.
//   Vlow [10] (optional): the lower triangle of V_l without the mu term, row-major — the record of the step side (gfbe_line_step.hip)
enum { LINE_JREC = 26, LINE_NP = 72 };
GF_HD bool line_reduce_line(const LineRT *Bs, const LineRT &Ex, const double *orth, int start, int k0, int m, const double *ob,
                            double sqrt_info, double huber, double mu, double *Wrow, double *Jrec, double *Vinv, double *bl, double *cost,
                            double *Vlow = nullptr) {
  double V[16], b4[4], We[24], c = 0.0;
  for (int q = 0; q < 16; q++) V[q] = 0.0;
  for (int q = 0; q < 4; q++) b4[q] = 0.0;
  for (int q = 0; q < 24; q++) We[q] = 0.0;
  for (int q = 0; q < LINE_NP * 4; q++) Wrow[q] = 0.0;
  for (int k = k0; k < m; k++) {
    double r[2], Jp[14], Je[14], Jo[8], sr;
    line_factor<true>(Bs[start + k], Ex, orth, ob + 4 * k, sqrt_info, r, Jp, Je, Jo);
    c += line_huber(r[0] * r[0] + r[1] * r[1], huber, &sr);
    double *rec = Jrec + (size_t)LINE_JREC * k;
    rec[0] = r[0] = r[0] * sr; rec[1] = r[1] = r[1] * sr;
    for (int i = 0; i < 2; i++)
      for (int a = 0; a < 6; a++) {
        rec[2 + 6 * i + a] = Jp[7 * i + a] = Jp[7 * i + a] * sr;
        rec[14 + 6 * i + a] = Je[7 * i + a] = Je[7 * i + a] * sr;
      }
    for (int q = 0; q < 8; q++) Jo[q] *= sr;
    double *Wp = Wrow + 24 * (start + k);
    for (int a = 0; a < 4; a++) {
      b4[a] += Jo[a] * r[0] + Jo[4 + a] * r[1];
      for (int b = 0; b < 4; b++) V[4 * a + b] += Jo[a] * Jo[b] + Jo[4 + a] * Jo[4 + b];
    }
    for (int a = 0; a < 6; a++)
      for (int b = 0; b < 4; b++) {
        Wp[4 * a + b] = Jp[a] * Jo[b] + Jp[7 + a] * Jo[4 + b];
        We[4 * a + b] += Je[a] * Jo[b] + Je[7 + a] * Jo[4 + b];
      }
  }
  for (int q = 0; q < 24; q++) Wrow[4 * 66 + q] = We[q];
  for (int q = 0; q < 4; q++) bl[q] = b4[q];
  *cost = c;
  if (Vlow)
    for (int i = 0, q = 0; i < 4; i++)
      for (int j = 0; j <= i; j++) Vlow[q++] = V[4 * i + j];
  return line_chol4_inv(V, mu, Vinv);
}
// Y = W V'^-1, one row
GF_HD void line_Y_row(const double *w, const double *Vinv, double *y) {
  for (int a = 0; a < 4; a++) y[a] = w[0] * Vinv[a] + w[1] * Vinv[4 + a] + w[2] * Vinv[8 + a] + w[3] * Vinv[12 + a];
}

// ---- the step half of a joint iteration over the line blocks (csrc/gfbe_line_step.hip, include/gfbe.h: gfbe_line_step; compiled for
//      the host by tests/line_step_host_shim.cpp). The scalar landmark code of the window solve (k_lm_step, k_step, k_candidate)
//      generalised to a 4-dimensional block: line columns unscaled, the block's metric d2 = clamp(diag V, 1e-6, 1e32).
// One line's back-substitution and dogleg shares. W [72][4], Vinv [16], bl [4], Vlow [10] (lower triangle of V without mu), yp / vp [72]
// the pose / extrinsic Gauss-Newton and Cauchy directions, x [4] the line. yl = Vinv (bl - W^T yp), vl = bl / d2,
// p = [G2, N2, gy, vHv, vHy, yHy, |x - Plus(x, -bl)|_inf, |x|^2]. W is streamed once for both products.
GF_HD void line_step_shares(const double *W, const double *Vinv, const double *bl, const double *Vlow, const double *yp, const double *vp,
                            const double *x, double *yl, double *vl, double *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  W = (const double *)__builtin_assume_aligned(W, 32);      // (a record: 2304 bytes from a 256-byte aligned base)
#endif
  double wy[4] = {0.0, 0.0, 0.0, 0.0}, wv[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < 72; r++) {
    const double w0 = W[4 * r], w1 = W[4 * r + 1], w2 = W[4 * r + 2], w3 = W[4 * r + 3], y = yp[r], v = vp[r];
    wy[0] += w0 * y; wy[1] += w1 * y; wy[2] += w2 * y; wy[3] += w3 * y;
    wv[0] += w0 * v; wv[1] += w1 * v; wv[2] += w2 * v; wv[3] += w3 * v;
  }
  double V[16], d2[4], rhs[4];
  for (int i = 0, q = 0; i < 4; i++)
    for (int j = 0; j <= i; j++) { V[4 * i + j] = Vlow[q]; V[4 * j + i] = Vlow[q]; q++; }
  for (int a = 0; a < 4; a++) { d2[a] = fmin(fmax(V[5 * a], 1e-6), 1e32); vl[a] = bl[a] / d2[a]; rhs[a] = bl[a] - wy[a]; }
  for (int a = 0; a < 4; a++) yl[a] = Vinv[4 * a] * rhs[0] + Vinv[4 * a + 1] * rhs[1] + Vinv[4 * a + 2] * rhs[2] + Vinv[4 * a + 3] * rhs[3];
  double Vv[4], Vy[4];
  for (int a = 0; a < 4; a++) {
    Vv[a] = V[4 * a] * vl[0] + V[4 * a + 1] * vl[1] + V[4 * a + 2] * vl[2] + V[4 * a + 3] * vl[3];
    Vy[a] = V[4 * a] * yl[0] + V[4 * a + 1] * yl[1] + V[4 * a + 2] * yl[2] + V[4 * a + 3] * yl[3];
  }
  for (int k = 0; k < 8; k++) p[k] = 0.0;
  double vwv = 0.0, vwy = 0.0, ywv = 0.0, ywy = 0.0, vVv = 0.0, vVy = 0.0, yVy = 0.0;
  for (int a = 0; a < 4; a++) {
    p[0] += bl[a] * bl[a] / d2[a];
    p[1] += d2[a] * yl[a] * yl[a];
    p[2] += bl[a] * yl[a];
    vwv += vl[a] * wv[a]; vwy += vl[a] * wy[a]; ywv += yl[a] * wv[a]; ywy += yl[a] * wy[a];
    vVv += vl[a] * Vv[a]; vVy += vl[a] * Vy[a]; yVy += yl[a] * Vy[a];
    p[7] += x[a] * x[a];
  }
  p[3] = 2.0 * vwv + vVv;
  p[4] = vwy + ywv + vVy;
  p[5] = 2.0 * ywy + yVy;
  double nb[4] = {-bl[0], -bl[1], -bl[2], -bl[3]}, xm[4];
  line_orth_plus(x, nb, xm);
  for (int a = 0; a < 4; a++) p[6] = fmax(p[6], fabs(x[a] - xm[a]));
}
// DoglegStrategy::ComputeStep's three branches and the model change, from the window's totals T = [G2, N2, gy, vHv, vHy, yHy, ..]
// (the rule of k_step, gfbe_kernels.hip, restated): step = c1 v + c2 y. coef = [c1, c2, step_norm, model_change]; returns the branch:
// 0 Gauss-Newton step inside the radius, 1 Cauchy point on or outside it, 2 the dogleg's crossing of the boundary.
GF_HD int line_dogleg(const double *T, double radius, double *coef) {
  const double G2 = T[0], N2 = T[1], gy = T[2], vHv = T[3], vHy = T[4], yHy = T[5];
  const double alpha = G2 / vHv;
  const double g_norm = sqrt(G2), gn_norm = sqrt(N2);
  double c1, c2, step_norm;
  int branch;
  if (gn_norm <= radius) { c1 = 0.0; c2 = -1.0; step_norm = gn_norm; branch = 0; }
  else if (g_norm * alpha >= radius) { c1 = -radius / g_norm; c2 = 0.0; step_norm = radius; branch = 1; }
  else {
    const double b_dot_a = alpha * gy;
    const double a_sq = (alpha * g_norm) * (alpha * g_norm);
    const double bma = a_sq - 2.0 * b_dot_a + N2;
    const double cc = b_dot_a - a_sq;
    const double dd = sqrt(cc * cc + bma * (radius * radius - a_sq));
    const double beta = (cc <= 0.0) ? (dd - cc) / bma : (radius * radius - a_sq) / (dd + cc);
    c1 = -alpha * (1.0 - beta); c2 = -beta;
    step_norm = sqrt(fmax(0.0, c1 * c1 * G2 + 2.0 * c1 * c2 * gy + c2 * c2 * N2));
    branch = 2;
  }
  coef[0] = c1; coef[1] = c2; coef[2] = step_norm;
  coef[3] = -(c1 * G2 + c2 * gy) - 0.5 * (c1 * c1 * vHv + 2.0 * c1 * c2 * vHy + c2 * c2 * yHy);
  return branch;
}
// One line's candidate: xc = Plus(x, c1 vl + c2 yl); its cost (sum of 1/2 rho_huber over its m observations, none skipped) at the
// candidate poses Bc / extrinsic Exc; plk = setLineOrth: xc expressed in the candidate start frame's camera Cs = (Rwc, twc).
GF_HD double line_step_candidate(const LineRT *Bc, const LineRT &Exc, const LineRT &Cs, const double *x, const double *yl, const double *vl,
                                 double c1, double c2, int start, int m, const double *ob, double sqrt_info, double huber, double *xc,
                                 double *plk) {
  double dl[4];
  for (int a = 0; a < 4; a++) dl[a] = c1 * vl[a] + c2 * yl[a];
  line_orth_plus(x, dl, xc);
  double cost = 0.0;
  for (int k = 0; k < m; k++) {
    double r[2], sr;
    line_factor<false>(Bc[start + k], Exc, xc, ob + 4 * k, sqrt_info, r, nullptr, nullptr, nullptr);
    cost += line_huber(r[0] * r[0] + r[1] * r[1], huber, &sr);
  }
  double lw[6];
  line_orth_to_plk(xc, lw);
  line_plk_from_pose(lw, Cs.R, Cs.t, plk);
  return cost;
}

// ---- a batch's line list as the kernels of gfbe_line.hip, gfbe_line_reduce.hip and gfbe_line_step.hip read it. Host-fed (TAB = false):
//      a CSR description packed by the host (upload_line_windows, gfbe_line_batch.h). Table-fed (TAB = true): the device-resident line
//      tables read IN PLACE (ltab_line_list) — window w owns lines [w F, w F + count[w]), line l has nobs[l] observations in its fixed
//      row of GFBE_NFRAMES slots. No scan, no compaction: a line's observations are contiguous either way, so the kernels walk the same
//      values in the same order and the arithmetic is the same instruction for instruction.
struct LineList {
  const int *line_off;          // [n_windows + 1]                          (host-fed)
  const int *obs_off;           // [n_lines + 1] (over the whole batch)     (host-fed)
  const int *count, *nobs;      // [n_windows], [n_windows][F]              (table-fed)
  int F;                        // line capacity of a table                 (table-fed)
  const int *start;             // [n_lines]
  const unsigned char *tri;     // [n_lines]
  const double *plk_in;         // [n_lines][6]
  const double *obs;            // [n_obs][4]
  const double *pose;           // [n_windows][11][7]
  const double *ex;             // [n_windows][7]
};

#if defined(__HIPCC__) && defined(GFBE_NFRAMES)      // (the kernels include gfbe_device.h first; the host shims of the tests do not know the ABI header)
template <bool TAB>
__device__ __forceinline__ int line_nobs(const LineList &L, int l) { return TAB ? L.nobs[l] : L.obs_off[l + 1] - L.obs_off[l]; }
template <bool TAB>
__device__ __forceinline__ const double *line_obs(const LineList &L, int l) {
  return L.obs + 4 * (TAB ? (size_t)l * GFBE_NFRAMES : (size_t)L.obs_off[l]);
}
template <bool TAB>
__device__ __forceinline__ bool line_eligible(const LineList &L, int l) {
  return line_nobs<TAB>(L, l) >= 5 && L.start[l] < GFBE_WINDOW_SIZE - 2 && L.tri[l];   // LINE_MIN_OBS, WINDOW_SIZE - 2
}
// the lines [*l0, *l1) of window w
template <bool TAB>
__device__ __forceinline__ void line_range(const LineList &L, int w, int *l0, int *l1) {
  *l0 = TAB ? w * L.F : L.line_off[w];
  *l1 = TAB ? *l0 + L.count[w] : L.line_off[w + 1];
}
// A window's prologue, in two halves with a workgroup barrier between them (the barrier stays in the kernel, which stages its own
// data beside these): the poses and the extrinsic of window w into LDS, then the cameras Rwc = Rs ric, twc = Ps + Rs tic.
__device__ __forceinline__ void line_stage_poses(const LineList &L, int w, LineRT *Bs, LineRT *Ex) {
  const int t = threadIdx.x;
  if (t < GFBE_NFRAMES) Bs[t] = line_make_pose(L.pose + (size_t)w * 77 + 7 * t);
  if (t == GFBE_NFRAMES) *Ex = line_make_pose(L.ex + (size_t)w * 7);
}
__device__ __forceinline__ void line_stage_cameras(const LineRT *Bs, const LineRT &Ex, LineRT *Cw) {
  const int t = threadIdx.x;
  if (t < GFBE_NFRAMES) { Cw[t].R = mul(Bs[t].R, Ex.R); Cw[t].t = add(Bs[t].t, mv(Bs[t].R, Ex.t)); }
}
// Fixed-order reduction of NQ per-thread values over a workgroup of WAVES waves: the shuffle tree within a wave, then the waves in
// index order starting from 0.0; bit q of maxmask: entry q is a maximum (fmax(0.0, .)) instead of a sum. Every thread gets all NQ
// results in v. sh: NQ * WAVES doubles of LDS. The order — and so every bit — is that of block_reduce_multi (gfbe_devutil.h); this one
// runs the NQ trees interleaved in one basic block and has every thread add the waves' values itself, two barriers in all:
// block_reduce_multi's tree-and-store per quantity and its third barrier measured 5 - 10 % on a window's time in k_line_step and 2 % in
// k_line_refine, whose windows are a few dozen microseconds of dependent work between reductions.
template <int NQ, int WAVES>
__device__ __forceinline__ void line_block_reduce(double (&v)[NQ], unsigned maxmask, double *sh) {
  const int t = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const double u = __shfl_down(v[q], o, 64);
      v[q] = ((maxmask >> q) & 1) ? fmax(v[q], u) : v[q] + u;
    }
  if ((t & 63) == 0)
#pragma unroll
    for (int q = 0; q < NQ; q++) sh[q * WAVES + (t >> 6)] = v[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < WAVES; k++) a = ((maxmask >> q) & 1) ? fmax(a, sh[q * WAVES + k]) : a + sh[q * WAVES + k];
    v[q] = a;
  }
  __syncthreads();
}
// rank: the lines of [l0, l1) that `enters` admits, in list order (block scan) — lineof[q] = the q-th of them, for q < cap (nothing is
// written past the slots); returns their count, at most cap. The caller fences and barriers before it reads lineof.
template <int THREADS, class Pred>
__device__ __forceinline__ int line_rank(int l0, int l1, Pred enters, int *lineof, int *scan_lds /* >= 17 ints */, int cap = 0x7fffffff) {
  int n = 0;
  for (int c0 = l0; c0 < l1; c0 += THREADS) {
    const int l = c0 + (int)threadIdx.x;
    const int e = (l < l1 && enters(l)) ? 1 : 0;
    int total;
    const int at = n + block_exclusive_scan<THREADS>(e, &total, scan_lds);
    if (e && at < cap) lineof[at] = l;
    n += total;
  }
  return min(n, cap);
}
#endif

// ---- removeLineOutlier (feature_manager.cpp:1372-1460)
// pi_from_ppp(x1, x2, x3) with x1 = the camera centre (0): [(x1 - x3) x (x2 - x3) | -x3 . (x1 x x2)]
GF_HD void line_plane_through_origin(const vec3 &x2, const vec3 &x3, double *pi) {
  const vec3 z = mk3(0.0, 0.0, 0.0);
  const vec3 c = lcross(sub(z, x3), sub(x2, x3));
  pi[0] = c[0]; pi[1] = c[1]; pi[2] = c[2];
  pi[3] = -dot3(x3, lcross(z, x2));
}
// The endpoint test on the start-frame Plücker line (camera frame) and its first observation: true = erase (an endpoint behind the
// camera, or the two endpoints more than 10 apart). Endpoints e = Lc pi / (Lc pi)[3], Lc = [[n]x v; -v^T 0].
GF_HD bool line_endpoints_bad(const double *plk_c, const double *obs0) {
  const vec3 nc = ld3(plk_c), vc = ld3(plk_c + 3);
  const vec3 p11 = mk3(obs0[0], obs0[1], 1.0), p21 = mk3(obs0[2], obs0[3], 1.0);
  const vec3 l = lcross(p11, p21);
  const double ln = sqrt(l[0] * l[0] + l[1] * l[1]), lx = l[0] / ln, ly = l[1] / ln;
  const vec3 p12 = mk3(p11[0] + lx, p11[1] + ly, 1.0), p22 = mk3(p21[0] + lx, p21[1] + ly, 1.0);
  double pi1[4], pi2[4], e1[4], e2[4];
  line_plane_through_origin(p11, p12, pi1);
  line_plane_through_origin(p21, p22, pi2);
  const mat3 N = hat(nc);
  for (int a = 0; a < 3; a++) {
    e1[a] = N(a, 0) * pi1[0] + N(a, 1) * pi1[1] + N(a, 2) * pi1[2] + vc[a] * pi1[3];
    e2[a] = N(a, 0) * pi2[0] + N(a, 1) * pi2[1] + N(a, 2) * pi2[2] + vc[a] * pi2[3];
  }
  e1[3] = -vc[0] * pi1[0] - vc[1] * pi1[1] - vc[2] * pi1[2] + 0.0 * pi1[3];
  e2[3] = -vc[0] * pi2[0] - vc[1] * pi2[1] - vc[2] * pi2[2] + 0.0 * pi2[3];
  const double d1 = e1[3], d2 = e2[3];
  for (int a = 0; a < 4; a++) { e1[a] = e1[a] / d1; e2[a] = e2[a] / d2; }
  if (e1[2] < 0 || e2[2] < 0) return true;
  double s = 0.0;
  for (int a = 0; a < 4; a++) s += (e1[a] - e2[a]) * (e1[a] - e2[a]);
  return sqrt(s) > 10;
}
// FeatureManager::reprojection_error: mean distance of the two observed endpoints to the projected line (camera pose Rwc, twc)
GF_HD double line_reprojection_error(const double *obs, const mat3 &Rwc, const vec3 &twc, const double *line_w) {
  double lc[6];
  line_plk_from_pose(line_w, Rwc, twc, lc);
  const double sql = sqrt(lc[0] * lc[0] + lc[1] * lc[1]);
  const double n0 = lc[0] / sql, n1 = lc[1] / sql, n2 = lc[2] / sql;
  double err = 0.0;
  err += fabs(n0 * obs[0] + n1 * obs[1] + n2);
  err += fabs(n0 * obs[2] + n1 * obs[3] + n2);
  return err / 2.0;
}

}  // namespace gfd
