// gfbe_loopgraph6.h — the HIP-free half of the 6-DoF loop-closure pose graph (gfbe_loopgraph.hip): the relative-pose factor with its
// analytic tangent Jacobian, the Huber corrector (gfbe_loopgraph.h's), the sequence measurement, QuaternionParameterization::Plus, the
// finiteness check, and the 6-DoF callers of gfbe_loopgraph.h's plan and graph check. No HIP
// call and no HIP header: a plain C++ compiler builds it for the host (tests/lc6_host_shim.cpp).
//
//   PoseGraph::optimize6DoF             dense_map/src/pose_graph.cpp:707-873 (options :736-745)
//   RelativeRTError                     dense_map/src/pose_graph.h:290-352
//
// A pose is q (w, x, y, z) + t(3); its tangent is [dq(3), t(3)] (Ceres orders a residual block's parameter blocks as they were added:
// q_array[i] before t_array[i], :770-771). In the padded system a pose takes 8 rows, the 6 tangent dimensions and 2 identity rows, so
// four poses form one 32 x 32 super-block of 2 x 2 matrix-core tiles and every row index is a shift.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gfbe_loopgraph.h"

// the small fixed-count loops of the factor are unrolled on the device, so that r and J stay in registers
#if defined(__HIPCC__)
#define LC6_UNROLL _Pragma("unroll")
#define LC6_HD __host__ __device__ __forceinline__
#else
#define LC6_UNROLL
#define LC6_HD inline
#endif

namespace gfd {

constexpr int LC6_MAX_LOOPS = 128;     // GFBE_LC6_MAX_LOOPS: the capacitance system has at most 768 rows (48 tile columns)
constexpr int LC6_SB = 32;             // a super-block: four consecutive poses x eight rows
constexpr int LC6_PR = 8;              // rows of a pose in the padded system (6 tangent dimensions + 2 identity rows)
constexpr int LC6_MAX_SPAN = 4;        // sequence edges reach at most four poses back: neighbours share or touch a super-block

// a * b, quaternions as (w, x, y, z); out may not alias
LC6_HD void lc6_qmul(const double *a, const double *b, double *o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
// the conjugate (QuaternionInverse of pose_graph.h: no division by the norm)
LC6_HD void lc6_qconj(const double *a, double *o) { o[0] = a[0]; o[1] = -a[1]; o[2] = -a[2]; o[3] = -a[3]; }

// R(q), row-major, of the normalised quaternion (ceres::QuaternionRotatePoint normalises before it rotates)
LC6_HD void lc6_quat_to_R(const double *q, double *R) {
  const double nn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / nn, x = q[1] / nn, y = q[2] / nn, z = q[3] / nn;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

// r(6) and J (6 x 12, row-major, columns dq_i t_i dq_j t_j) of RelativeRTError (pose_graph.h:300-337); meas = [t(3) | q wxyz].
//   r[0..2] = (R(q_i)^T (t_j - t_i) - meas_t) / t_var          (products left to right per row)
//   r[3..5] = 2 vec(meas_q^-1 (q_i^-1 q_j)) / q_var            (no sign normalisation of the error's w: the reference has none)
// The Jacobian is with respect to the tangent of Plus (q <- [1, d] q to first order): d r_t / d dq_i = 2 R_i^T [t_j - t_i]_x,
// d r_q / d dq_j = 2 (L(meas_q^-1 q_i^-1) R(q_j))[1.., 1..] = -d r_q / d dq_i.
// WITH_J is a template argument, not a test of the pointer: a kernel's J is a private array, and a comparison of its address with NULL
// is not folded on the device and keeps the whole array in scratch memory.
template <bool WITH_J>
LC6_HD void lc6_factor_t(const double *qi, const double *ti, const double *qj, const double *tj, const double *meas, double t_var, double q_var, double *r, double *J) {
  double Ri[9], ci[4], cm[4], A[4], e[4];
  lc6_quat_to_R(qi, Ri);
  const double d[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
  LC6_UNROLL
  for (int a = 0; a < 3; a++) r[a] = (Ri[a] * d[0] + Ri[3 + a] * d[1] + Ri[6 + a] * d[2] - meas[a]) / t_var;
  lc6_qconj(qi, ci);
  lc6_qconj(meas + 3, cm);
  lc6_qmul(cm, ci, A);
  lc6_qmul(A, qj, e);
  r[3] = 2 * e[1] / q_var; r[4] = 2 * e[2] / q_var; r[5] = 2 * e[3] / q_var;
  if (!WITH_J) return;
  const double dx[9] = {0, -d[2], d[1], d[2], 0, -d[0], -d[1], d[0], 0};
  LC6_UNROLL
  for (int a = 0; a < 3; a++)
    LC6_UNROLL
    for (int b = 0; b < 3; b++) {
      double s = 0;
      LC6_UNROLL
      for (int k = 0; k < 3; k++) s += Ri[3 * k + a] * dx[3 * k + b];
      J[a * 12 + b] = 2 * s / t_var;
      J[a * 12 + 3 + b] = -Ri[3 * b + a] / t_var;
      J[a * 12 + 6 + b] = 0.0;      // (r_t does not depend on q_j)
      J[a * 12 + 9 + b] = Ri[3 * b + a] / t_var;
    }
  const double La[16] = {A[0], -A[1], -A[2], -A[3], A[1], A[0], -A[3], A[2], A[2], A[3], A[0], -A[1], A[3], -A[2], A[1], A[0]};
  const double Rj[16] = {qj[0], -qj[1], -qj[2], -qj[3], qj[1], qj[0], qj[3], -qj[2], qj[2], -qj[3], qj[0], qj[1], qj[3], qj[2], -qj[1], qj[0]};
  LC6_UNROLL
  for (int a = 0; a < 3; a++)
    LC6_UNROLL
    for (int b = 0; b < 3; b++) {
      double s = 0;
      LC6_UNROLL
      for (int k = 0; k < 4; k++) s += La[4 * (a + 1) + k] * Rj[4 * k + (b + 1)];
      J[(3 + a) * 12 + 6 + b] = 2 * s / q_var;
      J[(3 + a) * 12 + b] = -2 * s / q_var;
      J[(3 + a) * 12 + 3 + b] = 0.0;      // (r_q does not depend on t_i, t_j)
      J[(3 + a) * 12 + 9 + b] = 0.0;
    }
}

// ... and with J == NULL allowed (host callers)
LC6_HD void lc6_factor(const double *qi, const double *ti, const double *qj, const double *tj, const double *meas, double t_var, double q_var, double *r, double *J) {
  if (J) lc6_factor_t<true>(qi, ti, qj, tj, meas, t_var, q_var, r, J);
  else lc6_factor_t<false>(qi, ti, qj, tj, meas, t_var, q_var, r, J);
}

// One edge as the solver sees it: kind 0 a sequence edge (no loss), kind 1 a loop edge through the Huber corrector
// (pose_graph.cpp:743, :809). Returns the edge's cost (loss included).
template <bool WITH_J>
LC6_HD double lc6_edge_t(int kind, const double *qi, const double *ti, const double *qj, const double *tj, const double *meas, double delta, double t_var, double q_var,
                         double *r, double *J) {
  lc6_factor_t<WITH_J>(qi, ti, qj, tj, meas, t_var, q_var, r, J);
  double sq = 0.0;
  LC6_UNROLL
  for (int q = 0; q < 6; q++) sq += r[q] * r[q];
  if (!kind) return 0.5 * sq;
  double s1, rs, asn;
  const double c = lc4_huber_corrector(sq, delta, &s1, &rs, &asn);
  if (WITH_J) {
    LC6_UNROLL
    for (int b = 0; b < 12; b++) {
      double rj = 0.0;
      LC6_UNROLL
      for (int q = 0; q < 6; q++) rj += r[q] * J[q * 12 + b];
      LC6_UNROLL
      for (int q = 0; q < 6; q++) J[q * 12 + b] = s1 * (J[q * 12 + b] - asn * r[q] * rj);
    }
  }
  LC6_UNROLL
  for (int q = 0; q < 6; q++) r[q] *= rs;
  return c;
}
// ... and with J == NULL allowed (host callers)
LC6_HD double lc6_edge(int kind, const double *qi, const double *ti, const double *qj, const double *tj, const double *meas, double delta, double t_var, double q_var, double *r,
                       double *J) {
  return J ? lc6_edge_t<true>(kind, qi, ti, qj, tj, meas, delta, t_var, q_var, r, J) : lc6_edge_t<false>(kind, qi, ti, qj, tj, meas, delta, t_var, q_var, r, J);
}

// The measurement the library forms for the sequence edge (a, b) from the input poses (pose_graph.cpp:784-788):
// relative_t = R(q_a)^T (t_b - t_a) through the rotation matrix, relative_q = q_a^-1 q_b (the conjugate: input quaternions are unit).
LC4_HD inline void lc6_sequence_meas(const double *ta, const double *qa, const double *tb, const double *qb, double *meas) {
  double R[9], ca[4];
  lc6_quat_to_R(qa, R);
  const double d0 = tb[0] - ta[0], d1 = tb[1] - ta[1], d2 = tb[2] - ta[2];
  for (int a = 0; a < 3; a++) meas[a] = R[a] * d0 + R[3 + a] * d1 + R[6 + a] * d2;
  lc6_qconj(qa, ca);
  lc6_qmul(ca, qb, meas + 3);
}

// ceres::QuaternionParameterization::Plus: out = [cos|d|, sin|d| / |d| d] * q, d = 0 leaves q as it is; no renormalisation
LC6_HD void lc6_plus(const double *q, const double *d, double *out) {
  const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (nd > 0.0) {
    const double sn = sin(nd) / nd, dq[4] = {cos(nd), sn * d[0], sn * d[1], sn * d[2]};
    lc6_qmul(dq, q, out);
  } else {
    for (int k = 0; k < 4; k++) out[k] = q[k];
  }
}

// ---- the plan of a solve (lc_plan of gfbe_loopgraph.h; the capacitance system is always factorised by the blocked kernels, which
// carry v). At n = 5000 with 128 loop edges 2 panels of 40 000 x 784 (0.50 GB), 0.61 GB in all; cap_ld is 768 at the cap.
LC4_HD inline bool lc6_plan(int n, int n_loop, LcPlan *p) { return lc_plan(n, n_loop, LC6_MAX_LOOPS, 6, LC6_PR, true, p); }

// Input validation of gfbe_lc6_solve (the GFBE_BAD_INPUT cases that need no device): 0 = fine, else which rule failed.
inline int lc6_check_graph(int n, int n_loop, const int32_t *loop_i, const int32_t *loop_c, int span, uint8_t *has_loop /* [n], scratch */) {
  return lc_check_graph(n, n_loop, LC6_MAX_LOOPS, LC6_MAX_SPAN, loop_i, loop_c, span, has_loop);
}
// every one of the `count` doubles is finite (rule 7 of gfbe_lc6_solve: a non-finite pose or measurement is refused)
inline bool lc6_all_finite(const double *p, size_t count) {
  for (size_t k = 0; k < count; k++)
    if (!isfinite(p[k])) return false;
  return true;
}

}  // namespace gfd
