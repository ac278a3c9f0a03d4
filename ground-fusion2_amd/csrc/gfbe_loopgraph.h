// gfbe_loopgraph.h — the HIP-free half of the loop-closure pose graph (gfbe_loopgraph.hip): the 4-DoF factor with its analytic
// tangent Jacobian, the Huber corrector and the plan of a solve (super-block count, padding, sweep count, panel width, scratch
// carve). No HIP call and no HIP header: a plain C++ compiler builds it for the host (tests/lc4_host_shim.cpp).
//
//   PoseGraph::optimize4DoF             dense_map/src/pose_graph.cpp:529-705
//   FourDOFError, FourDOFWeightError    dense_map/src/pose_graph.h:199-288
//   NormalizeAngle, YawPitchRollToRotationMatrix                 :129-175
//
// A pose is yaw (degrees) + t(3), pitch and roll frozen into the factor's measurement; its tangent is [yaw, t_x, t_y, t_z].
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LC4_HD __host__ __device__
#else
#define LC4_HD
#endif

namespace gfd {

constexpr int LC4_MAX_LOOPS = 64;      // GFBE_LC4_MAX_LOOPS: the capacitance system stays within 16 tile columns
constexpr int LC4_LONG_MAX_LOOPS = 512;      // GFBE_LC4_LONG_MAX_LOOPS: 128 tile columns, factorised across workgroups (gfbe_lc4_solve_long)
constexpr int LC4_SB = 16;             // a super-block: four consecutive poses x four tangent dimensions
constexpr int LC4_MAX_SPAN = 4;        // sequence edges reach at most four poses back: neighbours share or touch a super-block

LC4_HD inline double lc4_normalize_angle(double a) { return a > 180.0 ? a - 360.0 : (a < -180.0 ? a + 360.0 : a); }

LC4_HD inline void lc4_ypr_to_R(double yaw, double pitch, double roll, double *R) {
  const double y = yaw / 180.0 * M_PI, p = pitch / 180.0 * M_PI, r = roll / 180.0 * M_PI;
  const double cy = cos(y), sy = sin(y), cp = cos(p), sp = sin(p), cr = cos(r), sr = sin(r);
  R[0] = cy * cp; R[1] = -sy * cr + cy * sp * sr; R[2] = sy * sr + cy * sp * cr;
  R[3] = sy * cp; R[4] = cy * cr + sy * sp * sr; R[5] = -cy * sr + sy * sp * cr;
  R[6] = -sp; R[7] = cp * sr; R[8] = cp * cr;
}

// r(4) and J (4 x 8, row-major, columns yaw_i t_i(3) yaw_j t_j(3)) of one edge; meas = [t_x t_y t_z relative_yaw pitch_i roll_i].
// yaw_w = 1 for FourDOFError, 1 / loop_yaw_div for FourDOFWeightError (whose `weight` is the constant 1). J may be NULL.
// d R / d yaw: row 0' = -row 1, row 1' = row 0, row 2' = 0 (R = Rz(yaw) Ry(pitch) Rx(roll)), per degree: pi / 180.
LC4_HD inline void lc4_factor(double yaw_i, const double *ti, double yaw_j, const double *tj, const double *meas, double yaw_w, double *r, double *J) {
  double R[9];
  lc4_ypr_to_R(yaw_i, meas[4], meas[5], R);
  const double d0 = tj[0] - ti[0], d1 = tj[1] - ti[1], d2 = tj[2] - ti[2];
  for (int a = 0; a < 3; a++) r[a] = (R[a] * d0 + R[3 + a] * d1 + R[6 + a] * d2) - meas[a];
  r[3] = lc4_normalize_angle(yaw_j - yaw_i - meas[3]) * yaw_w;
  if (!J) return;
  for (int a = 0; a < 3; a++) {
    J[a * 8 + 0] = (R[a] * d1 - R[3 + a] * d0) * (M_PI / 180.0);
    J[a * 8 + 4] = 0.0;
    for (int b = 0; b < 3; b++) { J[a * 8 + 1 + b] = -R[3 * b + a]; J[a * 8 + 5 + b] = R[3 * b + a]; }
  }
  for (int b = 0; b < 8; b++) J[24 + b] = 0.0;
  J[24 + 0] = -yaw_w; J[24 + 4] = yaw_w;
}

// ceres::HuberLoss + Corrector (the statements of the f3 restatement): returns rho(s) / 2; a row of J becomes
// s1 (J - asn r r^T J), r becomes rs r.
LC4_HD inline double lc4_huber_corrector(double sq, double delta, double *s1, double *rs, double *asn) {
  const double b = delta * delta;
  double rho0, rho1, rho2;
  if (sq > b) { const double rr = sqrt(sq); rho0 = 2 * delta * rr - b; rho1 = fmax(1e-300, delta / rr); rho2 = -rho1 / (2 * sq); }
  else { rho0 = sq; rho1 = 1.0; rho2 = 0.0; }
  const double sqrt_rho1 = sqrt(rho1);
  if (sq == 0.0 || rho2 <= 0.0) { *s1 = sqrt_rho1; *rs = sqrt_rho1; *asn = 0.0; }
  else { const double D = 1.0 + 2.0 * sq * rho2 / rho1, alpha = 1.0 - sqrt(D); *s1 = sqrt_rho1; *rs = sqrt_rho1 / (1.0 - alpha); *asn = alpha / sq; }
  return 0.5 * rho0;
}

// One edge as the solver sees it: kind 1 goes through the corrector. Returns the edge's cost (loss included).
LC4_HD inline double lc4_edge(int kind, double yaw_i, const double *ti, double yaw_j, const double *tj, const double *meas, double delta, double yaw_div, double *r,
                              double *J) {
  lc4_factor(yaw_i, ti, yaw_j, tj, meas, kind ? 1.0 / yaw_div : 1.0, r, J);
  const double sq = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
  if (!kind) return 0.5 * sq;
  double s1, rs, asn;
  const double c = lc4_huber_corrector(sq, delta, &s1, &rs, &asn);
  if (J)
    for (int b = 0; b < 8; b++) {
      double rj = 0.0;
      for (int q = 0; q < 4; q++) rj += r[q] * J[q * 8 + b];
      for (int q = 0; q < 4; q++) J[q * 8 + b] = s1 * (J[q * 8 + b] - asn * r[q] * rj);
    }
  for (int q = 0; q < 4; q++) r[q] *= rs;
  return c;
}

// The measurement the library forms for the sequence edge (a, b) from the input poses (pose_graph.cpp:610-615; the rotation through
// YawPitchRollToRotationMatrix instead of the quaternion of the same rotation: DESIGN.md §6).
LC4_HD inline void lc4_sequence_meas(const double *ta, const double *ypr_a, const double *tb, const double *ypr_b, double *meas) {
  double R[9];
  lc4_ypr_to_R(ypr_a[0], ypr_a[1], ypr_a[2], R);
  const double d0 = tb[0] - ta[0], d1 = tb[1] - ta[1], d2 = tb[2] - ta[2];
  for (int a = 0; a < 3; a++) meas[a] = R[a] * d0 + R[3 + a] * d1 + R[6 + a] * d2;
  meas[3] = ypr_b[0] - ypr_a[0];      // (left un-normalised, as the reference leaves it)
  meas[4] = ypr_a[1]; meas[5] = ypr_a[2];
}

// ---- the plan of a solve
struct Lc4Plan {
  int n, n_loop;
  int M;            // super-blocks: ceil(n / 4)
  int rows;         // 16 M (the padding poses of the last super-block are identity rows)
  int pad_poses;    // 4 M - n
  int sweeps;       // ceil(log2 M) sweeps of parallel block cyclic reduction
  int ncol;         // columns of the panel [g | U]: 1 + 4 n_loop
  int ld;           // its leading dimension: ncol rounded up to a 16-column tile
  int ntile;        // ld / 16 (tile columns that are computed)
  int cap;          // dimension of the capacitance system, 4 n_loop
  int cap_ld;       // rounded up to a tile (identity padding), at least one tile
  // offsets in doubles into the context's scratch, each a multiple of 32 doubles (256 bytes)
  size_t off_panel[2], off_band[2][4] /* A B C Binv */, off_alpha, off_gamma, off_S, off_L, off_Dinv, off_w, off_y, total;
};

LC4_HD inline size_t lc4_align32(size_t v) { return (v + 31) & ~(size_t)31; }

// false for n < 1 or n_loop outside [0, max_loops]
LC4_HD inline bool lc4_plan_within(int n, int n_loop, int max_loops, Lc4Plan *p) {
  if (n < 1 || n_loop < 0 || n_loop > max_loops) return false;
  p->n = n; p->n_loop = n_loop;
  p->M = (n + 3) / 4;
  p->rows = LC4_SB * p->M;
  p->pad_poses = 4 * p->M - n;
  int s = 0;
  while (((size_t)1 << s) < (size_t)p->M) s++;
  p->sweeps = s;
  p->ncol = 1 + 4 * n_loop;
  p->ntile = (p->ncol + LC4_SB - 1) / LC4_SB;
  p->ld = LC4_SB * p->ntile;
  p->cap = 4 * n_loop;
  p->cap_ld = p->cap ? LC4_SB * ((p->cap + LC4_SB - 1) / LC4_SB) : LC4_SB;
  size_t at = 0;
  const size_t blk = lc4_align32((size_t)p->M * 256), pan = lc4_align32((size_t)p->rows * p->ld);
  for (int q = 0; q < 2; q++) { p->off_panel[q] = at; at += pan; }
  for (int q = 0; q < 2; q++)
    for (int k = 0; k < 4; k++) { p->off_band[q][k] = at; at += blk; }
  p->off_alpha = at; at += blk;
  p->off_gamma = at; at += blk;
  p->off_S = at; at += lc4_align32((size_t)p->cap_ld * p->cap_ld);
  p->off_L = at; at += lc4_align32((size_t)p->cap_ld * p->cap_ld);
  p->off_Dinv = at; at += lc4_align32((size_t)p->cap_ld * LC4_SB);
  p->off_w = at; at += lc4_align32((size_t)p->cap_ld);
  p->off_y = at; at += lc4_align32((size_t)p->rows);
  p->total = at;
  return true;
}
// false for n < 1 or n_loop outside [0, LC4_MAX_LOOPS]
LC4_HD inline bool lc4_plan(int n, int n_loop, Lc4Plan *p) { return lc4_plan_within(n, n_loop, LC4_MAX_LOOPS, p); }

// The plan of gfbe_lc4_solve_long: the same carve up to LC4_LONG_MAX_LOOPS loop edges (off_Dinv holds the cap_ld / 16 pivot tiles'
// inverses, 256 doubles each), and behind it the right-hand side v = U^T z_0 of the capacitance system, which the blocked
// factorisation carries through its forward substitution. p.total includes it: 2 rows ld + 2 cap_ld^2 + 161 rows + 18 cap_ld doubles
// (rounded up to 256-byte units); at n = 5000 with 512 loop edges 2 panels of 20 000 x 2064 and S, L of 2048 x 2048, 0.75 GB in all.
struct Lc4LongPlan {
  Lc4Plan p;
  size_t off_v;      // [cap_ld]
};
LC4_HD inline bool lc4_long_plan(int n, int n_loop, Lc4LongPlan *q) {
  if (!lc4_plan_within(n, n_loop, LC4_LONG_MAX_LOOPS, &q->p)) return false;
  q->off_v = q->p.total;
  q->p.total += lc4_align32((size_t)q->p.cap_ld);
  return true;
}

// The Levenberg-Marquardt loop's state on the device (PgState's fields; the statements of k_pg_decide restated in k_lc4_decide). The
// 6-DoF graph (gfbe_loopgraph6.hip) runs the same loop on the same struct: the capacitance kernels it shares read `done` from it.
struct Lc4State {
  double cost, radius, decrease, x_norm, model_change, step2, cand_x2, initial_cost;
  int it, invalid, reuse, have_scale, done, termination, status, num_successful;
  int cur, lb, cand_on, pad;
  int accepted[16];
  double cost_history[16];
};

// Input validation of gfbe_lc4_solve / gfbe_lc4_solve_long (the GFBE_BAD_INPUT cases that need no device): 0 = fine, else which rule
// failed (2: more than max_loops loop edges).
inline int lc4_check_graph_within(int n, int n_loop, int max_loops, const int32_t *loop_i, const int32_t *loop_c, int span, uint8_t *has_loop /* [n], scratch */) {
  if (n < 1) return 1;
  if (n_loop < 0 || n_loop > max_loops) return 2;
  if (span < 1 || span > LC4_MAX_SPAN) return 3;
  for (int i = 0; i < n; i++) has_loop[i] = 0;
  for (int l = 0; l < n_loop; l++) {
    if (loop_i[l] < 0 || loop_i[l] >= n || loop_c[l] < 0 || loop_c[l] >= n) return 4;
    if (loop_c[l] >= loop_i[l]) return 5;
    if (has_loop[loop_i[l]]) return 6;
    has_loop[loop_i[l]] = 1;
  }
  return 0;
}
inline int lc4_check_graph(int n, int n_loop, const int32_t *loop_i, const int32_t *loop_c, int span, uint8_t *has_loop) {
  return lc4_check_graph_within(n, n_loop, LC4_MAX_LOOPS, loop_i, loop_c, span, has_loop);
}
inline int lc4_long_check_graph(int n, int n_loop, const int32_t *loop_i, const int32_t *loop_c, int span, uint8_t *has_loop) {
  return lc4_check_graph_within(n, n_loop, LC4_LONG_MAX_LOOPS, loop_i, loop_c, span, has_loop);
}

}  // namespace gfd
