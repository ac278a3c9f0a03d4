// gfbe_loopgraph.h — the HIP-free half of the loop-closure pose graph (gfbe_loopgraph.hip): the 4-DoF factor with its analytic
// tangent Jacobian, the Huber corrector, and for both graphs (the 6-DoF factor is gfbe_loopgraph6.h's) the plan of a solve (super-block count, padding, sweep
// count, panel width, scratch carve), the graph check, the graph construction and the loop's state. No HIP call and no HIP header: a plain C++ compiler builds it for the host (tests/lc4_host_shim.cpp).
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

#include <vector>

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

// ---- the plan of a solve, for both graphs: `dof` tangent dimensions per pose (4 or 6), `pose_rows` rows per pose in the padded
// system (4, or 8 = 6 + 2 identity rows), so four consecutive poses form one super-block of 4 pose_rows rows; the panel and the
// capacitance system are padded to the 16-wide matrix-core tile
constexpr int LC_TILE = 16;
struct LcPlan {
  int n, n_loop;
  int M;            // super-blocks: ceil(n / 4)
  int rows;         // 4 pose_rows M (the padding rows of a pose and the padding poses of the last super-block are identity rows)
  int pad_poses;    // 4 M - n
  int sweeps;       // ceil(log2 M) sweeps of parallel block cyclic reduction
  int ncol;         // columns of the panel [g | U]: 1 + dof n_loop
  int ld;           // its leading dimension: ncol rounded up to a 16-column tile
  int ntile;        // ld / 16 (tile columns that are computed)
  int cap;          // dimension of the capacitance system, dof n_loop
  int cap_ld;       // rounded up to a tile (identity padding), at least one tile
  // offsets in doubles into the context's scratch, each a multiple of 32 doubles (256 bytes). off_Dinv holds the cap_ld / 16 pivot
  // tiles' inverses (256 doubles each); off_v, the right-hand side v = U^T z_0 that the blocked factorisation carries through its
  // forward substitution, is carved last and only when asked for (otherwise off_v == total)
  size_t off_panel[2], off_band[2][4] /* A B C Binv */, off_alpha, off_gamma, off_S, off_L, off_Dinv, off_w, off_y, off_v, total;
};

typedef LcPlan Lc4Plan, Lc6Plan;      // (the names the two families' callers use)

LC4_HD inline size_t lc4_align32(size_t v) { return (v + 31) & ~(size_t)31; }

// false for n < 1 or n_loop outside [0, max_loops]. total = 2 rows ld + 10 M (4 pose_rows)^2 + 2 cap_ld^2 + 17 cap_ld + rows doubles
// (+ cap_ld with v), rounded up to 256-byte units
LC4_HD inline bool lc_plan(int n, int n_loop, int max_loops, int dof, int pose_rows, bool with_v, LcPlan *p) {
  if (n < 1 || n_loop < 0 || n_loop > max_loops) return false;
  const int sb = 4 * pose_rows;
  p->n = n; p->n_loop = n_loop;
  p->M = (n + 3) / 4;
  p->rows = sb * p->M;
  p->pad_poses = 4 * p->M - n;
  int s = 0;
  while (((size_t)1 << s) < (size_t)p->M) s++;
  p->sweeps = s;
  p->ncol = 1 + dof * n_loop;
  p->ntile = (p->ncol + LC_TILE - 1) / LC_TILE;
  p->ld = LC_TILE * p->ntile;
  p->cap = dof * n_loop;
  p->cap_ld = p->cap ? LC_TILE * ((p->cap + LC_TILE - 1) / LC_TILE) : LC_TILE;
  size_t at = 0;
  const size_t blk = lc4_align32((size_t)p->M * sb * sb), pan = lc4_align32((size_t)p->rows * p->ld);
  for (int q = 0; q < 2; q++) { p->off_panel[q] = at; at += pan; }
  for (int q = 0; q < 2; q++)
    for (int k = 0; k < 4; k++) { p->off_band[q][k] = at; at += blk; }
  p->off_alpha = at; at += blk;
  p->off_gamma = at; at += blk;
  p->off_S = at; at += lc4_align32((size_t)p->cap_ld * p->cap_ld);
  p->off_L = at; at += lc4_align32((size_t)p->cap_ld * p->cap_ld);
  p->off_Dinv = at; at += lc4_align32((size_t)p->cap_ld * LC_TILE);
  p->off_w = at; at += lc4_align32((size_t)p->cap_ld);
  p->off_y = at; at += lc4_align32((size_t)p->rows);
  p->off_v = at; if (with_v) at += lc4_align32((size_t)p->cap_ld);
  p->total = at;
  return true;
}
// gfbe_lc4_solve: up to LC4_MAX_LOOPS loop edges, the capacitance system in one workgroup (no v)
LC4_HD inline bool lc4_plan(int n, int n_loop, LcPlan *p) { return lc_plan(n, n_loop, LC4_MAX_LOOPS, 4, 4, false, p); }
// gfbe_lc4_solve_long: the same carve up to LC4_LONG_MAX_LOOPS loop edges with v behind it; at n = 5000 with 512 loop edges 2 panels
// of 20 000 x 2064 and S, L of 2048 x 2048, 0.75 GB in all
struct Lc4LongPlan {
  LcPlan p;
  size_t off_v;      // [cap_ld], p.off_v
};
LC4_HD inline bool lc4_long_plan(int n, int n_loop, Lc4LongPlan *q) {
  if (!lc_plan(n, n_loop, LC4_LONG_MAX_LOOPS, 4, 4, true, &q->p)) return false;
  q->off_v = q->p.off_v;
  return true;
}

// The Levenberg-Marquardt loop's state on the device (PgState's fields), for both graphs
struct LcState {
  double cost, radius, decrease, x_norm, model_change, step2, cand_x2, initial_cost;
  int it, invalid, reuse, have_scale, done, termination, status, num_successful;
  int cur, lb, cand_on, pad;
  int accepted[16];
  double cost_history[16];
};

// Input validation of a solve (the GFBE_BAD_INPUT cases that need no device): 0 = fine, else which rule failed (2: more than
// max_loops loop edges).
inline int lc_check_graph(int n, int n_loop, int max_loops, int max_span, const int32_t *loop_i, const int32_t *loop_c, int span, uint8_t *has_loop /* [n], scratch */) {
  if (n < 1) return 1;
  if (n_loop < 0 || n_loop > max_loops) return 2;
  if (span < 1 || span > max_span) return 3;
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
  return lc_check_graph(n, n_loop, LC4_MAX_LOOPS, LC4_MAX_SPAN, loop_i, loop_c, span, has_loop);
}
inline int lc4_long_check_graph(int n, int n_loop, const int32_t *loop_i, const int32_t *loop_c, int span, uint8_t *has_loop) {
  return lc_check_graph(n, n_loop, LC4_LONG_MAX_LOOPS, LC4_MAX_SPAN, loop_i, loop_c, span, has_loop);
}

// ---- the graph of a solve as the kernels read it: which sequence edges exist (with their measurements, formed from the input poses
// by seq_meas(lo, hi, out[meas_len])), which loop edges are kept, who is in the problem, and per pose the loop edges whose shares its
// rows take. A sequence edge joins two poses of one sequence at most `span` apart unless both are constant; a loop edge between two
// constant poses is dropped; a pose is in the problem when a kept edge touches it and it is not constant.
struct LcGraph {
  std::vector<unsigned char> emask;      // [n] bit k - 1: the sequence edge (i - k, i) exists
  std::vector<unsigned char> free_;      // [n] the pose is in the problem
  std::vector<unsigned char> loop_on;    // [max(n_loop, 1)]
  std::vector<double> meas;              // [n][4][meas_len]
  std::vector<int> lp_begin, lp_entry;   // CSR per pose of 2 l + side (0: the pose is loop_c[l], 1: loop_i[l]), ascending l
};
template <typename SeqMeas>
inline void lc_build_graph(int n, int span, int meas_len, const int32_t *sequence, const uint8_t *fixed, int n_loop, const int32_t *loop_i, const int32_t *loop_c,
                           SeqMeas seq_meas, LcGraph *g) {
  g->emask.assign(n, 0); g->free_.assign(n, 0); g->loop_on.assign(n_loop > 1 ? n_loop : 1, 0);
  g->meas.assign((size_t)4 * meas_len * n, 0.0);
  for (int i = 0; i < n; i++)
    for (int k = 1; k <= span; k++)
      if (i - k >= 0 && sequence[i] == sequence[i - k] && !(fixed[i] && fixed[i - k])) {
        g->emask[i] |= (unsigned char)(1 << (k - 1));
        seq_meas(i - k, i, &g->meas[((size_t)i * 4 + (k - 1)) * meas_len]);
        g->free_[i] = g->free_[i - k] = 1;
      }
  g->lp_begin.assign(n + 1, 0);
  for (int l = 0; l < n_loop; l++) {
    g->loop_on[l] = !(fixed[loop_c[l]] && fixed[loop_i[l]]);
    if (g->loop_on[l]) { g->free_[loop_c[l]] = g->free_[loop_i[l]] = 1; g->lp_begin[loop_c[l] + 1]++; g->lp_begin[loop_i[l] + 1]++; }
  }
  for (int i = 0; i < n; i++) { g->lp_begin[i + 1] += g->lp_begin[i]; if (fixed[i]) g->free_[i] = 0; }
  g->lp_entry.assign(g->lp_begin[n] > 1 ? g->lp_begin[n] : 1, 0);
  std::vector<int> fill(g->lp_begin.begin(), g->lp_begin.end() - 1);
  for (int l = 0; l < n_loop; l++)
    if (g->loop_on[l]) { g->lp_entry[fill[loop_c[l]]++] = 2 * l; g->lp_entry[fill[loop_i[l]]++] = 2 * l + 1; }
}

}  // namespace gfd
