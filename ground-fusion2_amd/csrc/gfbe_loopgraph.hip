// gfbe_loopgraph.hip — the loop-closure pose graphs of dense_map on the device: 4-DoF (gfbe_lc4_eval, gfbe_lc4_solve,
// gfbe_lc4_solve_long; include/gfbe.h) and 6-DoF (gfbe_lc6_eval, gfbe_lc6_solve; include/gfbe_lc6.h). One solver, two models.
//
//   PoseGraph::optimize4DoF             dense_map/src/pose_graph.cpp:529-705 (options :558-566)
//   FourDOFError, FourDOFWeightError    dense_map/src/pose_graph.h:199-288
//   PoseGraph::optimize6DoF             dense_map/src/pose_graph.cpp:707-873 (options :736-745)
//   RelativeRTError                     dense_map/src/pose_graph.h:290-352
//
// A model (Lc4Model, Lc6Model) says what a pose is: D tangent dimensions in PR rows of the padded system (4-DoF: yaw in degrees + t,
// tangent [yaw t], 4 rows; 6-DoF: q (w, x, y, z) + t, tangent [dq(3) t(3)], 8 rows of which 2 are identity rows), its factor and its
// retraction. Sequence edges reach at most four keyframes back, so four consecutive poses form one SB x SB super-block (SB = 4 PR:
// T x T matrix-core tiles, T = 1 or 2) and the sequence part of J^T J is block-tridiagonal in super-blocks; a loop edge adds
// J_l^T J_l, D sparse columns (2 D non-zeros each) of U: H = T + U U^T. One Levenberg-Marquardt step solves
//   T Z = [-g | U]              parallel block cyclic reduction over the M super-blocks, ceil(log2 M) sweeps; the multipliers
//                               alpha = -A B^-1 are applied to the blocks and to the panel by v_mfma_f64_16x16x4_f64, one wave per
//                               16 x 16 tile, a product of inner dimension 32 as two chains (ping-pong in the context's scratch); the
//                               blocks' inverses by Gauss-Jordan on [B | I] in LDS;
//   S = I + U^T Z               gathered through U's 2 D non-zeros per column and factorised as a block LDL^T in 16-wide tiles (the
//                               pivot tile inverted as the super-blocks are, matrix cores for L_IP and the trailing update): by ONE
//                               workgroup through L2 (k_lc4_cap: the 4-DoF graph up to LC4_MAX_LOOPS loop edges), else across
//                               workgroups, one pivot step per launch pair (launch_cap_factor); then y = z_0 - Z S^-1 U^T z_0.
// Every sum runs in a fixed order (owner-computes linearisation, no atomics); the trust-region loop lives in a device struct (LcState,
// gfbe_loopgraph.h): the host enqueues max_num_iterations passes and waits once, every kernel returns at once when `done` is set,
// nothing spins, no kernel waits on another workgroup, there is no device-scope fence. Every entry that is read was written in this
// call: the bits do not depend on what the scratch held. tests/lc4_np.py and tests/lc6_np.py are the models, phase for phase.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gfbe_lc6.h"
#include "gfbe_device.h"
#include "gfbe_loopgraph6.h"

using namespace gfd;

namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));

struct LcDev {
  int n, M, rows, L, ld, ntile, cap_ld;
  const unsigned char *free_;     // [n] the pose is in the problem
  const unsigned char *emask;     // [n] bit k - 1: the sequence edge (i - k, i) exists
  const double *meas;             // [n][4][MEAS] its measurement
  const int *loop_c, *loop_i;     // [L]
  const double *loop_meas;        // [L][MEAS]
  const unsigned char *loop_on;   // [L] (an edge between two constant poses is dropped)
  const int *lp_begin, *lp_entry; // CSR per pose of 2 l + side, ascending l: the loop edges whose shares the pose's rows take
  double delta;
};
struct LcSets {
  double *x[2];                                  // [n][PR] the poses (Model::pack)
  double *Hb[2], *Ha[2], *Hc[2], *g[2];          // [M][SB][SB] diagonal / (m, m - 1) / (m, m + 1) super-blocks, [rows]
  double *Uv[2], *gl[2], *dl[2];                 // per loop edge: corrected J (D x 2 D), its gradient and diagonal shares [2 D]
};

// ---- the two models: the constants, the factor's parameters (passed to the kernels by value), the factor, the retraction; on the
// host the layout of a pose in x, the measurements, the drift, and the two properties of a call that differ
struct Lc4Model {
  enum { D = 4, PR = 4, MEAS = 6, NX = 4 /* ambient coordinates */, SB = 4 * PR, ROT = 3 /* ypr */, ROT_OUT = 1 /* yaw */, LOOP_MEAS = 4 };
  typedef gfbe_lc4_options Options;
  double yaw_div;
  // x: yaw | t
  __device__ __forceinline__ double edge(int kind, const double *x_lo, const double *x_hi, const double *meas, double delta, double *r, double *J) const {
    return lc4_edge(kind, x_lo[0], x_lo + 1, x_hi[0], x_hi + 1, meas, delta, yaw_div, r, J);
  }
  // NormalizeAngle (one wrap) on yaw, t by addition
  static __device__ __forceinline__ void retract(const double *x, const double *d, double *out) {
    out[0] = lc4_normalize_angle(x[0] + d[0]);
    for (int k = 1; k < 4; k++) out[k] = x[k] + d[k];
  }
  static const char *options_name() { return "gfbe_lc4_options"; }
  static bool options_ok(const Options *opt, Options *o) {
    gfbe_lc4_default_options(o);
    if (!opt) return true;
    if (opt->struct_size != (int32_t)sizeof(Options)) return false;
    *o = *opt;
    return o->span >= 1 && o->span <= LC4_MAX_SPAN && o->max_num_iterations >= 0 && o->huber_delta > 0.0 && o->loop_yaw_div > 0.0;
  }
  explicit Lc4Model(const Options &o) : yaw_div(o.loop_yaw_div) {}
  // non-finite input goes through to GFBE_NUMERICAL_FAILURE
  static constexpr bool REFUSE_NON_FINITE = false;
  // up to LC4_MAX_LOOPS loop edges the capacitance system is k_lc4_cap's, beyond it the blocked kernels'
  static bool blocked(int n_loop) { return n_loop > LC4_MAX_LOOPS; }
  static void pack(const double *t, const double *ypr, double *x) { x[0] = ypr[0]; for (int k = 0; k < 3; k++) x[1 + k] = t[k]; }
  static void unpack(const double *x, double *t, double *yaw) { yaw[0] = x[0]; for (int k = 0; k < 3; k++) t[k] = x[1 + k]; }
  static void sequence_meas(const double *ta, const double *ra, const double *tb, const double *rb, double *meas) { lc4_sequence_meas(ta, ra, tb, rb, meas); }
  // the caller's [t(3) relative_yaw] with the pitch and roll of pose loop_c
  static void loop_meas(const double *in, const double *ypr_c, double *meas) {
    for (int q = 0; q < 4; q++) meas[q] = in[q];
    meas[4] = ypr_c[1]; meas[5] = ypr_c[2];
  }
  // pose_graph.cpp:674-681: yaw_drift, t_drift = cur_t - Rz(yaw_drift) vio_t of the last keyframe
  static void drift(const double *v, const double *ypr, const double *u, const double *yaw_out, double *drift) {
    const double yd = yaw_out[0] - ypr[0], a = yd / 180.0 * M_PI;
    drift[0] = yd;
    drift[1] = u[0] - (std::cos(a) * v[0] - std::sin(a) * v[1]);
    drift[2] = u[1] - (std::sin(a) * v[0] + std::cos(a) * v[1]);
    drift[3] = u[2] - v[2];
  }
};
struct Lc6Model {
  enum { D = 6, PR = 8, MEAS = 7, NX = 7, SB = 4 * PR, ROT = 4 /* q */, ROT_OUT = 4, LOOP_MEAS = 7 };
  typedef gfbe_lc6_options Options;
  double t_var, q_var;
  // x: q | t | 0
  __device__ __forceinline__ double edge(int kind, const double *x_lo, const double *x_hi, const double *meas, double delta, double *r, double *J) const {
    return lc6_edge_t<true>(kind, x_lo, x_lo + 4, x_hi, x_hi + 4, meas, delta, t_var, q_var, r, J);
  }
  // q by QuaternionParameterization::Plus (no renormalisation), t by addition
  static __device__ __forceinline__ void retract(const double *x, const double *d, double *out) {
    lc6_plus(x, d, out);
    for (int k = 0; k < 3; k++) out[4 + k] = x[4 + k] + d[3 + k];
  }
  static const char *options_name() { return "gfbe_lc6_options"; }
  static bool options_ok(const Options *opt, Options *o) {
    gfbe_lc6_default_options(o);
    if (!opt) return true;
    if (opt->struct_size != (int32_t)sizeof(Options)) return false;
    *o = *opt;
    return o->span >= 1 && o->span <= LC6_MAX_SPAN && o->max_num_iterations >= 0 && o->huber_delta > 0.0 && o->t_var > 0.0 && o->q_var > 0.0;
  }
  explicit Lc6Model(const Options &o) : t_var(o.t_var), q_var(o.q_var) {}
  // a non-finite pose or loop measurement is refused with GFBE_BAD_INPUT
  static constexpr bool REFUSE_NON_FINITE = true;
  // the capacitance system is always the blocked kernels'
  static bool blocked(int) { return true; }
  static void pack(const double *t, const double *q, double *x) { for (int k = 0; k < 4; k++) x[k] = q[k]; for (int k = 0; k < 3; k++) x[4 + k] = t[k]; x[7] = 0.0; }
  static void unpack(const double *x, double *t, double *q) { for (int k = 0; k < 4; k++) q[k] = x[k]; for (int k = 0; k < 3; k++) t[k] = x[4 + k]; }
  static void sequence_meas(const double *ta, const double *ra, const double *tb, const double *rb, double *meas) { lc6_sequence_meas(ta, ra, tb, rb, meas); }
  static void loop_meas(const double *in, const double *, double *meas) { for (int q = 0; q < 7; q++) meas[q] = in[q]; }
  // pose_graph.cpp:849-850: r_drift = cur_r vio_r^T, t_drift = cur_t - r_drift vio_t of the last keyframe
  static void drift(const double *v, const double *q, const double *u, const double *q_out, double *drift) {
    double ci[4], R[9];
    lc6_qconj(q, ci);
    lc6_qmul(q_out, ci, drift);
    lc6_quat_to_R(drift, R);
    for (int a = 0; a < 3; a++) drift[4 + a] = u[a] - (R[3 * a] * v[0] + R[3 * a + 1] * v[1] + R[3 * a + 2] * v[2]);
  }
};

// p[a] for a < D by value: every index a constant, so that a private array stays in registers. The chain is spelled out per D: built
// by a loop or by recursion over the index the same selection leaves J of k_lc_lin in scratch memory (272 / 592 bytes per lane).
template <int D>
__device__ __forceinline__ double sel(const double *p, int a) {
  static_assert(D == 4 || D == 6, "one chain per tangent dimension");
  if constexpr (D == 4) return a == 0 ? p[0] : (a == 1 ? p[1] : (a == 2 ? p[2] : p[3]));
  else return a == 0 ? p[0] : (a == 1 ? p[1] : (a == 2 ? p[2] : (a == 3 ? p[3] : (a == 4 ? p[4] : p[5]))));
}

// ---- evaluation only (gfbe_lc4_eval, gfbe_lc6_eval): one thread per edge
template <class Mo>
__global__ __launch_bounds__(128) void k_lc_eval(int n_edges, Mo mo, const double *x, const int *ei, const int *ej, const unsigned char *kind, const double *meas, double delta,
                                                 double *r_out, double *J_out, double *cost_e) {
  constexpr int D = Mo::D, JN = 2 * D * D;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  double r[D], J[JN];
  cost_e[e] = mo.edge(kind[e], x + Mo::PR * (size_t)ei[e], x + Mo::PR * (size_t)ej[e], meas + Mo::MEAS * (size_t)e, delta, r, J);
#pragma unroll
  for (int q = 0; q < D; q++) r_out[D * (size_t)e + q] = r[q];
#pragma unroll
  for (int q = 0; q < JN; q++) J_out[JN * (size_t)e + q] = J[q];
}

// ---- fixed-order reduction of one array by a 1024-thread workgroup: thread t takes t, t + 1024, ..., the wave's shares by a shuffle
// tree, the sixteen waves' in wave order. Every thread returns the result. The maximum keeps a NaN (fmax would drop it, and a graph of
// non-finite values would pass for one with a zero gradient).
enum { LCD_THREADS = 1024 };
__device__ __forceinline__ double nanmax(double v, double w) { return (w > v || w != w) ? w : v; }
__device__ double block_reduce(const double *p, int len, bool take_max, double *sh /* [17] */) {
  const int t = threadIdx.x;
  double v = 0.0;
  for (int i = t; i < len; i += LCD_THREADS) v = take_max ? nanmax(v, p[i]) : v + p[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_down(v, o, 64); v = take_max ? nanmax(v, w) : v + w; }
  __syncthreads();
  if ((t & 63) == 0) sh[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int q = 0; q < LCD_THREADS / 64; q++) s = take_max ? nanmax(s, sh[q]) : s + sh[q];
    sh[16] = s;
  }
  __syncthreads();
  return sh[16];
}
__global__ __launch_bounds__(LCD_THREADS) void k_lc_sum(const double *p, int len, double *out) {
  __shared__ double sh[17];
  const double s = block_reduce(p, len, false, sh);
  if (threadIdx.x == 0) *out = s;
}

// ---- linearisation of the sequence edges, owner-computes: lane a < D of pose i (one thread per row of the padded system; the lanes
// D .. PR - 1 of a pose own its identity rows and only clear them) evaluates the pose's up to 2 x 4 sequence edges and writes ITS row
// of the super-blocks and of g — an off-diagonal D-block is one edge's term, the diagonal block and g are summed over the edges
// k = 1 .. 4 backwards, then k = 1 .. 4 forwards. The edge is evaluated by each of the D lanes of a pose (the alternative stages r and J
// per edge through LDS).
// cand = 0: the first linearisation (x into its set); 1: the candidate's cost AND linearisation, into the other set.
template <class Mo>
__global__ __launch_bounds__(256) void k_lc_lin(LcDev P, Mo mo, const LcState *st, LcSets S, int cand, double *cost_i) {
  constexpr int D = Mo::D, PR = Mo::PR, SB = Mo::SB;
  const int f_done = st->done, f_cand = st->cand_on, f_cur = st->cur, f_lb = st->lb;
  if (cand && (f_done || !f_cand)) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows) return;
  const int i = (unsigned)row / PR, a = (unsigned)row % PR, m = (unsigned)row / SB, R = (unsigned)row % SB;      // (unsigned: shifts and masks, and a >= 0 for sel)
  const int xb = cand ? 1 - f_cur : f_cur, sb = cand ? 1 - f_lb : f_lb;
  const double *x = S.x[xb];
  const size_t o = (size_t)m * SB * SB + R * SB;
  double *Hb = S.Hb[sb] + o, *Ha = S.Ha[sb] + o, *Hc = S.Hc[sb] + o;
  for (int c = 0; c < SB; c++) { Hb[c] = 0.0; Ha[c] = 0.0; Hc[c] = 0.0; }
  double dg[D], ga = 0.0, cost = 0.0;
#pragma unroll
  for (int b = 0; b < D; b++) dg[b] = 0.0;
  if (i < P.n && a < D) {
    const bool fi = P.free_[i] != 0;
#pragma unroll
    for (int dir = 0; dir < 2; dir++) {
#pragma unroll
      for (int k = 1; k <= LC4_MAX_SPAN; k++) {
        const int j = dir == 0 ? i - k : i + k;      // the other end
        if (j < 0 || j >= P.n) continue;
        const int hi = dir == 0 ? i : j, lo = dir == 0 ? j : i;      // the edge (lo, hi) is stored with hi
        if (!((P.emask[hi] >> (k - 1)) & 1)) continue;
        double r[D], J[2 * D * D];
        mo.edge(0, x + PR * (size_t)lo, x + PR * (size_t)hi, P.meas + ((size_t)hi * 4 + (k - 1)) * Mo::MEAS, P.delta, r, J);
        if (dir == 1 && a == 0) {      // (the edge's first pose owns its cost)
          double sq = 0.0;
#pragma unroll
          for (int q = 0; q < D; q++) sq += r[q] * r[q];
          cost += 0.5 * sq;
        }
        const bool fj = P.free_[j] != 0;
        // this pose's columns of J are the "j" side (D .. 2 D - 1) of a backward edge, the "i" side of a forward one. Where D = 6 they
        // are chosen by value, every index into J a constant: an offset that depends on dir leaves the dir loop rolled and J in
        // scratch memory (592 bytes per lane). Where D = 4 the sums below read them by that offset inside the product: by value
        // (or through a named temporary) takes 93 -> 120 registers and a wave per SIMD. The same operands in the same order either way.
        const int mine = dir == 0 ? D : 0, other = D - mine;
        double cm[D];
#pragma unroll
        for (int q = 0; q < D; q++) cm[q] = fi ? (dir == 0 ? sel<D>(J + q * 2 * D + D, a) : sel<D>(J + q * 2 * D, a)) : 0.0;
        const int mj = j >> 2;
        double *tgt = (mj == m ? Hb : (mj < m ? Ha : Hc)) + PR * (j & 3);
#pragma unroll
        for (int b = 0; b < D; b++) {
          double so = 0.0, sd = 0.0;
#pragma unroll
          for (int q = 0; q < D; q++) {
            if constexpr (D == 4) {
              so += cm[q] * (fj ? J[q * 2 * D + other + b] : 0.0);
              sd += cm[q] * (fi ? J[q * 2 * D + mine + b] : 0.0);
            } else {
              const double jm = dir == 0 ? J[q * 2 * D + D + b] : J[q * 2 * D + b], jo = dir == 0 ? J[q * 2 * D + b] : J[q * 2 * D + D + b];
              so += cm[q] * (fj ? jo : 0.0);
              sd += cm[q] * (fi ? jm : 0.0);
            }
          }
          tgt[b] = so;
          dg[b] += sd;
        }
        double sv = 0.0;
#pragma unroll
        for (int q = 0; q < D; q++) sv += cm[q] * r[q];
        ga += sv;
      }
    }
#pragma unroll
    for (int b = 0; b < D; b++) Hb[PR * (i & 3) + b] = dg[b];
    if (a == 0) cost_i[i] = cost;
  }
  S.g[sb][row] = ga;
}
// the loop edges: one thread per edge, through the corrector; D columns of U (the rows of the corrected J), the edge's share of g and
// of the diagonal the Jacobi scaling needs, its cost
template <class Mo>
__global__ __launch_bounds__(64) void k_lc_lin_loops(LcDev P, Mo mo, const LcState *st, LcSets S, int cand, double *cost_l) {
  constexpr int D = Mo::D, JN = 2 * D * D;
  const int f_done = st->done, f_cand = st->cand_on, f_cur = st->cur, f_lb = st->lb;
  if (cand && (f_done || !f_cand)) return;
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= P.L) return;
  const int xb = cand ? 1 - f_cur : f_cur, sb = cand ? 1 - f_lb : f_lb;
  const double *x = S.x[xb];
  double r[D], J[JN], cost = 0.0;
  for (int q = 0; q < D; q++) r[q] = 0.0;
  for (int q = 0; q < JN; q++) J[q] = 0.0;
  if (P.loop_on[l]) {
    const int c = P.loop_c[l], i = P.loop_i[l];
    cost = mo.edge(1, x + Mo::PR * (size_t)c, x + Mo::PR * (size_t)i, P.loop_meas + Mo::MEAS * (size_t)l, P.delta, r, J);
    const bool fc = P.free_[c] != 0, fi = P.free_[i] != 0;
    for (int q = 0; q < D; q++)
      for (int b = 0; b < D; b++) { if (!fc) J[q * 2 * D + b] = 0.0; if (!fi) J[q * 2 * D + D + b] = 0.0; }
  }
  cost_l[l] = cost;
  for (int q = 0; q < JN; q++) S.Uv[sb][JN * (size_t)l + q] = J[q];
  for (int k = 0; k < 2 * D; k++) {
    double sg = 0.0, sd = 0.0;
    for (int q = 0; q < D; q++) { sg += J[q * 2 * D + k] * r[q]; sd += J[q * 2 * D + k] * J[q * 2 * D + k]; }
    S.gl[sb][2 * D * (size_t)l + k] = sg;
    S.dl[sb][2 * D * (size_t)l + k] = sd;
  }
}

// ---- the scaled Levenberg-Marquardt system
// per row: the full gradient and diagonal (sequence part + the pose's loop shares in ascending edge order), the Jacobi scale (first pass)
template <class Mo>
__global__ __launch_bounds__(256) void k_lc_scale(LcDev P, const LcState *st, LcSets S, double *scale, double *g0, double *diag0, double *gabs) {
  constexpr int D = Mo::D, PR = Mo::PR, SB = Mo::SB;
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows) return;
  const int lb = st->lb, i = (unsigned)row / PR, a = (unsigned)row % PR, m = (unsigned)row / SB, R = (unsigned)row % SB;
  const bool act = i < P.n && a < D && P.free_[i];
  double d0 = S.Hb[lb][(size_t)m * SB * SB + R * (SB + 1)], gg = S.g[lb][row];
  if (i < P.n && a < D)
    for (int e = P.lp_begin[i]; e < P.lp_begin[i + 1]; e++) {
      const int en = P.lp_entry[e], l = en >> 1, k = D * (en & 1) + a;
      d0 += S.dl[lb][2 * D * (size_t)l + k];
      gg += S.gl[lb][2 * D * (size_t)l + k];
    }
  if (!st->have_scale) scale[row] = act ? 1.0 / (1.0 + sqrt(d0)) : 1.0;
  g0[row] = act ? gg : 0.0;
  gabs[row] = act ? fabs(gg) : 0.0;
  diag0[row] = act ? d0 : 0.0;
}
// per row: S T0 S (unregularised: Bs As Cs, for the model cost) and its copy with the LM diagonal (B A C, what the reduction consumes); a
// row out of the problem (a constant pose, a padding row, a padding pose) is an identity row
template <class Mo>
__global__ __launch_bounds__(256) void k_lc_system(LcDev P, const LcState *st, LcSets S, const double *scale, const double *g0, const double *diag0, double *diag2, double *gs,
                                                   double *Bs, double *As, double *Cs, double *B, double *A, double *C) {
  constexpr int D = Mo::D, PR = Mo::PR, SB = Mo::SB;
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows) return;
  const int lb = st->lb, i = (unsigned)row / PR, a = (unsigned)row % PR, m = (unsigned)row / SB, R = (unsigned)row % SB;
  const bool act = i < P.n && a < D && P.free_[i];
  const double sa = scale[row], radius = st->radius;
  const size_t o = (size_t)m * SB * SB + R * SB;
  for (int c = 0; c < SB; c++) {
    const double vb = S.Hb[lb][o + c] * sa * scale[SB * m + c];
    const double va = m > 0 ? S.Ha[lb][o + c] * sa * scale[SB * (m - 1) + c] : 0.0;
    const double vc = m + 1 < P.M ? S.Hc[lb][o + c] * sa * scale[SB * (m + 1) + c] : 0.0;
    Bs[o + c] = vb; As[o + c] = va; Cs[o + c] = vc;
    B[o + c] = vb; A[o + c] = va; C[o + c] = vc;
  }
  if (!st->reuse) diag2[row] = fmin(fmax(diag0[row] * sa * sa, 1e-6), 1e32);
  B[o + R] = act ? Bs[o + R] + diag2[row] / radius : 1.0;
  gs[row] = sa * g0[row];
}
// the panel [-gs | 0], element by element
__global__ __launch_bounds__(256) void k_lc_panel_fill(int rows, int ld, const LcState *st, const double *gs, double *panel) {
  if (st->done) return;
  const size_t total = (size_t)rows * ld;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t row = e / ld;
    panel[e] = (e - row * ld) == 0 ? -gs[row] : 0.0;
  }
}
// ... and the scaled columns of U scattered into it: one thread per non-zero (l, q, k); k = 0 .. 2 D - 1 are the D rows of pose
// loop_c, then the D of pose loop_i
template <class Mo>
__global__ __launch_bounds__(256) void k_lc_loop_cols(LcDev P, const LcState *st, LcSets S, const double *scale, double *Us, double *panel) {
  constexpr int D = Mo::D, JN = 2 * D * D;
  if (st->done) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= JN * P.L) return;
  const int l = (unsigned)e / JN, rem = e - JN * l, q = (unsigned)rem / (2 * D), k = rem - 2 * D * q;
  const int row = Mo::PR * (k < D ? P.loop_c[l] : P.loop_i[l]) + (k < D ? k : k - D);
  const double v = S.Uv[st->lb][e] * scale[row];
  Us[e] = v;
  panel[(size_t)row * P.ld + 1 + D * l + q] = v;
}

// ---- inverse of an SPD SB x SB block by Gauss-Jordan on [B | I] without pivoting, by the first NT threads of the workgroup (every
// thread of the workgroup calls it: block barriers). W: [SB][2 SB + 1] in LDS (the odd pitch: the lanes of a wave take consecutive
// banks, the multipliers are broadcasts), its left half loaded by the caller. Thread t < NT owns column t % (2 SB) of the rows
// t / (2 SB) + (NT / (2 SB)) j, j < 8. A pivot that is not positive (or not finite) raises *fail; the elimination goes on with 1.
// <16, 64>: one wave (of a workgroup of one or four); <32, 256>: four waves.
template <int SB, int NT>
__device__ void gj_inverse(double *W, int t, int *fail) {
  constexpr int LD = 2 * SB + 1, RS = NT / (2 * SB);
  static_assert(8 * RS == SB, "a thread owns eight rows of its column");
  const int col = t % (2 * SB), r0 = t / (2 * SB);
  if (t < NT) {
#pragma unroll
    for (int j = 0; j < 8; j++) if (col >= SB) W[(r0 + RS * j) * LD + col] = (col - SB == r0 + RS * j) ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int c = 0; c < SB; c++) {
    double rc = 0.0, f[8];
    if (t < NT) {
      double p = W[c * LD + c];
      if (!(p > 0.0) || !isfinite(p)) { if (t == 0) *fail = 1; p = 1.0; }
      rc = W[c * LD + col] / p;
#pragma unroll
      for (int j = 0; j < 8; j++) f[j] = W[(r0 + RS * j) * LD + c];
    }
    __syncthreads();
    if (t < NT) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int r = r0 + RS * j;
        W[r * LD + col] = r == c ? rc : W[r * LD + col] - f[j] * rc;
      }
    }
    __syncthreads();
  }
}
// the symmetrised inverse out of W's right half: entry e = t, t + NT, ... of the SB x SB block, to global memory and / or LDS
template <int SB, int NT>
__device__ __forceinline__ void gj_store(const double *W, int t, double *out, double *lds_out) {
  constexpr int LD = 2 * SB + 1;
  if (t < NT) {
#pragma unroll
    for (int j = 0; j < SB * SB / NT; j++) {
      const int e = t + NT * j, r = e / SB, c = e % SB;
      const double v = (W[r * LD + SB + c] + W[c * LD + SB + r]) / 2;
      if (out) out[e] = v;
      if (lds_out) lds_out[e] = v;
    }
  }
}
// the blocks' first inverses (before any sweep): one workgroup of T x T waves per super-block
template <int T>
__global__ __launch_bounds__(64 * T * T) void k_lc_inv0(int M, const LcState *st, const double *B, double *Binv, int *fail) {
  constexpr int SB = 16 * T, NT = 64 * T * T, LD = 2 * SB + 1;
  __shared__ double W[SB * LD];
  if (st->done) return;
  const int t = threadIdx.x, m = blockIdx.x;
  __builtin_assume(t < NT);      // (the workgroup has NT threads: the guards of gj_inverse and gj_store fold away)
#pragma unroll
  for (int j = 0; j < SB * SB / NT; j++) { const int e = t + NT * j; W[(e / SB) * LD + e % SB] = B[(size_t)m * SB * SB + e]; }
  gj_inverse<SB, NT>(W, t, fail);
  gj_store<SB, NT>(W, t, Binv + (size_t)m * SB * SB, nullptr);
}

// D = acc + X Y for 16 x 16 row-major X (A operand: lane (lr, lk) holds X[lr][4 kk + lk]) and Y (B operand: Y[4 kk + lk][lr]); the
// result's entry q of lane (lr, lk) is D[lk + 4 q][lr].
__device__ __forceinline__ dbl4 mm16(const double *X, int xs, const double *Y, int ys, dbl4 acc, int lr, int lk, double sign) {
  double va[4], vb[4];
#pragma unroll
  for (int kk = 0; kk < 4; kk++) { va[kk] = sign * X[lr * xs + 4 * kk + lk]; vb[kk] = Y[(size_t)(4 * kk + lk) * ys + lr]; }
#pragma unroll
  for (int kk = 0; kk < 4; kk++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va[kk], vb[kk], acc, 0, 0, 0);
  return acc;
}
// One 16 x 16 tile of a product with inner dimension 16 T: Xr = the tile's 16 rows of X (16 T columns), Yc = the tile's 16 columns of
// Y (16 T rows); T chained mm16 over the inner dimension in ascending order (the low half, then the high half).
template <int T>
__device__ __forceinline__ dbl4 mm_tile(const double *Xr, int xs, const double *Yc, int ys, dbl4 acc, int lr, int lk, double sign) {
#pragma unroll
  for (int h = 0; h < T; h++) acc = mm16(Xr + 16 * h, xs, Yc + (size_t)16 * h * ys, ys, acc, lr, lk, sign);
  return acc;
}

// One sweep of parallel block cyclic reduction at stride s over the super-blocks, the blocks' half: one workgroup of T x T waves per
// super-block i, wave w takes the 16 x 16 tile (w / T, w % T) of every product.
//   alpha = -A_i B_{i-s}^-1, gamma = -C_i B_{i+s}^-1 (kept for the panel's half)
//   B' = B + alpha C_{i-s} + gamma A_{i+s};  A' = alpha A_{i-s};  C' = gamma C_{i+s};  B'^-1 travels with the block.
// The multipliers pass through LDS: a single tile with a row of 16 doubles; 2 x 2 tiles with a row of 34, so that the A operand's 32
// lanes of a half-wave (16 rows x 2 columns) take 32 distinct bank pairs (68 lr + 2 lk mod 64), where a row of 32 would put all
// sixteen rows on one.
template <int T>
__global__ __launch_bounds__(64 * T * T) void k_lc_pcr_blocks(int M, int s, const LcState *st, const double *A, const double *B, const double *C, const double *Binv, double *A2,
                                                              double *B2, double *C2, double *Binv2, double *alpha, double *gamma, int *fail) {
  constexpr int SB = 16 * T, NT = 64 * T * T, BB = SB * SB, MUL_LD = T == 1 ? 16 : SB + 2, LD = 2 * SB + 1;
  __shared__ double sAl[SB * MUL_LD], sGa[SB * MUL_LD], W[SB * LD];
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4, ti = wave / T, tj = wave % T;
  __builtin_assume(t < NT);      // (as in k_lc_inv0)
  const int i = blockIdx.x, im = i - s, ip = i + s;
  const bool hm = im >= 0, hp = ip < M;
  const size_t o = (size_t)i * BB;
  const dbl4 zero = {0.0, 0.0, 0.0, 0.0};
  dbl4 al = zero, ga = zero;
  if (hm) al = mm_tile<T>(A + o + 16 * SB * ti, SB, Binv + (size_t)im * BB + 16 * tj, SB, zero, lr, lk, -1.0);
  if (hp) ga = mm_tile<T>(C + o + 16 * SB * ti, SB, Binv + (size_t)ip * BB + 16 * tj, SB, zero, lr, lk, -1.0);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int r = 16 * ti + lk + 4 * q, c = 16 * tj + lr;
    sAl[r * MUL_LD + c] = al[q]; sGa[r * MUL_LD + c] = ga[q];
    alpha[o + r * SB + c] = al[q]; gamma[o + r * SB + c] = ga[q];
  }
  __syncthreads();
  dbl4 Bn, An = zero, Cn = zero;
#pragma unroll
  for (int q = 0; q < 4; q++) Bn[q] = B[o + (16 * ti + lk + 4 * q) * SB + 16 * tj + lr];
  if (hm) {
    Bn = mm_tile<T>(sAl + 16 * ti * MUL_LD, MUL_LD, C + (size_t)im * BB + 16 * tj, SB, Bn, lr, lk, 1.0);
    An = mm_tile<T>(sAl + 16 * ti * MUL_LD, MUL_LD, A + (size_t)im * BB + 16 * tj, SB, zero, lr, lk, 1.0);
  }
  if (hp) {
    Bn = mm_tile<T>(sGa + 16 * ti * MUL_LD, MUL_LD, A + (size_t)ip * BB + 16 * tj, SB, Bn, lr, lk, 1.0);
    Cn = mm_tile<T>(sGa + 16 * ti * MUL_LD, MUL_LD, C + (size_t)ip * BB + 16 * tj, SB, zero, lr, lk, 1.0);
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int r = 16 * ti + lk + 4 * q, c = 16 * tj + lr;
    A2[o + r * SB + c] = An[q]; B2[o + r * SB + c] = Bn[q]; C2[o + r * SB + c] = Cn[q];
    W[r * LD + c] = Bn[q];
  }
  gj_inverse<SB, NT>(W, t, fail);
  gj_store<SB, NT>(W, t, Binv2 + o, nullptr);
}
// ... and the panel's half: wave w of workgroup (i, y) takes the tile (row part w % T, tile column (4 / T) y + w / T) of super-block i:
//   P'_i = P_i + alpha_i P_{i-s} + gamma_i P_{i+s}
template <int T>
__global__ __launch_bounds__(256) void k_lc_pcr_panel(int M, int s, int ld, int ntile, const LcState *st, const double *alpha, const double *gamma, const double *pin, double *pout) {
  constexpr int SB = 16 * T, BB = SB * SB;
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4, i = blockIdx.x, ti = wave % T, tc = blockIdx.y * (4 / T) + wave / T;
  if (tc >= ntile) return;
  const int im = i - s, ip = i + s;
  const size_t own = (size_t)(SB * i + 16 * ti) * ld + 16 * tc;
  dbl4 acc;
#pragma unroll
  for (int q = 0; q < 4; q++) acc[q] = pin[own + (size_t)(lk + 4 * q) * ld + lr];
  if (im >= 0) acc = mm_tile<T>(alpha + (size_t)i * BB + 16 * SB * ti, SB, pin + (size_t)SB * im * ld + 16 * tc, ld, acc, lr, lk, 1.0);
  if (ip < M) acc = mm_tile<T>(gamma + (size_t)i * BB + 16 * SB * ti, SB, pin + (size_t)SB * ip * ld + 16 * tc, ld, acc, lr, lk, 1.0);
#pragma unroll
  for (int q = 0; q < 4; q++) pout[own + (size_t)(lk + 4 * q) * ld + lr] = acc[q];
}
// after the last sweep the super-blocks are decoupled: Z_i = B_i^-1 P_i, tile by tile (the mapping of k_lc_pcr_panel)
template <int T>
__global__ __launch_bounds__(256) void k_lc_final(int ld, int ntile, const LcState *st, const double *Binv, const double *pin, double *Z) {
  constexpr int SB = 16 * T, BB = SB * SB;
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4, i = blockIdx.x, ti = wave % T, tc = blockIdx.y * (4 / T) + wave / T;
  if (tc >= ntile) return;
  const dbl4 zero = {0.0, 0.0, 0.0, 0.0};
  const dbl4 acc = mm_tile<T>(Binv + (size_t)i * BB + 16 * SB * ti, SB, pin + (size_t)SB * i * ld + 16 * tc, ld, zero, lr, lk, 1.0);
  const size_t own = (size_t)(SB * i + 16 * ti) * ld + 16 * tc;
#pragma unroll
  for (int q = 0; q < 4; q++) Z[own + (size_t)(lk + 4 * q) * ld + lr] = acc[q];
}

// ---- the capacitance system of the 4-DoF graph up to LC4_MAX_LOOPS loop edges, ONE workgroup: S = I + U^T Z[:, 1:] gathered through
// U's 8 non-zeros per column (identity padding up to a tile), v = U^T z_0; block LDL^T in 16-wide tiles through global memory (S is up
// to 256 x 256 doubles: 512 KB) — the pivot tile inverted by wave 0 (gj_inverse<16, 64>), L_IP = S_IP D_P^-1 and the trailing update
// S_IJ -= L_IP S_JP^T on the matrix cores, the tiles round-robin over the four waves —, then w = S^-1 v by substitution on LDS.
enum { GJ_LD = 33 };
__global__ __launch_bounds__(256) void k_lc4_cap(LcDev P, const LcState *st, const double *Us, const double *Z, double *Sm, double *Lb, double *Dinv, double *w, int *fail) {
  __shared__ double W[16 * GJ_LD], sD[256], sv[256], sn[256];
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4;
  const int N = P.cap_ld, nt = N / 16, c4 = 4 * P.L, ld = P.ld;
  for (int e = t; e < N * N; e += 256) {
    const int a = e / N, b = e - a * N;
    double v = a == b ? 1.0 : 0.0;
    if (a < c4 && b < c4) {
      const int l = a >> 2;
      for (int k = 0; k < 8; k++) {
        const int row = 4 * (k < 4 ? P.loop_c[l] : P.loop_i[l]) + (k & 3);
        v += Us[8 * (size_t)a + k] * Z[(size_t)row * ld + 1 + b];
      }
    }
    Sm[e] = v;
  }
  {
    double v = 0.0;
    if (t < c4) {
      const int l = t >> 2;
      for (int k = 0; k < 8; k++) {
        const int row = 4 * (k < 4 ? P.loop_c[l] : P.loop_i[l]) + (k & 3);
        v += Us[8 * (size_t)t + k] * Z[(size_t)row * ld];
      }
    }
    sv[t] = v;
  }
  __syncthreads();
  const dbl4 zero = {0.0, 0.0, 0.0, 0.0};
  for (int p = 0; p < nt; p++) {
    if (t < 64) {
#pragma unroll
      for (int j = 0; j < 4; j++) { const int e = t + 64 * j; W[(e >> 4) * GJ_LD + (e & 15)] = Sm[(size_t)(16 * p + (e >> 4)) * N + 16 * p + (e & 15)]; }
    }
    gj_inverse<16, 64>(W, t, fail);
    gj_store<16, 64>(W, t, Dinv + (size_t)p * 256, sD);
    __syncthreads();
    for (int I = p + 1 + wave; I < nt; I += 4) {
      const dbl4 acc = mm16(Sm + (size_t)16 * I * N + 16 * p, N, sD, 16, zero, lr, lk, 1.0);
#pragma unroll
      for (int q = 0; q < 4; q++) Lb[(size_t)(16 * I + lk + 4 * q) * N + 16 * p + lr] = acc[q];
    }
    __syncthreads();
    const int nrem = nt - 1 - p, ntr = nrem * (nrem + 1) / 2;
    for (int e = wave; e < ntr; e += 4) {
      int ii = 0, rr = e;
      while (rr > ii) { rr -= ii + 1; ii++; }
      const int I = p + 1 + ii, J = p + 1 + rr;
      double *Cij = Sm + (size_t)16 * I * N + 16 * J;
      const double *LI = Lb + (size_t)16 * I * N + 16 * p, *SJ = Sm + (size_t)16 * J * N + 16 * p;
      dbl4 acc;
      double va[4], vb[4];
#pragma unroll
      for (int q = 0; q < 4; q++) { acc[q] = Cij[(size_t)(lk + 4 * q) * N + lr]; va[q] = -LI[(size_t)lr * N + 4 * q + lk]; vb[q] = SJ[(size_t)lr * N + 4 * q + lk]; }
#pragma unroll
      for (int kk = 0; kk < 4; kk++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va[kk], vb[kk], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; q++) Cij[(size_t)(lk + 4 * q) * N + lr] = acc[q];
    }
    __syncthreads();
  }
  // w = S^-1 v: forward (unit lower block L), the pivot tiles' inverses, backward
  for (int p = 0; p < nt; p++) {
    if (t < N && t >= 16 * (p + 1)) {
      double s = 0.0;
      for (int k = 0; k < 16; k++) s += Lb[(size_t)t * N + 16 * p + k] * sv[16 * p + k];
      sv[t] -= s;
    }
    __syncthreads();
  }
  {
    double s = 0.0;
    if (t < N) for (int k = 0; k < 16; k++) s += Dinv[(size_t)(t >> 4) * 256 + (t & 15) * 16 + k] * sv[16 * (t >> 4) + k];
    sn[t] = s;
  }
  __syncthreads();
  sv[t] = sn[t];
  __syncthreads();
  for (int p = nt - 1; p >= 0; p--) {
    if (t >= 16 * p && t < 16 * p + 16) {
      double s = 0.0;
      for (int r = 16 * (p + 1); r < N; r++) s += Lb[(size_t)r * N + t] * sv[r];
      sv[t] -= s;
    }
    __syncthreads();
  }
  if (t < N) w[t] = sv[t];
}
// ---- the capacitance system across workgroups (the 4-DoF graph beyond LC4_MAX_LOOPS loop edges, the 6-DoF graph always; N = cap_ld up
// to 2048, 128 tile columns): the algorithm of k_lc4_cap spread over the device and ordered by launch boundaries alone — a gather, per
// pivot step p one launch for the tile column (k_lc4_cap_panel) and one for the trailing update (k_lc4_cap_trail), then the
// substitution (k_lc4_cap_back). Within a launch no workgroup reads what another one writes: the panel launch reads column p of S and
// writes column p of L, the trailing launch reads those two columns and writes the columns behind them. Every tile is written by one
// wave per launch, by one fixed sequence of operations, and every entry of S, L, D^-1 and v that is read was written in this pass.
enum { LC_GATHER_BLOCKS = 2048 };
// S = I + U^T Z[:, 1:] and v = U^T z_0 (entry N N + a), element by element: the 2 D-term sum in the order k = 0 .. 2 D - 1 (the D
// rows of pose loop_c, then the D of pose loop_i; k_lc4_cap's order); padding = identity
template <class Mo>
__global__ __launch_bounds__(256) void k_lc_cap_gather(LcDev P, const LcState *st, const double *Us, const double *Z, double *Sm, double *v) {
  constexpr int D = Mo::D;
  if (st->done) return;
  const size_t N = (size_t)P.cap_ld, NN = N * N, total = NN + N;
  const int cap = D * P.L, ld = P.ld;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const bool vec = e >= NN;
    const int a = vec ? (int)(e - NN) : (int)(e / N), b = vec ? -1 : (int)(e - (size_t)a * N);      // (b = -1: column 0 of Z)
    double s = a == b ? 1.0 : 0.0;
    if (a < cap && b < cap) {
      const int l = a / D, pc = P.loop_c[l], pi = P.loop_i[l];
      for (int k = 0; k < 2 * D; k++) {
        const int row = Mo::PR * (k < D ? pc : pi) + (k < D ? k : k - D);
        s += Us[2 * D * (size_t)a + k] * Z[(size_t)row * ld + 1 + b];
      }
    }
    if (vec) v[a] = s; else Sm[e] = s;
  }
}
// pivot step p, the tile column: every workgroup inverts the pivot tile S_pp for itself (the same instructions on the same values),
// workgroup 0 keeps D_p^-1; wave w of workgroup b takes tile row I = p + 1 + 4 b + w: L_Ip = S_Ip D_p^-1 on the matrix cores, and the
// forward substitution rides along, v_I -= L_Ip v_p (v_p is final since the launch of step p - 1), one lane per row, columns in order
__global__ __launch_bounds__(256) void k_lc4_cap_panel(int N, int p, const LcState *st, const double *Sm, double *Lb, double *Dinv, double *v, int *fail) {
  __shared__ double W[16 * GJ_LD], sD[256], sL[4][16 * 17], svp[16];
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4, nt = N / 16;
  if (t < 64) {
#pragma unroll
    for (int j = 0; j < 4; j++) { const int e = t + 64 * j; W[(e >> 4) * GJ_LD + (e & 15)] = Sm[(size_t)(16 * p + (e >> 4)) * N + 16 * p + (e & 15)]; }
  }
  if (t < 16) svp[t] = v[16 * p + t];
  gj_inverse<16, 64>(W, t, fail);
  gj_store<16, 64>(W, t, blockIdx.x == 0 ? Dinv + (size_t)p * 256 : nullptr, sD);
  __syncthreads();
  const int I = p + 1 + 4 * (int)blockIdx.x + wave;
  if (I < nt) {
    const dbl4 zero = {0.0, 0.0, 0.0, 0.0};
    const dbl4 acc = mm16(Sm + (size_t)16 * I * N + 16 * p, N, sD, 16, zero, lr, lk, 1.0);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      Lb[(size_t)(16 * I + lk + 4 * q) * N + 16 * p + lr] = acc[q];
      sL[wave][(lk + 4 * q) * 17 + lr] = acc[q];
    }
  }
  __syncthreads();
  if (I < nt && lane < 16) {
    double s = 0.0;
    for (int k = 0; k < 16; k++) s += sL[wave][lane * 17 + k] * svp[k];
    v[16 * I + lane] -= s;
  }
}
// ... and the trailing update S_IJ -= L_Ip S_Jp^T of the lower triangle p < J <= I, one wave per tile: workgroup (x, y) takes row
// I = p + 1 + x, its wave w column J = p + 1 + 4 y + w. The operands and the four matrix-core operations of k_lc4_cap.
__global__ __launch_bounds__(256) void k_lc4_cap_trail(int N, int p, const LcState *st, double *Sm, const double *Lb) {
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, lr = lane & 15, lk = lane >> 4;
  const int I = p + 1 + (int)blockIdx.x, J = p + 1 + 4 * (int)blockIdx.y + (t >> 6);
  if (J > I) return;
  double *Cij = Sm + (size_t)16 * I * N + 16 * J;
  const double *LI = Lb + (size_t)16 * I * N + 16 * p, *SJ = Sm + (size_t)16 * J * N + 16 * p;
  dbl4 acc;
  double va[4], vb[4];
#pragma unroll
  for (int q = 0; q < 4; q++) { acc[q] = Cij[(size_t)(lk + 4 * q) * N + lr]; va[q] = -LI[(size_t)lr * N + 4 * q + lk]; vb[q] = SJ[(size_t)lr * N + 4 * q + lk]; }
#pragma unroll
  for (int kk = 0; kk < 4; kk++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va[kk], vb[kk], acc, 0, 0, 0);
#pragma unroll
  for (int q = 0; q < 4; q++) Cij[(size_t)(lk + 4 * q) * N + lr] = acc[q];
}
// w = L^-T D^-1 (L^-1 v): the forward part came with the panels; here the pivot tiles' inverses, one thread per row, and the backward
// substitution with the vector in LDS (N <= 2048: 16 KB), one workgroup of 1024: once tile I of w is final every column c < 16 I takes
// its share, w_c -= sum_k L[16 I + k][c] w[16 I + k] (k in order; a thread owns its columns, the rows of L are read coalesced)
enum { LC4_BACK_THREADS = 1024, LC4_BACK_N = 16 * ((4 * LC4_LONG_MAX_LOOPS + 15) / 16) };
static_assert(16 * ((6 * LC6_MAX_LOOPS + 15) / 16) <= LC4_BACK_N, "the 6-DoF capacitance system fits k_lc4_cap_back");
__global__ __launch_bounds__(LC4_BACK_THREADS) void k_lc4_cap_back(int N, const LcState *st, const double *Lb, const double *Dinv, const double *v, double *w) {
  __shared__ double sv[LC4_BACK_N];
  if (st->done) return;
  const int t = threadIdx.x, nt = N / 16;
  for (int r = t; r < N; r += LC4_BACK_THREADS) sv[r] = v[r];
  __syncthreads();
  double z[LC4_BACK_N / LC4_BACK_THREADS];
#pragma unroll
  for (int j = 0; j < LC4_BACK_N / LC4_BACK_THREADS; j++) {
    const int r = t + LC4_BACK_THREADS * j;
    double s = 0.0;
    if (r < N) for (int k = 0; k < 16; k++) s += Dinv[(size_t)(r >> 4) * 256 + (r & 15) * 16 + k] * sv[16 * (r >> 4) + k];
    z[j] = s;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < LC4_BACK_N / LC4_BACK_THREADS; j++) { const int r = t + LC4_BACK_THREADS * j; if (r < N) sv[r] = z[j]; }
  __syncthreads();
  for (int I = nt - 1; I >= 1; I--) {
    const double *LI = Lb + (size_t)16 * I * N;
    for (int c = t; c < 16 * I; c += LC4_BACK_THREADS) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 16; k++) s += LI[(size_t)k * N + c] * sv[16 * I + k];
      sv[c] -= s;
    }
    __syncthreads();
  }
  for (int r = t; r < N; r += LC4_BACK_THREADS) w[r] = sv[r];
}
// The blocked factorisation of an SPD capacitance system S w = v that lies in device memory (N a multiple of 16, at most LC4_BACK_N;
// S and v as k_lc_cap_gather leaves them, identity padding included): per pivot step one k_lc4_cap_panel and one k_lc4_cap_trail
// launch, then k_lc4_cap_back, 2 N / 16 launches in all
void launch_cap_factor(int N, const LcState *st, double *Sm, double *Lb, double *Dinv, double *v, double *w, int *fail, hipStream_t s) {
  const int cap_nt = N / 16;
  for (int p = 0; p < cap_nt; p++) {
    const int nrem = cap_nt - 1 - p;
    hipLaunchKernelGGL(k_lc4_cap_panel, dim3(std::max(1, (nrem + 3) / 4)), dim3(256), 0, s, N, p, st, Sm, Lb, Dinv, v, fail);
    if (nrem) hipLaunchKernelGGL(k_lc4_cap_trail, dim3(nrem, (nrem + 3) / 4), dim3(256), 0, s, N, p, st, Sm, Lb);
  }
  hipLaunchKernelGGL(k_lc4_cap_back, dim3(1), dim3(LC4_BACK_THREADS), 0, s, N, st, Lb, Dinv, v, w);
}
// y = z_0 - Z[:, 1:] w, one thread per row, the columns in order
__global__ __launch_bounds__(256) void k_lc_apply(int rows, int ld, int cap, const LcState *st, const double *Z, const double *w, double *y) {
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const double *z = Z + (size_t)row * ld;
  double v = z[0];
  for (int b = 0; b < cap; b++) v -= z[1 + b] * w[b];
  y[row] = v;
}

// ---- the candidate: per row the share -(gs y + y (T0s y) / 2) of the model cost change, per loop edge -|Us_l^T y|^2 / 2 (threads
// behind the rows), and lane 0 of every pose retracts: x (+) S y by the model, with its shares of |step|^2 and |candidate|^2 over the
// pose's NX ambient coordinates (free poses only), as Ceres measures them
template <class Mo>
__global__ __launch_bounds__(256) void k_lc_candidate(LcDev P, const LcState *st, LcSets S, const double *Bs, const double *As, const double *Cs, const double *gs, const double *Us,
                                                      const double *y, const double *scale, double *model_r, double *step2_i, double *xn2_i) {
  constexpr int D = Mo::D, PR = Mo::PR, SB = Mo::SB, NX = Mo::NX;
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows + P.L) return;
  if (row >= P.rows) {
    const int l = row - P.rows, pc = P.loop_c[l], pi = P.loop_i[l];
    double s2 = 0.0;
    for (int q = 0; q < D; q++) {
      double p = 0.0;
      for (int k = 0; k < 2 * D; k++) p += Us[2 * D * D * (size_t)l + q * 2 * D + k] * y[PR * (k < D ? pc : pi) + (k < D ? k : k - D)];
      s2 += p * p;
    }
    model_r[row] = -0.5 * s2;
    return;
  }
  const int i = (unsigned)row / PR, m = (unsigned)row / SB, R = (unsigned)row % SB;
  const size_t o = (size_t)m * SB * SB + R * SB;
  double s = 0.0;
  for (int c = 0; c < SB; c++) s += Bs[o + c] * y[SB * m + c];
  if (m > 0) for (int c = 0; c < SB; c++) s += As[o + c] * y[SB * (m - 1) + c];
  if (m + 1 < P.M) for (int c = 0; c < SB; c++) s += Cs[o + c] * y[SB * (m + 1) + c];
  model_r[row] = -(gs[row] * y[row] + 0.5 * (y[row] * s));
  if ((unsigned)row % PR != 0 || i >= P.n) return;
  const double *x = S.x[st->cur] + PR * (size_t)i;
  double *cand = S.x[1 - st->cur] + PR * (size_t)i;
  double out[NX], s2 = 0.0, x2 = 0.0;
  for (int k = 0; k < NX; k++) out[k] = x[k];
  if (P.free_[i]) {
    double d[D];
    for (int k = 0; k < D; k++) d[k] = scale[row + k] * y[row + k];
    Mo::retract(x, d, out);
    for (int k = 0; k < NX; k++) { const double df = out[k] - x[k]; s2 += df * df; x2 += out[k] * out[k]; }
  }
  for (int k = 0; k < NX; k++) cand[k] = out[k];
  for (int k = NX; k < PR; k++) cand[k] = 0.0;
  step2_i[i] = s2; xn2_i[i] = x2;
}

// ---- the reductions of a pass and what follows from them: TrustRegionMinimizer with LevenbergMarquardtStrategy under the options of
// pose_graph.cpp:558-566 and :736-745 (Ceres 1.14 defaults otherwise):
//   mode 0 — the first point's cost; mode 1 — after the solve and the candidate (max |g|, model change, |step|^2, |candidate|^2, the
//   failure flag); mode 2 — after the candidate's evaluation (its cost).
struct LcRed { const double *cost_i, *cost_l, *gabs, *model_r, *step2_i, *xn2_i; };
// the scalar statements, by one thread: r0 .. r3 are the mode's reductions
__device__ void lc_trust_region(LcState &s, int *fail, int mode, double x_norm0, double r0, double r1, double r2, double r3) {
  if (mode == 0) {
    s.cost = r0; s.initial_cost = r0; s.cost_history[0] = r0;
    s.radius = 1e4; s.decrease = 2.0; s.x_norm = x_norm0;
    s.status = GFBE_NO_CONVERGENCE;
    return;
  }
  if (mode == 1) {
    s.have_scale = 1;
    s.cand_on = 0;
    if (s.radius < 1e-32) {
      if (r0 <= 1e-10) { s.termination = 3; s.status = GFBE_OK; } else s.termination = 4;
      s.done = 1;
      return;
    }
    if (r0 <= 1e-10) { s.termination = 3; s.status = GFBE_OK; s.done = 1; return; }
    s.it++;
    const int it = s.it;
    const double model_change = r1;
    const int failed = *fail;      // (raised by any pivot that was not positive, cleared here for the next pass)
    *fail = 0;
    if (failed || !(model_change > 0.0)) {
      s.accepted[it] = 0; s.cost_history[it] = s.cost;
      if (++s.invalid >= 5) { s.termination = 4; s.status = GFBE_NUMERICAL_FAILURE; s.done = 1; return; }
      s.radius /= s.decrease; s.decrease *= 2; s.reuse = 1;
      return;
    }
    s.invalid = 0;
    s.model_change = model_change; s.step2 = r2; s.cand_x2 = r3;
    s.cand_on = 1;
    return;
  }
  const int it = s.it;
  const double cand_cost = r0;
  s.cost_history[it] = s.cost;
  if (sqrt(s.step2) <= 1e-8 * (s.x_norm + 1e-8)) { s.termination = 2; s.status = GFBE_OK; s.done = 1; return; }
  const double change = s.cost - cand_cost;
  if (fabs(change) <= 1e-6 * s.cost) { s.termination = 1; s.status = GFBE_OK; s.done = 1; return; }
  const double rho = change / s.model_change;
  if (rho > 1e-3) {
    s.cur = 1 - s.cur; s.lb = 1 - s.lb;      // (the candidate's pass linearised into the other set)
    s.cost = cand_cost; s.x_norm = sqrt(s.cand_x2);
    s.accepted[it] = 1; s.num_successful++; s.cost_history[it] = cand_cost;
    const double q = 2.0 * rho - 1.0;
    s.radius = fmin(1e16, s.radius / fmax(1.0 / 3.0, 1.0 - q * q * q));
    s.decrease = 2.0; s.reuse = 0;
  } else {
    s.accepted[it] = 0;
    s.radius /= s.decrease; s.decrease *= 2; s.reuse = 1;
  }
}
__global__ __launch_bounds__(LCD_THREADS) void k_lc_decide(int n, int rows, int L, LcRed Q, LcState *st, int *fail, int mode, double x_norm0) {
  __shared__ double sh[17];
  const int f_done = mode != 0 ? st->done : 0, f_cand = st->cand_on;
  if (f_done || (mode == 2 && !f_cand)) return;      // (uniform over the workgroup)
  double r0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  if (mode == 1) {
    r0 = block_reduce(Q.gabs, rows, true, sh);
    r1 = block_reduce(Q.model_r, rows + L, false, sh);
    r2 = block_reduce(Q.step2_i, n, false, sh);
    r3 = block_reduce(Q.xn2_i, n, false, sh);
  } else {
    r0 = block_reduce(Q.cost_i, n, false, sh);
    r0 += block_reduce(Q.cost_l, L, false, sh);
  }
  if (threadIdx.x == 0) lc_trust_region(*st, fail, mode, x_norm0, r0, r1, r2, r3);
}
// the result: x (len = PR n doubles) and the loop's state into the call's pinned memory (the kernel's own stores cross PCIe)
__global__ __launch_bounds__(256) void k_lc_finish(size_t len, const LcState *st, LcSets S, double *x_out, LcState *st_out) {
  const double *x = S.x[st->cur];
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < len; e += (size_t)gridDim.x * 256) x_out[e] = x[e];
  if (blockIdx.x == 0 && threadIdx.x == 0) *st_out = *st;
}

// ---- the host side, once over the model
template <class Mo>
gfbe_status lc_eval_body(const char *name, gfbe_ctx *c, const typename Mo::Options *opt, int32_t n, const double *t, const double *rot, int32_t n_edges, const int32_t *edge_i,
                         const int32_t *edge_j, const uint8_t *kind, const double *meas, double *r_out, double *J_out, double *cost) {
  constexpr int D = Mo::D, JN = 2 * D * D, PR = Mo::PR;
  typename Mo::Options o;
  if (!c) return GFBE_BAD_INPUT;
  const std::string who(name);
  if (!Mo::options_ok(opt, &o)) { ctx_set_error(c, (who + ": " + Mo::options_name() + " of another size or out of range (ABI mismatch)").c_str()); return GFBE_BAD_INPUT; }
  if (n < 1 || n_edges < 0 || !t || !rot || (n_edges && (!edge_i || !edge_j || !kind || !meas))) return GFBE_BAD_INPUT;
  for (int e = 0; e < n_edges; e++)
    if (edge_i[e] < 0 || edge_i[e] >= n || edge_j[e] < 0 || edge_j[e] >= n || edge_i[e] == edge_j[e] || kind[e] > 1) {
      ctx_set_error(c, (who + ": an edge joins two distinct poses in range, kind 0 or 1").c_str());
      return GFBE_BAD_INPUT;
    }
  if (ctx_device(c) < 0) { ctx_set_error(c, (who + ": no device (no CPU fallback)").c_str()); return GFBE_NO_DEVICE; }
  std::vector<double> x0((size_t)PR * n);
  for (int i = 0; i < n; i++) Mo::pack(t + 3 * (size_t)i, rot + Mo::ROT * (size_t)i, &x0[PR * (size_t)i]);
  hipStream_t s = ctx_stream(c);
  CallBuffers buf(c);
  double *dx, *dm, *dr, *dJ, *dc, *hr = nullptr, *hJ = nullptr;
  int *di, *dj;
  unsigned char *dk;
  for (int pass = 0; pass < 2; pass++) {
    dx = buf.dev<double>((size_t)PR * n, x0.data());
    di = buf.dev<int>(n_edges, edge_i); dj = buf.dev<int>(n_edges, edge_j); dk = buf.dev<unsigned char>(n_edges, kind);
    dm = buf.dev<double>((size_t)Mo::MEAS * n_edges, meas);
    dr = buf.dev<double>((size_t)D * n_edges); dJ = buf.dev<double>((size_t)JN * n_edges); dc = buf.dev<double>(n_edges);
    hr = buf.pinned<double>((size_t)D * n_edges); hJ = buf.pinned<double>((size_t)JN * n_edges);
    if (pass == 0 && !buf.commit(0)) { ctx_set_error(c, (who + ": device allocation failed").c_str()); return GFBE_DEVICE_ERROR; }
  }
  double *res = (double *)buf.result();
  if (n_edges) hipLaunchKernelGGL(k_lc_eval<Mo>, dim3((n_edges + 127) / 128), dim3(128), 0, s, n_edges, Mo(o), dx, di, dj, dk, dm, o.huber_delta, dr, dJ, dc);
  hipLaunchKernelGGL(k_lc_sum, dim3(1), dim3(LCD_THREADS), 0, s, dc, n_edges, res);
  if (n_edges && r_out) (void)hipMemcpyAsync(hr, dr, sizeof(double) * D * n_edges, hipMemcpyDeviceToHost, s);
  if (n_edges && J_out) (void)hipMemcpyAsync(hJ, dJ, sizeof(double) * JN * n_edges, hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) { ctx_set_error(c, (who + ": device error").c_str()); return GFBE_DEVICE_ERROR; }
  if (n_edges && r_out) std::memcpy(r_out, hr, sizeof(double) * D * n_edges);
  if (n_edges && J_out) std::memcpy(J_out, hJ, sizeof(double) * JN * n_edges);
  if (cost) *cost = res[0];
  return GFBE_OK;
}

// The body of gfbe_lc4_solve (max_loops = LC4_MAX_LOOPS), gfbe_lc4_solve_long (LC4_LONG_MAX_LOOPS) and gfbe_lc6_solve (LC6_MAX_LOOPS):
// option check, validation, graph, carve, the blind launch loop, finish and summary. rot: ypr [n][3] or q [n][4]; rot_out: yaw [n] or
// q [n][4]; loop_meas [n_loop][Mo::LOOP_MEAS]; drift [Mo::NX].
template <class Mo>
gfbe_status lc_solve_body(const char *name, const char *limit_name, int max_loops, gfbe_ctx *c, const typename Mo::Options *opt, int32_t n, const double *t, const double *rot,
                          const int32_t *sequence, const uint8_t *fixed, int32_t n_loop, const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out,
                          double *rot_out, double *drift, gfbe_summary *S_out) {
  constexpr int D = Mo::D, PR = Mo::PR, SB = Mo::SB, BB = SB * SB, JN = 2 * D * D, MEAS = Mo::MEAS, T = SB / 16;
  typename Mo::Options o;
  if (!c) return GFBE_BAD_INPUT;
  const std::string who(name);
  if (!Mo::options_ok(opt, &o)) { ctx_set_error(c, (who + ": " + Mo::options_name() + " of another size or out of range (ABI mismatch)").c_str()); return GFBE_BAD_INPUT; }
  if (n < 1 || !t || !rot || !sequence || !fixed || !t_out || !rot_out || n_loop < 0 || (n_loop && (!loop_i || !loop_c || !loop_meas))) return GFBE_BAD_INPUT;
  LcPlan plan;
  const bool blocked = Mo::blocked(n_loop);
  std::vector<uint8_t> has_loop(n);
  const int bad = lc_check_graph(n, n_loop, max_loops, LC4_MAX_SPAN, loop_i, loop_c, o.span, has_loop.data());
  if (bad || !lc_plan(n, n_loop, max_loops, D, PR, blocked, &plan)) {
    ctx_set_error(c, (bad == 2 ? who + ": more than " + limit_name + " loop edges" : who + ": loop edges need 0 <= loop_c < loop_i < n, one per loop_i").c_str());
    return GFBE_BAD_INPUT;
  }
  if (Mo::REFUSE_NON_FINITE &&
      (!lc6_all_finite(t, (size_t)3 * n) || !lc6_all_finite(rot, (size_t)Mo::ROT * n) || (n_loop && !lc6_all_finite(loop_meas, (size_t)Mo::LOOP_MEAS * n_loop)))) {
    ctx_set_error(c, (who + ": a pose or a loop measurement is not finite").c_str());
    return GFBE_BAD_INPUT;
  }
  if (ctx_device(c) < 0) { ctx_set_error(c, (who + ": no device (no CPU fallback)").c_str()); return GFBE_NO_DEVICE; }
  const int max_it = std::min(o.max_num_iterations, 15);
  LcGraph G;
  lc_build_graph(n, o.span, MEAS, sequence, fixed, n_loop, loop_i, loop_c,
                 [&](int lo, int hi, double *m) { Mo::sequence_meas(t + 3 * (size_t)lo, rot + Mo::ROT * (size_t)lo, t + 3 * (size_t)hi, rot + Mo::ROT * (size_t)hi, m); }, &G);
  std::vector<double> lmeas((size_t)MEAS * std::max(n_loop, 1), 0.0), x0((size_t)PR * n);
  for (int l = 0; l < n_loop; l++) Mo::loop_meas(loop_meas + Mo::LOOP_MEAS * (size_t)l, rot + Mo::ROT * (size_t)loop_c[l], &lmeas[MEAS * (size_t)l]);
  double xn2 = 0.0;
  for (int i = 0; i < n; i++) {
    Mo::pack(t + 3 * (size_t)i, rot + Mo::ROT * (size_t)i, &x0[PR * (size_t)i]);
    if (G.free_[i]) for (int k = 0; k < Mo::NX; k++) xn2 += x0[PR * (size_t)i + k] * x0[PR * (size_t)i + k];
  }
  const double x_norm0 = std::sqrt(xn2);

  hipStream_t s = ctx_stream(c);
  static_assert(sizeof(LcState) <= CallBuffers::RESULT_BYTES, "the pinned result slot holds the loop's state");
  CallBuffers buf(c);
  LcDev P;
  LcSets S;
  const Mo mo(o);
  const int M = plan.M, rows = plan.rows, L = n_loop;
  double *cost_i, *cost_l, *gabs, *model_r, *step2_i, *xn2_i, *scale, *g0, *diag0, *diag2, *gs, *Bs, *As, *Cs, *Us, *big, *xo;
  LcState *dst;
  int *fail;
  size_t small_bytes = 0;
  for (int pass = 0; pass < 2; pass++) {
    dst = (LcState *)buf.dev<double>((sizeof(LcState) + 7) / 8);      // (cleared: cur = lb = 0, done = 0, ...)
    fail = buf.dev<int>(1);
    small_bytes = buf.used;
    P = {n, M, rows, L, plan.ld, plan.ntile, plan.cap_ld, buf.dev<unsigned char>(n, G.free_.data()), buf.dev<unsigned char>(n, G.emask.data()),
         buf.dev<double>((size_t)4 * MEAS * n, G.meas.data()), buf.dev<int>(L, loop_c), buf.dev<int>(L, loop_i), buf.dev<double>((size_t)MEAS * L, lmeas.data()),
         buf.dev<unsigned char>(L, G.loop_on.data()), buf.dev<int>(n + 1, G.lp_begin.data()), buf.dev<int>(G.lp_entry.size(), G.lp_entry.data()), o.huber_delta};
    S.x[0] = buf.dev<double>((size_t)PR * n, x0.data()); S.x[1] = buf.dev<double>((size_t)PR * n);
    for (int q = 0; q < 2; q++) {
      S.Hb[q] = buf.dev<double>((size_t)BB * M); S.Ha[q] = buf.dev<double>((size_t)BB * M); S.Hc[q] = buf.dev<double>((size_t)BB * M); S.g[q] = buf.dev<double>(rows);
      S.Uv[q] = buf.dev<double>((size_t)JN * L); S.gl[q] = buf.dev<double>((size_t)2 * D * L); S.dl[q] = buf.dev<double>((size_t)2 * D * L);
    }
    cost_i = buf.dev<double>(n); cost_l = buf.dev<double>(L); gabs = buf.dev<double>(rows); model_r = buf.dev<double>((size_t)rows + L);
    step2_i = buf.dev<double>(n); xn2_i = buf.dev<double>(n);
    scale = buf.dev<double>(rows); g0 = buf.dev<double>(rows); diag0 = buf.dev<double>(rows); diag2 = buf.dev<double>(rows); gs = buf.dev<double>(rows);
    Bs = buf.dev<double>((size_t)BB * M); As = buf.dev<double>((size_t)BB * M); Cs = buf.dev<double>((size_t)BB * M); Us = buf.dev<double>((size_t)JN * L);
    big = buf.dev<double>(plan.total);      // the plan's carve: panels, band sets, multipliers, capacitance, step
    xo = buf.pinned<double>((size_t)PR * n);
    if (pass == 0 && !buf.commit(small_bytes)) { ctx_set_error(c, (who + ": device allocation failed").c_str()); return GFBE_DEVICE_ERROR; }
  }
  const LcRed Q = {cost_i, cost_l, gabs, model_r, step2_i, xn2_i};
  double *panel[2] = {big + plan.off_panel[0], big + plan.off_panel[1]};
  double *band[2][4];
  for (int q = 0; q < 2; q++) for (int k = 0; k < 4; k++) band[q][k] = big + plan.off_band[q][k];
  double *alpha = big + plan.off_alpha, *gamma = big + plan.off_gamma, *Sm = big + plan.off_S, *Lb = big + plan.off_L, *Dinv = big + plan.off_Dinv,
         *w = big + plan.off_w, *y = big + plan.off_y, *vcap = big + plan.off_v;      // (vcap: the blocked path only)
  const dim3 gr((rows + 255) / 256), b256(256), bsb(64 * T * T);
  auto lin = [&](int cand) {
    hipLaunchKernelGGL(k_lc_lin<Mo>, gr, b256, 0, s, P, mo, dst, S, cand, cost_i);
    if (L) hipLaunchKernelGGL(k_lc_lin_loops<Mo>, dim3((L + 63) / 64), dim3(64), 0, s, P, mo, dst, S, cand, cost_l);
  };
  auto decide = [&](int mode) { hipLaunchKernelGGL(k_lc_decide, dim3(1), dim3(LCD_THREADS), 0, s, n, rows, L, Q, dst, fail, mode, x_norm0); };
  lin(0);
  decide(0);
  const dim3 gp(M, (plan.ntile + 4 / T - 1) / (4 / T));
  const int fill_blocks = (int)std::min<size_t>(((size_t)rows * plan.ld + 255) / 256, 4096);
  const int gather_blocks = (int)std::min<size_t>(((size_t)plan.cap_ld * (plan.cap_ld + 1) + 255) / 256, LC_GATHER_BLOCKS);
  // max_it passes, enqueued blindly: every kernel of a pass returns at once when the loop has ended
  for (int pass = 0; pass < max_it; pass++) {
    hipLaunchKernelGGL(k_lc_scale<Mo>, gr, b256, 0, s, P, dst, S, scale, g0, diag0, gabs);
    hipLaunchKernelGGL(k_lc_system<Mo>, gr, b256, 0, s, P, dst, S, scale, g0, diag0, diag2, gs, Bs, As, Cs, band[0][1], band[0][0], band[0][2]);
    hipLaunchKernelGGL(k_lc_panel_fill, dim3(fill_blocks), b256, 0, s, rows, plan.ld, dst, gs, panel[0]);
    if (L) hipLaunchKernelGGL(k_lc_loop_cols<Mo>, dim3((JN * L + 255) / 256), b256, 0, s, P, dst, S, scale, Us, panel[0]);
    hipLaunchKernelGGL(k_lc_inv0<T>, dim3(M), bsb, 0, s, M, dst, band[0][1], band[0][3], fail);
    int cur = 0;
    for (int sw = 0, stride = 1; sw < plan.sweeps; sw++, stride *= 2) {
      hipLaunchKernelGGL(k_lc_pcr_blocks<T>, dim3(M), bsb, 0, s, M, stride, dst, band[cur][0], band[cur][1], band[cur][2], band[cur][3], band[1 - cur][0], band[1 - cur][1],
                         band[1 - cur][2], band[1 - cur][3], alpha, gamma, fail);
      hipLaunchKernelGGL(k_lc_pcr_panel<T>, gp, b256, 0, s, M, stride, plan.ld, plan.ntile, dst, alpha, gamma, panel[cur], panel[1 - cur]);
      cur = 1 - cur;
    }
    double *Z = panel[1 - cur];
    hipLaunchKernelGGL(k_lc_final<T>, gp, b256, 0, s, plan.ld, plan.ntile, dst, band[cur][3], panel[cur], Z);
    if (L && !blocked) hipLaunchKernelGGL(k_lc4_cap, dim3(1), b256, 0, s, P, dst, Us, Z, Sm, Lb, Dinv, w, fail);
    if (L && blocked) {      // 1 + 2 cap_ld / 16 launches
      hipLaunchKernelGGL(k_lc_cap_gather<Mo>, dim3(gather_blocks), b256, 0, s, P, dst, Us, Z, Sm, vcap);
      launch_cap_factor(plan.cap_ld, dst, Sm, Lb, Dinv, vcap, w, fail, s);
    }
    hipLaunchKernelGGL(k_lc_apply, gr, b256, 0, s, rows, plan.ld, D * L, dst, Z, w, y);
    hipLaunchKernelGGL(k_lc_candidate<Mo>, dim3((rows + L + 255) / 256), b256, 0, s, P, dst, S, Bs, As, Cs, gs, Us, y, scale, model_r, step2_i, xn2_i);
    decide(1);
    lin(1);      // the candidate's cost — and its linearisation, should it be accepted
    decide(2);
  }
  LcState *hst = (LcState *)buf.result();
  hipLaunchKernelGGL(k_lc_finish, dim3(std::min(256, (PR * n + 255) / 256)), b256, 0, s, (size_t)PR * n, dst, S, xo, hst);
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) { ctx_set_error(c, (who + ": device error").c_str()); return GFBE_DEVICE_ERROR; }
  for (int i = 0; i < n; i++) Mo::unpack(xo + PR * (size_t)i, t_out + 3 * (size_t)i, rot_out + Mo::ROT_OUT * (size_t)i);
  if (drift) Mo::drift(t + 3 * (size_t)(n - 1), rot + Mo::ROT * (size_t)(n - 1), t_out + 3 * (size_t)(n - 1), rot_out + Mo::ROT_OUT * (size_t)(n - 1), drift);
  gfbe_summary sm;
  std::memset(&sm, 0, sizeof sm);
  sm.status = hst->status; sm.termination = hst->done ? hst->termination : 0;
  sm.iterations = hst->it; sm.num_successful = hst->num_successful;
  sm.initial_cost = hst->initial_cost; sm.final_cost = hst->cost; sm.final_radius = hst->radius;
  for (int q = 0; q < 16; q++) { sm.cost_history[q] = hst->cost_history[q]; sm.accepted[q] = (uint8_t)hst->accepted[q]; }
  if (S_out) *S_out = sm;
  return sm.status == GFBE_NUMERICAL_FAILURE ? GFBE_NUMERICAL_FAILURE : GFBE_OK;
}

}  // namespace

extern "C" {

void gfbe_lc4_default_options(gfbe_lc4_options *opt) {
  if (!opt) return;
  std::memset(opt, 0, sizeof *opt);
  opt->struct_size = (int32_t)sizeof(gfbe_lc4_options);
  opt->max_num_iterations = 5;      // pose_graph.cpp:563
  opt->span = 4;                    // :606
  opt->huber_delta = 0.1;           // :566
  opt->loop_yaw_div = 10.0;         // pose_graph.h:271
}

void gfbe_lc6_default_options(gfbe_lc6_options *opt) {
  if (!opt) return;
  std::memset(opt, 0, sizeof *opt);
  opt->struct_size = (int32_t)sizeof(gfbe_lc6_options);
  opt->max_num_iterations = 5;      // pose_graph.cpp:740
  opt->span = 4;                    // :780
  opt->huber_delta = 0.1;           // :743
  opt->t_var = 0.1;                 // :791, :808
  opt->q_var = 0.01;
}

gfbe_status gfbe_lc4_eval(gfbe_ctx *c, const gfbe_lc4_options *opt, int32_t n, const double *t, const double *ypr, int32_t n_edges, const int32_t *edge_i,
                          const int32_t *edge_j, const uint8_t *kind, const double *meas, double *r_out, double *J_out, double *cost) {
  return lc_eval_body<Lc4Model>("gfbe_lc4_eval", c, opt, n, t, ypr, n_edges, edge_i, edge_j, kind, meas, r_out, J_out, cost);
}

gfbe_status gfbe_lc6_eval(gfbe_ctx *c, const gfbe_lc6_options *opt, int32_t n, const double *t, const double *q, int32_t n_edges, const int32_t *edge_i,
                          const int32_t *edge_j, const uint8_t *kind, const double *meas, double *r_out, double *J_out, double *cost) {
  return lc_eval_body<Lc6Model>("gfbe_lc6_eval", c, opt, n, t, q, n_edges, edge_i, edge_j, kind, meas, r_out, J_out, cost);
}

gfbe_status gfbe_lc4_solve(gfbe_ctx *c, const gfbe_lc4_options *opt, int32_t n, const double *t, const double *ypr, const int32_t *sequence, const uint8_t *fixed,
                           int32_t n_loop, const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out, double *yaw_out, double *drift,
                           gfbe_summary *S_out) {
  return lc_solve_body<Lc4Model>("gfbe_lc4_solve", "GFBE_LC4_MAX_LOOPS", LC4_MAX_LOOPS, c, opt, n, t, ypr, sequence, fixed, n_loop, loop_i, loop_c, loop_meas, t_out, yaw_out,
                                 drift, S_out);
}

gfbe_status gfbe_lc4_solve_long(gfbe_ctx *c, const gfbe_lc4_options *opt, int32_t n, const double *t, const double *ypr, const int32_t *sequence, const uint8_t *fixed,
                                int32_t n_loop, const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out, double *yaw_out, double *drift,
                                gfbe_summary *S_out) {
  return lc_solve_body<Lc4Model>("gfbe_lc4_solve_long", "GFBE_LC4_LONG_MAX_LOOPS", LC4_LONG_MAX_LOOPS, c, opt, n, t, ypr, sequence, fixed, n_loop, loop_i, loop_c, loop_meas, t_out,
                                 yaw_out, drift, S_out);
}

gfbe_status gfbe_lc6_solve(gfbe_ctx *c, const gfbe_lc6_options *opt, int32_t n, const double *t, const double *q, const int32_t *sequence, const uint8_t *fixed,
                           int32_t n_loop, const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out, double *q_out, double *drift,
                           gfbe_summary *S_out) {
  return lc_solve_body<Lc6Model>("gfbe_lc6_solve", "GFBE_LC6_MAX_LOOPS", LC6_MAX_LOOPS, c, opt, n, t, q, sequence, fixed, n_loop, loop_i, loop_c, loop_meas, t_out, q_out, drift,
                                 S_out);
}

}  // extern "C"
