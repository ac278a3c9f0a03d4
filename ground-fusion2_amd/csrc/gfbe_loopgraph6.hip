// gfbe_loopgraph6.hip — the 6-DoF loop-closure pose graph of dense_map on the device (gfbe_lc6_eval, gfbe_lc6_solve; include/gfbe_lc6.h).
//
//   PoseGraph::optimize6DoF             dense_map/src/pose_graph.cpp:707-873 (options :736-745)
//   RelativeRTError                     dense_map/src/pose_graph.h:290-352
//
// State: q (w, x, y, z) + t per keyframe, tangent [dq(3) t(3)], padded to 8 rows (2 identity rows), so four consecutive poses form one
// 32 x 32 super-block of 2 x 2 matrix-core tiles and the sequence part of J^T J is block-tridiagonal in super-blocks; a loop edge adds
// J_l^T J_l, six sparse columns (12 non-zeros each) of U: H = T + U U^T. One Levenberg-Marquardt step is gfbe_loopgraph.hip's:
//   T Z = [-g | U]              parallel block cyclic reduction over the M super-blocks, ceil(log2 M) sweeps; a 32 x 32 product is
//                               2 x 2 tiles of two v_mfma_f64_16x16x4_f64 chains each, one wave per tile; the blocks' inverses by
//                               Gauss-Jordan on [B | I] in LDS by the workgroup's four waves;
//   S = I + U^T Z               gathered through U's 12 non-zeros per column, factorised by the blocked LDL^T of gfbe_lc4_solve_long
//                               (launch_lc4_cap_factor: the same kernels, N = 16 ceil(6 L / 16) <= 768), then y = z_0 - Z S^-1 U^T z_0.
// Every sum runs in a fixed order (owner-computes linearisation, no atomics); the trust-region loop (the statements of k_lc4_decide,
// restated) lives in the device struct of gfbe_loopgraph.h: the host enqueues max_num_iterations passes and waits once, every kernel
// returns at once when `done` is set, nothing spins, no kernel waits on another workgroup, there is no device-scope fence. Every entry
// that is read was written in this call: the bits do not depend on what the scratch held. tests/lc6_np.py is the model, phase for phase.
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

struct Lc6Dev {
  int n, M, rows, L, ld, ntile, cap_ld;
  const unsigned char *free_;     // [n] the pose is in the problem
  const unsigned char *emask;     // [n] bit k - 1: the sequence edge (i - k, i) exists
  const double *meas;             // [n][4][7] its measurement
  const int *loop_c, *loop_i;     // [L]
  const double *loop_meas;        // [L][7]
  const unsigned char *loop_on;   // [L] (an edge between two constant poses is dropped)
  const int *lp_begin, *lp_entry; // CSR per pose of 2 l + side, ascending l: the loop edges whose shares the pose's rows take
  double delta, t_var, q_var;
};
typedef Lc4State Lc6State;      // the Levenberg-Marquardt loop's state: gfbe_loopgraph.h (the shared capacitance kernels read its `done`)
struct Lc6Sets {
  double *x[2];                                  // [n][8] q(4) | t(3) | 0
  double *Hb[2], *Ha[2], *Hc[2], *g[2];          // [M][32][32] diagonal / (m, m - 1) / (m, m + 1) super-blocks, [rows]
  double *Uv[2], *gl[2], *dl[2];                 // per loop edge: corrected J (6 x 12), its gradient and diagonal shares [12]
};

__device__ __forceinline__ double sel6(const double *p, int a) { return a == 0 ? p[0] : (a == 1 ? p[1] : (a == 2 ? p[2] : (a == 3 ? p[3] : (a == 4 ? p[4] : p[5])))); }

// ---- evaluation only (gfbe_lc6_eval): one thread per edge
__global__ __launch_bounds__(128) void k_lc6_eval(int n_edges, const double *t, const double *q, const int *ei, const int *ej, const unsigned char *kind, const double *meas,
                                                  double delta, double t_var, double q_var, double *r_out, double *J_out, double *cost_e) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const int i = ei[e], j = ej[e];
  double r[6], J[72];
  cost_e[e] = lc6_edge_t<true>(kind[e], q + 4 * (size_t)i, t + 3 * (size_t)i, q + 4 * (size_t)j, t + 3 * (size_t)j, meas + 7 * (size_t)e, delta, t_var, q_var, r, J);
#pragma unroll
  for (int k = 0; k < 6; k++) r_out[6 * (size_t)e + k] = r[k];
#pragma unroll
  for (int k = 0; k < 72; k++) J_out[72 * (size_t)e + k] = J[k];
}

// ---- fixed-order reduction of one array by a 1024-thread workgroup (the scheme of gfbe_loopgraph.hip, restated: thread t takes t,
// t + 1024, ..., the wave's shares by a shuffle tree, the sixteen waves' in wave order; the maximum keeps a NaN)
enum { LC6_RED_THREADS = 1024 };
__device__ __forceinline__ double nanmax6(double v, double w) { return (w > v || w != w) ? w : v; }
__device__ double block_reduce6(const double *p, int len, bool take_max, double *sh /* [17] */) {
  const int t = threadIdx.x;
  double v = 0.0;
  for (int i = t; i < len; i += LC6_RED_THREADS) v = take_max ? nanmax6(v, p[i]) : v + p[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_down(v, o, 64); v = take_max ? nanmax6(v, w) : v + w; }
  __syncthreads();
  if ((t & 63) == 0) sh[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int q = 0; q < LC6_RED_THREADS / 64; q++) s = take_max ? nanmax6(s, sh[q]) : s + sh[q];
    sh[16] = s;
  }
  __syncthreads();
  return sh[16];
}
__global__ __launch_bounds__(LC6_RED_THREADS) void k_lc6_sum(const double *p, int len, double *out) {
  __shared__ double sh[17];
  const double s = block_reduce6(p, len, false, sh);
  if (threadIdx.x == 0) *out = s;
}

// ---- linearisation of the sequence edges, owner-computes: lane a of pose i (one thread per row of the padded system; the lanes 6 and
// 7 of a pose own its two identity rows and only clear them) evaluates the pose's up to 2 x 4 sequence edges and writes ITS row of the
// super-blocks and of g — an off-diagonal 6-block is one edge's term, the diagonal block and g are summed over the edges k = 1 .. 4
// backwards, then k = 1 .. 4 forwards. The edge is evaluated by each of the six lanes of a pose.
// cand = 0: the first linearisation (x into its set); 1: the candidate's cost AND linearisation, into the other set.
__global__ __launch_bounds__(256) void k_lc6_lin(Lc6Dev P, const Lc6State *st, Lc6Sets S, int cand, double *cost_i) {
  const int f_done = st->done, f_cand = st->cand_on, f_cur = st->cur, f_lb = st->lb;
  if (cand && (f_done || !f_cand)) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows) return;
  const int i = row >> 3, a = row & 7, m = row >> 5, R = row & 31;
  const int xb = cand ? 1 - f_cur : f_cur, sb = cand ? 1 - f_lb : f_lb;
  const double *x = S.x[xb];
  const size_t o = (size_t)m * 1024 + R * 32;
  double *Hb = S.Hb[sb] + o, *Ha = S.Ha[sb] + o, *Hc = S.Hc[sb] + o;
  for (int c = 0; c < 32; c++) { Hb[c] = 0.0; Ha[c] = 0.0; Hc[c] = 0.0; }
  double dg[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ga = 0.0, cost = 0.0;
  if (i < P.n && a < 6) {
    const bool fi = P.free_[i] != 0;
#pragma unroll
    for (int dir = 0; dir < 2; dir++) {
#pragma unroll
      for (int k = 1; k <= LC6_MAX_SPAN; k++) {
        const int j = dir == 0 ? i - k : i + k;      // the other end
        if (j < 0 || j >= P.n) continue;
        const int hi = dir == 0 ? i : j, lo = dir == 0 ? j : i;      // the edge (lo, hi) is stored with hi
        if (!((P.emask[hi] >> (k - 1)) & 1)) continue;
        double r[6], J[72];
        lc6_edge_t<true>(0, x + 8 * (size_t)lo, x + 8 * (size_t)lo + 4, x + 8 * (size_t)hi, x + 8 * (size_t)hi + 4, P.meas + ((size_t)hi * 4 + (k - 1)) * 7, P.delta, P.t_var, P.q_var, r, J);
        if (dir == 1 && a == 0) {      // (the edge's first pose owns its cost)
          double sq = 0.0;
#pragma unroll
          for (int q = 0; q < 6; q++) sq += r[q] * r[q];
          cost += 0.5 * sq;
        }
        const bool fj = P.free_[j] != 0;
        // this pose's columns of J are the "j" side (6 .. 11) of a backward edge, the "i" side of a forward one: chosen by value, every
        // index into J a constant
        double cm[6];
#pragma unroll
        for (int q = 0; q < 6; q++) cm[q] = fi ? (dir == 0 ? sel6(J + q * 12 + 6, a) : sel6(J + q * 12, a)) : 0.0;
        const int mj = j >> 2;
        double *tgt = (mj == m ? Hb : (mj < m ? Ha : Hc)) + 8 * (j & 3);
#pragma unroll
        for (int b = 0; b < 6; b++) {
          double so = 0.0, sd = 0.0;
#pragma unroll
          for (int q = 0; q < 6; q++) {
            const double jm = dir == 0 ? J[q * 12 + 6 + b] : J[q * 12 + b], jo = dir == 0 ? J[q * 12 + b] : J[q * 12 + 6 + b];
            so += cm[q] * (fj ? jo : 0.0);
            sd += cm[q] * (fi ? jm : 0.0);
          }
          tgt[b] = so;
          dg[b] += sd;
        }
        double sv = 0.0;
#pragma unroll
        for (int q = 0; q < 6; q++) sv += cm[q] * r[q];
        ga += sv;
      }
    }
#pragma unroll
    for (int b = 0; b < 6; b++) Hb[8 * (i & 3) + b] = dg[b];
    if (a == 0) cost_i[i] = cost;
  }
  S.g[sb][row] = ga;
}
// the loop edges: one thread per edge, through the corrector; six columns of U (the rows of the corrected J), the edge's share of g and
// of the diagonal the Jacobi scaling needs, its cost
__global__ __launch_bounds__(64) void k_lc6_lin_loops(Lc6Dev P, const Lc6State *st, Lc6Sets S, int cand, double *cost_l) {
  const int f_done = st->done, f_cand = st->cand_on, f_cur = st->cur, f_lb = st->lb;
  if (cand && (f_done || !f_cand)) return;
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= P.L) return;
  const int xb = cand ? 1 - f_cur : f_cur, sb = cand ? 1 - f_lb : f_lb;
  const double *x = S.x[xb];
  double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, J[72], cost = 0.0;
  for (int q = 0; q < 72; q++) J[q] = 0.0;
  if (P.loop_on[l]) {
    const int c = P.loop_c[l], i = P.loop_i[l];
    cost = lc6_edge_t<true>(1, x + 8 * (size_t)c, x + 8 * (size_t)c + 4, x + 8 * (size_t)i, x + 8 * (size_t)i + 4, P.loop_meas + 7 * (size_t)l, P.delta, P.t_var, P.q_var, r, J);
    const bool fc = P.free_[c] != 0, fi = P.free_[i] != 0;
    for (int q = 0; q < 6; q++)
      for (int b = 0; b < 6; b++) { if (!fc) J[q * 12 + b] = 0.0; if (!fi) J[q * 12 + 6 + b] = 0.0; }
  }
  cost_l[l] = cost;
  for (int q = 0; q < 72; q++) S.Uv[sb][72 * (size_t)l + q] = J[q];
  for (int k = 0; k < 12; k++) {
    double sg = 0.0, sd = 0.0;
    for (int q = 0; q < 6; q++) { sg += J[q * 12 + k] * r[q]; sd += J[q * 12 + k] * J[q * 12 + k]; }
    S.gl[sb][12 * (size_t)l + k] = sg;
    S.dl[sb][12 * (size_t)l + k] = sd;
  }
}

// ---- the scaled Levenberg-Marquardt system
// per row: the full gradient and diagonal (sequence part + the pose's loop shares in ascending edge order), the Jacobi scale (first pass)
__global__ __launch_bounds__(256) void k_lc6_scale(Lc6Dev P, const Lc6State *st, Lc6Sets S, double *scale, double *g0, double *diag0, double *gabs) {
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows) return;
  const int lb = st->lb, i = row >> 3, a = row & 7, m = row >> 5, R = row & 31;
  const bool act = i < P.n && a < 6 && P.free_[i];
  double d0 = S.Hb[lb][(size_t)m * 1024 + R * 33], gg = S.g[lb][row];
  if (i < P.n && a < 6)
    for (int e = P.lp_begin[i]; e < P.lp_begin[i + 1]; e++) {
      const int en = P.lp_entry[e], l = en >> 1, k = 6 * (en & 1) + a;
      d0 += S.dl[lb][12 * (size_t)l + k];
      gg += S.gl[lb][12 * (size_t)l + k];
    }
  if (!st->have_scale) scale[row] = act ? 1.0 / (1.0 + sqrt(d0)) : 1.0;
  g0[row] = act ? gg : 0.0;
  gabs[row] = act ? fabs(gg) : 0.0;
  diag0[row] = act ? d0 : 0.0;
}
// per row: S T0 S (unregularised: Bs As Cs, for the model cost) and its copy with the LM diagonal (B A C, what the reduction consumes); a
// row out of the problem (a constant pose, a padding row, a padding pose) is an identity row
__global__ __launch_bounds__(256) void k_lc6_system(Lc6Dev P, const Lc6State *st, Lc6Sets S, const double *scale, const double *g0, const double *diag0, double *diag2, double *gs,
                                                    double *Bs, double *As, double *Cs, double *B, double *A, double *C) {
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows) return;
  const int lb = st->lb, i = row >> 3, a = row & 7, m = row >> 5, R = row & 31;
  const bool act = i < P.n && a < 6 && P.free_[i];
  const double sa = scale[row], radius = st->radius;
  const size_t o = (size_t)m * 1024 + R * 32;
  for (int c = 0; c < 32; c++) {
    const double vb = S.Hb[lb][o + c] * sa * scale[32 * m + c];
    const double va = m > 0 ? S.Ha[lb][o + c] * sa * scale[32 * (m - 1) + c] : 0.0;
    const double vc = m + 1 < P.M ? S.Hc[lb][o + c] * sa * scale[32 * (m + 1) + c] : 0.0;
    Bs[o + c] = vb; As[o + c] = va; Cs[o + c] = vc;
    B[o + c] = vb; A[o + c] = va; C[o + c] = vc;
  }
  if (!st->reuse) diag2[row] = fmin(fmax(diag0[row] * sa * sa, 1e-6), 1e32);
  B[o + R] = act ? Bs[o + R] + diag2[row] / radius : 1.0;
  gs[row] = sa * g0[row];
}
// the panel [-gs | 0], element by element
__global__ __launch_bounds__(256) void k_lc6_panel_fill(int rows, int ld, const Lc6State *st, const double *gs, double *panel) {
  if (st->done) return;
  const size_t total = (size_t)rows * ld;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t row = e / ld;
    panel[e] = (e - row * ld) == 0 ? -gs[row] : 0.0;
  }
}
// ... and the scaled columns of U scattered into it: one thread per non-zero (l, q, k)
__global__ __launch_bounds__(256) void k_lc6_loop_cols(Lc6Dev P, const Lc6State *st, Lc6Sets S, const double *scale, double *Us, double *panel) {
  if (st->done) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 72 * P.L) return;
  const int l = e / 72, rem = e - 72 * l, q = rem / 12, k = rem - 12 * q;
  const int row = 8 * (k < 6 ? P.loop_c[l] : P.loop_i[l]) + (k < 6 ? k : k - 6);
  const double v = S.Uv[st->lb][e] * scale[row];
  Us[e] = v;
  panel[(size_t)row * P.ld + 1 + 6 * l + q] = v;
}

// ---- inverse of an SPD 32 x 32 super-block by Gauss-Jordan on [B | I] without pivoting, by the 256 threads of the workgroup. W:
// [32][65] in LDS (a row of 65 doubles: the 64 lanes of a wave take consecutive banks, the multipliers are broadcasts), its left half
// loaded by the caller. Thread t owns column t & 63 of the rows (t >> 6) + 4 j. A pivot that is not positive (or not finite) raises
// *fail; the elimination goes on with 1 — the test and the recovery of gj_inverse16 (gfbe_loopgraph.hip).
enum { GJ32_LD = 65 };
__device__ void gj_inverse32(double *W, int t, int *fail) {
  const int col = t & 63, r0 = t >> 6;
#pragma unroll
  for (int j = 0; j < 8; j++) if (col >= 32) W[(r0 + 4 * j) * GJ32_LD + col] = (col - 32 == r0 + 4 * j) ? 1.0 : 0.0;
  __syncthreads();
  for (int c = 0; c < 32; c++) {
    double f[8];
    double p = W[c * GJ32_LD + c];
    if (!(p > 0.0) || !isfinite(p)) { if (t == 0) *fail = 1; p = 1.0; }
    const double rc = W[c * GJ32_LD + col] / p;
#pragma unroll
    for (int j = 0; j < 8; j++) f[j] = W[(r0 + 4 * j) * GJ32_LD + c];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int r = r0 + 4 * j;
      W[r * GJ32_LD + col] = r == c ? rc : W[r * GJ32_LD + col] - f[j] * rc;
    }
    __syncthreads();
  }
}
// the symmetrised inverse out of W's right half: entry e = t, t + 256, ... of the 32 x 32 block
__device__ __forceinline__ void gj_store32(const double *W, int t, double *out) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int e = t + 256 * j, r = e >> 5, c = e & 31;
    out[e] = (W[r * GJ32_LD + 32 + c] + W[c * GJ32_LD + 32 + r]) / 2;
  }
}
// the blocks' first inverses (before any sweep): one workgroup per super-block
__global__ __launch_bounds__(256) void k_lc6_inv0(int M, const Lc6State *st, const double *B, double *Binv, int *fail) {
  __shared__ double W[32 * GJ32_LD];
  if (st->done) return;
  const int t = threadIdx.x, m = blockIdx.x;
#pragma unroll
  for (int j = 0; j < 4; j++) { const int e = t + 256 * j; W[(e >> 5) * GJ32_LD + (e & 31)] = B[(size_t)m * 1024 + e]; }
  gj_inverse32(W, t, fail);
  gj_store32(W, t, Binv + (size_t)m * 1024);
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
// One 16 x 16 tile of a product with inner dimension 32: Xr = the tile's 16 rows of X (32 columns), Yc = the tile's 16 columns of Y
// (32 rows); the two halves of the inner dimension in order.
__device__ __forceinline__ dbl4 mm32_tile(const double *Xr, int xs, const double *Yc, int ys, dbl4 acc, int lr, int lk, double sign) {
  acc = mm16(Xr, xs, Yc, ys, acc, lr, lk, sign);
  return mm16(Xr + 16, xs, Yc + (size_t)16 * ys, ys, acc, lr, lk, sign);
}

// One sweep of parallel block cyclic reduction at stride s over the super-blocks, the blocks' half: one workgroup per super-block i,
// wave w takes the 16 x 16 tile (w >> 1, w & 1) of every 32 x 32 product.
//   alpha = -A_i B_{i-s}^-1, gamma = -C_i B_{i+s}^-1 (kept for the panel's half)
//   B' = B + alpha C_{i-s} + gamma A_{i+s};  A' = alpha A_{i-s};  C' = gamma C_{i+s};  B'^-1 travels with the block.
// The multipliers pass through LDS with a row of 34 doubles: the A operand's 32 lanes of a half-wave (16 rows x 2 columns) then take
// 32 distinct bank pairs (68 lr + 2 lk mod 64), where a row of 32 would put all sixteen rows on one.
enum { MUL_LD = 34 };
__global__ __launch_bounds__(256) void k_lc6_pcr_blocks(int M, int s, const Lc6State *st, const double *A, const double *B, const double *C, const double *Binv,
                                                        double *A2, double *B2, double *C2, double *Binv2, double *alpha, double *gamma, int *fail) {
  __shared__ double sAl[32 * MUL_LD], sGa[32 * MUL_LD], W[32 * GJ32_LD];
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4, ti = wave >> 1, tj = wave & 1;
  const int i = blockIdx.x, im = i - s, ip = i + s;
  const bool hm = im >= 0, hp = ip < M;
  const size_t o = (size_t)i * 1024;
  const dbl4 zero = {0.0, 0.0, 0.0, 0.0};
  dbl4 al = zero, ga = zero;
  if (hm) al = mm32_tile(A + o + 512 * ti, 32, Binv + (size_t)im * 1024 + 16 * tj, 32, zero, lr, lk, -1.0);
  if (hp) ga = mm32_tile(C + o + 512 * ti, 32, Binv + (size_t)ip * 1024 + 16 * tj, 32, zero, lr, lk, -1.0);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int r = 16 * ti + lk + 4 * q, c = 16 * tj + lr;
    sAl[r * MUL_LD + c] = al[q]; sGa[r * MUL_LD + c] = ga[q];
    alpha[o + r * 32 + c] = al[q]; gamma[o + r * 32 + c] = ga[q];
  }
  __syncthreads();
  dbl4 Bn, An = zero, Cn = zero;
#pragma unroll
  for (int q = 0; q < 4; q++) Bn[q] = B[o + (16 * ti + lk + 4 * q) * 32 + 16 * tj + lr];
  if (hm) {
    Bn = mm32_tile(sAl + 16 * ti * MUL_LD, MUL_LD, C + (size_t)im * 1024 + 16 * tj, 32, Bn, lr, lk, 1.0);
    An = mm32_tile(sAl + 16 * ti * MUL_LD, MUL_LD, A + (size_t)im * 1024 + 16 * tj, 32, zero, lr, lk, 1.0);
  }
  if (hp) {
    Bn = mm32_tile(sGa + 16 * ti * MUL_LD, MUL_LD, A + (size_t)ip * 1024 + 16 * tj, 32, Bn, lr, lk, 1.0);
    Cn = mm32_tile(sGa + 16 * ti * MUL_LD, MUL_LD, C + (size_t)ip * 1024 + 16 * tj, 32, zero, lr, lk, 1.0);
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int r = 16 * ti + lk + 4 * q, c = 16 * tj + lr;
    A2[o + r * 32 + c] = An[q]; B2[o + r * 32 + c] = Bn[q]; C2[o + r * 32 + c] = Cn[q];
    W[r * GJ32_LD + c] = Bn[q];
  }
  gj_inverse32(W, t, fail);
  gj_store32(W, t, Binv2 + o);
}
// ... and the panel's half: wave w of workgroup (i, y) takes the tile (row half w & 1, tile column 2 y + (w >> 1)) of super-block i:
//   P'_i = P_i + alpha_i P_{i-s} + gamma_i P_{i+s}
__global__ __launch_bounds__(256) void k_lc6_pcr_panel(int M, int s, int ld, int ntile, const Lc6State *st, const double *alpha, const double *gamma, const double *pin, double *pout) {
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4, i = blockIdx.x, ti = wave & 1, tc = blockIdx.y * 2 + (wave >> 1);
  if (tc >= ntile) return;
  const int im = i - s, ip = i + s;
  const size_t own = (size_t)(32 * i + 16 * ti) * ld + 16 * tc;
  dbl4 acc;
#pragma unroll
  for (int q = 0; q < 4; q++) acc[q] = pin[own + (size_t)(lk + 4 * q) * ld + lr];
  if (im >= 0) acc = mm32_tile(alpha + (size_t)i * 1024 + 512 * ti, 32, pin + (size_t)32 * im * ld + 16 * tc, ld, acc, lr, lk, 1.0);
  if (ip < M) acc = mm32_tile(gamma + (size_t)i * 1024 + 512 * ti, 32, pin + (size_t)32 * ip * ld + 16 * tc, ld, acc, lr, lk, 1.0);
#pragma unroll
  for (int q = 0; q < 4; q++) pout[own + (size_t)(lk + 4 * q) * ld + lr] = acc[q];
}
// after the last sweep the super-blocks are decoupled: Z_i = B_i^-1 P_i, tile by tile
__global__ __launch_bounds__(256) void k_lc6_final(int ld, int ntile, const Lc6State *st, const double *Binv, const double *pin, double *Z) {
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4, i = blockIdx.x, ti = wave & 1, tc = blockIdx.y * 2 + (wave >> 1);
  if (tc >= ntile) return;
  const dbl4 zero = {0.0, 0.0, 0.0, 0.0};
  const dbl4 acc = mm32_tile(Binv + (size_t)i * 1024 + 512 * ti, 32, pin + (size_t)32 * i * ld + 16 * tc, ld, zero, lr, lk, 1.0);
  const size_t own = (size_t)(32 * i + 16 * ti) * ld + 16 * tc;
#pragma unroll
  for (int q = 0; q < 4; q++) Z[own + (size_t)(lk + 4 * q) * ld + lr] = acc[q];
}

// ---- the capacitance system: S = I + U^T Z[:, 1:] and v = U^T z_0 (entry N N + a), element by element, gathered through U's 12
// non-zeros per column in the order k = 0 .. 11 (the six rows of pose loop_c, then the six of pose loop_i); padding = identity. The
// factorisation and the substitution are launch_lc4_cap_factor's.
enum { LC6_GATHER_BLOCKS = 2048 };
__global__ __launch_bounds__(256) void k_lc6_cap_gather(Lc6Dev P, const Lc6State *st, const double *Us, const double *Z, double *Sm, double *v) {
  if (st->done) return;
  const size_t N = (size_t)P.cap_ld, NN = N * N, total = NN + N;
  const int c6 = 6 * P.L, ld = P.ld;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const bool vec = e >= NN;
    const int a = vec ? (int)(e - NN) : (int)(e / N), b = vec ? -1 : (int)(e - (size_t)a * N);      // (b = -1: column 0 of Z)
    double s = a == b ? 1.0 : 0.0;
    if (a < c6 && b < c6) {
      const int l = a / 6, pc = P.loop_c[l], pi = P.loop_i[l];
      for (int k = 0; k < 12; k++) {
        const int row = 8 * (k < 6 ? pc : pi) + (k < 6 ? k : k - 6);
        s += Us[12 * (size_t)a + k] * Z[(size_t)row * ld + 1 + b];
      }
    }
    if (vec) v[a] = s; else Sm[e] = s;
  }
}
// y = z_0 - Z[:, 1:] w, one thread per row, the columns in order
__global__ __launch_bounds__(256) void k_lc6_apply(int rows, int ld, int c6, const Lc6State *st, const double *Z, const double *w, double *y) {
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const double *z = Z + (size_t)row * ld;
  double v = z[0];
  for (int b = 0; b < c6; b++) v -= z[1 + b] * w[b];
  y[row] = v;
}

// ---- the candidate: per row the share -(gs y + y (T0s y) / 2) of the model cost change, per loop edge -|Us_l^T y|^2 / 2 (threads
// behind the rows), and lane 0 of every pose retracts: q by QuaternionParameterization::Plus, t by addition, with its shares of
// |step|^2 and |candidate|^2 over the pose's seven ambient coordinates (free poses only), as Ceres measures them
__global__ __launch_bounds__(256) void k_lc6_candidate(Lc6Dev P, const Lc6State *st, Lc6Sets S, const double *Bs, const double *As, const double *Cs, const double *gs, const double *Us,
                                                       const double *y, const double *scale, double *model_r, double *step2_i, double *xn2_i) {
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows + P.L) return;
  if (row >= P.rows) {
    const int l = row - P.rows, pc = P.loop_c[l], pi = P.loop_i[l];
    double s2 = 0.0;
    for (int q = 0; q < 6; q++) {
      double p = 0.0;
      for (int k = 0; k < 12; k++) p += Us[72 * (size_t)l + q * 12 + k] * y[8 * (k < 6 ? pc : pi) + (k < 6 ? k : k - 6)];
      s2 += p * p;
    }
    model_r[row] = -0.5 * s2;
    return;
  }
  const int i = row >> 3, m = row >> 5, R = row & 31;
  const size_t o = (size_t)m * 1024 + R * 32;
  double s = 0.0;
  for (int c = 0; c < 32; c++) s += Bs[o + c] * y[32 * m + c];
  if (m > 0) for (int c = 0; c < 32; c++) s += As[o + c] * y[32 * (m - 1) + c];
  if (m + 1 < P.M) for (int c = 0; c < 32; c++) s += Cs[o + c] * y[32 * (m + 1) + c];
  model_r[row] = -(gs[row] * y[row] + 0.5 * (y[row] * s));
  if ((row & 7) != 0 || i >= P.n) return;
  const double *x = S.x[st->cur] + 8 * (size_t)i;
  double *cand = S.x[1 - st->cur] + 8 * (size_t)i;
  double out[7] = {x[0], x[1], x[2], x[3], x[4], x[5], x[6]}, s2 = 0.0, x2 = 0.0;
  if (P.free_[i]) {
    double d[6];
    for (int k = 0; k < 6; k++) d[k] = scale[row + k] * y[row + k];
    lc6_plus(x, d, out);
    for (int k = 0; k < 3; k++) out[4 + k] = x[4 + k] + d[3 + k];
    for (int k = 0; k < 7; k++) { const double df = out[k] - x[k]; s2 += df * df; x2 += out[k] * out[k]; }
  }
  for (int k = 0; k < 7; k++) cand[k] = out[k];
  cand[7] = 0.0;
  step2_i[i] = s2; xn2_i[i] = x2;
}

// ---- the reductions of a pass and what follows from them: TrustRegionMinimizer with LevenbergMarquardtStrategy under the options of
// pose_graph.cpp:736-745 (Ceres 1.14 defaults otherwise), the statements and their order as in k_lc4_decide:
//   mode 0 — the first point's cost; mode 1 — after the solve and the candidate (max |g|, model change, |step|^2, |candidate|^2, the
//   failure flag); mode 2 — after the candidate's evaluation (its cost).
struct Lc6Red { const double *cost_i, *cost_l, *gabs, *model_r, *step2_i, *xn2_i; };
__global__ __launch_bounds__(LC6_RED_THREADS) void k_lc6_decide(int n, int rows, int L, Lc6Red Q, Lc6State *st, int *fail, int mode, double x_norm0) {
  __shared__ double sh[17];
  const int f_done = mode != 0 ? st->done : 0, f_cand = st->cand_on;
  if (f_done || (mode == 2 && !f_cand)) return;      // (uniform over the workgroup)
  double r0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  if (mode == 1) {
    r0 = block_reduce6(Q.gabs, rows, true, sh);
    r1 = block_reduce6(Q.model_r, rows + L, false, sh);
    r2 = block_reduce6(Q.step2_i, n, false, sh);
    r3 = block_reduce6(Q.xn2_i, n, false, sh);
  } else {
    r0 = block_reduce6(Q.cost_i, n, false, sh);
    r0 += block_reduce6(Q.cost_l, L, false, sh);
  }
  if (threadIdx.x != 0) return;
  Lc6State &s = *st;
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
// the result: x and the loop's state into the call's pinned memory (the kernel's own stores cross PCIe)
__global__ __launch_bounds__(256) void k_lc6_finish(int n, const Lc6State *st, Lc6Sets S, double *x_out, Lc6State *st_out) {
  const double *x = S.x[st->cur];
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)8 * n; e += (size_t)gridDim.x * 256) x_out[e] = x[e];
  if (blockIdx.x == 0 && threadIdx.x == 0) *st_out = *st;
}

// ---- one slab out of the context's grow-only scratch, carved by a dry run; host arrays travel through the pinned scratch
// (the scheme of gfbe_loopgraph.hip's Lc4Buffers, restated here: that one is file-local)
enum { LC6_RESULT_BYTES = 1024 };
struct Lc6Buffers {
  gfbe_ctx *c;
  char *slab = nullptr, *pin = nullptr;
  size_t cap = 0, used = 0, pin_cap = 0, pin_used = 0;
  bool dry = true;
  explicit Lc6Buffers(gfbe_ctx *ctx) : c(ctx) {}
  ~Lc6Buffers() { (void)hipStreamSynchronize(ctx_stream(c)); }
  bool commit(size_t clear_bytes) {      // clear_bytes: the head of the slab that is cleared (the loop's state and the failure flag)
    cap = used; used = 0; dry = false;
    pin_cap = pin_used; pin_used = 0;
    slab = (char *)ctx_scratch(c, std::max<size_t>(cap, 256));
    pin = (char *)ctx_scratch_pinned(c, pin_cap + LC6_RESULT_BYTES);
    if (!slab || !pin) return false;
    return hipMemsetAsync(slab, 0, std::max<size_t>(std::min(clear_bytes, cap), 256), ctx_stream(c)) == hipSuccess;
  }
  void *result() const { return pin + pin_cap; }
  template <typename T>
  T *pinned(size_t n) {
    const size_t bytes = (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255, at = pin_used;
    pin_used += bytes;
    return dry ? nullptr : (T *)(pin + at);
  }
  template <typename T>
  T *dev(size_t n, const T *h = nullptr) {
    const size_t bytes = (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255, at = used, pat = pin_used;
    used += bytes;
    if (h && n) pin_used += bytes;
    if (dry) return nullptr;
    T *q = (T *)(slab + at);
    if (h && n) {
      std::memcpy(pin + pat, h, n * sizeof(T));
      (void)hipMemcpyAsync(q, pin + pat, n * sizeof(T), hipMemcpyHostToDevice, ctx_stream(c));
    }
    return q;
  }
};

bool options_ok(const gfbe_lc6_options *opt, gfbe_lc6_options *o) {
  gfbe_lc6_default_options(o);
  if (!opt) return true;
  if (opt->struct_size != (int32_t)sizeof(gfbe_lc6_options)) return false;
  *o = *opt;
  return o->span >= 1 && o->span <= LC6_MAX_SPAN && o->max_num_iterations >= 0 && o->huber_delta > 0.0 && o->t_var > 0.0 && o->q_var > 0.0;
}

}  // namespace

extern "C" {

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

gfbe_status gfbe_lc6_eval(gfbe_ctx *c, const gfbe_lc6_options *opt, int32_t n, const double *t, const double *q, int32_t n_edges, const int32_t *edge_i,
                          const int32_t *edge_j, const uint8_t *kind, const double *meas, double *r_out, double *J_out, double *cost) {
  gfbe_lc6_options o;
  if (!c) return GFBE_BAD_INPUT;
  if (!options_ok(opt, &o)) { ctx_set_error(c, "gfbe_lc6_eval: gfbe_lc6_options of another size or out of range (ABI mismatch)"); return GFBE_BAD_INPUT; }
  if (n < 1 || n_edges < 0 || !t || !q || (n_edges && (!edge_i || !edge_j || !kind || !meas))) return GFBE_BAD_INPUT;
  for (int e = 0; e < n_edges; e++)
    if (edge_i[e] < 0 || edge_i[e] >= n || edge_j[e] < 0 || edge_j[e] >= n || edge_i[e] == edge_j[e] || kind[e] > 1) {
      ctx_set_error(c, "gfbe_lc6_eval: an edge joins two distinct poses in range, kind 0 or 1");
      return GFBE_BAD_INPUT;
    }
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_lc6_eval: no device (no CPU fallback)"); return GFBE_NO_DEVICE; }
  hipStream_t s = ctx_stream(c);
  Lc6Buffers buf(c);
  double *dt, *dq, *dm, *dr, *dJ, *dc, *hr = nullptr, *hJ = nullptr;
  int *di, *dj;
  unsigned char *dk;
  for (int pass = 0; pass < 2; pass++) {
    dt = buf.dev<double>((size_t)3 * n, t); dq = buf.dev<double>((size_t)4 * n, q);
    di = buf.dev<int>(n_edges, edge_i); dj = buf.dev<int>(n_edges, edge_j); dk = buf.dev<unsigned char>(n_edges, kind);
    dm = buf.dev<double>((size_t)7 * n_edges, meas);
    dr = buf.dev<double>((size_t)6 * n_edges); dJ = buf.dev<double>((size_t)72 * n_edges); dc = buf.dev<double>(n_edges);
    hr = buf.pinned<double>((size_t)6 * n_edges); hJ = buf.pinned<double>((size_t)72 * n_edges);
    if (pass == 0 && !buf.commit(0)) { ctx_set_error(c, "gfbe_lc6_eval: device allocation failed"); return GFBE_DEVICE_ERROR; }
  }
  double *res = (double *)buf.result();
  if (n_edges) hipLaunchKernelGGL(k_lc6_eval, dim3((n_edges + 127) / 128), dim3(128), 0, s, n_edges, dt, dq, di, dj, dk, dm, o.huber_delta, o.t_var, o.q_var, dr, dJ, dc);
  hipLaunchKernelGGL(k_lc6_sum, dim3(1), dim3(LC6_RED_THREADS), 0, s, dc, n_edges, res);
  if (n_edges && r_out) (void)hipMemcpyAsync(hr, dr, sizeof(double) * 6 * n_edges, hipMemcpyDeviceToHost, s);
  if (n_edges && J_out) (void)hipMemcpyAsync(hJ, dJ, sizeof(double) * 72 * n_edges, hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) { ctx_set_error(c, "gfbe_lc6_eval: device error"); return GFBE_DEVICE_ERROR; }
  if (n_edges && r_out) std::memcpy(r_out, hr, sizeof(double) * 6 * n_edges);
  if (n_edges && J_out) std::memcpy(J_out, hJ, sizeof(double) * 72 * n_edges);
  if (cost) *cost = res[0];
  return GFBE_OK;
}

gfbe_status gfbe_lc6_solve(gfbe_ctx *c, const gfbe_lc6_options *opt, int32_t n, const double *t, const double *q, const int32_t *sequence, const uint8_t *fixed,
                           int32_t n_loop, const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out, double *q_out, double *drift,
                           gfbe_summary *S_out) {
  gfbe_lc6_options o;
  if (!c) return GFBE_BAD_INPUT;
  if (!options_ok(opt, &o)) { ctx_set_error(c, "gfbe_lc6_solve: gfbe_lc6_options of another size or out of range (ABI mismatch)"); return GFBE_BAD_INPUT; }
  if (n < 1 || !t || !q || !sequence || !fixed || !t_out || !q_out || n_loop < 0 || (n_loop && (!loop_i || !loop_c || !loop_meas))) return GFBE_BAD_INPUT;
  Lc6Plan plan;
  std::vector<uint8_t> has_loop(n);
  const int bad = lc6_check_graph(n, n_loop, loop_i, loop_c, o.span, has_loop.data());
  if (bad || !lc6_plan(n, n_loop, &plan)) {
    ctx_set_error(c, bad == 2 ? "gfbe_lc6_solve: more than GFBE_LC6_MAX_LOOPS loop edges" : "gfbe_lc6_solve: loop edges need 0 <= loop_c < loop_i < n, one per loop_i");
    return GFBE_BAD_INPUT;
  }
  if (!lc6_all_finite(t, (size_t)3 * n) || !lc6_all_finite(q, (size_t)4 * n) || (n_loop && !lc6_all_finite(loop_meas, (size_t)7 * n_loop))) {
    ctx_set_error(c, "gfbe_lc6_solve: a pose or a loop measurement is not finite");
    return GFBE_BAD_INPUT;
  }
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_lc6_solve: no device (no CPU fallback)"); return GFBE_NO_DEVICE; }
  const int max_it = std::min(o.max_num_iterations, 15);
  // the graph: sequence edges with their measurements (formed from the input poses), the loop edges that are kept, who is in the problem
  std::vector<unsigned char> emask(n, 0), free_(n, 0), loop_on(std::max(n_loop, 1), 0);
  std::vector<double> meas((size_t)28 * n, 0.0);
  for (int i = 0; i < n; i++)
    for (int k = 1; k <= o.span; k++)
      if (i - k >= 0 && sequence[i] == sequence[i - k] && !(fixed[i] && fixed[i - k])) {
        emask[i] |= (unsigned char)(1 << (k - 1));
        lc6_sequence_meas(t + 3 * (size_t)(i - k), q + 4 * (size_t)(i - k), t + 3 * (size_t)i, q + 4 * (size_t)i, &meas[((size_t)i * 4 + (k - 1)) * 7]);
        free_[i] = free_[i - k] = 1;
      }
  std::vector<int> lp_begin(n + 1, 0), lp_entry;
  for (int l = 0; l < n_loop; l++) {
    loop_on[l] = !(fixed[loop_c[l]] && fixed[loop_i[l]]);
    if (loop_on[l]) { free_[loop_c[l]] = free_[loop_i[l]] = 1; lp_begin[loop_c[l] + 1]++; lp_begin[loop_i[l] + 1]++; }
  }
  for (int i = 0; i < n; i++) { lp_begin[i + 1] += lp_begin[i]; if (fixed[i]) free_[i] = 0; }
  lp_entry.assign(std::max(lp_begin[n], 1), 0);
  {
    std::vector<int> fill(lp_begin.begin(), lp_begin.end() - 1);
    for (int l = 0; l < n_loop; l++)
      if (loop_on[l]) { lp_entry[fill[loop_c[l]]++] = 2 * l; lp_entry[fill[loop_i[l]]++] = 2 * l + 1; }
  }
  std::vector<double> x0((size_t)8 * n, 0.0);
  double xn2 = 0.0;
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 4; k++) x0[8 * (size_t)i + k] = q[4 * (size_t)i + k];
    for (int k = 0; k < 3; k++) x0[8 * (size_t)i + 4 + k] = t[3 * (size_t)i + k];
    if (free_[i]) for (int k = 0; k < 7; k++) xn2 += x0[8 * (size_t)i + k] * x0[8 * (size_t)i + k];
  }
  const double x_norm0 = std::sqrt(xn2);

  hipStream_t s = ctx_stream(c);
  static_assert(sizeof(Lc6State) <= LC6_RESULT_BYTES, "the pinned result slot holds the loop's state");
  Lc6Buffers buf(c);
  Lc6Dev P;
  Lc6Sets S;
  const int M = plan.M, rows = plan.rows, L = n_loop;
  double *cost_i, *cost_l, *gabs, *model_r, *step2_i, *xn2_i, *scale, *g0, *diag0, *diag2, *gs, *Bs, *As, *Cs, *Us, *big, *xo;
  Lc6State *dst;
  int *fail;
  size_t small_bytes = 0;
  for (int pass = 0; pass < 2; pass++) {
    dst = (Lc6State *)buf.dev<double>((sizeof(Lc6State) + 7) / 8);      // (cleared: cur = lb = 0, done = 0, ...)
    fail = buf.dev<int>(1);
    small_bytes = buf.used;
    P = {n, M, rows, L, plan.ld, plan.ntile, plan.cap_ld, buf.dev<unsigned char>(n, free_.data()), buf.dev<unsigned char>(n, emask.data()),
         buf.dev<double>((size_t)28 * n, meas.data()), buf.dev<int>(L, loop_c), buf.dev<int>(L, loop_i), buf.dev<double>((size_t)7 * L, loop_meas),
         buf.dev<unsigned char>(L, loop_on.data()), buf.dev<int>(n + 1, lp_begin.data()), buf.dev<int>(lp_entry.size(), lp_entry.data()), o.huber_delta, o.t_var, o.q_var};
    S.x[0] = buf.dev<double>((size_t)8 * n, x0.data()); S.x[1] = buf.dev<double>((size_t)8 * n);
    for (int k = 0; k < 2; k++) {
      S.Hb[k] = buf.dev<double>((size_t)1024 * M); S.Ha[k] = buf.dev<double>((size_t)1024 * M); S.Hc[k] = buf.dev<double>((size_t)1024 * M); S.g[k] = buf.dev<double>(rows);
      S.Uv[k] = buf.dev<double>((size_t)72 * L); S.gl[k] = buf.dev<double>((size_t)12 * L); S.dl[k] = buf.dev<double>((size_t)12 * L);
    }
    cost_i = buf.dev<double>(n); cost_l = buf.dev<double>(L); gabs = buf.dev<double>(rows); model_r = buf.dev<double>((size_t)rows + L);
    step2_i = buf.dev<double>(n); xn2_i = buf.dev<double>(n);
    scale = buf.dev<double>(rows); g0 = buf.dev<double>(rows); diag0 = buf.dev<double>(rows); diag2 = buf.dev<double>(rows); gs = buf.dev<double>(rows);
    Bs = buf.dev<double>((size_t)1024 * M); As = buf.dev<double>((size_t)1024 * M); Cs = buf.dev<double>((size_t)1024 * M); Us = buf.dev<double>((size_t)72 * L);
    big = buf.dev<double>(plan.total);      // the plan's carve: panels, band sets, multipliers, capacitance, step
    xo = buf.pinned<double>((size_t)8 * n);
    if (pass == 0 && !buf.commit(small_bytes)) { ctx_set_error(c, "gfbe_lc6_solve: device allocation failed"); return GFBE_DEVICE_ERROR; }
  }
  const Lc6Red Q = {cost_i, cost_l, gabs, model_r, step2_i, xn2_i};
  double *panel[2] = {big + plan.off_panel[0], big + plan.off_panel[1]};
  double *band[2][4];
  for (int k = 0; k < 2; k++) for (int b = 0; b < 4; b++) band[k][b] = big + plan.off_band[k][b];
  double *alpha = big + plan.off_alpha, *gamma = big + plan.off_gamma, *Sm = big + plan.off_S, *Lb = big + plan.off_L, *Dinv = big + plan.off_Dinv,
         *vcap = big + plan.off_v, *w = big + plan.off_w, *y = big + plan.off_y;
  const dim3 gr((rows + 255) / 256), b256(256);
  auto lin = [&](int cand) {
    hipLaunchKernelGGL(k_lc6_lin, gr, b256, 0, s, P, dst, S, cand, cost_i);
    if (L) hipLaunchKernelGGL(k_lc6_lin_loops, dim3((L + 63) / 64), dim3(64), 0, s, P, dst, S, cand, cost_l);
  };
  auto decide = [&](int mode) { hipLaunchKernelGGL(k_lc6_decide, dim3(1), dim3(LC6_RED_THREADS), 0, s, n, rows, L, Q, dst, fail, mode, x_norm0); };
  lin(0);
  decide(0);
  const dim3 gp(M, (plan.ntile + 1) / 2);
  const int fill_blocks = (int)std::min<size_t>(((size_t)rows * plan.ld + 255) / 256, 4096);
  const int gather_blocks = (int)std::min<size_t>(((size_t)plan.cap_ld * (plan.cap_ld + 1) + 255) / 256, LC6_GATHER_BLOCKS);
  // max_it passes, enqueued blindly: every kernel of a pass returns at once when the loop has ended
  for (int pass = 0; pass < max_it; pass++) {
    hipLaunchKernelGGL(k_lc6_scale, gr, b256, 0, s, P, dst, S, scale, g0, diag0, gabs);
    hipLaunchKernelGGL(k_lc6_system, gr, b256, 0, s, P, dst, S, scale, g0, diag0, diag2, gs, Bs, As, Cs, band[0][1], band[0][0], band[0][2]);
    hipLaunchKernelGGL(k_lc6_panel_fill, dim3(fill_blocks), b256, 0, s, rows, plan.ld, dst, gs, panel[0]);
    if (L) hipLaunchKernelGGL(k_lc6_loop_cols, dim3((72 * L + 255) / 256), b256, 0, s, P, dst, S, scale, Us, panel[0]);
    hipLaunchKernelGGL(k_lc6_inv0, dim3(M), b256, 0, s, M, dst, band[0][1], band[0][3], fail);
    int cur = 0;
    for (int sw = 0, stride = 1; sw < plan.sweeps; sw++, stride *= 2) {
      hipLaunchKernelGGL(k_lc6_pcr_blocks, dim3(M), b256, 0, s, M, stride, dst, band[cur][0], band[cur][1], band[cur][2], band[cur][3], band[1 - cur][0], band[1 - cur][1],
                         band[1 - cur][2], band[1 - cur][3], alpha, gamma, fail);
      hipLaunchKernelGGL(k_lc6_pcr_panel, gp, b256, 0, s, M, stride, plan.ld, plan.ntile, dst, alpha, gamma, panel[cur], panel[1 - cur]);
      cur = 1 - cur;
    }
    double *Z = panel[1 - cur];
    hipLaunchKernelGGL(k_lc6_final, gp, b256, 0, s, plan.ld, plan.ntile, dst, band[cur][3], panel[cur], Z);
    if (L) {      // 1 + 2 cap_ld / 16 launches
      hipLaunchKernelGGL(k_lc6_cap_gather, dim3(gather_blocks), b256, 0, s, P, dst, Us, Z, Sm, vcap);
      launch_lc4_cap_factor(plan.cap_ld, dst, Sm, Lb, Dinv, vcap, w, fail, s);
    }
    hipLaunchKernelGGL(k_lc6_apply, gr, b256, 0, s, rows, plan.ld, 6 * L, dst, Z, w, y);
    hipLaunchKernelGGL(k_lc6_candidate, dim3((rows + L + 255) / 256), b256, 0, s, P, dst, S, Bs, As, Cs, gs, Us, y, scale, model_r, step2_i, xn2_i);
    decide(1);
    lin(1);      // the candidate's cost — and its linearisation, should it be accepted
    decide(2);
  }
  Lc6State *hst = (Lc6State *)buf.result();
  hipLaunchKernelGGL(k_lc6_finish, dim3(std::min(256, (8 * n + 255) / 256)), b256, 0, s, n, dst, S, xo, hst);
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) { ctx_set_error(c, "gfbe_lc6_solve: device error"); return GFBE_DEVICE_ERROR; }
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 4; k++) q_out[4 * (size_t)i + k] = xo[8 * (size_t)i + k];
    for (int k = 0; k < 3; k++) t_out[3 * (size_t)i + k] = xo[8 * (size_t)i + 4 + k];
  }
  if (drift) {      // pose_graph.cpp:849-850: r_drift = cur_r vio_r^T, t_drift = cur_t - r_drift vio_t of the last keyframe
    double ci[4], R[9];
    const double *v = t + 3 * (size_t)(n - 1), *u = t_out + 3 * (size_t)(n - 1);
    lc6_qconj(q + 4 * (size_t)(n - 1), ci);
    lc6_qmul(q_out + 4 * (size_t)(n - 1), ci, drift);
    lc6_quat_to_R(drift, R);
    for (int a = 0; a < 3; a++) drift[4 + a] = u[a] - (R[3 * a] * v[0] + R[3 * a + 1] * v[1] + R[3 * a + 2] * v[2]);
  }
  gfbe_summary sm;
  std::memset(&sm, 0, sizeof sm);
  sm.status = hst->status; sm.termination = hst->done ? hst->termination : 0;
  sm.iterations = hst->it; sm.num_successful = hst->num_successful;
  sm.initial_cost = hst->initial_cost; sm.final_cost = hst->cost; sm.final_radius = hst->radius;
  for (int k = 0; k < 16; k++) { sm.cost_history[k] = hst->cost_history[k]; sm.accepted[k] = (uint8_t)hst->accepted[k]; }
  if (S_out) *S_out = sm;
  return sm.status == GFBE_NUMERICAL_FAILURE ? GFBE_NUMERICAL_FAILURE : GFBE_OK;
}

}  // extern "C"
