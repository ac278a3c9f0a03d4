// gfbe_loopgraph.hip — the loop-closure pose graph of dense_map on the device (gfbe_lc4_eval, gfbe_lc4_solve, gfbe_lc4_solve_long).
//
//   PoseGraph::optimize4DoF             dense_map/src/pose_graph.cpp:529-705 (options :558-566)
//   FourDOFError, FourDOFWeightError    dense_map/src/pose_graph.h:199-288
//
// State: yaw (degrees) + t per keyframe, tangent [yaw t_x t_y t_z]. Sequence edges reach at most four keyframes back, so four
// consecutive poses form one 16 x 16 super-block and the sequence part of J^T J is block-tridiagonal in super-blocks; a loop edge adds
// J_l^T J_l, four sparse columns (8 non-zeros each) of U: H = T + U U^T. One Levenberg-Marquardt step solves
//   T Z = [-g | U]              parallel block cyclic reduction over the M super-blocks, ceil(log2 M) sweeps; the multipliers
//                               alpha = -A B^-1 are applied to the blocks and to the panel by v_mfma_f64_16x16x4_f64, one 16 x 16
//                               multiplier against 16-column tiles of the panel (ping-pong in the context's scratch);
//   S = I + U^T Z               gathered through U's 8 non-zeros per column, factorised by ONE workgroup as a block LDL^T in 16-wide
//                               tiles through L2 (the pivot tile inverted as the super-blocks are, matrix cores for L_IP and the
//                               trailing update), then y = z_0 - Z S^-1 U^T z_0. Beyond LC4_MAX_LOOPS loop edges
//                               (gfbe_lc4_solve_long) the same factorisation runs across workgroups, one pivot step per launch pair.
// Every sum runs in a fixed order (owner-computes linearisation, no atomics); the trust-region loop (the statements of k_pg_decide,
// restated) lives in a device struct: the host enqueues max_num_iterations passes and waits once, every kernel returns at once when
// `done` is set, nothing spins and no kernel waits on another workgroup. tests/lc4_np.py is the model, phase for phase.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"
#include "gfbe_loopgraph.h"

using namespace gfd;

namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));

struct Lc4Dev {
  int n, M, rows, L, ld, ntile, cap_ld;
  const unsigned char *free_;     // [n] the pose is in the problem
  const unsigned char *emask;     // [n] bit k - 1: the sequence edge (i - k, i) exists
  const double *meas;             // [n][4][6] its measurement
  const int *loop_c, *loop_i;     // [L]
  const double *loop_meas;        // [L][6]
  const unsigned char *loop_on;   // [L] (an edge between two constant poses is dropped)
  const int *lp_begin, *lp_entry; // CSR per pose of 2 l + side, ascending l: the loop edges whose shares the pose's rows take
  double delta, yaw_div;
};

struct Lc4Sets {
  double *x[2];                                  // [n][4] yaw | t
  double *Hb[2], *Ha[2], *Hc[2], *g[2];          // [M][16][16] diagonal / (m, m - 1) / (m, m + 1) super-blocks, [rows]
  double *Uv[2], *gl[2], *dl[2];                 // per loop edge: corrected J (4 x 8), its gradient and diagonal shares [8]
};

__device__ __forceinline__ double sel4(const double *p, int a) { return a == 0 ? p[0] : (a == 1 ? p[1] : (a == 2 ? p[2] : p[3])); }

// ---- evaluation only (gfbe_lc4_eval): one thread per edge
__global__ __launch_bounds__(128) void k_lc4_eval(int n_edges, const double *t, const double *ypr, const int *ei, const int *ej, const unsigned char *kind, const double *meas,
                                                  double delta, double yaw_div, double *r_out, double *J_out, double *cost_e) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const int i = ei[e], j = ej[e];
  double r[4], J[32];
  cost_e[e] = lc4_edge(kind[e], ypr[3 * (size_t)i], t + 3 * (size_t)i, ypr[3 * (size_t)j], t + 3 * (size_t)j, meas + 6 * (size_t)e, delta, yaw_div, r, J);
  for (int q = 0; q < 4; q++) r_out[4 * (size_t)e + q] = r[q];
  for (int q = 0; q < 32; q++) J_out[32 * (size_t)e + q] = J[q];
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
__global__ __launch_bounds__(LCD_THREADS) void k_lc4_sum(const double *p, int len, double *out) {
  __shared__ double sh[17];
  const double s = block_reduce(p, len, false, sh);
  if (threadIdx.x == 0) *out = s;
}

// ---- linearisation of the sequence edges, owner-computes: lane a of pose i (one thread per row of the padded system) evaluates the
// pose's up to 2 x 4 sequence edges and writes ITS row of the super-blocks and of g — an off-diagonal 4-block is one edge's term, the
// diagonal block and g are summed over the edges k = 1 .. 4 backwards, then k = 1 .. 4 forwards. The edge is evaluated by each of the
// four lanes of a pose (a rotation and 32 products; the alternative stages 36 doubles per edge through LDS).
// cand = 0: the first linearisation (x into its set); 1: the candidate's cost AND linearisation, into the other set.
__global__ __launch_bounds__(256) void k_lc4_lin(Lc4Dev P, const Lc4State *st, Lc4Sets S, int cand, double *cost_i) {
  const int f_done = st->done, f_cand = st->cand_on, f_cur = st->cur, f_lb = st->lb;
  if (cand && (f_done || !f_cand)) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows) return;
  const int i = row >> 2, a = row & 3, m = row >> 4, R = row & 15;
  const int xb = cand ? 1 - f_cur : f_cur, sb = cand ? 1 - f_lb : f_lb;
  const double *x = S.x[xb];
  double *Hb = S.Hb[sb] + (size_t)m * 256 + R * 16, *Ha = S.Ha[sb] + (size_t)m * 256 + R * 16, *Hc = S.Hc[sb] + (size_t)m * 256 + R * 16;
  for (int c = 0; c < 16; c++) { Hb[c] = 0.0; Ha[c] = 0.0; Hc[c] = 0.0; }
  double dg[4] = {0.0, 0.0, 0.0, 0.0}, ga = 0.0, cost = 0.0;
  if (i < P.n) {
    const bool fi = P.free_[i] != 0;
#pragma unroll
    for (int dir = 0; dir < 2; dir++) {
#pragma unroll
      for (int k = 1; k <= LC4_MAX_SPAN; k++) {
        const int j = dir == 0 ? i - k : i + k;      // the other end
        if (j < 0 || j >= P.n) continue;
        const int hi = dir == 0 ? i : j, lo = dir == 0 ? j : i;      // the edge (lo, hi) is stored with hi
        if (!((P.emask[hi] >> (k - 1)) & 1)) continue;
        double r[4], J[32];
        lc4_edge(0, x[4 * (size_t)lo], x + 4 * (size_t)lo + 1, x[4 * (size_t)hi], x + 4 * (size_t)hi + 1, P.meas + ((size_t)hi * 4 + (k - 1)) * 6, P.delta, P.yaw_div, r, J);
        if (dir == 1 && a == 0) cost += 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);      // (the edge's first pose owns its cost)
        const bool fj = P.free_[j] != 0;
        const int mine = dir == 0 ? 4 : 0, other = 4 - mine;      // this pose's columns of J: the "j" side of a backward edge
        double cm[4];
#pragma unroll
        for (int q = 0; q < 4; q++) cm[q] = fi ? sel4(J + q * 8 + mine, a) : 0.0;
        const int mj = j >> 2;
        double *tgt = (mj == m ? Hb : (mj < m ? Ha : Hc)) + 4 * (j & 3);
#pragma unroll
        for (int b = 0; b < 4; b++) {
          double so = 0.0, sd = 0.0;
#pragma unroll
          for (int q = 0; q < 4; q++) { so += cm[q] * (fj ? J[q * 8 + other + b] : 0.0); sd += cm[q] * (fi ? J[q * 8 + mine + b] : 0.0); }
          tgt[b] = so;
          dg[b] += sd;
        }
        double sv = 0.0;
#pragma unroll
        for (int q = 0; q < 4; q++) sv += cm[q] * r[q];
        ga += sv;
      }
    }
#pragma unroll
    for (int b = 0; b < 4; b++) Hb[4 * (i & 3) + b] = dg[b];
    if (a == 0) cost_i[i] = cost;
  }
  S.g[sb][row] = ga;
}
// the loop edges: one thread per edge, through the corrector; four columns of U (the rows of the corrected J), the edge's share of g and
// of the diagonal the Jacobi scaling needs, its cost
__global__ __launch_bounds__(64) void k_lc4_lin_loops(Lc4Dev P, const Lc4State *st, Lc4Sets S, int cand, double *cost_l) {
  const int f_done = st->done, f_cand = st->cand_on, f_cur = st->cur, f_lb = st->lb;
  if (cand && (f_done || !f_cand)) return;
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= P.L) return;
  const int xb = cand ? 1 - f_cur : f_cur, sb = cand ? 1 - f_lb : f_lb;
  const double *x = S.x[xb];
  double r[4] = {0.0, 0.0, 0.0, 0.0}, J[32], cost = 0.0;
  for (int q = 0; q < 32; q++) J[q] = 0.0;
  if (P.loop_on[l]) {
    const int c = P.loop_c[l], i = P.loop_i[l];
    cost = lc4_edge(1, x[4 * (size_t)c], x + 4 * (size_t)c + 1, x[4 * (size_t)i], x + 4 * (size_t)i + 1, P.loop_meas + 6 * (size_t)l, P.delta, P.yaw_div, r, J);
    const bool fc = P.free_[c] != 0, fi = P.free_[i] != 0;
    for (int q = 0; q < 4; q++)
      for (int b = 0; b < 4; b++) { if (!fc) J[q * 8 + b] = 0.0; if (!fi) J[q * 8 + 4 + b] = 0.0; }
  }
  cost_l[l] = cost;
  for (int q = 0; q < 32; q++) S.Uv[sb][32 * (size_t)l + q] = J[q];
  for (int k = 0; k < 8; k++) {
    double sg = 0.0, sd = 0.0;
    for (int q = 0; q < 4; q++) { sg += J[q * 8 + k] * r[q]; sd += J[q * 8 + k] * J[q * 8 + k]; }
    S.gl[sb][8 * (size_t)l + k] = sg;
    S.dl[sb][8 * (size_t)l + k] = sd;
  }
}

// ---- the scaled Levenberg-Marquardt system
// per row: the full gradient and diagonal (sequence part + the pose's loop shares in ascending edge order), the Jacobi scale (first pass)
__global__ __launch_bounds__(256) void k_lc4_scale(Lc4Dev P, const Lc4State *st, Lc4Sets S, double *scale, double *g0, double *diag0, double *gabs) {
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows) return;
  const int lb = st->lb, i = row >> 2, a = row & 3, m = row >> 4, R = row & 15;
  const bool act = i < P.n && P.free_[i];
  double d0 = S.Hb[lb][(size_t)m * 256 + R * 17], gg = S.g[lb][row];
  if (i < P.n)
    for (int e = P.lp_begin[i]; e < P.lp_begin[i + 1]; e++) {
      const int en = P.lp_entry[e], l = en >> 1, k = 4 * (en & 1) + a;
      d0 += S.dl[lb][8 * (size_t)l + k];
      gg += S.gl[lb][8 * (size_t)l + k];
    }
  if (!st->have_scale) scale[row] = act ? 1.0 / (1.0 + sqrt(d0)) : 1.0;
  g0[row] = act ? gg : 0.0;
  gabs[row] = act ? fabs(gg) : 0.0;
  diag0[row] = act ? d0 : 0.0;
}
// per row: S T0 S (unregularised: Bs As Cs, for the model cost) and its copy with the LM diagonal (B A C, what the reduction consumes); a
// row out of the problem is an identity row
__global__ __launch_bounds__(256) void k_lc4_system(Lc4Dev P, const Lc4State *st, Lc4Sets S, const double *scale, const double *g0, const double *diag0, double *diag2, double *gs,
                                                    double *Bs, double *As, double *Cs, double *B, double *A, double *C) {
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows) return;
  const int lb = st->lb, i = row >> 2, m = row >> 4, R = row & 15;
  const bool act = i < P.n && P.free_[i];
  const double sa = scale[row], radius = st->radius;
  const size_t o = (size_t)m * 256 + R * 16;
  for (int c = 0; c < 16; c++) {
    const double vb = S.Hb[lb][o + c] * sa * scale[16 * m + c];
    const double va = m > 0 ? S.Ha[lb][o + c] * sa * scale[16 * (m - 1) + c] : 0.0;
    const double vc = m + 1 < P.M ? S.Hc[lb][o + c] * sa * scale[16 * (m + 1) + c] : 0.0;
    Bs[o + c] = vb; As[o + c] = va; Cs[o + c] = vc;
    B[o + c] = vb; A[o + c] = va; C[o + c] = vc;
  }
  if (!st->reuse) diag2[row] = fmin(fmax(diag0[row] * sa * sa, 1e-6), 1e32);
  B[o + R] = act ? Bs[o + R] + diag2[row] / radius : 1.0;
  gs[row] = sa * g0[row];
}
// the panel [-gs | 0], element by element
__global__ __launch_bounds__(256) void k_lc4_panel_fill(int rows, int ld, const Lc4State *st, const double *gs, double *panel) {
  if (st->done) return;
  const size_t total = (size_t)rows * ld;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t row = e / ld;
    panel[e] = (e - row * ld) == 0 ? -gs[row] : 0.0;
  }
}
// ... and the scaled columns of U scattered into it: one thread per non-zero (l, q, k)
__global__ __launch_bounds__(256) void k_lc4_loop_cols(Lc4Dev P, const Lc4State *st, Lc4Sets S, const double *scale, double *Us, double *panel) {
  if (st->done) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 32 * P.L) return;
  const int l = e >> 5, q = (e >> 3) & 3, k = e & 7;
  const int row = 4 * (k < 4 ? P.loop_c[l] : P.loop_i[l]) + (k & 3);
  const double v = S.Uv[st->lb][e] * scale[row];
  Us[e] = v;
  panel[(size_t)row * P.ld + 1 + 4 * l + q] = v;
}

// ---- inverse of an SPD 16 x 16 block by Gauss-Jordan on [B | I] without pivoting, by the first 64 threads of the workgroup (every
// thread of the workgroup calls it: block barriers). W: [16][33] in LDS, its left half loaded by the caller. Thread t < 64 owns column
// t & 31 of the rows (t >> 5) + 2 j. A pivot that is not positive (or not finite) raises *fail; the elimination goes on with 1.
enum { GJ_LD = 33 };
__device__ void gj_inverse16(double *W, int t, int *fail) {
  const int col = t & 31, r0 = t >> 5;
  if (t < 64) {
#pragma unroll
    for (int j = 0; j < 8; j++) if (col >= 16) W[(r0 + 2 * j) * GJ_LD + col] = (col - 16 == r0 + 2 * j) ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int c = 0; c < 16; c++) {
    double rc = 0.0, f[8];
    if (t < 64) {
      double p = W[c * GJ_LD + c];
      if (!(p > 0.0) || !isfinite(p)) { if (t == 0) *fail = 1; p = 1.0; }
      rc = W[c * GJ_LD + col] / p;
#pragma unroll
      for (int j = 0; j < 8; j++) f[j] = W[(r0 + 2 * j) * GJ_LD + c];
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int r = r0 + 2 * j;
        W[r * GJ_LD + col] = r == c ? rc : W[r * GJ_LD + col] - f[j] * rc;
      }
    }
    __syncthreads();
  }
}
// the symmetrised inverse out of W's right half: entry e = t, t + 64, ... of the 16 x 16 block
__device__ __forceinline__ void gj_store(const double *W, int t, double *out, double *lds_out) {
  if (t < 64) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int e = t + 64 * j, r = e >> 4, c = e & 15;
      const double v = (W[r * GJ_LD + 16 + c] + W[c * GJ_LD + 16 + r]) / 2;
      if (out) out[e] = v;
      if (lds_out) lds_out[e] = v;
    }
  }
}
// the blocks' first inverses (before any sweep): one wave per super-block
__global__ __launch_bounds__(64) void k_lc4_inv0(int M, const Lc4State *st, const double *B, double *Binv, int *fail) {
  __shared__ double W[16 * GJ_LD];
  if (st->done) return;
  const int t = threadIdx.x, m = blockIdx.x;
#pragma unroll
  for (int j = 0; j < 4; j++) { const int e = t + 64 * j; W[(e >> 4) * GJ_LD + (e & 15)] = B[(size_t)m * 256 + e]; }
  gj_inverse16(W, t, fail);
  gj_store(W, t, Binv + (size_t)m * 256, nullptr);
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

// One sweep of parallel block cyclic reduction at stride s over the super-blocks, the blocks' half: one wave per super-block i.
//   alpha = -A_i B_{i-s}^-1, gamma = -C_i B_{i+s}^-1 (kept for the panel's half)
//   B' = B + alpha C_{i-s} + gamma A_{i+s};  A' = alpha A_{i-s};  C' = gamma C_{i+s};  B'^-1 travels with the block.
__global__ __launch_bounds__(64) void k_lc4_pcr_blocks(int M, int s, const Lc4State *st, const double *A, const double *B, const double *C, const double *Binv,
                                                       double *A2, double *B2, double *C2, double *Binv2, double *alpha, double *gamma, int *fail) {
  __shared__ double sAl[256], sGa[256], W[16 * GJ_LD];
  if (st->done) return;
  const int t = threadIdx.x, lr = t & 15, lk = t >> 4, i = blockIdx.x, im = i - s, ip = i + s;
  const bool hm = im >= 0, hp = ip < M;
  const size_t o = (size_t)i * 256;
  const dbl4 zero = {0.0, 0.0, 0.0, 0.0};
  dbl4 al = zero, ga = zero;
  if (hm) al = mm16(A + o, 16, Binv + (size_t)im * 256, 16, zero, lr, lk, -1.0);
  if (hp) ga = mm16(C + o, 16, Binv + (size_t)ip * 256, 16, zero, lr, lk, -1.0);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int e = (lk + 4 * q) * 16 + lr;
    sAl[e] = al[q]; sGa[e] = ga[q];
    alpha[o + e] = al[q]; gamma[o + e] = ga[q];
  }
  __syncthreads();
  dbl4 Bn, An = zero, Cn = zero;
#pragma unroll
  for (int q = 0; q < 4; q++) Bn[q] = B[o + (lk + 4 * q) * 16 + lr];
  if (hm) {
    Bn = mm16(sAl, 16, C + (size_t)im * 256, 16, Bn, lr, lk, 1.0);
    An = mm16(sAl, 16, A + (size_t)im * 256, 16, zero, lr, lk, 1.0);
  }
  if (hp) {
    Bn = mm16(sGa, 16, A + (size_t)ip * 256, 16, Bn, lr, lk, 1.0);
    Cn = mm16(sGa, 16, C + (size_t)ip * 256, 16, zero, lr, lk, 1.0);
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int r = lk + 4 * q, e = r * 16 + lr;
    A2[o + e] = An[q]; B2[o + e] = Bn[q]; C2[o + e] = Cn[q];
    W[r * GJ_LD + lr] = Bn[q];
  }
  gj_inverse16(W, t, fail);
  gj_store(W, t, Binv2 + o, nullptr);
}
// ... and the panel's half: wave w of workgroup (i, y) takes tile column 4 y + w of super-block i:
//   P'_i = P_i + alpha_i P_{i-s} + gamma_i P_{i+s}
__global__ __launch_bounds__(256) void k_lc4_pcr_panel(int M, int s, int ld, int ntile, const Lc4State *st, const double *alpha, const double *gamma, const double *pin, double *pout) {
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, lr = lane & 15, lk = lane >> 4, i = blockIdx.x, tc = blockIdx.y * 4 + (t >> 6);
  if (tc >= ntile) return;
  const int im = i - s, ip = i + s;
  const double *pi = pin + (size_t)16 * i * ld + 16 * tc;
  dbl4 acc;
#pragma unroll
  for (int q = 0; q < 4; q++) acc[q] = pi[(size_t)(lk + 4 * q) * ld + lr];
  if (im >= 0) acc = mm16(alpha + (size_t)i * 256, 16, pin + (size_t)16 * im * ld + 16 * tc, ld, acc, lr, lk, 1.0);
  if (ip < M) acc = mm16(gamma + (size_t)i * 256, 16, pin + (size_t)16 * ip * ld + 16 * tc, ld, acc, lr, lk, 1.0);
  double *po = pout + (size_t)16 * i * ld + 16 * tc;
#pragma unroll
  for (int q = 0; q < 4; q++) po[(size_t)(lk + 4 * q) * ld + lr] = acc[q];
}
// after the last sweep the super-blocks are decoupled: Z_i = B_i^-1 P_i, tile by tile
__global__ __launch_bounds__(256) void k_lc4_final(int ld, int ntile, const Lc4State *st, const double *Binv, const double *pin, double *Z) {
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, lr = lane & 15, lk = lane >> 4, i = blockIdx.x, tc = blockIdx.y * 4 + (t >> 6);
  if (tc >= ntile) return;
  const dbl4 zero = {0.0, 0.0, 0.0, 0.0};
  const dbl4 acc = mm16(Binv + (size_t)i * 256, 16, pin + (size_t)16 * i * ld + 16 * tc, ld, zero, lr, lk, 1.0);
  double *po = Z + (size_t)16 * i * ld + 16 * tc;
#pragma unroll
  for (int q = 0; q < 4; q++) po[(size_t)(lk + 4 * q) * ld + lr] = acc[q];
}

// ---- the capacitance system, ONE workgroup: S = I + U^T Z[:, 1:] gathered through U's 8 non-zeros per column (identity padding up to
// a tile), v = U^T z_0; block LDL^T in 16-wide tiles through global memory (S is up to 256 x 256 doubles: 512 KB) — the pivot tile
// inverted by wave 0 (gj_inverse16), L_IP = S_IP D_P^-1 and the trailing update S_IJ -= L_IP S_JP^T on the matrix cores, the tiles
// round-robin over the four waves —, then w = S^-1 v by substitution on LDS.
__global__ __launch_bounds__(256) void k_lc4_cap(Lc4Dev P, const Lc4State *st, const double *Us, const double *Z, double *Sm, double *Lb, double *Dinv, double *w, int *fail) {
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
    gj_inverse16(W, t, fail);
    gj_store(W, t, Dinv + (size_t)p * 256, sD);
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
// ---- the capacitance system beyond LC4_MAX_LOOPS loop edges (gfbe_lc4_solve_long; N = cap_ld up to 2048, 128 tile columns): the
// algorithm of k_lc4_cap spread over the device and ordered by launch boundaries alone — a gather, per pivot step p one launch for the
// tile column (k_lc4_cap_panel) and one for the trailing update (k_lc4_cap_trail), then the substitution (k_lc4_cap_back). Within a
// launch no workgroup reads what another one writes: the panel launch reads column p of S and writes column p of L, the trailing
// launch reads those two columns and writes the columns behind them. Every tile is written by one wave per launch, by one fixed
// sequence of operations, and every entry of S, L, D^-1 and v that is read was written in this pass.
enum { LC4_GATHER_BLOCKS = 2048 };
// S = I + U^T Z[:, 1:] and v = U^T z_0 (entry N N + a), element by element: the 8-term sum of k_lc4_cap in its order; padding = identity
__global__ __launch_bounds__(256) void k_lc4_cap_gather(Lc4Dev P, const Lc4State *st, const double *Us, const double *Z, double *Sm, double *v) {
  if (st->done) return;
  const size_t N = (size_t)P.cap_ld, NN = N * N, total = NN + N;
  const int c4 = 4 * P.L, ld = P.ld;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const bool vec = e >= NN;
    const int a = vec ? (int)(e - NN) : (int)(e / N), b = vec ? -1 : (int)(e - (size_t)a * N);      // (b = -1: column 0 of Z)
    double s = a == b ? 1.0 : 0.0;
    if (a < c4 && b < c4) {
      const int l = a >> 2;
      for (int k = 0; k < 8; k++) {
        const int row = 4 * (k < 4 ? P.loop_c[l] : P.loop_i[l]) + (k & 3);
        s += Us[8 * (size_t)a + k] * Z[(size_t)row * ld + 1 + b];
      }
    }
    if (vec) v[a] = s; else Sm[e] = s;
  }
}
// pivot step p, the tile column: every workgroup inverts the pivot tile S_pp for itself (the same instructions on the same values),
// workgroup 0 keeps D_p^-1; wave w of workgroup b takes tile row I = p + 1 + 4 b + w: L_Ip = S_Ip D_p^-1 on the matrix cores, and the
// forward substitution rides along, v_I -= L_Ip v_p (v_p is final since the launch of step p - 1), one lane per row, columns in order
__global__ __launch_bounds__(256) void k_lc4_cap_panel(int N, int p, const Lc4State *st, const double *Sm, double *Lb, double *Dinv, double *v, int *fail) {
  __shared__ double W[16 * GJ_LD], sD[256], sL[4][16 * 17], svp[16];
  if (st->done) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 15, lk = lane >> 4, nt = N / 16;
  if (t < 64) {
#pragma unroll
    for (int j = 0; j < 4; j++) { const int e = t + 64 * j; W[(e >> 4) * GJ_LD + (e & 15)] = Sm[(size_t)(16 * p + (e >> 4)) * N + 16 * p + (e & 15)]; }
  }
  if (t < 16) svp[t] = v[16 * p + t];
  gj_inverse16(W, t, fail);
  gj_store(W, t, blockIdx.x == 0 ? Dinv + (size_t)p * 256 : nullptr, sD);
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
__global__ __launch_bounds__(256) void k_lc4_cap_trail(int N, int p, const Lc4State *st, double *Sm, const double *Lb) {
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
__global__ __launch_bounds__(LC4_BACK_THREADS) void k_lc4_cap_back(int N, const Lc4State *st, const double *Lb, const double *Dinv, const double *v, double *w) {
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
// y = z_0 - Z[:, 1:] w, one thread per row, the columns in order
__global__ __launch_bounds__(256) void k_lc4_apply(int rows, int ld, int c4, const Lc4State *st, const double *Z, const double *w, double *y) {
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const double *z = Z + (size_t)row * ld;
  double v = z[0];
  for (int b = 0; b < c4; b++) v -= z[1 + b] * w[b];
  y[row] = v;
}

// ---- the candidate: per row the share -(gs y + y (T0s y) / 2) of the model cost change, per loop edge -|Us_l^T y|^2 / 2 (threads
// behind the rows), and lane 0 of every pose retracts: x (+) S y, with its shares of |step|^2 and |candidate|^2 (free poses only)
__global__ __launch_bounds__(256) void k_lc4_candidate(Lc4Dev P, const Lc4State *st, Lc4Sets S, const double *Bs, const double *As, const double *Cs, const double *gs, const double *Us,
                                                       const double *y, const double *scale, double *model_r, double *step2_i, double *xn2_i) {
  if (st->done) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= P.rows + P.L) return;
  if (row >= P.rows) {
    const int l = row - P.rows;
    double s2 = 0.0;
    for (int q = 0; q < 4; q++) {
      double p = 0.0;
      for (int k = 0; k < 8; k++) p += Us[32 * (size_t)l + q * 8 + k] * y[4 * (k < 4 ? P.loop_c[l] : P.loop_i[l]) + (k & 3)];
      s2 += p * p;
    }
    model_r[row] = -0.5 * s2;
    return;
  }
  const int i = row >> 2, m = row >> 4, R = row & 15;
  const size_t o = (size_t)m * 256 + R * 16;
  double s = 0.0;
  for (int c = 0; c < 16; c++) s += Bs[o + c] * y[16 * m + c];
  if (m > 0) for (int c = 0; c < 16; c++) s += As[o + c] * y[16 * (m - 1) + c];
  if (m + 1 < P.M) for (int c = 0; c < 16; c++) s += Cs[o + c] * y[16 * (m + 1) + c];
  model_r[row] = -(gs[row] * y[row] + 0.5 * (y[row] * s));
  if ((row & 3) != 0 || i >= P.n) return;
  const double *x = S.x[st->cur] + 4 * (size_t)i;
  double *cand = S.x[1 - st->cur] + 4 * (size_t)i;
  double out[4] = {x[0], x[1], x[2], x[3]}, s2 = 0.0, x2 = 0.0;
  if (P.free_[i]) {
    out[0] = lc4_normalize_angle(x[0] + scale[row] * y[row]);
    for (int k = 1; k < 4; k++) out[k] = x[k] + scale[row + k] * y[row + k];
    for (int k = 0; k < 4; k++) { const double df = out[k] - x[k]; s2 += df * df; x2 += out[k] * out[k]; }
  }
  for (int k = 0; k < 4; k++) cand[k] = out[k];
  step2_i[i] = s2; xn2_i[i] = x2;
}

// ---- the reductions of a pass and what follows from them: TrustRegionMinimizer with LevenbergMarquardtStrategy under the options of
// pose_graph.cpp:558-566 (Ceres 1.14 defaults otherwise), the statements and their order as in k_pg_decide:
//   mode 0 — the first point's cost; mode 1 — after the solve and the candidate (max |g|, model change, |step|^2, |candidate|^2, the
//   failure flag); mode 2 — after the candidate's evaluation (its cost).
struct Lc4Red { const double *cost_i, *cost_l, *gabs, *model_r, *step2_i, *xn2_i; };
__global__ __launch_bounds__(LCD_THREADS) void k_lc4_decide(Lc4Dev P, Lc4Red Q, Lc4State *st, int *fail, int mode, double x_norm0) {
  __shared__ double sh[17];
  const int f_done = mode != 0 ? st->done : 0, f_cand = st->cand_on;
  if (f_done || (mode == 2 && !f_cand)) return;      // (uniform over the workgroup)
  double r0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  if (mode == 1) {
    r0 = block_reduce(Q.gabs, P.rows, true, sh);
    r1 = block_reduce(Q.model_r, P.rows + P.L, false, sh);
    r2 = block_reduce(Q.step2_i, P.n, false, sh);
    r3 = block_reduce(Q.xn2_i, P.n, false, sh);
  } else {
    r0 = block_reduce(Q.cost_i, P.n, false, sh);
    r0 += block_reduce(Q.cost_l, P.L, false, sh);
  }
  if (threadIdx.x != 0) return;
  Lc4State &s = *st;
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
__global__ __launch_bounds__(256) void k_lc4_finish(int n, const Lc4State *st, Lc4Sets S, double *x_out, Lc4State *st_out) {
  const double *x = S.x[st->cur];
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)4 * n; e += (size_t)gridDim.x * 256) x_out[e] = x[e];
  if (blockIdx.x == 0 && threadIdx.x == 0) *st_out = *st;
}

// ---- one slab out of the context's grow-only scratch, carved by a dry run; host arrays travel through the pinned scratch
// (the scheme of PgBuffers, restated here: gfbe_posegraph.hip keeps its own, file-local one)
enum { LC4_RESULT_BYTES = 1024 };
struct Lc4Buffers {
  gfbe_ctx *c;
  char *slab = nullptr, *pin = nullptr;
  size_t cap = 0, used = 0, pin_cap = 0, pin_used = 0;
  bool dry = true;
  explicit Lc4Buffers(gfbe_ctx *ctx) : c(ctx) {}
  ~Lc4Buffers() { (void)hipStreamSynchronize(ctx_stream(c)); }
  bool commit(size_t clear_bytes) {      // clear_bytes: the head of the slab that is cleared (the loop's state and the small arrays)
    cap = used; used = 0; dry = false;
    pin_cap = pin_used; pin_used = 0;
    slab = (char *)ctx_scratch(c, std::max<size_t>(cap, 256));
    pin = (char *)ctx_scratch_pinned(c, pin_cap + LC4_RESULT_BYTES);
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

}  // namespace

// The blocked factorisation of an SPD capacitance system S w = v that lies in device memory (N a multiple of 16, at most LC4_BACK_N;
// S and v as k_lc4_cap_gather leaves them, identity padding included): per pivot step one k_lc4_cap_panel and one k_lc4_cap_trail
// launch, then k_lc4_cap_back, 2 N / 16 launches in all. gfbe_lc4_solve_long and gfbe_lc6_solve (gfbe_loopgraph6.hip) share it; `st` is
// the loop's state whose `done` the kernels read first.
void gfd::launch_lc4_cap_factor(int N, const Lc4State *st, double *Sm, double *Lb, double *Dinv, double *v, double *w, int *fail, hipStream_t s) {
  const int cap_nt = N / LC4_SB;
  for (int p = 0; p < cap_nt; p++) {
    const int nrem = cap_nt - 1 - p;
    hipLaunchKernelGGL(k_lc4_cap_panel, dim3(std::max(1, (nrem + 3) / 4)), dim3(256), 0, s, N, p, st, Sm, Lb, Dinv, v, fail);
    if (nrem) hipLaunchKernelGGL(k_lc4_cap_trail, dim3(nrem, (nrem + 3) / 4), dim3(256), 0, s, N, p, st, Sm, Lb);
  }
  hipLaunchKernelGGL(k_lc4_cap_back, dim3(1), dim3(LC4_BACK_THREADS), 0, s, N, st, Lb, Dinv, v, w);
}

namespace {

bool options_ok(const gfbe_lc4_options *opt, gfbe_lc4_options *o) {
  gfbe_lc4_default_options(o);
  if (!opt) return true;
  if (opt->struct_size != (int32_t)sizeof(gfbe_lc4_options)) return false;
  *o = *opt;
  return o->span >= 1 && o->span <= LC4_MAX_SPAN && o->max_num_iterations >= 0 && o->huber_delta > 0.0 && o->loop_yaw_div > 0.0;
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

gfbe_status gfbe_lc4_eval(gfbe_ctx *c, const gfbe_lc4_options *opt, int32_t n, const double *t, const double *ypr, int32_t n_edges, const int32_t *edge_i,
                          const int32_t *edge_j, const uint8_t *kind, const double *meas, double *r_out, double *J_out, double *cost) {
  gfbe_lc4_options o;
  if (!c) return GFBE_BAD_INPUT;
  if (!options_ok(opt, &o)) { ctx_set_error(c, "gfbe_lc4_eval: gfbe_lc4_options of another size or out of range (ABI mismatch)"); return GFBE_BAD_INPUT; }
  if (n < 1 || n_edges < 0 || !t || !ypr || (n_edges && (!edge_i || !edge_j || !kind || !meas))) return GFBE_BAD_INPUT;
  for (int e = 0; e < n_edges; e++)
    if (edge_i[e] < 0 || edge_i[e] >= n || edge_j[e] < 0 || edge_j[e] >= n || edge_i[e] == edge_j[e] || kind[e] > 1) {
      ctx_set_error(c, "gfbe_lc4_eval: an edge joins two distinct poses in range, kind 0 or 1");
      return GFBE_BAD_INPUT;
    }
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_lc4_eval: no device (no CPU fallback)"); return GFBE_NO_DEVICE; }
  hipStream_t s = ctx_stream(c);
  Lc4Buffers buf(c);
  double *dt, *dy, *dm, *dr, *dJ, *dc, *hr = nullptr, *hJ = nullptr;
  int *di, *dj;
  unsigned char *dk;
  for (int pass = 0; pass < 2; pass++) {
    dt = buf.dev<double>((size_t)3 * n, t); dy = buf.dev<double>((size_t)3 * n, ypr);
    di = buf.dev<int>(n_edges, edge_i); dj = buf.dev<int>(n_edges, edge_j); dk = buf.dev<unsigned char>(n_edges, kind);
    dm = buf.dev<double>((size_t)6 * n_edges, meas);
    dr = buf.dev<double>((size_t)4 * n_edges); dJ = buf.dev<double>((size_t)32 * n_edges); dc = buf.dev<double>(n_edges);
    hr = buf.pinned<double>((size_t)4 * n_edges); hJ = buf.pinned<double>((size_t)32 * n_edges);
    if (pass == 0 && !buf.commit(0)) { ctx_set_error(c, "gfbe_lc4_eval: device allocation failed"); return GFBE_DEVICE_ERROR; }
  }
  double *res = (double *)buf.result();
  if (n_edges) hipLaunchKernelGGL(k_lc4_eval, dim3((n_edges + 127) / 128), dim3(128), 0, s, n_edges, dt, dy, di, dj, dk, dm, o.huber_delta, o.loop_yaw_div, dr, dJ, dc);
  hipLaunchKernelGGL(k_lc4_sum, dim3(1), dim3(LCD_THREADS), 0, s, dc, n_edges, res);
  if (n_edges && r_out) (void)hipMemcpyAsync(hr, dr, sizeof(double) * 4 * n_edges, hipMemcpyDeviceToHost, s);
  if (n_edges && J_out) (void)hipMemcpyAsync(hJ, dJ, sizeof(double) * 32 * n_edges, hipMemcpyDeviceToHost, s);
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) { ctx_set_error(c, "gfbe_lc4_eval: device error"); return GFBE_DEVICE_ERROR; }
  if (n_edges && r_out) std::memcpy(r_out, hr, sizeof(double) * 4 * n_edges);
  if (n_edges && J_out) std::memcpy(J_out, hJ, sizeof(double) * 32 * n_edges);
  if (cost) *cost = res[0];
  return GFBE_OK;
}

}  // extern "C"

namespace {

// The body of gfbe_lc4_solve (max_loops = LC4_MAX_LOOPS) and gfbe_lc4_solve_long (LC4_LONG_MAX_LOOPS): one graph construction, one
// pass structure. Up to LC4_MAX_LOOPS loop edges the capacitance system is k_lc4_cap's, beyond it the blocked kernels'.
gfbe_status lc4_solve_body(const char *name, const char *limit_name, int max_loops, gfbe_ctx *c, const gfbe_lc4_options *opt, int32_t n, const double *t, const double *ypr,
                           const int32_t *sequence, const uint8_t *fixed, int32_t n_loop, const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out,
                           double *yaw_out, double *drift, gfbe_summary *S_out) {
  gfbe_lc4_options o;
  if (!c) return GFBE_BAD_INPUT;
  const std::string who(name);
  if (!options_ok(opt, &o)) { ctx_set_error(c, (who + ": gfbe_lc4_options of another size or out of range (ABI mismatch)").c_str()); return GFBE_BAD_INPUT; }
  if (n < 1 || !t || !ypr || !sequence || !fixed || !t_out || !yaw_out || n_loop < 0 || (n_loop && (!loop_i || !loop_c || !loop_meas))) return GFBE_BAD_INPUT;
  Lc4Plan plan;
  size_t off_v = 0;
  const bool blocked = n_loop > LC4_MAX_LOOPS;
  std::vector<uint8_t> has_loop(n);
  const int bad = lc4_check_graph_within(n, n_loop, max_loops, loop_i, loop_c, o.span, has_loop.data());
  bool planned = false;
  if (!bad && blocked) {
    Lc4LongPlan lp;
    planned = lc4_long_plan(n, n_loop, &lp);
    if (planned) { plan = lp.p; off_v = lp.off_v; }
  } else if (!bad) {
    planned = lc4_plan(n, n_loop, &plan);
  }
  if (bad || !planned) {
    ctx_set_error(c, (bad == 2 ? who + ": more than " + limit_name + " loop edges" : who + ": loop edges need 0 <= loop_c < loop_i < n, one per loop_i").c_str());
    return GFBE_BAD_INPUT;
  }
  if (ctx_device(c) < 0) { ctx_set_error(c, (who + ": no device (no CPU fallback)").c_str()); return GFBE_NO_DEVICE; }
  const int max_it = std::min(o.max_num_iterations, 15);
  // the graph: sequence edges with their measurements (formed from the input poses), the loop edges that are kept, who is in the problem
  std::vector<unsigned char> emask(n, 0), free_(n, 0), loop_on(std::max(n_loop, 1), 0);
  std::vector<double> meas((size_t)24 * n, 0.0), lmeas((size_t)6 * std::max(n_loop, 1), 0.0);
  for (int i = 0; i < n; i++)
    for (int k = 1; k <= o.span; k++)
      if (i - k >= 0 && sequence[i] == sequence[i - k] && !(fixed[i] && fixed[i - k])) {
        emask[i] |= (unsigned char)(1 << (k - 1));
        lc4_sequence_meas(t + 3 * (size_t)(i - k), ypr + 3 * (size_t)(i - k), t + 3 * (size_t)i, ypr + 3 * (size_t)i, &meas[((size_t)i * 4 + (k - 1)) * 6]);
        free_[i] = free_[i - k] = 1;
      }
  std::vector<int> lp_begin(n + 1, 0), lp_entry;
  for (int l = 0; l < n_loop; l++) {
    loop_on[l] = !(fixed[loop_c[l]] && fixed[loop_i[l]]);
    for (int q = 0; q < 4; q++) lmeas[6 * (size_t)l + q] = loop_meas[4 * (size_t)l + q];
    lmeas[6 * (size_t)l + 4] = ypr[3 * (size_t)loop_c[l] + 1]; lmeas[6 * (size_t)l + 5] = ypr[3 * (size_t)loop_c[l] + 2];
    if (loop_on[l]) { free_[loop_c[l]] = free_[loop_i[l]] = 1; lp_begin[loop_c[l] + 1]++; lp_begin[loop_i[l] + 1]++; }
  }
  for (int i = 0; i < n; i++) { lp_begin[i + 1] += lp_begin[i]; if (fixed[i]) free_[i] = 0; }
  lp_entry.assign(std::max(lp_begin[n], 1), 0);
  {
    std::vector<int> fill(lp_begin.begin(), lp_begin.end() - 1);
    for (int l = 0; l < n_loop; l++)
      if (loop_on[l]) { lp_entry[fill[loop_c[l]]++] = 2 * l; lp_entry[fill[loop_i[l]]++] = 2 * l + 1; }
  }
  std::vector<double> x0((size_t)4 * n);
  double xn2 = 0.0;
  for (int i = 0; i < n; i++) {
    x0[4 * (size_t)i] = ypr[3 * (size_t)i];
    for (int k = 0; k < 3; k++) x0[4 * (size_t)i + 1 + k] = t[3 * (size_t)i + k];
    if (free_[i]) for (int k = 0; k < 4; k++) xn2 += x0[4 * (size_t)i + k] * x0[4 * (size_t)i + k];
  }
  const double x_norm0 = std::sqrt(xn2);

  hipStream_t s = ctx_stream(c);
  static_assert(sizeof(Lc4State) <= LC4_RESULT_BYTES, "the pinned result slot holds the loop's state");
  Lc4Buffers buf(c);
  Lc4Dev P;
  Lc4Sets S;
  Lc4Red Q;
  const int M = plan.M, rows = plan.rows, L = n_loop;
  double *cost_i, *cost_l, *gabs, *model_r, *step2_i, *xn2_i, *scale, *g0, *diag0, *diag2, *gs, *Bs, *As, *Cs, *Us, *big, *xo;
  Lc4State *dst;
  int *fail;
  size_t small_bytes = 0;
  for (int pass = 0; pass < 2; pass++) {
    dst = (Lc4State *)buf.dev<double>((sizeof(Lc4State) + 7) / 8);      // (cleared: cur = lb = 0, done = 0, ...)
    fail = buf.dev<int>(1);
    small_bytes = buf.used;
    P = {n, M, rows, L, plan.ld, plan.ntile, plan.cap_ld, buf.dev<unsigned char>(n, free_.data()), buf.dev<unsigned char>(n, emask.data()),
         buf.dev<double>((size_t)24 * n, meas.data()), buf.dev<int>(L, loop_c), buf.dev<int>(L, loop_i), buf.dev<double>((size_t)6 * L, lmeas.data()),
         buf.dev<unsigned char>(L, loop_on.data()), buf.dev<int>(n + 1, lp_begin.data()), buf.dev<int>(lp_entry.size(), lp_entry.data()), o.huber_delta, o.loop_yaw_div};
    S.x[0] = buf.dev<double>((size_t)4 * n, x0.data()); S.x[1] = buf.dev<double>((size_t)4 * n);
    for (int q = 0; q < 2; q++) {
      S.Hb[q] = buf.dev<double>((size_t)256 * M); S.Ha[q] = buf.dev<double>((size_t)256 * M); S.Hc[q] = buf.dev<double>((size_t)256 * M); S.g[q] = buf.dev<double>(rows);
      S.Uv[q] = buf.dev<double>((size_t)32 * L); S.gl[q] = buf.dev<double>((size_t)8 * L); S.dl[q] = buf.dev<double>((size_t)8 * L);
    }
    cost_i = buf.dev<double>(n); cost_l = buf.dev<double>(L); gabs = buf.dev<double>(rows); model_r = buf.dev<double>((size_t)rows + L);
    step2_i = buf.dev<double>(n); xn2_i = buf.dev<double>(n);
    scale = buf.dev<double>(rows); g0 = buf.dev<double>(rows); diag0 = buf.dev<double>(rows); diag2 = buf.dev<double>(rows); gs = buf.dev<double>(rows);
    Bs = buf.dev<double>((size_t)256 * M); As = buf.dev<double>((size_t)256 * M); Cs = buf.dev<double>((size_t)256 * M); Us = buf.dev<double>((size_t)32 * L);
    big = buf.dev<double>(plan.total);      // the plan's carve: panels, band sets, multipliers, capacitance, step
    xo = buf.pinned<double>((size_t)4 * n);
    if (pass == 0 && !buf.commit(small_bytes)) { ctx_set_error(c, (who + ": device allocation failed").c_str()); return GFBE_DEVICE_ERROR; }
  }
  Q = {cost_i, cost_l, gabs, model_r, step2_i, xn2_i};
  double *panel[2] = {big + plan.off_panel[0], big + plan.off_panel[1]};
  double *band[2][4];
  for (int q = 0; q < 2; q++) for (int k = 0; k < 4; k++) band[q][k] = big + plan.off_band[q][k];
  double *alpha = big + plan.off_alpha, *gamma = big + plan.off_gamma, *Sm = big + plan.off_S, *Lb = big + plan.off_L, *Dinv = big + plan.off_Dinv,
         *w = big + plan.off_w, *y = big + plan.off_y, *vcap = big + off_v;      // (vcap: the blocked path only)
  const dim3 gr((rows + 255) / 256), b256(256);
  auto lin = [&](int cand) {
    hipLaunchKernelGGL(k_lc4_lin, gr, b256, 0, s, P, dst, S, cand, cost_i);
    if (L) hipLaunchKernelGGL(k_lc4_lin_loops, dim3((L + 63) / 64), dim3(64), 0, s, P, dst, S, cand, cost_l);
  };
  auto decide = [&](int mode) { hipLaunchKernelGGL(k_lc4_decide, dim3(1), dim3(LCD_THREADS), 0, s, P, Q, dst, fail, mode, x_norm0); };
  lin(0);
  decide(0);
  const dim3 gp(M, (plan.ntile + 3) / 4);
  const int fill_blocks = (int)std::min<size_t>(((size_t)rows * plan.ld + 255) / 256, 4096);
  const int gather_blocks = (int)std::min<size_t>(((size_t)plan.cap_ld * (plan.cap_ld + 1) + 255) / 256, LC4_GATHER_BLOCKS);
  // max_it passes, enqueued blindly: every kernel of a pass returns at once when the loop has ended
  for (int pass = 0; pass < max_it; pass++) {
    hipLaunchKernelGGL(k_lc4_scale, gr, b256, 0, s, P, dst, S, scale, g0, diag0, gabs);
    hipLaunchKernelGGL(k_lc4_system, gr, b256, 0, s, P, dst, S, scale, g0, diag0, diag2, gs, Bs, As, Cs, band[0][1], band[0][0], band[0][2]);
    hipLaunchKernelGGL(k_lc4_panel_fill, dim3(fill_blocks), b256, 0, s, rows, plan.ld, dst, gs, panel[0]);
    if (L) hipLaunchKernelGGL(k_lc4_loop_cols, dim3((32 * L + 255) / 256), b256, 0, s, P, dst, S, scale, Us, panel[0]);
    hipLaunchKernelGGL(k_lc4_inv0, dim3(M), dim3(64), 0, s, M, dst, band[0][1], band[0][3], fail);
    int cur = 0;
    for (int sw = 0, stride = 1; sw < plan.sweeps; sw++, stride *= 2) {
      hipLaunchKernelGGL(k_lc4_pcr_blocks, dim3(M), dim3(64), 0, s, M, stride, dst, band[cur][0], band[cur][1], band[cur][2], band[cur][3], band[1 - cur][0], band[1 - cur][1],
                         band[1 - cur][2], band[1 - cur][3], alpha, gamma, fail);
      hipLaunchKernelGGL(k_lc4_pcr_panel, gp, b256, 0, s, M, stride, plan.ld, plan.ntile, dst, alpha, gamma, panel[cur], panel[1 - cur]);
      cur = 1 - cur;
    }
    double *Z = panel[1 - cur];
    hipLaunchKernelGGL(k_lc4_final, gp, b256, 0, s, plan.ld, plan.ntile, dst, band[cur][3], panel[cur], Z);
    if (L && !blocked) hipLaunchKernelGGL(k_lc4_cap, dim3(1), b256, 0, s, P, dst, Us, Z, Sm, Lb, Dinv, w, fail);
    if (blocked) {      // 2 + 2 cap_nt - 1 launches
      hipLaunchKernelGGL(k_lc4_cap_gather, dim3(gather_blocks), b256, 0, s, P, dst, Us, Z, Sm, vcap);
      launch_lc4_cap_factor(plan.cap_ld, dst, Sm, Lb, Dinv, vcap, w, fail, s);
    }
    hipLaunchKernelGGL(k_lc4_apply, gr, b256, 0, s, rows, plan.ld, 4 * L, dst, Z, w, y);
    hipLaunchKernelGGL(k_lc4_candidate, dim3((rows + L + 255) / 256), b256, 0, s, P, dst, S, Bs, As, Cs, gs, Us, y, scale, model_r, step2_i, xn2_i);
    decide(1);
    lin(1);      // the candidate's cost — and its linearisation, should it be accepted
    decide(2);
  }
  Lc4State *hst = (Lc4State *)buf.result();
  hipLaunchKernelGGL(k_lc4_finish, dim3(std::min(256, (4 * n + 255) / 256)), b256, 0, s, n, dst, S, xo, hst);
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) { ctx_set_error(c, (who + ": device error").c_str()); return GFBE_DEVICE_ERROR; }
  for (int i = 0; i < n; i++) {
    yaw_out[i] = xo[4 * (size_t)i];
    for (int k = 0; k < 3; k++) t_out[3 * (size_t)i + k] = xo[4 * (size_t)i + 1 + k];
  }
  if (drift) {      // pose_graph.cpp:674-681: yaw_drift, t_drift = cur_t - Rz(yaw_drift) vio_t of the last keyframe
    const double yd = yaw_out[n - 1] - ypr[3 * (size_t)(n - 1)], a = yd / 180.0 * M_PI, *v = t + 3 * (size_t)(n - 1), *u = t_out + 3 * (size_t)(n - 1);
    drift[0] = yd;
    drift[1] = u[0] - (std::cos(a) * v[0] - std::sin(a) * v[1]);
    drift[2] = u[1] - (std::sin(a) * v[0] + std::cos(a) * v[1]);
    drift[3] = u[2] - v[2];
  }
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

gfbe_status gfbe_lc4_solve(gfbe_ctx *c, const gfbe_lc4_options *opt, int32_t n, const double *t, const double *ypr, const int32_t *sequence, const uint8_t *fixed,
                           int32_t n_loop, const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out, double *yaw_out, double *drift,
                           gfbe_summary *S_out) {
  return lc4_solve_body("gfbe_lc4_solve", "GFBE_LC4_MAX_LOOPS", LC4_MAX_LOOPS, c, opt, n, t, ypr, sequence, fixed, n_loop, loop_i, loop_c, loop_meas, t_out, yaw_out, drift, S_out);
}

gfbe_status gfbe_lc4_solve_long(gfbe_ctx *c, const gfbe_lc4_options *opt, int32_t n, const double *t, const double *ypr, const int32_t *sequence, const uint8_t *fixed,
                                int32_t n_loop, const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out, double *yaw_out, double *drift,
                                gfbe_summary *S_out) {
  return lc4_solve_body("gfbe_lc4_solve_long", "GFBE_LC4_LONG_MAX_LOOPS", LC4_LONG_MAX_LOOPS, c, opt, n, t, ypr, sequence, fixed, n_loop, loop_i, loop_c, loop_meas, t_out, yaw_out,
                        drift, S_out);
}

}  // extern "C"
