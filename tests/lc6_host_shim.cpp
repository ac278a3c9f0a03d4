// TEST INFRASTRUCTURE. The HIP-free half of the 6-DoF loop-closure pose graph (ground-fusion2_amd/csrc/gfbe_loopgraph6.h: the factor
// with its analytic Jacobian, the corrector, the sequence measurement, Plus, the plan, the graph check) behind a C interface for
// tests/test_lc6_host.py. Built by a plain C++ compiler: the header has no HIP in it.
#include "../ground-fusion2_amd/csrc/gfbe_loopgraph6.h"

using namespace gfd;

extern "C" {

// r [n][6], J [n][6][12], cost_e [n] of an explicit edge list; poses as t [.][3], q [.][4] (w, x, y, z)
void shim_lc6_eval(int n_edges, const double *t, const double *q, const int *ei, const int *ej, const unsigned char *kind, const double *meas, double delta, double t_var,
                   double q_var, double *r, double *J, double *cost_e) {
  for (int e = 0; e < n_edges; e++)
    cost_e[e] = lc6_edge(kind[e], q + 4 * ei[e], t + 3 * ei[e], q + 4 * ej[e], t + 3 * ej[e], meas + 7 * e, delta, t_var, q_var, r + 6 * e, J + 72 * e);
}

void shim_lc6_sequence_meas(const double *ta, const double *qa, const double *tb, const double *qb, double *meas) { lc6_sequence_meas(ta, qa, tb, qb, meas); }

void shim_lc6_plus(const double *q, const double *d, double *out) { lc6_plus(q, d, out); }

// out: M rows pad_poses sweeps ncol ld ntile cap cap_ld, then total and whether every carved array lies inside the slab
int shim_lc6_plan(int n, int n_loop, long long *out) {
  Lc6Plan p;
  if (!lc6_plan(n, n_loop, &p)) return 0;
  const long long v[9] = {p.M, p.rows, p.pad_poses, p.sweeps, p.ncol, p.ld, p.ntile, p.cap, p.cap_ld};
  for (int q = 0; q < 9; q++) out[q] = v[q];
  out[9] = (long long)p.total;
  // every carved array ends inside the slab and starts on a 256-byte boundary, in the order of the struct
  const size_t blk = (size_t)p.M * 1024;
  const size_t offs[] = {p.off_panel[0], p.off_panel[1], p.off_band[0][0], p.off_band[0][1], p.off_band[0][2], p.off_band[0][3], p.off_band[1][0], p.off_band[1][1],
                         p.off_band[1][2], p.off_band[1][3], p.off_alpha, p.off_gamma, p.off_S, p.off_L, p.off_Dinv, p.off_w, p.off_y, p.off_v, p.total};
  const size_t need[] = {(size_t)p.rows * p.ld, (size_t)p.rows * p.ld, blk, blk, blk, blk, blk, blk, blk, blk, blk, blk, (size_t)p.cap_ld * p.cap_ld,
                         (size_t)p.cap_ld * p.cap_ld, (size_t)p.cap_ld * 16, (size_t)p.cap_ld, (size_t)p.rows, (size_t)p.cap_ld};
  int ok = 1;
  for (int q = 0; q < 18; q++) ok = ok && offs[q] % 32 == 0 && offs[q] + need[q] <= offs[q + 1];
  out[10] = ok;
  return 1;
}

int shim_lc6_check_graph(int n, int n_loop, const int32_t *loop_i, const int32_t *loop_c, int span, unsigned char *scratch) {
  return lc6_check_graph(n, n_loop, loop_i, loop_c, span, scratch);
}

int shim_lc6_all_finite(const double *p, long long count) { return lc6_all_finite(p, (size_t)count) ? 1 : 0; }

// the graph of a solve as lc_build_graph makes it: emask [n], free_ [n], loop_on [max(n_loop, 1)], lp_begin [n + 1], lp_entry [2 n_loop]
// (returns how many of its entries are used), meas [n][4][7]; poses as t [.][3], q [.][4]
int shim_lc6_graph(int n, int span, const double *t, const double *q, const int32_t *sequence, const unsigned char *fixed, int n_loop, const int32_t *loop_i,
                   const int32_t *loop_c, unsigned char *emask, unsigned char *free_, unsigned char *loop_on, int *lp_begin, int *lp_entry, double *meas) {
  LcGraph g;
  lc_build_graph(n, span, 7, sequence, fixed, n_loop, loop_i, loop_c, [&](int lo, int hi, double *m) { lc6_sequence_meas(t + 3 * lo, q + 4 * lo, t + 3 * hi, q + 4 * hi, m); }, &g);
  for (int i = 0; i < n; i++) { emask[i] = g.emask[i]; free_[i] = g.free_[i]; }
  for (int l = 0; l < n_loop; l++) loop_on[l] = g.loop_on[l];
  for (int i = 0; i <= n; i++) lp_begin[i] = g.lp_begin[i];
  for (int e = 0; e < g.lp_begin[n]; e++) lp_entry[e] = g.lp_entry[e];
  for (size_t k = 0; k < g.meas.size(); k++) meas[k] = g.meas[k];
  return g.lp_begin[n];
}

}  // extern "C"
