// TEST INFRASTRUCTURE. The HIP-free half of the loop-closure pose graph (ground-fusion2_amd/csrc/gfbe_loopgraph.h: the factor with its
// analytic Jacobian, the corrector, the sequence measurement, the plan, the graph check) behind a C interface for
// tests/test_lc4_host.py. Built by a plain C++ compiler: the header has no HIP in it.
#include "../ground-fusion2_amd/csrc/gfbe_loopgraph.h"

using namespace gfd;

extern "C" {

double shim_lc4_normalize_angle(double a) { return lc4_normalize_angle(a); }

// r [n][4], J [n][4][8], cost_e [n] of an explicit edge list; poses as t [.][3], ypr [.][3]
void shim_lc4_eval(int n_edges, const double *t, const double *ypr, const int *ei, const int *ej, const unsigned char *kind, const double *meas, double delta,
                   double yaw_div, double *r, double *J, double *cost_e) {
  for (int e = 0; e < n_edges; e++)
    cost_e[e] = lc4_edge(kind[e], ypr[3 * ei[e]], t + 3 * ei[e], ypr[3 * ej[e]], t + 3 * ej[e], meas + 6 * e, delta, yaw_div, r + 4 * e, J + 32 * e);
}

void shim_lc4_sequence_meas(const double *ta, const double *ypr_a, const double *tb, const double *ypr_b, double *meas) { lc4_sequence_meas(ta, ypr_a, tb, ypr_b, meas); }

// out: M rows pad_poses sweeps ncol ld ntile cap cap_ld, then total and the largest end of any carved array (doubles)
int shim_lc4_plan(int n, int n_loop, long long *out) {
  Lc4Plan p;
  if (!lc4_plan(n, n_loop, &p)) return 0;
  const long long v[9] = {p.M, p.rows, p.pad_poses, p.sweeps, p.ncol, p.ld, p.ntile, p.cap, p.cap_ld};
  for (int q = 0; q < 9; q++) out[q] = v[q];
  out[9] = (long long)p.total;
  // every carved array ends inside the slab and starts on a 256-byte boundary, in the order of the struct
  const size_t offs[] = {p.off_panel[0], p.off_panel[1], p.off_band[0][0], p.off_band[0][1], p.off_band[0][2], p.off_band[0][3], p.off_band[1][0], p.off_band[1][1],
                         p.off_band[1][2], p.off_band[1][3], p.off_alpha, p.off_gamma, p.off_S, p.off_L, p.off_Dinv, p.off_w, p.off_y, p.total};
  const size_t need[] = {(size_t)p.rows * p.ld, (size_t)p.rows * p.ld, (size_t)p.M * 256, (size_t)p.M * 256, (size_t)p.M * 256, (size_t)p.M * 256, (size_t)p.M * 256,
                         (size_t)p.M * 256, (size_t)p.M * 256, (size_t)p.M * 256, (size_t)p.M * 256, (size_t)p.M * 256, (size_t)p.cap_ld * p.cap_ld,
                         (size_t)p.cap_ld * p.cap_ld, (size_t)p.cap_ld * 16, (size_t)p.cap_ld, (size_t)p.rows};
  int ok = 1;
  for (int q = 0; q < 17; q++) ok = ok && offs[q] % 32 == 0 && offs[q] + need[q] <= offs[q + 1];
  out[10] = ok;
  return 1;
}

int shim_lc4_check_graph(int n, int n_loop, const int32_t *loop_i, const int32_t *loop_c, int span, unsigned char *scratch) {
  return lc4_check_graph(n, n_loop, loop_i, loop_c, span, scratch);
}

// the graph of a solve as lc_build_graph makes it: emask [n], free_ [n], loop_on [max(n_loop, 1)], lp_begin [n + 1], lp_entry [2 n_loop]
// (returns how many of its entries are used), meas [n][4][6]; poses as t [.][3], ypr [.][3]
int shim_lc4_graph(int n, int span, const double *t, const double *ypr, const int32_t *sequence, const unsigned char *fixed, int n_loop, const int32_t *loop_i,
                   const int32_t *loop_c, unsigned char *emask, unsigned char *free_, unsigned char *loop_on, int *lp_begin, int *lp_entry, double *meas) {
  LcGraph g;
  lc_build_graph(n, span, 6, sequence, fixed, n_loop, loop_i, loop_c, [&](int lo, int hi, double *m) { lc4_sequence_meas(t + 3 * lo, ypr + 3 * lo, t + 3 * hi, ypr + 3 * hi, m); }, &g);
  for (int i = 0; i < n; i++) { emask[i] = g.emask[i]; free_[i] = g.free_[i]; }
  for (int l = 0; l < n_loop; l++) loop_on[l] = g.loop_on[l];
  for (int i = 0; i <= n; i++) lp_begin[i] = g.lp_begin[i];
  for (int e = 0; e < g.lp_begin[n]; e++) lp_entry[e] = g.lp_entry[e];
  for (size_t k = 0; k < g.meas.size(); k++) meas[k] = g.meas[k];
  return g.lp_begin[n];
}

}  // extern "C"
