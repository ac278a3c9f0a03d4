// TEST INFRASTRUCTURE. The plan and the graph check of gfbe_lc4_solve_long (ground-fusion2_amd/csrc/gfbe_loopgraph.h: lc4_long_plan,
// lc4_long_check_graph) behind a C interface for tests/test_lc4_long_host.py. Built by a plain C++ compiler: the header has no HIP in it.
#include "../ground-fusion2_amd/csrc/gfbe_loopgraph.h"

using namespace gfd;

extern "C" {

int shim_lc4_long_max_loops() { return LC4_LONG_MAX_LOOPS; }

// out: M rows pad_poses sweeps ncol ld ntile cap cap_ld, then total and whether every carved array starts on a 256-byte boundary, in the
// order of the struct, and ends before the next one (the last inside total)
int shim_lc4_long_plan(int n, int n_loop, long long *out) {
  Lc4LongPlan lp;
  if (!lc4_long_plan(n, n_loop, &lp)) return 0;
  const Lc4Plan &p = lp.p;
  const long long v[9] = {p.M, p.rows, p.pad_poses, p.sweeps, p.ncol, p.ld, p.ntile, p.cap, p.cap_ld};
  for (int q = 0; q < 9; q++) out[q] = v[q];
  out[9] = (long long)p.total;
  const size_t blk = (size_t)p.M * 256, pan = (size_t)p.rows * p.ld, sq = (size_t)p.cap_ld * p.cap_ld;
  const size_t offs[] = {p.off_panel[0], p.off_panel[1], p.off_band[0][0], p.off_band[0][1], p.off_band[0][2], p.off_band[0][3], p.off_band[1][0], p.off_band[1][1],
                         p.off_band[1][2], p.off_band[1][3], p.off_alpha, p.off_gamma, p.off_S, p.off_L, p.off_Dinv, p.off_w, p.off_y, lp.off_v, p.total};
  const size_t need[] = {pan, pan, blk, blk, blk, blk, blk, blk, blk, blk, blk, blk, sq, sq, (size_t)(p.cap_ld / 16) * 256 /* the pivot tiles' inverses */, (size_t)p.cap_ld,
                         (size_t)p.rows, (size_t)p.cap_ld /* v */};
  int ok = 1;
  for (int q = 0; q < 18; q++) ok = ok && offs[q] % 32 == 0 && offs[q] + need[q] <= offs[q + 1];
  out[10] = ok;
  return 1;
}

int shim_lc4_long_check_graph(int n, int n_loop, const int32_t *loop_i, const int32_t *loop_c, int span, unsigned char *scratch) {
  return lc4_long_check_graph(n, n_loop, loop_i, loop_c, span, scratch);
}

}  // extern "C"
