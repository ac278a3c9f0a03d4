// tests/lc4_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_loopgraph.h for a sanitizer run
// (-fsanitize=address,undefined; never on code loaded into Python): plans of every small size, graph checks with bad input, and the
// factor on a grid of yaw differences across the +-180 wrap. Prints "ok".
#include <stdio.h>

#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_loopgraph.h"

using namespace gfd;

int main() {
  for (int n = 1; n <= 300; n++)
    for (int L = 0; L <= LC4_MAX_LOOPS; L += (n % 7 == 0 ? 1 : 16)) {
      Lc4Plan p;
      if (!lc4_plan(n, L, &p)) return 1;
      if (p.rows != 16 * p.M || 4 * p.M - n != p.pad_poses || p.pad_poses < 0 || p.pad_poses > 3 || p.ld < p.ncol || p.ld % 16) return 2;
      if (((size_t)1 << p.sweeps) < (size_t)p.M || (p.sweeps && ((size_t)1 << (p.sweeps - 1)) >= (size_t)p.M)) return 3;
      if (p.off_y + (size_t)p.rows > p.total) return 4;
    }
  Lc4Plan p;
  if (lc4_plan(0, 0, &p) || lc4_plan(4, -1, &p) || lc4_plan(4, LC4_MAX_LOOPS + 1, &p)) return 5;
  std::vector<uint8_t> scratch(8);
  const int32_t li[3] = {3, 5, 7}, lc[3] = {0, 2, 6}, dup[2] = {3, 3}, dc[2] = {0, 1}, back[1] = {2}, bc[1] = {2}, far[1] = {8}, fc[1] = {0};
  if (lc4_check_graph(8, 3, li, lc, 4, scratch.data()) != 0) return 6;
  if (lc4_check_graph(8, 2, dup, dc, 4, scratch.data()) != 6 || lc4_check_graph(8, 1, back, bc, 4, scratch.data()) != 5 ||
      lc4_check_graph(8, 1, far, fc, 4, scratch.data()) != 4 || lc4_check_graph(8, 1, li, lc, 5, scratch.data()) != 3)
    return 7;
  double acc = 0.0;
  for (int k = -40; k <= 40; k++) {
    const double yi = 170.0 + k * 0.5, yj = -175.0 + k * 0.25, ti[3] = {1.0, 2.0, 3.0}, tj[3] = {1.5, 1.0, 3.2}, meas[6] = {0.4, -0.9, 0.2, 14.0, 3.0, -2.0};
    double r[4], J[32];
    acc += lc4_edge(k & 1, yi, ti, yj, tj, meas, 0.1, 10.0, r, J) + r[3] + J[0];
    double m6[6];
    const double ya[3] = {yi, 3.0, -2.0}, yb[3] = {yj, 1.0, 1.0};
    lc4_sequence_meas(ti, ya, tj, yb, m6);
    acc += m6[3];
  }
  if (!(acc == acc)) return 8;
  printf("ok\n");
  return 0;
}
