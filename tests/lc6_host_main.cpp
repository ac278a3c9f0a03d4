// tests/lc6_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_loopgraph6.h for a sanitizer run
// (-fsanitize=address,undefined; never on code loaded into Python): plans of every small size, graph checks with bad input, and the
// factor, the sequence measurement and Plus on a grid of rotations that passes through error quaternions with w < 0. Prints "ok".
#include <stdio.h>

#include <limits>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_loopgraph6.h"

using namespace gfd;

int main() {
  for (int n = 1; n <= 300; n++)
    for (int L = 0; L <= LC6_MAX_LOOPS; L += (n % 7 == 0 ? 1 : 16)) {
      Lc6Plan p;
      if (!lc6_plan(n, L, &p)) return 1;
      if (p.rows != 32 * p.M || 4 * p.M - n != p.pad_poses || p.pad_poses < 0 || p.pad_poses > 3 || p.ld < p.ncol || p.ld % 16) return 2;
      if (((size_t)1 << p.sweeps) < (size_t)p.M || (p.sweeps && ((size_t)1 << (p.sweeps - 1)) >= (size_t)p.M)) return 3;
      if (p.off_y + (size_t)p.rows > p.total || p.cap_ld < p.cap || p.cap_ld % 16 || p.cap_ld > 768) return 4;
    }
  Lc6Plan p;
  if (lc6_plan(0, 0, &p) || lc6_plan(4, -1, &p) || lc6_plan(4, LC6_MAX_LOOPS + 1, &p)) return 5;
  std::vector<uint8_t> scratch(8);
  const int32_t li[3] = {3, 5, 7}, lc[3] = {0, 2, 6}, dup[2] = {3, 3}, dc[2] = {0, 1}, back[1] = {2}, bc[1] = {2}, far[1] = {8}, fc[1] = {0};
  if (lc6_check_graph(8, 3, li, lc, 4, scratch.data()) != 0) return 6;
  if (lc6_check_graph(8, 2, dup, dc, 4, scratch.data()) != 6 || lc6_check_graph(8, 1, back, bc, 4, scratch.data()) != 5 ||
      lc6_check_graph(8, 1, far, fc, 4, scratch.data()) != 4 || lc6_check_graph(8, 1, li, lc, 5, scratch.data()) != 3)
    return 7;
  const double fin[3] = {1.0, -2.0, 0.0}, inf[3] = {1.0, std::numeric_limits<double>::infinity(), 0.0}, nan[2] = {std::numeric_limits<double>::quiet_NaN(), 0.0};
  if (!lc6_all_finite(fin, 3) || lc6_all_finite(inf, 3) || lc6_all_finite(nan, 2) || !lc6_all_finite(fin, 0)) return 8;
  double acc = 0.0;
  const double id[4] = {1.0, 0.0, 0.0, 0.0};
  for (int k = -40; k <= 40; k++) {
    const double di[3] = {0.05 * k, 0.3, -0.2}, dj[3] = {-0.04 * k, 0.1 * k, 0.7}, ti[3] = {1.0, 2.0, 3.0}, tj[3] = {1.5, 1.0, 3.2}, dm[3] = {0.0, 0.0, 0.1 * k};
    double qi[4], qj[4], meas[7] = {0.4, -0.9, 0.2, 0, 0, 0, 0}, r[6], J[72], m7[7];
    lc6_plus(id, di, qi);
    lc6_plus(id, dj, qj);
    lc6_plus(id, dm, meas + 3);
    acc += lc6_edge(k & 1, qi, ti, qj, tj, meas, 0.1, 0.1, 0.01, r, J) + r[3] + J[0] + J[71];
    acc += lc6_edge(k & 1, qi, ti, qj, tj, meas, 0.1, 0.1, 0.01, r, nullptr);
    lc6_sequence_meas(ti, qi, tj, qj, m7);
    acc += m7[0] + m7[6];
  }
  const double zero[3] = {0.0, 0.0, 0.0}, q0[4] = {0.5, -0.5, 0.5, 0.5};
  double out[4];
  lc6_plus(q0, zero, out);
  for (int k = 0; k < 4; k++)
    if (out[k] != q0[k]) return 9;
  if (!(acc == acc)) return 10;
  printf("ok\n");
  return 0;
}
