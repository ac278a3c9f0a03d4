// tests/lc4_long_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_loopgraph.h for a sanitizer run
// (-fsanitize=address,undefined; never on code loaded into Python): the plan of gfbe_lc4_solve_long at small sizes, at the sizes the
// blocked path is timed at and at the cap (where rows x ld passes 2^25), and its graph check at the limit. Prints "ok".
#include <stdio.h>

#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_loopgraph.h"

using namespace gfd;

static int check_plan(int n, int L) {
  Lc4LongPlan lp;
  Lc4Plan s;
  if (!lc4_long_plan(n, L, &lp)) return 1;
  const Lc4Plan &p = lp.p;
  if (p.rows != 16 * p.M || 4 * p.M - n != p.pad_poses || p.pad_poses < 0 || p.pad_poses > 3 || p.ld < p.ncol || p.ld % 16 || p.ld - p.ncol >= 16) return 2;
  if (((size_t)1 << p.sweeps) < (size_t)p.M || (p.sweeps && ((size_t)1 << (p.sweeps - 1)) >= (size_t)p.M)) return 3;
  if (p.cap != 4 * L || p.cap_ld % 16 || p.cap_ld < (L ? p.cap : 16) || p.cap_ld >= (L ? p.cap : 1) + 16) return 4;
  if (p.off_panel[1] - p.off_panel[0] < (size_t)p.rows * (size_t)p.ld || p.off_L - p.off_S < (size_t)p.cap_ld * (size_t)p.cap_ld) return 5;
  if (lp.off_v < p.off_y + (size_t)p.rows || lp.off_v + (size_t)p.cap_ld > p.total || lp.off_v % 32) return 6;
  // up to LC4_MAX_LOOPS the short plan is the same carve (the blocked path's vector comes behind it)
  if (L <= LC4_MAX_LOOPS && (!lc4_plan(n, L, &s) || s.total != lp.off_v || s.off_y != p.off_y || s.ld != p.ld || s.cap_ld != p.cap_ld)) return 7;
  if (L > LC4_MAX_LOOPS && lc4_plan(n, L, &s)) return 8;
  return 0;
}

int main() {
  for (int n = 1; n <= 300; n++)
    for (int L = 0; L <= LC4_LONG_MAX_LOOPS; L += (n % 37 == 0 ? 1 : 61))
      if (int rc = check_plan(n, L)) return rc;
  const int big[][2] = {{700, 512}, {1000, 65}, {1000, 512}, {5000, 65}, {5000, 256}, {5000, 512}, {5001, 511}};
  for (const auto &b : big)
    if (int rc = check_plan(b[0], b[1])) return 10 + rc;
  Lc4LongPlan lp;
  if (!lc4_long_plan(5000, 512, &lp) || lp.p.rows != 20000 || lp.p.ld != 2064 || lp.p.cap_ld != 2048 || lp.p.total * sizeof(double) < (size_t)700 << 20 ||
      lp.p.total * sizeof(double) > (size_t)800 << 20)
    return 20;      // the 0.75 GB of include/gfbe.h
  if (lc4_long_plan(0, 0, &lp) || lc4_long_plan(4, -1, &lp) || lc4_long_plan(4, LC4_LONG_MAX_LOOPS + 1, &lp)) return 21;
  const int n = 2 * LC4_LONG_MAX_LOOPS + 8;
  std::vector<uint8_t> scratch(n);
  std::vector<int32_t> li, lc;
  for (int l = 0; l <= LC4_LONG_MAX_LOOPS; l++) { li.push_back(2 * l + 1); lc.push_back(l); }
  if (lc4_long_check_graph(n, LC4_MAX_LOOPS + 1, li.data(), lc.data(), 4, scratch.data()) != 0) return 22;
  if (lc4_long_check_graph(n, LC4_LONG_MAX_LOOPS, li.data(), lc.data(), 4, scratch.data()) != 0) return 23;
  if (lc4_long_check_graph(n, LC4_LONG_MAX_LOOPS + 1, li.data(), lc.data(), 4, scratch.data()) != 2) return 24;
  if (lc4_check_graph(n, LC4_MAX_LOOPS + 1, li.data(), lc.data(), 4, scratch.data()) != 2) return 25;
  li[300] = li[299];
  if (lc4_long_check_graph(n, LC4_LONG_MAX_LOOPS, li.data(), lc.data(), 4, scratch.data()) != 6) return 26;
  li[300] = 601; lc[300] = 601;
  if (lc4_long_check_graph(n, LC4_LONG_MAX_LOOPS, li.data(), lc.data(), 4, scratch.data()) != 5) return 27;
  lc[300] = n;
  if (lc4_long_check_graph(n, LC4_LONG_MAX_LOOPS, li.data(), lc.data(), 4, scratch.data()) != 4) return 28;
  printf("ok\n");
  return 0;
}
