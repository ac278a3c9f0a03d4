// tests/dmap_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_dmap.h for a sanitizer run
// (-fsanitize=address,undefined): world point, gate, key, packing round trip, squared distance and the coarse cell on arrays of
// exactly the stated sizes, at the edges of the key range (the box's first and last voxel, one float outside, NaN, infinity). Prints "ok".
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_dmap.h"

using namespace gfd;

int main() {
  int bad = 0;
  const double origin = -10000.0, res = 0.01;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float edge[] = {-10000.0f, std::nextafterf(-10000.0f, -inf), 10971.5f, 10971.52f, 10972.0f, 0.0f, -0.0f, 3e38f, -3e38f, inf, -inf, nan};
  for (float e : edge) {
    const std::vector<float> p = {e, 0.015f, -0.015f};
    uint64_t k = 0;
    int x, y, z;
    const bool ok = dmap_key(p.data(), origin, res, &k);
    const bool inside = (double)e >= -10000.0 && (double)e < 10971.52;      // (10971.52f is the float below 10971.52: the last voxel)
    if (ok != inside) bad++;
    if (ok) {
      dmap_unpack(k, &x, &y, &z);
      if (dmap_pack(x, y, z) != k || k == ~0ull || x < 0 || x >= (1 << DM_KEY_BITS)) bad++;
    }
  }
  if (dmap_pack((1 << DM_KEY_BITS) - 1, (1 << DM_KEY_BITS) - 1, (1 << DM_KEY_BITS) - 1) != 0x7FFFFFFFFFFFFFFFull) bad++;
  // world points of a list of exactly n points under a pose, the gate and the coarse cell of the in-box ones
  const double pose[7] = {1.0, -2.0, 0.5, 0.0, 0.0, std::sin(0.2), std::cos(0.2)}, ex[7] = {0.08, 0.02, 0.25, -0.5, 0.5, -0.5, 0.5};
  double RP[12], RPic[12];
  dmap_pose_rp(pose, RP);
  dmap_pose_rp(ex, RPic);
  for (int n : {1, 7, 256}) {
    std::vector<float> pts(3 * (size_t)n), pf(3 * (size_t)n);
    for (int i = 0; i < 3 * n; i++) pts[(size_t)i] = 0.37f * (float)(i % 17) - 2.0f;
    const double side = dmap_cell_side(0.8);
    if (!(side * std::sqrt(3.0) <= 0.8) || !(2.0 * side >= 0.8) || !dmap_cells_fit(origin, res, 0.8) || dmap_cells_fit(origin, res, 0.01)) bad++;
    for (int i = 0; i < n; i++) {
      double pw[3];
      dmap_world(RP, RPic, pts.data() + 3 * (size_t)i, pw);
      for (int a = 0; a < 3; a++) pf[3 * (size_t)i + a] = (float)pw[a];
      (void)dmap_gated(pw[2], -0.5, 2.0);
      int c[3];
      dmap_cell(pf.data() + 3 * (size_t)i, side, c);
      for (int a = 0; a < 3; a++) if (c[a] < 2 || c[a] > (1 << DM_KEY_BITS) - 3) bad++;
      if (dmap_sqdist(pf.data() + 3 * (size_t)i, pf.data()) < 0.0) bad++;
    }
  }
  if (!dmap_gated(std::nextafter(2.0, 3.0), -0.5, 2.0) || dmap_gated(2.0, -0.5, 2.0) || dmap_gated(-0.5, -0.5, 2.0) || dmap_gated(std::nan(""), -0.5, 2.0)) bad++;
  std::printf(bad ? "bad %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
