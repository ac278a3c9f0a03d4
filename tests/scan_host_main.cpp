// tests/scan_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_scan.h for a sanitizer run
// (-fsanitize=address,undefined): the segment search and the interpolation on arrays of exactly the stated sizes, at the edges of the
// time rule (one state, stamps in front of / behind / equal to the state times, a zero-length segment, NaN). Prints "ok".
#include <cmath>
#include <cstdio>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_scan.h"

using namespace gfd;

int main() {
  int bad = 0;
  for (int n : {1, 2, 3, 21, 512}) {
    std::vector<double> t((size_t)n), pose(7 * (size_t)n);
    for (int k = 0; k < n; k++) {
      t[k] = 5.0 + 0.01 * k;
      const double th = 0.01 * k;
      const double q[7] = {0.1 * k, -0.05 * k, 0.02 * k, std::sin(th / 2), 0.0, 0.0, std::cos(th / 2)};
      for (int a = 0; a < 7; a++) pose[7 * (size_t)k + a] = q[a];
    }
    if (n >= 3) t[2] = t[1];      // a zero-length segment
    std::vector<double> stamps = {t[0] - 1.0, t[0], t[n - 1], t[n - 1] + 0.1, t[n - 1] + 9.0, t[n / 2], std::nextafter(t[n / 2], 1e9), std::nan("")};
    for (double q : stamps) {
      int seg = -7;
      double Ti[7], out[3];
      const double p[3] = {1.0, -2.0, 0.5};
      scan_pose_at(n, t.data(), pose.data(), q, &seg, Ti);
      scan_undistort_point(pose.data() + 7 * (size_t)(n - 1), Ti, p, out);
      if (seg < -1 || seg > n - 2) bad++;
      if (seg != scan_segment(n, t.data(), q)) bad++;
      if (q == q && !(std::isfinite(out[0]) && std::isfinite(out[1]) && std::isfinite(out[2]))) bad++;
    }
  }
  std::printf(bad ? "bad %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
