// tests/pnp_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_pnp.h for a sanitizer run
// (-fsanitize=address,undefined; never on code loaded into Python): planted problems of 26, 64, 65 and 300 points with outliers, a problem
// at and below min_loop_num, one hypothesis, no refinement, every point the same, points on one line, zero, huge, infinite and NaN inputs,
// and a singular 6 x 6 system. Every array is allocated at its exact size, so a read or write outside it stops the program. Prints "ok".
#include <stdio.h>

#include <limits>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_pnp.h"

using namespace gfd;

namespace {
uint64_t g_state = 12345;
double uni() {      // [0, 1)
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) / 9007199254740992.0;
}
struct Problem {
  std::vector<float> p3, pn;
  double pose_cur[12], tic_qic[12];
};
// points in front of a camera at a fixed pose, the first n_in observed exactly, the rest far off
Problem planted(int n, int n_in) {
  Problem P;
  const double R[9] = {0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6}, t[3] = {0.3, -0.2, 0.5};      // Xc = R Xw + t
  for (int i = 0; i < n; i++) {
    const double z = 2.0 + 6.0 * uni(), xc[3] = {(uni() - 0.5) * z, (uni() - 0.5) * z, z};
    float X[3];
    for (int a = 0; a < 3; a++) X[a] = (float)(R[a] * (xc[0] - t[0]) + R[3 + a] * (xc[1] - t[1]) + R[6 + a] * (xc[2] - t[2]));
    const double pose[12] = {t[0], t[1], t[2], R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]};
    double c[3];
    pnp_transform(pose, X[0], X[1], X[2], c);
    const double off = i < n_in ? 0.0 : 0.2 + 0.2 * uni();
    for (int a = 0; a < 3; a++) P.p3.push_back(X[a]);
    P.pn.push_back((float)(c[0] / c[2] + off)); P.pn.push_back((float)(c[1] / c[2] - off));
  }
  const double pc[12] = {0.1, 0.2, 0.3, 1, 0, 0, 0, 1, 0, 0, 0, 1}, tq[12] = {0.05, -0.02, 0.1, 0, 0, 1, -1, 0, 0, 0, -1, 0};
  for (int a = 0; a < 12; a++) { P.pose_cur[a] = pc[a]; P.tic_qic[a] = tq[a]; }
  return P;
}
PnpHostOut run(const Problem &P, int iterations, int refine, bool diag) {
  PnpParams Q;
  Q.iterations = iterations; Q.refine_iterations = refine; Q.min_loop_num = 25; Q.pad = 0; Q.seed = 7; Q.thr2 = (10.0 / 460.0) * (10.0 / 460.0);
  const int n = (int)(P.p3.size() / 3);
  const size_t H = (size_t)iterations;
  std::vector<uint8_t> status((size_t)n);
  std::vector<int32_t> si(3 * H), ns(H), hc(4 * H);
  std::vector<double> hp(48 * H);
  return pnp_host_problem(Q, 30.0, 20.0, n, P.p3.data(), P.pn.data(), P.pose_cur, P.tic_qic, status.data(), diag ? si.data() : nullptr, diag ? ns.data() : nullptr,
                          diag ? hp.data() : nullptr, diag ? hc.data() : nullptr);
}
}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (int n : {26, 64, 65, 300}) {
    const Problem P = planted(n, n - n / 3);
    const PnpHostOut r = run(P, 100, 5, true);
    if (r.n_inliers != n - n / 3 || r.best_h < 0 || r.refine_flag != 0) return 1;
    if (run(P, 1, 0, false).best_h > 0) return 2;
    if (run(P, 1024, 20, true).n_inliers != r.n_inliers) return 3;
  }
  for (int n : {0, 1, 25}) {
    const PnpHostOut r = run(planted(n, n), 100, 5, true);
    if (r.n_inliers != 0 || r.has_loop != 0 || r.best_h != -1) return 4;
  }
  {
    Problem P = planted(40, 40);      // every point the same: every sample is degenerate
    for (int i = 1; i < 40; i++) for (int a = 0; a < 3; a++) P.p3[3 * (size_t)i + (size_t)a] = P.p3[(size_t)a];
    if (run(P, 100, 5, true).best_h != -1) return 5;
    Problem L = planted(40, 40);      // points on one line
    for (int i = 0; i < 40; i++) { L.p3[3 * (size_t)i] = (float)i; L.p3[3 * (size_t)i + 1] = 2.f * (float)i; L.p3[3 * (size_t)i + 2] = 1.f; }
    if (run(L, 100, 5, true).best_h != -1) return 6;
  }
  for (float v : {0.f, 1e30f, -1e30f, inf, -inf, nan}) {
    Problem P = planted(60, 40);
    for (size_t k = 0; k < P.p3.size(); k += 7) P.p3[k] = v;
    for (size_t k = 0; k < P.pn.size(); k += 5) P.pn[k] = v;
    (void)run(P, 100, 5, true);
    for (auto &x : P.p3) x = v;
    for (auto &x : P.pn) x = v;
    (void)run(P, 50, 3, false);
  }
  // a singular system: the pivot rule
  double acc[27] = {}, d[6];
  if (pnp_solve6(acc, d)) return 7;
  for (int a = 0; a < 6; a++) acc[a * 6 - a * (a - 1) / 2] = 1.0;
  for (int a = 0; a < 6; a++) acc[21 + a] = -(double)(a + 1);
  if (!pnp_solve6(acc, d)) return 8;
  for (int a = 0; a < 6; a++) if (d[a] != (double)(a + 1)) return 9;
  acc[20] = -1.0;
  if (pnp_solve6(acc, d)) return 10;
  int idx[3];
  if (pnp_sample(1, 0, 2, idx) != 2 || idx[2] != -1 || pnp_sample(1, 0, 1, idx) != 1) return 11;
  printf("ok\n");
  return 0;
}
