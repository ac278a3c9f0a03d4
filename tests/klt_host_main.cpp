// tests/klt_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_klt.h for a sanitizer run
// (-fsanitize=address,undefined; never on code loaded into Python): pyramids of the smallest and of odd sizes, the tracker on points
// whose windows hang over every edge, start outside the image or leave it, on a flat and on a saturated patch, non-finite and huge
// coordinates through cvFloor / cvRound, and the tracking half with and without a prediction. Every read of a window lies inside the
// padded level or the address sanitizer stops the program. Prints "ok".
#include <stdio.h>

#include <limits>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_klt.h"

using namespace gfd;

static std::vector<uint8_t> image(int cols, int rows, int shift) {
  std::vector<uint8_t> im((size_t)cols * (size_t)rows);
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const double v = 128.0 + 50.0 * sin(0.21 * (x + shift) + 0.13 * y) + 40.0 * sin(0.08 * (x + shift) - 0.17 * y + 1.0) + 30.0 * sin(0.5 * y + 0.4 * (x + shift));
      im[(size_t)y * (size_t)cols + (size_t)x] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  for (int y = 0; y < rows / 3; y++)      // a flat and a saturated block
    for (int x = 0; x < cols / 3; x++) { im[(size_t)y * (size_t)cols + (size_t)x] = 90; im[(size_t)(rows - 1 - y) * (size_t)cols + (size_t)(cols - 1 - x)] = 255; }
  return im;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  if (klt_floor(inf) != (1 << 30) || klt_floor(-inf) != -(1 << 30) || klt_floor(nan) != -(1 << 30) || klt_round(3e38f) != (1 << 30) || klt_round(-3e38f) != -(1 << 30)) return 1;
  if (klt_round(0.5f) != 0 || klt_round(1.5f) != 2 || klt_round(2.5f) != 2 || klt_floor(-0.5f) != -1) return 2;
  const int sizes[5][3] = {{23, 23, 1}, {64, 48, 2}, {91, 89, 3}, {180, 177, 4}, {22, 400, 1}};
  for (const auto &s : sizes) {
    const int cols = s[0], rows = s[1];
    const std::vector<uint8_t> a = image(cols, rows, 0), b = image(cols, rows, 2);
    KltHostPyramid A, B;
    klt_host_build(a.data(), cols, rows, 3, &A);
    klt_host_build(b.data(), cols, rows, 3, &B);
    if (A.view.n_levels != s[2]) return 3;
    std::vector<float> pts;
    const float xs[9] = {-40.f, -11.5f, 0.f, 3.25f, cols * 0.5f, cols - 4.5f, cols - 1.f, cols + 9.75f, cols + 60.f};
    const float ys[9] = {-40.f, -11.5f, 0.f, 3.25f, rows * 0.5f, rows - 4.5f, rows - 1.f, rows + 9.75f, rows + 60.f};
    for (float x : xs) for (float y : ys) { pts.push_back(x); pts.push_back(y); }
    const float wild[4][2] = {{1e30f, 5.f}, {-1e30f, 5.f}, {5.f, 3e9f}, {cols * 0.25f, rows * 0.25f}};
    for (const auto &w : wild) { pts.push_back(w[0]); pts.push_back(w[1]); }
    const int n = (int)pts.size() / 2;
    std::vector<uint8_t> st((size_t)n);
    std::vector<float> err((size_t)n), next(pts);
    std::vector<int> trace((size_t)n * KLT_MAX_LEVELS);
    for (int ml = 0; ml <= 3; ml++)
      for (int init = 0; init < 2; init++) {
        next = pts;
        if (init) for (float &v : next) v += 3.5f;
        klt_host_flow(A.view, B.view, n, pts.data(), next.data(), st.data(), err.data(), ml, init, klt_params(30, 0.01, 1e-4), trace.data());
        klt_host_flow(B.view, A.view, n, pts.data(), next.data(), st.data(), err.data(), ml, 1, klt_params(200, -1.0, 1e-4), nullptr);
      }
    std::vector<int32_t> ids((size_t)n), cnt((size_t)n, 1), ido((size_t)n), cno((size_t)n);
    for (int i = 0; i < n; i++) ids[(size_t)i] = 100 + i;
    std::vector<float> po(2 * (size_t)n), co(2 * (size_t)n), pred(pts);
    for (float &v : pred) v -= 2.f;
    int32_t counters[4];
    const KltTrackOptions O{3, 1, 1, 250, 10, 0.5};
    for (int hp = 0; hp < 2; hp++) {
      const int m = klt_host_track(A.view, B.view, n, pts.data(), ids.data(), cnt.data(), hp, pred.data(), O, klt_params(30, 0.01, 1e-4), po.data(), co.data(), ido.data(),
                                   cno.data(), counters);
      if (m != counters[3] || counters[0] != n || counters[1] < counters[2] || counters[2] < m) return 4;
      for (int i = 0; i < m; i++) if (cno[(size_t)i] != 2 || (i && ido[(size_t)i] <= ido[(size_t)i - 1])) return 5;
    }
    if (klt_host_track(A.view, B.view, 0, nullptr, nullptr, nullptr, 0, nullptr, O, klt_params(30, 0.01, 1e-4), nullptr, nullptr, nullptr, nullptr, counters) != 0) return 6;
  }
  const int32_t off[3] = {0, 2, 3}, bad_off[3] = {0, 4, 3}, big[3] = {0, 3, 3};
  const float p[6] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f}, q[6] = {1.f, 2.f, nan, 4.f, 5.f, 6.f};
  if (klt_check_points(2, off, 2, p) != KLT_C_OK || klt_check_points(2, bad_off, 8, p) != KLT_C_COUNT || klt_check_points(2, big, 2, p) != KLT_C_COUNT ||
      klt_check_points(2, off, 2, q) != KLT_C_FINITE || klt_check_points(2, off, 2, nullptr) != KLT_C_COUNT)
    return 7;
  printf("ok\n");
  return 0;
}
