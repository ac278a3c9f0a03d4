// tests/det_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_det.h for a sanitizer run
// (-fsanitize=address,undefined; never on code loaded into Python): discs over every edge and corner at several radii, points far
// outside the image, huge and non-finite points, empty lists, a worst-case candidate list (a periodic image, every candidate walked at
// min_dist 0 and 1), the overflow rule and max_corners of 1. Every read lies inside its buffer or the address sanitizer stops the
// program. Prints "ok".
#include <stdio.h>

#include <limits>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_det.h"

using namespace gfd;

static std::vector<uint8_t> image(int cols, int rows, int kind) {
  std::vector<uint8_t> im((size_t)cols * (size_t)rows);
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const double v = 128.0 + 50.0 * sin(0.21 * x + 0.13 * y) + 40.0 * sin(0.08 * x - 0.17 * y + 1.0) + 30.0 * sin(0.5 * y + 0.4 * x);
      im[(size_t)y * (size_t)cols + (size_t)x] = kind == 0 ? (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)) : (kind == 1 ? (uint8_t)((((x / 2) + (y / 2)) % 2) * 140 + 50) : (uint8_t)77);
    }
  return im;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  // the order of the keys: the response first, then the index; the bits come back
  if (!(det_key(1.f, 5) > det_key(0.5f, 900)) || !(det_key(0.5f, 6) > det_key(0.5f, 5)) || !(det_key(1e-30f, 0) > det_key(-1e-30f, 7)) || !(det_key(-1.f, 0) < det_key(-0.5f, 0))) return 1;
  for (float v : {0.f, 1e-38f, 3.5f, -2.25f, 1e30f}) if (det_key_response(det_key(v, 3)) != v || det_key_index(det_key(v, 123456)) != 123456) return 2;
  if (!(det_mask_key(5, 1) < det_mask_key(4, 0)) || !(det_mask_key(5, 1) < det_mask_key(5, 2)) || !(det_mask_key(0, 0) < det_mask_key(-1, 0))) return 3;
  const int sizes[4][2] = {{23, 23}, {64, 48}, {91, 89}, {180, 177}};
  for (const auto &s : sizes) {
    const int cols = s[0], rows = s[1];
    for (int kind = 0; kind < 3; kind++) {
      const std::vector<uint8_t> im = image(cols, rows, kind);
      std::vector<float> pts;
      const float xs[7] = {-40.f, -0.5f, 0.f, cols * 0.5f, cols - 1.f, cols - 0.5f, cols + 60.f}, ys[7] = {-40.f, -0.5f, 0.f, rows * 0.5f, rows - 1.f, rows - 0.5f, rows + 60.f};
      for (float x : xs) for (float y : ys) { pts.push_back(x); pts.push_back(y); }
      const float wild[6][2] = {{1e30f, 5.f}, {-1e30f, 5.f}, {5.f, 3e9f}, {inf, 2.f}, {3.f, -inf}, {nan, nan}};
      for (const auto &w : wild) { pts.push_back(w[0]); pts.push_back(w[1]); }
      const int n = (int)pts.size() / 2;
      std::vector<int32_t> ids((size_t)n), cnt((size_t)n);
      for (int i = 0; i < n; i++) { ids[(size_t)i] = 100 + i; cnt[(size_t)i] = 1 + (i * 7) % 5; }
      for (int min_dist : {0, 1, 2, 3, 5, 10, 30, 500}) {
        const int max_cnt = 2 * n;
        std::vector<float> po(2 * (size_t)max_cnt);
        std::vector<int32_t> io((size_t)max_cnt), co((size_t)max_cnt);
        int32_t counters[6], next_id = 40;
        const int m = det_host_detect(im.data(), cols, rows, n, pts.data(), ids.data(), cnt.data(), max_cnt, min_dist, 0.01, 0, &next_id, po.data(), io.data(), co.data(), counters);
        if (m != counters[1] + counters[3] || counters[0] != n || counters[4] != 40 + counters[3] || m > max_cnt || counters[5] != 0) return 4;
        for (int i = 1; i < counters[1]; i++) if (co[(size_t)i] > co[(size_t)i - 1]) return 5;      // the kept points descend in track_cnt
        for (int i = counters[1]; i < m; i++) if (co[(size_t)i] != 1 || io[(size_t)i] != 40 + i - counters[1]) return 6;
        if (kind == 2 && counters[3] != 0) return 7;      // a flat image has no corner
        // the planes with the kept discs over every edge
        std::vector<int> order((size_t)n), kxy(2 * (size_t)n);
        const int kept = det_host_mask(n, pts.data(), cnt.data(), cols, rows, min_dist, order.data(), kxy.data());
        if (kept != counters[1]) return 8;
        std::vector<float> eig((size_t)cols * (size_t)rows);
        std::vector<uint8_t> mask((size_t)cols * (size_t)rows);
        det_host_planes(im.data(), cols, rows, kept, kxy.data(), min_dist, eig.data(), mask.data());
        for (int k = 0; k < kept; k++) if (mask[(size_t)kxy[2 * (size_t)k + 1] * (size_t)cols + (size_t)kxy[2 * (size_t)k]] != 0) return 9;
      }
      // empty lists; the overflow rule; a single corner
      int32_t counters[6], next_id = 0;
      std::vector<float> po(2 * 64);
      std::vector<int32_t> io(64), co(64);
      if (det_host_detect(im.data(), cols, rows, 0, nullptr, nullptr, nullptr, 64, 5, 0.01, 0, &next_id, po.data(), io.data(), co.data(), counters) != counters[3]) return 10;
      next_id = 0;
      if (counters[2] > 1 && (det_host_detect(im.data(), cols, rows, 0, nullptr, nullptr, nullptr, 64, 5, 0.01, 1, &next_id, po.data(), io.data(), co.data(), counters) != 0 ||
                              counters[5] != 1 || next_id != 0))
        return 11;
      float one[2], resp[1];
      int n_cand = -1;
      if (det_host_corners(im.data(), cols, rows, 1, 0.01, 10, 0, one, resp, &n_cand) > 1 || n_cand < 0) return 12;
      // the worst case: every candidate of the image accepted (min_dist 0 and 1 reject nothing)
      for (int min_dist : {0, 1}) {
        const int room = cols * rows;
        std::vector<float> p(2 * (size_t)room), r((size_t)room);
        const int got = det_host_corners(im.data(), cols, rows, room, 0.0, min_dist, 0, p.data(), r.data(), &n_cand);
        if (got != n_cand) return 13;
        for (int i = 1; i < got; i++) if (r[(size_t)i] > r[(size_t)i - 1]) return 14;
      }
    }
  }
  printf("ok\n");
  return 0;
}
