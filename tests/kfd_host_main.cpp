// tests/kfd_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_kfd.h for a sanitizer run
// (-fsanitize=address,undefined; never on code loaded into Python): 7 x 7 images (the single legal centre pixel, the blur's reflection at
// its widest), a 64 x 48 image with corners on the first and last row and column that have a ring, BRIEF points on and beyond every
// edge, the -0.5 case, huge and non-finite coordinates, pattern offsets at both ends of -64 .. 64, a capacity below the corner count.
// Every plane is allocated at its exact size, so a read or write outside it stops the program. Prints "ok".
#include <stdio.h>

#include <limits>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_kfd.h"

using namespace gfd;

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  int tap_sum = 0;
  for (int k = 0; k < 9; k++) tap_sum += kfd_tap(k);
  if (tap_sum != 256) return 1;
  // the pattern: both ends of the range and the packing's signs
  std::vector<int32_t> pattern(4 * KFD_PAIRS);
  for (int i = 0; i < 4 * KFD_PAIRS; i++) pattern[(size_t)i] = (i * 37) % 129 - 64;
  pattern[0] = -64; pattern[1] = 64; pattern[KFD_PAIRS] = 64; pattern[2 * KFD_PAIRS + 1] = -64;
  if (!kfd_pattern_ok(pattern.data())) return 2;
  uint32_t pairs[KFD_PAIRS];
  kfd_pack_pattern(pattern.data(), pairs);
  for (int i = 0; i < KFD_PAIRS; i++)
    for (int f = 0; f < 4; f++)
      if (kfd_pair_field(pairs[i], f) != pattern[(size_t)(f * KFD_PAIRS + i)]) return 3;
  pattern[7] = 65;
  if (kfd_pattern_ok(pattern.data())) return 4;
  pattern[7] = 0;
  const double cam[8] = {605.687407, 607.16452123, 323.35155412, 236.66167004, 0.15860811, -0.34018021, -0.00180768, 0.00032313};
  const int sizes[3][2] = {{7, 7}, {48, 64}, {61, 97}};
  for (const auto &sz : sizes) {
    const int rows = sz[0], cols = sz[1];
    const size_t px = (size_t)rows * (size_t)cols;
    std::vector<uint8_t> img(px, 100), blur(px), plane(px);
    // isolated bright pixels on every pixel of the first and last row and column that have a ring (7 x 7: the centre alone)
    const int xs[3] = {3, cols / 2, cols - 4}, ys[3] = {3, rows / 2, rows - 4};
    for (int y : ys) for (int x : xs) img[(size_t)y * (size_t)cols + (size_t)x] = (uint8_t)(180 + (x + y) % 60);
    kfd_host_blur(img.data(), rows, cols, blur.data());
    if (kfd_blur_pixel(img.data(), rows, cols, 0, 0) != blur[0] || kfd_blur_pixel(img.data(), rows, cols, cols - 1, rows - 1) != blur[px - 1]) return 5;
    for (int cap : {1, 4, 4096}) {
      std::vector<float> pts(2 * (size_t)cap), ptsn(2 * (size_t)cap);
      std::vector<int32_t> score((size_t)cap);
      std::vector<uint64_t> desc(4 * (size_t)cap);
      int32_t cn[4];
      kfd_host_fast(img.data(), rows, cols, 20, cap, plane.data(), pts.data(), score.data(), cn);
      const int want = rows == 7 ? 1 : 9;
      if (cn[1] != want || cn[2] != (want < cap ? want : cap) || cn[3] != (want > cap ? 1 : 0)) return 6;
      if (kfd_host_brief(blur.data(), rows, cols, pairs, cn[2], pts.data(), desc.data()) != 0) return 7;
      kfd_host_norm(cam, cn[2], pts.data(), ptsn.data());
    }
    // every pixel scored directly, the frame included
    for (int y = 0; y < rows; y++)
      for (int x = 0; x < cols; x++)
        if ((kfd_fast_score(img.data(), cols, rows, cols, x, y, 20) > 0) != (img[(size_t)y * (size_t)cols + (size_t)x] != 100)) return 8;
    // window points on and beyond every edge
    const float r = (float)rows, c = (float)cols;
    const float w[][2] = {{-0.5f, -0.5f}, {-0.5f, 3.f}, {3.f, -0.5f}, {-1.f, -1.f}, {0.f, 0.f}, {c - 1.f, r - 1.f}, {c - 0.5f, r - 0.5f}, {c, r}, {c + 64.f, r + 64.f}, {-64.f, -64.f},
                          {-65.f, 3.f}, {1e30f, 5.f}, {-1e30f, 5.f}, {5.f, 3e9f}, {inf, 2.f}, {3.f, -inf}, {nan, nan}, {1048576.f, 1.f}, {1048575.f, 1.f}, {-1048575.f, -1048575.f},
                          {c / 2.f, r / 2.f}, {2147483648.f, 0.f}};
    const int n = (int)(sizeof w / sizeof w[0]);
    std::vector<uint64_t> wd(4 * (size_t)n);
    const int bad = kfd_host_brief(blur.data(), rows, cols, pairs, n, &w[0][0], wd.data());
    if (bad != 8) return 9;      // six wild points, 2^20 and 2^31
    if (kfd_brief_coord(-0.5f, 0) != 0 || kfd_brief_coord(-1.5f, 1) != 0 || kfd_brief_coord(-1.5f, 0) != -1 || kfd_brief_coord(2.75f, -3) != 0) return 10;
    for (int j = 11; j < 18; j++)
      for (int q = 0; q < 4; q++)
        if (wd[4 * (size_t)j + (size_t)q] != 0) return 11;
  }
  printf("ok\n");
  return 0;
}
