// tests/eq_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_eq.h for a sanitizer run
// (-fsanitize=address,undefined; never on code loaded into Python): the largest legal padding (9 x 9 with 8 x 8 tiles, 65 x 65 with
// 64 x 64), a 2 x 2 image of one tile, both dimensions padded, a divisible dimension padded by a whole `tiles`, a clip_limit of 0, a
// tiny one and the largest finite double, in place and out of place. Every plane and LUT is allocated at its exact size, so a read or
// write outside it stops the program. Prints "ok".
#include <stdio.h>

#include <limits>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_eq.h"

using namespace gfd;

int main() {
  const double big = std::numeric_limits<double>::max(), inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  if (!eq_geom_error(8, 9, 8, 8, 40.0) || !eq_geom_error(9, 8, 8, 8, 40.0) || !eq_geom_error(9, 9, 0, 8, 40.0) || !eq_geom_error(9, 9, 8, 65, 40.0) || !eq_geom_error(16385, 9, 8, 8, 40.0) ||
      !eq_geom_error(9, 9, 8, 8, -1.0) || !eq_geom_error(9, 9, 8, 8, inf) || !eq_geom_error(9, 9, 8, 8, nan) || eq_geom_error(9, 9, 8, 8, big) || eq_geom_error(9, 9, 8, 8, 0.0))
    return 1;
  const struct { int rows, cols, tx, ty; double clip; } cases[] = {{9, 9, 8, 8, 40.0},  {2, 2, 1, 1, 40.0},   {17, 23, 8, 8, 40.0}, {24, 20, 8, 8, 40.0},  {65, 65, 64, 64, 40.0}, {128, 65, 64, 64, 1e-9},
                                                                  {61, 97, 1, 1, 3.0}, {61, 97, 8, 8, 0.0},  {33, 47, 5, 3, big},  {16, 16, 8, 8, 40.0},  {120, 188, 8, 8, 2.0}};
  for (const auto &k : cases) {
    if (eq_geom_error(k.rows, k.cols, k.tx, k.ty, k.clip)) return 2;
    const EqGeom g = eq_geom(k.rows, k.cols, k.tx, k.ty, k.clip);
    if (g.tw * k.tx < k.cols || g.th * k.ty < k.rows || g.tw * k.tx > k.cols + k.tx || g.th * k.ty > k.rows + k.ty) return 3;
    const size_t px = (size_t)k.rows * (size_t)k.cols, nl = (size_t)k.tx * (size_t)k.ty * EQ_BINS;
    for (int kind = 0; kind < 3; kind++) {
      std::vector<uint8_t> img(px), out(px), lut(nl);
      for (size_t p = 0; p < px; p++) img[p] = kind == 0 ? (uint8_t)((p * 2654435761u) >> 24) : kind == 1 ? (uint8_t)(p % 64 + 90) : (uint8_t)255;
      eq_host_lut(img.data(), g, lut.data());
      for (size_t t = 0; t < nl / EQ_BINS; t++) {
        if (lut[t * EQ_BINS + 255] != 255) return 4;
        for (int i = 1; i < EQ_BINS; i++)
          if (lut[t * EQ_BINS + (size_t)i] < lut[t * EQ_BINS + (size_t)i - 1]) return 5;
      }
      eq_host_apply(img.data(), g, lut.data(), out.data());
      eq_host_apply(img.data(), g, lut.data(), img.data());      // E6
      for (size_t p = 0; p < px; p++)
        if (img[p] != out[p]) return 6;
    }
  }
  printf("ok\n");
  return 0;
}
