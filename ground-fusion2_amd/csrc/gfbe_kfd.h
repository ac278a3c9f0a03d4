// gfbe_kfd.h — the rules of the keyframe descriptors (gfbe_kfd.hip) that need no HIP header: under a plain C++ compiler they are ordinary
// inline functions, under hipcc the per-pixel and per-point ones are __host__ __device__ (tests/kfd_host_shim.cpp compiles them for the
// host). The rules K1 .. K6 are stated in include/gfbe_kfd.h; citations are to
//
//   DVision::BRIEF::compute                                       dense_map/src/ThirdParty/DVision/BRIEF.cpp:39-106
//   KeyFrame::computeWindowBRIEFPoint, computeBRIEFPoint          dense_map/src/keyframe.cpp:148-191
//
// K1 and K2 are exact integer arithmetic, K4 one float addition and a conversion toward zero, K5 is obs_lift of gfbe_obs.h. The model
// tests/kfd_np.py reproduces every function bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gfbe_obs.h"

#define GF_KFD_HD GF_KLT_HD

namespace gfd {

constexpr int KFD_MIN_SIZE = 7;           // rows and cols: the FAST ring needs a 7 x 7 image
constexpr int KFD_PAIRS = 256;            // bits of a descriptor, GFBE_LDB_DESC_WORDS * 64
constexpr int KFD_MAX_OFFSET = 64;        // |x1|, |y1|, |x2|, |y2| of the pattern
constexpr int KFD_BLUR_R = 4;             // the blur is 9 x 9
constexpr int KFD_FAST_R = 3;             // the radius of the ring

// ---- K1 ---------------------------------------------------------------------------------------------------------------------------
// exp(-x^2 / 8) for x = -4 .. 4, normalised and rounded to 8 fractional bits: the taps sum to 256
GF_KFD_HD int kfd_tap(int k) {
  return k == 0 || k == 8 ? 7 : k == 1 || k == 7 ? 17 : k == 2 || k == 6 ? 32 : k == 3 || k == 5 ? 46 : 52;
}
// the horizontal sum at (x, y) of an unpadded plane, at most 255 * 256 = 65 280
GF_KFD_HD int kfd_blur_row(const uint8_t *row, int cols, int x) {
  int s = 0;
  for (int k = 0; k < 9; k++) s += kfd_tap(k) * (int)row[klt_reflect101(x + k - KFD_BLUR_R, cols)];
  return s;
}
// the vertical pass over nine horizontal sums and the rounding: below 2^24 before the shift
GF_KFD_HD int kfd_blur_round(int sum) { return (sum + 32768) >> 16; }
GF_KFD_HD int kfd_blur_pixel(const uint8_t *img, int rows, int cols, int x, int y) {
  int s = 0;
  for (int k = 0; k < 9; k++) s += kfd_tap(k) * kfd_blur_row(img + (size_t)klt_reflect101(y + k - KFD_BLUR_R, rows) * (size_t)cols, cols, x);
  return kfd_blur_round(s);
}

// ---- K2 ---------------------------------------------------------------------------------------------------------------------------
// ring pixel k of the radius-3 Bresenham circle, from (0, 3) on
GF_KFD_HD int kfd_ring_dx(int k) {
  const int d = k & 7, a = d == 0 ? 0 : d == 1 ? 1 : d == 2 ? 2 : d <= 5 ? 3 : d == 6 ? 2 : 1;
  return k < 8 ? a : -a;
}
GF_KFD_HD int kfd_ring_dy(int k) {
  const int d = k & 7, a = d == 0 || d == 1 ? 3 : d == 2 ? 2 : d == 3 ? 1 : d == 4 ? 0 : d == 5 ? -1 : d == 6 ? -2 : -3;
  return k < 8 ? a : -a;
}
GF_KFD_HD int kfd_clamp_threshold(int t) { return t < 0 ? 0 : (t > 255 ? 255 : t); }
// M over the 16 arcs of 9 contiguous ring pixels and both polarities: the largest over the arcs of the smallest difference of an arc
GF_KFD_HD int kfd_fast_m(int v, const int *ring /* [16] */) {
  int m = -256;
  for (int s = 0; s < 16; s++) {
    int lo = 256, hi = 256;      // the minima of p - v and of v - p over the arc
    for (int k = 0; k < 9; k++) {
      const int d = ring[(s + k) & 15] - v;
      lo = d < lo ? d : lo; hi = -d < hi ? -d : hi;
    }
    m = lo > m ? lo : m; m = hi > m ? hi : m;
  }
  return m;
}
// every arc of 9 holds two of the four compass pixels: a corner has two of them brighter than v + t or two darker than v - t
GF_KFD_HD bool kfd_fast_maybe(int v, int p0, int p4, int p8, int p12, int t) {
  const int b = (p0 - v > t) + (p4 - v > t) + (p8 - v > t) + (p12 - v > t), d = (v - p0 > t) + (v - p4 > t) + (v - p8 > t) + (v - p12 > t);
  return b >= 2 || d >= 2;
}
// the score of the pixel at c (rows `stride` bytes apart, the ring inside the plane): 0 where M <= t, M - 1 otherwise
GF_KFD_HD int kfd_fast_score_at(const uint8_t *c, int stride, int t) {
  const int v = c[0];
  if (!kfd_fast_maybe(v, c[(ptrdiff_t)3 * stride], c[3], c[-(ptrdiff_t)3 * stride], c[-3], t)) return 0;
  int ring[16];
  for (int k = 0; k < 16; k++) ring[k] = c[(ptrdiff_t)kfd_ring_dy(k) * stride + kfd_ring_dx(k)];
  const int m = kfd_fast_m(v, ring);
  return m > t ? m - 1 : 0;
}
// the pixels that have a ring: everything but the frame of 3 pixels
GF_KFD_HD bool kfd_fast_inside(int rows, int cols, int x, int y) { return x >= KFD_FAST_R && y >= KFD_FAST_R && x <= cols - 1 - KFD_FAST_R && y <= rows - 1 - KFD_FAST_R; }
GF_KFD_HD int kfd_fast_score(const uint8_t *img, int stride, int rows, int cols, int x, int y, int t) {
  return kfd_fast_inside(rows, cols, x, y) ? kfd_fast_score_at(img + (size_t)y * (size_t)stride + (size_t)x, stride, t) : 0;
}
// suppression: kept iff the score is positive and strictly above all 8 neighbours (nb in any order)
GF_KFD_HD bool kfd_nms_keep(int s, const int *nb /* [8] */) {
  bool keep = s > 0;
  for (int k = 0; k < 8; k++) keep = keep && s > nb[k];
  return keep;
}

// ---- K4 ---------------------------------------------------------------------------------------------------------------------------
// finite and below 2^20 in magnitude (false for a NaN): the cast of kfd_brief_coord is defined
GF_KFD_HD bool kfd_point_ok(float px, float py) { return fabsf(px) < 1048576.f && fabsf(py) < 1048576.f; }
GF_KFD_HD int kfd_brief_coord(float p, int offset) { return (int)(p + (float)offset); }
// a pair's four offsets in one word: x1 | y1 << 8 | x2 << 16 | y2 << 24, each a signed byte
GF_KFD_HD uint32_t kfd_pack_pair(int x1, int y1, int x2, int y2) {
  return (uint32_t)(uint8_t)(int8_t)x1 | (uint32_t)(uint8_t)(int8_t)y1 << 8 | (uint32_t)(uint8_t)(int8_t)x2 << 16 | (uint32_t)(uint8_t)(int8_t)y2 << 24;
}
GF_KFD_HD int kfd_pair_field(uint32_t pair, int f) { return (int)(int8_t)(uint8_t)(pair >> (8 * f)); }
// bit i of a descriptor: both ends inside the image and blur[y1][x1] < blur[y2][x2]; (px, py) passes kfd_point_ok
GF_KFD_HD int kfd_brief_bit(const uint8_t *blur, int rows, int cols, float px, float py, uint32_t pair) {
  const int x1 = kfd_brief_coord(px, kfd_pair_field(pair, 0)), y1 = kfd_brief_coord(py, kfd_pair_field(pair, 1));
  const int x2 = kfd_brief_coord(px, kfd_pair_field(pair, 2)), y2 = kfd_brief_coord(py, kfd_pair_field(pair, 3));
  if (!(x1 >= 0 && x1 < cols && y1 >= 0 && y1 < rows && x2 >= 0 && x2 < cols && y2 >= 0 && y2 < rows)) return 0;
  return blur[(size_t)y1 * (size_t)cols + (size_t)x1] < blur[(size_t)y2 * (size_t)cols + (size_t)x2] ? 1 : 0;
}
inline bool kfd_pattern_ok(const int32_t *pattern /* [4][256] */) {
  for (int k = 0; k < 4 * KFD_PAIRS; k++)
    if (pattern[k] < -KFD_MAX_OFFSET || pattern[k] > KFD_MAX_OFFSET) return false;
  return true;
}
inline void kfd_pack_pattern(const int32_t *pattern, uint32_t *pairs /* [256] */) {
  for (int i = 0; i < KFD_PAIRS; i++) pairs[i] = kfd_pack_pair(pattern[i], pattern[KFD_PAIRS + i], pattern[2 * KFD_PAIRS + i], pattern[3 * KFD_PAIRS + i]);
}

// ---- host side (the shim of the tests and the one-thread figure of tools/diag_kfd_bench.py) ------------------------------------------
inline void kfd_host_blur(const uint8_t *img, int rows, int cols, uint8_t *out) {
  std::vector<uint16_t> h((size_t)rows * (size_t)cols);
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) h[(size_t)y * (size_t)cols + (size_t)x] = (uint16_t)kfd_blur_row(img + (size_t)y * (size_t)cols, cols, x);
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      int s = 0;
      for (int k = 0; k < 9; k++) s += kfd_tap(k) * (int)h[(size_t)klt_reflect101(y + k - KFD_BLUR_R, rows) * (size_t)cols + (size_t)x];
      out[(size_t)y * (size_t)cols + (size_t)x] = (uint8_t)kfd_blur_round(s);
    }
}
// K2 and K3 of one image: plane [rows][cols] the scores after suppression; the first `cap` kept corners in row-major order as pts [.][2]
// and score [.]; counters [4] = corners before suppression, kept, listed, overflow flag
inline void kfd_host_fast(const uint8_t *img, int rows, int cols, int threshold, int cap, uint8_t *plane, float *pts, int32_t *score, int32_t *counters) {
  const int t = kfd_clamp_threshold(threshold);
  std::vector<uint8_t> raw((size_t)rows * (size_t)cols);
  int before = 0, kept = 0, listed = 0;
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const int s = kfd_fast_score(img, cols, rows, cols, x, y, t);
      raw[(size_t)y * (size_t)cols + (size_t)x] = (uint8_t)s;
      before += s > 0;
    }
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      int nb[8], q = 0;
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          if (!dx && !dy) continue;
          const int xx = x + dx, yy = y + dy;
          nb[q++] = xx < 0 || yy < 0 || xx >= cols || yy >= rows ? 0 : raw[(size_t)yy * (size_t)cols + (size_t)xx];
        }
      const int s = raw[(size_t)y * (size_t)cols + (size_t)x];
      const bool keep = kfd_nms_keep(s, nb);
      plane[(size_t)y * (size_t)cols + (size_t)x] = keep ? (uint8_t)s : (uint8_t)0;
      if (!keep) continue;
      if (kept < cap) { pts[2 * listed] = (float)x; pts[2 * listed + 1] = (float)y; score[listed] = s; listed++; }
      kept++;
    }
  counters[0] = before; counters[1] = kept; counters[2] = listed; counters[3] = kept > cap ? 1 : 0;
}
// K4 of n points on a blurred plane: desc [n][4]; returns the points of the deviation (all-zero descriptors)
inline int kfd_host_brief(const uint8_t *blur, int rows, int cols, const uint32_t *pairs, int n, const float *pts, uint64_t *desc) {
  int bad = 0;
  for (int j = 0; j < n; j++) {
    uint64_t w[4] = {0, 0, 0, 0};
    const float px = pts[2 * j], py = pts[2 * j + 1];
    if (kfd_point_ok(px, py))
      for (int i = 0; i < KFD_PAIRS; i++) w[i >> 6] |= (uint64_t)kfd_brief_bit(blur, rows, cols, px, py, pairs[i]) << (i & 63);
    else
      bad++;
    for (int k = 0; k < 4; k++) desc[4 * (size_t)j + k] = w[k];
  }
  return bad;
}
// K5 of n points
inline void kfd_host_norm(const double *cam8, int n, const float *pts, float *pts_norm) {
  const ObsCam c = obs_camera(cam8);
  for (int j = 0; j < n; j++) obs_lift(c, pts[2 * j], pts[2 * j + 1], pts_norm + 2 * j, pts_norm + 2 * j + 1);
}

}  // namespace gfd
