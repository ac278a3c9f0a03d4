// gfbe_eq.h — the rules of the image equalisation (gfbe_eq.hip) that need no HIP header: under a plain C++ compiler they are ordinary
// inline functions, under hipcc the per-tile and per-pixel ones are __host__ __device__ (tests/eq_host_shim.cpp compiles them for the
// host). Contrast-limited adaptive histogram equalisation of an 8-bit, one-channel image, where the reference calls
//
//   cv::createCLAHE()->apply(image, image)                         vins_estimator/src/rosNodeTest.cpp:271-276, dense_map/src/pose_graph_node.cpp:642-647
//   cv::createCLAHE(3.0, cv::Size(8, 8))                           linefeatureTracker/linefeature_tracker.cpp:56-60
//
// The rules are OpenCV's CLAHE as documented and as its clahe.cpp (3.4 / 4.x) is remembered: an ASSUMPTION of the model, nothing of
// OpenCV was at hand to run. The model tests/eq_np.py reproduces every function bit for bit.
//
// E1 geometry. Options tiles_x, tiles_y (8, 8) and clip_limit (40.0). If cols % tiles_x == 0 and rows % tiles_y == 0 the tile is
//    (cols / tiles_x, rows / tiles_y) and the histograms read the image. Otherwise the image is extended at the bottom by
//    tiles_y - rows % tiles_y rows AND at the right by tiles_x - cols % tiles_x columns with BORDER_REFLECT_101 (a dimension that is
//    divisible by itself then gets a whole extra `tiles` of padding: OpenCV's quirk, kept), and the tile is the extended size divided
//    by the tile counts. Nothing is extended in memory: pixel (X, Y) of the extended image is pixel (reflect(X), reflect(Y)).
// E2 histogram. Each tile has 256 bins over its area = tw * th pixels of the (extended) image.
// E3 clip and redistribute, only when clip_limit > 0: limit = max((int)(clip_limit * area / 256), 1) with the product and the quotient
//    in double (a quotient of area or more is taken as area: such a limit clips nothing, and the conversion stays defined for any
//    finite clip_limit). clipped is the sum of the excesses over limit, the bins are cut to limit, every bin gets clipped / 256, and
//    with residual = clipped % 256 > 0 and step = max(256 / residual, 1) the bins 0, step, 2 step, ... get one more until residual of
//    them have been served: bin i gets one more iff i % step == 0 && i / step < residual ((residual - 1) * step < 256, so the
//    loop's i < 256 never bites).
// E4 LUT. lut[i] = saturate_u8(cvRound((float)sum_i * scale)), sum_i the running sum of the bins up to and including i,
//    scale = 255.0f / (float)area one float division, cvRound half to even.
// E5 interpolation, all in single precision, nothing fused, in the written order: inv_tw = 1.0f / (float)tw; for column x
//    txf = (float)x * inv_tw - 0.5f, tx1 = floor(txf), xa = txf - (float)tx1, xa1 = 1.0f - xa, THEN tx1 is clamped to >= 0 and
//    tx2 = tx1 + 1 to <= tiles_x - 1; rows likewise. With v the source pixel,
//    res = (L[ty1][tx1][v] * xa1 + L[ty1][tx2][v] * xa) * ya1 + (L[ty2][tx1][v] * xa1 + L[ty2][tx2][v] * xa) * ya and
//    out = saturate_u8(cvRound(res)), over the ORIGINAL rows x cols with tw and th of E1.
// E6 in place. Output may overwrite input: a pixel reads only itself and the LUTs.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gfbe_klt.h"

#define GF_EQ_HD GF_KLT_HD

namespace gfd {

constexpr int EQ_BINS = 256;
constexpr int EQ_MAX_TILES = 64;          // tiles_x, tiles_y: 1 .. 64
constexpr int EQ_MAX_SIZE = 1 << 14;      // rows, cols

// ---- E1 ---------------------------------------------------------------------------------------------------------------------------
struct EqGeom {
  int rows, cols, tiles_x, tiles_y;
  int tw, th;                // the tile
  int limit;                 // E3's limit; 0: no clipping
  float scale;               // E4
  float inv_tw, inv_th;      // E5
};
inline const char *eq_geom_error(int rows, int cols, int tiles_x, int tiles_y, double clip_limit) {
  if (tiles_x < 1 || tiles_x > EQ_MAX_TILES || tiles_y < 1 || tiles_y > EQ_MAX_TILES) return "tiles_x / tiles_y outside 1 .. 64";
  if (rows <= tiles_y || cols <= tiles_x) return "rows <= tiles_y or cols <= tiles_x (the reflected extension must stay inside the image)";
  if (rows > EQ_MAX_SIZE || cols > EQ_MAX_SIZE) return "rows / cols above 16384";
  if (!(clip_limit >= 0.0) || !(clip_limit <= 1.7976931348623157e308)) return "clip_limit is not finite or is negative";
  return nullptr;
}
GF_EQ_HD bool eq_extended(int rows, int cols, int tiles_x, int tiles_y) { return cols % tiles_x != 0 || rows % tiles_y != 0; }
GF_EQ_HD int eq_limit(double clip_limit, int area) {
  if (!(clip_limit > 0.0)) return 0;
  const double q = clip_limit * (double)area / 256.0;
  if (q >= (double)area) return area;
  const int l = (int)q;
  return l > 1 ? l : 1;
}
inline EqGeom eq_geom(int rows, int cols, int tiles_x, int tiles_y, double clip_limit) {
  EqGeom g;
  g.rows = rows; g.cols = cols; g.tiles_x = tiles_x; g.tiles_y = tiles_y;
  const bool ext = eq_extended(rows, cols, tiles_x, tiles_y);
  g.tw = (ext ? cols + (tiles_x - cols % tiles_x) : cols) / tiles_x;
  g.th = (ext ? rows + (tiles_y - rows % tiles_y) : rows) / tiles_y;
  const int area = g.tw * g.th;
  g.limit = eq_limit(clip_limit, area);
  g.scale = 255.0f / (float)area;
  g.inv_tw = 1.0f / (float)g.tw;
  g.inv_th = 1.0f / (float)g.th;
  return g;
}
// pixel (X, Y) of the extended image
GF_EQ_HD uint8_t eq_pixel(const uint8_t *img, int rows, int cols, int X, int Y) {
  return img[(size_t)klt_reflect101(Y, rows) * (size_t)cols + (size_t)klt_reflect101(X, cols)];
}

// ---- E3, E4 -----------------------------------------------------------------------------------------------------------------------
GF_EQ_HD int eq_excess(int bin, int limit) { return limit > 0 && bin > limit ? bin - limit : 0; }
// bin i after the cut and the redistribution of `clipped` (the sum of the excesses of the tile)
GF_EQ_HD int eq_redistribute(int bin, int i, int limit, int clipped) {
  if (limit <= 0) return bin;
  int b = (bin > limit ? limit : bin) + clipped / EQ_BINS;
  const int residual = clipped % EQ_BINS;
  if (residual > 0) {
    const int step = EQ_BINS / residual > 1 ? EQ_BINS / residual : 1;
    if (i % step == 0 && i / step < residual) b += 1;
  }
  return b;
}
GF_EQ_HD int eq_saturate(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
GF_EQ_HD uint8_t eq_lut_value(int sum, float scale) { return (uint8_t)eq_saturate(klt_round((float)sum * scale)); }

// ---- E5 ---------------------------------------------------------------------------------------------------------------------------
struct EqAxis {
  int t1, t2;        // the two tiles, clamped
  float a, a1;       // the weight of t2 and of t1
};
GF_EQ_HD EqAxis eq_axis(int x, float inv_t, int tiles) {
  EqAxis r;
  const float tf = (float)x * inv_t - 0.5f;
  const int t1 = (int)floorf(tf);
  r.a = tf - (float)t1;
  r.a1 = 1.0f - r.a;
  r.t1 = t1 < 0 ? 0 : (t1 > tiles - 1 ? tiles - 1 : t1);      // (the upper clamp never bites for x < tiles * t: it only bounds the index)
  r.t2 = t1 + 1 > tiles - 1 ? tiles - 1 : t1 + 1;
  return r;
}
GF_EQ_HD uint8_t eq_interp(int l11, int l12, int l21, int l22, const EqAxis &X, const EqAxis &Y) {
  const float top = (float)l11 * X.a1 + (float)l12 * X.a, bottom = (float)l21 * X.a1 + (float)l22 * X.a;
  const float res = top * Y.a1 + bottom * Y.a;
  return (uint8_t)eq_saturate(klt_round(res));
}

// ---- the host statement of E1 .. E6 (one thread): lut [tiles_y][tiles_x][256], out may be img -------------------------------------------
inline void eq_host_lut(const uint8_t *img, const EqGeom &g, uint8_t *lut) {
  for (int ty = 0; ty < g.tiles_y; ty++)
    for (int tx = 0; tx < g.tiles_x; tx++) {
      int hist[EQ_BINS] = {};
      for (int y = 0; y < g.th; y++)
        for (int x = 0; x < g.tw; x++) hist[eq_pixel(img, g.rows, g.cols, tx * g.tw + x, ty * g.th + y)]++;
      int clipped = 0;
      for (int i = 0; i < EQ_BINS; i++) clipped += eq_excess(hist[i], g.limit);
      int sum = 0;
      uint8_t *l = lut + ((size_t)ty * (size_t)g.tiles_x + (size_t)tx) * EQ_BINS;
      for (int i = 0; i < EQ_BINS; i++) {
        sum += eq_redistribute(hist[i], i, g.limit, clipped);
        l[i] = eq_lut_value(sum, g.scale);
      }
    }
}
inline void eq_host_apply(const uint8_t *img, const EqGeom &g, const uint8_t *lut, uint8_t *out) {
  for (int y = 0; y < g.rows; y++) {
    const EqAxis Y = eq_axis(y, g.inv_th, g.tiles_y);
    const uint8_t *r1 = lut + (size_t)Y.t1 * (size_t)g.tiles_x * EQ_BINS, *r2 = lut + (size_t)Y.t2 * (size_t)g.tiles_x * EQ_BINS;
    for (int x = 0; x < g.cols; x++) {
      const EqAxis X = eq_axis(x, g.inv_tw, g.tiles_x);
      const size_t p = (size_t)y * (size_t)g.cols + (size_t)x;
      const int v = img[p];
      out[p] = eq_interp(r1[(size_t)X.t1 * EQ_BINS + v], r1[(size_t)X.t2 * EQ_BINS + v], r2[(size_t)X.t1 * EQ_BINS + v], r2[(size_t)X.t2 * EQ_BINS + v], X, Y);
    }
  }
}

}  // namespace gfd
