// gfbe_klt.h — the rules of the optical-flow tracker (gfbe_klt.hip) that need no HIP header: under a plain C++ compiler they are
// ordinary inline functions, under hipcc the per-pixel and per-point ones are __host__ __device__ (tests/klt_host_shim.cpp compiles
// them for the host). The rules R1 .. R5 are stated in include/gfbe_klt.h; citations are to
//
//   calc_sharr_deriv, the tracker, the pyramid builder      mesh/src/meshing/optical_flow/lkpyramid.cpp:56-149, :173-499, :516-619
//   FeatureTracker::trackImage, inBorder, distance          vins_estimator/src/featureTracker/feature_tracker.cpp:103-179, :14-28
//
// Every quantity summed over the 21 x 21 window is an integer and is summed as one (R3a); the float statements around the sums are
// single precision in the order written here, the epsilon / oscillation tests and the reverse distance are double as in the
// reference. There is no multiply-add: the build has -ffp-contract=off. The model tests/klt_np.py reproduces every function bit
// for bit.
//
// A per-point function is a template over a reducer R that owns the window: R::gram builds the patch (I, Ix, Iy) and returns the three
// sums of derivative products, R::mismatch the two sums of one iteration, R::abssum the sum of the err statement. On the host a
// reducer is a loop over the 441 pixels (KltHostWindow); on the device it is a wave whose lanes hold seven pixels of a row each and reduce
// with shuffles (gfbe_klt.hip). The sums are integers, so both give the same bits, and every lane of the wave then runs the same
// float statements on the same numbers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define GF_KLT_HD __host__ __device__ inline
#else
#define GF_KLT_HD inline
#endif

namespace gfd {

constexpr int KLT_WIN = 21;                 // winSize: the only one the reference passes
constexpr int KLT_PIX = KLT_WIN * KLT_WIN;  // 441
constexpr int KLT_MAX_LEVELS = 8;           // levels 0 .. 7 (gfbe_klt_options.max_level <= 7)
constexpr int KLT_W_BITS = 14;

// One level as the tracker reads it: the padded image (w + 42 bytes a row) and its padded derivative (interleaved Ix, Iy).
struct KltLevel {
  const uint8_t *img;
  const int16_t *der;
  int w, h, stride;      // stride = w + 2 * KLT_WIN (pixels; the derivative has 2 * stride int16 a row)
};
struct KltPyramid {
  int n_levels;
  KltLevel lv[KLT_MAX_LEVELS];
  const KltLevel &level(int l) const { return lv[l]; }
};

// ---- R1 / R2: borders, pyramid, derivative ------------------------------------------------------------------------------------
// BORDER_REFLECT_101 of an index that is at most n - 1 outside 0 .. n - 1 (n >= 2)
GF_KLT_HD int klt_reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// the size of level l + 1 (:604)
GF_KLT_HD int klt_half(int n) { return (n + 1) / 2; }

// The levels that are built for a request of max_level (:565-616): level l + 1 exists when its width and height are both > 21.
// Returns the number of levels (the effective maximum level + 1).
GF_KLT_HD int klt_plan_levels(int cols, int rows, int max_level, int *w, int *h) {
  int n = 0, cw = cols, ch = rows;
  for (int level = 0; level <= max_level && level < KLT_MAX_LEVELS; level++) {
    w[n] = cw; h[n] = ch; n++;
    cw = klt_half(cw); ch = klt_half(ch);
    if (cw <= KLT_WIN || ch <= KLT_WIN) break;
  }
  return n;
}

// pyrDown: pixel (x, y) of level l + 1 from the UNPADDED pixels of level l (src, row stride sstride, sw x sh): the 5 x 5 taps
// [1 4 6 4 1] x [1 4 6 4 1] around (2x, 2y), reflected, one rounding of the integer sum.
GF_KLT_HD int klt_down_pixel(const uint8_t *src, int sstride, int sw, int sh, int x, int y) {
  const int k[5] = {1, 4, 6, 4, 1};
  int sum = 0;
  for (int dy = -2; dy <= 2; dy++) {
    const uint8_t *row = src + (size_t)klt_reflect101(2 * y + dy, sh) * (size_t)sstride;
    int rs = 0;
    for (int dx = -2; dx <= 2; dx++) rs += k[dx + 2] * row[klt_reflect101(2 * x + dx, sw)];
    sum += k[dy + 2] * rs;
  }
  return (sum + 128) >> 8;
}

// calc_sharr_deriv at pixel (x, y) of an unpadded level (:76-80 rows, :112-119 columns: reflection without the edge pixel):
// t0 = 3 (above + below) + 10 centre, t1 = below - above per column; Ix = t0[x + 1] - t0[x - 1], Iy = 3 (t1[x - 1] + t1[x + 1]) + 10 t1[x].
GF_KLT_HD void klt_scharr_pixel(const uint8_t *src, int sstride, int w, int h, int x, int y, int *ix, int *iy) {
  const uint8_t *r0 = src + (size_t)klt_reflect101(y - 1, h) * (size_t)sstride, *r1 = src + (size_t)y * (size_t)sstride,
                *r2 = src + (size_t)klt_reflect101(y + 1, h) * (size_t)sstride;
  const int xm = klt_reflect101(x - 1, w), xp = klt_reflect101(x + 1, w);
  const int t0m = (r0[xm] + r2[xm]) * 3 + r1[xm] * 10, t0p = (r0[xp] + r2[xp]) * 3 + r1[xp] * 10;
  const int t1m = r2[xm] - r0[xm], t1c = r2[x] - r0[x], t1p = r2[xp] - r0[xp];
  *ix = (int16_t)(t0p - t0m);
  *iy = (int16_t)((t1p + t1m) * 3 + t1c * 10);
}

// ---- R3: one level of one point --------------------------------------------------------------------------------------------------
// cvFloor / cvRound of a float. A coordinate beyond +-2^30 is outside every image; it saturates there (the conversion of such a
// float is undefined in C++ and saturating on the device: the rule makes it one thing everywhere).
GF_KLT_HD int klt_floor(float v) {
  const float f = floorf(v);
  if (!(f > -1073741824.f)) return -1073741824;      // (also a NaN)
  if (f > 1073741824.f) return 1073741824;
  return (int)f;
}
GF_KLT_HD int klt_round(float v) {      // round half to even
  const float f = rintf(v);
  if (!(f > -1073741824.f)) return -1073741824;
  if (f > 1073741824.f) return 1073741824;
  return (int)f;
}

struct KltW { int w00, w01, w10, w11; };
// :228-231 — each float product in the order written: ((1 - a) (1 - b)) 2^14, (a (1 - b)) 2^14, ((1 - a) b) 2^14, the rest
GF_KLT_HD KltW klt_weights(float a, float b) {
  KltW w;
  const float oa = 1.f - a, ob = 1.f - b, s = (float)(1 << KLT_W_BITS);
  w.w00 = klt_round((oa * ob) * s);
  w.w01 = klt_round((a * ob) * s);
  w.w10 = klt_round((oa * b) * s);
  w.w11 = (1 << KLT_W_BITS) - w.w00 - w.w01 - w.w10;
  return w;
}

// the out-of-range test of :211-212, :359-360, :466-467 on the top-left corner of a window
GF_KLT_HD bool klt_outside(int x, int y, int w, int h) { return x < -KLT_WIN || x >= w || y < -KLT_WIN || y >= h; }

// CV_DESCALE(p00 iw00 + p01 iw01 + p10 iw10 + p11 iw11, shift) of the four neighbours of a window pixel (:302-310, :419-421)
GF_KLT_HD int klt_bilinear(int p00, int p01, int p10, int p11, const KltW &w, int shift) {
  return (p00 * w.w00 + p01 * w.w01 + p10 * w.w10 + p11 * w.w11 + (1 << (shift - 1))) >> shift;
}
// the image (descaled by 9) at the window pixel whose top-left neighbour is (x, y)
GF_KLT_HD int klt_sample_img(const KltLevel &L, int x, int y, const KltW &w) {
  const uint8_t *p = L.img + (size_t)(y + KLT_WIN) * (size_t)L.stride + (size_t)(x + KLT_WIN);
  return klt_bilinear(p[0], p[1], p[L.stride], p[L.stride + 1], w, 9);
}
// derivative component c (0: Ix, 1: Iy), descaled by 14
GF_KLT_HD int klt_sample_der(const KltLevel &L, int x, int y, int c, const KltW &w) {
  const int16_t *p = L.der + 2 * ((size_t)(y + KLT_WIN) * (size_t)L.stride + (size_t)(x + KLT_WIN)) + c;
  const size_t ds = 2 * (size_t)L.stride;
  return klt_bilinear(p[0], p[2], p[ds], p[ds + 2], w, 14);
}

// R3a: an exact integer sum becomes a float once, round to nearest even, times FLT_SCALE = 2^-20 (:227, :332-334, :435-436)
GF_KLT_HD float klt_scaled(long long s) { return (float)s * (1.f / (float)(1 << 20)); }

struct KltParams {
  int max_count;       // clamped to 0 .. 100
  double eps2;         // epsilon clamped to 0 .. 10, squared
  float min_eig;       // minEigThreshold
};
GF_KLT_HD KltParams klt_params(int max_count, double epsilon, double min_eig_threshold) {
  KltParams p;
  p.max_count = max_count < 0 ? 0 : (max_count > 100 ? 100 : max_count);
  const double e = epsilon < 0.0 ? 0.0 : (epsilon > 10.0 ? 10.0 : epsilon);
  p.eps2 = e * e;
  p.min_eig = (float)min_eig_threshold;
  return p;
}

// what a level did with a point, for the tests that look for a branch (bits; the top three of the last level that iterated)
enum { KLT_T_PREV_OUT = 1, KLT_T_FLAT = 2, KLT_T_NEXT_OUT = 4, KLT_T_EPS = 8, KLT_T_OSC = 16, KLT_T_COUNT = 32, KLT_T_ERR_OUT = 64, KLT_T_HALF = 128,
       KLT_T_MOVED = 256 /* with KLT_T_NEXT_OUT: the point left J after at least one step of this level */ };

// One level (:193-497). (ppx, ppy) = prevPts[ptidx]; (nx, ny) = nextPts[ptidx], read and written; status and err as the reference
// keeps them between levels. trace: or-ed KLT_T_* bits of this level (may be nullptr).
template <class R>
GF_KLT_HD void klt_level(R &red, const KltLevel &I, const KltLevel &J, int level, int max_level, int use_initial, float ppx, float ppy, float &nx, float &ny,
                         int &status, float &err, const KltParams &P, int *trace) {
  const float half = (float)(KLT_WIN - 1) * 0.5f, scale = (float)(1. / (double)(1 << level));
  float px = ppx * scale, py = ppy * scale;                                    // :193
  float qx, qy;
  if (level == max_level) {
    if (use_initial) { qx = nx * scale; qy = ny * scale; } else { qx = px; qy = py; }      // :195-201
  } else { qx = nx * 2.f; qy = ny * 2.f; }                                    // :203
  nx = qx; ny = qy;                                                            // :204
  px -= half; py -= half;
  const int ipx = klt_floor(px), ipy = klt_floor(py);
  int tr = 0;
  if (klt_outside(ipx, ipy, I.w, I.h)) {                                       // :211-222
    if (level == 0) { status = 0; err = 0.f; }
    if (trace) *trace = KLT_T_PREV_OUT;
    return;
  }
  const float a = px - (float)ipx, b = py - (float)ipy;
  KltW w = klt_weights(a, b);
  if (trace) { const float t = ((1.f - a) * (1.f - b)) * 16384.f; if (t - floorf(t) == 0.5f) tr |= KLT_T_HALF; }      // (iw00's product exactly on a half)
  long long s11, s12, s22;
  red.gram(I, ipx, ipy, w, s11, s12, s22);
  const float A11 = klt_scaled(s11), A12 = klt_scaled(s12), A22 = klt_scaled(s22);
  float D = A11 * A22 - A12 * A12;
  const float dd = A11 - A22;
  const float min_eig = ((A22 + A11) - sqrtf(dd * dd + (4.f * A12) * A12)) / (float)(2 * KLT_WIN * KLT_WIN);      // :337
  if (min_eig < P.min_eig || D < 1.1920928955078125e-7f) {                     // :342-347 (FLT_EPSILON)
    if (level == 0) status = 0;
    if (trace) *trace = tr | KLT_T_FLAT;
    return;
  }
  D = 1.f / D;
  float npx = qx - half, npy = qy - half;                                      // :351
  float pdx = 0.f, pdy = 0.f;
  int j;
  for (j = 0; j < P.max_count; j++) {
    const int inx = klt_floor(npx), iny = klt_floor(npy);
    if (klt_outside(inx, iny, J.w, J.h)) {                                     // :359-365
      if (level == 0) status = 0;
      tr |= KLT_T_NEXT_OUT | (j > 0 ? KLT_T_MOVED : 0);
      break;
    }
    const float ja = npx - (float)inx, jb = npy - (float)iny;
    w = klt_weights(ja, jb);
    long long sb1, sb2;
    red.mismatch(J, inx, iny, w, sb1, sb2);
    const float b1 = klt_scaled(sb1), b2 = klt_scaled(sb2);
    const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;      // :438-439
    npx += dx; npy += dy;
    nx = npx + half; ny = npy + half;                                          // :443
    if ((double)dx * (double)dx + (double)dy * (double)dy <= P.eps2) { tr |= KLT_T_EPS; break; }      // :445 (ddot is double)
    if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {                  // :448-453
      nx -= dx * 0.5f; ny -= dy * 0.5f;
      tr |= KLT_T_OSC;
      break;
    }
    pdx = dx; pdy = dy;
  }
  if (j == P.max_count) tr |= KLT_T_COUNT;
  if (status && level == 0) {                                                  // :458-497
    const float ex = nx - half, ey = ny - half;
    const int iex = klt_floor(ex), iey = klt_floor(ey);
    if (klt_outside(iex, iey, J.w, J.h)) {
      status = 0;
      tr |= KLT_T_ERR_OUT;
    } else {
      w = klt_weights(ex - (float)iex, ey - (float)iey);
      const long long s = red.abssum(J, iex, iey, w);
      err = ((float)s * 1.f) / (float)(32 * KLT_WIN * KLT_WIN);               // :496 (R3a: the sum is exact)
    }
  }
  if (trace) *trace = tr;
}

// R4: the descent of one point, levels max_level .. 0. status starts at 1, err at 0 (the reference leaves err unset where no level
// writes it; the library writes 0). (nx, ny): the initial flow when use_initial, the result afterwards. trace: [max_level + 1] or nullptr.
template <class R, class Pyr>
GF_KLT_HD void klt_point(R &red, const Pyr &I, const Pyr &J, int max_level, int use_initial, float ppx, float ppy, float &nx, float &ny, int &status,
                         float &err, const KltParams &P, int *trace) {      // (Pyr: level(l) gives the KltLevel)
  status = 1; err = 0.f;
  if (!use_initial) { nx = ppx; ny = ppy; }
  for (int level = max_level; level >= 0; level--)
    klt_level(red, I.level(level), J.level(level), level, max_level, use_initial, ppx, ppy, nx, ny, status, err, P, trace ? trace + level : nullptr);
}

// ---- R5: acceptance -------------------------------------------------------------------------------------------------------------
// distance() of feature_tracker.cpp:22-28: the differences are float, the rest double
GF_KLT_HD double klt_distance(float ax, float ay, float bx, float by) {
  const double dx = (double)(ax - bx), dy = (double)(ay - by);
  return sqrt(dx * dx + dy * dy);
}
// inBorder (:14-20) with BORDER_SIZE = border
GF_KLT_HD bool klt_in_border(float x, float y, int cols, int rows, int border) {
  const int ix = klt_round(x), iy = klt_round(y);
  return border <= ix && ix < cols - border && border <= iy && iy < rows - border;
}
// :137-167 for one point: 0 forward failed, 1 the reverse check failed, 2 border or grey failed, 3 kept. level0: the current image.
GF_KLT_HD int klt_decide(int status, int rstatus, float px, float py, float cx, float cy, float rx, float ry, int flow_back, double flow_back_dist, int border,
                         int grey_max, const KltLevel &level0) {
  if (!status) return 0;
  if (flow_back && !(rstatus && klt_distance(px, py, rx, ry) <= flow_back_dist)) return 1;
  if (!klt_in_border(cx, cy, level0.w, level0.h, border)) return 2;
  const int pu = (int)cx, pv = (int)cy;      // (inside the image: inBorder held, border >= 0)
  const int grey = level0.img[(size_t)(pv + KLT_WIN) * (size_t)level0.stride + (size_t)(pu + KLT_WIN)];
  return grey > grey_max ? 2 : 3;
}

// ---- the window on one thread ----------------------------------------------------------------------------------------------------
struct KltHostWindow {
  int16_t I[KLT_PIX], Ix[KLT_PIX], Iy[KLT_PIX];
  void gram(const KltLevel &L, int x0, int y0, const KltW &w, long long &s11, long long &s12, long long &s22) {
    s11 = s12 = s22 = 0;
    for (int k = 0; k < KLT_PIX; k++) {
      const int x = x0 + k % KLT_WIN, y = y0 + k / KLT_WIN;
      const int iv = klt_sample_img(L, x, y, w), ix = klt_sample_der(L, x, y, 0, w), iy = klt_sample_der(L, x, y, 1, w);
      I[k] = (int16_t)iv; Ix[k] = (int16_t)ix; Iy[k] = (int16_t)iy;
      s11 += (long long)(ix * ix); s12 += (long long)(ix * iy); s22 += (long long)(iy * iy);
    }
  }
  void mismatch(const KltLevel &L, int x0, int y0, const KltW &w, long long &b1, long long &b2) const {
    b1 = b2 = 0;
    for (int k = 0; k < KLT_PIX; k++) {
      const int diff = klt_sample_img(L, x0 + k % KLT_WIN, y0 + k / KLT_WIN, w) - I[k];
      b1 += (long long)(diff * Ix[k]); b2 += (long long)(diff * Iy[k]);
    }
  }
  long long abssum(const KltLevel &L, int x0, int y0, const KltW &w) const {
    long long s = 0;
    for (int k = 0; k < KLT_PIX; k++) {
      const int diff = klt_sample_img(L, x0 + k % KLT_WIN, y0 + k / KLT_WIN, w) - I[k];
      s += diff < 0 ? -diff : diff;
    }
    return s;
  }
};

// ---- host side (plain inline functions: the shim of the tests and the one-thread figure of tools/diag_klt_bench.py) ----------------
struct KltHostPyramid {
  std::vector<std::vector<uint8_t>> img;       // padded, (w + 42) (h + 42)
  std::vector<std::vector<int16_t>> der;       // padded, 2 int16 a pixel
  KltPyramid view;
};

// R1 and R2 of one image [rows][cols]
inline void klt_host_build(const uint8_t *image, int cols, int rows, int max_level, KltHostPyramid *P) {
  int w[KLT_MAX_LEVELS], h[KLT_MAX_LEVELS];
  const int n = klt_plan_levels(cols, rows, max_level, w, h);
  P->img.assign((size_t)n, {}); P->der.assign((size_t)n, {});
  P->view.n_levels = n;
  for (int l = 0; l < n; l++) {
    const int st = w[l] + 2 * KLT_WIN, ph = h[l] + 2 * KLT_WIN;
    std::vector<uint8_t> &im = P->img[(size_t)l];
    std::vector<int16_t> &de = P->der[(size_t)l];
    im.assign((size_t)st * (size_t)ph, 0); de.assign(2 * (size_t)st * (size_t)ph, 0);
    const uint8_t *src = l ? P->img[(size_t)l - 1].data() + (size_t)KLT_WIN * (size_t)(w[l - 1] + 2 * KLT_WIN) + KLT_WIN : image;
    const int sst = l ? w[l - 1] + 2 * KLT_WIN : cols;
    uint8_t *in = im.data() + (size_t)KLT_WIN * (size_t)st + KLT_WIN;
    for (int y = 0; y < h[l]; y++)
      for (int x = 0; x < w[l]; x++) in[(size_t)y * (size_t)st + (size_t)x] = l ? (uint8_t)klt_down_pixel(src, sst, w[l - 1], h[l - 1], x, y) : src[(size_t)y * (size_t)sst + (size_t)x];
    for (int y = 0; y < ph; y++)
      for (int x = 0; x < st; x++) {
        const int sx = klt_reflect101(x - KLT_WIN, w[l]), sy = klt_reflect101(y - KLT_WIN, h[l]);
        im[(size_t)y * (size_t)st + (size_t)x] = in[(size_t)sy * (size_t)st + (size_t)sx];
      }
    for (int y = 0; y < h[l]; y++)
      for (int x = 0; x < w[l]; x++) {
        int ix, iy;
        klt_scharr_pixel(in, st, w[l], h[l], x, y, &ix, &iy);
        int16_t *d = de.data() + 2 * ((size_t)(y + KLT_WIN) * (size_t)st + (size_t)(x + KLT_WIN));
        d[0] = (int16_t)ix; d[1] = (int16_t)iy;
      }
    P->view.lv[l] = KltLevel{im.data(), de.data(), w[l], h[l], st};
  }
}

// R4 on n points. next: the initial flow when use_initial, the result afterwards. trace: [n][KLT_MAX_LEVELS] or nullptr.
inline void klt_host_flow(const KltPyramid &I, const KltPyramid &J, int n, const float *prev, float *next, uint8_t *status, float *err, int max_level, int use_initial,
                          const KltParams &P, int *trace) {
  const int ml = max_level < I.n_levels - 1 ? max_level : I.n_levels - 1;
  KltHostWindow win;
  for (int i = 0; i < n; i++) {
    int st; float e, nx = next[2 * i], ny = next[2 * i + 1];
    if (trace) for (int l = 0; l < KLT_MAX_LEVELS; l++) trace[(size_t)i * KLT_MAX_LEVELS + l] = 0;
    klt_point(win, I, J, ml, use_initial, prev[2 * i], prev[2 * i + 1], nx, ny, st, e, P, trace ? trace + (size_t)i * KLT_MAX_LEVELS : nullptr);
    next[2 * i] = nx; next[2 * i + 1] = ny; status[i] = (uint8_t)st; err[i] = e;
  }
}

struct KltTrackOptions {
  int max_level, flow_back, border, grey_max, prediction_min_success;
  double flow_back_dist;
};

// R5 of one camera: prev -> cur. Outputs hold up to n rows; counters[4] = in, forward successes, after the reverse check, kept.
// Returns the number kept.
inline int klt_host_track(const KltPyramid &prev, const KltPyramid &cur, int n, const float *prev_pts, const int32_t *ids, const int32_t *track_cnt, int has_prediction,
                          const float *predict_pts, const KltTrackOptions &O, const KltParams &P, float *prev_out, float *cur_out, int32_t *ids_out,
                          int32_t *cnt_out, int32_t *counters) {
  const size_t N = (size_t)n;
  std::vector<float> c(2 * N), r(prev_pts, prev_pts + 2 * N), e(N);
  std::vector<uint8_t> st(N), rst(N, 1);
  auto successes = [&]() { int s = 0; for (size_t i = 0; i < N; i++) s += st[i] ? 1 : 0; return s; };
  bool full = true;
  if (has_prediction) {                                                        // :118-133
    for (size_t i = 0; i < 2 * N; i++) c[i] = predict_pts[i];
    klt_host_flow(prev, cur, n, prev_pts, c.data(), st.data(), e.data(), 1, 1, P, nullptr);
    full = successes() < O.prediction_min_success;
  }
  if (full) klt_host_flow(prev, cur, n, prev_pts, c.data(), st.data(), e.data(), O.max_level, 0, P, nullptr);
  if (O.flow_back) klt_host_flow(cur, prev, n, c.data(), r.data(), rst.data(), e.data(), 1, 1, P, nullptr);      // :141
  counters[0] = n; counters[1] = successes(); counters[2] = 0;
  int m = 0;
  for (size_t i = 0; i < N; i++) {
    const int d = klt_decide(st[i], rst[i], prev_pts[2 * i], prev_pts[2 * i + 1], c[2 * i], c[2 * i + 1], r[2 * i], r[2 * i + 1], O.flow_back, O.flow_back_dist,
                             O.border, O.grey_max, cur.lv[0]);
    if (d >= 2) counters[2]++;
    if (d != 3) continue;
    prev_out[2 * m] = prev_pts[2 * i]; prev_out[2 * m + 1] = prev_pts[2 * i + 1];
    cur_out[2 * m] = c[2 * i]; cur_out[2 * m + 1] = c[2 * i + 1];
    ids_out[m] = ids[i]; cnt_out[m] = track_cnt[i] + 1;                        // :170-179
    m++;
  }
  counters[3] = m;
  return m;
}

// the checks of the entry points, shared with the shim: 0 sound, else the rule that fails
enum { KLT_C_OK = 0, KLT_C_COUNT, KLT_C_FINITE };
inline int klt_check_points(int n_cameras, const int32_t *offset, int capacity, const float *pts) {
  if (!offset || offset[0] != 0) return KLT_C_COUNT;
  for (int c = 0; c < n_cameras; c++)
    if (offset[c + 1] < offset[c] || offset[c + 1] - offset[c] > capacity) return KLT_C_COUNT;
  const long long n = offset[n_cameras];
  if (n > 0 && !pts) return KLT_C_COUNT;
  for (long long i = 0; i < 2 * n; i++)
    if (!std::isfinite(pts[i])) return KLT_C_FINITE;
  return KLT_C_OK;
}

}  // namespace gfd
