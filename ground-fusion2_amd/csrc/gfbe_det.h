// gfbe_det.h — the rules of the corner detector (gfbe_det.hip) that need no HIP header: under a plain C++ compiler they are ordinary
// inline functions, under hipcc the per-pixel ones are __host__ __device__ (tests/det_host_shim.cpp compiles them for the host).
// The rules G1 .. G5 are stated in include/gfbe_det.h; citations are to
//
//   FeatureTracker::setMask, addPoints, trackImage      vins_estimator/src/featureTracker/feature_tracker.cpp:56-83, :85-93, :178-208
//
// Every sum over a 3 x 3 block is an integer and is summed as one; the float statements of G2 are single precision in the order
// written here. There is no multiply-add: the build has -ffp-contract=off. The model tests/det_np.py reproduces every function bit
// for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gfbe_klt.h"

#define GF_DET_HD GF_KLT_HD

namespace gfd {

constexpr int DET_MAX_POINTS = 2048;      // GFBE_DET_MAX_POINTS: held points a camera and corners a call
constexpr int DET_MAX_DIST = 32768;       // min_dist^2 and every dx^2 + dy^2 of an image up to 16384 x 16384 fit an int

// ---- G2 ---------------------------------------------------------------------------------------------------------------------------
// the 3 x 3 Sobel sums at a pixel whose eight neighbours can be read at p (an image with a border: no index logic here)
GF_DET_HD void det_sobel(const uint8_t *p, int stride, int *dx, int *dy) {
  const int a = p[-stride - 1], b = p[-stride], c = p[-stride + 1], d = p[-1], f = p[1], g = p[stride - 1], h = p[stride], i = p[stride + 1];
  *dx = (c + 2 * f + i) - (a + 2 * d + g);
  *dy = (g + 2 * h + i) - (a + 2 * b + c);
}
// A, B, C at pixel (x, y) of a w x h image; img0 is pixel (0, 0) inside a reflected border of at least 1 pixel. The planes of
// products are reflected: a block position outside the image takes the derivative of its mirror pixel (Dx of the padded image one
// pixel outside would have the other sign, and with it B).
GF_DET_HD void det_sums(const uint8_t *img0, int stride, int w, int h, int x, int y, int *A, int *B, int *C) {
  int a = 0, b = 0, c = 0;
  for (int j = -1; j <= 1; j++)
    for (int i = -1; i <= 1; i++) {
      int dx, dy;
      det_sobel(img0 + (ptrdiff_t)klt_reflect101(y + j, h) * stride + klt_reflect101(x + i, w), stride, &dx, &dy);
      a += dx * dx; b += dx * dy; c += dy * dy;
    }
  *A = a; *B = b; *C = c;
}
GF_DET_HD float det_eig(int A, int B, int C) {
  const float s2 = (float)((1.0 / (4.0 * 3.0 * 255.0)) * (1.0 / (4.0 * 3.0 * 255.0)));
  const float a = 0.5f * ((float)A * s2), b = (float)B * s2, c = 0.5f * ((float)C * s2);
  const float d = a - c;
  return (a + c) - sqrtf(d * d + b * b);
}
GF_DET_HD float det_response(const uint8_t *img0, int stride, int w, int h, int x, int y) {
  int A, B, C;
  det_sums(img0, stride, w, h, x, y, &A, &B, &C);
  return det_eig(A, B, C);
}

// ---- G3 ---------------------------------------------------------------------------------------------------------------------------
GF_DET_HD float det_threshold(float max_val, double quality) { return (float)((double)max_val * quality); }
// a value as its 3 x 3 maximum sees it
GF_DET_HD float det_thresholded(float v, float t) { return v > t ? v : 0.f; }
// candidate test of a clear interior pixel: v its response, m the largest thresholded value of its neighbours inside the image (itself included)
GF_DET_HD bool det_is_candidate(float v, float t, float m) { return v > t && v != 0.f && v == m; }
// the order of G3 as one unsigned key: the response's bits made monotonic, then the pixel index; larger keys are taken first
GF_DET_HD uint32_t det_float_order(float v) {
  union { float f; uint32_t u; } q;
  q.f = v;
  return (q.u & 0x80000000u) ? ~q.u : (q.u | 0x80000000u);
}
GF_DET_HD float det_float_unorder(uint32_t o) {
  union { float f; uint32_t u; } q;
  q.u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return q.f;
}
GF_DET_HD uint64_t det_key(float v, int index) { return ((uint64_t)det_float_order(v) << 32) | (uint32_t)index; }
GF_DET_HD float det_key_response(uint64_t k) { return det_float_unorder((uint32_t)(k >> 32)); }
GF_DET_HD int det_key_index(uint64_t k) { return (int)(uint32_t)k; }

// ---- G1 ---------------------------------------------------------------------------------------------------------------------------
// the order of setMask as one unsigned key: track_cnt descending, then the list index ascending; smaller keys come first
GF_DET_HD uint64_t det_mask_key(int track_cnt, int index) { return ((uint64_t)(~((uint32_t)track_cnt ^ 0x80000000u)) << 32) | (uint32_t)index; }
GF_DET_HD bool det_inside(int px, int py, int w, int h) { return px >= 0 && px < w && py >= 0 && py < h; }
GF_DET_HD int det_d2(int ax, int ay, int bx, int by) { return (ax - bx) * (ax - bx) + (ay - by) * (ay - by); }      // (both inside an image of <= 16384)

// ---- host side (the shim of the tests and the one-thread figure of tools/diag_det_bench.py) --------------------------------------------
// G1 of one camera: order [n] out = the list indices of the kept points in the order kept; kept_xy [n][2] their pixels. Returns the number kept.
inline int det_host_mask(int n, const float *pts, const int32_t *track_cnt, int w, int h, int min_dist, int *order, int *kept_xy) {
  std::vector<uint64_t> keys((size_t)n);
  for (int i = 0; i < n; i++) keys[(size_t)i] = det_mask_key(track_cnt[i], i);
  std::sort(keys.begin(), keys.end());
  const int r2 = min_dist * min_dist;
  int kept = 0;
  for (int s = 0; s < n; s++) {
    const int i = (int)(uint32_t)keys[(size_t)s], px = klt_round(pts[2 * i]), py = klt_round(pts[2 * i + 1]);
    if (!det_inside(px, py, w, h)) continue;
    bool clear = true;
    for (int k = 0; k < kept && clear; k++) clear = det_d2(px, py, kept_xy[2 * k], kept_xy[2 * k + 1]) > r2;
    if (!clear) continue;
    order[kept] = i; kept_xy[2 * kept] = px; kept_xy[2 * kept + 1] = py; kept++;
  }
  return kept;
}
inline bool det_host_clear(int x, int y, int kept, const int *kept_xy, int r2) {
  for (int k = 0; k < kept; k++)
    if (det_d2(x, y, kept_xy[2 * k], kept_xy[2 * k + 1]) <= r2) return false;
  return true;
}
// the image [h][w] with a reflected border of 1 (what the device reads from the tracker's level 0)
inline void det_host_pad(const uint8_t *image, int w, int h, std::vector<uint8_t> *out) {
  const int st = w + 2;
  out->assign((size_t)st * (size_t)(h + 2), 0);
  for (int y = -1; y <= h; y++)
    for (int x = -1; x <= w; x++) (*out)[(size_t)(y + 1) * (size_t)st + (size_t)(x + 1)] = image[(size_t)klt_reflect101(y, h) * (size_t)w + (size_t)klt_reflect101(x, w)];
}
// G2 of every pixel and the mask of the kept discs (255 clear, 0 cleared); either output may be nullptr
inline void det_host_planes(const uint8_t *image, int w, int h, int kept, const int *kept_xy, int min_dist, float *eig, uint8_t *mask) {
  std::vector<uint8_t> pad;
  det_host_pad(image, w, h, &pad);
  const uint8_t *img0 = pad.data() + (size_t)(w + 2) + 1;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      if (eig) eig[(size_t)y * (size_t)w + (size_t)x] = det_response(img0, w + 2, w, h, x, y);
      if (mask) mask[(size_t)y * (size_t)w + (size_t)x] = det_host_clear(x, y, kept, kept_xy, min_dist * min_dist) ? 255 : 0;
    }
}
// the candidates of G3 as keys, in no particular order
inline void det_host_candidates(const float *eig, int w, int h, int kept, const int *kept_xy, int min_dist, double quality, std::vector<uint64_t> *cand) {
  cand->clear();
  const int r2 = min_dist * min_dist;
  bool any = false;
  float max_val = 0.f;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      if (!det_host_clear(x, y, kept, kept_xy, r2)) continue;
      const float v = eig[(size_t)y * (size_t)w + (size_t)x];
      if (!any || v > max_val) max_val = v;
      any = true;
    }
  if (!any) return;
  const float t = det_threshold(max_val, quality);
  for (int y = 1; y <= h - 2; y++)
    for (int x = 1; x <= w - 2; x++) {
      if (!det_host_clear(x, y, kept, kept_xy, r2)) continue;
      float m = det_thresholded(eig[(size_t)y * (size_t)w + (size_t)x], t);
      for (int j = -1; j <= 1; j++)
        for (int i = -1; i <= 1; i++) m = std::max(m, det_thresholded(eig[(size_t)(y + j) * (size_t)w + (size_t)(x + i)], t));
      const float v = eig[(size_t)y * (size_t)w + (size_t)x];
      if (det_is_candidate(v, t, m)) cand->push_back(det_key(v, y * w + x));
    }
}
// the walk of G3 over candidate keys (any order in; they are sorted here): xy [max_corners][2], resp [max_corners]. Returns the number accepted.
inline int det_host_walk(std::vector<uint64_t> cand, int w, int min_dist, int max_corners, int *xy, float *resp) {
  std::sort(cand.begin(), cand.end(), [](uint64_t a, uint64_t b) { return a > b; });
  const int r2 = min_dist * min_dist;
  int n = 0;
  for (size_t s = 0; s < cand.size() && n < max_corners; s++) {
    const int idx = det_key_index(cand[s]), x = idx % w, y = idx / w;
    bool ok = true;
    for (int k = 0; k < n && ok; k++) ok = !(det_d2(x, y, xy[2 * k], xy[2 * k + 1]) < r2);
    if (!ok) continue;
    xy[2 * n] = x; xy[2 * n + 1] = y;
    if (resp) resp[n] = det_key_response(cand[s]);
    n++;
  }
  return n;
}
// G2 and G3 with no mask: the call of keyframe.cpp:169. candidate_capacity 0: no bound. Returns the number of corners, 0 on overflow.
inline int det_host_corners(const uint8_t *image, int w, int h, int max_corners, double quality, int min_dist, int candidate_capacity, float *pts, float *resp,
                            int *n_candidates) {
  std::vector<float> eig((size_t)w * (size_t)h);
  det_host_planes(image, w, h, 0, nullptr, 0, eig.data(), nullptr);
  std::vector<uint64_t> cand;
  det_host_candidates(eig.data(), w, h, 0, nullptr, 0, quality, &cand);
  if (n_candidates) *n_candidates = (int)cand.size();
  if (candidate_capacity > 0 && cand.size() > (size_t)candidate_capacity) return 0;
  std::vector<int> xy(2 * (size_t)std::max(max_corners, 1));
  const int n = det_host_walk(cand, w, min_dist, max_corners, xy.data(), resp);
  for (int k = 0; k < 2 * n; k++) pts[k] = (float)xy[(size_t)k];
  return n;
}
// G1, G3, G4, G5 of one camera. Outputs hold max(n, max_cnt) rows; counters [6] as gfbe_det_detect's; *next_id is advanced.
// Returns the number of points afterwards.
inline int det_host_detect(const uint8_t *image, int w, int h, int n, const float *pts, const int32_t *ids, const int32_t *track_cnt, int max_cnt, int min_dist,
                           double quality, int candidate_capacity, int32_t *next_id, float *pts_out, int32_t *ids_out, int32_t *cnt_out, int32_t *counters) {
  std::vector<int> order((size_t)std::max(n, 1)), kxy(2 * (size_t)std::max(n, 1));
  const int kept = det_host_mask(n, pts, track_cnt, w, h, min_dist, order.data(), kxy.data());
  for (int k = 0; k < kept; k++) {
    const int i = order[(size_t)k];
    pts_out[2 * k] = pts[2 * i]; pts_out[2 * k + 1] = pts[2 * i + 1]; ids_out[k] = ids[i]; cnt_out[k] = track_cnt[i];
  }
  const int want = max_cnt - kept;                                            // G4
  int added = 0, n_cand = 0, overflow = 0;
  if (want > 0) {
    std::vector<float> eig((size_t)w * (size_t)h);
    det_host_planes(image, w, h, 0, nullptr, 0, eig.data(), nullptr);
    std::vector<uint64_t> cand;
    det_host_candidates(eig.data(), w, h, kept, kxy.data(), min_dist, quality, &cand);
    n_cand = (int)cand.size();
    overflow = candidate_capacity > 0 && n_cand > candidate_capacity;
    if (!overflow) {
      std::vector<int> xy(2 * (size_t)want);
      added = det_host_walk(cand, w, min_dist, want, xy.data(), nullptr);
      for (int k = 0; k < added; k++) {                                       // G5
        pts_out[2 * (kept + k)] = (float)xy[2 * (size_t)k]; pts_out[2 * (kept + k) + 1] = (float)xy[2 * (size_t)k + 1];
        ids_out[kept + k] = (*next_id)++; cnt_out[kept + k] = 1;
      }
    }
  }
  counters[0] = n; counters[1] = kept; counters[2] = n_cand; counters[3] = added; counters[4] = *next_id; counters[5] = overflow;
  return kept + added;
}

}  // namespace gfd
