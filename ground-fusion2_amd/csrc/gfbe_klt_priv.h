// gfbe_klt_priv.h — the tracker's handle as the library's own sources see it: gfbe_klt.hip owns it, gfbe_det.hip (the corner detector,
// include/gfbe_det.h) borrows the current image set and the held points from it, gfbe_obs.hip (the frame observations,
// include/gfbe_obs.h) the held points. Nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/gfbe_klt.h"
#include "gfbe_handle.h"
#include "gfbe_klt.h"

namespace gfd {
// where the levels of one camera's set lie: images in bytes, derivatives in int16 elements, from the camera's base
struct KltGeom {
  int n_levels;
  int w[KLT_MAX_LEVELS], h[KLT_MAX_LEVELS];
  long long img_off[KLT_MAX_LEVELS], der_off[KLT_MAX_LEVELS];
  long long img_cam, der_cam;
};
__host__ __device__ inline KltLevel klt_view(const KltGeom &g, const uint8_t *img, const int16_t *der, int cam, int l) {
  return KltLevel{img + (size_t)cam * (size_t)g.img_cam + (size_t)g.img_off[l], der + (size_t)cam * (size_t)g.der_cam + (size_t)g.der_off[l], g.w[l], g.h[l],
                  g.w[l] + 2 * KLT_WIN};
}
}  // namespace gfd

struct gfbe_klt : gfbe_handle {
  gfbe_klt_options opt;
  int n_cam = 0, rows = 0, cols = 0, cap = 0;
  gfd::KltGeom g;
  uint8_t *img[2] = {nullptr, nullptr};       // the two sets; `cur_set` is the current image's
  int16_t *der[2] = {nullptr, nullptr};
  int cur_set = 0;
  long long n_pushed = 0;
  uint8_t *raw_d = nullptr, *raw_h = nullptr;      // the upload of a push and its pinned mirror
  hipEvent_t ev_raw = nullptr;
  bool raw_busy = false;
  // the held points (two halves: a track compacts from one into the other), rows [n_cam * cap]
  float *pts[2] = {nullptr, nullptr};
  int *ids[2] = {nullptr, nullptr}, *cnt[2] = {nullptr, nullptr};
  int *seg_count[2] = {nullptr, nullptr};
  int *seg_begin = nullptr;
  int half = 0;
  // a track's scratch
  float *w_cur = nullptr, *w_rev = nullptr, *w_err = nullptr;
  uint8_t *w_st = nullptr, *w_rst = nullptr, *w_dec = nullptr;      // forward / reverse status, the decision of a point
  int *gate = nullptr;
  std::vector<int> begin_h, count_h;          // exact host mirrors
};

namespace gfd {
// the two halves of gfbe_klt_push_image on a checked handle (gfbe_klt.hip): images through the pinned mirror into raw_d, then the
// pyramid build of raw_d into the other set. gfbe_eq.hip (include/gfbe_eq.h) equalises raw_d between them.
gfbe_status klt_push_upload(gfbe_ctx *c, gfbe_klt *m, const uint8_t *images);
gfbe_status klt_push_enqueue(gfbe_ctx *c, gfbe_klt *m);
}  // namespace gfd
