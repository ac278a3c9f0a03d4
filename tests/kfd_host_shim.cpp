// TEST INFRASTRUCTURE. ground-fusion2_amd/csrc/gfbe_kfd.h compiled for the host with a plain C++ compiler (no HIP): the same text the
// kernels of gfbe_kfd.hip compile for the device, behind C entry points for tests/test_kfd_model.py and tools/diag_kfd_bench.py.
#include "../ground-fusion2_amd/csrc/gfbe_kfd.h"

using namespace gfd;

extern "C" {

void shim_kfd_taps(int32_t *out9) {
  for (int k = 0; k < 9; k++) out9[k] = kfd_tap(k);
}
void shim_kfd_ring(int32_t *dx16, int32_t *dy16) {
  for (int k = 0; k < 16; k++) { dx16[k] = kfd_ring_dx(k); dy16[k] = kfd_ring_dy(k); }
}
void shim_kfd_blur(const uint8_t *img, int rows, int cols, uint8_t *out) { kfd_host_blur(img, rows, cols, out); }
int shim_kfd_blur_pixel(const uint8_t *img, int rows, int cols, int x, int y) { return kfd_blur_pixel(img, rows, cols, x, y); }
int shim_kfd_fast_score(const uint8_t *img, int rows, int cols, int x, int y, int t) { return kfd_fast_score(img, cols, rows, cols, x, y, kfd_clamp_threshold(t)); }
void shim_kfd_fast(const uint8_t *img, int rows, int cols, int t, int cap, uint8_t *plane, float *pts, int32_t *score, int32_t *counters) {
  kfd_host_fast(img, rows, cols, t, cap, plane, pts, score, counters);
}
int shim_kfd_pattern_ok(const int32_t *pattern) { return kfd_pattern_ok(pattern) ? 1 : 0; }
int shim_kfd_brief(const uint8_t *blur, int rows, int cols, const int32_t *pattern, int n, const float *pts, uint64_t *desc) {
  uint32_t pairs[KFD_PAIRS];
  kfd_pack_pattern(pattern, pairs);
  return kfd_host_brief(blur, rows, cols, pairs, n, pts, desc);
}
void shim_kfd_norm(const double *cam8, int n, const float *pts, float *pts_norm) { kfd_host_norm(cam8, n, pts, pts_norm); }
// a whole keyframe of one camera on one thread: what a caller had to do on the host before gfbe_kfd_*
int shim_kfd_keyframe(const uint8_t *img, int rows, int cols, const int32_t *pattern, const double *cam8, int t, int cap, uint8_t *blur, uint8_t *plane, float *pts,
                      int32_t *score, float *pts_norm, uint64_t *desc, int32_t *counters) {
  uint32_t pairs[KFD_PAIRS];
  kfd_pack_pattern(pattern, pairs);
  kfd_host_blur(img, rows, cols, blur);
  kfd_host_fast(img, rows, cols, t, cap, plane, pts, score, counters);
  kfd_host_brief(blur, rows, cols, pairs, counters[2], pts, desc);
  kfd_host_norm(cam8, counters[2], pts, pts_norm);
  return counters[2];
}

}  // extern "C"
