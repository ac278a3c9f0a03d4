// TEST INFRASTRUCTURE. The HIP-free half of the corner detector (ground-fusion2_amd/csrc/gfbe_det.h: the mask of setMask, the
// response, the candidates, the walk, addPoints) behind a C interface for tests/test_det_model.py and tools/diag_det_bench.py.
// Built by a plain C++ compiler: the header has no HIP in it.
#include "../ground-fusion2_amd/csrc/gfbe_det.h"

#include <string.h>

using namespace gfd;

extern "C" {

int shim_det_mask(int n, const float *pts, const int *track_cnt, int w, int h, int min_dist, int *order, int *kept_xy) {
  return det_host_mask(n, pts, track_cnt, w, h, min_dist, order, kept_xy);
}
void shim_det_planes(const unsigned char *image, int w, int h, int kept, const int *kept_xy, int min_dist, float *eig, unsigned char *mask) {
  det_host_planes(image, w, h, kept, kept_xy, min_dist, eig, mask);
}
// the candidate keys in the order of G3; returns their number (keys_out may be NULL to count)
int shim_det_candidates(const float *eig, int w, int h, int kept, const int *kept_xy, int min_dist, double quality, unsigned long long *keys_out, int room) {
  std::vector<uint64_t> cand;
  det_host_candidates(eig, w, h, kept, kept_xy, min_dist, quality, &cand);
  std::sort(cand.begin(), cand.end(), [](uint64_t a, uint64_t b) { return a > b; });
  for (size_t i = 0; keys_out && i < cand.size() && (int)i < room; i++) keys_out[i] = cand[i];
  return (int)cand.size();
}
unsigned long long shim_det_key(float v, int index) { return det_key(v, index); }
float shim_det_key_response(unsigned long long k) { return det_key_response(k); }
int shim_det_walk(const unsigned long long *keys, int n, int w, int min_dist, int max_corners, int *xy, float *resp) {
  return det_host_walk(std::vector<uint64_t>(keys, keys + n), w, min_dist, max_corners, xy, resp);
}
int shim_det_corners(const unsigned char *image, int w, int h, int max_corners, double quality, int min_dist, int candidate_capacity, float *pts, float *resp, int *n_cand) {
  return det_host_corners(image, w, h, max_corners, quality, min_dist, candidate_capacity, pts, resp, n_cand);
}
int shim_det_detect(const unsigned char *image, int w, int h, int n, const float *pts, const int *ids, const int *cnt, int max_cnt, int min_dist, double quality,
                    int candidate_capacity, int *next_id, float *pts_out, int *ids_out, int *cnt_out, int *counters) {
  return det_host_detect(image, w, h, n, pts, ids, cnt, max_cnt, min_dist, quality, candidate_capacity, next_id, pts_out, ids_out, cnt_out, counters);
}
}
