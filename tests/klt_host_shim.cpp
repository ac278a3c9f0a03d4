// TEST INFRASTRUCTURE. The HIP-free half of the optical-flow tracker (ground-fusion2_amd/csrc/gfbe_klt.h: pyramid, derivative, the
// tracker of one point on one thread, the tracking half of trackImage, the point checks) behind a C interface for
// tests/test_klt_model.py and tools/diag_klt_bench.py. Built by a plain C++ compiler: the header has no HIP in it.
#include "../ground-fusion2_amd/csrc/gfbe_klt.h"

#include <string.h>

using namespace gfd;

extern "C" {

void *shim_klt_build(const unsigned char *image, int cols, int rows, int max_level) {
  KltHostPyramid *p = new KltHostPyramid();
  klt_host_build(image, cols, rows, max_level, p);
  return p;
}
void shim_klt_free(void *p) { delete (KltHostPyramid *)p; }
int shim_klt_levels(const void *p) { return ((const KltHostPyramid *)p)->view.n_levels; }
// dims [3] = w, h, stride; the padded image / derivative of a level when the pointers are not NULL
void shim_klt_level(const void *p, int level, unsigned char *img, short *der, int *dims) {
  const KltHostPyramid *P = (const KltHostPyramid *)p;
  const KltLevel &L = P->view.lv[level];
  dims[0] = L.w; dims[1] = L.h; dims[2] = L.stride;
  if (img) memcpy(img, P->img[(size_t)level].data(), P->img[(size_t)level].size());
  if (der) memcpy(der, P->der[(size_t)level].data(), P->der[(size_t)level].size() * sizeof(short));
}
void shim_klt_flow(const void *I, const void *J, int n, const float *prev, float *next, unsigned char *status, float *err, int max_level, int use_initial, int max_count,
                   double epsilon, double min_eig, int *trace) {
  klt_host_flow(((const KltHostPyramid *)I)->view, ((const KltHostPyramid *)J)->view, n, prev, next, status, err, max_level, use_initial,
                klt_params(max_count, epsilon, min_eig), trace);
}
// iopt = max_level, flow_back, border, grey_max, prediction_min_success, max_count; dopt = flow_back_dist, epsilon, min_eig_threshold
int shim_klt_track(const void *prev, const void *cur, int n, const float *pts, const int *ids, const int *cnt, int has_prediction, const float *predict, const int *iopt,
                   const double *dopt, float *prev_out, float *cur_out, int *ids_out, int *cnt_out, int *counters) {
  const KltTrackOptions O{iopt[0], iopt[1], iopt[2], iopt[3], iopt[4], dopt[0]};
  return klt_host_track(((const KltHostPyramid *)prev)->view, ((const KltHostPyramid *)cur)->view, n, pts, ids, cnt, has_prediction, predict, O,
                        klt_params(iopt[5], dopt[1], dopt[2]), prev_out, cur_out, ids_out, cnt_out, counters);
}
int shim_klt_check_points(int n_cameras, const int *offset, int capacity, const float *pts) { return klt_check_points(n_cameras, offset, capacity, pts); }
int shim_klt_in_border(float x, float y, int cols, int rows, int border) { return klt_in_border(x, y, cols, rows, border) ? 1 : 0; }
double shim_klt_distance(float ax, float ay, float bx, float by) { return klt_distance(ax, ay, bx, by); }
int shim_klt_floor(float v) { return klt_floor(v); }
int shim_klt_round(float v) { return klt_round(v); }
void shim_klt_weights(float a, float b, int *w) { const KltW k = klt_weights(a, b); w[0] = k.w00; w[1] = k.w01; w[2] = k.w10; w[3] = k.w11; }
}
