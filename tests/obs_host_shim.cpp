// TEST INFRASTRUCTURE. The HIP-free half of the frame observations (ground-fusion2_amd/csrc/gfbe_obs.h: the lift, the velocity, the
// depth index, the id order, the row, the prediction chain) behind a C interface for tests/test_obs_model.py and
// tools/diag_obs_bench.py. Built by a plain C++ compiler: the header has no HIP in it.
#include "../ground-fusion2_amd/csrc/gfbe_obs.h"

#include <string.h>

using namespace gfd;

extern "C" {

void shim_obs_distortion(const double *cam8, double x, double y, double *dx, double *dy) { obs_distortion(obs_camera(cam8), x, y, dx, dy); }
void shim_obs_lift(const double *cam8, int n, const float *pts, float *un) {
  const ObsCam c = obs_camera(cam8);
  for (int i = 0; i < n; i++) obs_lift(c, pts[2 * i], pts[2 * i + 1], un + 2 * i, un + 2 * i + 1);
}
int shim_obs_camera_ok(const double *cam8) { return obs_camera_ok(cam8) ? 1 : 0; }
float shim_obs_velocity(float un, float prev_un, double dt) { return obs_velocity(un, prev_un, dt); }
// returns inside (0 / 1)
int shim_obs_depth_index(float u, float v, int cols, int rows, int *x, int *y) {
  bool inside;
  obs_depth_index(u, v, cols, rows, x, y, &inside);
  return inside ? 1 : 0;
}
// returns the duplicate flag
int shim_obs_sort(int n, const int *ids, int *order) { return obs_host_sort(n, ids, order) ? 1 : 0; }
void shim_obs_observe(const double *cam8, int n, const float *pts, const int *ids, int n_prev, const int *prev_ids, const float *prev_un, double dt,
                      const unsigned short *depth, int cols, int rows, int *ids_out, double *obs8, float *un_out, int *counters) {
  obs_host_observe(cam8, n, pts, ids, n_prev, prev_ids, prev_un, dt, depth, cols, rows, ids_out, obs8, un_out, counters);
}
int shim_obs_predict(const double *cam8, int n, const float *pts, const int *ids, int n_feat, const int *feature_id, const int *start_frame, const int *n_obs,
                     const double *depth, const double *obs0, int frame_count, const double *poses, const double *tic_ric, const double *next_pose, float *predict_pts) {
  return obs_host_predict(cam8, n, pts, ids, n_feat, feature_id, start_frame, n_obs, depth, obs0, frame_count, poses, tic_ric, next_pose, predict_pts);
}
// the host path of a frame for n_cam cameras on one thread (tools/diag_obs_bench.py): lists packed over the cameras by offset
void shim_obs_observe_all(int n_cam, const double *cams, const int *offset, const float *pts, const int *ids, const int *prev_offset, const int *prev_ids,
                          const float *prev_un, const double *dt, const unsigned short *depth, int cols, int rows, int *ids_out, double *obs8, float *un_out,
                          int *counters) {
  for (int k = 0; k < n_cam; k++) {
    const int a = offset[k], n = offset[k + 1] - a, pa = prev_offset[k], pn = prev_offset[k + 1] - pa;
    obs_host_observe(cams + 8 * k, n, pts + 2 * a, ids + a, pn, prev_ids + pa, prev_un + 2 * pa, dt[k], depth ? depth + (size_t)k * (size_t)rows * (size_t)cols : nullptr,
                     cols, rows, ids_out + a, obs8 + (size_t)OBS_OW * (size_t)a, un_out + 2 * a, counters + 4 * k);
  }
}
}
