// TEST INFRASTRUCTURE. ground-fusion2_amd/csrc/gfbe_gate.h compiled for the host with a plain C++ compiler (no HIP): the same text the
// kernels of gfbe_gate.hip compile for the device, behind C entry points for tests/test_gate_model.py and tools/diag_gate_bench.py.
// iopt [4] = use_wheel, wdetect, min_pair_count, mode; dopt [10] = the ten double fields of gfbe_gate_options in their order.
#include "../ground-fusion2_amd/csrc/gfbe_gate.h"

using namespace gfd;

namespace {
GateParams params(const int32_t *iopt, const double *d) {
  GateParams G;
  G.use_wheel = iopt[0]; G.wdetect = iopt[1]; G.min_pair_count = iopt[2]; G.pad = 0;
  G.dis_threshold = d[0]; G.wheel_still_norm = d[1]; G.preint_still_norm = d[2]; G.var_still = d[3]; G.var_excited = d[4]; G.still_parallax_px = d[5];
  G.init_parallax_px = d[6]; G.parallax_focal = d[7]; G.depth_min = d[8]; G.depth_max = d[9];
  return G;
}
}  // namespace

extern "C" {

void shim_gate_delta_rot(const double *theta3, double *M9) { gate_delta_rot(theta3[0], theta3[1], theta3[2], M9); }
double shim_gate_var(const double *frames, int M) { return gate_var(frames, M); }

// gfbe_gate_frame of B robots on one thread; the tables packed: table b at rows toff[b] .. toff[b + 1]
void shim_gate_frame(const int32_t *iopt, const double *dopt, int B, const int32_t *toff, const int32_t *start, const int32_t *nobs, const double *obs, const int32_t *frame_count,
                     const int32_t *imu_off, const double *imu, const double *imu_first, const int32_t *wheel_off, const double *wheel, const double *wheel_first, const double *pose,
                     const double *vel_ba, double g_norm, const int32_t *stationary_prev, const int32_t *frames_off, const double *frames, int32_t *flags, int32_t *l_still,
                     int32_t *l_init, int32_t *pair_count, double *pair_sum, double *dP_imu, double *dP_wheel, double *dis, double *var, double *pose_out, double *vel_out) {
  gate_frame_host(params(iopt, dopt), iopt[3], B, toff, start, nobs, obs, frame_count, imu_off, imu, imu_first, wheel_off, wheel, wheel_first, pose, vel_ba, g_norm,
                  stationary_prev, frames_off, frames, flags, l_still, l_init, pair_count, pair_sum, dP_imu, dP_wheel, dis, var, pose_out, vel_out);
}

void shim_gate_pair_stats(const int32_t *iopt, const double *dopt, int B, const int32_t *toff, const int32_t *start, const int32_t *nobs, const double *obs, int32_t *pair_count,
                          double *pair_sum, int32_t *l_still, int32_t *l_init) {
  const GateParams G = params(iopt, dopt);
  for (int b = 0; b < B; b++) {
    gate_pairs_host(G, iopt[3], toff[b + 1] - toff[b], start + toff[b], nobs + toff[b], obs + (size_t)toff[b] * GATE_NOBS * GATE_OW, pair_count + GATE_NL * (size_t)b,
                    pair_sum + GATE_NL * (size_t)b);
    gate_decide(G, pair_count + GATE_NL * (size_t)b, pair_sum + GATE_NL * (size_t)b, l_still + b, l_init + b);
  }
}

int shim_gate_corresponding(const int32_t *iopt, const double *dopt, int n, const int32_t *start, const int32_t *nobs, const double *obs, int l, int r, int room, double *a3,
                            double *b3) {
  return gate_corres_host(params(iopt, dopt), iopt[3], n, start, nobs, obs, l, r, room, a3, b3);
}

}  // extern "C"
