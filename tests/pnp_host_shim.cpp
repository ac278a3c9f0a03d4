// TEST INFRASTRUCTURE. ground-fusion2_amd/csrc/gfbe_pnp.h compiled for the host with a plain C++ compiler (no HIP): the same text the
// kernels of gfbe_pnp.hip compile for the device, behind C entry points for tests/test_pnp_model.py and tools/diag_pnp_bench.py.
#include "../ground-fusion2_amd/csrc/gfbe_pnp.h"

using namespace gfd;

extern "C" {

uint64_t shim_pnp_hash(uint64_t seed, int h, int k) { return pnp_hash(seed, h, k); }
int shim_pnp_sample(uint64_t seed, int h, int n, int32_t *idx3) { return pnp_sample(seed, h, n, idx3); }
int shim_pnp_p3p(const double *X9, const double *uv6, double *out48) { return pnp_p3p(X9, uv6, out48); }
int shim_pnp_solve6(const double *acc27, double *d6) { return pnp_solve6(acc27, d6) ? 1 : 0; }
void shim_pnp_rot_to_quat(const double *R9, double *q4) { pnp_rot_to_quat(R9, q4); }
double shim_pnp_normalize_angle(double a) { return pnp_normalize_angle(a); }

// V1 .. V8 of B problems on one thread; the outputs of gfbe_pnp_verify (any may be null), ints [B][4] = n_inliers, has_loop, best h, best s
void shim_pnp_verify(int B, const int32_t *offset, const float *point_3d, const float *pt_norm, const double *pose_cur, const double *tic_qic, int iterations, int refine_iterations,
                     int min_loop_num, uint64_t seed, double reproj_threshold, double max_yaw_deg, double max_translation, uint8_t *status, int32_t *n_inliers, int32_t *has_loop,
                     double *loop_info, double *pnp_pose, int32_t *best, int32_t *refine_flag, int32_t *sample_idx, int32_t *n_solutions, double *hyp_pose, int32_t *hyp_count) {
  PnpParams P;
  P.iterations = iterations; P.refine_iterations = refine_iterations; P.min_loop_num = min_loop_num; P.pad = 0; P.seed = seed; P.thr2 = reproj_threshold * reproj_threshold;
  const size_t H = (size_t)iterations;
  for (int b = 0; b < B; b++) {
    const size_t o = (size_t)offset[b], bb = (size_t)b;
    const PnpHostOut r = pnp_host_problem(P, max_yaw_deg, max_translation, offset[b + 1] - offset[b], point_3d + 3 * o, pt_norm + 2 * o, pose_cur + 12 * bb, tic_qic + 12 * bb,
                                          status ? status + o : nullptr, sample_idx ? sample_idx + 3 * H * bb : nullptr, n_solutions ? n_solutions + H * bb : nullptr,
                                          hyp_pose ? hyp_pose + 48 * H * bb : nullptr, hyp_count ? hyp_count + 4 * H * bb : nullptr);
    if (n_inliers) n_inliers[b] = r.n_inliers;
    if (has_loop) has_loop[b] = r.has_loop;
    if (loop_info) for (int a = 0; a < 8; a++) loop_info[8 * bb + a] = r.loop_info[a];
    if (pnp_pose) for (int a = 0; a < 12; a++) pnp_pose[12 * bb + a] = r.res[7 + a];
    if (best) { best[2 * bb] = r.best_h; best[2 * bb + 1] = r.best_s; }
    if (refine_flag) refine_flag[b] = r.refine_flag;
  }
}

}  // extern "C"
