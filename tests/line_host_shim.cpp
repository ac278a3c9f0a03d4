// tests/line_host_shim.cpp — TEST HARNESS ONLY. Compiles the product's __host__ __device__ line arithmetic
// (ground-fusion2_amd/csrc/gfbe_line.h) for the HOST so that tests/test_line_host.py can pin it against tests/line_np.py without a GPU.
// Never loaded by the package: the product calls these functions only from the kernels of gfbe_line.hip.
#include "../ground-fusion2_amd/csrc/gfbe_line.h"

using namespace gfd;

extern "C" {
void shim_orth_to_plk(const double *o, double *plk) { line_orth_to_plk(o, plk); }
void shim_plk_to_orth(const double *plk, double *o) { line_plk_to_orth(plk, o); }
void shim_plk_to_pose(const double *plk, const double *p7, double *out) {   // (R, t) of the pose [p | q]
  const LineRT P = line_make_pose(p7);
  line_plk_to_pose(plk, P.R, P.t, out);
}
void shim_plk_from_pose(const double *plk, const double *p7, double *out) {
  const LineRT P = line_make_pose(p7);
  line_plk_from_pose(plk, P.R, P.t, out);
}
void shim_orth_plus(const double *x, const double *d, double *out) { line_orth_plus(x, d, out); }
void shim_line_factor(const double *pose, const double *ex, const double *orth, const double *obs, double sqrt_info, double *r, double *Jp,
                      double *Je, double *Jo) {
  line_factor<true>(line_make_pose(pose), line_make_pose(ex), orth, obs, sqrt_info, r, Jp, Je, Jo);
}
double shim_cauchy(double s, double a, double *sqrt_rho1) { return line_cauchy(s, a, sqrt_rho1); }
int shim_endpoints_bad(const double *plk_c, const double *obs0) { return line_endpoints_bad(plk_c, obs0) ? 1 : 0; }
double shim_reprojection_error(const double *obs, const double *cam7, const double *line_w) {   // camera pose [twc | q_wc]
  const LineRT C = line_make_pose(cam7);
  return line_reprojection_error(obs, C.R, C.t, line_w);
}
}
