// tests/line_reduce_host_shim.cpp — TEST HARNESS ONLY. Compiles the per-line device functions of the reduced line normal equations
// (ground-fusion2_amd/csrc/gfbe_line.h: line_huber, line_chol4_inv, line_reduce_line, line_Y_row) for the HOST so that
// tests/test_line_reduce_host.py can pin them against tests/line_reduce_np.py without a GPU. Never loaded by the package.
#include "../ground-fusion2_amd/csrc/gfbe_line.h"

using namespace gfd;

extern "C" {
double shim_huber(double s, double a, double *sqrt_rho1) { return line_huber(s, a, sqrt_rho1); }
int shim_chol4_inv(const double *V, double mu, double *Vinv) { return line_chol4_inv(V, mu, Vinv) ? 1 : 0; }
// One line as k_line_reduce's thread sees it: poses [11][7], ex [7], line_plucker [6] in the start frame's camera frame.
// Wrow [72][4], Jrec [11][26], Vinv [16], bl [4], cost, Y [72][4] = W V'^-1. Returns 1 when V' has a Cholesky factor.
int shim_reduce_line(const double *pose77, const double *ex7, const double *plk, int start, int k0, int m, const double *obs,
                     double sqrt_info, double huber, double mu, double *Wrow, double *Jrec, double *Vinv, double *bl, double *cost, double *Y) {
  LineRT Bs[11], Ex = line_make_pose(ex7);
  for (int i = 0; i < 11; i++) Bs[i] = line_make_pose(pose77 + 7 * i);
  const mat3 Rwc = mul(Bs[start].R, Ex.R);
  const vec3 twc = add(Bs[start].t, mv(Bs[start].R, Ex.t));
  double lw[6], x[4];
  line_plk_to_pose(plk, Rwc, twc, lw);
  line_plk_to_orth(lw, x);
  const bool ok = line_reduce_line(Bs, Ex, x, start, k0, m, obs, sqrt_info, huber, mu, Wrow, Jrec, Vinv, bl, cost);
  if (ok) for (int r = 0; r < LINE_NP; r++) line_Y_row(Wrow + 4 * r, Vinv, Y + 4 * r);
  return ok ? 1 : 0;
}
}
