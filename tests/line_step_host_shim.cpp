// tests/line_step_host_shim.cpp — TEST HARNESS ONLY. Compiles the per-line device functions of the step half of a joint iteration
// (ground-fusion2_amd/csrc/gfbe_line.h: line_step_shares, line_dogleg, line_step_candidate; gfbe_factors.h: pose_plus) for the HOST so
// that tests/test_line_step_host.py can pin them against tests/line_step_np.py without a GPU. Never loaded by the package.
#include "../ground-fusion2_amd/csrc/gfbe_factors.h"
#include "../ground-fusion2_amd/csrc/gfbe_line.h"

using namespace gfd;

extern "C" {
// the line as k_line_step's thread forms it: line_plucker [6] in the start frame's camera -> orth [4]
void shim_line_orth(const double *pose77, const double *ex7, const double *plk, int start, double *x) {
  const LineRT B = line_make_pose(pose77 + 7 * start), E = line_make_pose(ex7);
  double lw[6];
  line_plk_to_pose(plk, mul(B.R, E.R), add(B.t, mv(B.R, E.t)), lw);
  line_plk_to_orth(lw, x);
}
void shim_step_shares(const double *W, const double *Vinv, const double *bl, const double *Vlow, const double *yp, const double *vp,
                      const double *x, double *yl, double *vl, double *p) {
  line_step_shares(W, Vinv, bl, Vlow, yp, vp, x, yl, vl, p);
}
int shim_dogleg(const double *T, double radius, double *coef) { return line_dogleg(T, radius, coef); }
void shim_pose_plus(const double *x7, const double *d6, double *y7) { pose_plus(x7, d6, nullptr, y7); }
// candidate poses [11][7] and extrinsic [7] given; returns the line's candidate cost, xc [4], plk [6]
double shim_step_candidate(const double *pose77_c, const double *ex7_c, const double *x, const double *yl, const double *vl, double c1,
                           double c2, int start, int m, const double *obs, double sqrt_info, double huber, double *xc, double *plk) {
  LineRT Bc[11], Exc = line_make_pose(ex7_c), Cs;
  for (int i = 0; i < 11; i++) Bc[i] = line_make_pose(pose77_c + 7 * i);
  Cs.R = mul(Bc[start].R, Exc.R);
  Cs.t = add(Bc[start].t, mv(Bc[start].R, Exc.t));
  return line_step_candidate(Bc, Exc, Cs, x, yl, vl, c1, c2, start, m, obs, sqrt_info, huber, xc, plk);
}
}
