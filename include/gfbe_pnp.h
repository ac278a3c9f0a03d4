/*
 * gfbe_pnp.h — the loop verification on the device: the second half of KeyFrame::findConnection, between gfbe_ldb_match / gfbe_kfd_match
 * (the matched lists) and a loop edge of gfbe_lc4_solve / gfbe_lc6_solve. A batch of problems, each n pairs of a world point and a
 * normalised observation in the old keyframe, goes through a P3P RANSAC, a refit on the inliers, the loop_info arithmetic and the
 * acceptance test; find_connection chains rule 6 of the loop database, reduceVector, the gather of the window's points and all of that
 * behind one host wait. The symbols live in libgfbe.so; this companion header keeps them apart from the other surfaces.
 *
 *       KeyFrame::PnPRANSAC (cv::solvePnPRansac)                   dense_map/src/keyframe.cpp:273-329
 *       KeyFrame::findConnection, loop_info and its test           :479-565
 *       Utility::R2ypr, Utility::normalizeAngle                    dense_map/src/utility/utility.cpp, utility.h:140-148
 *
 * The stage is unpinned against the reference, like gfbe_kfd: cv::RNG's stream, OpenCV's minimal solver and its iterative refit are not
 * reproduced (nothing of OpenCV was at hand to run). It is pinned bit for bit against the model tests/pnp_np.py: every rule is plain FP64
 * arithmetic (+ - * /, sqrt, fabs, comparisons) written once in ground-fusion2_amd/csrc/gfbe_pnp.h and compiled for device and host
 * without contraction.
 *
 * V1 inputs of one problem. n pairs: point_3d float [n][3] (world, cv::Point3f) and pt_norm float [n][2] (the old keyframe's
 *    keypoints_norm), both converted to double once. pose_cur double [12] = origin_vio_T, then origin_vio_R row-major; tic_qic double [12]
 *    = tic, then qic row-major. n <= min_loop_num (25, keyframe.h:29; the reference tests >): no PnP runs and the problem gives
 *    has_loop 0, n_inliers 0, status all 0, loop_info 8 zeros, pnp_pose 12 zeros, best (-1, -1), refine_flag 0. n above max_points:
 *    GFBE_BAD_INPUT.
 * V2 samples (:305: 100 iterations). Hypothesis h = 0 .. iterations - 1 draws k = 0, 1, 2, ... by a counter-based hash with 64-bit
 *    wraparound: z = seed + 0x9E3779B97F4A7C15 * (1 + 256 h + k); z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *    z *= 0x94D049BB133111EB; z ^= z >> 31; idx = z mod n. A draw equal to an index already accepted is skipped; three accepted indices
 *    make the sample; k stops at 64, and a hypothesis that has not filled its sample by then has no solution (sample_idx -1 where
 *    unfilled). Deviation: cv::RNG's stream and OpenCV's 5-point EPnP minimal solver are not reproduced.
 * V3 P3P. From the three pairs, up to four poses (R, t) with Xc = R Xw + t and positive depths of the three sample points. With unit
 *    bearings y_i = (u, v, 1) / |(u, v, 1)|, b_ij = y_i . y_j and a_ij = |X_i - X_j|^2 the depths l_i satisfy l_i^2 + l_j^2 - 2 b_ij l_i l_j
 *    = a_ij. The conics D1 = M12 a23 - M23 a12 and D2 = M13 a23 - M23 a13 in (l_1 : l_2 : l_3) share the solutions. A real root g of the
 *    cubic det(D1 + g D2) is found by 100 halvings of [-r, r], r = 1 + max(|c0|, |c1|, |c2|) / |c3|; D0 = D1 + g D2 is a pair of lines:
 *    B = -adj(D0) = p p^T gives p from the column of the largest diagonal entry (B_jj <= 0: no solution), C = D0 + [p]x has rank one, the
 *    row and the column through its entry of largest magnitude (the first in row-major order) are line 0 and line 1. A line is solved for
 *    its component of largest magnitude and cut with D2 when |g| <= 1, else D1: a quadratic with roots + and - (a negative discriminant:
 *    none). The ratio is scaled by a12, the sign taken so that l_1 > 0, and a solution is kept iff all three depths are positive; R, t
 *    follow from Y [d12 d13 d12 x d13]^-1 on the camera-side and world-side edges and are kept iff finite. Order: line 0 +, line 0 -,
 *    line 1 +, line 1 -. Degenerate samples give zero solutions: |d12 x d13|^2 <= 1e-12 |d12|^2 |d13|^2 (two equal points, points on
 *    a line), or a non-finite intermediate. R is orthonormal only by the construction, never re-projected.
 * V4 score (:305: reprojectionError 10.0 / 460.0). For every solution and every point of the problem, point i is an inlier iff
 *    Xc.z > 0 and (Xc.x / Xc.z - u)^2 + (Xc.y / Xc.z - v)^2 <= thr * thr. Deviations: the reference computes the error in float and
 *    does not test Xc.z.
 * V5 select. The winner is the solution with the largest count; ties go to the lower h, then the lower solution index. All hypotheses
 *    are scored. Deviation: the reference's confidence-driven early stop (0.99) is not reproduced. No solution anywhere gives V1's
 *    outputs of a problem without PnP. status [i] = the winner's inlier mask (:309-316), n_inliers its count.
 * V6 refine, in the place of the SOLVEPNP_ITERATIVE refit. refine_iterations Gauss-Newton steps on the winner's inliers from the
 *    winner's pose: state a unit quaternion (from R by V7's conversion) and t; residual the two normalised-plane differences;
 *    perturbation Xc' = Xc + dtheta x Xc + dt. The 21 + 6 sums of the normal equations run over the inliers in ascending point index:
 *    lane l of 64 sums the inliers l, l + 64, ... from 0.0, then s = s + shfl_xor(s, off) for off = 32, 16, 8, 4, 2, 1. The 6 x 6 system
 *    is solved by L D L^T without pivoting; a pivot <= 0 or non-finite ends the refinement, keeps the pose before that step and sets
 *    refine_flag. Update: dq = normalize(1, dtheta / 2), q <- dq q renormalised, t <- R(dq) t + dt, R <- R(q). No trigonometry.
 * V7 loop_info (:318-327, :547-560). R_w_c_old = R^T, T_w_c_old = R_w_c_old (-t); PnP_R_old = R_w_c_old qic^T, PnP_T_old = T_w_c_old -
 *    PnP_R_old tic; relative_t = PnP_R_old^T (origin_vio_T - PnP_T_old); relative_q = the quaternion of M = PnP_R_old^T origin_vio_R by
 *    Eigen's rule: with tr = M00 + M11 + M22 > 0, s = sqrt(tr + 1), w = s / 2, (x y z) = (M21 - M12, M02 - M20, M10 - M01) * (0.5 / s);
 *    else i = the largest diagonal entry (the first of equal ones), j, k the next two cyclically, s = sqrt(Mii - Mjj - Mkk + 1),
 *    q_i = s / 2, w = (Mkj - Mjk) * (0.5 / s), q_j = (Mji + Mij) * (0.5 / s), q_k = (Mki + Mik) * (0.5 / s). relative_yaw =
 *    normalizeAngle(yaw(origin_vio_R) - yaw(PnP_R_old)), yaw(R) = atan2(R10, R00) / M_PI * 180.0: the two atan2 are the stage's only
 *    libm calls and are taken on the host, from the doubles the call brings back. loop_info = t.x t.y t.z q.w q.x q.y q.z yaw.
 * V8 decision (:545-565). has_loop iff n_inliers > min_loop_num, fabs(relative_yaw) < max_yaw_deg (30.0) and |relative_t| <
 *    max_translation (20.0). loop_info is written only then, otherwise it is 8 zeros (keyframe.cpp:46). pnp_pose = PnP_T_old, PnP_R_old
 *    is written whenever a winner exists.
 * Not covered: FundmantalMatrixRANSAC (dead in the reference), the debug image, camera models other than the normalised plane.
 *
 *   verify               a batch of n_problems problems from host arrays: offset [n_problems + 1] (from 0, ascending), point_3d [n][3],
 *                        pt_norm [n][2], pose_cur / tic_qic [n_problems][12]. One host wait. Outputs (any may be NULL): status [n],
 *                        n_inliers / has_loop / refine_flag [n_problems], loop_info [n_problems][8], pnp_pose [n_problems][12], best
 *                        [n_problems][2] = h, solution; for narrow tests sample_idx [n_problems][H][3], n_solutions [n_problems][H],
 *                        hyp_pose [n_problems][H][4][12] (t, then R; unused rows zero), hyp_count [n_problems][H][4], H = iterations.
 *   find_connection      rule 6 of the loop database and reduceVector on n_window window descriptors against held keyframe old_index
 *                        (gfbe_ldb_match), the gather of point_3d [n_window][3] by matched_src, and V1 .. V8 on the matches, on the
 *                        device with one wait: the kernels are sized by n_window and read the count from device memory. Outputs (any may
 *                        be NULL): n_matched, matched_src [n_matched], matched_pt / matched_pt_norm [n_matched][2] as gfbe_ldb_match's
 *                        (room for n_window rows), status_pnp [n_matched], then n_inliers, has_loop, loop_info [8], pnp_pose [12],
 *                        best [2], refine_flag of the one problem. n_window at most max_points.
 *   find_connection_kfd  the same on camera's window descriptors of the last gfbe_kfd_describe; no descriptor crosses the bus.
 * Failure contract: GFBE_BAD_INPUT with nothing written and no state changed for an options struct of another size or a field out of
 * range, n_problems outside 0 .. max_problems, offsets that do not ascend from 0, a problem above max_points, n_window above max_points,
 * old_index that is no held keyframe, a camera outside the describer's or a describer without window descriptors, a handle of another
 * context, a NULL required argument; GFBE_NO_DEVICE without a GPU (gfbe_last_error: "no CPU fallback").
 */
#ifndef GFBE_PNP_H_
#define GFBE_PNP_H_
#include "gfbe.h"
#include "gfbe_kfd.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct gfbe_pnp gfbe_pnp;
typedef struct gfbe_pnp_options {
  int32_t struct_size;             /* sizeof(gfbe_pnp_options), written by gfbe_pnp_default_options */
  int32_t max_problems;            /* 64; problems of one verify, 1 .. 4096 */
  int32_t max_points;              /* 4096; points of a problem, 1 .. 4096 */
  int32_t iterations;              /* 100 (keyframe.cpp:305); hypotheses of a problem, 1 .. 1024 */
  int32_t refine_iterations;       /* 5; Gauss-Newton steps of V6, 0 .. 20 */
  int32_t min_loop_num;            /* 25 (keyframe.h:29), >= 0 */
  uint64_t seed;                   /* 0; V2 */
  double reproj_threshold;         /* 10.0 / 460.0 (keyframe.cpp:305), finite and > 0 */
  double max_yaw_deg;              /* 30.0 (keyframe.cpp:553), finite */
  double max_translation;          /* 20.0 (keyframe.cpp:553), finite */
} gfbe_pnp_options;
void gfbe_pnp_default_options(gfbe_pnp_options *opt);
gfbe_status gfbe_pnp_create(gfbe_ctx *ctx, const gfbe_pnp_options *opt /* NULL: defaults */, gfbe_pnp **out);
void gfbe_pnp_destroy(gfbe_ctx *ctx, gfbe_pnp *h);
gfbe_status gfbe_pnp_verify(gfbe_ctx *ctx, gfbe_pnp *h, int32_t n_problems, const int32_t *offset, const float *point_3d, const float *pt_norm, const double *pose_cur,
                            const double *tic_qic, uint8_t *status, int32_t *n_inliers, int32_t *has_loop, double *loop_info, double *pnp_pose, int32_t *best,
                            int32_t *refine_flag, int32_t *sample_idx, int32_t *n_solutions, double *hyp_pose, int32_t *hyp_count);
gfbe_status gfbe_pnp_find_connection(gfbe_ctx *ctx, gfbe_pnp *h, gfbe_ldb *db, int32_t old_index, int32_t n_window, const uint64_t *window_desc, const float *point_3d,
                                     const double *pose_cur, const double *tic_qic, int32_t *n_matched, int32_t *matched_src, float *matched_pt, float *matched_pt_norm,
                                     uint8_t *status_pnp, int32_t *n_inliers, int32_t *has_loop, double *loop_info, double *pnp_pose, int32_t *best, int32_t *refine_flag);
gfbe_status gfbe_pnp_find_connection_kfd(gfbe_ctx *ctx, gfbe_pnp *h, gfbe_kfd *kfd, int32_t camera, gfbe_ldb *db, int32_t old_index, const float *point_3d,
                                         const double *pose_cur, const double *tic_qic, int32_t *n_matched, int32_t *matched_src, float *matched_pt, float *matched_pt_norm,
                                         uint8_t *status_pnp, int32_t *n_inliers, int32_t *has_loop, double *loop_info, double *pnp_pose, int32_t *best, int32_t *refine_flag);
#ifdef __cplusplus
}
#endif
#endif
