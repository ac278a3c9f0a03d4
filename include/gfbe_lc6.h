/*
 * gfbe_lc6.h — loop-closure pose graph of dense_map, the 6-DoF solve that runs on VO input (a deployment without an IMU:
 * PoseGraph::setIMUFlag, dense_map/src/pose_graph.cpp:56-69, starts optimize6DoF instead of optimize4DoF). The symbols
 * live in libgfbe.so; this companion header keeps them apart from the surface of gfbe.h (f3b is the 4-DoF solve).
 *
 *       PoseGraph::optimize6DoF             dense_map/src/pose_graph.cpp:707-873 (options :736-745)
 *       RelativeRTError                     dense_map/src/pose_graph.h:290-352 (automatic differentiation in the
 *                                           reference; analytic tangent Jacobians here)
 *
 * A keyframe is t(3) and q(4) in the order w, x, y, z (q_array, :763-766), unit. The full rotation is free.
 * Tangent of a pose: [dq(3), t(3)] — Ceres adds q_array[i] before t_array[i] (:770-771).
 * Step (ceres::QuaternionParameterization::Plus, :745): q <- [cos|d|, sin|d| / |d| d] * q, d = 0 leaves q as it is; t <- t + dt.
 * There is no renormalisation, as in Ceres.
 * Residual (pose_graph.h:300-337): r[0..2] = (R(q_i)^T (t_j - t_i) - meas_t) / t_var through the rotation matrix of the
 * normalised q_i, products left to right per row; r[3..5] = 2 vec(meas_q^-1 (q_i^-1 q_j)) / q_var, inverses as conjugates
 * (QuaternionInverse), with no sign normalisation of the error's w: the reference has none either.
 * Edge kinds: 0 = a sequence edge with no loss (:792), 1 = a loop edge through the corrector of HuberLoss(huber_delta)
 * (:743, :809).
 *
 * gfbe_lc6_eval: an explicit edge list (edge_i, edge_j) of distinct poses, meas [n_edges][7] = t(3) | q(w, x, y, z).
 * Returns r [n_edges][6], J [n_edges][6][12] (columns dq_i t_i dq_j t_j; kind 1 through the corrector) and the cost with the
 * loss. Any output pointer may be NULL.
 *
 * gfbe_lc6_solve: the graph optimize6DoF builds. t [n][3] / q [n][4] are the VO poses: the starting point AND the source of
 * the sequence measurements — for every i and k = 1 .. span with sequence[i] == sequence[i - k] (:780-794) an edge (i - k, i)
 * with relative_t = R(q_{i-k})^T (t_i - t_{i-k}), through the rotation matrix, products left to right per row, and
 * relative_q = q_{i-k}^-1 * q_i (the conjugate), formed by the library in FP64: the convention gfbe_lc4_solve states.
 * fixed[i] != 0: the pose is constant (the caller sets it for the earliest looped keyframe and for sequence 0, :773-777).
 * Loop edges (loop_c[l], loop_i[l]) with loop_c < loop_i, at most one per loop_i (:798-810), loop_meas [n_loop][7] =
 * relative t | relative q (w, x, y, z). At most GFBE_LC6_MAX_LOOPS loop edges.
 * Deviations carried over from gfbe_lc4_solve unchanged: a pose out of the problem (constant, or on no
 * edge with a free pose) is an identity row of the system; an edge between two constant poses is dropped.
 * Solver: the statements of gfbe_lc4_solve — what ceres::Solve does with the reference's options (:736-745):
 * Levenberg-Marquardt, Jacobi scaling, Ceres 1.14 defaults, the normal equations solved exactly. They are block-tridiagonal
 * in 32 x 32 super-blocks of four poses (a pose takes 8 rows: its 6 tangent dimensions and 2 identity rows) plus a rank-6
 * term per loop edge: parallel block cyclic reduction with the loop columns as right-hand sides, then the 6 n_loop
 * capacitance system.
 * Outputs: t_out [n][3], q_out [n][4]; drift[7] = q_drift (w, x, y, z) | t_drift of the last keyframe (:849-850; may be
 * NULL): q_drift = q_out[n-1] * q_in[n-1]^-1, t_drift = t_out[n-1] - R(q_drift) t_in[n-1]; summary as gfbe_pg_solve
 * fills it (may be NULL). Applying the drift to later keyframes (:855-864) stays with the caller, as with gfbe_lc4_solve.
 * Failure contract: GFBE_BAD_INPUT with nothing written for n_loop > GFBE_LC6_MAX_LOOPS, an index out of range,
 * loop_c >= loop_i, two loops on one loop_i, a non-finite pose or measurement, or an options struct of another size;
 * GFBE_NO_DEVICE without a GPU (gfbe_last_error: "no CPU fallback"). A pivot that is not positive makes the step invalid,
 * as in gfbe_lc4_solve: the radius shrinks, five invalid steps in a row end the solve with GFBE_NUMERICAL_FAILURE.
 * Device scratch of a call (grow-only, owned by the context), in doubles, with rows = 32 ceil(n / 4),
 * ld = 16 ceil((1 + 6 n_loop) / 16) and cap_ld = 16 ceil(6 n_loop / 16):
 *     2 rows ld  (the two panels)  +  2 cap_ld^2  (S and L)  +  about 650 rows + 300 n_loop + 18 cap_ld  (band sets, vectors)
 * At n = 5000, n_loop = 128: 2 x 40 000 x 784 + 2 x 768^2 doubles = 0.51 GB for panels, S and L, 0.72 GB with the rest; a
 * failed allocation is GFBE_DEVICE_ERROR.
 */
#ifndef GFBE_LC6_H_
#define GFBE_LC6_H_
#include "gfbe.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GFBE_LC6_MAX_LOOPS 128
typedef struct gfbe_lc6_options {
  int32_t struct_size;          /* sizeof(gfbe_lc6_options), written by gfbe_lc6_default_options */
  int32_t max_num_iterations;   /* 5 (pose_graph.cpp:740); at most 15 are run */
  int32_t span;                 /* 4 (:780): sequence edges reach this many keyframes back, 1 .. 4 */
  int32_t reserved;
  double huber_delta;           /* 0.1 (:743), loop edges only */
  double t_var, q_var;          /* 0.1, 0.01 (:791, :808) */
} gfbe_lc6_options;
void gfbe_lc6_default_options(gfbe_lc6_options *opt);
gfbe_status gfbe_lc6_eval(gfbe_ctx *ctx, const gfbe_lc6_options *opt /* NULL: defaults */, int32_t n_poses, const double *t,
                          const double *q, int32_t n_edges, const int32_t *edge_i, const int32_t *edge_j,
                          const uint8_t *kind, const double *meas, double *r, double *J, double *cost);
gfbe_status gfbe_lc6_solve(gfbe_ctx *ctx, const gfbe_lc6_options *opt /* NULL: defaults */, int32_t n_poses, const double *t,
                           const double *q, const int32_t *sequence, const uint8_t *fixed, int32_t n_loop,
                           const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out,
                           double *q_out, double *drift, gfbe_summary *summary);
#ifdef __cplusplus
}
#endif
#endif
