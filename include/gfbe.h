/*
 * gfbe.h — C ABI of the MI355X-native sliding-window visual-inertial-wheel back end.
 *
 * This is the drop-in boundary for ONE hot path of sjtuyinjie/Ground-Fusion2:
 *   Ground-Fusion++/vins_estimator/src/estimator/estimator.cpp:2951-3698  (Estimator::optimization())
 * A maintainer binds these entry points from Estimator::optimization();
 * everything else in the reference (ROS node, front end, LIO, mapping) is untouched.
 *
 * Conventions (identical to the reference's parameter blocks, estimator.h:230-238,336-342):
 *   pose block       = [px py pz qx qy qz qw]            (estimator.cpp:2341-2348)
 *   speed-bias block = [vx vy vz bax bay baz bgx bgy bgz] (estimator.cpp:2352-2362)
 *   quaternions are x,y,z,w inside every block.
 *   tangent order per pose = (dP, dtheta) with right perturbation q <- q * [1, dtheta/2]
 *   (pose_local_parameterization.cpp:12-36).
 * All floating point is FP64; all indices are int32. Plain pointers + sizes only: no C++/torch
 * types cross this boundary. Memory passed in is caller-owned host memory unless a function
 * name says "_dev". One gfbe_ctx per Estimator; a ctx is thread-compatible (one call at a time).
 */
#ifndef GFBE_H_
#define GFBE_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFBE_WINDOW_SIZE 10 /* parameters.h:24 */
#define GFBE_NFRAMES 11     /* WINDOW_SIZE + 1 */
#define GFBE_MAX_OBS 11     /* a landmark has at most one observation per frame */
#define GFBE_DENSE_DIM 246  /* tangent dims of the non-landmark blocks: 11*6 + 11*9 + 6 + 6 + 3 + 1 + 1 + 4 + 1 of the ground
                               plane (para_plane_R is marginalised as a 4-D block without a manifold, marginalization_factor.cpp:140-143:
                               four prior columns) = 187, + 3 + 1 + 44 + 11 of the GNSS blocks (anc_ecef, yaw_enu_local, rcv_dt, rcv_ddt) */
#define GFBE_CORE_DIM 187   /* the tangent dims without the GNSS blocks */
#define GFBE_MAX_PRIOR_BLOCKS 32

typedef enum gfbe_status {
  GFBE_OK = 0,
  GFBE_NO_CONVERGENCE = 1,   /* ran out of iterations (normal for an 8-iteration budget) */
  GFBE_NUMERICAL_FAILURE = 2,/* linear solve failed for every mu < max_mu, or NaN */
  GFBE_BAD_INPUT = 3,
  GFBE_DEVICE_ERROR = 4,
  GFBE_NO_DEVICE = 5         /* HIP back end asked for, no GPU / kernels missing: fails loudly */
} gfbe_status;

/* Symbolic parameter-block ids. They replace the raw double* addresses the reference uses as
 * block identity (marginalization_factor.cpp:104-116, estimator.cpp:3561-3588 addr_shift). */
enum {
  GFBE_BLK_POSE0 = 0,   /* .. GFBE_BLK_POSE0+10  para_Pose[i]      size 7 */
  GFBE_BLK_SB0 = 11,    /* .. GFBE_BLK_SB0+10    para_SpeedBias[i] size 9 */
  GFBE_BLK_EX_CAM = 22, /* para_Ex_Pose[0]       size 7 */
  GFBE_BLK_EX_WHEEL = 23, /* para_Ex_Pose_wheel[0] size 7 */
  GFBE_BLK_SX = 24, GFBE_BLK_SY = 25, GFBE_BLK_SW = 26, /* para_Ix_s{x,y,w}_wheel size 1 */
  GFBE_BLK_TD = 27,     /* para_Td       size 1 */
  GFBE_BLK_TD_WHEEL = 28, /* para_Td_wheel size 1 */
  GFBE_BLK_PLANE_R = 29,  /* para_plane_R  size 4 (quaternion x y z w, OrientationSubsetParameterization({2}): estimator.cpp:3120-3123) */
  GFBE_BLK_PLANE_Z = 30,  /* para_plane_Z  size 1 */
  /* GNSS blocks (estimator.h:306-309, estimator.cpp:2965-3002; only in the problem when gfbe_window.gnss_ready) */
  GFBE_BLK_ANC_ECEF = 31, /* para_anc_ecef       size 3 */
  GFBE_BLK_YAW_ENU = 32,  /* para_yaw_enu_local  size 1 — always SetParameterBlockConstant (estimator.cpp:2991) */
  GFBE_BLK_RCV_DT0 = 33,  /* .. +43: para_rcv_dt + 4 i + k (frame i, constellation k)  size 1 */
  GFBE_BLK_RCV_DDT0 = 77, /* .. +10: para_rcv_ddt + i                                  size 1 */
  GFBE_BLK_COUNT = 88
};

/* One GNSS observation of the window with everything GnssPsrDoppFactor's constructor derives from it (see f2 below). */
typedef struct gfbe_gnss_obs {
  double sv_pos[3], sv_vel[3];   /* satellite ECEF position / velocity at transmission time (:20-35) */
  double svdt, svddt, tgd;       /* satellite clock bias (s), drift (s/s), group delay (s) */
  double pr_uura, dp_uura;       /* pseudo-range / Doppler deviation scalings (:24-26, :38-40) */
  double psr, dopp;              /* obs->psr[freq_idx] (m), obs->dopp[freq_idx] (Hz) */
  double wavelength;             /* LIGHT_SPEED / freq (m) */
  double ratio;                  /* ts_ratio (estimator.cpp:3262): weight of frame lower_idx against lower_idx + 1 */
  double doy, tow;               /* time2doy(obs->time), time2gpst(obs->time): the atmosphere models' time arguments */
  int32_t frame;                 /* i of gnss_meas_buf[i]: uses rcv_dt[i][sys_idx] and rcv_ddt[i] */
  int32_t lower_idx;             /* the factor connects Pose / SpeedBias lower_idx and lower_idx + 1 */
  int32_t sys_idx;               /* gnss_comm::sys2idx: 0 GPS, 1 GLO, 2 GAL, 3 BDS */
  int32_t _pad;
} gfbe_gnss_obs;

typedef struct gfbe_gnss_state {   /* estimator.h: para_rcv_dt, para_rcv_ddt, para_yaw_enu_local, para_anc_ecef */
  double rcv_dt[GFBE_WINDOW_SIZE + 1][4];
  double rcv_ddt[GFBE_WINDOW_SIZE + 1];
  double yaw_enu_local;
  double anc_ecef[3];
} gfbe_gnss_state;

/* The dense ("camera side") parameter blocks of one window — what vector2double() fills
 * (estimator.cpp:2337-2414) and double2vector() reads back (estimator.cpp:2501-2630). */
typedef struct gfbe_state {
  double para_Pose[GFBE_NFRAMES][7];
  double para_SpeedBias[GFBE_NFRAMES][9];
  double para_Ex_Pose[7];        /* camera 0 (the only one optimization() wires: estimator.cpp:3351) */
  double para_Ex_Pose_wheel[7];
  double para_Ix_wheel[3];       /* sx, sy, sw */
  double para_Td;
  double para_Td_wheel;
  double para_plane_R[4];        /* ground plane in the world: rotation (x y z w) and height (estimator.h:233-236); used with use_plane */
  double para_plane_Z;
  gfbe_gnss_state gnss;          /* para_rcv_dt, para_rcv_ddt, para_yaw_enu_local, para_anc_ecef; used with gnss_ready */
} gfbe_state; /* 259 doubles */

/* What IMUFactor reads from IntegrationBase (imu_factor.h:69-90, integration_base.h:169-195). */
typedef struct gfbe_imu_preint {
  double sum_dt;
  double delta_p[3];
  double delta_q[4]; /* x y z w */
  double delta_v[3];
  double linearized_ba[3];
  double linearized_bg[3];
  double jacobian[225];   /* 15x15 row-major, order P,R,V,BA,BG (parameters.h:166-173) */
  double covariance[225]; /* 15x15 row-major */
} gfbe_imu_preint; /* 467 doubles */

/* What WheelFactor reads from WheelIntegrationBase (wheel_factor.h:80-243,
 * wheel_integration_base.h:180-219). */
typedef struct gfbe_wheel_preint {
  double sum_dt;
  double delta_p[3];
  double delta_q[4]; /* x y z w */
  double linearized_sx, linearized_sy, linearized_sw, linearized_td;
  double linearized_vel[3], linearized_gyr[3]; /* first sample of the interval */
  double vel_1[3], gyr_1[3];                   /* last sample of the interval */
  double jacobian[18];   /* 6x3 row-major: d(p,theta)/d(sx,sy,sw) */
  double covariance[36]; /* 6x6 row-major */
} gfbe_wheel_preint; /* 78 doubles */

/* Marginalisation prior = MarginalizationInfo's result fields
 * (marginalization_factor.h:67-81): linearized_jacobians, linearized_residuals,
 * keep_block_{size,idx,data}; block identity is symbolic (block_id) instead of an address. */
typedef struct gfbe_prior {
  int32_t valid;    /* MarginalizationInfo::valid */
  int32_t n;        /* tangent dimension (rows == cols of J0) */
  int32_t n_blocks;
  int32_t block_id[GFBE_MAX_PRIOR_BLOCKS];   /* GFBE_BLK_* the block is attached to NOW (after addr_shift) */
  int32_t block_size[GFBE_MAX_PRIOR_BLOCKS]; /* global size: 7, 9 or 1 */
  int32_t block_idx[GFBE_MAX_PRIOR_BLOCKS];  /* tangent offset in [0,n)  (keep_block_idx - m) */
  double x0[GFBE_NFRAMES * 16 + 32];         /* keep_block_data, concatenated in block order */
  double *J0;       /* n*n row-major, caller-owned, capacity >= GFBE_DENSE_DIM^2 */
  double *r0;       /* n,             caller-owned, capacity >= GFBE_DENSE_DIM   */
} gfbe_prior;

/* Visual factor list: one entry per ProjectionTwoFrameOneCamFactor that optimization() would
 * `new` (estimator.cpp:3330-3358). Produced bit-exactly by gfbe_build_visual_factors(). */
typedef struct gfbe_visual {
  int32_t n_factor;             /* K */
  const int32_t *feature_index; /* [K] index into para_Feature */
  const int32_t *imu_i;         /* [K] start_frame of the landmark */
  const int32_t *imu_j;         /* [K] observing frame, != imu_i */
  const double *pts_i;          /* [K][3] first observation (normalised coords) */
  const double *pts_j;          /* [K][3] */
  const double *vel_i;          /* [K][2] */
  const double *vel_j;          /* [K][2] */
  const double *td_i;           /* [K] cur_td of the first observation */
  const double *td_j;           /* [K] */
} gfbe_visual;

/* f4 (BASELINE configs[4]): LiDAR point-to-plane factors attached to ONE window pose — the
 * joint LIO + VIO solve, a capability the reference does not have (its LIO solves them alone, lidarodom.cpp:538-581).
 * Factor k: residual = sqrt_info * weight[k] * (normal[k] . (R p[k] + t) + offset[k]) on pose `frame` = [t | q]
 * (LidarPlaneNormFactor::Evaluate, lio/src/liw/lidarFactor.cpp:18-51; points already in the IMU frame), robustified by
 * ceres::HuberLoss(huber_delta) as the LIO does (lidarodom.cpp:539: 0.5); huber_delta <= 0: no loss. n == 0: no block. */
typedef struct gfbe_lio_block {
  int32_t n;
  int32_t frame;                /* window pose the scan belongs to (the newest: frame_count) */
  const double *pts;            /* [n][3] */
  const double *normals;        /* [n][3] */
  const double *offsets;        /* [n] */
  const double *weights;        /* [n] or NULL (= 1) */
  double sqrt_info;
  double huber_delta;
} gfbe_lio_block;

/* One call of optimization(): everything it reads. */
typedef struct gfbe_window {
  int32_t frame_count;          /* poses 0..frame_count are in the problem (== WINDOW_SIZE when full) */
  gfbe_state state;             /* in: vector2double() output */
  int32_t n_feature;            /* L = FeatureManager::getFeatureCount() */
  const double *para_Feature;   /* [L] inverse depths (getDepthVector, feature_manager.cpp:286-302) */
  const uint8_t *feature_const; /* [L] 1 => SetParameterBlockConstant (estimate_flag==1, estimator.cpp:3352) */
  /* SetParameterBlockConstant decisions (estimator.cpp:3022,3059,3101,3114-3116,3159-3161,3302-3303) */
  uint8_t pose_const[GFBE_NFRAMES];
  uint8_t sb_const[GFBE_NFRAMES];
  uint8_t ex_cam_const, ex_wheel_const, ix_wheel_const, td_const, td_wheel_const;
  /* PoseSubsetParameterization constancy masks (pose_subset_parameterization.cpp:11-45): tangent
   * components zeroed in Plus only (the Jacobian stays unmasked — reference quirk, reproduced). */
  uint8_t ex_cam_mask[6], ex_wheel_mask[6];
  /* Optional in-window factors (estimator.cpp:3120-3136, 3214-3228, 3004-3012; all shipped yamls: plane 0, gnss_enable 0):
   *   use_plane   one PlaneFactor (plane_factor.h:25-122) per window pose i < frame_count on {Pose[i], Ex_Pose_wheel, plane_R,
   *               plane_Z}; the MARGIN_OLD set takes the one of frame 0 (estimator.cpp:3441-3448). plane_const = the
   *               SetParameterBlockConstant decision of :3126-3135.
   *   use_anchor  one PoseAnchorFactor (pose_anchor_factor.cpp:8-32) on Pose[0] (the `first_optimization && GNSS_ENABLE`
   *               block, :3004-3012). */
  uint8_t use_plane, plane_const, use_anchor;
  int32_t n_imu;                /* IMU factors; factor k links frames imu_frame[k], imu_frame[k]+1 */
  const int32_t *imu_frame;
  const gfbe_imu_preint *imu;
  int32_t n_wheel;
  const int32_t *wheel_frame;
  const gfbe_wheel_preint *wheel;
  gfbe_visual vis;
  const gfbe_prior *prior;      /* NULL or !valid => no MarginalizationFactor */
  gfbe_lio_block lio;           /* optional LiDAR factors on one pose (n = 0: none) */
  double plane_noise_inv[3];    /* PITCH_N_INV, ROLL_N_INV, ZPW_N_INV (parameters.cpp:340-345) */
  double anchor_pose[7];        /* PoseAnchorFactor's anchor_value (para_Pose[0] at the first optimisation) */
  double anchor_sqrt_info;      /* 120 in the reference (pose_anchor_factor.h:19) */
  /* GNSS inside the window (estimator.cpp:2965-3002, 3239-3291, 3462-3496; gnss_enable: 0 in every shipped yaml).
   *   gnss_ready  the blocks para_yaw_enu_local (held constant, :2991), para_anc_ecef, para_rcv_dt[11][4], para_rcv_ddt[11] join the
   *               problem. Unless the window moves too slowly — mean |Vs[i].xy| over the window below 0.3 m/s at the start of the
   *               call, `lowspeed`, :2969-2984, computed by the library from `state` — one GnssPsrDoppFactor per observation, one
   *               DtDdtFactor per constellation and frame interval and one DdtSmoothFactor per interval are added (:3239-3291).
   *               MARGIN_OLD takes the factors of frame 0 with the drop sets of :3462-3496 whether the window is slow or not.
   *   gnss_obs    the n_gnss observations of gnss_meas_buf[0 .. WINDOW_SIZE] in the reference's insertion order (frame-major);
   *               `frame`, `lower_idx`, `ratio`, `sys_idx` as :3250-3263 computes them (frame 0 always has lower_idx 0).
   *   gnss_iono   latest_gnss_iono_params (8 Klobuchar parameters) or NULL; gnss_frame_dt[i] = Headers[i + 1] - Headers[i];
   *               gnss_ddt_weight = GNSS_DDT_WEIGHT. The GNSS state travels in `state.gnss` and comes back in out_state->gnss. */
  int32_t gnss_ready;
  int32_t n_gnss;
  const gfbe_gnss_obs *gnss_obs;
  const double *gnss_iono;
  double gnss_frame_dt[GFBE_WINDOW_SIZE];
  double gnss_ddt_weight;
} gfbe_window;

typedef struct gfbe_options {
  /* sizeof(gfbe_options) of the header the CALLER was compiled against, written by gfbe_default_options (always start from it).
   * gfbe_create refuses a struct whose size is not the library's own (GFBE_BAD_INPUT, "options ABI mismatch"): the struct has grown
   * by trailing fields from round to round, and a caller built against an older header would otherwise hand over a shorter struct
   * whose missing fields the library reads from whatever follows it. gfbe_options_size() returns the library's. */
  int32_t struct_size;
  int32_t max_num_iterations;   /* NUM_ITERATIONS = 8 (m3dgr.yaml:109) */
  double huber_delta;           /* HuberLoss(1.0)  (estimator.cpp:2959) */
  double vis_sqrt_info;         /* FOCAL_LENGTH/1.5 = 400 (estimator.cpp:193) */
  double g_norm;                /* G = (0,0,g_norm) (parameters.cpp:223; m3dgr.yaml:117) */
  /* Ceres 1.14 Solver::Options defaults the reference leaves untouched (estimator.cpp:3364-3376) */
  double initial_trust_region_radius; /* 1e4 */
  double function_tolerance;          /* 1e-6 */
  double gradient_tolerance;          /* 1e-10 */
  double parameter_tolerance;         /* 1e-8 */
  double min_relative_decrease;       /* 1e-3 */
  int32_t jacobi_scaling;             /* 1 */
  double marg_eps;                    /* eps = 1e-8, marginalization_factor.h:70 */
  /* Square root of the marginalised information A' (marginalization_factor.cpp:294-302):
   *   0  eigen-decomposition, S > eps thresholding — the reference's construction
   *   1  diagonally pivoted LDL^T with pivots > eps — same J0^T J0 / J0^T r0 up to O(n*eps) absolute
   *      (1e-14 relative to |A'|); the cheaper one on the device: 0.09 ms of a 1.15 ms call, where mode 0 — Householder
   *      tridiagonalisation + divide & conquer since round 6 — takes 0.64 ms of a 1.72 ms call. Default.
   *   The two square roots carry the same information J0^T J0, J0^T r0; they do NOT share the prior's constant term |r0|^2 (the
   *   smallest kept eigenvalues of A' amplify b'): a caller that logs costs sees a constant offset between the modes (and between
   *   mode 0 and the reference's own Eigen build), never a different step.
   *   Batch independence of the new prior: a window's J0, r0 do not depend IN BITS on the batch it is solved in as long as the batch
   *   stays inside one kernel set — fewer than 32 windows (k_marg on 1024 threads, k_marg_ldlt<4>) or 32 and more (512 threads,
   *   k_marg_ldlt_tp). Across the two sets the same window gets a prior that differs in its last bits, in both modes: measured
   *   against an extended-precision model (tests/test_gpu_prior.py, priors of 71 .. 177 dims), J0^T J0 of the two sets agrees to
   *   1.7e-5 u |A| for the LDL^T kernels and 1.4e-3 u |A| for the eigen path (MARGIN_SECOND_NEW: 0.14 / 12 u |A|; u = 2^-53, |A| the
   *   largest entry of the un-reduced information; each set is within 7 u |A| of the model), and the number of non-zero rows is
   *   the same whenever no eigenvalue / pivot of A' lies near marg_eps. A pivot within rounding (~64 u |A|) of marg_eps can be kept
   *   by one set and dropped by the other. */
  int32_t marg_sqrt;
  /* 1: gfbe_batch_solve replays its fixed kernel sequence as a hipGraph from the third call on a batch (first
   * call eager, second captured); 0 (default): eager launches — on ROCm 7.2 / MI355X the replay measured 2.50 vs
   * 2.54 ms for one window and 3 % slower at 256 windows. Ignored while profiling / landmark sharding. */
  int32_t use_graph;
  /* Parts a batch of >= 128 windows is split into by gfbe_batch_upload; gfbe_batch_solve runs the parts side by side,
   * each on its own pair of streams (kernels of different stages share the GPU). 1 (default): four parts for batches of
   * >= 2048 windows, one below (measured round 3: 1024 windows 62.7k solves/s whole, 61.2k as four parts, 56.7k as two;
   * 4096 windows 67.2k as four parts, 65.0k whole); n >= 2: exactly n parts. Results per window are unchanged (every window is independent). 0: one launch sequence for the
   * whole batch. */
  int32_t split_batch;
  /* Solver::Options::max_solver_time_in_seconds (estimator.cpp:3369-3376: SOLVER_TIME = 0.04 s, x 4/5 before a MARGIN_OLD).
   * Checked ON THE DEVICE at the start of every trust-region iteration against the device's wall clock (no host
   * synchronisation inside a solve); a window over budget stops with termination 0 / GFBE_NO_CONVERGENCE like Ceres'
   * "maximum solver time reached". 0 (default) = no cap: results then depend on the inputs only. A binding that wants the
   * reference's behaviour sets 0.04 (or 0.032); at 2 ms per solve it never triggers. */
  double max_solver_time_in_seconds;
  /* Host threads gfbe_batch_upload / gfbe_batch_download pack and unpack windows with (one window per task).
   * 0 (default) = the library's choice per job: the packing passes of an upload min(hardware threads, 24) — 48 on a host with 128 or more
   * hardware threads —, the unpacking of a download min(hardware threads, 16); 1 = the calling thread only. */
  int32_t host_threads;
  /* Factorisation of the reduced system (the DENSE_SCHUR linear solve of estimator.cpp:3364-3379 after the landmark elimination):
   *   0 (default)  the speed-bias blocks are eliminated as a chain of 9 x 9 blocks before the dense pose / extrinsic part is
   *                factorised (~70 KB of LDS, two workgroups per CU). Needs the structure every factor of the reference has:
   *                a prior that keeps a speed-bias block other than SpeedBias[0] switches its batch to 1 by itself.
   *                Batches below 32 windows — the reference's call pattern is ONE — eliminate the chain from both ends at once
   *                (eight waves, one workgroup per CU: 6 sequential block steps instead of 11), larger ones from one end (four waves, two
   *                workgroups per CU: throughput). Same step to rounding.
   *   1            one blocked factorisation of the whole reduced system (160 KB of LDS). Same step to rounding.
   *   2 / 3        (tests, measurements) the one-ended / the two-ended chain kernel whatever the batch size.
   * A batch with GNSS blocks (gfbe_window.gnss_enable; 246 tangent dims instead of 187) takes the one-ended chain kernel with the
   * 58 GNSS dims as dense columns when every window's dense part fits nine 16-wide tile columns (<= 142 dims), and the blocked
   * out-of-LDS factorisation of rounds 3-5 otherwise;
   *   4            (tests, measurements) that blocked factorisation for every batch with GNSS blocks. Same step to rounding. */
  int32_t solve_kernel;
  /* TEST HOOK (0 = off, the default; never set it in production): the first factorisation of trust-region iteration
   * `test_fail_chol_iter` is declared failed, so that DoglegStrategy's mu retry — which well-posed windows never take —
   * can be exercised (tests/test_gpu_branches.py). */
  int32_t test_fail_chol_iter;
  /* TEST HOOK: how many consecutive factorisation attempts of that iteration fail (default 1; 0 is taken as 1). */
  int32_t test_fail_chol_count;
  /* Landmark sharding (gfbe_set_allreduce) only: how many times a window whose reduced system failed to factorise is retried with
   * mu x 10 (DoglegStrategy::ComputeGaussNewtonStep retries up to max_mu = 1, i.e. 8 times from min_mu = 1e-8; the unsharded kernels
   * do so inside the solve kernel). Every retry is one more [E rebuild | all-reduce | factorisation] triple in the FIXED launch
   * sequence of every linearisation, taken or not: default 1 (well-posed windows never take even that one); 8 reproduces Ceres;
   * 0: no retry — a failed factorisation ends the solve as a failed linear solve, and every linearisation carries one all-reduce
   * less (three per trust-region iteration instead of four: the packed system and the two scalar exchanges). */
  int32_t sharded_mu_retries;
  /* Batches without an all-reduce hook: 1 (default) — the pass that evaluates the candidate of a trust-region
   * iteration LINEARISES there (every iteration but the last of a solve), into a second set of the linearisation's outputs; an accepted
   * step makes it the current set, a rejected one leaves the old linearisation in place (DoglegStrategy's reuse), and the next
   * iteration starts at the landmark elimination. The evaluations are TrustRegionMinimizer's own, in its order — the candidate's
   * cost, then residuals + Jacobians at the accepted point: the same state —, so nothing a solve returns changes by a bit
   * (tests/test_gpu_speculative.py); what goes is one evaluation pass per iteration: the cost-only pass of the visual and the dense
   * factors (8192 resident windows: +10 % solves/s; a single window: one launch less per iteration, -3.5 %). Costs the second set:
   * ~1.5 MB per 2k-landmark window. 0 — cost pass and linearisation separately, as in rounds 1-4. */
  int32_t speculative_linearization;
  /* Throughput batches (>= 32 windows) whose windows all hold the camera extrinsic and td constant, without an all-reduce hook:
   * 1 — the visual factors are evaluated AND the landmarks eliminated by one kernel (k_linschur: one workgroup per window and group of
   * start frames; a landmark tile's rows go from the evaluating lanes' registers into the LDS panel the matrix cores multiply, and are
   * not re-read from HBM by a second kernel); 0 (default) — k_vis<0> + k_schur. Same quantities, the per-landmark sums added in
   * another order (last bits). Built in round 6 because the two kernels exchange ~1.4 GB per 2048 windows; MEASURED SLOWER on MI355X
   * (per 512 windows: 281 us at the first iteration against 133 + 143, 325 us at a candidate against 137 + 142; 8192 resident windows:
   * 97k against 114k solves/s, profiles/r6_linschur_ab.txt): neither kernel was bound by that traffic, and one workgroup that
   * alternates between the two phases behind three barriers per tile overlaps worse than two kernels that each fill the device.
   * Kept as an option with its tests (tests/test_gpu_linschur.py); DESIGN.md section 4. */
  int32_t merge_lin_schur;
} gfbe_options;

typedef struct gfbe_summary {
  int32_t status;            /* gfbe_status */
  int32_t iterations;        /* trust-region iterations run (excluding iteration 0) */
  int32_t num_successful;    /* accepted steps */
  int32_t termination;       /* 0 max-iter, 1 function tol, 2 parameter tol, 3 gradient tol, 4 failure */
  double initial_cost;
  double final_cost;
  double final_radius;
  double cost_history[16];   /* cost after each iteration (accepted or not), [0] = initial */
  uint8_t accepted[16];      /* accept/reject per iteration */
  /* Phase times from the device's wall clock (100 MHz), per window: first kernel of the solve -> re-anchored state, and
   * re-anchored state -> prior written (0 when no marginalisation ran). In a batch all windows advance together, so these
   * are the batch's phase times as seen by this window. */
  double ms_solve, ms_marginalize;
  /* Host <-> device bytes of this window: packed upload (landmarks, factors, pre-integrations, prior) and result download. */
  double bytes_uploaded, bytes_downloaded;
} gfbe_summary;

enum { GFBE_MARGIN_OLD = 0, GFBE_MARGIN_SECOND_NEW = 1, GFBE_MARGIN_NONE = 2 };

/* ------------------------------------------------------------------------------------------
 * Context
 * ------------------------------------------------------------------------------------------ */
typedef struct gfbe_ctx gfbe_ctx;

void gfbe_default_options(gfbe_options *opt);
/* sizeof(gfbe_options) as the LIBRARY was built (gfbe_options.struct_size must equal it). */
int32_t gfbe_options_size(void);

/* device < 0: host-only context (bookkeeping functions only; every compute entry point returns
 * GFBE_NO_DEVICE). device >= 0: HIP device ordinal; fails with GFBE_NO_DEVICE if absent.
 * The solver drives up to eight HIP streams (two solver lanes with a side stream each, upload, download, the caller's); they
 * share the hardware queues the HIP runtime gives the process. The library does not touch the environment.
 * gfbe_create_note holds remarks that are not errors (never in gfbe_last_error, which only ever holds the cause of a failing
 * call): gfbe_batch_upload leaves one there when it had to switch speculative_linearization off for a batch whose second set of
 * outputs did not fit the device. */
gfbe_status gfbe_create(gfbe_ctx **ctx, int device, const gfbe_options *opt);
/* Frees the context and the device memory it caches. Batches (gfbe_batch_free) and feature tables (gfbe_ftab_destroy) made with
 * the context must be released BEFORE it. The HIP streams the context created are kept in a process-wide pool for the next
 * gfbe_create on the same device (a later context then runs on the hardware queues the first one had); they live until the process ends. */
void gfbe_destroy(gfbe_ctx *ctx);
const char *gfbe_last_error(const gfbe_ctx *ctx);
/* Informational remarks of gfbe_create ("" when there are none); the reference has no counterpart (ROS_WARN at start-up). */
const char *gfbe_create_note(const gfbe_ctx *ctx);
const char *gfbe_version(void);
/* Launch kernels on this hipStream_t (e.g. torch's current stream). NULL = the ctx's own stream. */
gfbe_status gfbe_set_stream(gfbe_ctx *ctx, void *hip_stream);

/* ------------------------------------------------------------------------------------------
 * a13  Landmark bookkeeping (host, integer, bit-exact):
 *   FeatureManager::getFeatureCount   feature_manager.cpp:43-55
 *   FeatureManager::getDepthVector    feature_manager.cpp:286-302
 *   visual-factor loop                estimator.cpp:3326-3358 (solve) and 3498-3531 (marginalise)
 * Input is the std::list<FeaturePerId> flattened in list order: feature f has n_obs[f]
 * observations starting at frame start_frame[f]; obs rows are [x y z u v vx vy] (7 doubles) plus
 * cur_td, stored contiguously at obs_offset[f].
 * ------------------------------------------------------------------------------------------ */
typedef struct gfbe_feature_list {
  int32_t n;                    /* features in the list (all, including used_num < 4) */
  const int32_t *start_frame;   /* [n] */
  const int32_t *n_obs;         /* [n] feature_per_frame.size() */
  const int32_t *obs_offset;    /* [n] first row of this feature in obs / obs_td */
  const double *obs;            /* [sum n_obs][7]  x y z u v vx vy */
  const double *obs_td;         /* [sum n_obs]     cur_td */
  const double *estimated_depth;/* [n] */
  const int32_t *estimate_flag; /* [n] 1 => depth came from the RGB-D image */
} gfbe_feature_list;

/* Returns the number of landmarks L (getFeatureCount). */
int32_t gfbe_feature_count(const gfbe_feature_list *fl);
/* Counts factors: total (solve) or only landmarks with start_frame == 0 (marginalise). */
int32_t gfbe_visual_factor_count(const gfbe_feature_list *fl, int32_t only_start_frame0);
/* Fills caller-allocated arrays (capacity from the two functions above); returns K written.
 * para_Feature/feature_const have capacity L. */
int32_t gfbe_build_visual_factors(const gfbe_feature_list *fl, int32_t only_start_frame0,
                                  int32_t *feature_index, int32_t *imu_i, int32_t *imu_j,
                                  double *pts_i, double *pts_j, double *vel_i, double *vel_j,
                                  double *td_i, double *td_j,
                                  double *para_Feature, uint8_t *feature_const);
/* FeatureManager::setDepth (feature_manager.cpp:249-267): solve_flag[f] = 0 untouched,
 * 1 ok, 2 failed (negative depth); estimated_depth updated for landmarks with used_num >= 4. */
void gfbe_set_depth(const gfbe_feature_list *fl, const double *para_Feature,
                    double *estimated_depth, int32_t *solve_flag);

/* ------------------------------------------------------------------------------------------
 * f1  FeatureManager / slideWindow operations on device-resident feature tables
 *     (SURVEY.md section 8f rank 1 — the step either side of the solve):
 *       FeatureManager::addFeatureCheckParallax   feature_manager.cpp:57-116 (+ compensatedParallax2 :978-1011)
 *       setDepth / removeFailures / clearDepth / getDepthVector   :249-302
 *       triangulate :669-724, triangulateWithDepth :726-799
 *       removeOutlier :801-816, removeBackShiftDepth :818-856, removeBack :858-874, removeFront :914-934
 *       Estimator::slideWindow / slideWindowNew / slideWindowOld   estimator.cpp:3700-3899
 *       Estimator::outliersRejection :3971-4028, movingConsistencyCheckW :4030-4074
 * A gfbe_ftab holds W independent tables in HBM (one per window; every call applies the same operation to
 * all W tables, per-table arguments are arrays of length W). A table is FeatureManager's
 * std::list<FeaturePerId> in insertion order — the order that defines para_Feature[k]
 * (getFeatureCount / getDepthVector) — with at most WINDOW_SIZE+1 observations per feature, each
 * [x y z u v vx vy depth] + cur_td (FeaturePerFrame, feature_manager.h:30-64). Erasures keep the order.
 * Integer contents are bit-exact against the CPU oracle; depths to the tolerance stated in the tests.
 * Pose arguments: [P(3) | R(9, row-major)] per frame; extrinsic: [tic(3) | ric(9, row-major)].
 * ------------------------------------------------------------------------------------------ */
typedef struct gfbe_ftab gfbe_ftab;
typedef struct gfbe_ftab_options {
  double init_depth;       /* INIT_DEPTH = 5.0 (parameters.cpp:484) */
  double min_parallax;     /* MIN_PARALLAX = keyframe_parallax / FOCAL_LENGTH = 10 / 600 (parameters.cpp:351-352, m3dgr.yaml:110) */
  double focal_length;     /* FOCAL_LENGTH = 600 (parameters.h:23) in the parallax / outlier thresholds */
  double depth_threshold;  /* triangulateWithDepth: RGB-D depths in [0.1, depth_threshold] are trusted (parameters.cpp:178; yaml) */
} gfbe_ftab_options;
void gfbe_ftab_default_options(gfbe_ftab_options *opt);
/* feature_capacity <= 16384 features per table.
 * Every table operation runs in order on the context's stream. The ones without outputs (triangulate, set_depth, clear_depth,
 * remove_*) copy their arguments and return without waiting for the device; the ones that hand something back (add_frame,
 * check_outliers, get_depth_vector, size, download, gfbe_batch_upload_tables) wait for what was enqueued before them. Capacity /
 * observation-count overflow is raised by gfbe_ftab_add_frame (GFBE_BAD_INPUT, sticky).
 * A device error of a deferred operation (its kernel has not run when the call returns) is reported by the NEXT table call that
 * synchronises — usually add_frame or check_outliers — and gfbe_last_error then names that call, not the operation that faulted.
 * gfbe_ftab_create leaves *out null and frees what it had allocated when any of its allocations fails. */
gfbe_status gfbe_ftab_create(gfbe_ctx *ctx, int32_t n_tables, int32_t feature_capacity,
                             const gfbe_ftab_options *opt, gfbe_ftab **out);
void gfbe_ftab_destroy(gfbe_ctx *ctx, gfbe_ftab *t);
/* addFeatureCheckParallax. Table w receives the features [offset[w], offset[w+1]) — ascending feature_id, the
 * iteration order of the reference's std::map — with observation rows obs8 [x y z u v vx vy depth].
 * Outputs per table: keyframe (1 = the function returns true = MARGIN_OLD), counters
 * [last_track_num, new_feature_num, long_track_num], avg_parallax (last_average_parallax). */
gfbe_status gfbe_ftab_add_frame(gfbe_ctx *ctx, gfbe_ftab *t, const int32_t *frame_count, const int32_t *offset,
                                const int32_t *feature_id, const double *obs8, const double *td,
                                int32_t *keyframe, int32_t *counters, double *avg_parallax);
/* removeBackShiftDepth(marg_R, marg_P, new_R, new_P); *_PR = [W][12]. */
gfbe_status gfbe_ftab_remove_back_shift_depth(gfbe_ctx *ctx, gfbe_ftab *t, const double *marg_PR, const double *new_PR);
gfbe_status gfbe_ftab_remove_back(gfbe_ctx *ctx, gfbe_ftab *t);
gfbe_status gfbe_ftab_remove_front(gfbe_ctx *ctx, gfbe_ftab *t, const int32_t *frame_count);
/* removeOutlier: ids of table w are [offset[w], offset[w+1]). */
gfbe_status gfbe_ftab_remove_outlier(gfbe_ctx *ctx, gfbe_ftab *t, const int32_t *offset, const int32_t *ids);
gfbe_status gfbe_ftab_remove_failures(gfbe_ctx *ctx, gfbe_ftab *t);
gfbe_status gfbe_ftab_clear_depth(gfbe_ctx *ctx, gfbe_ftab *t);
/* setDepth(x) / getDepthVector(): para_Feature of table w starts at offset[w] (capacity offset[w+1]-offset[w]);
 * count[w] = getFeatureCount(). */
gfbe_status gfbe_ftab_set_depth(gfbe_ctx *ctx, gfbe_ftab *t, const int32_t *offset, const double *para_Feature);
gfbe_status gfbe_ftab_get_depth_vector(gfbe_ctx *ctx, gfbe_ftab *t, const int32_t *offset, double *para_Feature,
                                       int32_t *count);
/* triangulate (with_depth = 0) / triangulateWithDepth (1). poses [W][11][12], tic_ric [W][12]. */
gfbe_status gfbe_ftab_triangulate(gfbe_ctx *ctx, gfbe_ftab *t, const double *poses, const double *tic_ric,
                                  int32_t with_depth);
/* mode 0: outliersRejection, 1: movingConsistencyCheckW. ids_out of table w start at offset[w] (ascending, the
 * iteration order of the reference's std::set); count_out[w] ids are written. */
gfbe_status gfbe_ftab_check_outliers(gfbe_ctx *ctx, gfbe_ftab *t, const double *poses, const double *tic_ric,
                                     int32_t mode, const int32_t *offset, int32_t *ids_out, int32_t *count_out);
gfbe_status gfbe_ftab_size(gfbe_ctx *ctx, gfbe_ftab *t, int32_t *n_features);
/* Snapshot of table w in list order; obs8 [n][11][8], obs_td [n][11] (rows >= n_obs are zero). Any pointer may be NULL. */
gfbe_status gfbe_ftab_download(gfbe_ctx *ctx, gfbe_ftab *t, int32_t w, int32_t *feature_id, int32_t *start_frame,
                               int32_t *n_obs, double *obs8, double *obs_td, double *estimated_depth,
                               int32_t *estimate_flag, int32_t *solve_flag);
struct gfbe_batch;
/* gfbe_batch_upload with the visual part of window w read from table w of `t` ON THE DEVICE (landmarks = features with
 * >= 4 observations in list order, para_Feature[k] = 1 / estimated_depth, constant when estimate_flag == 1:
 * estimator.cpp:3330-3358): wins[w]->vis, n_feature, para_Feature and feature_const are ignored; state, pre-integrations,
 * prior and the constant flags come from wins[w]. gfbe_batch_download returns the features in list order, ready for
 * gfbe_ftab_set_depth. n_windows <= the number of tables. */
gfbe_status gfbe_batch_upload_tables(gfbe_ctx *ctx, gfbe_ftab *t, int32_t n_windows, const gfbe_window *const *win,
                                     struct gfbe_batch **out);
/* Landmarks of window w of a batch (= the length of out_feature[w] in gfbe_batch_download; getFeatureCount(),
 * feature_manager.cpp:56-68); -1 for a bad index. */
int32_t gfbe_batch_feature_count(const struct gfbe_batch *batch, int32_t w);
/* slideWindow()'s shift of the state blocks (estimator.cpp:3700-3858): MARGIN_OLD moves frames 1..WINDOW_SIZE to
 * 0..WINDOW_SIZE-1 and leaves the newest duplicated at WINDOW_SIZE; MARGIN_SECOND_NEW copies frame WINDOW_SIZE
 * onto WINDOW_SIZE-1. Host function (the caller owns the state). */
void gfbe_slide_window_state(gfbe_state *state, int32_t margin_flag);

/* ------------------------------------------------------------------------------------------
 * f3  global_fusion pose graph (BASELINE configs[3]):
 *       GlobalOptimization::optimize     global_fusion/src/globalOpt.cpp:107-236
 *       RelativeRTError / TError         global_fusion/src/Factors.h:26-114 (ceres::AutoDiffCostFunction in the
 *                                        reference; analytic tangent Jacobians here)
 * A chain of n poses [t(3) | q(w,x,y,z)] (the quaternion order of globalOpt.cpp:46-47, NOT the x,y,z,w of the VIO
 * blocks), one RelativeRTError between consecutive poses (rel_i[k], rel_i[k] + 1) with measurement [t(3) | q(wxyz)]
 * and the reference's constant weights 1 / t_var, 1 / q_var (0.1, 0.01: globalOpt.cpp:171-173), and Huber-robustified
 * (delta 1.0) position fixes TError [x y z var] on a subset of the poses (GPS / AprilTag, :177-185). Solver = what
 * ceres::Solve does with the reference's options (:117-121): Levenberg-Marquardt trust region, Jacobi scaling,
 * max_num_iterations 5, quaternions on ceres::QuaternionParameterization (x <- [cos|d|, sin|d|/|d| d] * x) — the normal
 * equations are block-tridiagonal (6 x 6 blocks), factorised by a block Cholesky recurrence instead of
 * SPARSE_NORMAL_CHOLESKY's general sparse factorisation.
 * gfbe_pg_eval: residuals and tangent Jacobians at `pose` (columns: dq_i(3) t_i(3) dq_j(3) t_j(3)); cost includes the
 * Huber loss of the fixes. Any output pointer may be NULL.
 * ------------------------------------------------------------------------------------------ */
gfbe_status gfbe_pg_eval(gfbe_ctx *ctx, int32_t n_poses, const double *pose, int32_t n_rel, const int32_t *rel_i,
                         const double *rel_meas, double t_var, double q_var, int32_t n_fix, const int32_t *fix_i,
                         const double *fix_meas, double huber_delta, double *rel_r, double *rel_J, double *fix_r,
                         double *cost);
gfbe_status gfbe_pg_solve(gfbe_ctx *ctx, int32_t n_poses, const double *pose_in, int32_t n_rel, const int32_t *rel_i,
                          const double *rel_meas, double t_var, double q_var, int32_t n_fix, const int32_t *fix_i,
                          const double *fix_meas, double huber_delta, int32_t max_num_iterations, double *pose_out,
                          gfbe_summary *summary);

/* ------------------------------------------------------------------------------------------
 * f3b loop-closure pose graph of dense_map, the 4-DoF solve that runs on VIO input:
 *       PoseGraph::optimize4DoF             dense_map/src/pose_graph.cpp:529-705 (options :558-566)
 *       FourDOFError / FourDOFWeightError   dense_map/src/pose_graph.h:199-288 (automatic differentiation in the
 *                                           reference; analytic tangent Jacobians here)
 * A keyframe is t(3) and ypr(3) in DEGREES (Utility::R2ypr's order); the solve moves yaw and t, pitch and roll are frozen
 * into the factors. Tangent of a pose: [yaw, t_x, t_y, t_z]; yaw moves by NormalizeAngle(yaw + delta), a single wrap.
 * gfbe_lc4_eval: an explicit edge list (edge_i, edge_j), kind 0 = FourDOFError, 1 = FourDOFWeightError under HuberLoss,
 * meas [n_edges][6] = t_x t_y t_z relative_yaw pitch_i roll_i. Returns r [n_edges][4], J [n_edges][4][8] (columns yaw_i
 * t_i(3) yaw_j t_j(3); kind 1 through the corrector) and the cost with the loss. Any output pointer may be NULL.
 * gfbe_lc4_solve: the graph optimize4DoF builds. t / ypr [n][3] are the VIO poses: the starting point AND the source of
 * the sequence measurements — for every i and k = 1 .. span with sequence[i] == sequence[i - k] an edge (i - k, i) with
 * relative_t = R(ypr_{i-k})^T (t_i - t_{i-k}), relative_yaw = yaw_i - yaw_{i-k} (not normalised), formed by the library.
 * fixed[i] != 0: the pose is constant (the caller sets it for the earliest looped keyframe and for sequence 0). Loop edges
 * (loop_c[l], loop_i[l]) with loop_c < loop_i, at most one per loop_i, loop_meas [n_loop][4] = relative t, relative yaw
 * (pitch and roll of the connected pose come from ypr). At most GFBE_LC4_MAX_LOOPS loop edges. Solver = what ceres::Solve
 * does with the reference's options: Levenberg-Marquardt, Jacobi scaling, Ceres 1.14 defaults; the normal equations are
 * block-tridiagonal in 16 x 16 super-blocks of four poses plus a rank-4 term per loop edge, solved exactly (parallel block
 * cyclic reduction with the loop columns as right-hand sides, then the 4 n_loop capacitance system).
 * Outputs: t_out [n][3], yaw_out [n], drift[4] = yaw_drift, t_drift of the last keyframe (:674-681; may be NULL), summary
 * as gfbe_pg_solve fills it. GFBE_BAD_INPUT with nothing written for n_loop > GFBE_LC4_MAX_LOOPS, an index out of range,
 * loop_c >= loop_i, two loops on one loop_i or an options struct of another size; GFBE_NO_DEVICE without a GPU.
 * gfbe_lc4_solve_long: the same call for a long revisit, up to GFBE_LC4_LONG_MAX_LOOPS loop edges: the same arguments, graph,
 * solver statements, outputs and failure contract (GFBE_BAD_INPUT with nothing written beyond GFBE_LC4_LONG_MAX_LOOPS). Up to
 * GFBE_LC4_MAX_LOOPS loop edges it runs the code of gfbe_lc4_solve and returns its bits; beyond, the 4 n_loop capacitance system
 * (up to 2048 x 2048, 128 tile columns) is factorised across the device, one pair of launches per 16-column pivot step.
 * Device scratch of a call (grow-only, owned by the context), in doubles, with rows = 16 ceil(n / 4), ld = 16 ceil((1 + 4 n_loop) / 16)
 * and cap_ld = 16 ceil(4 n_loop / 16):
 *     2 rows ld  (the two panels)  +  2 cap_ld^2  (S and L)  +  about 330 rows + 140 n_loop + 18 cap_ld  (band sets, vectors)
 * At n = 5000, n_loop = 512: 2 x 20 000 x 2064 + 2 x 2048^2 doubles = 0.73 GB for panels, S and L, 0.78 GB with the rest; a failed
 * allocation is GFBE_DEVICE_ERROR.
 * ------------------------------------------------------------------------------------------ */
#define GFBE_LC4_MAX_LOOPS 64
#define GFBE_LC4_LONG_MAX_LOOPS 512
typedef struct gfbe_lc4_options {
  int32_t struct_size;          /* sizeof(gfbe_lc4_options), written by gfbe_lc4_default_options */
  int32_t max_num_iterations;   /* 5 (pose_graph.cpp:563); at most 15 are run */
  int32_t span;                 /* 4 (:606): sequence edges reach this many keyframes back, 1 .. 4 */
  int32_t reserved;
  double huber_delta;           /* 0.1 (:566), loop edges only */
  double loop_yaw_div;          /* 10.0 (pose_graph.h:271) */
} gfbe_lc4_options;
void gfbe_lc4_default_options(gfbe_lc4_options *opt);
gfbe_status gfbe_lc4_eval(gfbe_ctx *ctx, const gfbe_lc4_options *opt /* NULL: defaults */, int32_t n_poses, const double *t,
                          const double *ypr, int32_t n_edges, const int32_t *edge_i, const int32_t *edge_j,
                          const uint8_t *kind, const double *meas, double *r, double *J, double *cost);
gfbe_status gfbe_lc4_solve(gfbe_ctx *ctx, const gfbe_lc4_options *opt /* NULL: defaults */, int32_t n_poses, const double *t,
                           const double *ypr, const int32_t *sequence, const uint8_t *fixed, int32_t n_loop,
                           const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out,
                           double *yaw_out, double *drift, gfbe_summary *summary);
gfbe_status gfbe_lc4_solve_long(gfbe_ctx *ctx, const gfbe_lc4_options *opt /* NULL: defaults */, int32_t n_poses, const double *t,
                                const double *ypr, const int32_t *sequence, const uint8_t *fixed, int32_t n_loop,
                                const int32_t *loop_i, const int32_t *loop_c, const double *loop_meas, double *t_out,
                                double *yaw_out, double *drift, gfbe_summary *summary);

/* ------------------------------------------------------------------------------------------
 * f3c dense RGB-D map of dense_map, what the loop-closure thread does with the solved poses (paths under dense_map/src/):
 *       addKeyFrame: gate, density < 3, the keyframe's list shrunk to the survivors   pose_graph.cpp:191-221   gfbe_dmap_add_keyframe
 *       updatePath: the map cleared and rebuilt at the corrected poses, density < 5   :997-1032                gfbe_dmap_rebuild
 *       RadiusOutlierRemoval 0.8 m / 10 neighbours, the published cloud               :228-239, :1041-1056     gfbe_dmap_filter
 *     The handle holds the keyframes' camera-frame point lists (KeyFrame::point_rgbd: float xyz, uint8 rgb) in one pool, in
 *     keyframe order then list order, the voxel table (key -> point count) and the cloud in insertion order (world float
 *     xyz, rgb, keyframe index, pool index). Conventions of gfbe_scan: operations run in order on the context's stream,
 *     every count lives in device memory and nothing but gfbe_dmap_size, the downloads and gfbe_dmap_filter waits for the
 *     device (an insert whose arrays exceed a 64 KB staging slot, about 3 900 points, also waits); without a GPU every
 *     entry point returns GFBE_NO_DEVICE; a bad argument returns GFBE_BAD_INPUT with gfbe_last_error set and the handle
 *     untouched.
 *     World point: pw = R(q) (R(q_ic) (double)p + t_ic) + P in FP64, quaternions x y z w and unit, products left to right
 *     per row; the stored and keyed point is (float)pw. Gate (insert only): dropped when pw.z > z_max || pw.z < z_min on the
 *     FP64 value; gated points leave the keyframe's list too. Voxel key per axis: floor(((double)pf - origin) / resolution)
 *     of the float point, valid for 0 <= key < 2^21 (with the defaults the box -10000 .. 10971.52 m); a NaN point or one
 *     outside the box is skipped and counted. PCL's octree key arithmetic is not part of the reference tree: this key is a
 *     stated deviation.
 *     Density cap: within one call the candidates are the call's points that pass the gate and have a key, in list order; a
 *     candidate is kept iff base + rank < cap, base = the voxel's count before the call, rank = the number of earlier
 *     candidates of this call in the same voxel; kept points raise the count. After a rebuild (cap 5) a voxel may hold 5,
 *     and a later insert (cap 3) keeps nothing there, as in the reference. No result depends on the order workgroups ran in.
 *     Capacity: an insert keeps, of the points it would keep, the first that fit the pool, and counts the rest in
 *     n_refused; an insert that meets a full pool or a full keyframe table is refused whole, all n points counted
 *     unexamined, and adds no keyframe. Never an out-of-bounds write. The table has the next power of two >= 2
 *     point_capacity slots, so a claim cannot fail.
 * ------------------------------------------------------------------------------------------ */
typedef struct gfbe_dmap gfbe_dmap;
typedef struct gfbe_dmap_options {
  int32_t struct_size;            /* sizeof(gfbe_dmap_options), written by gfbe_dmap_default_options */
  int32_t add_cap;                /* 3 (pose_graph.cpp:212), 1 .. 8 */
  int32_t rebuild_cap;            /* 5 (:1025), 1 .. 8 */
  int32_t filter_min_neighbors;   /* 10 (:236): a point is kept with MORE than this many points within the radius, itself
                                     counted. This is how PCL's RadiusOutlierRemoval is remembered (self counted, outlier
                                     when k <= min_pts); PCL is not in the reference tree, so it cannot be checked here */
  double resolution;              /* 0.01 (:29) */
  double origin;                  /* -10000 (:1004; the constructor's box has y_min = -1000, :34: both whole voxels) */
  double z_min, z_max;            /* -0.5, 2 (:201) */
  double ex_cam[7];               /* t_ic, q_ic (x y z w, unit); default identity */
  double filter_radius;           /* 0.8 (:234) */
} gfbe_dmap_options;
void gfbe_dmap_default_options(gfbe_dmap_options *opt);
/* GFBE_BAD_INPUT: point_capacity outside 1 .. 2^26, keyframe_capacity outside 1 .. 2^24, caps outside 1 .. 8, an options
 * struct of another size, non-finite options, a filter_radius too small for its coarse grid to cover the voxel box. */
gfbe_status gfbe_dmap_create(gfbe_ctx *ctx, int32_t point_capacity, int32_t keyframe_capacity,
                             const gfbe_dmap_options *opt /* NULL: defaults */, gfbe_dmap **out);
void gfbe_dmap_destroy(gfbe_ctx *ctx, gfbe_dmap *map);
/* addKeyFrame: a new keyframe at pose7 [t | q] with n points pts_cam [n][3], rgb [n][3]; cap = add_cap. The kept points are
 * appended to the cloud and, camera-frame, to the pool as the keyframe's list, both in ascending input index.
 * GFBE_BAD_INPUT: n < 0, n > point_capacity, a NULL array with n > 0, a non-finite pose. */
gfbe_status gfbe_dmap_add_keyframe(gfbe_ctx *ctx, gfbe_dmap *map, const double *pose7, int32_t n, const float *pts_cam,
                                   const uint8_t *rgb);
/* updatePath: the table and the cloud are cleared; the candidates are all pool points in pool order at pose7
 * [n_keyframes][7]; no gate; cap = rebuild_cap. The pool is not changed. GFBE_BAD_INPUT: n_keyframes is not the number of
 * keyframes held, a non-finite pose. Returns without waiting. */
gfbe_status gfbe_dmap_rebuild(gfbe_ctx *ctx, gfbe_dmap *map, int32_t n_keyframes, const double *pose7);
/* keep [n_cloud] = 1 iff more than filter_min_neighbors cloud points, the point itself counted, have
 * (dx dx + dy dy) + dz dz <= radius radius in FP64 on the float coordinates. xyz_out / rgb_out [n_cloud][3] (both or
 * neither): the kept points compacted in cloud order, what pub_octree publishes. Any output may be NULL; waits. */
gfbe_status gfbe_dmap_filter(gfbe_ctx *ctx, gfbe_dmap *map, uint8_t *keep, int32_t *n_keep, float *xyz_out,
                             uint8_t *rgb_out);
/* counts [GFBE_DMAP_N_COUNTS]: keyframes, stored points (the pool), cloud points, voxels, skipped (NaN or outside the
 * box; inserts and rebuilds), gated, refused for capacity (the last three since the handle was made), and the points the
 * last filter kept through its dense-cell fast path. Waits. */
#define GFBE_DMAP_N_COUNTS 8
gfbe_status gfbe_dmap_size(gfbe_ctx *ctx, gfbe_dmap *map, int32_t *counts);
/* The cloud in insertion order: xyz [n_cloud][3], rgb [n_cloud][3], kf [n_cloud], src [n_cloud] (pool index). Any may be
 * NULL; waits. */
gfbe_status gfbe_dmap_download_cloud(gfbe_ctx *ctx, gfbe_dmap *map, float *xyz, uint8_t *rgb, int32_t *kf, int32_t *src);
/* Keyframe k's list as it is now: *n, pts [n][3] camera frame, rgb [n][3] (pts / rgb NULL: the count only). Waits.
 * GFBE_BAD_INPUT: no such keyframe. */
gfbe_status gfbe_dmap_download_keyframe(gfbe_ctx *ctx, gfbe_dmap *map, int32_t k, int32_t *n, float *pts, uint8_t *rgb);

/* ------------------------------------------------------------------------------------------
 * f3d loop database of dense_map: what produces the loop edges that gfbe_lc4_solve consumes (paths under dense_map/src/;
 *     DBoW2 is vendored under ThirdParty/DBoW/):
 *       detectLoop: BoW vector, query, add, the decision             pose_graph.cpp:432-512          gfbe_ldb_add_keyframe, detect_loop = 1
 *       addKeyFrameIntoVoc: add without a query                      :514-527                        gfbe_ldb_add_keyframe, detect_loop = 0
 *       searchByBRIEFDes / searchInAera / HammingDis, reduceVector   keyframe.cpp:194-244, 571-576, 374-380   gfbe_ldb_match
 *     PnPRANSAC (cv::solvePnPRansac) and the loop_info arithmetic behind it are gfbe_pnp_* of the companion header gfbe_pnp.h.
 *     A descriptor is uint64_t [4], the four blocks loadBin hands to boost::dynamic_bitset (TemplatedVocabulary.h:1541); pts /
 *     pts_norm are float [n][2] (keypoints[i].pt, keypoints_norm[i].pt). Conventions of gfbe_dmap: operations run in order on
 *     the context's stream, the counts live in device memory, without a GPU every entry point returns GFBE_NO_DEVICE, a bad
 *     argument returns GFBE_BAD_INPUT with gfbe_last_error set and the handle untouched.
 *     Every rule below is an integer operation or an IEEE FP64 addition, subtraction, fabs, comparison or division in a stated
 *     order (no multiply-add), and the device returns the bits of a sequential FP64 walk: word ids, BoW values, scores, result
 *     order, loop_index and every match output. No result depends on the order workgroups ran in or on what the scratch or
 *     the pools held before.
 *     1 Descent (TemplatedVocabulary.h:1217-1258): from the root, among the node's children in file order take the one with
 *       the smallest Hamming distance, a later child only with a strictly smaller distance; stop at a leaf (isLeaf, :1253,
 *       wherever it sits: trees need not be balanced, a node may have fewer than k children). Result: the leaf's word id, weight.
 *     2 BoW vector (:1065-1121, BowVector.cpp:34-84): a word met c times has the value ((w + w) + w) + ..., c - 1 additions, not
 *       c w; words with w <= 0 are dropped; norm = the sum of fabs(value) in ascending word id from 0.0; every value is divided
 *       by the norm when it is > 0.
 *     3 Query (TemplatedDatabase.h:656-723): entry e takes part iff e < max_id || max_id == -1 || e == n_entries - 1, with
 *       max_id = frame_index - query_gap and n_entries the count before this keyframe is added: the previous keyframe always
 *       takes part, at frame_index == query_gap - 1 every entry does (max_id is -1), below that only the previous one. An
 *       entry with no word in common is absent. raw = the sum over the common words in ascending word id of
 *       (fabs(q - d) - fabs(q)) - fabs(d), from the first term. The results are the max_results smallest in (raw, id) order:
 *       ascending raw, ties to the lower id (std::sort leaves ties open: a stated deviation). The
 *       reported score is -raw / 2.0.
 *     4 Decision (pose_graph.cpp:476-511): find_loop iff there is a result, score[0] > score_first and some i >= 1 has
 *       score[i] > score_other. When find_loop && frame_index > min_loop_frame, loop_index starts as result 0's id, taken
 *       unconditionally, and a later result replaces it only when its id is lower and its score is above score_other;
 *       otherwise loop_index = -1. frame_index is the entry id: the count of keyframes held before the call (:98).
 *     5 Add: the keyframe's BoW vector, descriptors and keypoints are appended to the handle's pools. n = 0 is a valid keyframe
 *       with an empty vector. REFUSAL: a keyframe that does not fit keyframe_capacity or descriptor_capacity is refused whole:
 *       the handle is unchanged, index_out = -1, loop_index = -1, no result, the call returns GFBE_OK and the keyframe is counted
 *       in n_refused. From then on the caller's keyframe indices and the database's part ways: the caller has to size the pools.
 *     6 Match (keyframe.cpp:194-244): per window descriptor best = match_start, index = -1; over the old keyframe's descriptors in
 *       order a strictly smaller distance wins, so a distance of match_start or more never does; status = 1 iff index != -1 &&
 *       best < match_max. matched_src = the window indices with status 1, ascending (reduceVector); matched_pt / matched_pt_norm
 *       = the old keyframe's pt / pt_norm at their best indices. The caller reduces its own point_3d, point_id and the rest with
 *       matched_src and compares n_matched with MIN_LOOP_NUM (25, keyframe.h:29) before its PnP.
 *     Vocabulary: plain arrays in the order of the vocabulary file as loadBin reads it (TemplatedVocabulary.h:1509-1561); the
 *     children of a node are its nodes in file order (push_back, :1538), which decides ties. Accepted: scoring 0 (L1) with
 *     weighting 0 (TF-IDF) or 1 (TF), one code path once the weights are read (:1081-1093, mustNormalize true). Checked on the
 *     host, GFBE_BAD_INPUT otherwise: node ids 1 .. n_nodes each once; a parent is the root (0) or an earlier-defined id; every
 *     leaf has exactly one word and every word a leaf, word ids 0 .. n_words - 1 each once; finite non-negative weights; at
 *     most GFBE_LDB_MAX_CHILDREN children per node (256: the child position is the low byte of the descent's packed key); depth
 *     at most 16; 1 <= k <= GFBE_LDB_MAX_CHILDREN and 1 <= L <= 16 (neither bounds the tree beyond that).
 * ------------------------------------------------------------------------------------------ */
#define GFBE_LDB_MAX_CHILDREN 256
#define GFBE_LDB_MAX_RESULTS 16
#define GFBE_LDB_MAX_KEYFRAME_DESCRIPTORS 4096
typedef struct gfbe_ldb gfbe_ldb;
typedef struct gfbe_ldb_vocab {
  int32_t k, L;                   /* branching factor and depth levels of the file's header */
  int32_t scoring, weighting;     /* ScoringType (0 = L1_NORM), WeightingType (0 = TF_IDF, 1 = TF) */
  int32_t n_nodes;                /* without the root */
  int32_t n_words;
  const int32_t *node_id;         /* [n_nodes] */
  const int32_t *parent_id;       /* [n_nodes], 0 = the root */
  const double *weight;           /* [n_nodes] */
  const uint64_t *descriptor;     /* [n_nodes][4] */
  const int32_t *word_id;         /* [n_words] */
  const int32_t *word_node;       /* [n_words] node id of the word's leaf */
} gfbe_ldb_vocab;
typedef struct gfbe_ldb_options {
  int32_t struct_size;                /* sizeof(gfbe_ldb_options), written by gfbe_ldb_default_options */
  int32_t max_results;                /* 4 (pose_graph.cpp:447), 1 .. GFBE_LDB_MAX_RESULTS */
  int32_t query_gap;                  /* 50 (:447): max_id = frame_index - query_gap, >= 0 */
  int32_t min_loop_frame;             /* 50 (:500): a loop needs frame_index > min_loop_frame */
  int32_t max_keyframe_descriptors;   /* 4096: descriptors of one keyframe, 1 .. GFBE_LDB_MAX_KEYFRAME_DESCRIPTORS */
  int32_t match_start;                /* 128 (keyframe.cpp:202), 1 .. 257 */
  int32_t match_max;                  /* 80 (:215), >= 0 */
  int32_t reserved;
  double score_first;                 /* 0.05 (pose_graph.cpp:476) */
  double score_other;                 /* 0.015 (:480, :505) */
} gfbe_ldb_options;
void gfbe_ldb_default_options(gfbe_ldb_options *opt);
/* The vocabulary is checked and copied to the device; the pools hold up to keyframe_capacity keyframes and descriptor_capacity
 * descriptors (and as many BoW words). GFBE_BAD_INPUT: a vocabulary that fails a check above, keyframe_capacity outside
 * 1 .. 2^24, descriptor_capacity outside 1 .. 2^26, an option outside its range or non-finite, an options struct of another size. */
gfbe_status gfbe_ldb_create(gfbe_ctx *ctx, const gfbe_ldb_vocab *voc, int32_t keyframe_capacity, int64_t descriptor_capacity,
                            const gfbe_ldb_options *opt /* NULL: defaults */, gfbe_ldb **out);
void gfbe_ldb_destroy(gfbe_ctx *ctx, gfbe_ldb *db);
/* Rules 1 and 2 on n descriptors without any change to the database: word_out [n] (the word of every descriptor, stopped words
 * included), *n_bow, bow_word / bow_value [up to n] ascending. Any output may be NULL; waits.
 * GFBE_BAD_INPUT: n < 0, n > max_keyframe_descriptors, desc NULL with n > 0. */
gfbe_status gfbe_ldb_transform(gfbe_ctx *ctx, gfbe_ldb *db, int32_t n, const uint64_t *desc, int32_t *word_out, int32_t *n_bow,
                               int32_t *bow_word, double *bow_value);
/* Rules 1 to 5 for one keyframe. detect_loop = 1 is detectLoop: it waits once, for loop_index and the results: *n_results,
 * result_id / result_score [max_results], best first. detect_loop = 0 is addKeyFrameIntoVoc: no query, loop_index = -1,
 * *n_results = 0, and no wait unless the arrays exceed a 64 KB staging slot (about 1 190 descriptors). *index_out = the entry id
 * of the keyframe, or -1 when it was refused (rule 5). Any output may be NULL.
 * GFBE_BAD_INPUT: n < 0, n > max_keyframe_descriptors, a NULL input array with n > 0. */
gfbe_status gfbe_ldb_add_keyframe(gfbe_ctx *ctx, gfbe_ldb *db, int32_t n, const uint64_t *desc, const float *pts,
                                  const float *pts_norm, int32_t detect_loop, int32_t *index_out, int32_t *loop_index,
                                  int32_t *n_results, int32_t *result_id, double *result_score);
/* Rule 6 of n_window descriptors against held keyframe old_index: status [n_window], best_index / best_dist [n_window] for every
 * window descriptor, *n_matched, matched_src [up to n_window], matched_pt / matched_pt_norm [up to n_window][2]. Any output may
 * be NULL; waits once. GFBE_BAD_INPUT: old_index is not a held keyframe, n_window outside 0 .. 2^20, window_desc NULL with
 * n_window > 0. */
gfbe_status gfbe_ldb_match(gfbe_ctx *ctx, gfbe_ldb *db, int32_t old_index, int32_t n_window, const uint64_t *window_desc,
                           uint8_t *status, int32_t *best_index, int32_t *best_dist, int32_t *n_matched, int32_t *matched_src,
                           float *matched_pt, float *matched_pt_norm);
/* counts [GFBE_LDB_N_COUNTS]: keyframes, descriptors, BoW words held, and the keyframes refused since the handle was made. Waits. */
#define GFBE_LDB_N_COUNTS 4
gfbe_status gfbe_ldb_size(gfbe_ctx *ctx, gfbe_ldb *db, int32_t *counts);
/* Entry e as it is held: *n_bow, bow_word / bow_value [n_bow] ascending, *n_desc, desc [n_desc][4], pts / pts_norm [n_desc][2]
 * (arrays NULL: the counts only). Waits. GFBE_BAD_INPUT: no such entry. */
gfbe_status gfbe_ldb_download_entry(gfbe_ctx *ctx, gfbe_ldb *db, int32_t e, int32_t *n_bow, int32_t *bow_word, double *bow_value,
                                    int32_t *n_desc, uint64_t *desc, float *pts, float *pts_norm);

/* ------------------------------------------------------------------------------------------
 * f4  LIO scan residuals (BASELINE configs[4]): point-to-plane factors of the LiDAR
 *     odometry, evaluated and reduced to normal equations on the device (the voxel neighbour search that produces
 *     the planes runs on the device too: the voxel map section below, gfbe_vmap_associate / gfbe_vmap_linearize):
 *       LidarPlaneNormFactor::Evaluate     lio/src/liw/lidarFactor.cpp:18-51   (ct = 0: one pose [t | q(x,y,z,w)])
 *       CTLidarPlaneNormFactor::Evaluate   lio/src/liw/lidarFactor.cpp:59-120  (ct = 1: begin and end pose, the point
 *                                          is taken at slerp(alpha) / lerp(alpha) between them)
 *     residual = sqrt_info * weight * (n . (R p + t) + offset); tangent = RotationParameterization (q * deltaQ(d),
 *     poseParameterization.cpp:31-42). Jacobian columns: ct = 0: [t(3) | theta(3)]; ct = 1: [t_b | theta_b | t_e | theta_e]
 *     (the parameter-block order of the factor). pts are the points the factor stores (point_body / raw_keypoint,
 *     already in the IMU frame). Outputs (any may be NULL): r [n], J [n][6 or 12], H [d][d] = J^T J, g [d] = J^T r,
 *     cost = 1/2 sum r^2.
 * ------------------------------------------------------------------------------------------ */
gfbe_status gfbe_lio_linearize(gfbe_ctx *ctx, int32_t ct, int32_t n, const double *pts, const double *normals,
                               const double *offsets, const double *alpha, const double *weights, double sqrt_info,
                               const double *pose_begin, const double *pose_end, double *r, double *J, double *H,
                               double *g, double *cost);

/* ------------------------------------------------------------------------------------------
 * f4b Device voxel map and scan-to-map association (lio/src/liw/lio/lidarodom.cpp): the step that produces the rows of
 *     gfbe_lio_linearize, without a trip through host memory.
 *       map_incremental / addPointToMap :1167-1266   gfbe_vmap_add_points
 *       lasermap_fov_segment            :1268-1284   gfbe_vmap_erase_far
 *       addSurfCostFactor, loop body    :929-1071    gfbe_vmap_associate (searchNeighbors :1086-1165,
 *                                                    computeNeighborhoodDistribution :887-927)
 *       checkLocalizability             :811-885     gfbe_vmap_localizability
 *     Conventions of gfbe_ltab: operations run in order on the context's stream; add_points / erase_far / upload return
 *     without waiting (arguments that do not fit a staging slot are waited for); without a GPU every entry point
 *     returns GFBE_NO_DEVICE. A voxel key is (short)(p / size_voxel_map) per axis, truncated toward zero; a point with
 *     |p / size| >= 32767 on an axis is skipped and counted. An add that would pass voxel_capacity changes nothing and
 *     raises a sticky overflow flag: gfbe_vmap_size reports it and gfbe_vmap_associate returns GFBE_BAD_INPUT from then
 *     on. No output depends on the table's layout or on the order in which workgroups ran. INTEGRATION.md lists the
 *     deviations from the reference (voxel_neighborhood 3 refused, ties by visit order, NaN a2D dropped and counted).
 * ------------------------------------------------------------------------------------------ */
typedef struct gfbe_vmap_options {
  int32_t struct_size;               /* sizeof(gfbe_vmap_options) as the caller was built (refused otherwise) */
  int32_t max_num_points_in_voxel;   /* 20 (1..32) */
  int32_t voxel_neighborhood;        /* 1 (0..2) */
  int32_t max_number_neighbors;      /* 20 (1..32) */
  int32_t min_number_neighbors;      /* 20 */
  int32_t threshold_voxel_occupancy; /* 1 */
  int32_t num_closest_neighbors;     /* 1 (1..max_number_neighbors) */
  int32_t max_num_residuals;         /* 2000 */
  double size_voxel_map;             /* 0.2 */
  double min_distance_points;        /* 0.05 */
  double max_distance;               /* 500 */
  double max_dist_to_plane_icp;      /* 0.3 */
  double power_planarity;            /* 2 */
  double weight_alpha;               /* 0.9 */
  double weight_neighborhood;        /* 0.1 */
} gfbe_vmap_options;
void gfbe_vmap_default_options(gfbe_vmap_options *opt);

typedef struct gfbe_vmap gfbe_vmap;
/* opt NULL: the defaults. GFBE_BAD_INPUT: wrong struct_size, an option outside its range, voxel_capacity outside 1 .. 2^21. */
gfbe_status gfbe_vmap_create(gfbe_ctx *ctx, int32_t voxel_capacity, const gfbe_vmap_options *opt, gfbe_vmap **out);
void gfbe_vmap_destroy(gfbe_ctx *ctx, gfbe_vmap *map);
/* map_incremental: equal to adding pts_world [n][3] one after another in input order. */
gfbe_status gfbe_vmap_add_points(gfbe_ctx *ctx, gfbe_vmap *map, int32_t n, const double *pts_world, int32_t min_num_points);
/* lasermap_fov_segment: a voxel goes when its FIRST point is farther than max_distance from location [3]. */
gfbe_status gfbe_vmap_erase_far(gfbe_ctx *ctx, gfbe_vmap *map, const double *location);
/* any output may be NULL; waits for the operations queued before it */
gfbe_status gfbe_vmap_size(gfbe_ctx *ctx, gfbe_vmap *map, int32_t *n_voxels, int32_t *n_points, int32_t *n_skipped,
                           int32_t *overflow);
/* Voxels in ascending (x, y, z) key order: keys [n_voxels][3], counts [n_voxels], points [n_points][3] concatenated in
 * voxel order, insertion order inside a voxel. upload replaces the map's contents (for tests and for seeding a map). */
gfbe_status gfbe_vmap_download(gfbe_ctx *ctx, gfbe_vmap *map, int16_t *keys, int32_t *counts, double *points);
gfbe_status gfbe_vmap_upload(gfbe_ctx *ctx, gfbe_vmap *map, int32_t n_voxels, const int16_t *keys, const int32_t *counts,
                             const double *points);
/* The loop body of addSurfCostFactor for a whole scan: raw_pts [n][3], alpha [n] (ct = 1), poses [t | q(x,y,z,w)] as in
 * gfbe_lio_linearize; frame_init != 0: 2 voxels visited, occupancy threshold 1. Outputs in keypoint order, cut at
 * max_num_residuals (any may be NULL; they hold up to min(n * num_closest_neighbors, max_num_residuals) rows): n_res,
 * src [n_res] keypoint index, pts [n_res][3] (ct = 1: the raw point; ct = 0: point_end), normals, offsets, alpha_out,
 * weights; per keypoint neighbor_count [n], a2D [n], neighbor_visit [n][max_number_neighbors] (the neighbours' identities: their
 * index in the search's visit order, voxels kxx, kyy, kzz then the point's place, -1 behind the last); n_nan: keypoints dropped
 * for a NaN a2D. The rows stay on the handle. */
gfbe_status gfbe_vmap_associate(gfbe_ctx *ctx, gfbe_vmap *map, int32_t ct, int32_t n, const double *raw_pts,
                                const double *alpha, const double *pose_begin, const double *pose_end, int32_t frame_init,
                                int32_t *n_res, int32_t *src, double *pts, double *normals, double *offsets,
                                double *alpha_out, double *weights, int32_t *neighbor_count, double *a2D, int32_t *n_nan,
                                int32_t *neighbor_visit);
/* gfbe_lio_linearize on the rows held on the handle (bit-identical to the host-fed call on the downloaded rows).
 * GFBE_BAD_INPUT when the map changed after the last associate, or ct differs from the association's. */
gfbe_status gfbe_vmap_linearize(gfbe_ctx *ctx, gfbe_vmap *map, int32_t ct, double sqrt_info, const double *pose_begin,
                                const double *pose_end, double *r, double *J, double *H, double *g, double *cost);
/* checkLocalizability on the held normals: sv [3] descending, degenerate = N <= 10 || mean(sv) < 10 || sv[2] < 7. */
gfbe_status gfbe_vmap_localizability(gfbe_ctx *ctx, gfbe_vmap *map, double *sv, int32_t *degenerate);

/* ------------------------------------------------------------------------------------------
 * f4c Scan-to-map registration loop on the device: one call of lidarodom::optimize from the head of its ICP loop to the
 *     loop's end (lio/src/liw/lio/lidarodom.cpp:534-748; gridSampling in front of the loop: the caller's, or f4d's):
 *       the ICP loop, exit test           lidarodom.cpp:534-748      gfbe_vmap_register
 *       addSurfCostFactor                 :929-1071                  (gfbe_vmap_associate's kernels, at the current poses)
 *       point-to-plane factors            lidarFactor.cpp:18-120     (the rows of gfbe_lio_linearize) under HuberLoss(0.5)
 *       Location / Rotation / SmallVelocity consistency factors      lidarFactor.cpp:125-219 (ct = 1 only, no loss)
 *       Plus: q * deltaQ(d), normalised   poseParameterization.cpp:31-50
 *       checkLocalizability               lidarodom.cpp:811-885      (on the last association)
 *       transformKeypoints + map_incremental  :509-532, :758, :1167-1266   gfbe_vmap_add_scan
 *     The inner solve is Ceres 1.14's Levenberg-Marquardt with the rules gfbe_pg_solve follows (radius 1e4, Jacobi
 *     scaling, diagonal clamp, step quality 1e-3, the three tolerances); lm_termination: 0 iteration cap, 1 function
 *     tolerance, 2 parameter tolerance, 3 gradient tolerance, 4 radius / five invalid steps in a row. The loop and its
 *     decisions run on the device: one upload, a fixed sequence of launches, one host wait. ct = 0: pose_begin is the
 *     pose (as in gfbe_vmap_associate), pose_end is carried unchanged (NULL: a copy of pose_begin's input).
 *     Deviations: the acos of the exit test is clamped to [-1, 1]; an association without residuals
 *     ends the loop (no_residuals = 1, poses as they are); a solve Ceres would call unusable returns
 *     GFBE_NUMERICAL_FAILURE with every output written at the last accepted poses.
 *     GFBE_BAD_INPUT: as gfbe_vmap_associate, a wrong struct_size, an option out of range, the sticky overflow flag
 *     (outputs untouched). On GFBE_OK the handle holds the last association (gfbe_vmap_linearize / _localizability).
 * ------------------------------------------------------------------------------------------ */
typedef struct gfbe_vreg_options {
  int32_t struct_size;                 /* refused when it differs, as gfbe_vmap_options */
  int32_t max_num_iteration;           /* 10 (1..32)  outer ICP iterations */
  int32_t lm_max_num_iterations;       /* 5  (0..16)  options.max_num_iterations of the inner solve */
  int32_t min_num_residuals;           /* 300: reported only, as the reference only prints */
  double laser_point_cov;              /* 0.001; sqrt_info of the factors = sqrt(1 / laser_point_cov) */
  double huber_delta;                  /* 0.5; <= 0: no loss */
  double beta_location_consistency;    /* 1.0 */
  double beta_orientation_consistency; /* 1.0 */
  double beta_small_velocity;          /* 0.0 */
  double thres_translation_norm;       /* 0.01 m */
  double thres_orientation_norm;       /* 0.1 deg */
} gfbe_vreg_options;

typedef struct gfbe_vreg_summary {      /* every field written whenever the call returns GFBE_OK */
  int32_t outer_iterations, converged, too_few_residuals, no_residuals, degenerate;
  double sv[3];
  int32_t n_res[32], lm_iterations[32], lm_accepted[32];   /* lm_accepted: bit i = inner step i was accepted */
  int32_t lm_termination[32];                              /* codes as gfbe_pg_solve's summary uses them */
  double cost_initial[32], cost_final[32], diff_trans[32], diff_rot[32];
  double pose_trace[32][14];                               /* [begin | end] after each outer iteration */
} gfbe_vreg_summary;

void gfbe_vreg_default_options(gfbe_vreg_options *opt);
/* opt NULL: the defaults. prev_translation [3], prev_rotation [4] (x,y,z,w): the previous frame's end pose (ct = 1; NULL: zero /
 * identity, the reference's first frames). summary may be NULL; pose_end_out may be NULL for ct = 0. */
gfbe_status gfbe_vmap_register(gfbe_ctx *ctx, gfbe_vmap *map, const gfbe_vreg_options *opt, int32_t ct, int32_t n,
                               const double *raw_pts, const double *alpha, const double *pose_begin, const double *pose_end,
                               const double *prev_translation, const double *prev_rotation, int32_t frame_init,
                               double *pose_begin_out, double *pose_end_out, gfbe_vreg_summary *summary);
/* The scan's world points (lio_world_point on the device) added to the map as gfbe_vmap_add_points adds them; returns
 * without waiting unless pts_world_out [n][3] is given. */
gfbe_status gfbe_vmap_add_scan(gfbe_ctx *ctx, gfbe_vmap *map, int32_t ct, int32_t n, const double *raw_pts,
                               const double *alpha, const double *pose_begin, const double *pose_end,
                               int32_t min_num_points, double *pts_world_out /* [n][3], may be NULL */);

/* ------------------------------------------------------------------------------------------
 * f4d Device-resident LiDAR scan: what the reference does on the host between the driver's cloud and lidarodom::optimize,
 *     and the hand-over of the result to the registration and the map update (paths under lio/src/):
 *       subSampleFrame            apps/main_eskf.cpp:56-64, common/utility.cpp:34-54             gfbe_scan_subsample
 *       Undistort / PoseInterp    liw/lio/lidarodom.cpp:1578-1600, common/math_utils.h:530-585    gfbe_scan_undistort
 *       transformPoint            lidarodom.cpp:1301-1304, common/utility.cpp:91-111              gfbe_scan_keypoints
 *       gridSampling              lidarodom.cpp:503-505, common/utility.cpp:56-71                 gfbe_scan_keypoints
 *       optimize on the keypoints :534-748                                                        gfbe_vmap_register_scan
 *       map_incremental           :758, :1167-1266                                                gfbe_vmap_add_scan_handle
 *     Conventions of gfbe_vmap / gfbe_ltab: operations run in order on the context's stream; without a GPU every entry
 *     point returns GFBE_NO_DEVICE; a bad argument returns GFBE_BAD_INPUT with gfbe_last_error set and the handle
 *     untouched. Points are held in the IMU frame: til [t | q(x,y,z,w)] at upload applies T_IL once (NULL: identity, what
 *     every other LiDAR entry point assumes), so the T_IL^-1 .. T_IL sandwich of Undistort disappears.
 *     Voxel key (subsample on the held points, keypoints on the WORLD points): (short)(p / size_voxel) per axis, truncated
 *     toward zero, as gfbe_vmap; a point with |p / size| >= 32767 on an axis or a NaN coordinate is dropped and counted
 *     in n_skipped (the reference's cast is undefined there). size_voxel must be finite and > 0.
 *     One point per voxel: the kept SET is the reference's ("first pushed" = the LOWEST input index); the ORDER is
 *     ascending input index, where the reference has the iteration order of its unordered_map (a deliberate deviation).
 *     No result depends on the order workgroups ran in or on the layout of a table.
 *     Undistort, the time rule (PoseInterp restated): a stamp q behind the last state time gives Ti = T_end (inside and
 *     outside the reference's 0.5 s allowance: it leaves Ti = T_end when it returns false); otherwise the first k with
 *     t_k < q && t_k+1 >= q; when there is none (q <= t_0) segment 0 with s = (q - t_0) / (t_1 - t_0) as it comes out
 *     (s <= 0: extrapolation, the reference's arithmetic); |t_k+1 - t_k| < 1e-6: Ti = T_k; n_states == 1: every point gets
 *     T_end (the reference dereferences end()). Ti = (slerp(q_k, s, q_k+1) normalised, p_k (1 - s) + p_k+1 s); the new
 *     point is T_end^-1 Ti p. State quaternions must be unit.
 *     A LiDAR frame has TWO host waits with the handle: gfbe_scan_keypoints (the counts) and gfbe_vmap_register_scan.
 * ------------------------------------------------------------------------------------------ */
typedef struct gfbe_scan gfbe_scan;
/* GFBE_BAD_INPUT: point_capacity outside 1 .. 2^21. */
gfbe_status gfbe_scan_create(gfbe_ctx *ctx, int32_t point_capacity, gfbe_scan **out);
void gfbe_scan_destroy(gfbe_ctx *ctx, gfbe_scan *scan);
/* The cloud as CloudConvert leaves it: raw_pts [n][3], alpha [n], timestamp [n] or NULL (then gfbe_scan_undistort is
 * refused; downloads give 0), til [7] or NULL. Replaces the handle's contents and clears the keypoints and n_skipped.
 * n > point_capacity: GFBE_BAD_INPUT. Returns without waiting when the arrays fit a staging slot. */
gfbe_status gfbe_scan_upload(gfbe_ctx *ctx, gfbe_scan *scan, int32_t n, const double *raw_pts, const double *alpha,
                             const double *timestamp, const double *til);
/* subSampleFrame: keeps, per voxel of size_voxel, the point of LOWEST input index; survivors stay in ascending input
 * index. Clears the keypoints; returns without waiting. */
gfbe_status gfbe_scan_subsample(gfbe_ctx *ctx, gfbe_scan *scan, double size_voxel);
/* Undistort: n_states (1 .. 512) nominal states, state_time [n_states] finite and ascending, state_pose [n_states][7];
 * T_end = the last state. Clears the keypoints; returns without waiting. */
gfbe_status gfbe_scan_undistort(gfbe_ctx *ctx, gfbe_scan *scan, int32_t n_states, const double *state_time,
                                const double *state_pose);
/* transformPoint + gridSampling: world points at (ct, pose_begin, pose_end) exactly as gfbe_vmap_add_scan forms them
 * (bit-identical to its pts_world_out), then one keypoint per voxel of size_voxel of the WORLD point (lowest index,
 * ascending index order). The points stay as they are. Waits; writes the keypoint count (n_keypoints may be NULL). */
gfbe_status gfbe_scan_keypoints(gfbe_ctx *ctx, gfbe_scan *scan, int32_t ct, const double *pose_begin,
                                const double *pose_end, double size_voxel, int32_t *n_keypoints);
/* any output may be NULL; waits. n_keypoints: 0 until gfbe_scan_keypoints ran on the scan as it is now. n_skipped: points
 * dropped by gfbe_scan_subsample since the upload + points without a voxel in the last gfbe_scan_keypoints. */
gfbe_status gfbe_scan_size(gfbe_ctx *ctx, gfbe_scan *scan, int32_t *n_points, int32_t *n_keypoints, int32_t *n_skipped);
/* which 0: the points, 1: the keypoints (their IMU-frame point, not the world point). src = index in the uploaded
 * cloud; any output may be NULL; waits. */
gfbe_status gfbe_scan_download(gfbe_ctx *ctx, gfbe_scan *scan, int32_t which, int32_t *src, double *pts, double *alpha,
                               double *timestamp);
/* gfbe_vmap_register on the handle's KEYPOINTS (points + alpha in keypoint order; max_num_residuals cuts in that order), no
 * geometry through the host: the same kernels in the same order on the same values as the host-fed call on the downloaded
 * keypoints, bit-identical outputs. GFBE_BAD_INPUT also: no gfbe_scan_keypoints since the last upload / subsample /
 * undistort; a handle of another context. */
gfbe_status gfbe_vmap_register_scan(gfbe_ctx *ctx, gfbe_vmap *map, const gfbe_vreg_options *opt, int32_t ct, gfbe_scan *scan,
                                    const double *pose_begin, const double *pose_end, const double *prev_translation,
                                    const double *prev_rotation, int32_t frame_init, double *pose_begin_out,
                                    double *pose_end_out, gfbe_vreg_summary *summary);
/* gfbe_vmap_add_scan on the handle's POINTS (lidarodom.cpp:758 + map_incremental); returns without waiting (when the
 * point count changed since the host last read it — a subsample without a later gfbe_scan_keypoints / _size — it is read
 * back first). */
gfbe_status gfbe_vmap_add_scan_handle(gfbe_ctx *ctx, gfbe_vmap *map, int32_t ct, gfbe_scan *scan, const double *pose_begin,
                                      const double *pose_end, int32_t min_num_points);

/* ------------------------------------------------------------------------------------------
 * f2  Optional in-window factors. PlaneFactor and PoseAnchorFactor run INSIDE
 *     gfbe_solve_window / gfbe_batch_solve when gfbe_window.use_plane / use_anchor are set (see gfbe_window); the
 *     functions below evaluate them stand-alone. The GNSS factors run inside the solve and MARGIN_OLD as well when
 *     gfbe_window.gnss_ready is set: the problem then grows by rcv_dt[11][4], rcv_ddt[11], yaw_enu_local and anc_ecef
 *     (59 more tangent dimensions, GFBE_DENSE_DIM = 246); such batches factorise their reduced system from global memory
 *     (k_solve_big) instead of the LDS-resident kernels. Every shipped yaml sets gnss_enable: 0.
 *       PlaneFactor::Evaluate        factor/plane_factor.h:25-122  — n factors sharing ex_wheel [p | q(x,y,z,w)],
 *           plane_R [q(x,y,z,w)] and plane_Z (estimator.cpp:3214-3220: one factor per window pose);
 *           noise_inv = {PITCH_N_INV, ROLL_N_INV, ZPW_N_INV} (parameters.cpp:340-345).
 *           r [n][3]; J [n][3][16], tangent columns = pose_i(6) ex_wheel(6) plane_R(3) plane_Z(1).
 *       PoseAnchorFactor::Evaluate   factor/pose_anchor_factor.cpp:8-32 — sqrt_info = 120 in the reference
 *           (pose_anchor_factor.h:19). r [n][6]; J [n][6][6] (tangent of the pose). The reference's Jacobian is 2 sqrt_info
 *           times [I 0; 0 Qright(q_anchor^-1)] — twice the derivative of its own position residual; reproduced as it is.
 *       OrientationSubsetParameterization::Plus   factor/orientation_subset_parameterization.cpp:27-45 (host function):
 *           out = normalize(q * deltaQ(delta with the constant components zeroed)); plane_R uses constant = {0, 0, 1}
 *           (estimator.cpp:3122).
 *     r, J, cost may be NULL. cost = 1/2 sum r^2.
 * ------------------------------------------------------------------------------------------ */
gfbe_status gfbe_plane_eval(gfbe_ctx *ctx, int32_t n, const double *pose /*[n][7]*/, const double *ex_wheel /*[7]*/,
                            const double *plane_R /*[4]*/, double plane_Z, const double *noise_inv /*[3]*/, double *r,
                            double *J, double *cost);
gfbe_status gfbe_anchor_eval(gfbe_ctx *ctx, int32_t n, const double *pose /*[n][7]*/, const double *anchor /*[n][7]*/,
                             double sqrt_info, double *r, double *J, double *cost);
void gfbe_orientation_subset_plus(const double *q /*[4] x y z w*/, const double *delta /*[3]*/,
                                  const uint8_t *constant /*[3]*/, double *out /*[4]*/);

/* ------------------------------------------------------------------------------------------
 * f2  GNSS factors of the window (estimator.cpp:3239-3291), evaluated stand-alone on the device (inspection / parity API; inside
 *     the solve they are driven by gfbe_window.gnss_*):
 *       GnssPsrDoppFactor::Evaluate   factor/gnss_psr_dopp_factor.cpp:50-208   (2 rows: pseudo-range, Doppler)
 *       DtDdtFactor::Evaluate         factor/gnss_dt_ddt_factor.cpp:3-34       (receiver clock bias / drift chain)
 *       DdtSmoothFactor::Evaluate     factor/gnss_ddt_smooth_factor.cpp:3-22
 *     together with the gnss_comm functions the pseudo-range factor calls per evaluation (gnss_comm/src/gnss_utility.cpp:
 *     ecef2geo :347, ecef2rotation :757, sat_azel :762, calculate_trop_delay :841 — Saastamoinen + Niell mapping,
 *     calculate_ion_delay :865 — Klobuchar). What the factor's CONSTRUCTOR derives from the observation and the
 *     broadcast ephemeris (gnss_psr_dopp_factor.cpp:3-47: eph2pos / geph2pos / eph2svdt at the transmission time, the
 *     group delay, the URA scalings) is front-end work and crosses the boundary precomputed in gfbe_gnss_obs.
 * ------------------------------------------------------------------------------------------ */
/* (gfbe_gnss_obs and gfbe_gnss_state are defined with gfbe_state near the top of this header) */

/* One thread per factor. iono: the 8 Klobuchar parameters (latest_gnss_iono_params) or NULL (no ionosphere term).
 * frame_dt[i] = Headers[i+1] - Headers[i]. Outputs (any may be NULL):
 *   r_obs [n_obs][2]; J_obs [n_obs][2][18] with columns P_lower(3) V_lower(3) P_upper(3) V_upper(3) rcv_dt rcv_ddt yaw_enu_local
 *   anc_ecef(3) — the non-zero parts of the reference's 2 x {7, 9, 7, 9, 1, 1, 1, 3} blocks; like the reference the Jacobian leaves
 *   out the atmosphere and Sagnac derivatives and approximates d/d anc_ecef;
 *   r_dt_ddt [4][GFBE_WINDOW_SIZE] (k-major, the reference's insertion order; Jacobian = {-50, 50, -25 dt, -25 dt});
 *   r_smooth [GFBE_WINDOW_SIZE] (Jacobian = {w, -w});
 *   cost = 1/2 sum r^2 over the three families, summed in the reference's insertion order. */
gfbe_status gfbe_gnss_eval(gfbe_ctx *ctx, int32_t n_obs, const gfbe_gnss_obs *obs, const double *iono /*[8] or NULL*/,
                           const gfbe_state *state, const gfbe_gnss_state *gnss, const double *frame_dt /*[WINDOW_SIZE]*/,
                           double ddt_weight, double *r_obs, double *J_obs, double *r_dt_ddt, double *r_smooth, double *cost);

/* ------------------------------------------------------------------------------------------
 * Line landmarks (use_line: 1). The line-only refinement every use_line frame runs before optimizationwithLine
 * (estimator.cpp:1426-1438), on the device:
 *   lineProjectionFactor::Evaluate           factor/line_projection_factor.cpp:18-231
 *   LineOrthParameterization::Plus           factor/line_parameterization.cpp:10-95
 *   Estimator::onlyLineOpt                   estimator.cpp:4264-4332 (poses and extrinsic constant, CauchyLoss(1.0), Ceres' default
 *                                            Levenberg-Marquardt, max_num_iterations = NUM_ITERATIONS)
 *   FeatureManager::getLineOrthVector / setLineOrth / removeLineOutlier   feature_manager.cpp:1068-1125, 1372-1460
 * Plücker lines are [n(3) | v(3)], orthonormal lines [theta(3) | phi], poses [p(3) | q(x, y, z, w)].
 * ------------------------------------------------------------------------------------------ */

/* gfbe_line_eval: n independent factors; factor k sees pose[k], the shared camera extrinsic, the world line orth[k] and the observed
 * endpoints obs[k] = [x1 y1 x2 y2] (normalised image plane). sqrt_info is FOCAL_LENGTH / 1.5 = 400 in the reference. robustify != 0
 * applies CauchyLoss(1.0) and its corrector (r and J scaled by sqrt(rho')). Outputs (any may be NULL): r [n][2]; J_pose [n][2][7] and
 * J_ex [n][2][7] (tangent columns dp(3) dtheta(3), the 7th zero, as the reference writes them); J_orth [n][2][4]; cost = sum of
 * 1/2 rho(|r|^2) (1/2 |r|^2 without the loss). */
gfbe_status gfbe_line_eval(gfbe_ctx *ctx, int32_t n, const double *pose /*[n][7]*/, const double *ex_cam /*[7]*/,
                           const double *orth /*[n][4]*/, const double *obs /*[n][4]*/, double sqrt_info, int32_t robustify,
                           double *r, double *J_pose, double *J_ex, double *J_orth, double *cost);

/* What FeatureManager::linefeature holds for one window, in list order. Observation k of line i is in frame start_frame[i] + k
 * (start_frame[i] + n_obs[i] <= GFBE_NFRAMES); the observations of all lines are packed in line order. */
typedef struct gfbe_line_window {
  int32_t struct_size;                /* sizeof(gfbe_line_window) as the caller was built (refused otherwise: GFBE_BAD_INPUT) */
  int32_t n_lines;
  const int32_t *start_frame;         /* [n_lines] */
  const int32_t *n_obs;               /* [n_lines] linefeature_per_frame.size() */
  const double *obs;                  /* [sum n_obs][4] lineobs */
  const uint8_t *is_triangulation;    /* [n_lines] */
  const double *line_plucker;         /* [n_lines][6] in the start frame's camera frame */
  double pose[GFBE_NFRAMES][7];       /* Ps / Rs of the window */
  double ex_cam[7];                   /* tic / ric */
} gfbe_line_window;

/* gfbe_line_refine: onlyLineOpt() followed by removeLineOutlier(Ps, tic, ric), for n_windows independent windows in one launch.
 * Eligible lines (n_obs >= LINE_MIN_OBS = 5, start_frame < GFBE_WINDOW_SIZE - 2, is_triangulation) are refined and written back through
 * setLineOrth; every other line comes back bit-identical. With fewer than 4 eligible lines nothing is solved, every line comes back
 * bit-identical and none is culled (estimator.cpp:4318-4321). plucker_out [sum n_lines][6] and keep_out [sum n_lines] are concatenated
 * in window order; keep_out[i] = 0: the reference erases line i. sqrt_info: 400 in the reference; cauchy_scale: 1.0;
 * max_num_iterations: NUM_ITERATIONS (8 in every shipped yaml; at most 15 are run). summary [n_windows] as gfbe_pg_solve fills it
 * (ms_solve: the window's time in the kernel); iterations = 0 and termination = 5 when the < 4 exit was taken.
 * Return value: the worst summary status. GFBE_BAD_INPUT / GFBE_NO_DEVICE / GFBE_DEVICE_ERROR: no output has been touched. */
gfbe_status gfbe_line_refine(gfbe_ctx *ctx, int32_t n_windows, const gfbe_line_window *const *win, double sqrt_info,
                             double cauchy_scale, int32_t max_num_iterations, double *plucker_out, uint8_t *keep_out,
                             gfbe_summary *summary);

/* ------------------------------------------------------------------------------------------
 * Reduced normal equations of a window's line factors: the line loops of optimizationwithLine() (estimator.cpp:4566-4598 for the solve,
 * :4736-4771 for MARGIN_OLD) linearised with respect to the poses, the camera extrinsic and the lines, the 4-dimensional line blocks
 * eliminated. With x_p the 72 tangent dims [pose 0 .. pose 10 (dp, dtheta) | ex_cam (dp, dtheta)] and x_l the orthonormal 4 dims of line l:
 *     U = sum Jp^T Jp (72 x 72), bp = sum Jp^T r; per line V_l = sum Jl^T Jl, bl = sum Jl^T r, W_l = sum Jp^T Jl (72 x 4)
 *     V'_l = V_l + mu diag(clamp(diag V_l, 1e-6, 1e32));   H = U - sum_l W_l V'_l^-1 W_l^T;   g = bp - sum_l W_l V'_l^-1 bl
 * r, Jp, Jl: lineProjectionFactor::Evaluate after ceres::HuberLoss(huber_width) and its corrector (rho'' <= 0: r and J scaled by
 * sqrt(rho')); huber_width <= 0: no loss. The reference uses sqrt_info = 400, HuberLoss(1.0) (estimator.cpp:4342). Lines enter through
 * getLineOrthVector as in gfbe_line_refine.
 * THE 72 DIMS ARE, IN THIS ORDER, DIMS 0..71 OF THE WINDOW'S DENSE BLOCK (poses 0..65, camera extrinsic 66..71):
 * joining H, g into the window solve is a plain add into the leading 72 x 72 corner / the first 72 entries.
 * mode GFBE_LINE_REDUCE_SOLVE: every line of gfbe_line_refine's predicate (n_obs >= 5, start_frame < GFBE_WINDOW_SIZE - 2,
 *   is_triangulation), list order, every observation including the start frame's own. There is no "fewer than 4 lines" exit here.
 * mode GFBE_LINE_REDUCE_MARG_OLD: of those only the lines with start_frame == 0, and their observation in frame 0 is skipped: the rows
 *   and columns of pose 0 are exactly zero. "Eligible" below means the lines that enter in the given mode.
 * A line whose V'_l has no Cholesky factor (a pivot that is not positive and finite) is left out of EVERY sum (U, bp and cost too),
 * flagged in `failed` and counted in n_failed. Observation values are not validated (gfbe_line_refine does not either): a NaN
 * observation makes its line such a line and nothing else.
 * Outputs: caller-owned, any pointer may be NULL. Per-line records are concatenated over the windows in list order of the eligible
 * lines; size them for the total number of lines, sum(n_eligible) records are written.
 * ------------------------------------------------------------------------------------------ */
enum { GFBE_LINE_REDUCE_SOLVE = 0, GFBE_LINE_REDUCE_MARG_OLD = 1, GFBE_LINE_REDUCE_DIM = 72 };
typedef struct gfbe_line_reduced {
  int32_t struct_size;                /* sizeof(gfbe_line_reduced) as the caller was built (refused otherwise: GFBE_BAD_INPUT) */
  int32_t reserved;                   /* 0 */
  double *H;                          /* [W][72][72] full, symmetric bit for bit */
  double *g;                          /* [W][72] */
  double *U;                          /* [W][72][72] the unreduced pose / extrinsic block */
  double *bp;                         /* [W][72] */
  double *cost;                       /* [W] sum of 1/2 rho */
  int32_t *n_eligible;                /* [W] */
  int32_t *n_failed;                  /* [W] */
  double *Vinv;                       /* [.][4][4] V'_l^-1 (symmetric bit for bit) */
  double *bl;                         /* [.][4] */
  double *W;                          /* [.][72][4] */
  uint8_t *failed;                    /* [.] 1: left out (its Vinv, bl, W are not meaningful) */
  double *ms_kernel;                  /* [W][2] the window's time in the kernel, and the part of it in the matrix-core contraction
                                         loop (device clock, like gfbe_summary.ms_solve) */
  double *V;                          /* [.][10] the lower triangle of V_l WITHOUT the mu term, row-major (00 10 11 20 21 22 30 31 32 33):
                                         what the step side needs beside V'_l^-1, which does not give V_l back when a diagonal is
                                         clamped. A caller built before this member existed passes the smaller struct_size
                                         (GFBE_LINE_REDUCED_SIZE_V0); both sizes are admitted, and the smaller one means V = NULL. */
} gfbe_line_reduced;
#define GFBE_LINE_REDUCED_SIZE_V0 ((int32_t)offsetof(gfbe_line_reduced, V))
/* Host-fed: the windows of gfbe_line_refine. GFBE_BAD_INPUT (bad mode, negative or non-finite mu, wrong struct_size of either
 * structure, observations past the window), GFBE_NO_DEVICE, GFBE_DEVICE_ERROR: no output has been touched. */
gfbe_status gfbe_line_reduce(gfbe_ctx *ctx, int32_t n_windows, const gfbe_line_window *const *win, int32_t mode, double sqrt_info,
                             double huber_width, double mu, gfbe_line_reduced *out);

/* ------------------------------------------------------------------------------------------
 * The step half of a joint trust-region iteration over the line blocks (solve mode only; MARG_OLD has no step): everything the
 * iteration does with the line blocks once the pose / extrinsic directions exist. The scalar landmark code of the window solve,
 * generalised to a 4-dimensional block in the coordinates of gfbe_line_reduce:
 *   - line columns are NOT Jacobi-scaled; the block's metric is d2_l = clamp(diag V_l, 1e-6, 1e32), the diagonal of the V'_l term above.
 *     While no diagonal is clamped every scalar below is invariant under Ceres' column scaling; with a clamped diagonal it is not (Ceres
 *     clamps the scaled diagonal) - a deviation, stated in DESIGN.md section 10.3;
 *   - pose / extrinsic vectors are in the same unscaled tangent coordinates as H, g.
 * Inputs per window: y_p [72] the caller's Gauss-Newton direction, (H_all + mu D^2) y = g_all; v_p [72] its D^-2 g_all; rest [8] the
 * eight scalars of everything that is not a line block, p = [G2, N2, gy, vHv, vHy, yHy, max|gradient|, |x|^2]; radius; the poses and
 * ex_cam the records were reduced at; mu, the one they were reduced with (V'_l^-1 carries it; it is validated and not used again).
 * Per entering, non-failed line with the records Vinv, bl, W, V:
 *     y_l = Vinv (bl - W^T y_p);   v_l = bl / d2_l
 *     G2 = sum bl^2 / d2;  N2 = sum d2 y_l^2;  gy = bl . y_l
 *     vHv = 2 v_l . W^T v_p + v_l^T V_l v_l;   vHy = v_l . W^T y_p + y_l . W^T v_p + v_l^T V_l y_l;   yHy = 2 y_l . W^T y_p + y_l^T V_l y_l
 *     max |x_l - Plus(x_l, -bl)|_inf (the gradient norm as Ceres takes it through the manifold);   |x_l|^2 over the four parameters
 * total = rest + the line shares (entry 6: the larger), summed in a fixed order. alpha = G2 / vHv; c1, c2, step_norm, model_change by
 * the three-branch dogleg rule of the window solve (Gauss-Newton inside the radius: 0, -1; Cauchy point outside: -radius / |g|, 0;
 * else the point of the dogleg on the boundary), step = c1 v + c2 y. model_change <= 0 (or NaN): invalid = 1, no candidate is formed -
 * every candidate array holds its input, cost_cand the largest double - and the caller raises mu and reduces again (HandleInvalidStep).
 * Otherwise delta_l = c1 v_l + c2 y_l, x_l' = LineOrthParameterization::Plus(x_l, delta_l); candidate poses and extrinsic =
 * Plus(., c1 v_p + c2 y_p) of the pose blocks; plucker_cand = x_l' expressed in the CANDIDATE start frame's camera (setLineOrth);
 * cost_cand = sum of 1/2 rho_huber over the entering lines' observations at the candidate poses and lines.
 * A failed line takes part in nothing: y_l = v_l = 0, orth_cand = x_l and plucker_cand = its input, bit for bit.
 * Per-line arrays are concatenated over the windows in the order of the records. Any pointer may be NULL.
 * ------------------------------------------------------------------------------------------ */
typedef struct gfbe_line_stepped {
  int32_t struct_size;                /* sizeof(gfbe_line_stepped) as the caller was built (refused otherwise: GFBE_BAD_INPUT) */
  int32_t reserved;                   /* 0 */
  double *gram;                       /* [W][8] the line shares */
  double *total;                      /* [W][8] rest + gram */
  double *coef;                       /* [W][4] c1, c2, step_norm, model_change */
  uint8_t *invalid;                   /* [W] */
  double *y_l;                        /* [.][4] */
  double *v_l;                        /* [.][4] */
  double *orth_cand;                  /* [.][4] */
  double *plucker_cand;               /* [.][6] in the candidate start frame's camera frame */
  double *pose_cand;                  /* [W][11][7] */
  double *ex_cand;                    /* [W][7] */
  double *cost_cand;                  /* [W] */
  double *ms_kernel;                  /* [W] the window's time in the kernel (device clock) */
} gfbe_line_stepped;
/* Host-fed, stateless: win and rec are the windows gfbe_line_reduce ran on (solve mode) and what it wrote for them - Vinv, bl, W, V,
 * failed, n_eligible, all required. y_p, v_p [W][72], rest [W][8], radius [W]. GFBE_BAD_INPUT: a wrong struct_size of any structure, a
 * missing record array, n_eligible that is not the windows' own count, a negative or non-finite mu or radius, a non-finite y_p, v_p or
 * rest. GFBE_NO_DEVICE, GFBE_DEVICE_ERROR as elsewhere. On any error no output has been touched. */
gfbe_status gfbe_line_step(gfbe_ctx *ctx, int32_t n_windows, const gfbe_line_window *const *win, const gfbe_line_reduced *rec,
                           double sqrt_info, double huber_width, double mu, const double *y_p, const double *v_p, const double *rest,
                           const double *radius, gfbe_line_stepped *out);

/* ------------------------------------------------------------------------------------------
 * Line feature tables: FeatureManager::linefeature on the device, and the line calls of a use_line frame against it
 *   addFeatureCheckParallaxwithline -> triangulateLine -> onlyLineOpt (+ removeLineOutlier) -> [optimizationwithLine on the CPU; its
 *   line loops reduced on the device by gfbe_ltab_reduce]
 *   -> slideWindow (removeBackShiftDepthline / removeBackline / removeFrontline)      estimator.cpp:1426-1438, 3859-3899
 * A gfbe_ltab holds W independent tables in HBM, one per window; every call applies one operation to all W tables, per-table arguments
 * are arrays of length W. A table is std::list<lineFeaturePerId> in insertion order — the order that defines the line index of
 * getLineOrthVector / setLineOrth / para_LineFeature[]. Per line: feature_id, start_frame, n_obs (<= GFBE_NFRAMES), the observations
 * lineobs [x1 y1 x2 y2] (observation k is in frame start_frame + k), is_triangulation and line_plucker[6] in the start frame's camera
 * frame. line_plucker of a line that was never triangulated is uninitialised memory in the reference (feature_manager.h:139-145); the
 * table holds zeros there. removed_cnt / all_obs_cnt / ptw1 / ptw2 / line_plk_init are only ever printed by the reference and are not
 * kept. Erasures keep the order.
 * Pose arguments as in the point tables: poses [W][11][12] = [P(3) | R(9, row-major)], tic_ric [W][12] — except gfbe_ltab_refine, which
 * takes the quaternion forms of gfbe_line_window so that it agrees with gfbe_line_refine bit for bit.
 * Every operation runs in order on the context's stream. The ones without outputs (triangulate, remove_*) copy their arguments and
 * return without waiting for the device; the ones that hand something back (add_frame, refine, size, line_count, download) and upload
 * wait for what was enqueued before them. Capacity / observation overflow is raised by gfbe_ltab_add_frame (GFBE_BAD_INPUT, sticky). A
 * device error of a deferred operation is reported by the next call that synchronises. gfbe_ltab_create leaves *out null and frees
 * what it had allocated when it fails; without a device every call returns GFBE_NO_DEVICE. line_capacity <= 16384 lines per table.
 * ------------------------------------------------------------------------------------------ */
typedef struct gfbe_ltab gfbe_ltab;
gfbe_status gfbe_ltab_create(gfbe_ctx *ctx, int32_t n_tables, int32_t line_capacity, gfbe_ltab **out);
void gfbe_ltab_destroy(gfbe_ctx *ctx, gfbe_ltab *t);
/* Line loop of addFeatureCheckParallaxwithline (feature_manager.cpp:149-170). Table w receives the lines [offset[w], offset[w+1]) —
 * ascending line_id, the iteration order of the reference's std::map — with observations obs4 [x1 y1 x2 y2]. A known id gets the
 * observation appended; an unknown id becomes a new line at the end of the list with start_frame = frame_count[w], not triangulated.
 * counters_out [W][2] = [tracked, new] (may be NULL). The keyframe decision is gfbe_ftab_add_frame's: lines take no part in it. */
gfbe_status gfbe_ltab_add_frame(gfbe_ctx *ctx, gfbe_ltab *t, const int32_t *frame_count, const int32_t *offset,
                                const int32_t *line_id, const double *obs4, int32_t *counters_out);
/* triangulateLine (feature_manager.cpp:1151-1262): every line with n_obs >= LINE_MIN_OBS (5), start_frame < WINDOW_SIZE - 2 that is
 * not yet triangulated: the plane through the start observation and the camera centre is intersected with the plane of the later
 * observation whose normal makes the SMALLEST cosine with it (strict <, the first wins); skipped while that cosine is above 0.998.
 * line_plucker = pipi_plk(pi_i, pi_j), not normalised. */
gfbe_status gfbe_ltab_triangulate(gfbe_ctx *ctx, gfbe_ltab *t, const double *poses, const double *tic_ric);
/* Line loop of removeBackShiftDepthline (feature_manager.cpp:1499-1527), applied ONCE per call (the reference nests it inside the
 * loop over the point features — a misplaced brace): start_frame != 0 is decremented; otherwise observation 0
 * is dropped, the line is erased when fewer than 2 are left, and else line_plucker moves into the new start frame,
 * plk_to_pose(line_plucker, new_R^T marg_R, new_R^T (marg_P - new_P)). *_PR = [W][12]. */
gfbe_status gfbe_ltab_remove_back_shift(gfbe_ctx *ctx, gfbe_ltab *t, const double *marg_PR, const double *new_PR);
/* Line loops of removeBackline (:896-911, erases at 0 observations left) and removeFrontline (:958-975). */
gfbe_status gfbe_ltab_remove_back(gfbe_ctx *ctx, gfbe_ltab *t);
gfbe_status gfbe_ltab_remove_front(gfbe_ctx *ctx, gfbe_ltab *t, const int32_t *frame_count);
/* onlyLineOpt() + removeLineOutlier(Ps, tic, ric) on every table, what gfbe_line_refine does for host lists, without leaving the
 * device: refined lines are written back, culled lines erased in order, ineligible lines untouched; a table with fewer than 4 eligible
 * lines stays as it was (summary.termination = 5). pose7 [W][11][7], ex_cam [W][7] = [p | q(x, y, z, w)] as in gfbe_line_window: with
 * the same pose bits the result equals gfbe_line_refine's bit for bit. summary [W]; return value: the worst summary status. */
gfbe_status gfbe_ltab_refine(gfbe_ctx *ctx, gfbe_ltab *t, const double *pose7, const double *ex_cam, double sqrt_info,
                             double cauchy_scale, int32_t max_num_iterations, gfbe_summary *summary);
/* gfbe_line_reduce on every table, read in place: the tables are not changed. pose7 [W][11][7], ex_cam [W][7] as for
 * gfbe_ltab_refine; with the same pose bits every output equals gfbe_line_reduce's on the downloaded list bit for bit. The call's
 * device scratch and output staging (4.8 KB per line slot, min(W, 256) x (largest table + 8) slots, plus the outputs asked for) stays on
 * the table handle between calls, grows to the largest size ever needed and is released by gfbe_ltab_destroy. */
gfbe_status gfbe_ltab_reduce(gfbe_ctx *ctx, gfbe_ltab *t, int32_t mode, const double *pose7, const double *ex_cam, double sqrt_info,
                             double huber_width, double mu, gfbe_line_reduced *out);
/* The step half against the tables (the product path; conventions: gfbe_line_step above). A joint iteration is
 *   gfbe_ltab_reduce -> the caller's 72-dim solve -> gfbe_ltab_step -> the caller's accept test -> gfbe_ltab_commit.
 * gfbe_ltab_keep_records: off by default (behaviour and memory as without it). While on, gfbe_ltab_reduce in solve mode also leaves every
 *   entering line's Vinv, bl, W, V, failed in a per-line store on the table handle (2.5 KB per line slot, one slot per line of the
 *   tables; grown on demand, released by gfbe_ltab_destroy), together with the mu and the pose bits of the call. The line's
 *   orthonormal form is not stored: the step forms it from the table and the poses with the operations of the reduce, the same bits.
 *   The outputs of gfbe_ltab_reduce keep their bits. Switching it off drops the store's contents.
 * gfbe_ltab_step: reads that store and the tables in place, keeps the candidates on the handle and copies down only what `out` asks
 *   for. y_p, v_p [W][72], rest [W][8], radius [W]. GFBE_BAD_INPUT when no records are held, when any gfbe_ltab_* operation has changed
 *   the tables since the reduce that wrote them (a generation counter on the handle), or when pose7 / ex_cam differ in any bit from the
 *   reduce's. With the same bits every output equals gfbe_line_step's on the downloaded list, bit for bit.
 * gfbe_ltab_commit: tables with accept[w] != 0 take their candidate Pluecker vectors (the entering, non-failed lines); every other
 *   table, every non-entering line and every failed line keeps its bits. Deferred like the other table operations without outputs.
 *   It invalidates the records and the candidates: the next step needs a new reduce. GFBE_BAD_INPUT without candidates. */
gfbe_status gfbe_ltab_keep_records(gfbe_ctx *ctx, gfbe_ltab *t, int32_t on);
gfbe_status gfbe_ltab_step(gfbe_ctx *ctx, gfbe_ltab *t, const double *pose7, const double *ex_cam, double sqrt_info, double huber_width,
                           const double *y_p, const double *v_p, const double *rest, const double *radius, gfbe_line_stepped *out);
gfbe_status gfbe_ltab_commit(gfbe_ctx *ctx, gfbe_ltab *t, const uint8_t *accept /*[W]*/);
/* linefeature.size() and getLineFeatureCount() (feature_manager.cpp:1013-1027) of every table. */
gfbe_status gfbe_ltab_size(gfbe_ctx *ctx, gfbe_ltab *t, int32_t *n_lines);
gfbe_status gfbe_ltab_line_count(gfbe_ctx *ctx, gfbe_ltab *t, int32_t *count);
/* Snapshot of table w in list order; obs4 [n][11][4] (rows >= n_obs are zero), line_plucker [n][6]. Any pointer may be NULL. With it
 * the caller builds the gfbe_line_window of gfbe_line_refine and feeds the CPU's optimizationwithLine(). */
gfbe_status gfbe_ltab_download(gfbe_ctx *ctx, gfbe_ltab *t, int32_t w, int32_t *line_id, int32_t *start_frame, int32_t *n_obs,
                               double *obs4, uint8_t *is_triangulation, double *line_plucker);
/* Replaces table w by n lines in the layout of gfbe_ltab_download (what optimizationwithLine()'s setLineOrth and culling left on the
 * host goes back in). n <= line_capacity, 1 <= n_obs, start_frame + n_obs <= GFBE_NFRAMES. */
gfbe_status gfbe_ltab_upload(gfbe_ctx *ctx, gfbe_ltab *t, int32_t w, int32_t n, const int32_t *line_id, const int32_t *start_frame,
                             const int32_t *n_obs, const double *obs4, const uint8_t *is_triangulation, const double *line_plucker);

/* ------------------------------------------------------------------------------------------
 * a4/a5/a7/a9/a10  Factor evaluation on the device, block-CSR output (parity / inspection API).
 * Each evaluates residuals and TANGENT-space Jacobian blocks at the window's current state,
 * exactly what ceres::CostFunction::Evaluate + the manifold lift produce:
 *   ProjectionTwoFrameOneCamFactor::Evaluate  projectionTwoFrameOneCamFactor.cpp:43-151
 *   IMUFactor::Evaluate                       imu_factor.h:28-191
 *   WheelFactor::Evaluate                     wheel_factor.h:28-247
 *   MarginalizationFactor::Evaluate           marginalization_factor.cpp:344-392
 * robustify != 0 additionally applies the loss corrector of ResidualBlockInfo::Evaluate
 * (marginalization_factor.cpp:46-77) to the visual blocks.
 * Output layouts (host, row-major):
 *   vis_r [K][2]; vis_J [K][2][20]  columns = pose_i(6) pose_j(6) ex_cam(6) lambda(1) td(1)
 *   imu_r [n_imu][15]; imu_J [n_imu][15][30]  columns = pose_i(6) sb_i(9) pose_j(6) sb_j(9)
 *   wheel_r [n_wheel][6]; wheel_J [n_wheel][6][22] columns = pose_i(6) pose_j(6) ex_wheel(6) sx sy sw td_wheel
 *   prior_r [n]; prior_J is J0 itself (constant), not returned.
 * Any output pointer may be NULL to skip that factor family.
 * ------------------------------------------------------------------------------------------ */
gfbe_status gfbe_eval_factors(gfbe_ctx *ctx, const gfbe_window *win, int32_t robustify,
                              double *vis_r, double *vis_J,
                              double *imu_r, double *imu_J,
                              double *wheel_r, double *wheel_J,
                              double *prior_r, double *cost);

/* ------------------------------------------------------------------------------------------
 * a6/a8  Pre-integration on the device (the producers of gfbe_imu_preint / gfbe_wheel_preint):
 *   IntegrationBase::push_back/propagate/midPointIntegration   integration_base.h:39-167
 *   WheelIntegrationBase::push_back/propagate/midPointIntegration wheel_integration_base.h:41-178
 * n_interval independent intervals; interval k owns samples [offset[k], offset[k+1]).
 * Sample rows: IMU [dt ax ay az gx gy gz], wheel [dt vx vy vz gx gy gz]. first_* is the
 * (acc_0,gyr_0)/(vel_0,gyr_0) the interval was constructed with. noise: ACC_N GYR_N ACC_W GYR_W
 * (integration_base.h:30-36) / VEL_N_wheel GYR_N_wheel (wheel_integration_base.h:32-36).
 * An empty interval (offset[k] == offset[k+1]) gives the record the reference's constructor leaves: the identity jacobian (wheel:
 * zero), zero covariance, the identity quaternion, sum_dt = 0, and first_* / lin_* passed through.
 * Every argument is checked on the host before anything is copied or launched. GFBE_BAD_INPUT, with a gfbe_last_error text and
 * no output touched: n_interval <= 0; offset[0] < 0 or offset[k+1] < offset[k] for any k; a NULL offset, first_*, lin_*, noise or
 * out (all are required: there is no default linearisation point or noise); a NULL samples unless offset[n_interval] == 0.
 * ------------------------------------------------------------------------------------------ */
gfbe_status gfbe_preintegrate_imu(gfbe_ctx *ctx, int32_t n_interval, const int32_t *offset,
                                  const double *samples, const double *first_acc_gyr /*[n][6]*/,
                                  const double *lin_ba_bg /*[n][6]*/, const double noise[4],
                                  gfbe_imu_preint *out);
gfbe_status gfbe_preintegrate_wheel(gfbe_ctx *ctx, int32_t n_interval, const int32_t *offset,
                                    const double *samples, const double *first_vel_gyr /*[n][6]*/,
                                    const double *lin_sx_sy_sw_td /*[n][4]*/, const double noise[2],
                                    gfbe_wheel_preint *out);

/* ------------------------------------------------------------------------------------------
 * a1/a2/a3/a11/a12  The whole optimization() call.
 *   solve:        ceres::Solve with DENSE_SCHUR + DOGLEG + HuberLoss   estimator.cpp:2956-3379
 *   write-back:   double2vector() yaw/position re-anchoring            estimator.cpp:2501-2630
 *   marginalise:  MARGIN_OLD / MARGIN_SECOND_NEW                       estimator.cpp:3394-3693,
 *                 MarginalizationInfo::{preMarginalize,marginalize,getParameterBlocks}
 *                                                                      marginalization_factor.cpp:119-330
 * out_state / out_feature receive the re-anchored parameter blocks (what a second vector2double()
 * would produce, estimator.cpp:3398).
 * FAILURE CONTRACT (one rule for gfbe_solve_window, gfbe_solve_batch and gfbe_batch_download; INTEGRATION.md and
 * examples/estimator_binding.cpp say the same; tests/test_gpu_branches.py asserts both halves through this entry point):
 *   status <= GFBE_NUMERICAL_FAILURE (GFBE_OK, GFBE_NO_CONVERGENCE, GFBE_NUMERICAL_FAILURE): the solve RAN and every output has been
 *     written — out_state / out_feature / the in-out prior / summary. For GFBE_NUMERICAL_FAILURE they hold what the failed solve left:
 *     the last state its iterations accepted (the uploaded state if none was), re-anchored, and the prior marginalised at that state —
 *     exactly what the reference goes on with, since Estimator::optimization() never looks at Ceres' termination_type
 *     (estimator.cpp:3377-3379). A caller that wants "keep the previous state on failure" tests the status and discards the outputs.
 *   status >= GFBE_BAD_INPUT: the CALL failed (bad argument, no device, device error) — no output has been touched.
 * (SURVEY.md section 8b asked for "outputs untouched on failure"; that holds for failed calls. A numerically failed solve is not a failed
 *  call: leaving its outputs unwritten would make a batch's result depend on which of its windows failed.)
 * prior_out (may be NULL when margin_flag == GFBE_MARGIN_NONE) is IN/OUT like last_marginalization_info: when a marginalisation
 * ran — margin_flag != GFBE_MARGIN_NONE and the window is full (frame_count == GFBE_WINDOW_SIZE, estimator.cpp:3391) — it
 * receives the new prior with block ids already shifted (slot i -> i-1 for MARGIN_OLD; slot 10 -> 9 for SECOND_NEW), `valid`
 * = 0 if the marginalisation produced none (marginalization_factor.cpp:205-210). When NO marginalisation ran (a window that is
 * still filling up) it is left exactly as the caller passed it: pass the previous prior, or a structure whose `valid` the
 * caller has set to 0 — an uninitialised gfbe_prior stays uninitialised.
 * ------------------------------------------------------------------------------------------ */
gfbe_status gfbe_solve_window(gfbe_ctx *ctx, const gfbe_window *win, int32_t margin_flag,
                              gfbe_state *out_state, double *out_feature,
                              gfbe_prior *prior_out, gfbe_summary *summary);

/* Batched form: n independent windows, one launch sequence. Arrays are per-window. The windows do not influence one another:
 * summary[w].status is window w's own outcome, the return value the worst of them (GFBE_NO_CONVERGENCE or
 * GFBE_NUMERICAL_FAILURE: every window's outputs have been written, a failed window's from the last state its iterations
 * accepted; anything larger: the call itself failed and no output is valid). The same holds for gfbe_batch_download. */
gfbe_status gfbe_solve_batch(gfbe_ctx *ctx, int32_t n_window, const gfbe_window *const *win,
                             int32_t margin_flag, gfbe_state *out_state, double *const *out_feature,
                             gfbe_prior *const *prior_out, gfbe_summary *summary);

/* Device-resident form used for throughput measurement: upload once, (re)solve many times.
 *   (Window order: outputs and gfbe_batch_feature_count always use the caller's indices; inside, a batch that is solved in parts
 *   holds its windows sorted by size — a window's result does not depend on its place.)
 *   gfbe_batch_upload   packs the windows into pinned staging memory and ENQUEUES one host-to-device copy plus the
 *                       preparation kernels on the context's private copy stream. It returns when the
 *                       caller's gfbe_window structures have been read — they may be reused at once — but the copy may still
 *                       be in flight: gfbe_batch_solve waits for it on the device (an event), never on the host
 *   gfbe_batch_solve    resets every window to its uploaded state, then runs the full
 *                       optimization() sequence on the ctx stream; asynchronous, no host sync
 *   gfbe_batch_download runs the gather kernel and ONE device-to-host copy on the context's private download stream
 *                       (after the solve's event), waits for that copy only, and unpacks. prior_out: in/out as described
 *                       above (untouched for windows whose marginalisation did not run)
 * ------------------------------------------------------------------------------------------ */
typedef struct gfbe_batch gfbe_batch;
gfbe_status gfbe_batch_upload(gfbe_ctx *ctx, int32_t n_window, const gfbe_window *const *win,
                              gfbe_batch **batch);
gfbe_status gfbe_batch_solve(gfbe_ctx *ctx, gfbe_batch *batch, int32_t margin_flag);
gfbe_status gfbe_batch_download(gfbe_ctx *ctx, gfbe_batch *batch, gfbe_state *out_state,
                                double *const *out_feature, gfbe_prior *const *prior_out,
                                gfbe_summary *summary);
void gfbe_batch_free(gfbe_ctx *ctx, gfbe_batch *batch);

/* Measurement hooks (bench.py): name/launch count/accumulated GPU milliseconds of each kernel
 * family since the last reset, measured with hipEvents on the ctx stream when profiling is on. */
gfbe_status gfbe_profile_enable(gfbe_ctx *ctx, int32_t on);
int32_t gfbe_profile_count(const gfbe_ctx *ctx);
gfbe_status gfbe_profile_get(const gfbe_ctx *ctx, int32_t i, const char **name, int64_t *launches,
                             double *total_ms, double *algorithmic_bytes);
void gfbe_profile_reset(gfbe_ctx *ctx);
/* Where the calling thread spent the LAST gfbe_batch_upload(_tables) and the LAST gfbe_batch_download of this context, milliseconds on the
 * host's clock: out4 = [ upload: scan + packing into pinned memory | upload: the rest of the call (allocation, enqueue of the copy and the
 * expansion kernels) | download: WAITING for the device (the solve, the gather kernel, the copy) | download: unpacking into the caller's
 * structures ]. A pipeline that keeps several batches in flight is host-bound when the first, second and fourth add up to its time per
 * batch, and device-bound when the third is what is left (bench.py's end_to_end block reports both). */
void gfbe_host_times(const gfbe_ctx *ctx, double *out4);

/* Diagnostics: phase time stamps (10 ns ticks) of the dense solve kernel for window w of a batch. */
gfbe_status gfbe_debug_timing(gfbe_ctx *ctx, gfbe_batch *batch, int32_t w, double *out32);
/* Diagnostics: a per-window vector of the LAST linearisation of a solved batch (GFBE_DENSE_DIM doubles each; waits for the solve):
 * which = 0 Gauss-Newton step y of the dense block (Jacobi-scaled), 1 Cauchy direction v, 2 Jacobi scaling s, 3 gradient g.
 * Lets a test compare the two factorisations of gfbe_options.solve_kernel entry by entry. which = 1000 + r: row r of the assembled
 * normal equations H (lower triangle valid); 2000 + r: row r of the Schur term E (73 entries; r = 73: its gradient share eg).
 * Coordinates: H and g are unscaled, constant dims removed. E = sum_l w_l h_l h_l^T and eg = sum_l w_l h_l g_l with the UNSCALED pose
 * columns h_l = H_pl[l] of H and g; only the landmark side is Jacobi-scaled and mu-regularised, through the weight
 * w_l = s_l^2 / (s_l^2 H_ll + mu clamp(s_l^2 H_ll)), s_l = 1 / (1 + sqrt(H_ll)) fixed at iteration 0 (w_l = 0 for a constant landmark
 * and one without factors). The dense solve scales H - E afterwards. tests/test_gpu_normal_equations.py compares all four entry by entry.
 * Dims the batch does not carry — the GNSS dims of a batch without a GNSS window, which no kernel of such a batch reads or writes — are
 * reported like inactive dims: 0.0 in y, v, g and H, 1.0 in s.
 * which = 4: the scalars of the dense solve of that linearisation, out[0..7] = mu of the factorisation that succeeded, G2 = sum gt^2 / D^2,
 * N2 = sum D^2 y^2, gy = sum gt y, v^T Ht v, v^T Ht y, y^T Ht y (Ht = s H s, gt = s g, D^2 the clamped scaled diagonal) and max |g|: the
 * DENSE shares as the solve kernel formed them, before the step kernel adds the landmarks' and before an accepted step changes mu
 * (copies kept in the window's control block for this call; the mu is the factorisation's own, not the trust-region state's). The rest
 * of out is zero. tests/test_gpu_solve_step.py holds y, s, v and these against an extended-precision restatement of the reduced system. */
gfbe_status gfbe_debug_vector(gfbe_ctx *ctx, gfbe_batch *batch, int32_t w, int32_t which, double *out);

/* Multi-GPU landmark sharding: when set, the library calls
 * fn(user, device_ptr, n_doubles, hip_stream) once per linearisation on the packed partial reduced
 * system [S | g | cost ...] (and on a few small exchange blocks per iteration); the callee performs an in-place sum
 * all-reduce (RCCL) on that stream and returns 0, or a non-zero code: the solve that enqueued the call then returns
 * GFBE_DEVICE_ERROR with the code in gfbe_last_error — un-reduced partial sums are never handed back as a result.
 * A hook installed with world_size 1 still runs the sharded launch sequence (every all-reduce is then the identity): that is
 * how a single-GPU box exercises the whole path. fn == NULL switches the sharding off.
 * Limits of the sharded mode: no solver time cap (max_solver_time_in_seconds is refused: the ranks' clocks would stop them at
 * different iterations), no device-resident feature tables, and ONE mu retry per linearisation — a factorisation that fails
 * again at the larger mu ends the window with GFBE_NUMERICAL_FAILURE, where the unsharded solve keeps raising mu up to max_mu. */
typedef int32_t (*gfbe_allreduce_fn)(void *user, void *device_ptr, int64_t n_doubles, void *hip_stream);
gfbe_status gfbe_set_allreduce(gfbe_ctx *ctx, gfbe_allreduce_fn fn, void *user, int32_t rank,
                               int32_t world_size);

#ifdef __cplusplus
}
#endif
#endif /* GFBE_H_ */
