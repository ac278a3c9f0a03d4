/*
 * gfbe_klt.h — the optical-flow tracker in front of the feature tables: image pyramids and pyramidal Lucas-Kanade on the device,
 * the tracking half of FeatureTracker::trackImage for n independent cameras. The symbols live in libgfbe.so; this companion header
 * keeps them apart from the surface of gfbe.h.
 *
 *       FeatureTracker::trackImage, inBorder, distance   vins_estimator/src/featureTracker/feature_tracker.cpp:103-179, :14-28
 *       calc_sharr_deriv                                  mesh/src/meshing/optical_flow/lkpyramid.cpp:56-149
 *       the tracker of one level                          :173-499
 *       opencv_buildOpticalFlowPyramid                    :516-619
 *
 * The window is 21 x 21, the only size the reference passes; images are one channel of uint8.
 *
 * R1 pyramid. Level 0 is the image. Level l + 1 has size ((w + 1) / 2, (h + 1) / 2) (:604); its pixel (x, y) is
 *    (sum of the 5 x 5 taps [1 4 6 4 1] x [1 4 6 4 1] of level l around (2x, 2y), BORDER_REFLECT_101, + 128) >> 8.
 *    cv::pyrDown is called at :580 and its body is not part of the reference tree: the rule is OpenCV's documented kernel, an
 *    assumption of the model. Level l + 1 is built when its width and height are both > 21 (:604-613); the
 *    effective maximum level of a call is the smaller of the last level built and the request. Every level carries a border of 21
 *    pixels: BORDER_REFLECT_101 for the image (:557, :583), zeros for the derivative (:659).
 * R2 derivative (:56-149), int16 pairs (Ix, Iy) per pixel: per column t0 = 3 (above + below) + 10 centre, t1 = below - above;
 *    Ix = t0[x + 1] - t0[x - 1], Iy = 3 (t1[x - 1] + t1[x + 1]) + 10 t1[x]; rows and columns beyond the unpadded level are
 *    reflected without the edge (:76-80, :112-119).
 * R3 one level of one point (:191-498), statement for statement, in single precision unless said otherwise:
 *    prevPt = prevPts * 2^-level; nextPt = nextPts * 2^-level (top level with an initial flow), prevPt (top level without), or
 *    nextPts * 2 (below the top); halfWin = 10; iprevPt = cvFloor(prevPt - halfWin). iprevPt.x < -21 or >= cols (and y likewise):
 *    the level is skipped, at level 0 status = 0 and err = 0. a, b = the fractions; iw00 = cvRound(((1 - a)(1 - b)) 2^14),
 *    iw01 = cvRound((a (1 - b)) 2^14), iw10 = cvRound(((1 - a) b) 2^14), iw11 = 2^14 - iw00 - iw01 - iw10; cvRound rounds half to
 *    even, cvFloor and cvRound saturate at +-2^30. The patch: I = CV_DESCALE(bilinear sum, 9), Ix, Iy = CV_DESCALE(.., 14), int16.
 *    A11, A12, A22 = sums of Ix Ix, Ix Iy, Iy Iy times 2^-20; D = A11 A22 - A12 A12;
 *    minEig = ((A22 + A11) - sqrt((A11 - A22)^2 + (4 A12) A12)) / 882; minEig < min_eig_threshold or D < FLT_EPSILON: the level is
 *    skipped, at level 0 status = 0. Else D = 1 / D, nextPt -= halfWin and up to max_count times: inextPt = cvFloor(nextPt), the same
 *    range test (break, at level 0 status = 0), the weights, b1, b2 = sums of diff Ix, diff Iy times 2^-20 with
 *    diff = CV_DESCALE(J, 9) - I; delta = ((A12 b2 - A22 b1) D, (A12 b1 - A11 b2) D); nextPt += delta; nextPts = nextPt + halfWin;
 *    delta . delta (double) <= epsilon^2: break; from the second iteration |delta.x + prevDelta.x| < 0.01 and the same in y (compared
 *    as double): nextPts -= delta / 2, break (:448-453). At level 0 with status still set: nextPoint = nextPts - halfWin, the range
 *    test (status = 0), the weights, err = (sum |diff|) / (32 * 441) (:458-497).
 * R3a, the one deviation: the reference accumulates (float)(ixval * ixval) and its likes in a float, in an order that depends on the
 *    SIMD path OpenCV was built with. Here the six sums are exact integer sums (each summand < 2^30, 441 of them), converted to float
 *    once, round to nearest even. The result does not depend on the order of summation.
 * R4 the call (cv::calcOpticalFlowPyrLK): status starts at 1 (and err at 0: the reference leaves it unset where no level writes it);
 *    max_count is clamped to 0 .. 100, epsilon to 0 .. 10 and then squared (the vendored copy has the squaring commented out at
 *    :682; the feature tracker calls cv::); levels run from the effective maximum down to 0.
 * R5 tracking (feature_tracker.cpp:113-179) per camera. With a prediction: the 1-level call from predict_pts with
 *    OPTFLOW_USE_INITIAL_FLOW; fewer than prediction_min_success successes: the max_level call without an initial flow, which
 *    overwrites cur_pts (:118-133). Without a prediction: that call. flow_back: the reverse call current -> previous, 1 level, initial
 *    flow = prev_pts (:141). A point is kept when status && reverse_status && distance(prev, reverse) <= flow_back_dist (the
 *    differences in float, the rest in double, :22-28), inBorder holds for cur (cvRound, :14-20) and the grey value of the current
 *    image at the truncated cur is <= grey_max (:159-167; a point inBorder rejected is not read). The kept points stay in ascending
 *    order (reduceVector, :170-173) and their track_cnt is incremented (:178-179).
 *
 * The handle holds, for n_cameras cameras, two image sets (previous, current), each with the padded pyramid and its derivative
 * pyramid, and the current point list (up to point_capacity points a camera).
 *   push_image   the current set becomes the previous one; images [n_cameras][rows][cols] are uploaded and R1, R2 run for every
 *                level. Returns without waiting for the device (the images are copied before it returns). With `equalize: 1` the
 *                CLAHE in front of it is gfbe_eq_push_klt of gfbe_eq.h.
 *   set_points   the points of the CURRENT image as the caller's setMask / goodFeaturesToTrack / addPoints left them: offset
 *                [n_cameras + 1] (offset[0] = 0), pts [n][2], ids [n], track_cnt [n]. They are prev_pts of the next track.
 *   track        R5 for every camera, one host wait. has_prediction [n_cameras] (NULL: none), predict_pts [n][2] in the order of the
 *                held points (NULL: none; rows of cameras without a prediction are not read). Outputs: offset_out [n_cameras + 1],
 *                prev_pts / cur_pts [kept][2], ids / track_cnt [kept] (each with room for the held points), counters [n_cameras][4] =
 *                points in, forward successes, after the reverse check, kept. The survivors (cur_pts, ids, track_cnt) become the held points.
 *   flow         R4 alone on explicit points: direction 0 tracks previous -> current, 1 current -> previous; next_pts [n][2] is the
 *                initial flow when use_initial_flow and always the result; status [n], err [n]. The held points are not touched.
 *   download_level  the padded image [(h + 42)][(w + 42)] and derivative [(h + 42)][(w + 42)][2] of a level of set `which` (0: previous,
 *                1: current) of a camera; dims_out [4] = w, h, w + 42, levels built. image_out / deriv_out may be NULL.
 * Failure contract: GFBE_BAD_INPUT with nothing written for a count above the capacity (or offsets that do not ascend from 0), a
 * non-finite point, track or flow before two images were pushed (download_level: before the set was pushed), rows or cols <= 21, a
 * level that was not built, an options struct of another size or with a field out of range; GFBE_NO_DEVICE without a GPU
 * (gfbe_last_error: "no CPU fallback").
 */
#ifndef GFBE_KLT_H_
#define GFBE_KLT_H_
#include "gfbe.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GFBE_KLT_WIN 21
#define GFBE_KLT_MAX_LEVEL 7
typedef struct gfbe_klt gfbe_klt;
typedef struct gfbe_klt_options {
  int32_t struct_size;             /* sizeof(gfbe_klt_options), written by gfbe_klt_default_options */
  int32_t max_level;               /* 3 (feature_tracker.cpp:132, :135), 0 .. GFBE_KLT_MAX_LEVEL */
  int32_t max_count;               /* 30 (TermCriteria) */
  int32_t flow_back;               /* 1 (FLOW_BACK) */
  int32_t border;                  /* 1 (BORDER_SIZE, :16), >= 0 */
  int32_t grey_max;                /* 250 (:163) */
  int32_t prediction_min_success;  /* 10 (:131) */
  int32_t reserved;
  double epsilon;                  /* 0.01 (TermCriteria) */
  double min_eig_threshold;        /* 1e-4 */
  double flow_back_dist;           /* 0.5 (:146) */
} gfbe_klt_options;
void gfbe_klt_default_options(gfbe_klt_options *opt);
gfbe_status gfbe_klt_create(gfbe_ctx *ctx, int32_t n_cameras, int32_t rows, int32_t cols, int32_t point_capacity,
                            const gfbe_klt_options *opt /* NULL: defaults */, gfbe_klt **out);
void gfbe_klt_destroy(gfbe_ctx *ctx, gfbe_klt *h);
gfbe_status gfbe_klt_push_image(gfbe_ctx *ctx, gfbe_klt *h, const uint8_t *images);
gfbe_status gfbe_klt_set_points(gfbe_ctx *ctx, gfbe_klt *h, const int32_t *offset, const float *pts, const int32_t *ids,
                                const int32_t *track_cnt);
gfbe_status gfbe_klt_track(gfbe_ctx *ctx, gfbe_klt *h, const uint8_t *has_prediction, const float *predict_pts, int32_t *offset_out,
                           float *prev_pts, float *cur_pts, int32_t *ids, int32_t *track_cnt, int32_t *counters);
gfbe_status gfbe_klt_flow(gfbe_ctx *ctx, gfbe_klt *h, int32_t direction, int32_t max_level, int32_t use_initial_flow,
                          const int32_t *offset, const float *pts, float *next_pts, uint8_t *status, float *err);
gfbe_status gfbe_klt_download_level(gfbe_ctx *ctx, gfbe_klt *h, int32_t which, int32_t camera, int32_t level, uint8_t *image_out,
                                    int16_t *deriv_out, int32_t *dims_out);
#ifdef __cplusplus
}
#endif
#endif
