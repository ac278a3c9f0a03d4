/*
 * gfbe_obs.h — the frame observations on the device, the second half of FeatureTracker::trackImage between the tracker and detector
 * (gfbe_klt.h, gfbe_det.h) and the feature tables (gfbe_ftab_* of gfbe.h): undistortedPts, ptsVelocity, the RGB-D depth lookup and the
 * frame ordered by feature id, for the n cameras of a tracker handle on the points the tracker holds; and the two calls that go back
 * from the estimator to the tracker, removeOutliers and predictPtsInNextFrame / setPrediction. A frame is
 * push_image -> track -> detect -> observe -> add_frame and, after the solve, check_outliers -> remove_outliers -> predict: the point
 * list and the observation list never leave the device. Camera k of the tracker feeds table k of a gfbe_ftab. The symbols live in
 * libgfbe.so; this companion header keeps them apart from the surfaces of gfbe.h, gfbe_klt.h and gfbe_det.h.
 *
 *       the second half of trackImage          vins_estimator/src/featureTracker/feature_tracker.cpp:210-372
 *       undistortedPts, ptsVelocity            :797-808, :810-847
 *       removeOutliers, setPrediction          :1029-1045, :1006-1027
 *       Estimator::predictPtsInNextFrame       vins_estimator/src/estimator/estimator.cpp:3915-3948
 *       PinholeCamera                          camera_models/src/camera_models/PinholeCamera.cc (readParameters :278-295,
 *                                              liftProjective :450-510, spaceToPlane :520-542, distortion :646-662)
 *
 * O1 camera. Each camera has eight doubles fx fy cx cy k1 k2 p1 p2: camodocal's PINHOLE model, the model of nine of the reference's
 *    ten shipped calibrations. inv_K11 = 1.0 / fx, inv_K13 = -cx / fx, inv_K22 = 1.0 / fy, inv_K23 = -cy / fy. no_distortion holds
 *    iff all four of k1, k2, p1, p2 are == 0.0 (:278-295). Out of scope: KANNALA_BRANDT (cam_HILTI22.yaml); its lift runs an Eigen
 *    eigenvalue solve that cannot be stated bit for bit here.
 * O2 distortion d(x, y) (:646-662), double, in the order written, no contraction:
 *    mx2 = x*x; my2 = y*y; mxy = x*y; rho2 = mx2 + my2; rad = k1*rho2 + (k2*rho2)*rho2;
 *    dx = (x*rad + (2.0*p1)*mxy) + p2*(rho2 + 2.0*mx2); dy = (y*rad + (2.0*p2)*mxy) + p1*(rho2 + 2.0*my2).
 * O3 lift (liftProjective :450-510, undistortedPts feature_tracker.cpp:797-808). mx_d = inv_K11 * (double)u + inv_K13;
 *    my_d = inv_K22 * (double)v + inv_K23. With no_distortion the result is (mx_d, my_d). Otherwise eight evaluations of O2:
 *    m_u = m_d - d(m_d), then seven times m_u = m_d - d(m_u). cur_un_pts = ((float)(mx_u / 1.0), (float)(my_u / 1.0)), round to
 *    nearest even.
 * O4 velocity (ptsVelocity :810-847). dt = cur_time - prev_time in double. A point whose id was in the previous call's list of that
 *    camera has vx = (float)((double)(un.x - prev_un.x) / dt), and vy likewise; the difference is taken in float (both operands are
 *    cv::Point2f members). Every other point has velocity 0, and so has every point of the first call of a camera and of the first
 *    call after reset. After the call the previous list is this call's whole list of (id, un), the newly detected points included
 *    (:310).
 * O5 depth (:320-368). With depth_cam == 0 every row has depth -2.4. With depth_cam == 1, depth = (double)(int)D[round(v)][round(u)]
 *    / 1000, D the camera's uint16 depth image of the tracker's size and round C's round of the float promoted to double (half away
 *    from zero; it is not the cvRound of inBorder). Deviation a: a pixel outside the image reads as 0 and is counted (the reference
 *    reads out of bounds; reachable only with the tracker's border == 0). Deviation b: with depth_cam == 1 a call without depth
 *    images is refused (the reference returns an empty frame). The depth_cam block of :214-258 changes no output (its status vector
 *    is all ones) and is not modelled. trackImagebox's YOLO boxes are out of scope: every shipped config has use_yolo: 0.
 * O6 the frame. The row of a point is [(double)un.x, (double)un.y, 1.0, (double)u, (double)v, (double)vx, (double)vy, depth]. Rows are
 *    in ascending feature id, the iteration order of the reference's std::map. Two held points of a camera with the same id are a
 *    refusal: the reference would put both into one map entry, and the tables refuse that. The call reports it in its counters, and
 *    the frame it left cannot be added. (Such a frame's rows keep equal ids in held order; a later lookup in the previous list finds the first of them.)
 * O7 removeOutliers (:1029-1045). The held points of camera k whose id is in the given list are dropped, the others keep their order.
 *    Afterwards the tracker is in the state gfbe_klt_set_points with the surviving lists leaves it in. The previous list of O4 is
 *    not touched.
 * O8 prediction (estimator.cpp:3927-3946, feature_tracker.cpp:1006-1027, spaceToPlane PinholeCamera.cc:520-542). The caller passes
 *    frame_count [W], the window's poses [W][11][12] and tic_ric [W][12] in the layout of gfbe_ftab_triangulate, and the predicted
 *    next pose [W][12] (the 4 x 4 curT * (prevT^-1 * curT) stays with the caller: Eigen's general inverse is not restated). Only the
 *    rows a feature's start frame selects, and frame_count, are read. A feature of table k predicts when estimated_depth > 0, it has
 *    at least 2 observations and start_frame + n_obs - 1 == frame_count. The chain: pts_j = ric * (depth * point0) + tic;
 *    pts_w = R[start] * pts_j + P[start]; pts_local = R_next^T * (pts_w - P_next); pts_cam = ric^T * (pts_local - tic), each 3-vector
 *    product summed as (a0*b0 + a1*b1) + a2*b2 with no contraction; x = X/Z, y = Y/Z; p_d = p_u + d(p_u), or p_u with no_distortion;
 *    u = fx * p_d.x + cx, v likewise; the prediction is ((float)u, (float)v). For every held point of camera k, in held order,
 *    predict_pts[i] is the prediction of the table feature with that id, or the held point itself where there is none. Deviation: a
 *    prediction that is not finite falls back to the held point (the reference never checks Z; gfbe_klt_track refuses non-finite
 *    points). Whether a camera "has a prediction" (frame_count >= 2) is the caller's decision, as in the reference; predict_pts goes
 *    into gfbe_klt_track as it is.
 *
 *   create          borrows the tracker: the handle is destroyed before its tracker. cameras [n_cameras][8] (O1). The tracker's
 *                   point_capacity must be <= GFBE_DET_MAX_POINTS.
 *   reset           forgets the previous lists and the times (and the held frame).
 *   observe         O3 .. O6 for every camera on the tracker's held points; one host wait. cur_time [n_cameras]; depth [n_cameras]
 *                   [rows][cols] uint16 (NULL with depth_cam == 0). offset_out [n_cameras + 1], feature_id [n], obs8 [n][8] with room
 *                   for the held points; counters [n_cameras][4] = points, points found in the previous list, depth reads outside the
 *                   image, duplicate-id flag (0 / 1). The outputs other than counters may be NULL: then nothing but the counters is
 *                   downloaded. The frame stays on the device in the handle until the next observe.
 *   add_frame       gfbe_ftab_add_frame with the frame observe left on the device: the same kernels on the same values, no observation
 *                   crosses the bus, one host wait. frame_count [n_cameras], td [n_cameras]; keyframe, counters [n_cameras][3],
 *                   avg_parallax as gfbe_ftab_add_frame's. Refused when the table count is not n_cameras, no frame is held, the frame
 *                   was already added, or a duplicate flag is set.
 *   remove_outliers O7: offset [n_cameras + 1] (offset[0] = 0, ascending), ids [offset[n_cameras]]. No list comes back; held_out
 *                   [n_cameras] (may be NULL) is the number of points each camera holds afterwards, which sizes predict_pts. One wait:
 *                   the tracker's own counts stay exact.
 *   predict         O8; one host wait. predict_pts [n][2] in the order of the held points, n_predicted [n_cameras].
 *   download_prev   the previous list of a camera, ascending in id: *n_out its length, ids [n], un_pts [n][2] (either may be NULL), for
 *                   tests and diagnosis.
 * Failure contract: GFBE_BAD_INPUT with nothing written and no state changed when no image has been pushed, an options struct has
 * another size or a field out of range (depth_cam outside 0 .. 1, match_tile no power of two in 64 .. 1024), a camera parameter is not
 * finite or fx / fy is 0, a time is not finite or not greater than the camera's previous time, depth is NULL with depth_cam == 1,
 * a handle belongs to another context, the tracker's point_capacity is above GFBE_DET_MAX_POINTS, offsets do not ascend from 0, or a
 * camera or table count does not fit; GFBE_NO_DEVICE without a GPU (gfbe_last_error: "no CPU fallback").
 */
#ifndef GFBE_OBS_H_
#define GFBE_OBS_H_
#include "gfbe_det.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct gfbe_obs gfbe_obs;
typedef struct gfbe_obs_options {
  int32_t struct_size;             /* sizeof(gfbe_obs_options), written by gfbe_obs_default_options */
  int32_t depth_cam;               /* 1 (depth: 1 of the realsense configs): O5 reads the depth images; 0: every depth is -2.4 */
  int32_t match_tile;              /* 256; table ids a workgroup of predict stages at a time, a power of two, 64 .. 1024; changes no result */
  int32_t reserved;
} gfbe_obs_options;
void gfbe_obs_default_options(gfbe_obs_options *opt);
gfbe_status gfbe_obs_create(gfbe_ctx *ctx, gfbe_klt *tracker, const double *cameras, const gfbe_obs_options *opt /* NULL: defaults */, gfbe_obs **out);
void gfbe_obs_destroy(gfbe_ctx *ctx, gfbe_obs *h);
gfbe_status gfbe_obs_reset(gfbe_ctx *ctx, gfbe_obs *h);
gfbe_status gfbe_obs_observe(gfbe_ctx *ctx, gfbe_obs *h, const double *cur_time, const uint16_t *depth, int32_t *offset_out, int32_t *feature_id, double *obs8,
                             int32_t *counters);
gfbe_status gfbe_obs_add_frame(gfbe_ctx *ctx, gfbe_obs *h, gfbe_ftab *ftab, const int32_t *frame_count, const double *td, int32_t *keyframe, int32_t *counters,
                               double *avg_parallax);
gfbe_status gfbe_obs_remove_outliers(gfbe_ctx *ctx, gfbe_obs *h, const int32_t *offset, const int32_t *ids, int32_t *held_out);
gfbe_status gfbe_obs_predict(gfbe_ctx *ctx, gfbe_obs *h, gfbe_ftab *ftab, const int32_t *frame_count, const double *poses, const double *tic_ric,
                             const double *next_pose, float *predict_pts, int32_t *n_predicted);
gfbe_status gfbe_obs_download_prev(gfbe_ctx *ctx, gfbe_obs *h, int32_t camera, int32_t *n_out, int32_t *ids, float *un_pts);
#ifdef __cplusplus
}
#endif
#endif
