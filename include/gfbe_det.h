/*
 * gfbe_det.h — corner detection on the device, the other half of FeatureTracker::trackImage behind the tracker of gfbe_klt.h:
 * setMask, cv::goodFeaturesToTrack and addPoints for the n cameras of a tracker handle, on the images and the held points the
 * tracker already keeps. After it a frame is push_image -> track -> detect and the point list leaves the device only as results.
 * The symbols live in libgfbe.so; this companion header keeps them apart from the surfaces of gfbe.h and gfbe_klt.h.
 *
 *       FeatureTracker::setMask                vins_estimator/src/featureTracker/feature_tracker.cpp:56-83
 *       FeatureTracker::addPoints              :85-93
 *       the detection of trackImage            :178-208 (cv::goodFeaturesToTrack at :198)
 *       the keyframe's corners                 dense_map/src/keyframe.cpp:169 (no mask, 500 corners, distance 10)
 *
 * Images are one channel of uint8, as the tracker holds them. The bodies of cv::goodFeaturesToTrack, cv::cornerMinEigenVal,
 * cv::circle and std::sort are not part of the reference tree: what G1 .. G3 say about them is OpenCV's documented behaviour, an
 * assumption of the model.
 *
 * G1 setMask (:56-83). The held points are ordered by track_cnt, descending; the mask starts at 255. For each point in that order
 *    the pixel is p = (cvRound(x), cvRound(y)), half to even and saturating as inBorder's (gfbe_klt.h R5). If p is inside the image
 *    and mask[p] == 255 the point is kept (its position, id and track_cnt, in this order) and the disc around p is cleared.
 *    Deviation a: std::sort is not stable; here equal counts keep their list order. Deviation b: a point whose pixel is outside
 *    the image is dropped (the reference reads the mask out of bounds). Deviation c: cv::circle's filled circle is taken as the
 *    disc dx^2 + dy^2 <= min_dist^2. The mask is never an image on the product path: "pixel q is clear" is "q lies in no kept
 *    point's disc".
 * G2 the response of a pixel (cv::cornerMinEigenVal, block 3, aperture 3, BORDER_REFLECT_101). Dx, Dy: the 3 x 3 Sobel sums of the
 *    image, integers with |.| <= 1020, the image reflected without its edge. A, B, C: the 3 x 3 sums of Dx^2, Dx Dy, Dy^2, the
 *    planes of products reflected by the same rule; exact integers below 2^24. s2 = (float)((1 / (4 * 3 * 255))^2);
 *    a = 0.5f (A s2), b = B s2, c = 0.5f (C s2); eig = (a + c) - sqrtf((a - c)(a - c) + b b), single precision in the order
 *    written, no contraction, a correctly rounded square root. Deviation: OpenCV scales Dx before it squares and sums in float;
 *    here the sums are exact, as in R3a of gfbe_klt.h.
 * G3 goodFeaturesToTrack. maxVal = the largest eig over the clear pixels of the image; no clear pixel: no corners.
 *    t = (float)((double)maxVal * quality). A pixel (x, y), 1 <= x <= cols - 2, 1 <= y <= rows - 2, is a candidate when it is
 *    clear, eig > t, eig != 0 and eig equals the largest thresholded value (a value <= t counts as 0) of its 3 x 3 neighbours
 *    inside the image. Candidates are taken by descending eig, equal values the larger y * cols + x first. A candidate is accepted
 *    when no corner accepted before it has dx^2 + dy^2 < min_dist^2 (strict); the walk stops at max_corners accepted.
 * G4 (:191-201) max_corners = max_cnt - kept; <= 0: nothing is detected.
 * G5 addPoints (:85-93). The accepted corners are appended in order as ((float)x, (float)y) with ids next_id++ and track_cnt 1.
 * Overflow. A camera with more candidates than candidate_capacity adds nothing and sets its overflow counter; its G1 result
 *    stands. Which candidates a full list would lose depends on timing; the all-or-nothing rule keeps every result free of it.
 *
 *   create       borrows the tracker: the detector is destroyed before its tracker. The tracker's point_capacity must be
 *                <= GFBE_DET_MAX_POINTS.
 *   set_next_id  n_id of :90 per camera (it starts at 0).
 *   detect       G1, G3, G4, G5 for every camera on the current image and the held points; the result becomes the tracker's held
 *                points exactly as gfbe_klt_set_points with the same lists would leave them, and is returned: offset_out
 *                [n_cameras + 1], pts [n][2], ids [n], track_cnt [n] (each with room for max(held, max_cnt) rows a camera),
 *                counters [n_cameras][6] = points in, kept by G1, candidates of G3, points added, next_id afterwards, candidate
 *                overflow (0 / 1). One host wait.
 *   corners      G2 and G3 alone with no mask (keyframe.cpp:169): the corners of every camera in order of acceptance with their
 *                response; offset_out [n_cameras + 1], pts / response with room for n_cameras * max_corners rows. The held points
 *                and next_id are not touched. A camera whose candidates overflow returns none.
 *   download     a camera's response plane and the mask the last detect applied (255 everywhere before the first), for tests and
 *                diagnosis: the product path stores neither. Either pointer may be NULL.
 * Failure contract: GFBE_BAD_INPUT with nothing written when no image has been pushed, an options struct has another size or a
 * field out of range (max_cnt outside 1 .. the tracker's point_capacity, min_dist outside 0 .. 32768, candidate_capacity < 0,
 * sort_chunk no power of two in 64 .. 2048, quality negative or not finite), the tracker's point_capacity is above
 * GFBE_DET_MAX_POINTS, max_corners outside 1 .. GFBE_DET_MAX_POINTS, or a camera outside the handle's; GFBE_NO_DEVICE without a
 * GPU (gfbe_last_error: "no CPU fallback").
 */
#ifndef GFBE_DET_H_
#define GFBE_DET_H_
#include "gfbe_klt.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GFBE_DET_MAX_POINTS 2048
typedef struct gfbe_det gfbe_det;
typedef struct gfbe_det_options {
  int32_t struct_size;             /* sizeof(gfbe_det_options), written by gfbe_det_default_options */
  int32_t max_cnt;                 /* 150 (m3dgr.yaml:100) */
  int32_t min_dist;                /* 30 (m3dgr.yaml:101), >= 0 */
  int32_t candidate_capacity;      /* 0: the worst case (rows - 2)(cols - 2) a camera */
  int32_t sort_chunk;              /* 512; a power of two, 64 .. 2048; changes no result */
  int32_t reserved;
  double quality;                  /* 0.01 (feature_tracker.cpp:198), finite, >= 0 */
} gfbe_det_options;
void gfbe_det_default_options(gfbe_det_options *opt);
gfbe_status gfbe_det_create(gfbe_ctx *ctx, gfbe_klt *tracker, const gfbe_det_options *opt /* NULL: defaults */, gfbe_det **out);
void gfbe_det_destroy(gfbe_ctx *ctx, gfbe_det *h);
gfbe_status gfbe_det_set_next_id(gfbe_ctx *ctx, gfbe_det *h, const int32_t *next_id);
gfbe_status gfbe_det_detect(gfbe_ctx *ctx, gfbe_det *h, int32_t *offset_out, float *pts, int32_t *ids, int32_t *track_cnt, int32_t *counters);
gfbe_status gfbe_det_corners(gfbe_ctx *ctx, gfbe_det *h, int32_t max_corners, double quality, int32_t min_dist, int32_t *offset_out, float *pts,
                             float *response);
gfbe_status gfbe_det_download(gfbe_ctx *ctx, gfbe_det *h, int32_t camera, float *eig_out, uint8_t *mask_out);
#ifdef __cplusplus
}
#endif
#endif
