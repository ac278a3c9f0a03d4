/*
 * gfbe_kfd.h — the keyframe descriptors on the device: FAST corners, the blurred image, BRIEF descriptors and keypoints_norm of a
 * keyframe for the n cameras of a handle, and their hand-over to the loop database (gfbe_ldb_* of gfbe.h) without a host copy. It is
 * the producer of what gfbe_ldb_add_keyframe and gfbe_ldb_match take, between the tracker that holds the images (gfbe_klt.h) and the
 * loop database. A keyframe is capture -> extract -> describe -> add_keyframe, and match when a loop is reported; what crosses the bus
 * is counts and results. The symbols live in libgfbe.so; this companion header keeps them apart from the other surfaces.
 *
 *       KeyFrame::computeWindowBRIEFPoint, computeBRIEFPoint       dense_map/src/keyframe.cpp:148-191
 *       BriefExtractor                                             :628-646
 *       DVision::BRIEF::compute                                    dense_map/src/ThirdParty/DVision/BRIEF.cpp:39-106
 *
 * Images are one channel of uint8, rows x cols, both at least 7. What K1 and K2 say about cv::GaussianBlur and cv::FAST is their
 * documented behaviour, an ASSUMPTION of the model: nothing of OpenCV was at hand to run. The stage is unpinned against the reference,
 * like the tracker and the detector; it is pinned bit for bit against the model tests/kfd_np.py.
 *
 * K1 blur (BRIEF.cpp:44-60): 9 x 9, sigma 2, BORDER_REFLECT_101. The taps are {7, 17, 32, 46, 52, 46, 32, 17, 7} / 256:
 *    exp(-x^2 / 8) normalised and rounded to 8 fractional bits (the plain rounding sums to 256). out = (sum_ij k_i k_j p_ij + 32768)
 *    >> 16 in exact integers; the sum is below 2^24, so the order of the two passes cannot matter. Deviation: this is the 8-bit
 *    fixed-point form; an OpenCV build that filters 8-bit images another way may differ in the last grey level.
 * K2 FAST-9/16 (keyframe.cpp:163-165: threshold t = 20, non-maximum suppression on). The ring is the 16 pixels of the radius-3
 *    Bresenham circle from (0, 3) on. For a pixel v with 3 <= x <= cols - 4 and 3 <= y <= rows - 4, M is the maximum over the 16 arcs
 *    of 9 contiguous ring pixels and both polarities of the minimum over the arc of p_k - v, respectively v - p_k. The pixel is a
 *    corner iff M > t, and its score is M - 1 (t <= score <= 254); every other pixel has score 0, the 3-pixel frame included. A
 *    corner is kept iff its score is strictly greater than the scores of all 8 neighbours: two equal neighbours both lose. Kept
 *    corners are listed in row-major order, y then x ascending, as ((float)x, (float)y) with their score: the order the reference
 *    appends in, which decides the ties of gfbe_ldb_match's rule 6. t is clamped to 0 .. 255. (With t = 0 a corner of M = 1 has score
 *    0 and is neither counted nor kept.)
 * K3 capacity. A camera with more kept corners than keypoint_capacity keeps the first keypoint_capacity in that order and sets its
 *    overflow flag. Order and count come from a scan, nothing depends on timing. Deviation: the reference has no cap.
 * K4 BRIEF (BRIEF.cpp:83-105). For a point (px, py) in float and pair i: x1 = (int)(px + (float)x1[i]), a float addition and a
 *    conversion toward zero, so -0.5 becomes 0 and is inside, as in the reference; y1, x2, y2 likewise. Bit i is 1 iff all four are
 *    inside the image and blur[y1][x1] < blur[y2][x2]. Bit i is bit i % 64 of word i / 64, the block order gfbe_ldb takes.
 *    Deviation: a point with a non-finite coordinate or |coordinate| >= 2^20 gets an all-zero descriptor and is counted; the
 *    reference's cast is undefined there.
 * K5 keypoints_norm (keyframe.cpp:178-185): the lift of gfbe_obs.h's O3 on the keypoint's pixel in double, PINHOLE camera
 *    [fx fy cx cy k1 k2 p1 p2], then ((float)(X / Z), (float)(Y / Z)) with Z = 1.0; no contraction.
 * K6 the image of a keyframe. A keyframe is the frame at WINDOW_SIZE - 2 (visualization.cpp:1155-1197, pose_graph_node.cpp:519-526),
 *    two pushes behind the tracker's current image: the handle owns a ring of ring_slots image sets. A slot is filled by a device copy
 *    of a tracker's current level-0 images (capture) or by a host upload (push_image); filling writes the slot's image and its blurred
 *    image whole, and voids the slot's score plane until the next extract of that slot.
 * Not covered: colour input, the 80 x 60 thumbnail, the dead goodFeaturesToTrack branch of :166-176 (gfbe_det_corners has it), camera
 * models other than PINHOLE. PnPRANSAC / findConnection are gfbe_pnp_* of gfbe_pnp.h (gfbe_pnp_find_connection_kfd on this handle).
 *
 *   create          pattern int32 [4][256] = x1, y1, x2, y2 of the pairs (the caller's brief_pattern.yml), every offset in -64 .. 64;
 *                   cameras double [n_cameras][8].
 *   push_image      images uint8 [n_cameras][rows][cols] into slot; does not wait beyond the pinned mirror's previous copy. With
 *                   `equalize: 1` the CLAHE in front of it is gfbe_eq_push_kfd of gfbe_eq.h.
 *   capture         the tracker's current level-0 images into slot, device to device; no wait. The tracker's n_cameras, rows and cols
 *                   must match and an image must have been pushed.
 *   extract         K2, K3, K5 and K4 on the kept corners of slot, for every camera; one host wait, for the counters, and a second one
 *                   only when a list is asked for (its size is not known before the first). Outputs (any may be NULL):
 *                   offset_out [n_cameras + 1], pts [n][2], score [n], pts_norm [n][2], desc [n][4] with n = the listed corners of all
 *                   cameras (room for n_cameras * keypoint_capacity is always enough), counters [n_cameras][4] = corners before
 *                   suppression, kept, listed, overflow flag. The lists stay on the handle until the next extract.
 *   describe        K4 on caller-supplied window points (point_2d_uv of computeWindowBRIEFPoint) with the slot's blurred image:
 *                   offset [n_cameras + 1] (from 0, ascending, at most window_capacity a camera), pts_uv [n][2]; desc_out [n][4] and
 *                   counters [n_cameras][2] = points, points of K4's deviation (either may be NULL). The window descriptors stay on
 *                   the handle until the next describe. One wait.
 *   add_keyframe    gfbe_ldb_add_keyframe on camera's lists of the last extract: same results, same refusals (rule 5 included), same
 *                   wait behaviour; no list crosses the bus.
 *   match           gfbe_ldb_match's rule 6 with camera's window descriptors of the last describe; outputs as gfbe_ldb_match's.
 *   download        for tests and diagnosis: blurred_out / score_out [rows][cols] uint8 of a camera of slot (either may be NULL);
 *                   score_out is the plane after K2's suppression, zero where nothing is kept, and needs an extract of the slot
 *                   since it was filled.
 * Failure contract: GFBE_BAD_INPUT with nothing written and no state changed for an options struct of another size or a field out of
 * range, a bad slot or camera, a slot never filled, add_keyframe / match before an extract / describe of that handle, a mismatching
 * tracker, a handle of another context, pattern offsets out of range, a camera parameter that is not finite or fx / fy of 0, an image
 * below 7 x 7 (or above 16384), offsets that do not ascend from 0 or exceed window_capacity, a NULL required argument;
 * GFBE_NO_DEVICE without a GPU (gfbe_last_error: "no CPU fallback").
 */
#ifndef GFBE_KFD_H_
#define GFBE_KFD_H_
#include "gfbe.h"
#include "gfbe_klt.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct gfbe_kfd gfbe_kfd;
typedef struct gfbe_kfd_options {
  int32_t struct_size;             /* sizeof(gfbe_kfd_options), written by gfbe_kfd_default_options */
  int32_t ring_slots;              /* 3; image sets the handle holds (K6), 1 .. 8 */
  int32_t fast_threshold;          /* 20 (keyframe.cpp:163), 0 .. 255 */
  int32_t keypoint_capacity;       /* 4096; listed corners a camera (K3), 1 .. GFBE_LDB_MAX_KEYFRAME_DESCRIPTORS */
  int32_t window_capacity;         /* 2048; window points a camera of describe, 1 .. 2^20 */
  int32_t reserved;
} gfbe_kfd_options;
void gfbe_kfd_default_options(gfbe_kfd_options *opt);
gfbe_status gfbe_kfd_create(gfbe_ctx *ctx, int32_t n_cameras, int32_t rows, int32_t cols, const int32_t *pattern, const double *cameras,
                            const gfbe_kfd_options *opt /* NULL: defaults */, gfbe_kfd **out);
void gfbe_kfd_destroy(gfbe_ctx *ctx, gfbe_kfd *h);
gfbe_status gfbe_kfd_push_image(gfbe_ctx *ctx, gfbe_kfd *h, int32_t slot, const uint8_t *images);
gfbe_status gfbe_kfd_capture(gfbe_ctx *ctx, gfbe_kfd *h, gfbe_klt *tracker, int32_t slot);
gfbe_status gfbe_kfd_extract(gfbe_ctx *ctx, gfbe_kfd *h, int32_t slot, int32_t *offset_out, float *pts, int32_t *score, float *pts_norm, uint64_t *desc,
                             int32_t *counters);
gfbe_status gfbe_kfd_describe(gfbe_ctx *ctx, gfbe_kfd *h, int32_t slot, const int32_t *offset, const float *pts_uv, uint64_t *desc_out, int32_t *counters);
gfbe_status gfbe_kfd_add_keyframe(gfbe_ctx *ctx, gfbe_kfd *h, int32_t camera, gfbe_ldb *db, int32_t detect_loop, int32_t *index_out, int32_t *loop_index,
                                  int32_t *n_results, int32_t *result_id, double *result_score);
gfbe_status gfbe_kfd_match(gfbe_ctx *ctx, gfbe_kfd *h, int32_t camera, gfbe_ldb *db, int32_t old_index, uint8_t *status, int32_t *best_index, int32_t *best_dist,
                           int32_t *n_matched, int32_t *matched_src, float *matched_pt, float *matched_pt_norm);
gfbe_status gfbe_kfd_download(gfbe_ctx *ctx, gfbe_kfd *h, int32_t slot, int32_t camera, uint8_t *blurred_out, uint8_t *score_out);
#ifdef __cplusplus
}
#endif
#endif
