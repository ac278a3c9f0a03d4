/*
 * gfbe_eq.h — image equalisation on the device: contrast-limited adaptive histogram equalisation (CLAHE) of the 8-bit, one-channel
 * images of the n cameras of a handle, in front of the tracker (gfbe_klt.h) and of the keyframe descriptors (gfbe_kfd.h). With
 * `equalize: 1` (config/realsense/m3dgr.yaml) the reference equalises every camera image before the tracker sees it and every keyframe
 * image of the loop node; here that is two kernels in front of the pyramid build or the blur, and no pixel is touched on the host. The
 * symbols live in libgfbe.so; this companion header keeps them apart from the other surfaces.
 *
 *       cv::createCLAHE()->apply(image, image)           vins_estimator/src/rosNodeTest.cpp:271-276
 *       the same on a keyframe's image                   dense_map/src/pose_graph_node.cpp:642-647
 *       cv::createCLAHE(3.0, cv::Size(8, 8))             linefeatureTracker/linefeature_tracker.cpp:56-60
 *
 * The rules E1 .. E6 below are OpenCV's CLAHE as documented and as its clahe.cpp (3.4 / 4.x) is remembered, an ASSUMPTION of the
 * model: nothing of OpenCV was at hand to run. The stage is unpinned against the reference, like the tracker, the detector and the
 * descriptors; it is pinned bit for bit against the model tests/eq_np.py.
 *
 * E1 geometry. If cols % tiles_x == 0 and rows % tiles_y == 0 the tile is (cols / tiles_x, rows / tiles_y) and the histograms read the
 *    image. Otherwise the image is extended at the bottom by tiles_y - rows % tiles_y rows AND at the right by tiles_x - cols % tiles_x
 *    columns with BORDER_REFLECT_101; a dimension that is divisible by itself then gets a whole extra `tiles` of padding (OpenCV's
 *    quirk, kept). The tile is the extended size divided by the tile counts.
 * E2 histogram. Each tile has 256 bins over its area = tw * th pixels of the (extended) image.
 * E3 clip and redistribute, only when clip_limit > 0: limit = max((int)(clip_limit * area / 256), 1), product and quotient in double
 *    (a quotient of area or more counts as area: it clips nothing). clipped is the sum of the excesses over limit; the bins are cut to
 *    limit; every bin gets clipped / 256; with residual = clipped % 256 > 0 and step = max(256 / residual, 1), bin i gets one more iff
 *    i % step == 0 && i / step < residual.
 * E4 LUT. lut[i] = saturate_u8(cvRound((float)sum_i * scale)), sum_i the running sum of the bins up to and including i,
 *    scale = 255.0f / (float)area, cvRound half to even.
 * E5 interpolation in single precision, nothing fused, in the written order: inv_tw = 1.0f / (float)tw; for column x
 *    txf = (float)x * inv_tw - 0.5f, tx1 = floor(txf), xa = txf - (float)tx1, xa1 = 1.0f - xa; then tx1 is clamped to >= 0 and
 *    tx2 = tx1 + 1 to <= tiles_x - 1 (the clamps come after xa is taken); rows likewise. With v the source pixel
 *    res = (L[ty1][tx1][v] * xa1 + L[ty1][tx2][v] * xa) * ya1 + (L[ty2][tx1][v] * xa1 + L[ty2][tx2][v] * xa) * ya and
 *    out = saturate_u8(cvRound(res)), over the original rows x cols.
 * E6 in place. Output may overwrite input: a pixel reads only itself and the LUTs.
 * Not covered: 16-bit images, colour input, the line tracker itself (its CLAHE is this stage with clip_limit 3.0).
 *
 *   create          n_cameras 1 .. 65535 images of rows x cols; opt NULL: the defaults (8 x 8 tiles, clip_limit 40.0, cv::createCLAHE()).
 *   apply           images_in uint8 [n_cameras][rows][cols] equalised into images_out, host to host, one wait; images_out may be
 *                   images_in.
 *   push_klt        gfbe_klt_push_image of the equalised images: the upload goes through the tracker's own pinned mirror, the raw
 *                   images are equalised in place on the device and the same pyramid build follows. Returns without waiting, as
 *                   gfbe_klt_push_image does.
 *   push_kfd        gfbe_kfd_push_image of the equalised images into slot, likewise.
 *   download_lut    for tests and diagnosis: lut_out uint8 [n_cameras][tiles_y][tiles_x][256] of the last apply / push. One wait.
 * gfbe_kfd_capture from a tracker fed by push_klt needs nothing more: in the reference both nodes equalise the same raw image with the
 * same default CLAHE, and the captured level 0 is the equalised image.
 * Failure contract: GFBE_BAD_INPUT with nothing written and no state changed for an options struct of another size, tiles_x or
 * tiles_y outside 1 .. 64, rows <= tiles_y or cols <= tiles_x (the reflection must stay inside the image), rows or cols above 16384,
 * n_cameras outside 1 .. 65535, a clip_limit that is not finite or is negative (0: no clipping), a NULL argument, a handle, tracker or
 * describer of another context, a tracker or describer whose n_cameras, rows or cols are not the handle's, a bad slot, download_lut
 * before any apply or push; GFBE_NO_DEVICE without a GPU (gfbe_last_error: "no CPU fallback").
 */
#ifndef GFBE_EQ_H_
#define GFBE_EQ_H_
#include "gfbe.h"
#include "gfbe_kfd.h"
#include "gfbe_klt.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct gfbe_eq gfbe_eq;
typedef struct gfbe_eq_options {
  int32_t struct_size;             /* sizeof(gfbe_eq_options), written by gfbe_eq_default_options */
  int32_t tiles_x;                 /* 8; tiles a row (tileGridSize.width), 1 .. 64 */
  int32_t tiles_y;                 /* 8; tiles a column (tileGridSize.height), 1 .. 64 */
  int32_t reserved;
  double clip_limit;               /* 40.0 (cv::createCLAHE()); the line front end passes 3.0; 0: no clipping */
} gfbe_eq_options;
void gfbe_eq_default_options(gfbe_eq_options *opt);
gfbe_status gfbe_eq_create(gfbe_ctx *ctx, int32_t n_cameras, int32_t rows, int32_t cols, const gfbe_eq_options *opt /* NULL: defaults */, gfbe_eq **out);
void gfbe_eq_destroy(gfbe_ctx *ctx, gfbe_eq *h);
gfbe_status gfbe_eq_apply(gfbe_ctx *ctx, gfbe_eq *h, const uint8_t *images_in, uint8_t *images_out);
gfbe_status gfbe_eq_push_klt(gfbe_ctx *ctx, gfbe_eq *h, gfbe_klt *tracker, const uint8_t *images);
gfbe_status gfbe_eq_push_kfd(gfbe_ctx *ctx, gfbe_eq *h, gfbe_kfd *kfd, int32_t slot, const uint8_t *images);
gfbe_status gfbe_eq_download_lut(gfbe_ctx *ctx, gfbe_eq *h, uint8_t *lut_out);
#ifdef __cplusplus
}
#endif
#endif
