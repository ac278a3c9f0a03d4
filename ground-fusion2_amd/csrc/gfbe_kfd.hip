// gfbe_kfd.hip — the keyframe descriptors of the loop-closure thread on the device: the blurred image, FAST corners with their
// suppression, the ordered keypoint lists, BRIEF descriptors and keypoints_norm for n cameras, and the hand-over of a camera's lists to
// the loop database (gfbe_ldb.hip).
//
//   cv::GaussianBlur of BRIEF::compute                 dense_map/src/ThirdParty/DVision/BRIEF.cpp:44-60     k_kfd_blur
//   cv::FAST(image, keypoints, 20, true)               dense_map/src/keyframe.cpp:163-165                   k_kfd_fast, k_kfd_list
//   BRIEF::compute's pairs, keypoints_norm             BRIEF.cpp:83-105, keyframe.cpp:178-185               k_kfd_brief
//
// The rules are in gfbe_kfd.h and include/gfbe_kfd.h; every per-pixel and per-point statement is the header's function, compiled here for
// the device. k_kfd_blur: a 64 x 32 tile a workgroup, the horizontal sums of its 40 rows in LDS as uint16, the vertical pass from there.
// k_kfd_fast: a 64 x 16 tile a workgroup; the tile with a halo of 4 in LDS, the scores of the tile with a halo of 1 in LDS, the
// suppression from there; a wave owns a row of the tile, so one ballot is the row's count (an integer atomic per row and tile).
// k_kfd_list: one workgroup per camera scans the row counts (block_exclusive_scan), then each wave compacts whole rows in x order with
// ballots: order and count come from the scan. k_kfd_brief: one wave per point, lane l owns pairs l, l + 64, l + 128, l + 192, four
// ballots are the four words; the packed pattern sits in LDS; one lane lifts the point (K5). None of it is arithmetic-bound: what counts
// is that no plane and no list crosses the bus. Integer atomics only, no scratch, workgroups communicate across kernel boundaries only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gfbe_kfd.h"
#include "gfbe_device.h"
#include "gfbe_klt_priv.h"
#include "gfbe_kfd.h"
#include "gfbe_handle.h"

using namespace gfd;

static_assert(KFD_PAIRS == 256, "four words of 64 bits, the descriptor of gfbe_ldb");
static_assert(sizeof(gfbe_kfd_options) == 24, "the layout of include/gfbe_kfd.h");

struct gfbe_kfd : gfbe_handle {
  gfbe_kfd_options opt;
  int n_cam = 0, rows = 0, cols = 0, cap = 0, wcap = 0, threshold = 0;
  uint32_t *pairs = nullptr;                   // [256] the packed pattern
  ObsCam *cams = nullptr;                      // [n_cam]
  // the ring (K6): slot s at s * n_cam * rows * cols
  uint8_t *img = nullptr, *blur = nullptr, *plane = nullptr;
  bool filled[8] = {}, scored[8] = {};
  uint8_t *raw_h = nullptr;                    // the pinned mirror of a push
  hipEvent_t ev_raw = nullptr;
  bool raw_busy = false;
  // an extract's scratch and what it leaves: camera k's lists at rows k * cap
  int *rowcnt = nullptr;                       // [n_cam][rows]
  int *cnt_d = nullptr, *cnt_h = nullptr;      // [n_cam][4] and its pinned mirror
  float *l_pts = nullptr, *l_ptsn = nullptr;   // [n_cam * cap][2]
  int *l_score = nullptr;
  uint64_t *l_desc = nullptr;                  // [n_cam * cap][4]
  bool extracted = false;
  std::vector<int> listed;                     // [n_cam] exact host mirror
  // what a describe leaves: the window descriptors packed over the cameras
  uint64_t *w_desc = nullptr;                  // [n_cam * wcap][4]
  bool described = false;
  std::vector<int> w_off;                      // [n_cam + 1]
  size_t plane_bytes() const { return (size_t)n_cam * (size_t)rows * (size_t)cols; }
};

namespace {
constexpr int KFD_THREADS = 256, KFD_BW = 64, KFD_BH = 32, KFD_FW = 64, KFD_FH = 16;

// the tracker's level 0 without its border -> a slot
__global__ __launch_bounds__(KFD_THREADS) void k_kfd_copy(KltGeom g, const uint8_t *src, int rows, int cols, uint8_t *dst) {
  const int cam = blockIdx.z, y = blockIdx.y, x = blockIdx.x * KFD_THREADS + threadIdx.x;
  if (x >= cols) return;
  const size_t st = (size_t)(g.w[0] + 2 * KLT_WIN);
  dst[((size_t)cam * (size_t)rows + (size_t)y) * (size_t)cols + (size_t)x] =
      src[(size_t)cam * (size_t)g.img_cam + (size_t)g.img_off[0] + (size_t)(y + KLT_WIN) * st + (size_t)(x + KLT_WIN)];
}

// ---- K1 -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KFD_THREADS) void k_kfd_blur(const uint8_t *img, int rows, int cols, uint8_t *out) {
  __shared__ uint16_t s_h[KFD_BH + 2 * KFD_BLUR_R][KFD_BW];
  const int cam = blockIdx.z, x0 = blockIdx.x * KFD_BW, y0 = blockIdx.y * KFD_BH, t = threadIdx.x;
  const uint8_t *src = img + (size_t)cam * (size_t)rows * (size_t)cols;
  for (int e = t; e < (KFD_BH + 2 * KFD_BLUR_R) * KFD_BW; e += KFD_THREADS) {
    const int ry = e / KFD_BW, x = x0 + e % KFD_BW, yy = y0 + ry - KFD_BLUR_R;
    if (x < cols && yy < rows + KFD_BLUR_R)      // (the rows a pixel of the image reads: -4 .. rows + 3)
      s_h[ry][e % KFD_BW] = (uint16_t)kfd_blur_row(src + (size_t)klt_reflect101(yy, rows) * (size_t)cols, cols, x);
  }
  __syncthreads();
  const int lx = t % KFD_BW, x = x0 + lx;
  for (int ly = t / KFD_BW; ly < KFD_BH; ly += KFD_THREADS / KFD_BW) {
    const int y = y0 + ly;
    if (x >= cols || y >= rows) continue;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 9; k++) s += kfd_tap(k) * (int)s_h[ly + k][lx];
    out[((size_t)cam * (size_t)rows + (size_t)y) * (size_t)cols + (size_t)x] = (uint8_t)kfd_blur_round(s);
  }
}

// ---- K2: the scores and the suppression ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KFD_THREADS) void k_kfd_fast(const uint8_t *img, int rows, int cols, int threshold, uint8_t *plane, int *rowcnt, int *counters) {
  constexpr int IW = KFD_FW + 8, IH = KFD_FH + 8, SW = KFD_FW + 2, SH = KFD_FH + 2;
  __shared__ uint8_t s_img[IH][IW];      // pixel (x0 - 4 + i, y0 - 4 + j) at [j][i]; outside the image 0 (never a ring pixel of a scored one)
  __shared__ uint8_t s_sc[SH][SW];       // the score of pixel (x0 - 1 + i, y0 - 1 + j)
  const int cam = blockIdx.z, x0 = blockIdx.x * KFD_FW, y0 = blockIdx.y * KFD_FH, t = threadIdx.x;
  const uint8_t *src = img + (size_t)cam * (size_t)rows * (size_t)cols;
  for (int e = t; e < IW * IH; e += KFD_THREADS) {
    const int i = e % IW, j = e / IW, x = x0 - 4 + i, y = y0 - 4 + j;
    s_img[j][i] = x >= 0 && y >= 0 && x < cols && y < rows ? src[(size_t)y * (size_t)cols + (size_t)x] : (uint8_t)0;
  }
  __syncthreads();
  for (int e = t; e < SW * SH; e += KFD_THREADS) {
    const int i = e % SW, j = e / SW, x = x0 - 1 + i, y = y0 - 1 + j;
    s_sc[j][i] = (uint8_t)(kfd_fast_inside(rows, cols, x, y) ? kfd_fast_score_at(&s_img[j + 3][i + 3], IW, threshold) : 0);
  }
  __syncthreads();
  const int lane = t & 63, x = x0 + lane;
  int before = 0;
  for (int ly = t >> 6; ly < KFD_FH; ly += KFD_THREADS / 64) {      // (wave-uniform: a wave owns row ly of the tile)
    const int y = y0 + ly;
    if (y >= rows) break;
    const int s = s_sc[ly + 1][lane + 1];
    const int nb[8] = {s_sc[ly][lane], s_sc[ly][lane + 1], s_sc[ly][lane + 2], s_sc[ly + 1][lane], s_sc[ly + 1][lane + 2], s_sc[ly + 2][lane], s_sc[ly + 2][lane + 1], s_sc[ly + 2][lane + 2]};
    const bool live = x < cols, keep = live && kfd_nms_keep(s, nb);
    if (live) plane[((size_t)cam * (size_t)rows + (size_t)y) * (size_t)cols + (size_t)x] = keep ? (uint8_t)s : (uint8_t)0;
    const int kept = __popcll(__ballot(keep));
    before += __popcll(__ballot(live && s > 0));
    if (lane == 0 && kept) atomicAdd(&rowcnt[(size_t)cam * (size_t)rows + (size_t)y], kept);
  }
  if (lane == 0 && before) atomicAdd(&counters[4 * (size_t)cam], before);
}

// ---- K2's order and K3 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KFD_THREADS) void k_kfd_list(int rows, int cols, int cap, const uint8_t *plane, int *rowcnt, float *pts, int *score, int *counters) {
  __shared__ int lds[20];
  const int cam = blockIdx.x, t = threadIdx.x, lane = t & 63;
  int *rc = rowcnt + (size_t)cam * (size_t)rows;
  const int chunk = (rows + KFD_THREADS - 1) / KFD_THREADS, b0 = min(rows, t * chunk), b1 = min(rows, b0 + chunk);
  int mine = 0, total;
  for (int y = b0; y < b1; y++) mine += rc[y];
  int base = block_exclusive_scan<KFD_THREADS>(mine, &total, lds);
  for (int y = b0; y < b1; y++) { const int n = rc[y]; rc[y] = base; base += n; }      // a row's count becomes the corners before it
  __threadfence_block();
  __syncthreads();
  const uint8_t *pl = plane + (size_t)cam * (size_t)rows * (size_t)cols;
  const size_t list = (size_t)cam * (size_t)cap;
  for (int y = t >> 6; y < rows; y += KFD_THREADS / 64) {      // (wave-uniform)
    int b = rc[y];
    const int e = y + 1 < rows ? rc[y + 1] : total;
    if (e == b || b >= cap) continue;
    for (int c0 = 0; c0 < cols; c0 += 64) {
      const int x = c0 + lane, s = x < cols ? pl[(size_t)y * (size_t)cols + (size_t)x] : 0;
      const unsigned long long m = __ballot(s > 0);
      const int dst = b + __popcll(m & ((1ull << lane) - 1ull));
      if (s > 0 && dst < cap) { pts[2 * (list + dst)] = (float)x; pts[2 * (list + dst) + 1] = (float)y; score[list + dst] = s; }
      b += __popcll(m);
    }
  }
  if (t == 0) { int *cn = counters + 4 * (size_t)cam; cn[1] = total; cn[2] = min(total, cap); cn[3] = total > cap ? 1 : 0; }
}

// ---- K4, K5 -----------------------------------------------------------------------------------------------------------------------------
struct KfdBriefArgs {
  const uint8_t *blur;                         // the slot's blurred planes
  const uint32_t *pairs;
  const ObsCam *cams;
  const float *pts;
  const int *off;                              // [n_cam + 1] the packed rows of the points; nullptr: camera k at k * cap, counters[k][2] of them
  const int *counters;
  int cap, rows, cols;
  uint64_t *desc;
  float *ptsn;                                 // nullptr: no K5
  int *bad;                                    // [n_cam] points of K4's deviation, zero before the launch; nullptr: not counted
};
__global__ __launch_bounds__(KFD_THREADS) void k_kfd_brief(KfdBriefArgs A) {
  __shared__ uint32_t s_pair[KFD_PAIRS];
  const int cam = blockIdx.y, t = threadIdx.x, lane = t & 63, j = blockIdx.x * (KFD_THREADS / 64) + (t >> 6);
  s_pair[t] = A.pairs[t];
  __syncthreads();
  const size_t begin = A.off ? (size_t)A.off[cam] : (size_t)cam * (size_t)A.cap;
  const int n = A.off ? A.off[cam + 1] - A.off[cam] : min(A.counters[4 * (size_t)cam + 2], A.cap);
  if (j >= n) return;      // (wave-uniform)
  const size_t p = begin + (size_t)j;
  const float px = A.pts[2 * p], py = A.pts[2 * p + 1];
  const bool ok = kfd_point_ok(px, py);
  const uint8_t *pl = A.blur + (size_t)cam * (size_t)A.rows * (size_t)A.cols;
  unsigned long long w[4];
#pragma unroll
  for (int q = 0; q < 4; q++) w[q] = __ballot(ok && kfd_brief_bit(pl, A.rows, A.cols, px, py, s_pair[lane + 64 * q]));
  if (lane == 0) {
    for (int q = 0; q < 4; q++) A.desc[4 * p + q] = w[q];
    if (!ok && A.bad) atomicAdd(&A.bad[cam], 1);
  }
  if (lane == 1 && A.ptsn) obs_lift(A.cams[cam], px, py, &A.ptsn[2 * p], &A.ptsn[2 * p + 1]);
}

const char *kfd_options_error(const gfbe_kfd_options *o) {
  if (o->struct_size != (int32_t)sizeof(gfbe_kfd_options)) return "gfbe_kfd_options.struct_size does not match this library (ABI mismatch)";
  if (o->ring_slots < 1 || o->ring_slots > 8) return "ring_slots outside 1 .. 8";
  if (o->fast_threshold < 0 || o->fast_threshold > 255) return "fast_threshold outside 0 .. 255";
  if (o->keypoint_capacity < 1 || o->keypoint_capacity > GFBE_LDB_MAX_KEYFRAME_DESCRIPTORS) return "keypoint_capacity outside 1 .. GFBE_LDB_MAX_KEYFRAME_DESCRIPTORS";
  if (o->window_capacity < 1 || o->window_capacity > (1 << 20)) return "window_capacity outside 1 .. 2^20";
  return nullptr;
}
gfbe_status kfd_slot(gfbe_ctx *c, const gfbe_kfd *m, const char *who, int slot, bool must_be_filled) {
  if (slot < 0 || slot >= m->opt.ring_slots) return handle_bad(c, who, "slot outside the handle's ring");
  if (must_be_filled && !m->filled[slot]) return handle_bad(c, who, "the slot was never filled");
  return GFBE_OK;
}
int kfd_grid(long long n, int per) { return (int)((n + per - 1) / per); }
// behind a fill: the slot's blurred image, whole
void kfd_launch_blur(gfbe_ctx *c, gfbe_kfd *m, int slot) {
  const size_t o = (size_t)slot * m->plane_bytes();
  hipLaunchKernelGGL(k_kfd_blur, dim3(kfd_grid(m->cols, KFD_BW), kfd_grid(m->rows, KFD_BH), m->n_cam), dim3(KFD_THREADS), 0, ctx_stream(c), (const uint8_t *)m->img + o, m->rows,
                     m->cols, m->blur + o);
  m->filled[slot] = true; m->scored[slot] = false;
}

}  // namespace

// ---- what gfbe_pnp.hip (include/gfbe_pnp.h) sees of a describer (gfbe_handle.h)
namespace gfd {
gfbe_status kfd_window_desc(gfbe_ctx *c, gfbe_kfd *m, const char *who, int camera, int *n, const uint64_t **desc) {
  gfbe_status rc = handle_ready(c, m, who, "describer");
  if (rc != GFBE_OK) return rc;
  if (camera < 0 || camera >= m->n_cam) return handle_bad(c, who, "camera outside the describer's");
  if (!m->described) return handle_bad(c, who, "no window descriptors are held: describe first");
  const int b = m->w_off[(size_t)camera];
  *n = m->w_off[(size_t)camera + 1] - b;
  *desc = m->w_desc + 4 * (size_t)b;
  return GFBE_OK;
}

// ---- gfbe_kfd_push_image in its parts, for gfbe_eq.hip (include/gfbe_eq.h) as well: it equalises the slot's images before the blur
gfbe_status kfd_push_check(gfbe_ctx *c, gfbe_kfd *m, const char *who, int slot, int n_cam, int rows, int cols) {
  gfbe_status rc = handle_ready(c, m, who, "describer");
  if (rc != GFBE_OK) return rc;
  if ((rc = kfd_slot(c, m, who, slot, false)) != GFBE_OK) return rc;
  if (m->n_cam != n_cam || m->rows != rows || m->cols != cols) return handle_bad(c, who, "the describer's n_cameras, rows or cols are not the handle's");
  return GFBE_OK;
}
gfbe_status kfd_push_upload(gfbe_ctx *c, gfbe_kfd *m, int slot, const uint8_t *images, uint8_t **img_d) {
  hipStream_t st = ctx_stream(c);
  const size_t P = m->plane_bytes();
  if (m->raw_busy) GFBE_CHECK(c, hipEventSynchronize(m->ev_raw));      // (the mirror's last copy has left it)
  std::memcpy(m->raw_h, images, P);
  GFBE_CHECK(c, hipMemcpyAsync(m->img + (size_t)slot * P, m->raw_h, P, hipMemcpyHostToDevice, st));
  GFBE_CHECK(c, hipEventRecord(m->ev_raw, st));
  m->raw_busy = true;
  if (img_d) *img_d = m->img + (size_t)slot * P;
  return GFBE_OK;
}
gfbe_status kfd_push_enqueue(gfbe_ctx *c, gfbe_kfd *m, int slot) {
  kfd_launch_blur(c, m, slot);
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}
}  // namespace gfd

extern "C" {

void gfbe_kfd_default_options(gfbe_kfd_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = (int32_t)sizeof *o;
  o->ring_slots = 3; o->fast_threshold = 20; o->keypoint_capacity = 4096; o->window_capacity = 2048;
}

void gfbe_kfd_destroy(gfbe_ctx *c, gfbe_kfd *m) {
  if (!m) return;
  m->release(c);
  delete m;
}

gfbe_status gfbe_kfd_create(gfbe_ctx *c, int32_t n_cameras, int32_t rows, int32_t cols, const int32_t *pattern, const double *cameras, const gfbe_kfd_options *opt,
                            gfbe_kfd **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  gfbe_kfd_options o;
  if (opt) o = *opt; else gfbe_kfd_default_options(&o);
  if (const char *bad = kfd_options_error(&o)) return handle_bad(c, "gfbe_kfd_create", bad);
  if (n_cameras < 1 || n_cameras > 65535) return handle_bad(c, "gfbe_kfd_create", "n_cameras outside 1 .. 65535 (a camera is a grid row)");
  if (rows < KFD_MIN_SIZE || cols < KFD_MIN_SIZE || rows > (1 << 14) || cols > (1 << 14)) return handle_bad(c, "gfbe_kfd_create", "rows / cols outside 7 .. 16384 (the FAST ring is 7 x 7)");
  if (!pattern || !cameras) return handle_bad(c, "gfbe_kfd_create", "pattern or cameras NULL");
  if (!kfd_pattern_ok(pattern)) return handle_bad(c, "gfbe_kfd_create", "a pattern offset outside -64 .. 64");
  const size_t C = (size_t)n_cameras;
  std::vector<ObsCam> cams(C);
  for (size_t q = 0; q < C; q++) {
    if (!obs_camera_ok(cameras + 8 * q)) return handle_bad(c, "gfbe_kfd_create", "a camera parameter is not finite, or fx / fy is 0");
    cams[q] = obs_camera(cameras + 8 * q);
  }
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_kfd_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  uint32_t pairs[KFD_PAIRS];
  kfd_pack_pattern(pattern, pairs);
  gfbe_kfd *m = new gfbe_kfd();
  CreateGuard<gfbe_kfd> guard{c, m, gfbe_kfd_destroy};
  m->owner = c; m->opt = o; m->n_cam = n_cameras; m->rows = rows; m->cols = cols; m->cap = o.keypoint_capacity; m->wcap = o.window_capacity;
  m->threshold = kfd_clamp_threshold(o.fast_threshold);
  m->listed.assign(C, 0); m->w_off.assign(C + 1, 0);
  const size_t P = m->plane_bytes(), S = (size_t)o.ring_slots, N = C * (size_t)m->cap;
  bool ok = m->alloc(&m->pairs, (size_t)KFD_PAIRS) && m->alloc(&m->cams, C) && m->alloc(&m->img, S * P) && m->alloc(&m->blur, S * P) && m->alloc(&m->plane, S * P) &&
            m->alloc_pinned(&m->raw_h, P) && m->create(&m->ev_raw) && m->alloc(&m->rowcnt, C * (size_t)rows) && m->alloc(&m->cnt_d, 4 * C) && m->alloc_pinned(&m->cnt_h, 4 * C) &&
            m->alloc(&m->l_pts, 2 * N) && m->alloc(&m->l_ptsn, 2 * N) && m->alloc(&m->l_score, N) && m->alloc(&m->l_desc, 4 * N) && m->alloc(&m->w_desc, 4 * C * (size_t)m->wcap);
  if (!ok) { ctx_set_error(c, "gfbe_kfd_create: device allocation failed"); return GFBE_DEVICE_ERROR; }
  if (!m->make_staging(c, "gfbe_kfd_create", 1 << 16, false)) return GFBE_DEVICE_ERROR;
  hipStream_t st = ctx_stream(c);
  GFBE_CHECK(c, hipMemcpyAsync(m->pairs, pairs, sizeof pairs, hipMemcpyHostToDevice, st));
  GFBE_CHECK(c, hipMemcpyAsync(m->cams, cams.data(), sizeof(ObsCam) * C, hipMemcpyHostToDevice, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));      // (pairs and cams leave scope)
  guard.armed = false;
  *out = m;
  return GFBE_OK;
}

gfbe_status gfbe_kfd_push_image(gfbe_ctx *c, gfbe_kfd *m, int32_t slot, const uint8_t *images) {
  gfbe_status rc = handle_ready(c, m, "gfbe_kfd_push_image");
  if (rc != GFBE_OK) return rc;
  if ((rc = kfd_slot(c, m, "gfbe_kfd_push_image", slot, false)) != GFBE_OK) return rc;
  if (!images) return handle_bad(c, "gfbe_kfd_push_image", "images NULL");
  if ((rc = kfd_push_upload(c, m, slot, images, nullptr)) != GFBE_OK) return rc;
  return kfd_push_enqueue(c, m, slot);
}

gfbe_status gfbe_kfd_capture(gfbe_ctx *c, gfbe_kfd *m, gfbe_klt *k, int32_t slot) {
  gfbe_status rc = handle_ready(c, m, "gfbe_kfd_capture");
  if (rc != GFBE_OK) return rc;
  if ((rc = kfd_slot(c, m, "gfbe_kfd_capture", slot, false)) != GFBE_OK) return rc;
  if (!k) return handle_bad(c, "gfbe_kfd_capture", "tracker NULL");
  if (k->owner != c) return handle_bad(c, "gfbe_kfd_capture", "the tracker belongs to another context");
  if (k->n_cam != m->n_cam || k->rows != m->rows || k->cols != m->cols) return handle_bad(c, "gfbe_kfd_capture", "the tracker's n_cameras, rows or cols are not the handle's");
  if (k->n_pushed < 1) return handle_bad(c, "gfbe_kfd_capture", "no image has been pushed");
  hipLaunchKernelGGL(k_kfd_copy, dim3(kfd_grid(m->cols, KFD_THREADS), m->rows, m->n_cam), dim3(KFD_THREADS), 0, ctx_stream(c), k->g, (const uint8_t *)k->img[k->cur_set], m->rows,
                     m->cols, m->img + (size_t)slot * m->plane_bytes());
  kfd_launch_blur(c, m, slot);
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_kfd_extract(gfbe_ctx *c, gfbe_kfd *m, int32_t slot, int32_t *offset_out, float *pts, int32_t *score, float *pts_norm, uint64_t *desc, int32_t *counters) {
  gfbe_status rc = handle_ready(c, m, "gfbe_kfd_extract");
  if (rc != GFBE_OK) return rc;
  if ((rc = kfd_slot(c, m, "gfbe_kfd_extract", slot, true)) != GFBE_OK) return rc;
  hipStream_t st = ctx_stream(c);
  const size_t C = (size_t)m->n_cam, o = (size_t)slot * m->plane_bytes();
  GFBE_CHECK(c, hipMemsetAsync(m->rowcnt, 0, sizeof(int) * C * (size_t)m->rows, st));
  GFBE_CHECK(c, hipMemsetAsync(m->cnt_d, 0, sizeof(int) * 4 * C, st));
  hipLaunchKernelGGL(k_kfd_fast, dim3(kfd_grid(m->cols, KFD_FW), kfd_grid(m->rows, KFD_FH), m->n_cam), dim3(KFD_THREADS), 0, st, (const uint8_t *)m->img + o, m->rows, m->cols,
                     m->threshold, m->plane + o, m->rowcnt, m->cnt_d);
  hipLaunchKernelGGL(k_kfd_list, dim3(m->n_cam), dim3(KFD_THREADS), 0, st, m->rows, m->cols, m->cap, (const uint8_t *)m->plane + o, m->rowcnt, m->l_pts, m->l_score, m->cnt_d);
  KfdBriefArgs A;
  std::memset(&A, 0, sizeof A);
  A.blur = m->blur + o; A.pairs = m->pairs; A.cams = m->cams; A.pts = m->l_pts; A.counters = m->cnt_d; A.cap = m->cap; A.rows = m->rows; A.cols = m->cols;
  A.desc = m->l_desc; A.ptsn = m->l_ptsn;
  hipLaunchKernelGGL(k_kfd_brief, dim3(kfd_grid(m->cap, KFD_THREADS / 64), m->n_cam), dim3(KFD_THREADS), 0, st, A);
  GFBE_CHECK(c, hipMemcpyAsync(m->cnt_h, m->cnt_d, sizeof(int) * 4 * C, hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));      // the one wait
  GFBE_CHECK(c, hipGetLastError());
  m->scored[slot] = true; m->extracted = true;
  std::vector<int32_t> off(C + 1, 0);
  for (size_t q = 0; q < C; q++) { m->listed[q] = std::max(0, std::min(m->cnt_h[4 * q + 2], m->cap)); off[q + 1] = off[q] + m->listed[q]; }
  if (offset_out) std::memcpy(offset_out, off.data(), sizeof(int32_t) * (C + 1));
  if (counters) std::memcpy(counters, m->cnt_h, sizeof(int32_t) * 4 * C);
  if (pts || score || pts_norm || desc) {      // the lists, packed over the cameras: a second wait, for callers that want them on the host
    for (size_t q = 0; q < C; q++) {
      const size_t n = (size_t)m->listed[q], src = q * (size_t)m->cap, dst = (size_t)off[q];
      if (!n) continue;
      if (pts) GFBE_CHECK(c, hipMemcpyAsync(pts + 2 * dst, m->l_pts + 2 * src, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, st));
      if (score) GFBE_CHECK(c, hipMemcpyAsync(score + dst, m->l_score + src, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
      if (pts_norm) GFBE_CHECK(c, hipMemcpyAsync(pts_norm + 2 * dst, m->l_ptsn + 2 * src, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, st));
      if (desc) GFBE_CHECK(c, hipMemcpyAsync(desc + 4 * dst, m->l_desc + 4 * src, sizeof(uint64_t) * 4 * n, hipMemcpyDeviceToHost, st));
    }
    GFBE_CHECK(c, hipStreamSynchronize(st));
  }
  return GFBE_OK;
}

gfbe_status gfbe_kfd_describe(gfbe_ctx *c, gfbe_kfd *m, int32_t slot, const int32_t *offset, const float *pts_uv, uint64_t *desc_out, int32_t *counters) {
  gfbe_status rc = handle_ready(c, m, "gfbe_kfd_describe");
  if (rc != GFBE_OK) return rc;
  if ((rc = kfd_slot(c, m, "gfbe_kfd_describe", slot, true)) != GFBE_OK) return rc;
  const size_t C = (size_t)m->n_cam;
  if (!offset || offset[0] != 0) return handle_bad(c, "gfbe_kfd_describe", "offsets that do not ascend from 0");
  int most = 0;
  for (size_t q = 0; q < C; q++) {
    if (offset[q + 1] < offset[q]) return handle_bad(c, "gfbe_kfd_describe", "offsets that do not ascend from 0");
    if (offset[q + 1] - offset[q] > m->wcap) return handle_bad(c, "gfbe_kfd_describe", "a camera has more points than window_capacity");
    most = std::max(most, offset[q + 1] - offset[q]);
  }
  const size_t n = (size_t)offset[C];
  if (n > 0 && !pts_uv) return handle_bad(c, "gfbe_kfd_describe", "pts_uv NULL");
  std::vector<int32_t> bad(C, 0);
  {
    Staged sg(c, m, n * 8 + C * 8 + 8192);
    const int *d_off = sg.up((const int *)offset, C + 1);
    const float *d_pts = sg.up(pts_uv, 2 * n);
    int *o_bad = sg.up((const int *)nullptr, C);
    if (!sg.ok) { ctx_set_error(c, "gfbe_kfd_describe: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    GFBE_CHECK(c, hipMemsetAsync(o_bad, 0, sizeof(int) * C, ctx_stream(c)));
    if (most > 0) {
      KfdBriefArgs A;
      std::memset(&A, 0, sizeof A);
      A.blur = m->blur + (size_t)slot * m->plane_bytes(); A.pairs = m->pairs; A.cams = m->cams; A.pts = d_pts; A.off = d_off; A.cap = m->wcap; A.rows = m->rows; A.cols = m->cols;
      A.desc = m->w_desc; A.bad = o_bad;
      hipLaunchKernelGGL(k_kfd_brief, dim3(kfd_grid(most, KFD_THREADS / 64), m->n_cam), dim3(KFD_THREADS), 0, ctx_stream(c), A);
    }
    sg.down(bad.data(), (const int32_t *)o_bad, C);
    sg.down(desc_out, (const uint64_t *)m->w_desc, 4 * n);
    sg.finish();      // the one wait
    GFBE_CHECK(c, hipGetLastError());
  }
  m->w_off.assign(offset, offset + C + 1);
  m->described = true;
  if (counters) for (size_t q = 0; q < C; q++) { counters[2 * q] = offset[q + 1] - offset[q]; counters[2 * q + 1] = bad[q]; }
  return GFBE_OK;
}

gfbe_status gfbe_kfd_add_keyframe(gfbe_ctx *c, gfbe_kfd *m, int32_t camera, gfbe_ldb *db, int32_t detect_loop, int32_t *index_out, int32_t *loop_index, int32_t *n_results,
                                  int32_t *result_id, double *result_score) {
  gfbe_status rc = handle_ready(c, m, "gfbe_kfd_add_keyframe");
  if (rc != GFBE_OK) return rc;
  if (camera < 0 || camera >= m->n_cam) return handle_bad(c, "gfbe_kfd_add_keyframe", "camera outside the handle's");
  if (!db) return handle_bad(c, "gfbe_kfd_add_keyframe", "loop database NULL");
  if (!m->extracted) return handle_bad(c, "gfbe_kfd_add_keyframe", "no lists are held: extract first");
  const size_t list = (size_t)camera * (size_t)m->cap;
  return ldb_add_keyframe_device(c, db, "gfbe_kfd_add_keyframe", m->listed[(size_t)camera], m->l_desc + 4 * list, m->l_pts + 2 * list, m->l_ptsn + 2 * list, detect_loop, index_out,
                                 loop_index, n_results, result_id, result_score);
}

gfbe_status gfbe_kfd_match(gfbe_ctx *c, gfbe_kfd *m, int32_t camera, gfbe_ldb *db, int32_t old_index, uint8_t *status, int32_t *best_index, int32_t *best_dist, int32_t *n_matched,
                           int32_t *matched_src, float *matched_pt, float *matched_pt_norm) {
  gfbe_status rc = handle_ready(c, m, "gfbe_kfd_match");
  if (rc != GFBE_OK) return rc;
  if (camera < 0 || camera >= m->n_cam) return handle_bad(c, "gfbe_kfd_match", "camera outside the handle's");
  if (!db) return handle_bad(c, "gfbe_kfd_match", "loop database NULL");
  if (!m->described) return handle_bad(c, "gfbe_kfd_match", "no window descriptors are held: describe first");
  const int b = m->w_off[(size_t)camera], n = m->w_off[(size_t)camera + 1] - b;
  return ldb_match_device(c, db, "gfbe_kfd_match", old_index, n, m->w_desc + 4 * (size_t)b, status, best_index, best_dist, n_matched, matched_src, matched_pt, matched_pt_norm);
}

gfbe_status gfbe_kfd_download(gfbe_ctx *c, gfbe_kfd *m, int32_t slot, int32_t camera, uint8_t *blurred_out, uint8_t *score_out) {
  gfbe_status rc = handle_ready(c, m, "gfbe_kfd_download");
  if (rc != GFBE_OK) return rc;
  if ((rc = kfd_slot(c, m, "gfbe_kfd_download", slot, true)) != GFBE_OK) return rc;
  if (camera < 0 || camera >= m->n_cam) return handle_bad(c, "gfbe_kfd_download", "camera outside the handle's");
  if (score_out && !m->scored[slot]) return handle_bad(c, "gfbe_kfd_download", "the slot has no score plane: extract it first");
  hipStream_t st = ctx_stream(c);
  const size_t px = (size_t)m->rows * (size_t)m->cols, o = (size_t)slot * m->plane_bytes() + (size_t)camera * px;
  if (blurred_out) GFBE_CHECK(c, hipMemcpyAsync(blurred_out, m->blur + o, px, hipMemcpyDeviceToHost, st));
  if (score_out) GFBE_CHECK(c, hipMemcpyAsync(score_out, m->plane + o, px, hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  return GFBE_OK;
}

}  // extern "C"
