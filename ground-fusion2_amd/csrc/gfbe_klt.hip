// gfbe_klt.hip — the optical-flow tracker held on the device: for n cameras the padded image pyramids and derivative pyramids of the
// previous and the current image, the point lists, pyramidal Lucas-Kanade and the tracking half of FeatureTracker::trackImage.
//
//   opencv_buildOpticalFlowPyramid, calc_sharr_deriv    mesh/src/meshing/optical_flow/lkpyramid.cpp:516-619, :56-149     gfbe_klt_push_image
//   the tracker, calcOpticalFlowPyrLK                   :173-499                                                         gfbe_klt_flow
//   trackImage (tracking half)                          vins_estimator/src/featureTracker/feature_tracker.cpp:113-179    gfbe_klt_track
//
// The rules are in gfbe_klt.h and include/gfbe_klt.h; every per-pixel and per-point statement is the header's function, compiled here
// for the device. Pyramid: one thread per padded pixel, cameras in grid.z, one launch per level (a level reads the one before it);
// the Scharr derivative of level l and the reduction to level l + 1 both read level l only and share a launch; borders are written
// by the same threads, so every byte the tracker can read is written by every push. Tracker: one wave per point, the 441 window
// pixels seven of a row to a lane on 63 lanes, held in registers, the integer sums reduced with shuffles, the float statements run by every lane on the
// same numbers (the loop is wave-uniform by construction); the whole descent over the levels is one launch per pass. Decision and
// ordered compaction: one workgroup per camera. No atomics, no communication between workgroups inside a launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gfbe_klt.h"
#include "gfbe_device.h"
#include "gfbe_klt.h"
#include "gfbe_klt_priv.h"
#include "gfbe_handle.h"

using namespace gfd;

namespace {
constexpr int KLT_THREADS = 256, KLT_WAVES = KLT_THREADS / 64, KLT_DECIDE_THREADS = 1024, KLT_LANE_PIX = 7;

struct KltDevPyramid {      // klt_point's view of a camera's set
  const KltGeom &g; const uint8_t *img; const int16_t *der; int cam;
  __device__ KltLevel level(int l) const { return klt_view(g, img, der, cam, l); }
};

// ---- R1 / R2 ----------------------------------------------------------------------------------------------------------------------
// level 0 with its reflected border from the uploaded image
__global__ __launch_bounds__(KLT_THREADS) void k_klt_level0(KltGeom g, const uint8_t *raw, uint8_t *img) {
  const int st = g.w[0] + 2 * KLT_WIN, ph = g.h[0] + 2 * KLT_WIN, cam = blockIdx.z;
  const long long p = (long long)blockIdx.x * KLT_THREADS + threadIdx.x;
  if (p >= (long long)st * ph) return;
  const int x = (int)(p % st), y = (int)(p / st);
  const int sx = klt_reflect101(x - KLT_WIN, g.w[0]), sy = klt_reflect101(y - KLT_WIN, g.h[0]);
  img[(size_t)cam * (size_t)g.img_cam + (size_t)g.img_off[0] + (size_t)p] = raw[((size_t)cam * (size_t)g.h[0] + (size_t)sy) * (size_t)g.w[0] + (size_t)sx];
}

// the derivative of level l (zero border) and, when it exists, level l + 1 with its reflected border: both read level l only
__global__ __launch_bounds__(KLT_THREADS) void k_klt_step(KltGeom g, int l, int with_down, uint8_t *img, int16_t *der) {
  const int cam = blockIdx.z;
  const long long p = (long long)blockIdx.x * KLT_THREADS + threadIdx.x;
  const int st = g.w[l] + 2 * KLT_WIN, ph = g.h[l] + 2 * KLT_WIN;
  const uint8_t *src = img + (size_t)cam * (size_t)g.img_cam + (size_t)g.img_off[l] + (size_t)KLT_WIN * (size_t)st + KLT_WIN;      // pixel (0, 0) of level l
  if (p < (long long)st * ph) {
    const int x = (int)(p % st) - KLT_WIN, y = (int)(p / st) - KLT_WIN;
    int ix = 0, iy = 0;
    if (x >= 0 && x < g.w[l] && y >= 0 && y < g.h[l]) klt_scharr_pixel(src, st, g.w[l], g.h[l], x, y, &ix, &iy);
    int16_t *d = der + (size_t)cam * (size_t)g.der_cam + (size_t)g.der_off[l] + 2 * (size_t)p;
    d[0] = (int16_t)ix; d[1] = (int16_t)iy;
  }
  if (with_down) {
    const int st1 = g.w[l + 1] + 2 * KLT_WIN, ph1 = g.h[l + 1] + 2 * KLT_WIN;
    if (p < (long long)st1 * ph1) {
      const int x = klt_reflect101((int)(p % st1) - KLT_WIN, g.w[l + 1]), y = klt_reflect101((int)(p / st1) - KLT_WIN, g.h[l + 1]);
      img[(size_t)cam * (size_t)g.img_cam + (size_t)g.img_off[l + 1] + (size_t)p] = (uint8_t)klt_down_pixel(src, st, g.w[l], g.h[l], x, y);
    }
  }
}

// ---- R3 / R4: one wave per point -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The window of a wave: lane l < 63 holds the seven pixels 7 (l % 3) .. + 6 of window row l / 3 in registers; lane 63 holds none.
// A lane's pixels need the 8 x 2 block of neighbours at its first pixel: 16 byte loads for the image, 16 dword loads for the
// derivative (an (Ix, Iy) pair is one aligned dword).
struct KltWaveWindow {
  int lane;
  int I[KLT_LANE_PIX], Ix[KLT_LANE_PIX], Iy[KLT_LANE_PIX];
  __device__ __forceinline__ size_t first(const KltLevel &L, int x0, int y0) const {
    return (size_t)(y0 + lane / 3 + KLT_WIN) * (size_t)L.stride + (size_t)(x0 + KLT_LANE_PIX * (lane % 3) + KLT_WIN);
  }
  // the image values (descaled by 9) of the lane's seven pixels
  __device__ __forceinline__ void image_row(const KltLevel &L, int x0, int y0, const KltW &w, int *v) const {
    const uint8_t *p = L.img + first(L, x0, y0);
    int a[KLT_LANE_PIX + 1], b[KLT_LANE_PIX + 1];
#pragma unroll
    for (int q = 0; q <= KLT_LANE_PIX; q++) { a[q] = p[q]; b[q] = p[L.stride + q]; }
#pragma unroll
    for (int j = 0; j < KLT_LANE_PIX; j++) v[j] = klt_bilinear(a[j], a[j + 1], b[j], b[j + 1], w, 9);
  }
  __device__ __forceinline__ void gram(const KltLevel &L, int x0, int y0, const KltW &w, long long &s11, long long &s12, long long &s22) {
    int a11 = 0, a12 = 0, a22 = 0;      // (seven summands below 2^25 each)
#pragma unroll
    for (int j = 0; j < KLT_LANE_PIX; j++) I[j] = Ix[j] = Iy[j] = 0;
    if (lane < 63) {
      int v[KLT_LANE_PIX], a[KLT_LANE_PIX + 1], b[KLT_LANE_PIX + 1];
      image_row(L, x0, y0, w, v);
      const int *d = reinterpret_cast<const int *>(L.der + 2 * first(L, x0, y0));
#pragma unroll
      for (int q = 0; q <= KLT_LANE_PIX; q++) { a[q] = d[q]; b[q] = d[L.stride + q]; }
#pragma unroll
      for (int j = 0; j < KLT_LANE_PIX; j++) {
        I[j] = (int16_t)v[j];
        Ix[j] = (int16_t)klt_bilinear((int16_t)a[j], (int16_t)a[j + 1], (int16_t)b[j], (int16_t)b[j + 1], w, 14);      // (low half: Ix)
        Iy[j] = (int16_t)klt_bilinear(a[j] >> 16, a[j + 1] >> 16, b[j] >> 16, b[j + 1] >> 16, w, 14);
        a11 += Ix[j] * Ix[j]; a12 += Ix[j] * Iy[j]; a22 += Iy[j] * Iy[j];
      }
    }
    s11 = wave_sum(a11); s12 = wave_sum(a12); s22 = wave_sum(a22);
  }
  __device__ __forceinline__ void mismatch(const KltLevel &L, int x0, int y0, const KltW &w, long long &b1, long long &b2) const {
    int p1 = 0, p2 = 0;                  // (seven summands below 2^26 each)
    if (lane < 63) {
      int v[KLT_LANE_PIX];
      image_row(L, x0, y0, w, v);
#pragma unroll
      for (int j = 0; j < KLT_LANE_PIX; j++) { const int diff = v[j] - I[j]; p1 += diff * Ix[j]; p2 += diff * Iy[j]; }
    }
    b1 = wave_sum(p1); b2 = wave_sum(p2);
  }
  __device__ __forceinline__ long long abssum(const KltLevel &L, int x0, int y0, const KltW &w) const {
    int s = 0;
    if (lane < 63) {
      int v[KLT_LANE_PIX];
      image_row(L, x0, y0, w, v);
#pragma unroll
      for (int j = 0; j < KLT_LANE_PIX; j++) { const int diff = v[j] - I[j]; s += diff < 0 ? -diff : diff; }
    }
    return wave_sum(s);
  }
};

struct KltFlowArgs {
  KltGeom g;
  const uint8_t *imgI, *imgJ;
  const int16_t *derI, *derJ;
  const int *seg_begin, *seg_count;
  const float *prev;
  float *next;
  uint8_t *status;
  float *err;
  const int *gate;      // nullptr: every camera; else only the cameras with gate[c] == gate_want
  int gate_want, max_level, use_initial;
  KltParams P;
};

__global__ __launch_bounds__(KLT_THREADS) void k_klt_flow(KltFlowArgs A) {
  const int cam = blockIdx.y, i = blockIdx.x * KLT_WAVES + (threadIdx.x >> 6);
  if (A.gate && A.gate[cam] != A.gate_want) return;
  if (i >= A.seg_count[cam]) return;
  const size_t p = (size_t)A.seg_begin[cam] + (size_t)i;
  KltWaveWindow win;
  win.lane = threadIdx.x & 63;
  const KltDevPyramid I{A.g, A.imgI, A.derI, cam}, J{A.g, A.imgJ, A.derJ, cam};
  float nx = A.next[2 * p], ny = A.next[2 * p + 1], err;
  int status;
  klt_point(win, I, J, A.max_level, A.use_initial, A.prev[2 * p], A.prev[2 * p + 1], nx, ny, status, err, A.P, nullptr);
  if (win.lane == 0) { A.next[2 * p] = nx; A.next[2 * p + 1] = ny; A.status[p] = (uint8_t)status; A.err[p] = err; }
}

// ---- R5 -----------------------------------------------------------------------------------------------------------------------------
// the fallback of :131-132, decided per camera: a camera that tried its prediction (gate 2) takes the full call (gate 1) when fewer
// than min_success points succeeded, else none (gate 0)
__global__ __launch_bounds__(KLT_THREADS) void k_klt_fallback(const int *seg_begin, const int *seg_count, const uint8_t *status, int min_success, int *gate) {
  __shared__ int lds[20];
  const int cam = blockIdx.x;
  if (gate[cam] != 2) return;
  int mine = 0, total;
  for (int i = threadIdx.x; i < seg_count[cam]; i += KLT_THREADS) mine += status[(size_t)seg_begin[cam] + i] ? 1 : 0;
  (void)block_exclusive_scan<KLT_THREADS>(mine, &total, lds);
  if (threadIdx.x == 0) gate[cam] = total < min_success ? 1 : 0;
}

struct KltDecideArgs {
  KltGeom g;
  const uint8_t *img_cur;
  const int16_t *der_cur;
  const int *seg_begin, *count_in;
  const float *prev, *cur, *rev;
  const uint8_t *status, *rstatus;
  const int *ids_in, *cnt_in;
  uint8_t *dec;                                  // [rows] scratch: a point's decision, formed once
  float *pts_out;                                // the survivors on the handle (the other half) ...
  int *ids_out, *cnt_out, *count_out;
  float *prev_dl, *cur_dl;                       // ... and the call's results in the staging chunk
  int *ids_dl, *cnt_dl, *counters;
  int flow_back, border, grey_max;
  double flow_back_dist;
};
// klt_decide once per point, then reduceVector in one workgroup: every thread a contiguous chunk, a scan over the threads, the survivors
// in ascending order at the head of the camera's rows of the other half; track_cnt + 1
__global__ __launch_bounds__(KLT_DECIDE_THREADS) void k_klt_decide(KltDecideArgs A) {
  __shared__ int lds[20];
  const int cam = blockIdx.x, t = threadIdx.x, n = A.count_in[cam];
  const size_t base = (size_t)A.seg_begin[cam];
  const int chunk = (n + KLT_DECIDE_THREADS - 1) / KLT_DECIDE_THREADS, b0 = min(n, t * chunk), b1 = min(n, b0 + chunk);
  const KltLevel level0 = klt_view(A.g, A.img_cur, A.der_cur, cam, 0);
  int fwd = 0, back = 0, kept = 0, total, total_fwd, total_back;
  for (int i = b0; i < b1; i++) {
    const size_t p = base + (size_t)i;
    const int d = klt_decide(A.status[p], A.flow_back ? A.rstatus[p] : 1, A.prev[2 * p], A.prev[2 * p + 1], A.cur[2 * p], A.cur[2 * p + 1], A.rev[2 * p], A.rev[2 * p + 1],
                             A.flow_back, A.flow_back_dist, A.border, A.grey_max, level0);
    A.dec[p] = (uint8_t)d;      // (read back by this thread only)
    fwd += d >= 1; back += d >= 2; kept += d == 3;
  }
  (void)block_exclusive_scan<KLT_DECIDE_THREADS>(fwd, &total_fwd, lds);
  (void)block_exclusive_scan<KLT_DECIDE_THREADS>(back, &total_back, lds);
  int dst = block_exclusive_scan<KLT_DECIDE_THREADS>(kept, &total, lds);
  for (int i = b0; i < b1; i++) {
    const size_t p = base + (size_t)i;
    if (A.dec[p] != 3) continue;
    const size_t q = base + (size_t)dst;
    const float px = A.prev[2 * p], py = A.prev[2 * p + 1], cx = A.cur[2 * p], cy = A.cur[2 * p + 1];
    const int id = A.ids_in[p], tc = A.cnt_in[p] + 1;
    A.prev_dl[2 * q] = px; A.prev_dl[2 * q + 1] = py;
    A.pts_out[2 * q] = cx; A.pts_out[2 * q + 1] = cy; A.cur_dl[2 * q] = cx; A.cur_dl[2 * q + 1] = cy;
    A.ids_out[q] = id; A.ids_dl[q] = id; A.cnt_out[q] = tc; A.cnt_dl[q] = tc;
    dst++;
  }
  if (t == 0) {
    A.count_out[cam] = total;
    A.counters[4 * cam] = n; A.counters[4 * cam + 1] = total_fwd; A.counters[4 * cam + 2] = total_back; A.counters[4 * cam + 3] = total;
  }
}

const char *klt_options_error(const gfbe_klt_options *o) {
  if (o->struct_size != (int32_t)sizeof(gfbe_klt_options)) return "gfbe_klt_options.struct_size does not match this library (ABI mismatch)";
  if (o->max_level < 0 || o->max_level > GFBE_KLT_MAX_LEVEL) return "max_level outside 0 .. GFBE_KLT_MAX_LEVEL";
  if (o->border < 0 || o->prediction_min_success < 0) return "border / prediction_min_success < 0";
  if (!std::isfinite(o->epsilon) || !std::isfinite(o->min_eig_threshold) || !std::isfinite(o->flow_back_dist)) return "epsilon / min_eig_threshold / flow_back_dist must be finite";
  return nullptr;
}
int klt_grid(long long n, int per) { return (int)((n + per - 1) / per); }

KltFlowArgs klt_flow_args(const gfbe_klt *m, int direction, int max_level, int use_initial) {
  KltFlowArgs A;
  std::memset(&A, 0, sizeof A);
  const int si = direction ? m->cur_set : m->cur_set ^ 1, sj = si ^ 1;
  A.g = m->g; A.imgI = m->img[si]; A.derI = m->der[si]; A.imgJ = m->img[sj]; A.derJ = m->der[sj];
  A.max_level = std::min(max_level, m->g.n_levels - 1); A.use_initial = use_initial;
  A.P = klt_params(m->opt.max_count, m->opt.epsilon, m->opt.min_eig_threshold);
  return A;
}
void klt_launch_flow(gfbe_ctx *c, const gfbe_klt *m, const KltFlowArgs &A, int max_count) {
  if (max_count > 0) hipLaunchKernelGGL(k_klt_flow, dim3(klt_grid(max_count, KLT_WAVES), m->n_cam), dim3(KLT_THREADS), 0, ctx_stream(c), A);
}

}  // namespace

// ---- the two halves of a push, for gfbe_eq.hip (include/gfbe_eq.h) as well: it equalises raw_d between them
namespace gfd {
gfbe_status klt_push_upload(gfbe_ctx *c, gfbe_klt *m, const uint8_t *images) {
  hipStream_t st = ctx_stream(c);
  const size_t R = (size_t)m->n_cam * (size_t)m->rows * (size_t)m->cols;
  if (m->raw_busy) GFBE_CHECK(c, hipEventSynchronize(m->ev_raw));      // (the mirror's last copy has left it)
  std::memcpy(m->raw_h, images, R);
  GFBE_CHECK(c, hipMemcpyAsync(m->raw_d, m->raw_h, R, hipMemcpyHostToDevice, st));
  GFBE_CHECK(c, hipEventRecord(m->ev_raw, st));
  m->raw_busy = true;
  return GFBE_OK;
}

gfbe_status klt_push_enqueue(gfbe_ctx *c, gfbe_klt *m) {
  hipStream_t st = ctx_stream(c);
  m->cur_set ^= 1;
  m->n_pushed++;
  const KltGeom &g = m->g;
  uint8_t *img = m->img[m->cur_set];
  int16_t *der = m->der[m->cur_set];
  hipLaunchKernelGGL(k_klt_level0, dim3(klt_grid((long long)(g.w[0] + 2 * KLT_WIN) * (g.h[0] + 2 * KLT_WIN), KLT_THREADS), 1, m->n_cam), dim3(KLT_THREADS), 0, st, g,
                     (const uint8_t *)m->raw_d, img);
  for (int l = 0; l < g.n_levels; l++)
    hipLaunchKernelGGL(k_klt_step, dim3(klt_grid((long long)(g.w[l] + 2 * KLT_WIN) * (g.h[l] + 2 * KLT_WIN), KLT_THREADS), 1, m->n_cam), dim3(KLT_THREADS), 0, st, g, l,
                       (int)(l + 1 < g.n_levels), img, der);
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}
}  // namespace gfd

extern "C" {

void gfbe_klt_default_options(gfbe_klt_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = (int32_t)sizeof *o;
  o->max_level = 3; o->max_count = 30; o->flow_back = 1; o->border = 1; o->grey_max = 250; o->prediction_min_success = 10;
  o->epsilon = 0.01; o->min_eig_threshold = 1e-4; o->flow_back_dist = 0.5;
}

void gfbe_klt_destroy(gfbe_ctx *c, gfbe_klt *m) {
  if (!m) return;
  m->release(c);
  delete m;
}

gfbe_status gfbe_klt_create(gfbe_ctx *c, int32_t n_cameras, int32_t rows, int32_t cols, int32_t point_capacity, const gfbe_klt_options *opt, gfbe_klt **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  gfbe_klt_options o;
  if (opt) o = *opt; else gfbe_klt_default_options(&o);
  if (const char *bad = klt_options_error(&o)) return handle_bad(c, "gfbe_klt_create", bad);
  if (rows <= KLT_WIN || cols <= KLT_WIN || rows > (1 << 14) || cols > (1 << 14)) return handle_bad(c, "gfbe_klt_create", "rows / cols outside 22 .. 16384 (the window is 21 x 21)");
  if (n_cameras < 1 || n_cameras > (1 << 16) || point_capacity < 1 || point_capacity > (1 << 20) || (long long)n_cameras * point_capacity > (1ll << 28))
    return handle_bad(c, "gfbe_klt_create", "n_cameras outside 1 .. 2^16, point_capacity outside 1 .. 2^20 or more than 2^28 points in all");
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_klt_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  gfbe_klt *m = new gfbe_klt();
  CreateGuard<gfbe_klt> guard{c, m, gfbe_klt_destroy};
  m->owner = c; m->opt = o; m->n_cam = n_cameras; m->rows = rows; m->cols = cols; m->cap = point_capacity;
  KltGeom &g = m->g;
  std::memset(&g, 0, sizeof g);
  g.n_levels = klt_plan_levels(cols, rows, std::max(o.max_level, 1), g.w, g.h);      // (the prediction and the reverse call ask for level 1)
  long long io = 0;
  for (int l = 0; l < g.n_levels; l++) {
    g.img_off[l] = io; g.der_off[l] = 2 * io;
    io += ((long long)(g.w[l] + 2 * KLT_WIN) * (g.h[l] + 2 * KLT_WIN) + 255) & ~255ll;
  }
  g.img_cam = io; g.der_cam = 2 * io;
  hipStream_t st = ctx_stream(c);
  const size_t C = (size_t)n_cameras, N = C * (size_t)point_capacity, R = C * (size_t)rows * (size_t)cols;
  bool ok = m->alloc(&m->raw_d, R);
  for (int s = 0; s < 2 && ok; s++)
    ok = m->alloc(&m->img[s], C * (size_t)g.img_cam) && m->alloc(&m->der[s], C * (size_t)g.der_cam) && m->alloc(&m->pts[s], 2 * N) && m->alloc(&m->ids[s], N) && m->alloc(&m->cnt[s], N) &&
         m->alloc(&m->seg_count[s], C);
  ok = ok && m->alloc(&m->seg_begin, C) && m->alloc(&m->w_cur, 2 * N) && m->alloc(&m->w_rev, 2 * N) && m->alloc(&m->w_err, N) && m->alloc(&m->w_st, N) &&
       m->alloc(&m->w_rst, N) && m->alloc(&m->w_dec, N) && m->alloc(&m->gate, C);
  if (!ok) { ctx_set_error(c, "gfbe_klt_create: device allocation failed"); return GFBE_DEVICE_ERROR; }
  if (!m->alloc_pinned(&m->raw_h, R) || !m->create(&m->ev_raw) || !m->make_staging(c, "gfbe_klt_create", 1 << 16, false)) return GFBE_DEVICE_ERROR;
  m->begin_h.assign(C, 0); m->count_h.assign(C, 0);
  GFBE_CHECK(c, hipStreamSynchronize(st));
  guard.armed = false;
  *out = m;
  return GFBE_OK;
}

gfbe_status gfbe_klt_push_image(gfbe_ctx *c, gfbe_klt *m, const uint8_t *images) {
  gfbe_status rc = handle_ready(c, m, "gfbe_klt_push_image");
  if (rc != GFBE_OK) return rc;
  if (!images) return handle_bad(c, "gfbe_klt_push_image", "images NULL");
  if ((rc = klt_push_upload(c, m, images)) != GFBE_OK) return rc;
  return klt_push_enqueue(c, m);
}

gfbe_status gfbe_klt_set_points(gfbe_ctx *c, gfbe_klt *m, const int32_t *offset, const float *pts, const int32_t *ids, const int32_t *track_cnt) {
  gfbe_status rc = handle_ready(c, m, "gfbe_klt_set_points");
  if (rc != GFBE_OK) return rc;
  const int bad = klt_check_points(m->n_cam, offset, m->cap, pts);
  if (bad == KLT_C_COUNT) return handle_bad(c, "gfbe_klt_set_points", "offsets that do not ascend from 0, a camera with more points than point_capacity, or pts NULL");
  if (bad == KLT_C_FINITE) return handle_bad(c, "gfbe_klt_set_points", "a non-finite point");
  const size_t C = (size_t)m->n_cam, N = (size_t)offset[m->n_cam];
  if (N > 0 && (!ids || !track_cnt)) return handle_bad(c, "gfbe_klt_set_points", "ids / track_cnt NULL");
  std::vector<int> cnt(C);
  for (size_t k = 0; k < C; k++) cnt[k] = offset[k + 1] - offset[k];
  hipStream_t st = ctx_stream(c);
  {
    Staged sg(c, m, N * 16 + C * 8 + 4096);
    const float *dp = sg.up(pts, 2 * N);
    const int32_t *di = sg.up(ids, N), *dc = sg.up(track_cnt, N), *dof = sg.up(offset, C), *dn = sg.up((const int32_t *)cnt.data(), C);
    if (!sg.ok) { ctx_set_error(c, "gfbe_klt_set_points: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    const int hf = m->half;
    if (N > 0) {
      GFBE_CHECK(c, hipMemcpyAsync(m->pts[hf], dp, sizeof(float) * 2 * N, hipMemcpyDeviceToDevice, st));
      GFBE_CHECK(c, hipMemcpyAsync(m->ids[hf], di, sizeof(int) * N, hipMemcpyDeviceToDevice, st));
      GFBE_CHECK(c, hipMemcpyAsync(m->cnt[hf], dc, sizeof(int) * N, hipMemcpyDeviceToDevice, st));
    }
    GFBE_CHECK(c, hipMemcpyAsync(m->seg_begin, dof, sizeof(int) * C, hipMemcpyDeviceToDevice, st));
    GFBE_CHECK(c, hipMemcpyAsync(m->seg_count[hf], dn, sizeof(int) * C, hipMemcpyDeviceToDevice, st));
    sg.finish();
  }
  for (size_t k = 0; k < C; k++) { m->begin_h[k] = offset[k]; m->count_h[k] = cnt[k]; }
  return GFBE_OK;
}

gfbe_status gfbe_klt_track(gfbe_ctx *c, gfbe_klt *m, const uint8_t *has_prediction, const float *predict_pts, int32_t *offset_out, float *prev_pts, float *cur_pts,
                           int32_t *ids, int32_t *track_cnt, int32_t *counters) {
  gfbe_status rc = handle_ready(c, m, "gfbe_klt_track");
  if (rc != GFBE_OK) return rc;
  if (m->n_pushed < 2) return handle_bad(c, "gfbe_klt_track", "two images must have been pushed");
  const size_t C = (size_t)m->n_cam;
  // the held rows: camera k at begin_h[k] .. + count_h[k]; `span` covers them all
  size_t span = 0;
  int max_count = 0;
  for (size_t k = 0; k < C; k++) { span = std::max(span, (size_t)m->begin_h[k] + (size_t)m->count_h[k]); max_count = std::max(max_count, m->count_h[k]); }
  bool any_pred = false;
  std::vector<int> gate(C, 1);
  std::vector<float> pred(2 * span, 0.f);
  if (has_prediction && predict_pts) {
    size_t row = 0;      // predict_pts follows the held points camera by camera
    for (size_t k = 0; k < C; k++) {
      const size_t n = (size_t)m->count_h[k];
      if (has_prediction[k]) {
        any_pred = true; gate[k] = 2;
        for (size_t i = 0; i < 2 * n; i++) {
          const float v = predict_pts[2 * row + i];
          if (!std::isfinite(v)) return handle_bad(c, "gfbe_klt_track", "a non-finite point in predict_pts");
          pred[2 * (size_t)m->begin_h[k] + i] = v;
        }
      }
      row += n;
    }
  }
  hipStream_t st = ctx_stream(c);
  const int hf = m->half, nh = hf ^ 1;
  std::vector<int32_t> cnts(4 * C, 0);
  size_t row = 0;
  {
    Staged sg(c, m, span * 32 + C * 20 + 4096);
    const int *dgate = sg.up((const int *)gate.data(), C);
    const float *dpred = sg.up(any_pred ? pred.data() : (const float *)nullptr, 2 * span);
    // the results: written into the staging chunk by k_klt_decide, one copy back and one wait (Staged::finish)
    int *o_cnts = sg.up((const int *)nullptr, 4 * C), *o_ids = sg.up((const int *)nullptr, span), *o_cnt = sg.up((const int *)nullptr, span);
    float *o_prev = sg.up((const float *)nullptr, 2 * span), *o_cur = sg.up((const float *)nullptr, 2 * span);
    if (!sg.ok) { ctx_set_error(c, "gfbe_klt_track: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    GFBE_CHECK(c, hipMemcpyAsync(m->gate, dgate, sizeof(int) * C, hipMemcpyDeviceToDevice, st));
    KltFlowArgs A = klt_flow_args(m, 0, 1, 1);
    A.seg_begin = m->seg_begin; A.seg_count = m->seg_count[hf]; A.prev = m->pts[hf]; A.next = m->w_cur; A.status = m->w_st; A.err = m->w_err; A.gate = m->gate;
    if (any_pred && span > 0) {                                                  // :121-131
      GFBE_CHECK(c, hipMemcpyAsync(m->w_cur, dpred, sizeof(float) * 2 * span, hipMemcpyDeviceToDevice, st));
      A.gate_want = 2;
      klt_launch_flow(c, m, A, max_count);
      hipLaunchKernelGGL(k_klt_fallback, dim3(m->n_cam), dim3(KLT_THREADS), 0, st, (const int *)m->seg_begin, (const int *)m->seg_count[hf], (const uint8_t *)m->w_st,
                         (int)m->opt.prediction_min_success, m->gate);
    }
    A.max_level = std::min((int)m->opt.max_level, m->g.n_levels - 1); A.use_initial = 0; A.gate_want = 1;      // :132, :135
    klt_launch_flow(c, m, A, max_count);
    if (m->opt.flow_back && span > 0) {                                          // :141
      GFBE_CHECK(c, hipMemcpyAsync(m->w_rev, m->pts[hf], sizeof(float) * 2 * span, hipMemcpyDeviceToDevice, st));
      KltFlowArgs B = klt_flow_args(m, 1, 1, 1);
      B.seg_begin = m->seg_begin; B.seg_count = m->seg_count[hf]; B.prev = m->w_cur; B.next = m->w_rev; B.status = m->w_rst; B.err = m->w_err;
      klt_launch_flow(c, m, B, max_count);
    }
    KltDecideArgs D;
    std::memset(&D, 0, sizeof D);
    D.g = m->g; D.img_cur = m->img[m->cur_set]; D.der_cur = m->der[m->cur_set]; D.seg_begin = m->seg_begin; D.count_in = m->seg_count[hf];
    D.prev = m->pts[hf]; D.cur = m->w_cur; D.rev = m->w_rev; D.status = m->w_st; D.rstatus = m->w_rst; D.ids_in = m->ids[hf]; D.cnt_in = m->cnt[hf];
    D.dec = m->w_dec; D.pts_out = m->pts[nh]; D.ids_out = m->ids[nh]; D.cnt_out = m->cnt[nh]; D.count_out = m->seg_count[nh];
    D.prev_dl = o_prev; D.cur_dl = o_cur; D.ids_dl = o_ids; D.cnt_dl = o_cnt; D.counters = o_cnts;
    D.flow_back = m->opt.flow_back; D.border = m->opt.border; D.grey_max = m->opt.grey_max; D.flow_back_dist = m->opt.flow_back_dist;
    hipLaunchKernelGGL(k_klt_decide, dim3(m->n_cam), dim3(KLT_DECIDE_THREADS), 0, st, D);
    // the result range comes back in one copy; the rows are compacted over the cameras straight from the pinned mirror
    sg.dlo = (size_t)((const char *)o_cnts - sg.bd); sg.dhi = (size_t)((const char *)(o_cur + 2 * span) - sg.bd);
    sg.finish();      // the one wait
    GFBE_CHECK(c, hipGetLastError());
    auto host = [&](const auto *d) { return (decltype(d))(sg.bh + ((const char *)d - sg.bd)); };
    const float *h_prev = host(o_prev), *h_cur = host(o_cur);
    const int *h_ids = host(o_ids), *h_cnt = host(o_cnt);
    std::memcpy(cnts.data(), host(o_cnts), sizeof(int32_t) * 4 * C);
    m->half = nh;
    for (size_t k = 0; k < C; k++) {
      const size_t n = (size_t)cnts[4 * k + 3], b = (size_t)m->begin_h[k];
      if (offset_out) offset_out[k] = (int32_t)row;
      if (prev_pts) std::memcpy(prev_pts + 2 * row, h_prev + 2 * b, sizeof(float) * 2 * n);
      if (cur_pts) std::memcpy(cur_pts + 2 * row, h_cur + 2 * b, sizeof(float) * 2 * n);
      if (ids) std::memcpy(ids + row, h_ids + b, sizeof(int32_t) * n);
      if (track_cnt) std::memcpy(track_cnt + row, h_cnt + b, sizeof(int32_t) * n);
      m->count_h[k] = (int)n;
      row += n;
    }
  }
  if (offset_out) offset_out[C] = (int32_t)row;
  if (counters) std::memcpy(counters, cnts.data(), sizeof(int32_t) * 4 * C);
  return GFBE_OK;
}

gfbe_status gfbe_klt_flow(gfbe_ctx *c, gfbe_klt *m, int32_t direction, int32_t max_level, int32_t use_initial_flow, const int32_t *offset, const float *pts, float *next_pts,
                          uint8_t *status, float *err) {
  gfbe_status rc = handle_ready(c, m, "gfbe_klt_flow");
  if (rc != GFBE_OK) return rc;
  if (m->n_pushed < 2) return handle_bad(c, "gfbe_klt_flow", "two images must have been pushed");
  if ((direction != 0 && direction != 1) || max_level < 0 || max_level > GFBE_KLT_MAX_LEVEL) return handle_bad(c, "gfbe_klt_flow", "direction outside 0 .. 1 or max_level outside 0 .. GFBE_KLT_MAX_LEVEL");
  int bad = klt_check_points(m->n_cam, offset, m->cap, pts);
  const size_t C = (size_t)m->n_cam, N = bad ? 0 : (size_t)offset[m->n_cam];
  if (!bad && N > 0 && !next_pts) bad = KLT_C_COUNT;
  if (!bad && use_initial_flow)
    for (size_t i = 0; i < 2 * N; i++) if (!std::isfinite(next_pts[i])) { bad = KLT_C_FINITE; break; }
  if (bad == KLT_C_COUNT) return handle_bad(c, "gfbe_klt_flow", "offsets that do not ascend from 0, a camera with more points than point_capacity, or a NULL array");
  if (bad == KLT_C_FINITE) return handle_bad(c, "gfbe_klt_flow", "a non-finite point");
  std::vector<int> cnt(C);
  int max_count = 0;
  for (size_t k = 0; k < C; k++) { cnt[k] = offset[k + 1] - offset[k]; max_count = std::max(max_count, cnt[k]); }
  {
    Staged sg(c, m, N * 24 + C * 8 + 8192);
    const float *dp = sg.up(pts, 2 * N);
    float *dn = sg.up(use_initial_flow ? (const float *)next_pts : (const float *)nullptr, 2 * N);
    const int *dof = sg.up(offset, C), *dc = sg.up((const int *)cnt.data(), C);
    float *de = sg.up((const float *)nullptr, N);
    uint8_t *ds = sg.up((const uint8_t *)nullptr, N);
    if (!sg.ok) { ctx_set_error(c, "gfbe_klt_flow: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    KltFlowArgs A = klt_flow_args(m, direction, max_level, use_initial_flow ? 1 : 0);
    A.seg_begin = dof; A.seg_count = dc; A.prev = dp; A.next = dn; A.status = ds; A.err = de;
    klt_launch_flow(c, m, A, max_count);
    sg.down(next_pts, (const float *)dn, 2 * N);
    sg.down(status, (const uint8_t *)ds, N);
    sg.down(err, (const float *)de, N);
    sg.finish();
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_klt_download_level(gfbe_ctx *c, gfbe_klt *m, int32_t which, int32_t camera, int32_t level, uint8_t *image_out, int16_t *deriv_out, int32_t *dims_out) {
  gfbe_status rc = handle_ready(c, m, "gfbe_klt_download_level");
  if (rc != GFBE_OK) return rc;
  if ((which != 0 && which != 1) || camera < 0 || camera >= m->n_cam || level < 0 || level >= m->g.n_levels)
    return handle_bad(c, "gfbe_klt_download_level", "which outside 0 .. 1, camera outside the handle's, or a level that was not built");
  if (m->n_pushed < (which ? 1 : 2)) return handle_bad(c, "gfbe_klt_download_level", "that image set has not been pushed");
  const KltGeom &g = m->g;
  const int s = which ? m->cur_set : m->cur_set ^ 1;
  const size_t px = (size_t)(g.w[level] + 2 * KLT_WIN) * (size_t)(g.h[level] + 2 * KLT_WIN);
  hipStream_t st = ctx_stream(c);
  if (image_out) GFBE_CHECK(c, hipMemcpyAsync(image_out, m->img[s] + (size_t)camera * (size_t)g.img_cam + (size_t)g.img_off[level], px, hipMemcpyDeviceToHost, st));
  if (deriv_out) GFBE_CHECK(c, hipMemcpyAsync(deriv_out, m->der[s] + (size_t)camera * (size_t)g.der_cam + (size_t)g.der_off[level], 2 * px * sizeof(int16_t), hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  if (dims_out) { dims_out[0] = g.w[level]; dims_out[1] = g.h[level]; dims_out[2] = g.w[level] + 2 * KLT_WIN; dims_out[3] = g.n_levels; }
  return GFBE_OK;
}

}  // extern "C"
