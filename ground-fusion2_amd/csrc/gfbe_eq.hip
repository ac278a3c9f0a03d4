// gfbe_eq.hip — the image equalisation in front of the tracker and of the keyframe descriptors on the device: CLAHE of the 8-bit images
// of n cameras, in place, where the reference calls
//
//   cv::createCLAHE()->apply(image, image)             vins_estimator/src/rosNodeTest.cpp:271-276, dense_map/src/pose_graph_node.cpp:642-647      k_eq_lut, k_eq_apply
//
// The rules are in gfbe_eq.h and include/gfbe_eq.h; every per-bin and per-pixel statement is the header's function, compiled here for
// the device. k_eq_lut: one workgroup per (tile, camera); the tile's pixels as 4-byte words where a row allows it and by reflected
// index in the extension, into one LDS sub-histogram per wave; thread i then owns bin i: the sum of the sub-histograms, the excess
// (one workgroup scan for its sum), the closed-form redistribution, a second scan for the running sum, one byte of the LUT. All
// integer: the order of the atomics cannot matter. k_eq_apply: a workgroup owns a 64 x 16 block of the image, four pixels a thread
// as one word; the LUTs its block can reach (a 64 x 16 block spans at most a few cells of the half-tile-shifted grid) are staged in
// LDS, or read from global memory when the tiles are so small that more than EQ_STAGE of them are in reach; the coefficients of
// E5 are computed in registers. Two launches, no host wait, no scratch, integer LDS atomics only.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/gfbe_eq.h"
#include "gfbe_device.h"
#include "gfbe_klt_priv.h"
#include "gfbe_eq.h"
#include "gfbe_handle.h"

using namespace gfd;

static_assert(sizeof(gfbe_eq_options) == 24, "the layout of include/gfbe_eq.h");

struct gfbe_eq : gfbe_handle {
  gfbe_eq_options opt;
  int n_cam = 0;
  EqGeom g;
  uint8_t *lut = nullptr;                      // [n_cam][tiles_y][tiles_x][256]
  bool has_lut = false;
  uint8_t *img_d = nullptr, *img_h = nullptr;  // apply's images and their pinned mirror
  size_t plane_bytes() const { return (size_t)n_cam * (size_t)g.rows * (size_t)g.cols; }
  size_t lut_bytes() const { return (size_t)n_cam * (size_t)g.tiles_y * (size_t)g.tiles_x * EQ_BINS; }
};

namespace {
constexpr int EQ_THREADS = 256, EQ_WAVES = EQ_THREADS / 64;
constexpr int EQ_BW = 64, EQ_BH = 16;        // k_eq_apply's block: 16 threads of 4 pixels a row, 16 rows
constexpr int EQ_STAGE = 16;                 // LUTs a block stages in LDS (4 KiB)
static_assert(EQ_BINS == EQ_THREADS, "thread i owns bin i");
static_assert(EQ_BW / 4 * EQ_BH == EQ_THREADS, "four pixels a thread");

// ---- E1 .. E4 -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EQ_THREADS) void k_eq_lut(EqGeom g, const uint8_t *img, uint8_t *lut) {
  __shared__ int s_hist[EQ_WAVES][EQ_BINS];
  __shared__ int s_scan[20];
  const int t = threadIdx.x, tile = blockIdx.x, cam = blockIdx.y, tx = tile % g.tiles_x, ty = tile / g.tiles_x;
#pragma unroll
  for (int w = 0; w < EQ_WAVES; w++) s_hist[w][t] = 0;
  __syncthreads();
  int *hist = s_hist[t >> 6];
  const uint8_t *src = img + (size_t)cam * (size_t)g.rows * (size_t)g.cols;
  const int X0 = tx * g.tw, Y0 = ty * g.th;
  // a row of the tile in groups: the pixels before the first 4-byte boundary of its source row, then words
  const int gpr = g.tw / 4 + 2, n = g.th * gpr;
  for (int e = t; e < n; e += EQ_THREADS) {
    const int ry = e / gpr, q = e - ry * gpr;
    const uint8_t *row = src + (size_t)klt_reflect101(Y0 + ry, g.rows) * (size_t)g.cols;
    const int lead = min((int)((4 - ((uintptr_t)(row + X0) & 3)) & 3), g.tw);
    const int xa = q == 0 ? 0 : lead + 4 * (q - 1), xb = q == 0 ? lead : min(xa + 4, g.tw);
    if (xa >= xb) continue;
    if (xb - xa == 4 && X0 + xb <= g.cols) {      // (inside the image and aligned by construction)
      const uint32_t v = *(const uint32_t *)(row + X0 + xa);
      atomicAdd(&hist[v & 255u], 1); atomicAdd(&hist[(v >> 8) & 255u], 1); atomicAdd(&hist[(v >> 16) & 255u], 1); atomicAdd(&hist[v >> 24], 1);
    } else {
      for (int x = xa; x < xb; x++) atomicAdd(&hist[row[klt_reflect101(X0 + x, g.cols)]], 1);
    }
  }
  __syncthreads();
  int bin = 0;
#pragma unroll
  for (int w = 0; w < EQ_WAVES; w++) bin += s_hist[w][t];
  int clipped = 0;
  (void)block_exclusive_scan<EQ_THREADS>(eq_excess(bin, g.limit), &clipped, s_scan);
  const int b = eq_redistribute(bin, t, g.limit, clipped);
  int total;
  const int sum = block_exclusive_scan<EQ_THREADS>(b, &total, s_scan) + b;
  lut[((size_t)cam * (size_t)(g.tiles_x * g.tiles_y) + (size_t)tile) * EQ_BINS + (size_t)t] = eq_lut_value(sum, g.scale);
}

// ---- E5, E6 -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EQ_THREADS) void k_eq_apply(EqGeom g, const uint8_t *lut, const uint8_t *in, uint8_t *out) {
  __shared__ uint32_t s_lut[EQ_STAGE * EQ_BINS / 4];
  const int t = threadIdx.x, cam = blockIdx.z, x0 = blockIdx.x * EQ_BW, y0 = blockIdx.y * EQ_BH;
  const uint8_t *L = lut + (size_t)cam * (size_t)(g.tiles_x * g.tiles_y) * EQ_BINS;
  // the tiles in reach of the block: eq_axis is monotone in x, so its first and last pixel bound them
  const int xl = min(x0 + EQ_BW, g.cols) - 1, yl = min(y0 + EQ_BH, g.rows) - 1;
  const int tx_lo = eq_axis(x0, g.inv_tw, g.tiles_x).t1, tx_hi = eq_axis(xl, g.inv_tw, g.tiles_x).t2;
  const int ty_lo = eq_axis(y0, g.inv_th, g.tiles_y).t1, ty_hi = eq_axis(yl, g.inv_th, g.tiles_y).t2;
  const int nx = tx_hi - tx_lo + 1, ny = ty_hi - ty_lo + 1;
  const bool staged = nx * ny <= EQ_STAGE;      // (uniform over the workgroup)
  if (staged) {
    for (int e = t; e < nx * ny * (EQ_BINS / 4); e += EQ_THREADS) {
      const int k = e / (EQ_BINS / 4), w = e % (EQ_BINS / 4), jy = k / nx, jx = k - jy * nx;
      s_lut[e] = *(const uint32_t *)(L + ((size_t)(ty_lo + jy) * (size_t)g.tiles_x + (size_t)(tx_lo + jx)) * EQ_BINS + 4 * (size_t)w);
    }
  }
  __syncthreads();
  const int x = x0 + 4 * (t % (EQ_BW / 4)), y = y0 + t / (EQ_BW / 4);
  if (x >= g.cols || y >= g.rows) return;
  const size_t p = ((size_t)cam * (size_t)g.rows + (size_t)y) * (size_t)g.cols + (size_t)x;
  const int np = min(4, g.cols - x);
  const bool word = np == 4 && (((uintptr_t)(in + p) | (uintptr_t)(out + p)) & 3) == 0;
  uint32_t v4 = 0;
  if (word) v4 = *(const uint32_t *)(in + p);
  else for (int k = 0; k < np; k++) v4 |= (uint32_t)in[p + k] << (8 * k);
  const EqAxis Y = eq_axis(y, g.inv_th, g.tiles_y);
  const uint8_t *sl = (const uint8_t *)s_lut;
  uint32_t r4 = 0;
  for (int k = 0; k < np; k++) {
    const EqAxis X = eq_axis(x + k, g.inv_tw, g.tiles_x);
    const int v = (int)((v4 >> (8 * k)) & 255u);
    int l11, l12, l21, l22;
    if (staged) {
      const int a = (Y.t1 - ty_lo) * nx - tx_lo, b = (Y.t2 - ty_lo) * nx - tx_lo;
      l11 = sl[(a + X.t1) * EQ_BINS + v]; l12 = sl[(a + X.t2) * EQ_BINS + v]; l21 = sl[(b + X.t1) * EQ_BINS + v]; l22 = sl[(b + X.t2) * EQ_BINS + v];
    } else {
      const size_t a = (size_t)Y.t1 * (size_t)g.tiles_x, b = (size_t)Y.t2 * (size_t)g.tiles_x;
      l11 = L[(a + (size_t)X.t1) * EQ_BINS + v]; l12 = L[(a + (size_t)X.t2) * EQ_BINS + v]; l21 = L[(b + (size_t)X.t1) * EQ_BINS + v]; l22 = L[(b + (size_t)X.t2) * EQ_BINS + v];
    }
    r4 |= (uint32_t)eq_interp(l11, l12, l21, l22, X, Y) << (8 * k);
  }
  if (word) *(uint32_t *)(out + p) = r4;
  else for (int k = 0; k < np; k++) out[p + k] = (uint8_t)(r4 >> (8 * k));
}

const char *eq_options_error(const gfbe_eq_options *o) {
  if (o->struct_size != (int32_t)sizeof(gfbe_eq_options)) return "gfbe_eq_options.struct_size does not match this library (ABI mismatch)";
  return nullptr;
}
int eq_grid(int n, int per) { return (n + per - 1) / per; }

// E1 .. E6 on [n_cam][rows][cols] device images in place, behind everything queued on the context's stream
void eq_enqueue(gfbe_ctx *c, gfbe_eq *m, uint8_t *img) {
  hipStream_t st = ctx_stream(c);
  const EqGeom &g = m->g;
  hipLaunchKernelGGL(k_eq_lut, dim3(g.tiles_x * g.tiles_y, m->n_cam), dim3(EQ_THREADS), 0, st, g, (const uint8_t *)img, m->lut);
  hipLaunchKernelGGL(k_eq_apply, dim3(eq_grid(g.cols, EQ_BW), eq_grid(g.rows, EQ_BH), m->n_cam), dim3(EQ_THREADS), 0, st, g, (const uint8_t *)m->lut, (const uint8_t *)img, img);
  m->has_lut = true;
}

}  // namespace

extern "C" {

void gfbe_eq_default_options(gfbe_eq_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = (int32_t)sizeof *o;
  o->tiles_x = 8; o->tiles_y = 8; o->clip_limit = 40.0;
}

void gfbe_eq_destroy(gfbe_ctx *c, gfbe_eq *m) {
  if (!m) return;
  m->release(c);
  delete m;
}

gfbe_status gfbe_eq_create(gfbe_ctx *c, int32_t n_cameras, int32_t rows, int32_t cols, const gfbe_eq_options *opt, gfbe_eq **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  gfbe_eq_options o;
  if (opt) o = *opt; else gfbe_eq_default_options(&o);
  if (const char *bad = eq_options_error(&o)) return handle_bad(c, "gfbe_eq_create", bad);
  if (const char *bad = eq_geom_error(rows, cols, o.tiles_x, o.tiles_y, o.clip_limit)) return handle_bad(c, "gfbe_eq_create", bad);
  if (n_cameras < 1 || n_cameras > 65535) return handle_bad(c, "gfbe_eq_create", "n_cameras outside 1 .. 65535 (a camera is a grid row)");
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_eq_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  gfbe_eq *m = new gfbe_eq();
  CreateGuard<gfbe_eq> guard{c, m, gfbe_eq_destroy};
  m->owner = c; m->opt = o; m->n_cam = n_cameras;
  m->g = eq_geom(rows, cols, o.tiles_x, o.tiles_y, o.clip_limit);
  if (!(m->alloc(&m->lut, m->lut_bytes()) && m->alloc(&m->img_d, m->plane_bytes()) && m->alloc_pinned(&m->img_h, m->plane_bytes()))) {
    ctx_set_error(c, "gfbe_eq_create: device allocation failed");
    return GFBE_DEVICE_ERROR;
  }
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  guard.armed = false;
  *out = m;
  return GFBE_OK;
}

gfbe_status gfbe_eq_apply(gfbe_ctx *c, gfbe_eq *m, const uint8_t *images_in, uint8_t *images_out) {
  gfbe_status rc = handle_ready(c, m, "gfbe_eq_apply");
  if (rc != GFBE_OK) return rc;
  if (!images_in || !images_out) return handle_bad(c, "gfbe_eq_apply", "images_in or images_out NULL");
  hipStream_t st = ctx_stream(c);
  const size_t P = m->plane_bytes();
  std::memcpy(m->img_h, images_in, P);      // (every apply ends with a wait: the mirror is free)
  GFBE_CHECK(c, hipMemcpyAsync(m->img_d, m->img_h, P, hipMemcpyHostToDevice, st));
  eq_enqueue(c, m, m->img_d);
  GFBE_CHECK(c, hipMemcpyAsync(m->img_h, m->img_d, P, hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));      // the one wait
  GFBE_CHECK(c, hipGetLastError());
  std::memcpy(images_out, m->img_h, P);
  return GFBE_OK;
}

gfbe_status gfbe_eq_push_klt(gfbe_ctx *c, gfbe_eq *m, gfbe_klt *k, const uint8_t *images) {
  gfbe_status rc = handle_ready(c, m, "gfbe_eq_push_klt");
  if (rc != GFBE_OK) return rc;
  if (!k) return handle_bad(c, "gfbe_eq_push_klt", "tracker NULL");
  if (!images) return handle_bad(c, "gfbe_eq_push_klt", "images NULL");
  if (k->owner != c) return handle_bad(c, "gfbe_eq_push_klt", "the tracker belongs to another context");
  if (k->n_cam != m->n_cam || k->rows != m->g.rows || k->cols != m->g.cols) return handle_bad(c, "gfbe_eq_push_klt", "the tracker's n_cameras, rows or cols are not the handle's");
  if ((rc = klt_push_upload(c, k, images)) != GFBE_OK) return rc;
  eq_enqueue(c, m, k->raw_d);
  return klt_push_enqueue(c, k);
}

gfbe_status gfbe_eq_push_kfd(gfbe_ctx *c, gfbe_eq *m, gfbe_kfd *d, int32_t slot, const uint8_t *images) {
  gfbe_status rc = handle_ready(c, m, "gfbe_eq_push_kfd");
  if (rc != GFBE_OK) return rc;
  if (!d) return handle_bad(c, "gfbe_eq_push_kfd", "describer NULL");
  if (!images) return handle_bad(c, "gfbe_eq_push_kfd", "images NULL");
  if ((rc = kfd_push_check(c, d, "gfbe_eq_push_kfd", slot, m->n_cam, m->g.rows, m->g.cols)) != GFBE_OK) return rc;
  uint8_t *img = nullptr;
  if ((rc = kfd_push_upload(c, d, slot, images, &img)) != GFBE_OK) return rc;
  eq_enqueue(c, m, img);
  return kfd_push_enqueue(c, d, slot);
}

gfbe_status gfbe_eq_download_lut(gfbe_ctx *c, gfbe_eq *m, uint8_t *lut_out) {
  gfbe_status rc = handle_ready(c, m, "gfbe_eq_download_lut");
  if (rc != GFBE_OK) return rc;
  if (!lut_out) return handle_bad(c, "gfbe_eq_download_lut", "lut_out NULL");
  if (!m->has_lut) return handle_bad(c, "gfbe_eq_download_lut", "no LUTs are held: apply or push first");
  hipStream_t st = ctx_stream(c);
  GFBE_CHECK(c, hipMemcpyAsync(lut_out, m->lut, m->lut_bytes(), hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  return GFBE_OK;
}

}  // extern "C"
