// gfbe_det.hip — corner detection on the images and the held points of a tracker handle (gfbe_klt.hip): setMask, goodFeaturesToTrack
// and addPoints of FeatureTracker::trackImage for n cameras, and the mask-free call of the keyframes.
//
//   setMask                         vins_estimator/src/featureTracker/feature_tracker.cpp:56-83      k_det_mask
//   cv::goodFeaturesToTrack         :198 (and dense_map/src/keyframe.cpp:169)                        k_det_tile<1>, k_det_thresh, k_det_tile<2>, k_det_select
//   addPoints                       :85-93                                                           k_det_offsets, k_det_pack
//
// The rules are in gfbe_det.h and include/gfbe_det.h; every per-pixel statement is the header's function, compiled here for the
// device. k_det_mask: one workgroup per camera, the order of G1 by a bitonic sort of 64-bit keys in LDS, the walk by one wave whose
// lanes test a point against the kept ones. k_det_tile: 32 x 8 pixels a workgroup, cameras in grid.z; the uint8 tile with a halo of 3
// is staged in LDS from the tracker's padded level 0, the Sobel pairs (halo 2) and the responses (halo 1) follow in LDS. The response
// plane is never stored: pass 1 reduces the largest clear response of a tile, k_det_thresh the tiles of a camera (no float atomics),
// pass 2 recomputes the responses and appends the candidates as 64-bit keys (response bits, pixel index). The append is atomic on an
// integer counter: the order of the list is arbitrary and is used by nothing, because the order of G3 is total on the keys and a list
// that overflows is dropped whole. k_det_select: one workgroup per camera; the next sort_chunk largest keys below the last bound by a
// radix select (eight 8-bit histograms in LDS), a bitonic sort of the chunk, the walk by one wave against the accepted corners in LDS;
// again while corners are wanted and candidates remain. k_det_offsets / k_det_pack: the kept points and the new corners of every camera,
// packed over the cameras as gfbe_klt_set_points leaves them, into the tracker's half and the staging chunk. No communication
// between workgroups inside a launch, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gfbe_det.h"
#include "gfbe_det.h"
#include "gfbe_device.h"
#include "gfbe_klt_priv.h"
#include "gfbe_handle.h"

using namespace gfd;

static_assert(DET_MAX_POINTS == GFBE_DET_MAX_POINTS, "the header's bound");

struct gfbe_det : gfbe_handle {
  gfbe_klt *trk = nullptr;
  gfbe_det_options opt;
  long long cand_cap = 0;
  int nbx = 0, nby = 0;
  int *kept_xy = nullptr;                      // [n_cam * cap][2] the pixels of the points G1 kept
  int *kept = nullptr, *want = nullptr, *n_in = nullptr, *next_id = nullptr, *cand_n = nullptr, *acc_n = nullptr, *ovf = nullptr, *none = nullptr, *zero = nullptr;      // [n_cam]
  float *bmax = nullptr, *thr = nullptr;      // [n_cam][tiles], [n_cam]
  unsigned long long *cand = nullptr;          // [n_cam][cand_cap]
  float *acc_pts = nullptr, *acc_resp = nullptr;      // [n_cam * cap][2], [n_cam * cap]: the corners a detect accepted
  int mask_min_dist = 0;                       // of the last detect
};

namespace {
constexpr int DET_THREADS = 256, DET_TW = 32, DET_TH = 8, DET_SCAN_THREADS = 1024;
typedef unsigned long long u64;

// ascending (or descending) bitonic sort of n = 2^k keys in LDS by the whole workgroup; the keys are complete and a barrier has passed
__device__ __forceinline__ void lds_bitonic(u64 *k, int n, bool descending) {
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < n / 2; i += DET_THREADS) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool up = ((lo & size) == 0) != descending;
        const u64 a = k[lo], b = k[hi];
        if ((a > b) == up) { k[lo] = b; k[hi] = a; }
      }
      __syncthreads();
    }
}
// one wave: is a listed pixel within r2 of (x, y)? inclusive: d2 <= r2 (the disc of G1), else d2 < r2 (the walk of G3)
__device__ __forceinline__ bool wave_hit(const volatile int *lx, const volatile int *ly, int n, int x, int y, int r2, bool inclusive, int lane) {
  int hit = 0;
  for (int k = lane; k < n; k += 64) {
    const int d = det_d2(x, y, lx[k], ly[k]);
    hit |= inclusive ? d <= r2 : d < r2;
  }
  return __any(hit) != 0;
}

// ---- G1 -----------------------------------------------------------------------------------------------------------------------------
struct DetMaskArgs {
  const int *seg_begin, *count_in;
  const float *pts_in;
  const int *ids_in, *cnt_in;
  float *pts_out;                              // the tracker's other half, camera k at rows k * cap
  int *ids_out, *cnt_out;
  int *kept_xy, *kept, *want, *n_in, *cand_n, *acc_n;
  int cap, w, h, r2, max_cnt;
};
__global__ __launch_bounds__(DET_THREADS) void k_det_mask(DetMaskArgs A) {
  __shared__ u64 s_key[DET_MAX_POINTS];
  __shared__ volatile int s_x[DET_MAX_POINTS], s_y[DET_MAX_POINTS];
  __shared__ int s_ord[DET_MAX_POINTS], s_nk;
  const int cam = blockIdx.x, t = threadIdx.x, n = min(A.count_in[cam], DET_MAX_POINTS);
  const size_t base = (size_t)A.seg_begin[cam], out = (size_t)cam * (size_t)A.cap;
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = t; i < np2; i += DET_THREADS) s_key[i] = i < n ? det_mask_key(A.cnt_in[base + i], i) : ~0ull;
  __syncthreads();
  lds_bitonic(s_key, np2, false);
  if (t < 64) {
    int nk = 0;
    for (int s = 0; s < n; s++) {
      const int idx = (int)(uint32_t)s_key[s], px = klt_round(A.pts_in[2 * (base + idx)]), py = klt_round(A.pts_in[2 * (base + idx) + 1]);
      if (!det_inside(px, py, A.w, A.h)) continue;
      if (wave_hit(s_x, s_y, nk, px, py, A.r2, true, t)) continue;
      if (t == 0) { s_x[nk] = px; s_y[nk] = py; s_ord[nk] = idx; }
      nk++;
      __threadfence_block();
    }
    if (t == 0) s_nk = nk;
  }
  __syncthreads();
  const int nk = s_nk;
  for (int j = t; j < nk; j += DET_THREADS) {
    const size_t p = base + (size_t)s_ord[j], q = out + (size_t)j;
    A.pts_out[2 * q] = A.pts_in[2 * p]; A.pts_out[2 * q + 1] = A.pts_in[2 * p + 1];
    A.ids_out[q] = A.ids_in[p]; A.cnt_out[q] = A.cnt_in[p];
    A.kept_xy[2 * q] = s_x[j]; A.kept_xy[2 * q + 1] = s_y[j];
  }
  if (t == 0) { A.kept[cam] = nk; A.want[cam] = max(0, A.max_cnt - nk); A.n_in[cam] = n; A.cand_n[cam] = 0; A.acc_n[cam] = 0; }
}

// ---- G2 / G3: the tiles ---------------------------------------------------------------------------------------------------------------
struct DetTileArgs {
  KltGeom g;
  const uint8_t *img;                          // the current set
  const int *kept, *want, *kept_xy;            // the discs of G1 (kept: zeros for the mask-free call)
  int cap, r2, min_dist;
  float *bmax;                                 // pass 1: [n_cam][tiles]
  const float *thr;                            // pass 2
  const int *none;
  u64 *cand;
  long long cand_cap;
  int *cand_n;
};
template <int PASS>
__global__ __launch_bounds__(DET_THREADS) void k_det_tile(DetTileArgs A) {
  __shared__ uint8_t s_img[DET_TH + 6][DET_TW + 8];
  __shared__ short s_dx[DET_TH + 4][DET_TW + 4], s_dy[DET_TH + 4][DET_TW + 4];
  __shared__ float s_e[DET_TH + 2][DET_TW + 2], s_red[DET_THREADS / 64];
  __shared__ int s_near[2 * DET_MAX_POINTS], s_nnear, s_nc, s_base;
  __shared__ u64 s_cand[DET_THREADS];
  const int cam = blockIdx.z, t = threadIdx.x, w = A.g.w[0], h = A.g.h[0], st = w + 2 * KLT_WIN;
  const int tile = blockIdx.y * gridDim.x + blockIdx.x, tiles = gridDim.x * gridDim.y;
  if (A.want[cam] <= 0 || (PASS == 2 && A.none[cam])) {      // (the same for the whole workgroup)
    if (PASS == 1 && t == 0) A.bmax[(size_t)cam * tiles + tile] = -INFINITY;
    return;
  }
  const int gx0 = blockIdx.x * DET_TW, gy0 = blockIdx.y * DET_TH;
  const uint8_t *img0 = A.img + (size_t)cam * (size_t)A.g.img_cam + (size_t)A.g.img_off[0] + (size_t)KLT_WIN * (size_t)st + KLT_WIN;      // pixel (0, 0)
  if (t == 0) { s_nnear = 0; s_nc = 0; }
  // the tile with a halo of 3 from the padded level (its border is 21 wide: nothing beyond w + 2, h + 2 is read)
  for (int i = t; i < (DET_TH + 6) * (DET_TW + 6); i += DET_THREADS) {
    const int ly = i / (DET_TW + 6), lx = i % (DET_TW + 6), gx = gx0 - 3 + lx, gy = gy0 - 3 + ly;
    s_img[ly][lx] = (gx <= w + 2 && gy <= h + 2) ? img0[(ptrdiff_t)gy * st + gx] : (uint8_t)0;
  }
  __syncthreads();
  // the kept points whose disc can reach the tile
  const int nk = A.kept[cam];
  for (int k = t; k < nk; k += DET_THREADS) {
    const size_t q = (size_t)cam * (size_t)A.cap + (size_t)k;
    const int kx = A.kept_xy[2 * q], ky = A.kept_xy[2 * q + 1];
    if (kx >= gx0 - A.min_dist && kx <= gx0 + DET_TW - 1 + A.min_dist && ky >= gy0 - A.min_dist && ky <= gy0 + DET_TH - 1 + A.min_dist) {
      const int s = atomicAdd(&s_nnear, 1);
      s_near[2 * s] = kx; s_near[2 * s + 1] = ky;
    }
  }
  // the Sobel pairs with a halo of 2; a position one pixel outside the image takes its mirror pixel's (det_sums)
  for (int i = t; i < (DET_TH + 4) * (DET_TW + 4); i += DET_THREADS) {
    const int ly = i / (DET_TW + 4), lx = i % (DET_TW + 4), gx = gx0 - 2 + lx, gy = gy0 - 2 + ly;
    int dx = 0, dy = 0;
    if (gx >= -1 && gx <= w && gy >= -1 && gy <= h) {
      const int rx = klt_reflect101(gx, w), ry = klt_reflect101(gy, h);
      det_sobel(&s_img[ry - gy0 + 3][rx - gx0 + 3], DET_TW + 8, &dx, &dy);
    }
    s_dx[ly][lx] = (short)dx; s_dy[ly][lx] = (short)dy;
  }
  __syncthreads();
  // the responses with a halo of 1
  for (int i = t; i < (DET_TH + 2) * (DET_TW + 2); i += DET_THREADS) {
    const int ly = i / (DET_TW + 2), lx = i % (DET_TW + 2), gx = gx0 - 1 + lx, gy = gy0 - 1 + ly;
    float v = 0.f;
    if (det_inside(gx, gy, w, h)) {
      int a = 0, b = 0, c = 0;
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int q = 0; q < 3; q++) { const int dx = s_dx[ly + j][lx + q], dy = s_dy[ly + j][lx + q]; a += dx * dx; b += dx * dy; c += dy * dy; }
      v = det_eig(a, b, c);
    }
    s_e[ly][lx] = v;
  }
  __syncthreads();
  const int lx = t % DET_TW, ly = t / DET_TW, gx = gx0 + lx, gy = gy0 + ly;
  const float v = s_e[ly + 1][lx + 1];
  bool clear = det_inside(gx, gy, w, h);
  const int nn = s_nnear;
  for (int k = 0; k < nn && clear; k++) clear = det_d2(gx, gy, s_near[2 * k], s_near[2 * k + 1]) > A.r2;
  if (PASS == 1) {
    float m = clear ? v : -INFINITY;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((t & 63) == 0) s_red[t >> 6] = m;
    __syncthreads();
    if (t == 0) A.bmax[(size_t)cam * tiles + tile] = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  } else {
    const float thr = A.thr[cam];
    if (clear && gx >= 1 && gx <= w - 2 && gy >= 1 && gy <= h - 2) {      // (an interior pixel: its 3 x 3 neighbours are inside the image)
      float m = 0.f;
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int q = 0; q < 3; q++) m = fmaxf(m, det_thresholded(s_e[ly + j][lx + q], thr));
      if (det_is_candidate(v, thr, m)) s_cand[atomicAdd(&s_nc, 1)] = det_key(v, gy * w + gx);
    }
    __syncthreads();
    const int nc = s_nc;
    if (t == 0 && nc > 0) s_base = atomicAdd(&A.cand_n[cam], nc);
    __syncthreads();
    if (t < nc && (long long)s_base + t < A.cand_cap) A.cand[(size_t)cam * (size_t)A.cand_cap + (size_t)s_base + (size_t)t] = s_cand[t];
  }
}

// maxVal of a camera from its tiles, and t
__global__ __launch_bounds__(DET_THREADS) void k_det_thresh(const float *bmax, int tiles, const int *want, double quality, float *thr, int *none) {
  __shared__ float s_red[DET_THREADS / 64];
  const int cam = blockIdx.x, t = threadIdx.x;
  float m = -INFINITY;
  if (want[cam] > 0)
    for (int i = t; i < tiles; i += DET_THREADS) m = fmaxf(m, bmax[(size_t)cam * tiles + i]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((t & 63) == 0) s_red[t >> 6] = m;
  __syncthreads();
  if (t == 0) {
    m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    const bool any = m > -INFINITY;
    none[cam] = any ? 0 : 1;
    thr[cam] = any ? det_threshold(m, quality) : 0.f;
  }
}

// ---- G3: selection and walk --------------------------------------------------------------------------------------------------------------
struct DetSelectArgs {
  const u64 *cand;
  long long cand_cap;
  const int *cand_n, *want, *none;
  int w, r2, chunk, acc_stride;
  float *acc_pts, *acc_resp;                  // camera k at rows k * acc_stride
  int *acc_n, *ovf;
};
__global__ __launch_bounds__(DET_THREADS) void k_det_select(DetSelectArgs A) {
  __shared__ u64 s_buf[DET_MAX_POINTS], s_prefix;
  __shared__ volatile int s_ax[DET_MAX_POINTS], s_ay[DET_MAX_POINTS];
  __shared__ float s_ar[DET_MAX_POINTS];
  __shared__ int s_hist[256], s_total, s_all, s_need, s_n, s_acc;
  const int cam = blockIdx.x, t = threadIdx.x, want = min(A.want[cam], DET_MAX_POINTS), K = A.chunk;
  const int listed = A.cand_n[cam], overflow = (long long)listed > A.cand_cap ? 1 : 0;
  const int N = (overflow || want <= 0 || A.none[cam]) ? 0 : listed;
  const u64 *C = A.cand + (size_t)cam * (size_t)A.cand_cap;
  int acc = 0;
  u64 bound = ~0ull;      // the keys below it are still to be walked (no key is all ones: the pixel index is below 2^28)
  while (acc < want && N > 0) {
    // the K-th largest key below the bound, byte by byte from the top
    u64 prefix = 0;
    int need = K, total = 0, all = 0;
    for (int d = 7; d >= 0; d--) {
      s_hist[t] = 0;
      __syncthreads();
      for (int i = t; i < N; i += DET_THREADS) {
        const u64 k = C[i];
        if (k < bound && (d == 7 || (k >> (8 * (d + 1))) == (prefix >> (8 * (d + 1))))) atomicAdd(&s_hist[(int)((k >> (8 * d)) & 255)], 1);
      }
      __syncthreads();
      if (t == 0) {
        if (d == 7) {
          int sum = 0;
          for (int b = 0; b < 256; b++) sum += s_hist[b];
          s_total = sum; s_all = sum <= K ? 1 : 0; s_n = 0;
        }
        if (!s_all) {
          int cum = 0;
          for (int b = 255; b >= 0; b--) {
            if (cum + s_hist[b] >= need) { s_prefix = prefix | ((u64)b << (8 * d)); s_need = need - cum; break; }
            cum += s_hist[b];
          }
        }
      }
      __syncthreads();
      total = s_total; all = s_all;
      if (all) break;
      prefix = s_prefix; need = s_need;
    }
    if (total == 0) break;
    const u64 low = all ? 0 : prefix;
    for (int i = t; i < N; i += DET_THREADS) {
      const u64 k = C[i];
      if (k < bound && k >= low) {      // (K of them, or all: the keys of a camera differ in their index)
        const int s = atomicAdd(&s_n, 1);
        if (s < K) s_buf[s] = k;
      }
    }
    __syncthreads();
    const int take = min(s_n, K);
    for (int i = take + t; i < K; i += DET_THREADS) s_buf[i] = 0;
    __syncthreads();
    lds_bitonic(s_buf, K, true);
    if (t < 64) {
      for (int j = 0; j < take && acc < want; j++) {
        const u64 k = s_buf[j];
        const int idx = det_key_index(k), x = idx % A.w, y = idx / A.w;
        if (wave_hit(s_ax, s_ay, acc, x, y, A.r2, false, t)) continue;
        if (t == 0) { s_ax[acc] = x; s_ay[acc] = y; s_ar[acc] = det_key_response(k); }
        acc++;
        __threadfence_block();
      }
      if (t == 0) s_acc = acc;
    }
    __syncthreads();
    acc = s_acc;
    if (all) break;
    bound = low;
  }
  __syncthreads();
  for (int j = t; j < acc; j += DET_THREADS) {
    const size_t q = (size_t)cam * (size_t)A.acc_stride + (size_t)j;
    A.acc_pts[2 * q] = (float)s_ax[j]; A.acc_pts[2 * q + 1] = (float)s_ay[j]; A.acc_resp[q] = s_ar[j];
  }
  if (t == 0) { A.acc_n[cam] = acc; A.ovf[cam] = overflow; }
}

// ---- G5 and the hand-over ------------------------------------------------------------------------------------------------------------
// the rows of the cameras packed one behind the other, as gfbe_klt_set_points lays them out
__global__ __launch_bounds__(DET_SCAN_THREADS) void k_det_offsets(int n_cam, const int *kept, const int *acc_n, int *seg_begin, int *seg_count, int *off_out) {
  __shared__ int lds[20];
  const int t = threadIdx.x, chunk = (n_cam + DET_SCAN_THREADS - 1) / DET_SCAN_THREADS, b0 = min(n_cam, t * chunk), b1 = min(n_cam, b0 + chunk);
  int mine = 0, total;
  for (int k = b0; k < b1; k++) mine += kept[k] + acc_n[k];
  int run = block_exclusive_scan<DET_SCAN_THREADS>(mine, &total, lds);
  for (int k = b0; k < b1; k++) {
    const int n = kept[k] + acc_n[k];
    seg_begin[k] = run; seg_count[k] = n; off_out[k] = run;
    run += n;
  }
  if (t == 0) off_out[n_cam] = total;
}
struct DetPackArgs {
  const int *seg_begin, *kept, *acc_n, *n_in, *cand_n, *ovf;
  const float *pts_in, *acc_pts;               // the kept rows (camera k at k * cap) and the accepted corners
  const int *ids_in, *cnt_in;
  int cap;
  float *pts_out, *pts_dl;                     // the tracker's half and the staging chunk
  int *ids_out, *cnt_out, *ids_dl, *cnt_dl, *next_id, *counters;
};
__global__ __launch_bounds__(DET_THREADS) void k_det_pack(DetPackArgs A) {
  const int cam = blockIdx.x, t = threadIdx.x, kept = A.kept[cam], added = A.acc_n[cam], nid = A.next_id[cam];
  const size_t in = (size_t)cam * (size_t)A.cap, out = (size_t)A.seg_begin[cam];
  __syncthreads();      // (every thread has read next_id)
  for (int j = t; j < kept + added; j += DET_THREADS) {
    float x, y;
    int id, tc;
    if (j < kept) { x = A.pts_in[2 * (in + j)]; y = A.pts_in[2 * (in + j) + 1]; id = A.ids_in[in + j]; tc = A.cnt_in[in + j]; }
    else { x = A.acc_pts[2 * (in + j - kept)]; y = A.acc_pts[2 * (in + j - kept) + 1]; id = nid + (j - kept); tc = 1; }
    const size_t q = out + (size_t)j;
    A.pts_out[2 * q] = x; A.pts_out[2 * q + 1] = y; A.pts_dl[2 * q] = x; A.pts_dl[2 * q + 1] = y;
    A.ids_out[q] = id; A.ids_dl[q] = id; A.cnt_out[q] = tc; A.cnt_dl[q] = tc;
  }
  if (t == 0) {
    A.next_id[cam] = nid + added;
    int *c = A.counters + 6 * (size_t)cam;
    c[0] = A.n_in[cam]; c[1] = kept; c[2] = A.cand_n[cam]; c[3] = added; c[4] = nid + added; c[5] = A.ovf[cam];
  }
}

// ---- the planes, for tests and diagnosis ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DET_THREADS) void k_det_planes(KltGeom g, const uint8_t *img, int cam, const int *kept, const int *kept_xy, int cap, int r2, float *eig, uint8_t *mask) {
  const int w = g.w[0], h = g.h[0], st = w + 2 * KLT_WIN;
  const long long p = (long long)blockIdx.x * DET_THREADS + threadIdx.x;
  if (p >= (long long)w * h) return;
  const int x = (int)(p % w), y = (int)(p / w);
  const uint8_t *img0 = img + (size_t)cam * (size_t)g.img_cam + (size_t)g.img_off[0] + (size_t)KLT_WIN * (size_t)st + KLT_WIN;
  eig[p] = det_response(img0, st, w, h, x, y);
  bool clear = true;
  const int nk = kept[cam];
  for (int k = 0; k < nk && clear; k++) {
    const size_t q = (size_t)cam * (size_t)cap + (size_t)k;
    clear = det_d2(x, y, kept_xy[2 * q], kept_xy[2 * q + 1]) > r2;
  }
  mask[p] = clear ? 255 : 0;
}

bool det_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
const char *det_options_error(const gfbe_det_options *o) {
  if (o->struct_size != (int32_t)sizeof(gfbe_det_options)) return "gfbe_det_options.struct_size does not match this library (ABI mismatch)";
  if (o->max_cnt < 1) return "max_cnt < 1";
  if (o->min_dist < 0 || o->min_dist > DET_MAX_DIST) return "min_dist outside 0 .. 32768";
  if (o->candidate_capacity < 0) return "candidate_capacity < 0";
  if (!det_pow2(o->sort_chunk) || o->sort_chunk < 64 || o->sort_chunk > DET_MAX_POINTS) return "sort_chunk is no power of two in 64 .. 2048";
  if (!std::isfinite(o->quality) || o->quality < 0.0) return "quality must be finite and >= 0";
  return nullptr;
}

// G2 / G3 of every camera up to the accepted corners: pass 1, the threshold, pass 2, the selection
void det_launch_corners(gfbe_ctx *c, gfbe_det *m, const int *kept, const int *want, int min_dist, double quality, int acc_stride, float *acc_pts, float *acc_resp,
                        int *acc_n) {
  const gfbe_klt *k = m->trk;
  hipStream_t st = ctx_stream(c);
  DetTileArgs T;
  std::memset(&T, 0, sizeof T);
  T.g = k->g; T.img = k->img[k->cur_set]; T.kept = kept; T.want = want; T.kept_xy = m->kept_xy; T.cap = k->cap; T.r2 = min_dist * min_dist; T.min_dist = min_dist;
  T.bmax = m->bmax; T.thr = m->thr; T.none = m->none; T.cand = m->cand; T.cand_cap = m->cand_cap; T.cand_n = m->cand_n;
  const dim3 grid(m->nbx, m->nby, k->n_cam);
  hipLaunchKernelGGL(k_det_tile<1>, grid, dim3(DET_THREADS), 0, st, T);
  hipLaunchKernelGGL(k_det_thresh, dim3(k->n_cam), dim3(DET_THREADS), 0, st, (const float *)m->bmax, m->nbx * m->nby, want, quality, m->thr, m->none);
  hipLaunchKernelGGL(k_det_tile<2>, grid, dim3(DET_THREADS), 0, st, T);
  DetSelectArgs S;
  std::memset(&S, 0, sizeof S);
  S.cand = m->cand; S.cand_cap = m->cand_cap; S.cand_n = m->cand_n; S.want = want; S.none = m->none; S.w = k->cols; S.r2 = min_dist * min_dist; S.chunk = m->opt.sort_chunk;
  S.acc_stride = acc_stride; S.acc_pts = acc_pts; S.acc_resp = acc_resp; S.acc_n = acc_n; S.ovf = m->ovf;
  hipLaunchKernelGGL(k_det_select, dim3(k->n_cam), dim3(DET_THREADS), 0, st, S);
}

}  // namespace

extern "C" {

void gfbe_det_default_options(gfbe_det_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = (int32_t)sizeof *o;
  o->max_cnt = 150; o->min_dist = 30; o->candidate_capacity = 0; o->sort_chunk = 512; o->quality = 0.01;
}

void gfbe_det_destroy(gfbe_ctx *c, gfbe_det *m) {
  if (!m) return;
  m->release(c);
  delete m;
}

gfbe_status gfbe_det_create(gfbe_ctx *c, gfbe_klt *k, const gfbe_det_options *opt, gfbe_det **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  gfbe_det_options o;
  if (opt) o = *opt; else gfbe_det_default_options(&o);
  if (const char *bad = det_options_error(&o)) return handle_bad(c, "gfbe_det_create", bad);
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_det_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (!k) return handle_bad(c, "gfbe_det_create", "tracker NULL");
  if (k->owner != c) return handle_bad(c, "gfbe_det_create", "the tracker belongs to another context");
  if (k->cap > DET_MAX_POINTS) return handle_bad(c, "gfbe_det_create", "the tracker's point_capacity is above GFBE_DET_MAX_POINTS");
  if (o.max_cnt > k->cap) return handle_bad(c, "gfbe_det_create", "max_cnt is above the tracker's point_capacity");
  gfbe_det *m = new gfbe_det();
  CreateGuard<gfbe_det> guard{c, m, gfbe_det_destroy};
  m->owner = c; m->trk = k; m->opt = o; m->mask_min_dist = o.min_dist;
  m->cand_cap = o.candidate_capacity > 0 ? (long long)o.candidate_capacity : (long long)(k->rows - 2) * (long long)(k->cols - 2);
  m->nbx = (k->cols + DET_TW - 1) / DET_TW; m->nby = (k->rows + DET_TH - 1) / DET_TH;
  hipStream_t st = ctx_stream(c);
  const size_t C = (size_t)k->n_cam, N = C * (size_t)k->cap;
  const bool ok = m->alloc(&m->kept_xy, 2 * N) && m->alloc(&m->kept, C) && m->alloc(&m->want, C) && m->alloc(&m->n_in, C) && m->alloc(&m->next_id, C) && m->alloc(&m->cand_n, C) &&
                  m->alloc(&m->acc_n, C) && m->alloc(&m->ovf, C) && m->alloc(&m->none, C) && m->alloc(&m->zero, C) && m->alloc(&m->bmax, C * (size_t)m->nbx * (size_t)m->nby) &&
                  m->alloc(&m->thr, C) && m->alloc(&m->cand, C * (size_t)m->cand_cap) && m->alloc(&m->acc_pts, 2 * N) && m->alloc(&m->acc_resp, N);
  if (!ok) { ctx_set_error(c, "gfbe_det_create: device allocation failed"); return GFBE_DEVICE_ERROR; }
  GFBE_CHECK(c, hipStreamSynchronize(st));
  guard.armed = false;
  *out = m;
  return GFBE_OK;
}

gfbe_status gfbe_det_set_next_id(gfbe_ctx *c, gfbe_det *m, const int32_t *next_id) {
  gfbe_status rc = handle_ready(c, m, "gfbe_det_set_next_id");
  if (rc != GFBE_OK) return rc;
  if (!next_id) return handle_bad(c, "gfbe_det_set_next_id", "next_id NULL");
  const size_t C = (size_t)m->trk->n_cam;
  Staged sg(c, m->trk, C * 4 + 4096);
  const int32_t *d = sg.up(next_id, C);
  if (!sg.ok) { ctx_set_error(c, "gfbe_det_set_next_id: staging allocation failed"); return GFBE_DEVICE_ERROR; }
  sg.flush();
  GFBE_CHECK(c, hipMemcpyAsync(m->next_id, d, sizeof(int) * C, hipMemcpyDeviceToDevice, ctx_stream(c)));
  sg.finish();
  return GFBE_OK;
}

gfbe_status gfbe_det_detect(gfbe_ctx *c, gfbe_det *m, int32_t *offset_out, float *pts, int32_t *ids, int32_t *track_cnt, int32_t *counters) {
  gfbe_status rc = handle_ready(c, m, "gfbe_det_detect");
  if (rc != GFBE_OK) return rc;
  gfbe_klt *k = m->trk;
  if (k->n_pushed < 1) return handle_bad(c, "gfbe_det_detect", "no image has been pushed");
  const size_t C = (size_t)k->n_cam;
  size_t room = 0;      // rows of the result at most
  for (size_t q = 0; q < C; q++) room += (size_t)std::max(k->count_h[q], (int)m->opt.max_cnt);
  hipStream_t st = ctx_stream(c);
  const int hf = k->half, nh = hf ^ 1;
  {
    Staged sg(c, k, room * 16 + C * 28 + 8192);
    int *o_off = sg.up((const int *)nullptr, C + 1), *o_cnts = sg.up((const int *)nullptr, 6 * C), *o_ids = sg.up((const int *)nullptr, room),
        *o_cnt = sg.up((const int *)nullptr, room);
    float *o_pts = sg.up((const float *)nullptr, 2 * room);
    if (!sg.ok) { ctx_set_error(c, "gfbe_det_detect: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    DetMaskArgs M;
    std::memset(&M, 0, sizeof M);
    M.seg_begin = k->seg_begin; M.count_in = k->seg_count[hf]; M.pts_in = k->pts[hf]; M.ids_in = k->ids[hf]; M.cnt_in = k->cnt[hf];
    M.pts_out = k->pts[nh]; M.ids_out = k->ids[nh]; M.cnt_out = k->cnt[nh];
    M.kept_xy = m->kept_xy; M.kept = m->kept; M.want = m->want; M.n_in = m->n_in; M.cand_n = m->cand_n; M.acc_n = m->acc_n;
    M.cap = k->cap; M.w = k->cols; M.h = k->rows; M.r2 = m->opt.min_dist * m->opt.min_dist; M.max_cnt = m->opt.max_cnt;
    hipLaunchKernelGGL(k_det_mask, dim3(k->n_cam), dim3(DET_THREADS), 0, st, M);
    det_launch_corners(c, m, m->kept, m->want, m->opt.min_dist, m->opt.quality, k->cap, m->acc_pts, m->acc_resp, m->acc_n);
    hipLaunchKernelGGL(k_det_offsets, dim3(1), dim3(DET_SCAN_THREADS), 0, st, k->n_cam, (const int *)m->kept, (const int *)m->acc_n, k->seg_begin, k->seg_count[hf], o_off);
    DetPackArgs P;
    std::memset(&P, 0, sizeof P);
    P.seg_begin = k->seg_begin; P.kept = m->kept; P.acc_n = m->acc_n; P.n_in = m->n_in; P.cand_n = m->cand_n; P.ovf = m->ovf;
    P.pts_in = k->pts[nh]; P.acc_pts = m->acc_pts; P.ids_in = k->ids[nh]; P.cnt_in = k->cnt[nh]; P.cap = k->cap;
    P.pts_out = k->pts[hf]; P.ids_out = k->ids[hf]; P.cnt_out = k->cnt[hf]; P.pts_dl = o_pts; P.ids_dl = o_ids; P.cnt_dl = o_cnt;
    P.next_id = m->next_id; P.counters = o_cnts;
    hipLaunchKernelGGL(k_det_pack, dim3(k->n_cam), dim3(DET_THREADS), 0, st, P);
    m->mask_min_dist = m->opt.min_dist;
    sg.dlo = (size_t)((const char *)o_off - sg.bd); sg.dhi = (size_t)((const char *)(o_pts + 2 * room) - sg.bd);
    sg.finish();      // the one wait
    GFBE_CHECK(c, hipGetLastError());
    auto host = [&](const auto *d) { return (decltype(d))(sg.bh + ((const char *)d - sg.bd)); };
    const int *h_off = host(o_off);
    const size_t n = (size_t)h_off[C];
    for (size_t q = 0; q < C; q++) { k->begin_h[q] = h_off[q]; k->count_h[q] = h_off[q + 1] - h_off[q]; }
    if (offset_out) std::memcpy(offset_out, h_off, sizeof(int32_t) * (C + 1));
    if (pts) std::memcpy(pts, host(o_pts), sizeof(float) * 2 * n);
    if (ids) std::memcpy(ids, host(o_ids), sizeof(int32_t) * n);
    if (track_cnt) std::memcpy(track_cnt, host(o_cnt), sizeof(int32_t) * n);
    if (counters) std::memcpy(counters, host(o_cnts), sizeof(int32_t) * 6 * C);
  }
  return GFBE_OK;
}

gfbe_status gfbe_det_corners(gfbe_ctx *c, gfbe_det *m, int32_t max_corners, double quality, int32_t min_dist, int32_t *offset_out, float *pts, float *response) {
  gfbe_status rc = handle_ready(c, m, "gfbe_det_corners");
  if (rc != GFBE_OK) return rc;
  gfbe_klt *k = m->trk;
  if (k->n_pushed < 1) return handle_bad(c, "gfbe_det_corners", "no image has been pushed");
  if (max_corners <= 0 || max_corners > DET_MAX_POINTS) return handle_bad(c, "gfbe_det_corners", "max_corners outside 1 .. GFBE_DET_MAX_POINTS");
  if (!std::isfinite(quality) || quality < 0.0 || min_dist < 0 || min_dist > DET_MAX_DIST) return handle_bad(c, "gfbe_det_corners", "quality negative or not finite, or min_dist outside 0 .. 32768");
  const size_t C = (size_t)k->n_cam, R = C * (size_t)max_corners;
  hipStream_t st = ctx_stream(c);
  {
    Staged sg(c, k, R * 12 + C * 8 + 8192);
    const std::vector<int> want(C, (int)max_corners);
    const int *d_want = sg.up(want.data(), C);
    int *o_n = sg.up((const int *)nullptr, C);
    float *o_resp = sg.up((const float *)nullptr, R), *o_pts = sg.up((const float *)nullptr, 2 * R);
    if (!sg.ok) { ctx_set_error(c, "gfbe_det_corners: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    GFBE_CHECK(c, hipMemsetAsync(m->cand_n, 0, sizeof(int) * C, st));
    det_launch_corners(c, m, m->zero, d_want, min_dist, quality, max_corners, o_pts, o_resp, o_n);
    sg.dlo = (size_t)((const char *)o_n - sg.bd); sg.dhi = (size_t)((const char *)(o_pts + 2 * R) - sg.bd);
    sg.finish();
    GFBE_CHECK(c, hipGetLastError());
    auto host = [&](const auto *d) { return (decltype(d))(sg.bh + ((const char *)d - sg.bd)); };
    const int *h_n = host(o_n);
    const float *h_pts = host(o_pts), *h_resp = host(o_resp);
    size_t row = 0;
    for (size_t q = 0; q < C; q++) {
      const size_t n = (size_t)h_n[q];
      if (offset_out) offset_out[q] = (int32_t)row;
      if (pts) std::memcpy(pts + 2 * row, h_pts + 2 * q * (size_t)max_corners, sizeof(float) * 2 * n);
      if (response) std::memcpy(response + row, h_resp + q * (size_t)max_corners, sizeof(float) * n);
      row += n;
    }
    if (offset_out) offset_out[C] = (int32_t)row;
  }
  return GFBE_OK;
}

gfbe_status gfbe_det_download(gfbe_ctx *c, gfbe_det *m, int32_t camera, float *eig_out, uint8_t *mask_out) {
  gfbe_status rc = handle_ready(c, m, "gfbe_det_download");
  if (rc != GFBE_OK) return rc;
  gfbe_klt *k = m->trk;
  if (k->n_pushed < 1) return handle_bad(c, "gfbe_det_download", "no image has been pushed");
  if (camera < 0 || camera >= k->n_cam) return handle_bad(c, "gfbe_det_download", "camera outside the handle's");
  const size_t px = (size_t)k->rows * (size_t)k->cols;
  {
    Staged sg(c, k, px * 5 + 8192);
    float *d_eig = sg.up((const float *)nullptr, px);
    uint8_t *d_mask = sg.up((const uint8_t *)nullptr, px);
    if (!sg.ok) { ctx_set_error(c, "gfbe_det_download: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    hipLaunchKernelGGL(k_det_planes, dim3((unsigned)((px + DET_THREADS - 1) / DET_THREADS)), dim3(DET_THREADS), 0, ctx_stream(c), k->g, (const uint8_t *)k->img[k->cur_set],
                       (int)camera, (const int *)m->kept, (const int *)m->kept_xy, k->cap, m->mask_min_dist * m->mask_min_dist, d_eig, d_mask);
    sg.down(eig_out, (const float *)d_eig, px);
    sg.down(mask_out, (const uint8_t *)d_mask, px);
    sg.finish();
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

}  // extern "C"
