// gfbe_lio.hip — LiDAR point-to-plane factors on the device (BASELINE configs[4]).
//
//   LidarPlaneNormFactor::Evaluate     lio/src/liw/lidarFactor.cpp:18-51
//   CTLidarPlaneNormFactor::Evaluate   lio/src/liw/lidarFactor.cpp:59-120 (the reference's approximate slerp Jacobians are
//                                      reproduced as they are: tests/test_lio_oracle.py quantifies them)
//
// One thread per residual evaluates r and the 1 x 6 / 1 x 12 tangent Jacobian; a workgroup accumulates its J^T J, J^T r and
// cost in registers (thread-strided), reduces them in a fixed order (64-lane shuffles, then its waves through LDS) and writes
// one partial per workgroup; the host adds the partials in workgroup order. Thousands of identical tiny residuals on one or
// two poses: bandwidth- and latency-shaped, no MFMA ("genuinely bandwidth-shaped").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"
#include "gfbe_lio_pose.h"

using namespace gfd;

namespace {

constexpr int LIO_THREADS = 256;
constexpr int LIO_ZERO_COPY_N = 8192;     // gfbe_lio_linearize: scans up to this many residuals are read from / written to pinned host memory by the kernel itself
constexpr int LIO_PART = 12 * 13 / 2 + 12 + 1;   // lower triangle of J^T J (78) + J^T r (12) + cost

template <int CT>
__global__ __launch_bounds__(LIO_THREADS) void k_lio(int n, const double *pts, const double *normals, const double *offsets, const double *alpha,
                                                     const double *weights, double sqrt_info, const double *pb, const double *pe, double *r_out,
                                                     double *J_out, double *part) {
  constexpr int DN = CT ? 12 : 6;
  const int t = threadIdx.x;
  double acc[LIO_PART];
#pragma unroll
  for (int q = 0; q < LIO_PART; q++) acc[q] = 0.0;
  const Qx qb = {pb[3], pb[4], pb[5], pb[6]};
  const Qx qe = {pe[3], pe[4], pe[5], pe[6]};
  for (int k = blockIdx.x * LIO_THREADS + t; k < n; k += gridDim.x * LIO_THREADS) {
    const double *p = pts + 3 * (size_t)k, *nv = normals + 3 * (size_t)k;
    const double wgt = weights[k];
    double Jk[DN], rk, al = 0.0;
    if (CT) al = alpha[k];
    lio_row<CT>(p, nv, offsets[k], wgt, al, sqrt_info, qb, qe, pb, pe, Jk, &rk);
    if (r_out) r_out[k] = rk;
    if (J_out) for (int a = 0; a < DN; a++) J_out[(size_t)DN * k + a] = Jk[a];
    int e = 0;
#pragma unroll
    for (int a = 0; a < DN; a++)
#pragma unroll
      for (int b = 0; b <= a; b++) acc[e++] += Jk[a] * Jk[b];
#pragma unroll
    for (int a = 0; a < DN; a++) acc[78 + a] += Jk[a] * rk;
    acc[90] += 0.5 * rk * rk;
  }
  // fixed-order reduction: 64-lane butterflies, then the waves through LDS
  __shared__ double red[LIO_THREADS / 64][LIO_PART];
#pragma unroll
  for (int q = 0; q < LIO_PART; q++) {
    double v = acc[q];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((t & 63) == 0) red[t >> 6][q] = v;
  }
  __syncthreads();
  if (t < LIO_PART) {
    double v = 0.0;
    for (int wv = 0; wv < LIO_THREADS / 64; wv++) v += red[wv][t];
    part[(size_t)blockIdx.x * LIO_PART + t] = v;
  }
}

}  // namespace

// dev_in: the five residual arrays (pts, normals, offsets, alpha, weights) already on the device (gfbe_vmap_linearize: the
// association held on a voxel map handle); only the two poses are staged then. Same grid, same kernel, same host sum as the host-fed call.
static gfbe_status lio_run(gfbe_ctx *c, int32_t ct, int32_t n, const double *pts, const double *normals, const double *offsets, const double *alpha,
                           const double *weights, bool dev_in, double sqrt_info, const double *pose_begin, const double *pose_end, double *r, double *J,
                           double *H, double *g, double *cost) {
  const int dn = ct ? 12 : 6;
  hipStream_t s = ctx_stream(c);
  // One host-to-device copy in, one device-to-host copy out, through the context's scratch and its pinned mirror (round 5: the call
  // made ten allocations and ten copies — 0.14 ms for a 2 000-point scan, which one CPU core evaluates in 0.06 ms):
  //   in  : pts [3 n] | normals [3 n] | offsets [n] | alpha [n] | weights [n] | pose_begin [7] | pose_end [7] (+ 2 of padding)
  //   out : partial sums [G][LIO_PART] | r [n] | J [n][dn]      (r, J only when asked for)
  const int G = std::max(1, std::min(256, (n + LIO_THREADS - 1) / LIO_THREADS));
  const size_t nn = (size_t)std::max(n, 1), arr_d = dev_in ? 0 : 9 * nn;
  const size_t in_d = arr_d + 16, out_d = (size_t)G * LIO_PART + (r ? nn : 0) + (J ? (size_t)dn * nn : 0);
  double *dev = (double *)ctx_scratch(c, sizeof(double) * (in_d + out_d));
  double *pin = (double *)ctx_scratch_pinned(c, sizeof(double) * (in_d + out_d));
  if (!dev || !pin) { ctx_set_error(c, dev_in ? "gfbe_vmap_linearize: device / pinned allocation failed" : "gfbe_lio_linearize: device / pinned allocation failed"); return GFBE_DEVICE_ERROR; }
  double *hp = pin, *hn = hp + 3 * nn, *ho = hn + 3 * nn, *ha = ho + nn, *hw = ha + nn, *hb = pin + arr_d, *he = hb + 8;
  if (n > 0 && !dev_in) {
    std::memcpy(hp, pts, sizeof(double) * 3 * n); std::memcpy(hn, normals, sizeof(double) * 3 * n); std::memcpy(ho, offsets, sizeof(double) * n);
    if (ct) std::memcpy(ha, alpha, sizeof(double) * n); else std::memset(ha, 0, sizeof(double) * n);
    if (weights) std::memcpy(hw, weights, sizeof(double) * n); else std::fill(hw, hw + n, 1.0);
  }
  std::memcpy(hb, pose_begin, sizeof(double) * 7); std::memcpy(he, pose_end ? pose_end : pose_begin, sizeof(double) * 7);
  const double *dp = dev, *dnv = dp + 3 * nn, *doff = dnv + 3 * nn, *dal = doff + nn, *dw = dal + nn, *dpb = dev + arr_d, *dpe = dpb + 8;
  double *dpart = dev + in_d, *dr = dpart + (size_t)G * LIO_PART, *dJ = dr + (r ? nn : 0);
  gfbe_status st = GFBE_OK;
  // A scan of the reference's size (lidarodom.cpp:929-1071 produces ~2 000 residuals per ICP iteration) is three dependent latencies —
  // copy in, launch, copy out — around 10 us of arithmetic: 0.055 ms, where one CPU core takes 0.044. Round 6: up to
  // LIO_ZERO_COPY_N residuals the kernel reads the pinned staging buffer across PCIe itself and writes its partial sums (and r, J) into
  // it — ONE launch and the wait for it, no copy command (the k_ingest_small pattern of gfbe_solve_window); larger scans keep the two DMA
  // copies, which stream faster than a kernel's loads across the bus.
  const bool zero_copy = n <= LIO_ZERO_COPY_N;
  if (zero_copy) {
    dp = pin; dnv = dp + 3 * nn; doff = dnv + 3 * nn; dal = doff + nn; dw = dal + nn; dpb = pin + arr_d; dpe = dpb + 8;
    dpart = pin + in_d; dr = dpart + (size_t)G * LIO_PART; dJ = dr + (r ? nn : 0);
  } else if (hipMemcpyAsync(dev, pin, sizeof(double) * in_d, hipMemcpyHostToDevice, s) != hipSuccess) st = GFBE_DEVICE_ERROR;
  if (dev_in) { dp = pts; dnv = normals; doff = offsets; dal = alpha; dw = weights; }
  if (st == GFBE_OK) {
    if (ct) hipLaunchKernelGGL(k_lio<1>, dim3(G), dim3(LIO_THREADS), 0, s, n, dp, dnv, doff, dal, dw, sqrt_info, dpb, dpe, r ? dr : nullptr, J ? dJ : nullptr, dpart);
    else hipLaunchKernelGGL(k_lio<0>, dim3(G), dim3(LIO_THREADS), 0, s, n, dp, dnv, doff, dal, dw, sqrt_info, dpb, dpe, r ? dr : nullptr, J ? dJ : nullptr, dpart);
    double *hout = pin + in_d;
    if (!zero_copy && hipMemcpyAsync(hout, dpart, sizeof(double) * out_d, hipMemcpyDeviceToHost, s) != hipSuccess) st = GFBE_DEVICE_ERROR;
    if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) st = GFBE_DEVICE_ERROR;
    if (st == GFBE_OK) {
      double tot[LIO_PART] = {0};
      for (int b = 0; b < G; b++) for (int q = 0; q < LIO_PART; q++) tot[q] += hout[(size_t)b * LIO_PART + q];   // workgroup order
      if (H) { int e = 0; for (int a = 0; a < dn; a++) for (int b = 0; b <= a; b++, e++) { H[a * dn + b] = tot[e]; H[b * dn + a] = tot[e]; } }
      if (g) for (int a = 0; a < dn; a++) g[a] = tot[78 + a];
      if (cost) *cost = tot[90];
      const double *hr = hout + (size_t)G * LIO_PART, *hJ = hr + (r ? nn : 0);
      if (r && n) std::memcpy(r, hr, sizeof(double) * n);
      if (J && n) std::memcpy(J, hJ, sizeof(double) * dn * n);
    }
  }
  if (st != GFBE_OK) ctx_set_error(c, dev_in ? "gfbe_vmap_linearize: copy / launch failed" : "gfbe_lio_linearize: copy / launch failed");
  return st;
}

extern "C" gfbe_status gfbe_lio_linearize(gfbe_ctx *c, int32_t ct, int32_t n, const double *pts, const double *normals, const double *offsets,
                                          const double *alpha, const double *weights, double sqrt_info, const double *pose_begin,
                                          const double *pose_end, double *r, double *J, double *H, double *g, double *cost) {
  if (!c || n < 0 || !pose_begin || (n > 0 && (!pts || !normals || !offsets)) || (ct && (!alpha || !pose_end))) return GFBE_BAD_INPUT;
  if (ctx_device(c) < 0) return GFBE_NO_DEVICE;
  return lio_run(c, ct, n, pts, normals, offsets, alpha, weights, false, sqrt_info, pose_begin, pose_end, r, J, H, g, cost);
}

namespace gfd {
gfbe_status lio_linearize_device(gfbe_ctx *c, int32_t ct, int32_t n, const double *pts, const double *normals, const double *offsets, const double *alpha,
                                 const double *weights, double sqrt_info, const double *pose_begin, const double *pose_end, double *r, double *J,
                                 double *H, double *g, double *cost) {
  return lio_run(c, ct, n, pts, normals, offsets, alpha, weights, true, sqrt_info, pose_begin, pose_end, r, J, H, g, cost);
}
}  // namespace gfd
