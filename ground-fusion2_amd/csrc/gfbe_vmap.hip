// gfbe_vmap.hip — device-resident voxel map of the LiDAR odometry and the association of a scan against it: what produces the
// (point, normal, offset, weight) rows of gfbe_lio_linearize without a trip through host memory.
//
//   map_incremental / addPointToMap      lio/src/liw/lio/lidarodom.cpp:1167-1266   gfbe_vmap_add_points
//   lasermap_fov_segment                 :1268-1284                                gfbe_vmap_erase_far
//   addSurfCostFactor (loop body)        :929-1071                                 gfbe_vmap_associate
//     searchNeighbors :1086-1165, computeNeighborhoodDistribution :887-927
//   checkLocalizability                  :811-885                                  gfbe_vmap_localizability
//
// Layout: an open-addressing table (linear probing) of 2^k >= 2 voxel_capacity slots; a slot holds the packed key (VM_EMPTY when
// free), the point count and max_num_points_in_voxel points in insertion order. There are no tombstones: erase_far re-inserts the
// surviving voxels into the other half of a ping-pong pair, so a probe sequence ends at the first free slot and the table never fills
// (live voxels <= capacity <= slots / 2). The only atomic of the kernels in this file is the compare-and-swap that claims a slot (the
// library radix sort of add_points has its own inside; it is stable, its output does not depend on them); every count is a block scan.
// Nothing observable depends on the slot a voxel landed in: downloads are sorted by key, the association walks voxels by key.
//
// add_points: key per point -> stable radix sort of (key, input index) -> one lane per run of equal keys walks its points in input
// order against its voxel (the sequential rule of addPointToMap; voxels are independent of each other).
// associate: one wave per keypoint. Lanes look up the (2v + 1)^3 voxels, stream their points 64 at a time and merge them into the
// running list of the k nearest by rank counting on (distance, visit index) — deterministic, no queue; then the 20-point moments,
// a cyclic Jacobi in registers, flip, weight and the plane-distance filter. A single-workgroup scan compacts the residuals in
// keypoint order and cuts them at max_num_residuals. FP64 throughout; 3 x 3 blocks leave the matrix cores nothing to do.
#include <hip/hip_runtime.h>
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"
#include "gfbe_line_batch.h"      // grow()
#include "gfbe_lio_pose.h"
#include "gfbe_handle.h"
#include "gfbe_vmap.h"
#include "gfbe_vmap_impl.h"

using namespace gfd;

namespace {

constexpr int VM_THREADS = 1024;

__global__ __launch_bounds__(256) void k_vm_keys(int n, const double *pts, double size, unsigned long long *key, int *idx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint64_t k;
  key[i] = vmap_key(pts + 3 * (size_t)i, size, &k) ? k : VM_INVALID;
  idx[i] = i;
}
// the world point of every scan point at its pose (transformKeypoints)
__global__ __launch_bounds__(256) void k_vm_world(int n, int ct, const double *raw, const double *alpha, const double *pb, const double *pe, double *out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  lio_world_store(i, ct, raw, alpha, pb, pe, out);
}
// per sorted position: an out-of-range point; the head of a run whose voxel would be created
__global__ __launch_bounds__(256) void k_vm_probe(VmDev V, int n, const unsigned long long *skey, int min_num_points, int *isnew, int *skip) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const unsigned long long key = skey[j];
  const bool head = key != VM_INVALID && (j == 0 || skey[j - 1] != key);
  skip[j] = key == VM_INVALID;
  isnew[j] = head && min_num_points <= 0 && vm_find(V, key) < 0;
}
__device__ __forceinline__ int vm_block_sum(const int *a, int n, int *lds) {
  int mine = 0, total;
  for (int i = threadIdx.x; i < n; i += VM_THREADS) mine += a[i];
  (void)block_exclusive_scan<VM_THREADS>(mine, &total, lds);
  return total;
}
// the capacity rule: an add that would pass voxel_capacity changes nothing and raises the sticky flag
__global__ __launch_bounds__(VM_THREADS) void k_vm_admit(VmDev V, int n, const int *isnew, const int *skip) {
  __shared__ int lds[20];
  const int fresh = vm_block_sum(isnew, n, lds), skipped = vm_block_sum(skip, n, lds);
  if (threadIdx.x == 0) {
    V.meta[M_SKIP] += skipped;
    if (V.meta[M_VOX] + fresh > V.cap) { V.meta[M_OVER] = 1; V.meta[M_GO] = 0; }
    else { V.meta[M_GO] = 1; V.meta[M_VOX] += fresh; }
  }
}
// addPointToMap for the points of one voxel, in input order (one lane per run of equal keys)
__global__ __launch_bounds__(256) void k_vm_insert(VmDev V, int n, const unsigned long long *skey, const int *sidx, const double *in, double size,
                                                   double min_dist, int min_num_points, int *added) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  added[j] = 0;
  if (!V.meta[M_GO]) return;
  const unsigned long long key = skey[j];
  if (key == VM_INVALID || (j > 0 && skey[j - 1] == key)) return;
  bool fresh = false;
  const int slot = min_num_points <= 0 ? vm_claim(V, key, &fresh) : vm_find(V, key);
  if (slot < 0) return;      // (min_num_points > 0: no voxel is created)
  double *vp = V.pts + (size_t)slot * V.P * 3;
  int c = fresh ? 0 : V.cnt[slot], add = 0;
  const double md2 = min_dist * min_dist;
  for (int jj = j; jj < n && skey[jj] == key && c < V.P; jj++) {
    const double *p = in + 3 * (size_t)sidx[jj];
    bool take = c == 0;        // a new voxel takes its first point unconditionally
    if (!take) {
      double sq_min = 10 * size * size;
      for (int i = 0; i < c; i++) { const double sq = vmap_sqdist(vp + 3 * i, p); if (sq < sq_min) sq_min = sq; }
      take = sq_min > md2 && (min_num_points <= 0 || c >= min_num_points);
    }
    if (take) { vp[3 * c] = p[0]; vp[3 * c + 1] = p[1]; vp[3 * c + 2] = p[2]; c++; add++; }
  }
  V.cnt[slot] = c;
  added[j] = add;
}
__global__ __launch_bounds__(VM_THREADS) void k_vm_added(VmDev V, int n, const int *added) {
  __shared__ int lds[20];
  const int total = vm_block_sum(added, n, lds);
  if (threadIdx.x == 0) V.meta[M_PTS] += total;
}

// lasermap_fov_segment: the voxels whose FIRST point is within max_distance of `loc` move to the other half
__global__ __launch_bounds__(256) void k_vm_rehash(VmDev O, VmDev N, const double *loc, double max_d2, int *part) {
  __shared__ int lds[20];
  const int s = blockIdx.x * 256 + threadIdx.x;
  int vox = 0, npts = 0;
  if (s <= O.mask && O.keys[s] != VM_EMPTY) {
    const double *src = O.pts + (size_t)s * O.P * 3;
    if (!(vmap_sqdist(src, loc) > max_d2)) {
      bool fresh;
      const int d = vm_claim(N, O.keys[s], &fresh);
      if (d >= 0) {
        const int c = O.cnt[s];
        double *dst = N.pts + (size_t)d * N.P * 3;
        for (int i = 0; i < 3 * c; i++) dst[i] = src[i];
        N.cnt[d] = c;
        vox = 1; npts = c;
      }
    }
  }
  int tv, tp;
  (void)block_exclusive_scan<256>(vox, &tv, lds);
  (void)block_exclusive_scan<256>(npts, &tp, lds);
  if (threadIdx.x == 0) { part[blockIdx.x] = tv; part[gridDim.x + blockIdx.x] = tp; }
}
__global__ __launch_bounds__(VM_THREADS) void k_vm_recount(VmDev V, int nb, const int *part) {
  __shared__ int lds[20];
  const int tv = vm_block_sum(part, nb, lds), tp = vm_block_sum(part + nb, nb, lds);
  if (threadIdx.x == 0) { V.meta[M_VOX] = tv; V.meta[M_PTS] = tp; }
}

// download / upload: voxels in ascending key order, points concatenated
__global__ __launch_bounds__(256) void k_vm_gather(VmDev V, int nv, const int *slot, const int *off, double *out) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const double *src = V.pts + (size_t)slot[v] * V.P * 3;
  double *dst = out + 3 * (size_t)off[v];
  const int c = off[v + 1] - off[v];
  for (int i = 0; i < 3 * c; i++) dst[i] = src[i];
}
__global__ __launch_bounds__(256) void k_vm_scatter(VmDev V, int nv, const unsigned long long *key, const int *off, const double *in) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  bool fresh;
  const int d = vm_claim(V, key[v], &fresh);
  if (d < 0) return;
  const int c = off[v + 1] - off[v];
  double *dst = V.pts + (size_t)d * V.P * 3;
  const double *src = in + 3 * (size_t)off[v];
  for (int i = 0; i < 3 * c; i++) dst[i] = src[i];
  V.cnt[d] = c;
  if (v == 0) { V.meta[M_VOX] = nv; V.meta[M_PTS] = off[nv]; }
}

// ---- association: one wave (= one workgroup of 64) per keypoint
struct AssocArgs {
  int n, ct, v, thr, K, min_nn, ncn;
  double size, max_plane, power, w_alpha, w_nb;
  const double *raw, *alpha, *pb, *pe;
  int *kp_cnt;               // [n] neighbours found
  unsigned int *kp_mask;     // [n] bit i: neighbour i gives a residual
  int *kp_nan;               // [n] dropped for a NaN a2D
  int *kp_vis;               // [n][K] visit index of the neighbours in the (voxel, point) order of the search, -1 behind the last
  double *kp_a2d, *kp_nrm, *kp_w, *kp_pt, *kp_off;     // [n], [n][3], [n], [n][3], [n][ncn]
  const int *skip;           // device flag (or NULL): non-zero = k_vm_assoc / k_vm_compact return at once (the registration loop has ended)
};
__global__ __launch_bounds__(64) void k_vm_assoc(VmDev V, AssocArgs A) {
  const int kp = blockIdx.x, lane = threadIdx.x;
  if (A.skip && *A.skip) return;      // (grid-uniform)
  __shared__ int s_slot[125], s_off[126];
  __shared__ double s_bd[VM_MAXP], s_nd[64];
  __shared__ int s_bc[VM_MAXP], s_br[VM_MAXP], s_nr[64];
  __shared__ double s_nb[3 * VM_MAXP];
  const double *raw = A.raw + 3 * (size_t)kp;
  const double al = A.ct ? A.alpha[kp] : 0.0;
  const Qx qb = {A.pb[3], A.pb[4], A.pb[5], A.pb[6]}, qe = {A.pe[3], A.pe[4], A.pe[5], A.pe[6]};
  double R[9], pw[3];
  lio_world_point(A.ct, qb, qe, A.pb, A.pe, al, raw, R, pw);
  if (lane == 0) { A.kp_cnt[kp] = 0; A.kp_mask[kp] = 0u; A.kp_nan[kp] = 0; A.kp_a2d[kp] = 0.0; }
  if (lane < A.K) A.kp_vis[(size_t)kp * A.K + lane] = -1;
  int kx, ky, kz;
  if (!vmap_axis_key(pw[0], A.size, &kx) || !vmap_axis_key(pw[1], A.size, &ky) || !vmap_axis_key(pw[2], A.size, &kz)) return;   // (wave-uniform)
  // the voxels in the reference's kxx, kyy, kzz order; below the occupancy threshold: skipped
  const int side = 2 * A.v + 1, nvox = side * side * side;
  for (int l = lane; l < nvox; l += 64) {
    const int x = kx - A.v + l / (side * side), y = ky - A.v + (l / side) % side, z = kz - A.v + l % side;
    int slot = -1, c = 0;
    if (abs(x) <= 32767 && abs(y) <= 32767 && abs(z) <= 32767) slot = vm_find(V, vmap_pack(x, y, z));
    if (slot >= 0) c = V.cnt[slot];
    if (c < A.thr) c = 0;
    s_slot[l] = slot; s_off[l + 1] = c;
  }
  __syncthreads();
  if (lane == 0) { int run = 0; s_off[0] = 0; for (int l = 0; l < nvox; l++) { run += s_off[l + 1]; s_off[l + 1] = run; } }
  __syncthreads();
  const int C = s_off[nvox];
  // the K nearest by (distance, visit index): 64 candidates at a time merged into the sorted list by rank counting
  int nb = 0;
  for (int base = 0; base < C; base += 64) {
    const int c = base + lane;
    double d = INFINITY;
    int ref = 0;
    if (c < C) {
      int lo = 0, hi = nvox - 1;      // the voxel of candidate c: the last l with s_off[l] <= c
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_off[mid] <= c) lo = mid; else hi = mid - 1; }
      ref = s_slot[lo] * V.P + (c - s_off[lo]);
      d = sqrt(vmap_sqdist(V.pts + 3 * (size_t)ref, pw));
    }
    s_nd[lane] = d; s_nr[lane] = ref;
    __syncthreads();
    const int m = min(64, C - base);
    int rn = 0, ro = 0;
    for (int j = 0; j < nb; j++) rn += s_bd[j] <= d;                       // (an equal distance met earlier stays in front)
    for (int j = 0; j < m; j++) rn += s_nd[j] < d || (s_nd[j] == d && j < lane);
    const double od = lane < nb ? s_bd[lane] : 0.0;
    const int oc = lane < nb ? s_bc[lane] : 0, orf = lane < nb ? s_br[lane] : 0;
    if (lane < nb) { ro = lane; for (int j = 0; j < m; j++) ro += s_nd[j] < od; }
    __syncthreads();
    if (lane < nb && ro < A.K) { s_bd[ro] = od; s_bc[ro] = oc; s_br[ro] = orf; }
    if (c < C && rn < A.K) { s_bd[rn] = d; s_bc[rn] = c; s_br[rn] = ref; }
    __syncthreads();
    nb = min(A.K, nb + m);
  }
  if (lane == 0) A.kp_cnt[kp] = nb;
  if (lane < nb) A.kp_vis[(size_t)kp * A.K + lane] = s_bc[lane];      // (neighbour identities: a diagnostic output)
  if (nb < A.min_nn || nb == 0) return;
  for (int q = lane; q < 3 * nb; q += 64) s_nb[q] = V.pts[3 * (size_t)s_br[q / 3] + q % 3];
  __syncthreads();
  // every lane forms the same moments, eigenvector and weight (no divergence); lane 0 writes
  double bary[3], cov[6], nrm[3];
  vmap_moments(s_nb, nb, bary, cov);
  const double a2d = vmap_normal_a2d(cov, nrm);
  if (a2d != a2d) { if (lane == 0) A.kp_nan[kp] = 1; return; }      // (the reference throws)
  // towards translation_begin, seen from location = the raw point (the reference's TIL_ is the identity)
  if (nrm[0] * (A.pb[0] - raw[0]) + nrm[1] * (A.pb[1] - raw[1]) + nrm[2] * (A.pb[2] - raw[2]) < 0) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
  const double w = vmap_weight(a2d, s_bd[0], A.w_alpha, A.w_nb, A.power, A.max_plane, A.min_nn);
  const double nn = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
  const double nv[3] = {nrm[0] / nn, nrm[1] / nn, nrm[2] / nn};
  if (lane != 0) return;
  unsigned int mask = 0u;
  for (int i = 0; i < A.ncn && i < nb; i++) {
    const double *q = s_nb + 3 * i;
    const double dist = fabs((pw[0] - q[0]) * nrm[0] + (pw[1] - q[1]) * nrm[1] + (pw[2] - q[2]) * nrm[2]);
    if (dist >= A.max_plane) continue;
    mask |= 1u << i;
    A.kp_off[(size_t)kp * A.ncn + i] = -(nv[0] * q[0] + nv[1] * q[1] + nv[2] * q[2]);
  }
  A.kp_mask[kp] = mask; A.kp_a2d[kp] = a2d; A.kp_w[kp] = w;
  double *po = A.kp_pt + 3 * (size_t)kp, *no = A.kp_nrm + 3 * (size_t)kp;
  for (int a = 0; a < 3; a++) no[a] = nv[a];
  if (A.ct) { for (int a = 0; a < 3; a++) po[a] = raw[a]; }
  else {      // point_end = rotation.inverse() * point - rotation.inverse() * translation
    const double q2 = qb.x * qb.x + qb.y * qb.y + qb.z * qb.z + qb.w * qb.w;
    const Qx qi = {-qb.x / q2, -qb.y / q2, -qb.z / q2, qb.w / q2};
    double Ri[9];
    qrotx(qi, Ri);
    for (int a = 0; a < 3; a++)
      po[a] = (Ri[3 * a] * pw[0] + Ri[3 * a + 1] * pw[1] + Ri[3 * a + 2] * pw[2]) - (Ri[3 * a] * A.pb[0] + Ri[3 * a + 1] * A.pb[1] + Ri[3 * a + 2] * A.pb[2]);
  }
}
// residuals in (keypoint, neighbour) order, cut at max_res: exactly the rows the reference's two breaks let through
struct ResOut { int *src; double *pts, *nrm, *off, *al, *w; };
__global__ __launch_bounds__(VM_THREADS) void k_vm_compact(VmDev V, AssocArgs A, ResOut O, int max_res) {
  __shared__ int lds[20];
  if (A.skip && *A.skip) return;
  const int t = threadIdx.x, chunk = (A.n + VM_THREADS - 1) / VM_THREADS, k0 = min(A.n, t * chunk), k1 = min(A.n, k0 + chunk);
  int mine = 0, nan = 0, total, tnan;
  for (int k = k0; k < k1; k++) { mine += __popc(A.kp_mask[k]); nan += A.kp_nan[k]; }
  int dst = block_exclusive_scan<VM_THREADS>(mine, &total, lds);
  (void)block_exclusive_scan<VM_THREADS>(nan, &tnan, lds);
  for (int k = k0; k < k1 && dst < max_res; k++) {
    const unsigned int mask = A.kp_mask[k];
    for (int i = 0; i < A.ncn && dst < max_res; i++) {
      if (!(mask >> i & 1u)) continue;
      O.src[dst] = k; O.off[dst] = A.kp_off[(size_t)k * A.ncn + i]; O.al[dst] = A.ct ? A.alpha[k] : 0.0; O.w[dst] = A.kp_w[k];
      for (int a = 0; a < 3; a++) { O.pts[3 * (size_t)dst + a] = A.kp_pt[3 * (size_t)k + a]; O.nrm[3 * (size_t)dst + a] = A.kp_nrm[3 * (size_t)k + a]; }
      dst++;
    }
  }
  if (t == 0) { V.meta[M_NRES] = min(total, max_res); V.meta[M_TOTAL] = total; V.meta[M_NAN] = tnan; }
}

// checkLocalizability: singular values of the N x 3 normal matrix = sqrt of the eigenvalues of N^T N, summed in a fixed order
__global__ __launch_bounds__(256) void k_vm_local(VmDev V, const double *nrm, double *out) {
  const int t = threadIdx.x, n = V.meta[M_NRES];
  __shared__ double red[4][6];
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = t; k < n; k += 256) {
    const double *v = nrm + 3 * (size_t)k;
    acc[0] += v[0] * v[0]; acc[1] += v[0] * v[1]; acc[2] += v[0] * v[2]; acc[3] += v[1] * v[1]; acc[4] += v[1] * v[2]; acc[5] += v[2] * v[2];
  }
#pragma unroll
  for (int q = 0; q < 6; q++) {
    double v = acc[q];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((t & 63) == 0) red[t >> 6][q] = v;
  }
  __syncthreads();
  if (t == 0) {
    double M[6], lam[3], Q[9];
    for (int q = 0; q < 6; q++) M[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    vmap_eig3(M, lam, Q);
    const double sv[3] = {sqrt(fabs(lam[2])), sqrt(fabs(lam[1])), sqrt(fabs(lam[0]))};
    out[0] = sv[0]; out[1] = sv[1]; out[2] = sv[2];
    out[3] = (n <= 10 || (sv[0] + sv[2] + sv[1]) / 3 < 10 || sv[2] < 7) ? 1.0 : 0.0;
  }
}

VmDev vm_dev(const gfbe_vmap *m, int half) { return VmDev{m->keys[half], m->cnt[half], m->pts[half], m->slots - 1, m->P, m->cap, m->meta}; }
gfbe_status vm_ready(gfbe_ctx *c, gfbe_vmap *m) { return handle_device(c, m, "gfbe_vmap"); }
bool vm_options_ok(const gfbe_vmap_options *o) {
  return o->struct_size == (int32_t)sizeof(gfbe_vmap_options) && o->size_voxel_map > 0.0 && std::isfinite(o->size_voxel_map) &&
         o->max_num_points_in_voxel >= 1 && o->max_num_points_in_voxel <= VM_MAXP && o->min_distance_points >= 0.0 && o->max_distance > 0.0 &&
         o->voxel_neighborhood >= 0 && o->voxel_neighborhood <= 2 && o->max_number_neighbors >= 1 && o->max_number_neighbors <= VM_MAXP &&
         o->min_number_neighbors >= 1 && o->threshold_voxel_occupancy >= 0 && o->num_closest_neighbors >= 1 &&
         o->num_closest_neighbors <= o->max_number_neighbors && o->max_dist_to_plane_icp > 0.0 && std::isfinite(o->power_planarity) &&
         std::fabs(o->weight_alpha) + std::fabs(o->weight_neighborhood) > 0.0 && o->max_num_residuals >= 1 && o->max_num_residuals <= (1 << 22);
}
template <typename T>
T *vm_carve(char *&p, size_t n) { T *r = (T *)p; p += (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255; return r; }

// the per-keypoint scratch of one association and the options it reads (raw, alpha, pb, pe, skip are the caller's)
gfbe_status vm_assoc_args(gfbe_ctx *c, gfbe_vmap *m, int ct, int n, int frame_init, AssocArgs *out) {
  const gfbe_vmap_options &o = m->opt;
  const size_t N = (size_t)std::max(n, 1);
  GFBE_CHECK(c, grow(ctx_stream(c), m->kp_buf, 3 * ((N * 4 + 255) & ~(size_t)255) + ((N * 4 * o.max_number_neighbors + 255) & ~(size_t)255) + 2 * ((N * 8 + 255) & ~(size_t)255) + 2 * ((N * 24 + 255) & ~(size_t)255) +
                                     ((N * 8 * o.num_closest_neighbors + 255) & ~(size_t)255)));
  char *p = m->kp_buf.d;
  AssocArgs A;
  A.n = n; A.ct = ct ? 1 : 0; A.v = frame_init ? 2 : o.voxel_neighborhood; A.thr = frame_init ? 1 : o.threshold_voxel_occupancy;
  A.K = o.max_number_neighbors; A.min_nn = o.min_number_neighbors; A.ncn = o.num_closest_neighbors;
  A.size = o.size_voxel_map; A.max_plane = o.max_dist_to_plane_icp; A.power = o.power_planarity; A.w_alpha = o.weight_alpha; A.w_nb = o.weight_neighborhood;
  A.kp_cnt = vm_carve<int>(p, N); A.kp_mask = vm_carve<unsigned int>(p, N); A.kp_nan = vm_carve<int>(p, N); A.kp_vis = vm_carve<int>(p, N * o.max_number_neighbors);
  A.kp_a2d = vm_carve<double>(p, N); A.kp_w = vm_carve<double>(p, N); A.kp_nrm = vm_carve<double>(p, 3 * N); A.kp_pt = vm_carve<double>(p, 3 * N);
  A.kp_off = vm_carve<double>(p, N * o.num_closest_neighbors);
  A.raw = A.alpha = A.pb = A.pe = nullptr; A.skip = nullptr;
  *out = A;
  return GFBE_OK;
}

}  // namespace

extern "C" {

void gfbe_vmap_default_options(gfbe_vmap_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = (int32_t)sizeof(gfbe_vmap_options);
  o->size_voxel_map = 0.2; o->max_num_points_in_voxel = 20; o->min_distance_points = 0.05; o->max_distance = 500.0;
  o->voxel_neighborhood = 1; o->max_number_neighbors = 20; o->min_number_neighbors = 20; o->threshold_voxel_occupancy = 1;
  o->num_closest_neighbors = 1; o->max_dist_to_plane_icp = 0.3; o->power_planarity = 2.0; o->weight_alpha = 0.9;
  o->weight_neighborhood = 0.1; o->max_num_residuals = 2000;
}

void gfbe_vmap_destroy(gfbe_ctx *c, gfbe_vmap *m) {
  if (!m) return;
  m->release(c);
  for (const DevBuf *b : {&m->add_buf, &m->kp_buf, &m->sort_buf})
    if (b->d) (void)hipFree(b->d);
  delete m;
}

gfbe_status gfbe_vmap_create(gfbe_ctx *c, int32_t voxel_capacity, const gfbe_vmap_options *opt, gfbe_vmap **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  gfbe_vmap_options o;
  if (opt) { if (opt->struct_size != (int32_t)sizeof(gfbe_vmap_options)) return GFBE_BAD_INPUT; o = *opt; }
  else gfbe_vmap_default_options(&o);
  if (!vm_options_ok(&o)) { ctx_set_error(c, "gfbe_vmap_create: an option is outside its admitted range"); return GFBE_BAD_INPUT; }
  if (voxel_capacity < 1 || voxel_capacity > (1 << 21)) return GFBE_BAD_INPUT;
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_vmap_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  gfbe_vmap *m = new gfbe_vmap();
  CreateGuard<gfbe_vmap> guard{c, m, gfbe_vmap_destroy};
  m->owner = c; m->opt = o; m->cap = voxel_capacity; m->P = o.max_num_points_in_voxel;
  int slots = 64;
  while (slots < 2 * voxel_capacity) slots <<= 1;
  m->slots = slots;
#define VA(p, n, fill) if (!m->alloc(&p, n, fill)) return GFBE_DEVICE_ERROR
  for (int b = 0; b < 2; b++) { VA(m->keys[b], (size_t)slots, 0xFF); VA(m->cnt[b], (size_t)slots, 0); VA(m->pts[b], (size_t)slots * m->P * 3, 0); }
  VA(m->meta, VM_META, 0); VA(m->part, 2 * (size_t)(slots / 256 + 1), 0);
  const size_t R = (size_t)o.max_num_residuals;
  VA(m->res_src, R, 0); VA(m->res_pts, 3 * R, 0); VA(m->res_nrm, 3 * R, 0); VA(m->res_off, R, 0); VA(m->res_al, R, 0); VA(m->res_w, R, 0);
#undef VA
  if (!m->make_staging(c, "gfbe_vmap_create", 1 << 16, true)) return GFBE_DEVICE_ERROR;
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  guard.armed = false;
  *out = m;
  return GFBE_OK;
}

// the add_points pipeline on points already on the device (din [n][3], valid on the stream until the last kernel below has run)
static gfbe_status vm_add_device(gfbe_ctx *c, gfbe_vmap *m, int n, const double *din, int min_num_points, unsigned long long *key, unsigned long long *skey,
                                 int *idx, int *sidx, int *isnew, int *skip, int *added, size_t tmp_bytes) {
  hipStream_t s = ctx_stream(c);
  const size_t N = (size_t)n;
  const VmDev V = vm_dev(m, m->cur);
  const unsigned g = (unsigned)((N + 255) / 256);
  hipLaunchKernelGGL(k_vm_keys, dim3(g), dim3(256), 0, s, n, din, m->opt.size_voxel_map, key, idx);
  GFBE_CHECK(c, rocprim::radix_sort_pairs(m->sort_buf.d, tmp_bytes, key, skey, idx, sidx, N, 0, 49, s));      // (stable: input order inside a voxel)
  hipLaunchKernelGGL(k_vm_probe, dim3(g), dim3(256), 0, s, V, n, skey, min_num_points, isnew, skip);
  hipLaunchKernelGGL(k_vm_admit, dim3(1), dim3(VM_THREADS), 0, s, V, n, isnew, skip);
  hipLaunchKernelGGL(k_vm_insert, dim3(g), dim3(256), 0, s, V, n, skey, sidx, din, m->opt.size_voxel_map, m->opt.min_distance_points, min_num_points, added);
  hipLaunchKernelGGL(k_vm_added, dim3(1), dim3(VM_THREADS), 0, s, V, n, added);
  return GFBE_OK;
}
struct AddScratch { unsigned long long *key, *skey; int *idx, *sidx, *isnew, *skip, *added; double *world; size_t tmp_bytes; };
// scratch: key, idx, sorted key, sorted idx, isnew, skip, added (+ world points [n][3] when asked for)
static gfbe_status vm_add_scratch(gfbe_ctx *c, gfbe_vmap *m, int n, bool world, AddScratch *a) {
  hipStream_t s = ctx_stream(c);
  const size_t N = (size_t)n;
  GFBE_CHECK(c, grow(s, m->add_buf, 2 * ((N * 8 + 255) & ~(size_t)255) + 5 * ((N * 4 + 255) & ~(size_t)255) + (world ? ((N * 24 + 255) & ~(size_t)255) : 0)));
  char *p = m->add_buf.d;
  a->key = vm_carve<unsigned long long>(p, N); a->skey = vm_carve<unsigned long long>(p, N);
  a->idx = vm_carve<int>(p, N); a->sidx = vm_carve<int>(p, N); a->isnew = vm_carve<int>(p, N); a->skip = vm_carve<int>(p, N); a->added = vm_carve<int>(p, N);
  a->world = world ? vm_carve<double>(p, 3 * N) : nullptr;
  a->tmp_bytes = 0;
  GFBE_CHECK(c, rocprim::radix_sort_pairs(nullptr, a->tmp_bytes, a->key, a->skey, a->idx, a->sidx, N, 0, 49, s));
  GFBE_CHECK(c, grow(s, m->sort_buf, std::max<size_t>(a->tmp_bytes, 256)));
  return GFBE_OK;
}

gfbe_status gfbe_vmap_add_points(gfbe_ctx *c, gfbe_vmap *m, int32_t n, const double *pts_world, int32_t min_num_points) {
  gfbe_status st = vm_ready(c, m);
  if (st != GFBE_OK) return st;
  if (n < 0 || (n > 0 && !pts_world)) return GFBE_BAD_INPUT;
  if (n == 0) return GFBE_OK;
  m->gen++;
  const size_t N = (size_t)n;
  AddScratch a;
  if ((st = vm_add_scratch(c, m, n, false, &a)) != GFBE_OK) return st;
  {
    Staged sg(c, m, N * 24 + 1024, /*defer=*/true);
    double *din = sg.up(pts_world, 3 * N);
    if (!sg.ok) { ctx_set_error(c, "gfbe_vmap_add_points: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    if ((st = vm_add_device(c, m, n, din, min_num_points, a.key, a.skey, a.idx, a.sidx, a.isnew, a.skip, a.added, a.tmp_bytes)) != GFBE_OK) return st;
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

// transformKeypoints (lidarodom.cpp:509-532) on the device, then the add_points pipeline on the device buffer: the body on a scan
// already on the device (draw [n][3], dal [n], the poses dpb / dpe [7]; n > 0 known to the host)
static gfbe_status vm_add_scan_device(gfbe_ctx *c, gfbe_vmap *m, int ct, int n, const double *draw, const double *dal, const double *dpb, const double *dpe,
                                      int min_num_points, const AddScratch &a, double *pts_world_out) {
  hipStream_t s = ctx_stream(c);
  const size_t N = (size_t)n;
  gfbe_status st;
  hipLaunchKernelGGL(k_vm_world, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, n, ct ? 1 : 0, draw, dal, dpb, dpe, a.world);
  if ((st = vm_add_device(c, m, n, a.world, min_num_points, a.key, a.skey, a.idx, a.sidx, a.isnew, a.skip, a.added, a.tmp_bytes)) != GFBE_OK) return st;
  if (pts_world_out) GFBE_CHECK(c, hipMemcpyAsync(pts_world_out, a.world, sizeof(double) * 3 * N, hipMemcpyDeviceToHost, s));
  return GFBE_OK;
}

// the staging front of the host-fed call
gfbe_status gfbe_vmap_add_scan(gfbe_ctx *c, gfbe_vmap *m, int32_t ct, int32_t n, const double *raw_pts, const double *alpha, const double *pose_begin,
                               const double *pose_end, int32_t min_num_points, double *pts_world_out) {
  gfbe_status st = vm_ready(c, m);
  if (st != GFBE_OK) return st;
  if (n < 0 || !pose_begin || (n > 0 && !raw_pts) || (ct && (!pose_end || (n > 0 && !alpha)))) return GFBE_BAD_INPUT;
  if (n == 0) return GFBE_OK;
  m->gen++;
  const size_t N = (size_t)n;
  AddScratch a;
  if ((st = vm_add_scratch(c, m, n, true, &a)) != GFBE_OK) return st;
  {
    Staged sg(c, m, N * 32 + 2048, /*defer=*/pts_world_out == nullptr);
    const double *draw = sg.up(raw_pts, 3 * N), *dal = sg.up(ct ? alpha : nullptr, N), *dpb = sg.up(pose_begin, 7), *dpe = sg.up(pose_end ? pose_end : pose_begin, 7);
    if (!sg.ok) { ctx_set_error(c, "gfbe_vmap_add_scan: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    if ((st = vm_add_scan_device(c, m, ct, n, draw, dal, dpb, dpe, min_num_points, a, pts_world_out)) != GFBE_OK) return st;
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

// the same body on the POINTS of a scan handle: only the two poses are staged, nobody waits
gfbe_status gfbe_vmap_add_scan_handle(gfbe_ctx *c, gfbe_vmap *m, int32_t ct, gfbe_scan *scan, const double *pose_begin, const double *pose_end,
                                      int32_t min_num_points) {
  gfbe_status st = vm_ready(c, m);
  if (st != GFBE_OK) return st;
  if (!scan || !pose_begin || (ct && !pose_end)) return GFBE_BAD_INPUT;
  ScanView sv;
  if ((st = scan_points_view(c, scan, "gfbe_vmap_add_scan_handle", &sv)) != GFBE_OK) return st;
  if (sv.n == 0) return GFBE_OK;
  m->gen++;
  AddScratch a;
  if ((st = vm_add_scratch(c, m, sv.n, true, &a)) != GFBE_OK) return st;
  {
    Staged sg(c, m, 2048, /*defer=*/true);
    const double *dpb = sg.up(pose_begin, 7), *dpe = sg.up(pose_end ? pose_end : pose_begin, 7);
    if (!sg.ok) { ctx_set_error(c, "gfbe_vmap_add_scan_handle: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    if ((st = vm_add_scan_device(c, m, ct, sv.n, sv.pts, sv.alpha, dpb, dpe, min_num_points, a, nullptr)) != GFBE_OK) return st;
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_vmap_erase_far(gfbe_ctx *c, gfbe_vmap *m, const double *location) {
  gfbe_status st = vm_ready(c, m);
  if (st != GFBE_OK) return st;
  if (!location) return GFBE_BAD_INPUT;
  hipStream_t s = ctx_stream(c);
  m->gen++;
  {
    Staged sg(c, m, 1024, /*defer=*/true);
    double *dloc = sg.up(location, 3);
    if (!sg.ok) { ctx_set_error(c, "gfbe_vmap_erase_far: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    const int nb = (m->slots + 255) / 256;
    hipLaunchKernelGGL(k_vm_rehash, dim3(nb), dim3(256), 0, s, vm_dev(m, m->cur), vm_dev(m, 1 - m->cur), dloc, m->opt.max_distance * m->opt.max_distance, m->part);
    hipLaunchKernelGGL(k_vm_recount, dim3(1), dim3(VM_THREADS), 0, s, vm_dev(m, m->cur), nb, m->part);
    GFBE_CHECK(c, hipMemsetAsync(m->keys[m->cur], 0xFF, sizeof(unsigned long long) * (size_t)m->slots, s));
    m->cur = 1 - m->cur;
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_vmap_size(gfbe_ctx *c, gfbe_vmap *m, int32_t *n_voxels, int32_t *n_points, int32_t *n_skipped, int32_t *overflow) {
  gfbe_status st = vm_ready(c, m);
  if (st != GFBE_OK) return st;
  hipStream_t s = ctx_stream(c);
  GFBE_CHECK(c, hipMemcpyAsync(m->stage_h, m->meta, sizeof(int) * VM_META, hipMemcpyDeviceToHost, s));
  GFBE_CHECK(c, hipStreamSynchronize(s));
  const int *h = (const int *)m->stage_h;
  if (n_voxels) *n_voxels = h[M_VOX];
  if (n_points) *n_points = h[M_PTS];
  if (n_skipped) *n_skipped = h[M_SKIP];
  if (overflow) *overflow = h[M_OVER];
  return GFBE_OK;
}

gfbe_status gfbe_vmap_download(gfbe_ctx *c, gfbe_vmap *m, int16_t *keys, int32_t *counts, double *points) {
  gfbe_status st = vm_ready(c, m);
  if (st != GFBE_OK) return st;
  hipStream_t s = ctx_stream(c);
  const size_t S = (size_t)m->slots;
  std::vector<unsigned long long> hk(S);
  std::vector<int> hc(S);
  GFBE_CHECK(c, hipMemcpyAsync(hk.data(), m->keys[m->cur], 8 * S, hipMemcpyDeviceToHost, s));
  GFBE_CHECK(c, hipMemcpyAsync(hc.data(), m->cnt[m->cur], 4 * S, hipMemcpyDeviceToHost, s));
  GFBE_CHECK(c, hipStreamSynchronize(s));
  std::vector<int> slot;
  for (size_t i = 0; i < S; i++) if (hk[i] != VM_EMPTY) slot.push_back((int)i);
  std::sort(slot.begin(), slot.end(), [&](int a, int b) { return hk[a] < hk[b]; });
  const size_t nv = slot.size();
  std::vector<int> off(nv + 1, 0);
  for (size_t v = 0; v < nv; v++) {
    off[v + 1] = off[v] + hc[slot[v]];
    if (keys) { int x, y, z; vmap_unpack(hk[slot[v]], &x, &y, &z); keys[3 * v] = (int16_t)x; keys[3 * v + 1] = (int16_t)y; keys[3 * v + 2] = (int16_t)z; }
    if (counts) counts[v] = hc[slot[v]];
  }
  if (!points || nv == 0) return GFBE_OK;
  const size_t np = (size_t)off[nv];
  {
    Staged sg(c, m, nv * 8 + np * 24 + 4096);
    int *dslot = sg.up(slot.data(), nv), *doff = sg.up(off.data(), nv + 1);
    double *dout = sg.up<double>(nullptr, 3 * np);
    if (!sg.ok) { ctx_set_error(c, "gfbe_vmap_download: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    hipLaunchKernelGGL(k_vm_gather, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, vm_dev(m, m->cur), (int)nv, dslot, doff, dout);
    sg.down(points, dout, 3 * np);
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_vmap_upload(gfbe_ctx *c, gfbe_vmap *m, int32_t n_voxels, const int16_t *keys, const int32_t *counts, const double *points) {
  gfbe_status st = vm_ready(c, m);
  if (st != GFBE_OK) return st;
  if (n_voxels < 0 || n_voxels > m->cap || (n_voxels > 0 && (!keys || !counts || !points))) return GFBE_BAD_INPUT;
  const size_t nv = (size_t)n_voxels;
  std::vector<unsigned long long> hk(nv + 1);
  std::vector<int> off(nv + 1, 0);
  for (size_t v = 0; v < nv; v++) {
    const int x = keys[3 * v], y = keys[3 * v + 1], z = keys[3 * v + 2];
    if (std::abs(x) > 32766 || std::abs(y) > 32766 || std::abs(z) > 32766 || counts[v] < 1 || counts[v] > m->P) { ctx_set_error(c, "gfbe_vmap_upload: a key or a count is out of range"); return GFBE_BAD_INPUT; }
    hk[v] = vmap_pack(x, y, z);
    if (v > 0 && hk[v] <= hk[v - 1]) { ctx_set_error(c, "gfbe_vmap_upload: keys must be strictly ascending in (x, y, z)"); return GFBE_BAD_INPUT; }
    off[v + 1] = off[v] + counts[v];
  }
  hipStream_t s = ctx_stream(c);
  m->gen++;
  {
    const size_t np = (size_t)off[nv];
    Staged sg(c, m, nv * 12 + np * 24 + 4096);
    unsigned long long *dk = sg.up(hk.data(), nv);
    int *doff = sg.up(off.data(), nv + 1);
    double *dp = sg.up(points, 3 * np);
    if (!sg.ok) { ctx_set_error(c, "gfbe_vmap_upload: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    GFBE_CHECK(c, hipMemsetAsync(m->keys[m->cur], 0xFF, sizeof(unsigned long long) * (size_t)m->slots, s));
    GFBE_CHECK(c, hipMemsetAsync(m->meta, 0, sizeof(int) * 2, s));      // voxel and point count (the sticky counters stay)
    if (nv) hipLaunchKernelGGL(k_vm_scatter, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, vm_dev(m, m->cur), (int)nv, dk, doff, dp);
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_vmap_associate(gfbe_ctx *c, gfbe_vmap *m, int32_t ct, int32_t n, const double *raw_pts, const double *alpha, const double *pose_begin,
                                const double *pose_end, int32_t frame_init, int32_t *n_res, int32_t *src, double *pts, double *normals, double *offsets,
                                double *alpha_out, double *weights, int32_t *neighbor_count, double *a2D, int32_t *n_nan, int32_t *neighbor_visit) {
  gfbe_status st = vm_ready(c, m);
  if (st != GFBE_OK) return st;
  if (n < 0 || !pose_begin || (n > 0 && !raw_pts) || (ct && (!pose_end || (n > 0 && !alpha)))) return GFBE_BAD_INPUT;
  hipStream_t s = ctx_stream(c);
  const gfbe_vmap_options &o = m->opt;
  const size_t N = (size_t)std::max(n, 1);
  m->assoc_valid = false;
  AssocArgs A;
  if ((st = vm_assoc_args(c, m, ct, n, frame_init, &A)) != GFBE_OK) return st;
  int hmeta[VM_META] = {0};
  {
    Staged sg(c, m, N * 32 + 4096);
    A.raw = sg.up(raw_pts, 3 * (size_t)n);
    A.alpha = sg.up(ct ? alpha : nullptr, (size_t)n);
    A.pb = sg.up(pose_begin, 7);
    A.pe = sg.up(pose_end ? pose_end : pose_begin, 7);
    if (!sg.ok) { ctx_set_error(c, "gfbe_vmap_associate: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    const VmDev V = vm_dev(m, m->cur);
    if (n > 0) hipLaunchKernelGGL(k_vm_assoc, dim3(n), dim3(64), 0, s, V, A);
    hipLaunchKernelGGL(k_vm_compact, dim3(1), dim3(VM_THREADS), 0, s, V, A, ResOut{m->res_src, m->res_pts, m->res_nrm, m->res_off, m->res_al, m->res_w}, o.max_num_residuals);
    sg.down(hmeta, (const int *)m->meta, VM_META);
    if (n > 0) { sg.down(neighbor_count, (const int *)A.kp_cnt, (size_t)n); sg.down(a2D, (const double *)A.kp_a2d, (size_t)n); sg.down(neighbor_visit, (const int *)A.kp_vis, (size_t)n * o.max_number_neighbors); }
  }
  GFBE_CHECK(c, hipGetLastError());
  if (hmeta[M_OVER]) { ctx_set_error(c, "voxel map capacity exceeded"); return GFBE_BAD_INPUT; }
  const size_t R = (size_t)hmeta[M_NRES];
  m->n_res = (int)R; m->assoc_ct = A.ct; m->assoc_gen = m->gen; m->assoc_valid = true;
  if (n_res) *n_res = (int32_t)R;
  if (n_nan) *n_nan = hmeta[M_NAN];
  if (R) {
#define DN(h, d, cnt) if (h) GFBE_CHECK(c, hipMemcpyAsync(h, d, sizeof(*h) * (cnt), hipMemcpyDeviceToHost, s))
    DN(src, m->res_src, R); DN(pts, m->res_pts, 3 * R); DN(normals, m->res_nrm, 3 * R); DN(offsets, m->res_off, R); DN(alpha_out, m->res_al, R); DN(weights, m->res_w, R);
#undef DN
    GFBE_CHECK(c, hipStreamSynchronize(s));
  }
  return GFBE_OK;
}

static gfbe_status vm_assoc_current(gfbe_ctx *c, gfbe_vmap *m, const char *who) {
  if (m->assoc_valid && m->assoc_gen == m->gen) return GFBE_OK;
  ctx_set_error(c, (std::string(who) + ": no association of the map as it is now (call gfbe_vmap_associate after the last change)").c_str());
  return GFBE_BAD_INPUT;
}

gfbe_status gfbe_vmap_linearize(gfbe_ctx *c, gfbe_vmap *m, int32_t ct, double sqrt_info, const double *pose_begin, const double *pose_end, double *r,
                                double *J, double *H, double *g, double *cost) {
  gfbe_status st = vm_ready(c, m);
  if (st != GFBE_OK) return st;
  if (!pose_begin || (ct && !pose_end)) return GFBE_BAD_INPUT;
  if ((st = vm_assoc_current(c, m, "gfbe_vmap_linearize")) != GFBE_OK) return st;
  if ((ct ? 1 : 0) != m->assoc_ct) { ctx_set_error(c, "gfbe_vmap_linearize: ct differs from the association's"); return GFBE_BAD_INPUT; }
  return lio_linearize_device(c, ct, m->n_res, m->res_pts, m->res_nrm, m->res_off, m->res_al, m->res_w, sqrt_info, pose_begin, pose_end, r, J, H, g, cost);
}

gfbe_status gfbe_vmap_localizability(gfbe_ctx *c, gfbe_vmap *m, double *sv, int32_t *degenerate) {
  gfbe_status st = vm_ready(c, m);
  if (st != GFBE_OK) return st;
  if ((st = vm_assoc_current(c, m, "gfbe_vmap_localizability")) != GFBE_OK) return st;
  double out[4] = {0.0, 0.0, 0.0, 0.0};
  {
    Staged sg(c, m, 4096);
    double *dout = sg.up<double>(nullptr, 4);
    if (!sg.ok) { ctx_set_error(c, "gfbe_vmap_localizability: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    hipLaunchKernelGGL(k_vm_local, dim3(1), dim3(256), 0, ctx_stream(c), vm_dev(m, m->cur), m->res_nrm, dout);
    sg.down(out, (const double *)dout, 4);
  }
  GFBE_CHECK(c, hipGetLastError());
  if (sv) for (int a = 0; a < 3; a++) sv[a] = out[a];
  if (degenerate) *degenerate = out[3] != 0.0;
  return GFBE_OK;
}

}  // extern "C"

// ---- what the registration loop (gfbe_vreg.hip) enqueues from this file's kernels: every argument is already on the device
namespace gfd {
gfbe_status vmap_enqueue_assoc(gfbe_ctx *c, gfbe_vmap *m, int ct, int n, const double *d_raw, const double *d_alpha, const double *d_pb, const double *d_pe,
                               int frame_init, const int *d_skip) {
  AssocArgs A;
  const gfbe_status st = vm_assoc_args(c, m, ct, n, frame_init, &A);
  if (st != GFBE_OK) return st;
  A.raw = d_raw; A.alpha = d_alpha; A.pb = d_pb; A.pe = d_pe; A.skip = d_skip;
  const VmDev V = vm_dev(m, m->cur);
  if (n > 0) hipLaunchKernelGGL(k_vm_assoc, dim3(n), dim3(64), 0, ctx_stream(c), V, A);
  hipLaunchKernelGGL(k_vm_compact, dim3(1), dim3(VM_THREADS), 0, ctx_stream(c), V, A, ResOut{m->res_src, m->res_pts, m->res_nrm, m->res_off, m->res_al, m->res_w}, m->opt.max_num_residuals);
  return GFBE_OK;
}
void vmap_enqueue_local(gfbe_ctx *c, gfbe_vmap *m, double *d_out4) {
  hipLaunchKernelGGL(k_vm_local, dim3(1), dim3(256), 0, ctx_stream(c), vm_dev(m, m->cur), m->res_nrm, d_out4);
}
}  // namespace gfd
