// gfbe_vmap.h — the per-point pieces of the device voxel map (gfbe_vmap.hip), __host__ __device__ so that tests/vmap_host_shim.cpp
// can compile them for the host: the voxel key, the neighbourhood moments, the 3 x 3 symmetric eigensolver, a2D and the weight.
//
//   addPointToMap / searchNeighbors key   lio/src/liw/lio/lidarodom.cpp:1096-1098, 1172-1174
//   computeNeighborhoodDistribution       :887-927
//   the weight of addSurfCostFactor       :944-948, 992-997
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace gfd {

constexpr uint64_t VM_EMPTY = ~0ull;           // a free slot of the table
constexpr uint64_t VM_INVALID = 1ull << 48;    // key of a point outside the short range (sorts behind every voxel)
constexpr int VM_MAXP = 32;                    // admitted max_num_points_in_voxel / max_number_neighbors

// (short)(p / size): truncation TOWARD ZERO (the voxels touching a coordinate plane are twice as wide). false: |p / size| >= 32767
// (or NaN), where the reference's cast is undefined.
__host__ __device__ inline bool vmap_axis_key(double p, double size, int *k) {
  const double q = p / size;
  if (!(fabs(q) < 32767.0)) return false;
  *k = (int)q;
  return true;
}
// keys ordered as (x, y, z) signed triples when compared as unsigned integers
__host__ __device__ inline uint64_t vmap_pack(int x, int y, int z) {
  return ((uint64_t)(x + 32768) << 32) | ((uint64_t)(y + 32768) << 16) | (uint64_t)(z + 32768);
}
__host__ __device__ inline void vmap_unpack(uint64_t key, int *x, int *y, int *z) {
  *x = (int)((key >> 32) & 0xFFFF) - 32768; *y = (int)((key >> 16) & 0xFFFF) - 32768; *z = (int)(key & 0xFFFF) - 32768;
}
__host__ __device__ inline bool vmap_key(const double *p, double size, uint64_t *key) {
  int x, y, z;
  if (!vmap_axis_key(p[0], size, &x) || !vmap_axis_key(p[1], size, &y) || !vmap_axis_key(p[2], size, &z)) return false;
  *key = vmap_pack(x, y, z);
  return true;
}
__host__ __device__ inline uint64_t vmap_hash(uint64_t k) {   // splitmix64 finaliser
  k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull; k ^= k >> 27; k *= 0x94d049bb133111ebull; k ^= k >> 31;
  return k;
}
__host__ __device__ inline double vmap_sqdist(const double *a, const double *b) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return dx * dx + dy * dy + dz * dz;
}

// barycentre and the upper triangle of the covariance [xx xy xz yy yz zz], the reference's order of sums (neighbour order)
__host__ __device__ inline void vmap_moments(const double *nb, int k, double *bary, double *cov) {
  double b[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < k; i++) for (int a = 0; a < 3; a++) b[a] += nb[3 * i + a];
  for (int a = 0; a < 3; a++) b[a] /= (double)k;
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < k; i++) {
    const double d[3] = {nb[3 * i] - b[0], nb[3 * i + 1] - b[1], nb[3 * i + 2] - b[2]};
    c[0] += d[0] * d[0]; c[1] += d[0] * d[1]; c[2] += d[0] * d[2]; c[3] += d[1] * d[1]; c[4] += d[1] * d[2]; c[5] += d[2] * d[2];
  }
  for (int a = 0; a < 3; a++) bary[a] = b[a];
  for (int a = 0; a < 6; a++) cov[a] = c[a];
}

// Cyclic Jacobi on a symmetric 3 x 3 [xx xy xz yy yz zz]: eigenvalues ascending in lam, eigenvector j in V[3 * a + j] (column j).
// A rotation is skipped once |a_pq| <= eps / 16 * sqrt|a_pp a_qq| (the relative criterion: small eigenvalues keep their digits).
__host__ __device__ inline void vmap_eig3(const double *cov, double *lam, double *V) {
  double A[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
  double Q[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  const double tol = 0.0625 * 2.220446049250313e-16;
  for (int sweep = 0; sweep < 12; sweep++) {
    int rotated = 0;
    for (int pq = 0; pq < 3; pq++) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2, o = 3 - p - q;
      const double apq = A[p][q];
      if (fabs(apq) <= tol * sqrt(fabs(A[p][p] * A[q][q]))) { A[p][q] = A[q][p] = 0.0; continue; }
      rotated = 1;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
      A[p][p] -= t * apq; A[q][q] += t * apq; A[p][q] = A[q][p] = 0.0;
      const double aop = A[o][p], aoq = A[o][q];
      A[o][p] = A[p][o] = c * aop - s * aoq;
      A[o][q] = A[q][o] = s * aop + c * aoq;
      for (int a = 0; a < 3; a++) {
        const double qp = Q[a][p], qq = Q[a][q];
        Q[a][p] = c * qp - s * qq;
        Q[a][q] = s * qp + c * qq;
      }
    }
    if (!rotated) break;
  }
  int i0 = 0, i1 = 1, i2 = 2;
  if (A[i1][i1] < A[i0][i0]) { const int t = i0; i0 = i1; i1 = t; }
  if (A[i2][i2] < A[i1][i1]) { const int t = i1; i1 = i2; i2 = t; }
  if (A[i1][i1] < A[i0][i0]) { const int t = i0; i0 = i1; i1 = t; }
  lam[0] = A[i0][i0]; lam[1] = A[i1][i1]; lam[2] = A[i2][i2];
  for (int a = 0; a < 3; a++) { V[3 * a] = Q[a][i0]; V[3 * a + 1] = Q[a][i1]; V[3 * a + 2] = Q[a][i2]; }
}

// the normal (eigenvector of the smallest eigenvalue, normalised) and a2D = (sigma_2 - sigma_3) / sigma_1, sigma = sqrt|lambda|
__host__ __device__ inline double vmap_normal_a2d(const double *cov, double *normal) {
  double lam[3], V[9];
  vmap_eig3(cov, lam, V);
  const double nn = sqrt(V[0] * V[0] + V[3] * V[3] + V[6] * V[6]);
  normal[0] = V[0] / nn; normal[1] = V[3] / nn; normal[2] = V[6] / nn;
  const double s1 = sqrt(fabs(lam[2])), s2 = sqrt(fabs(lam[1])), s3 = sqrt(fabs(lam[0]));
  return (s2 - s3) / s1;
}

// lambda_weight * a2D^power_planarity + lambda_neighborhood * exp(-d0 / (max_dist_to_plane_icp * min_number_neighbors))
__host__ __device__ inline double vmap_weight(double a2d, double d0, double weight_alpha, double weight_neighborhood, double power_planarity,
                                              double max_dist_to_plane, int min_number_neighbors) {
  double lw = fabs(weight_alpha), ln = fabs(weight_neighborhood);
  const double sum = lw + ln;
  lw /= sum; ln /= sum;
  return lw * pow(a2d, power_planarity) + ln * exp(-d0 / (max_dist_to_plane * min_number_neighbors));
}

}  // namespace gfd
