// gfbe_dmap.h — the per-point pieces of the dense RGB-D map (gfbe_dmap.hip). No HIP header is needed: under a plain C++ compiler
// the functions are ordinary inline functions, under hipcc they are __host__ __device__ (tests/dmap_host_shim.cpp compiles them for
// the host): the world point, the height gate, the voxel key and its packing, the squared distance and the coarse cell of the filter.
//
//   addKeyFrame   world point, gate, density test   dense_map/src/pose_graph.cpp:199-219
//   updatePath    world point, density test         :1015-1029
//   RadiusOutlierRemoval                            :230-238, :1043-1051
//
// Every operation is written once and in one order (products left to right per row, no contraction: the library is built with
// -ffp-contract=off), so that the model tests/dmap_np.py reproduces it bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GF_DM_HD __host__ __device__ inline
#else
#define GF_DM_HD inline
#endif

namespace gfd {

constexpr int DM_KEY_BITS = 21;                     // per axis: 0 <= key < 2^21, three axes in 63 bits (VM_EMPTY = ~0 stays free)
constexpr int DM_MAX_CAP = 8;                       // admitted add_cap / rebuild_cap
constexpr double DM_CELL_DIV = 1.75;                // coarse cell side s = radius / 1.75: s sqrt(3) = 0.98974 radius <= radius, 2 s >= radius
constexpr int DM_CELL_OFF = 1 << 20;                // offset of the signed coarse-cell index

// the rotation matrix of a quaternion x y z w: the formula and the order of qrot (gfbe_math.h), row-major
GF_DM_HD void dmap_rot(const double *q, double *R) {
  const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}
// RP = R(q) [9] | P [3] of a pose [t | q]
GF_DM_HD void dmap_pose_rp(const double *pose7, double *RP) {
  dmap_rot(pose7 + 3, RP);
  RP[9] = pose7[0]; RP[10] = pose7[1]; RP[11] = pose7[2];
}
// pw = R (R_ic p + t_ic) + P in FP64 (pose_graph.cpp:200, :1016); RP, RPic as dmap_pose_rp leaves them
GF_DM_HD void dmap_world(const double *RP, const double *RPic, const float *p, double *pw) {
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  double c[3];
  for (int a = 0; a < 3; a++) c[a] = ((RPic[3 * a] * x + RPic[3 * a + 1] * y) + RPic[3 * a + 2] * z) + RPic[9 + a];
  for (int a = 0; a < 3; a++) pw[a] = ((RP[3 * a] * c[0] + RP[3 * a + 1] * c[1]) + RP[3 * a + 2] * c[2]) + RP[9 + a];
}
// the height gate of addKeyFrame (:201) on the FP64 value; a NaN passes here and has no voxel
GF_DM_HD bool dmap_gated(double z, double z_min, double z_max) { return z > z_max || z < z_min; }

// floor(((double)pf - origin) / resolution) of the float point; false: outside 0 .. 2^21 - 1 or NaN
GF_DM_HD bool dmap_axis_key(float pf, double origin, double resolution, int *k) {
  const double q = floor(((double)pf - origin) / resolution);
  if (!(q >= 0.0 && q < (double)(1 << DM_KEY_BITS))) return false;
  *k = (int)q;
  return true;
}
GF_DM_HD uint64_t dmap_pack(int x, int y, int z) { return ((uint64_t)x << (2 * DM_KEY_BITS)) | ((uint64_t)y << DM_KEY_BITS) | (uint64_t)z; }
GF_DM_HD void dmap_unpack(uint64_t key, int *x, int *y, int *z) {
  const uint64_t m = ((uint64_t)1 << DM_KEY_BITS) - 1;
  *x = (int)((key >> (2 * DM_KEY_BITS)) & m); *y = (int)((key >> DM_KEY_BITS) & m); *z = (int)(key & m);
}
GF_DM_HD bool dmap_key(const float *pf, double origin, double resolution, uint64_t *key) {
  int x, y, z;
  if (!dmap_axis_key(pf[0], origin, resolution, &x) || !dmap_axis_key(pf[1], origin, resolution, &y) || !dmap_axis_key(pf[2], origin, resolution, &z)) return false;
  *key = dmap_pack(x, y, z);
  return true;
}

// (dx dx + dy dy) + dz dz, differences and products in FP64 on the float coordinates
GF_DM_HD double dmap_sqdist(const float *a, const float *b) {
  const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// ---- the coarse grid of the radius filter: side s = radius / DM_CELL_DIV. Two points of one cell differ by less than s (1 + 2^-50)
// per axis, so their distance is below radius; two points within radius lie at most two cells apart per axis.
GF_DM_HD double dmap_cell_side(double radius) { return radius / DM_CELL_DIV; }
GF_DM_HD int dmap_cell_axis(float pf, double side) { return (int)floor((double)pf / side) + DM_CELL_OFF; }
// the cell of a cloud point (inside the voxel box, which gfbe_dmap_create checks to fit 2 .. 2^21 - 3 per axis)
GF_DM_HD void dmap_cell(const float *pf, double side, int *c) {
  for (int a = 0; a < 3; a++) c[a] = dmap_cell_axis(pf[a], side);
}
// false: the box [origin, origin + 2^21 resolution) does not fit the coarse grid with its two-cell border, or an argument is unusable
GF_DM_HD bool dmap_cells_fit(double origin, double resolution, double radius) {
  if (!(radius > 0.0) || !(resolution > 0.0) || !isfinite(radius) || !isfinite(resolution) || !isfinite(origin)) return false;
  const double side = dmap_cell_side(radius), hi = origin + (double)(1 << DM_KEY_BITS) * resolution;
  const double reach = (fabs(origin) > fabs(hi) ? fabs(origin) : fabs(hi)) / side;
  return reach < (double)(DM_CELL_OFF - 4);
}

}  // namespace gfd
