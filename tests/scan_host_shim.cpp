// tests/scan_host_shim.cpp — TEST HARNESS ONLY. Compiles the __host__ __device__ pieces of the device-resident LiDAR scan
// (ground-fusion2_amd/csrc/gfbe_scan.h: the segment search, the interpolated pose, the motion compensation of a point, T_IL) for the
// HOST so that tests/test_scan_model.py can pin them against tests/scan_np.py without a GPU, and holds a single-thread host
// restatement of the one-point-per-voxel step on std::unordered_map and of the world points (hscan_*): the host leg of
// tools/diag_scan_bench.py. Never loaded by the package.
#include <unordered_map>

#include "../ground-fusion2_amd/csrc/gfbe_scan.h"
#include "../ground-fusion2_amd/csrc/gfbe_vmap.h"

using namespace gfd;

extern "C" {
int shim_scan_segment(int n, const double *t, double q) { return scan_segment(n, t, q); }
// Ti [7] of a point stamped q; returns the segment
int shim_scan_pose_at(int n, const double *t, const double *pose, double q, double *Ti) {
  int seg;
  scan_pose_at(n, t, pose, q, &seg, Ti);
  return seg;
}
// Undistort of m points: out [m][3], seg [m]
void shim_scan_undistort(int n, const double *t, const double *pose, int m, const double *pts, const double *ts, double *out, int *seg) {
  for (int i = 0; i < m; i++) {
    double Ti[7];
    scan_pose_at(n, t, pose, ts[i], seg + i, Ti);
    scan_undistort_point(pose + 7 * (n - 1), Ti, pts + 3 * i, out + 3 * i);
  }
}
void shim_scan_til(const double *til, const double *p, double *out) { scan_til_point(til, p, out); }
// the voxel key the one-point-per-voxel steps use (gfbe_vmap.h): 1 and key [3], or 0 for a dropped point
int shim_scan_key(const double *p, double size, int *key) {
  uint64_t k;
  if (!vmap_key(p, size, &k)) return 0;
  vmap_unpack(k, key, key + 1, key + 2);
  return 1;
}
// subSampleFrame on the host: the first index of every voxel, ascending; returns their number (dropped points in *skipped)
int hscan_subsample(int n, const double *pts, double size, int *kept, int *skipped) {
  std::unordered_map<uint64_t, int> first;
  first.reserve((size_t)n);
  int m = 0, drop = 0;
  for (int i = 0; i < n; i++) {
    uint64_t k;
    if (!vmap_key(pts + 3 * (size_t)i, size, &k)) { drop++; continue; }
    if (first.emplace(k, i).second) kept[m++] = i;
  }
  *skipped = drop;
  return m;
}
// transformPoint of n points
void hscan_world(int ct, int n, const double *pts, const double *alpha, const double *pb, const double *pe, double *out) {
  const Qx qb = {pb[3], pb[4], pb[5], pb[6]}, qe = {pe[3], pe[4], pe[5], pe[6]};
  for (int i = 0; i < n; i++) {
    double R[9];
    lio_world_point(ct, qb, qe, pb, pe, ct ? alpha[i] : 0.0, pts + 3 * (size_t)i, R, out + 3 * (size_t)i);
  }
}
}
