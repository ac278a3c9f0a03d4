// tests/dmap_host_shim.cpp — TEST HARNESS ONLY. Compiles the per-point pieces of the dense RGB-D map
// (ground-fusion2_amd/csrc/gfbe_dmap.h: world point, gate, voxel key and packing, squared distance, coarse cell) for the HOST so that
// tests/test_dmap_model.py can pin them against tests/dmap_np.py without a GPU, and holds a single-thread host restatement of the
// capped insert on std::unordered_map (hdmap_insert): the host leg of tools/diag_dmap_bench.py. Never loaded by the package.
#include <unordered_map>

#include "../ground-fusion2_amd/csrc/gfbe_dmap.h"
#include "../ground-fusion2_amd/csrc/gfbe_math.h"

using namespace gfd;

extern "C" {
// R [9] of dmap_rot; returns 1 when qrot of gfbe_math.h gives the same bits
int shim_dmap_rot(const double *q, double *R) {
  dmap_rot(q, R);
  const mat3 M = qrot(ldq(q));
  int same = 1;
  for (int a = 0; a < 9; a++) same &= (M.m[a] == R[a]) || (M.m[a] != M.m[a] && R[a] != R[a]);
  return same;
}
// pw [n][3] (FP64) and pf [n][3] (float) of n camera-frame points
void shim_dmap_world(const double *pose7, const double *ex_cam, int n, const float *pts, double *pw, float *pf) {
  double RP[12], RPic[12];
  dmap_pose_rp(pose7, RP);
  dmap_pose_rp(ex_cam, RPic);
  for (int i = 0; i < n; i++) {
    dmap_world(RP, RPic, pts + 3 * (size_t)i, pw + 3 * (size_t)i);
    for (int a = 0; a < 3; a++) pf[3 * (size_t)i + a] = (float)pw[3 * (size_t)i + a];
  }
}
int shim_dmap_gated(double z, double z_min, double z_max) { return dmap_gated(z, z_min, z_max) ? 1 : 0; }
// 1, key [3] and the packed key (round trip through dmap_unpack checked: 2 on a mismatch), or 0 for a point without a voxel
int shim_dmap_key(const float *pf, double origin, double resolution, int *key, unsigned long long *packed) {
  uint64_t k;
  if (!dmap_key(pf, origin, resolution, &k)) return 0;
  dmap_unpack(k, key, key + 1, key + 2);
  *packed = k;
  return dmap_pack(key[0], key[1], key[2]) == k && k != ~0ull ? 1 : 2;
}
double shim_dmap_sqdist(const float *a, const float *b) { return dmap_sqdist(a, b); }
double shim_dmap_cell_side(double radius) { return dmap_cell_side(radius); }
void shim_dmap_cell(const float *pf, double side, int *c) { dmap_cell(pf, side, c); }
int shim_dmap_cells_fit(double origin, double resolution, double radius) { return dmap_cells_fit(origin, resolution, radius) ? 1 : 0; }

// The sequential walk of addKeyFrame / updatePath on one list at one pose: kept [n] (0 / 1), the counts in a map the caller keeps
// between calls (hdmap_new / hdmap_free); gate != 0: the height gate. Returns the number kept.
void *hdmap_new() { return new std::unordered_map<uint64_t, int>(); }
void hdmap_free(void *h) { delete (std::unordered_map<uint64_t, int> *)h; }
int hdmap_insert(void *h, const double *pose7, const double *ex_cam, int n, const float *pts, int cap, int gate, double origin, double resolution,
                 double z_min, double z_max, float *world_out) {
  auto &counts = *(std::unordered_map<uint64_t, int> *)h;
  double RP[12], RPic[12];
  dmap_pose_rp(pose7, RP);
  dmap_pose_rp(ex_cam, RPic);
  int m = 0;
  for (int i = 0; i < n; i++) {
    double pw[3];
    dmap_world(RP, RPic, pts + 3 * (size_t)i, pw);
    if (gate && dmap_gated(pw[2], z_min, z_max)) continue;
    const float pf[3] = {(float)pw[0], (float)pw[1], (float)pw[2]};
    uint64_t k;
    if (!dmap_key(pf, origin, resolution, &k)) continue;
    int &c = counts[k];
    if (c >= cap) continue;
    c++;
    for (int a = 0; a < 3; a++) world_out[3 * (size_t)m + a] = pf[a];
    m++;
  }
  return m;
}
}
