// gfbe_vmap_impl.h — the voxel map handle (gfbe_vmap.hip) as the registration loop (gfbe_vreg.hip) sees it: the handle's
// fields, the device meta words and the launches of the association / localizability kernels on arguments already on the device;
// the probes of the open-addressing table and the views of a scan handle (gfbe_scan.hip), which shares them.
#pragma once
#include <vector>

#include "gfbe.h"
#include "gfbe_handle.h"      // gfbe_handle, gfd::DevBuf
#include "gfbe_vmap.h"        // vmap_hash, VM_EMPTY

struct gfbe_vmap : gfbe_handle {
  gfbe_vmap_options opt;
  int cap = 0, slots = 0, P = 0;
  unsigned long long *keys[2] = {};     // [slots]
  int *cnt[2] = {};                     // [slots]
  double *pts[2] = {};                  // [slots][P][3]
  int cur = 0;
  int *meta = nullptr;                  // [VM_META]
  int *part = nullptr;                  // [2][slots / 256] per-workgroup survivor counts of erase_far
  gfd::DevBuf add_buf, kp_buf, sort_buf;
  // the association held on the handle: [max_num_residuals] each
  int *res_src = nullptr;
  double *res_pts = nullptr, *res_nrm = nullptr, *res_off = nullptr, *res_al = nullptr, *res_w = nullptr;
  unsigned long long gen = 0, assoc_gen = 0;     // gen: bumped by every operation that may change the map
  bool assoc_valid = false;
  int assoc_ct = 0, n_res = 0;
};

namespace gfd {

enum { M_VOX = 0, M_PTS, M_SKIP, M_OVER, M_GO, M_NRES, M_NAN, M_TOTAL, VM_META };

struct VmDev {
  unsigned long long *keys;
  int *cnt;
  double *pts;
  int mask, P, cap;
  int *meta;
};

// ---- the probes of an open-addressing table of packed keys (linear probing, VM_EMPTY = free): of the voxel map, and of the scan
// handle's one-point-per-voxel table (keys and mask are all they read)
__device__ __forceinline__ unsigned long long vm_load_key(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// slot of `key`, or -1 (bounded by the table size: a probe sequence always meets a free slot, the bound only guards a corrupted table)
__device__ __forceinline__ int vm_find(const VmDev &V, unsigned long long key) {
  int h = (int)(vmap_hash(key) & (unsigned long long)V.mask);
  for (int probe = 0; probe <= V.mask; probe++) {
    const unsigned long long k = V.keys[h];
    if (k == key) return h;
    if (k == VM_EMPTY) return -1;
    h = (h + 1) & V.mask;
  }
  return -1;
}
// slot of `key`, claiming a free one when absent (*fresh); -1 only for a full table, which the capacity rule excludes
__device__ __forceinline__ int vm_claim(const VmDev &V, unsigned long long key, bool *fresh) {
  int h = (int)(vmap_hash(key) & (unsigned long long)V.mask);
  *fresh = false;
  for (int probe = 0; probe <= V.mask; probe++) {
    unsigned long long k = vm_load_key(V.keys + h);
    if (k == VM_EMPTY) {
      k = atomicCAS(V.keys + h, (unsigned long long)VM_EMPTY, key);
      if (k == VM_EMPTY) { *fresh = true; return h; }
    }
    if (k == key) return h;
    h = (h + 1) & V.mask;
  }
  return -1;
}

// k_vm_assoc + k_vm_compact at the poses d_pb / d_pe; *d_skip != 0 (read on the device): both return at once
gfbe_status vmap_enqueue_assoc(gfbe_ctx *c, gfbe_vmap *m, int ct, int n, const double *d_raw, const double *d_alpha, const double *d_pb, const double *d_pe,
                               int frame_init, const int *d_skip);
// k_vm_local on the held normals: d_out4 = sv [3] | degenerate
void vmap_enqueue_local(gfbe_ctx *c, gfbe_vmap *m, double *d_out4);

// ---- a scan handle (gfbe_scan.hip) as the hand-over sees it: n rows [n][3] / [n] in device memory, n known to the host.
// GFBE_BAD_INPUT (message set): a handle of another context; keypoints: none of the scan as it is now. points: reads the count back
// (a wait) when an operation changed it since the host last saw it.
struct ScanView { int n; const double *pts, *alpha; };
gfbe_status scan_keypoints_view(gfbe_ctx *c, gfbe_scan *s, const char *who, ScanView *v);
gfbe_status scan_points_view(gfbe_ctx *c, gfbe_scan *s, const char *who, ScanView *v);

}  // namespace gfd
