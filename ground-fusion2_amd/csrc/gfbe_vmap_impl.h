// gfbe_vmap_impl.h — the voxel map handle (gfbe_vmap.hip) as the registration loop (gfbe_vreg.hip) sees it: the handle's
// fields, the device meta words and the launches of the association / localizability kernels on arguments already on the device.
#pragma once
#include <vector>

#include "gfbe.h"
#include "gfbe_device.h"      // gfbe_tab_staging, gfd::DevBuf

struct gfbe_vmap : gfbe_tab_staging {
  gfbe_vmap_options opt;
  int cap = 0, slots = 0, P = 0;
  unsigned long long *keys[2] = {};     // [slots]
  int *cnt[2] = {};                     // [slots]
  double *pts[2] = {};                  // [slots][P][3]
  int cur = 0;
  int *meta = nullptr;                  // [VM_META]
  int *part = nullptr;                  // [2][slots / 256] per-workgroup survivor counts of erase_far
  std::vector<void *> allocs;
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

// k_vm_assoc + k_vm_compact at the poses d_pb / d_pe; *d_skip != 0 (read on the device): both return at once
gfbe_status vmap_enqueue_assoc(gfbe_ctx *c, gfbe_vmap *m, int ct, int n, const double *d_raw, const double *d_alpha, const double *d_pb, const double *d_pe,
                               int frame_init, const int *d_skip);
// k_vm_local on the held normals: d_out4 = sv [3] | degenerate
void vmap_enqueue_local(gfbe_ctx *c, gfbe_vmap *m, double *d_out4);

}  // namespace gfd
