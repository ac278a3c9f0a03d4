// gfbe_dmap.hip — the dense RGB-D map of the loop-closure thread held on the device: the keyframes' point lists, the 1 cm voxel
// table with its density cap, the cloud in insertion order and the radius outlier filter.
//
//   addKeyFrame   gate, density < 3, the keyframe's list shrunk to the survivors   dense_map/src/pose_graph.cpp:191-244   gfbe_dmap_add_keyframe
//   updatePath    the map thrown away and rebuilt at the corrected poses, < 5      :997-1032                              gfbe_dmap_rebuild
//   RadiusOutlierRemoval 0.8 m / 10 neighbours                                     :230-238, :1043-1051                   gfbe_dmap_filter
//
// Every count lives in device memory (meta); grids are sized by the host's upper bounds, every kernel reads the count it works on.
// Only gfbe_dmap_size, the downloads and gfbe_dmap_filter wait for the device.
//
// The density cap ("the first `cap` points of a voxel in list order") without a sequential walk: every candidate claims its voxel in
// the open-addressing table (vm_claim), then `cap` rounds of an integer atomicMin per slot: round r finds, per voxel, the lowest index
// among the candidates no earlier round picked, and only candidates with base + r < cap take part (base = the voxel's count before
// the call, which no kernel changes until the compaction). A round's value is index - (r + 1) 2^26, below every value of an earlier
// round, and the rounds alternate between two arrays: a round reads the finished array of the one before and posts into the other,
// so nothing is reset between rounds. The picked candidates are compacted in ascending index by a two-level scan; the voxel counts
// rise by integer atomicAdd. Nothing depends on the order workgroups ran in or on the slot a key landed in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"
#include "gfbe_dmap.h"
#include "gfbe_handle.h"
#include "gfbe_vmap.h"
#include "gfbe_vmap_impl.h"

using namespace gfd;

namespace {
enum { DM_NKF = 0, DM_NSTORED, DM_NCLOUD, DM_NVOX, DM_NSKIP, DM_NGATED, DM_NREFUSED, DM_N, DM_ROOM, DM_TOTAL, DM_PBASE, DM_CBASE, DM_FIT, DM_FAST, DM_META = 16 };
enum { DM_GATED = -2, DM_SKIPPED = -3, DM_REFUSED = -4 };
constexpr int DM_THREADS = 256, DM_SCAN_THREADS = 1024, DM_NONE = 0x7F7F7F7F, DM_MAX_POINTS = 1 << 26;
}  // namespace

struct gfbe_dmap : gfbe_handle {
  gfbe_dmap_options opt;
  int pcap = 0, kcap = 0, slots = 0;
  // the keyframes' lists: one pool in keyframe order then list order
  float *pool_xyz = nullptr;              // [pcap][3] camera frame
  uint8_t *pool_rgb = nullptr;            // [pcap][3]
  int *pool_kf = nullptr;                 // [pcap] keyframe of a pool point
  int *kf_tab = nullptr;                  // [kcap][2] begin, count
  // the map: voxel table and the cloud in insertion order
  unsigned long long *keys = nullptr;     // [slots]
  int *cnt = nullptr;                     // [slots] points of the voxel
  float *cl_xyz = nullptr;                // [pcap][3] world
  uint8_t *cl_rgb = nullptr;
  int *cl_kf = nullptr, *cl_src = nullptr;
  // one call's candidates
  int *rank_min[2] = {};                  // [slots] the rounds' minima (DM_NONE between calls)
  int *slot_of = nullptr, *won = nullptr; // [pcap]
  float *cand = nullptr;                  // [pcap][3] world float of a candidate
  int *part = nullptr;                    // [slots / 256 + 2]
  double *rp = nullptr, *rp_ic = nullptr; // [kcap][12] R | P of the call's poses, [12] of ex_cam
  double *pose_d = nullptr, *pose_h = nullptr;      // [kcap][7] the poses of a rebuild, device and pinned host
  hipEvent_t ev_pose = nullptr;
  bool pose_busy = false;
  // the filter
  unsigned long long *ckeys = nullptr;    // [slots] coarse cells
  int *ccnt = nullptr, *cstart = nullptr, *cfill = nullptr;      // [slots]
  int *cslot = nullptr, *keep_i = nullptr;                      // [pcap]
  float *sorted = nullptr, *out_xyz = nullptr;                  // [pcap][3]
  uint8_t *keep_b = nullptr, *out_rgb = nullptr;                // [pcap], [pcap][3]
  int *meta = nullptr;                    // [DM_META]
  int n_kf = 0;                           // exact: every accepted gfbe_dmap_add_keyframe adds one keyframe
  long long bound_stored = 0, bound_cloud = 0;      // the host's upper bounds of the device counts
};

namespace {

__device__ __forceinline__ int dm_enc(int i, int round) { return i - ((round + 1) << 26); }

__global__ void k_dm_poses(int n, const double *pose7, double *rp) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) dmap_pose_rp(pose7 + 7 * (size_t)k, rp + 12 * (size_t)k);
}

// the call's counts: insert (mode 0) n candidates into the room the pool has left; rebuild (mode 1) every pool point into an empty map
__global__ void k_dm_begin(int *meta, int mode, int n, int pcap, int kcap) {
  if (threadIdx.x || blockIdx.x) return;
  if (mode == 0) {
    meta[DM_N] = n;
    meta[DM_ROOM] = meta[DM_NKF] < kcap ? pcap - meta[DM_NSTORED] : 0;
    meta[DM_PBASE] = meta[DM_NSTORED]; meta[DM_CBASE] = meta[DM_NCLOUD];
  } else {
    meta[DM_N] = meta[DM_NSTORED];
    meta[DM_ROOM] = pcap; meta[DM_PBASE] = 0; meta[DM_CBASE] = 0; meta[DM_NVOX] = 0; meta[DM_NCLOUD] = 0;
  }
}
__global__ void k_dm_refuse_all(int *meta, int n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) meta[DM_NREFUSED] += n;
}

struct DmPoint { double origin, resolution, z_min, z_max; int cap; };

// world point, gate, key, claim; round 0 of the rank
__global__ __launch_bounds__(DM_THREADS) void k_dm_point(const int *meta, int mode, DmPoint O, const double *rp, const double *rp_ic, const float *pts, const int *pool_kf,
                                                         VmDev T, int *min0, int *slot_of, int *won, float *cand) {
  const int i = blockIdx.x * DM_THREADS + threadIdx.x;
  if (i >= meta[DM_N]) return;
  won[i] = 0;
  if (meta[DM_ROOM] <= 0) { slot_of[i] = DM_REFUSED; return; }
  double pw[3];
  dmap_world(rp + (mode ? 12 * (size_t)pool_kf[i] : 0), rp_ic, pts + 3 * (size_t)i, pw);
  if (mode == 0 && dmap_gated(pw[2], O.z_min, O.z_max)) { slot_of[i] = DM_GATED; return; }
  const float pf[3] = {(float)pw[0], (float)pw[1], (float)pw[2]};
  uint64_t key;
  if (!dmap_key(pf, O.origin, O.resolution, &key)) { slot_of[i] = DM_SKIPPED; return; }
  bool fresh;
  const int s = vm_claim(T, key, &fresh);      // (never -1: at most 2 point_capacity - 1 keys in >= 2 point_capacity slots)
  if (s < 0) { slot_of[i] = DM_REFUSED; return; }
  for (int a = 0; a < 3; a++) cand[3 * (size_t)i + a] = pf[a];
  slot_of[i] = s;
  if (T.cnt[s] < O.cap) atomicMin(min0 + s, dm_enc(i, 0));
}
// round r >= 1: who won round r - 1 (its array is final), the others post into this round's array while base + r < cap
__global__ __launch_bounds__(DM_THREADS) void k_dm_rank(const int *meta, int r, int cap, const int *slot_of, const int *cnt, const int *min_prev, int *min_cur, int *won) {
  const int i = blockIdx.x * DM_THREADS + threadIdx.x;
  if (i >= meta[DM_N]) return;
  const int s = slot_of[i];
  if (s < 0 || won[i]) return;
  if (min_prev[s] == dm_enc(i, r - 1)) { won[i] = 1; return; }
  if (cnt[s] + r < cap) atomicMin(min_cur + s, dm_enc(i, r));
}
// the winners of the last round; first level of the scan: the picked candidates of each workgroup; the dropped ones by reason
__global__ __launch_bounds__(DM_THREADS) void k_dm_flags(int *meta, int last, const int *slot_of, const int *min_last, int *won, int *part) {
  __shared__ int lds[20];
  const int i = blockIdx.x * DM_THREADS + threadIdx.x;
  int keep = 0, cls = 0, tk, tc;
  if (i < meta[DM_N]) {
    const int s = slot_of[i];
    if (s >= 0) { keep = won[i] || min_last[s] == dm_enc(i, last); won[i] = keep; }
    else cls = s == DM_GATED ? 1 : s == DM_SKIPPED ? 1 << 10 : 1 << 20;
  }
  (void)block_exclusive_scan<DM_THREADS>(keep, &tk, lds);
  (void)block_exclusive_scan<DM_THREADS>(cls, &tc, lds);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = tk;
    if (tc & 1023) atomicAdd(meta + DM_NGATED, tc & 1023);
    if ((tc >> 10) & 1023) atomicAdd(meta + DM_NSKIP, (tc >> 10) & 1023);
    if (tc >> 20) atomicAdd(meta + DM_NREFUSED, tc >> 20);
  }
}
// first level of a scan over int values (the coarse cells' counts)
__global__ __launch_bounds__(DM_THREADS) void k_dm_partial(int n, const int *val, int *part) {
  __shared__ int lds[20];
  const int i = blockIdx.x * DM_THREADS + threadIdx.x;
  int t;
  (void)block_exclusive_scan<DM_THREADS>(i < n ? val[i] : 0, &t, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
// second level: one workgroup turns the G counts into offsets, every thread a contiguous chunk of them; the total into meta
__global__ __launch_bounds__(DM_SCAN_THREADS) void k_dm_offsets(int *meta, int G, int *part) {
  __shared__ int lds[20];
  const int t = threadIdx.x, chunk = (G + DM_SCAN_THREADS - 1) / DM_SCAN_THREADS, b0 = min(G, t * chunk), b1 = min(G, b0 + chunk);
  int mine = 0, total;
  for (int b = b0; b < b1; b++) mine += part[b];
  int run = block_exclusive_scan<DM_SCAN_THREADS>(mine, &total, lds);
  for (int b = b0; b < b1; b++) { const int c = part[b]; part[b] = run; run += c; }
  if (t == 0) meta[DM_TOTAL] = total;
}
// what fits is kept, in order; the rest is counted
__global__ void k_dm_commit(int *meta, int mode, int *kf_tab) {
  if (threadIdx.x || blockIdx.x) return;
  const int total = meta[DM_TOTAL], fit = min(total, max(meta[DM_ROOM], 0));
  meta[DM_FIT] = fit;
  meta[DM_NREFUSED] += total - fit;
  if (mode == 0) {
    const int k = meta[DM_NKF];
    kf_tab[2 * k] = meta[DM_NSTORED]; kf_tab[2 * k + 1] = fit;
    meta[DM_NKF] = k + 1; meta[DM_NSTORED] += fit; meta[DM_NCLOUD] += fit;
  } else {
    meta[DM_NCLOUD] = fit;
  }
}

struct DmStore {
  float *pool_xyz; uint8_t *pool_rgb; int *pool_kf;
  float *cl_xyz; uint8_t *cl_rgb; int *cl_kf, *cl_src;
};
// the picked candidates in ascending index: appended to the cloud and (insert) to the pool; the voxel counts; the rank arrays cleaned
__global__ __launch_bounds__(DM_THREADS) void k_dm_compact(int *meta, int mode, const int *slot_of, const int *won, const int *part, const float *cand,
                                                           const float *in_pts, const uint8_t *in_rgb, DmStore S, int *cnt, int *min0, int *min1) {
  __shared__ int lds[20];
  const int i = blockIdx.x * DM_THREADS + threadIdx.x, n = meta[DM_N];
  const int s = i < n ? slot_of[i] : -1, keep = s >= 0 && won[i];
  int tk, tf, fresh = 0;
  const int dst = part[blockIdx.x] + block_exclusive_scan<DM_THREADS>(keep, &tk, lds);
  if (s >= 0) { min0[s] = DM_NONE; min1[s] = DM_NONE; }
  if (keep && dst < meta[DM_FIT]) {
    const size_t c = (size_t)meta[DM_CBASE] + dst;
    const uint8_t *rgb = (mode ? S.pool_rgb : in_rgb) + 3 * (size_t)i;
    for (int a = 0; a < 3; a++) { S.cl_xyz[3 * c + a] = cand[3 * (size_t)i + a]; S.cl_rgb[3 * c + a] = rgb[a]; }
    if (mode == 0) {
      const size_t p = (size_t)meta[DM_PBASE] + dst;
      const int k = meta[DM_NKF] - 1;      // (k_dm_commit counted the new keyframe)
      for (int a = 0; a < 3; a++) { S.pool_xyz[3 * p + a] = in_pts[3 * (size_t)i + a]; S.pool_rgb[3 * p + a] = rgb[a]; }
      S.pool_kf[p] = k; S.cl_kf[c] = k; S.cl_src[c] = (int)p;
    } else {
      S.cl_kf[c] = S.pool_kf[i]; S.cl_src[c] = i;
    }
    fresh = atomicAdd(cnt + s, 1) == 0;
  }
  (void)block_exclusive_scan<DM_THREADS>(fresh, &tf, lds);
  if (threadIdx.x == 0 && tf) atomicAdd(meta + DM_NVOX, tf);
}

// ---- the radius filter
__global__ __launch_bounds__(DM_THREADS) void k_df_cell(const int *meta, const float *xyz, double side, VmDev C, int *cslot) {
  const int i = blockIdx.x * DM_THREADS + threadIdx.x;
  if (i >= meta[DM_NCLOUD]) return;
  int c[3];
  dmap_cell(xyz + 3 * (size_t)i, side, c);
  bool fresh;
  const int s = vm_claim(C, dmap_pack(c[0], c[1], c[2]), &fresh);
  cslot[i] = s;
  if (s >= 0) atomicAdd(C.cnt + s, 1);
}
__global__ __launch_bounds__(DM_THREADS) void k_df_starts(int n, const int *ccnt, const int *part, int *cstart, int *cfill) {
  __shared__ int lds[20];
  const int j = blockIdx.x * DM_THREADS + threadIdx.x;
  int t;
  const int at = part[blockIdx.x] + block_exclusive_scan<DM_THREADS>(j < n ? ccnt[j] : 0, &t, lds);
  if (j < n) { cstart[j] = at; cfill[j] = 0; }
}
// the points grouped by cell (the order inside a cell is free: the filter's outcome is a count)
__global__ __launch_bounds__(DM_THREADS) void k_df_scatter(const int *meta, const float *xyz, const int *cslot, const int *cstart, int *cfill, float *sorted) {
  const int i = blockIdx.x * DM_THREADS + threadIdx.x;
  if (i >= meta[DM_NCLOUD]) return;
  const int s = cslot[i];
  if (s < 0) return;
  const size_t pos = (size_t)cstart[s] + atomicAdd(cfill + s, 1);
  for (int a = 0; a < 3; a++) sorted[3 * pos + a] = xyz[3 * (size_t)i + a];
}
// keep[i]: more than min_nb points (i itself counted) within the radius. A cell of more than min_nb points keeps all its points at
// once; every other point walks the 5^3 cells around its own and leaves at the count that decides.
__global__ __launch_bounds__(DM_THREADS) void k_df_decide(int *meta, const float *xyz, const int *cslot, VmDev C, const int *cstart, const float *sorted, double side,
                                                          double r2, int min_nb, int *keep_i, uint8_t *keep_b, int *part) {
  __shared__ int lds[20];
  const int i = blockIdx.x * DM_THREADS + threadIdx.x;
  int keep = 0, fast = 0, tk, tf;
  if (i < meta[DM_NCLOUD]) {
    const int s = cslot[i];
    const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    if (s >= 0 && C.cnt[s] > min_nb) { keep = 1; fast = 1; }
    else {
      int c[3], count = 0;
      dmap_cell(p, side, c);
      for (int dz = -2; dz <= 2 && !keep; dz++)
        for (int dy = -2; dy <= 2 && !keep; dy++)
          for (int dx = -2; dx <= 2 && !keep; dx++) {
            const int j = (dx | dy | dz) == 0 ? s : vm_find(C, dmap_pack(c[0] + dx, c[1] + dy, c[2] + dz));
            if (j < 0) continue;
            const int q0 = cstart[j], q1 = q0 + C.cnt[j];
            for (int q = q0; q < q1; q++)
              if (dmap_sqdist(p, sorted + 3 * (size_t)q) <= r2 && ++count > min_nb) { keep = 1; break; }
          }
    }
    keep_i[i] = keep; keep_b[i] = (uint8_t)keep;
  }
  (void)block_exclusive_scan<DM_THREADS>(keep, &tk, lds);
  (void)block_exclusive_scan<DM_THREADS>(fast, &tf, lds);
  if (threadIdx.x == 0) { part[blockIdx.x] = tk; if (tf) atomicAdd(meta + DM_FAST, tf); }
}
__global__ __launch_bounds__(DM_THREADS) void k_df_compact(const int *meta, const int *keep_i, const int *part, const float *xyz, const uint8_t *rgb, float *out_xyz, uint8_t *out_rgb) {
  __shared__ int lds[20];
  const int i = blockIdx.x * DM_THREADS + threadIdx.x;
  const int keep = i < meta[DM_NCLOUD] ? keep_i[i] : 0;
  int tk;
  const size_t dst = (size_t)part[blockIdx.x] + block_exclusive_scan<DM_THREADS>(keep, &tk, lds);
  if (!keep) return;
  for (int a = 0; a < 3; a++) { out_xyz[3 * dst + a] = xyz[3 * (size_t)i + a]; out_rgb[3 * dst + a] = rgb[3 * (size_t)i + a]; }
}
__global__ void k_df_begin(int *meta) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { meta[DM_FAST] = 0; meta[DM_TOTAL] = 0; }
}

gfbe_status dm_ready(gfbe_ctx *c, gfbe_dmap *m, const char *who) { return handle_ready(c, m, who, "map handle"); }
bool dm_finite(const double *p, size_t n) {
  for (size_t a = 0; a < n; a++) if (!std::isfinite(p[a])) return false;
  return true;
}
const char *dm_options_error(const gfbe_dmap_options *o) {
  if (o->struct_size != (int32_t)sizeof(gfbe_dmap_options)) return "gfbe_dmap_options.struct_size does not match this library (ABI mismatch)";
  if (o->add_cap < 1 || o->add_cap > DM_MAX_CAP || o->rebuild_cap < 1 || o->rebuild_cap > DM_MAX_CAP) return "add_cap / rebuild_cap outside 1 .. 8";
  if (o->filter_min_neighbors < 0) return "filter_min_neighbors < 0";
  if (!dm_finite(&o->resolution, 4) || !dm_finite(o->ex_cam, 7) || !(o->resolution > 0.0) || !(o->z_min <= o->z_max)) return "resolution, origin, gates and ex_cam must be finite, resolution > 0";
  if (!dmap_cells_fit(o->origin, o->resolution, o->filter_radius)) return "filter_radius must be finite, > 0 and large enough for the coarse grid to cover the voxel box";
  return nullptr;
}
int dm_grid(long long n) { return (int)((n + DM_THREADS - 1) / DM_THREADS); }

// rank rounds 1 .. cap - 1, the two-level scan, the commit and the compaction of a call whose k_dm_point ran on G workgroups
void dm_enqueue_cap(gfbe_ctx *c, gfbe_dmap *m, int mode, int cap, int G, const float *in_pts, const uint8_t *in_rgb) {
  hipStream_t st = ctx_stream(c);
  if (G > 0) {
    for (int r = 1; r < cap; r++)
      hipLaunchKernelGGL(k_dm_rank, dim3(G), dim3(DM_THREADS), 0, st, (const int *)m->meta, r, cap, (const int *)m->slot_of, (const int *)m->cnt,
                         (const int *)m->rank_min[(r - 1) & 1], m->rank_min[r & 1], m->won);
    hipLaunchKernelGGL(k_dm_flags, dim3(G), dim3(DM_THREADS), 0, st, m->meta, cap - 1, (const int *)m->slot_of, (const int *)m->rank_min[(cap - 1) & 1], m->won, m->part);
  }
  hipLaunchKernelGGL(k_dm_offsets, dim3(1), dim3(DM_SCAN_THREADS), 0, st, m->meta, G, m->part);
  hipLaunchKernelGGL(k_dm_commit, dim3(1), dim3(1), 0, st, m->meta, mode, m->kf_tab);
  if (G > 0)
    hipLaunchKernelGGL(k_dm_compact, dim3(G), dim3(DM_THREADS), 0, st, m->meta, mode, (const int *)m->slot_of, (const int *)m->won, (const int *)m->part,
                       (const float *)m->cand, in_pts, in_rgb, DmStore{m->pool_xyz, m->pool_rgb, m->pool_kf, m->cl_xyz, m->cl_rgb, m->cl_kf, m->cl_src}, m->cnt,
                       m->rank_min[0], m->rank_min[1]);
}
DmPoint dm_point_args(const gfbe_dmap *m, int cap) { return DmPoint{m->opt.origin, m->opt.resolution, m->opt.z_min, m->opt.z_max, cap}; }

gfbe_status dm_read_meta(gfbe_ctx *c, gfbe_dmap *m, int *h) {
  GFBE_CHECK(c, hipMemcpyAsync(h, m->meta, sizeof(int) * DM_META, hipMemcpyDeviceToHost, ctx_stream(c)));
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  m->bound_stored = h[DM_NSTORED]; m->bound_cloud = h[DM_NCLOUD];
  return GFBE_OK;
}

}  // namespace

extern "C" {

void gfbe_dmap_default_options(gfbe_dmap_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = (int32_t)sizeof *o;
  o->add_cap = 3; o->rebuild_cap = 5; o->filter_min_neighbors = 10;
  o->resolution = 0.01; o->origin = -10000.0; o->z_min = -0.5; o->z_max = 2.0;
  o->ex_cam[6] = 1.0;
  o->filter_radius = 0.8;
}

void gfbe_dmap_destroy(gfbe_ctx *c, gfbe_dmap *m) {
  if (!m) return;
  m->release(c);
  delete m;
}

gfbe_status gfbe_dmap_create(gfbe_ctx *c, int32_t point_capacity, int32_t keyframe_capacity, const gfbe_dmap_options *opt, gfbe_dmap **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  gfbe_dmap_options o;
  if (opt) o = *opt; else gfbe_dmap_default_options(&o);
  if (opt && opt->struct_size != (int32_t)sizeof(gfbe_dmap_options)) { ctx_set_error(c, "gfbe_dmap_create: gfbe_dmap_options.struct_size does not match this library (ABI mismatch)"); return GFBE_BAD_INPUT; }
  if (const char *bad = dm_options_error(&o)) { ctx_set_error(c, (std::string("gfbe_dmap_create: ") + bad).c_str()); return GFBE_BAD_INPUT; }
  if (point_capacity < 1 || point_capacity > DM_MAX_POINTS || keyframe_capacity < 1 || keyframe_capacity > (1 << 24)) {
    ctx_set_error(c, "gfbe_dmap_create: point_capacity outside 1 .. 2^26 or keyframe_capacity outside 1 .. 2^24");
    return GFBE_BAD_INPUT;
  }
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_dmap_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  gfbe_dmap *m = new gfbe_dmap();
  CreateGuard<gfbe_dmap> guard{c, m, gfbe_dmap_destroy};
  m->owner = c; m->opt = o; m->pcap = point_capacity; m->kcap = keyframe_capacity;
  long long slots = 64;
  while (slots < 2ll * point_capacity) slots <<= 1;
  m->slots = (int)slots;
  const size_t N = (size_t)point_capacity, K = (size_t)keyframe_capacity, S = (size_t)slots;
  hipStream_t st = ctx_stream(c);
  bool ok = m->alloc(&m->pool_xyz, 3 * N, 0) && m->alloc(&m->pool_rgb, 3 * N, 0) && m->alloc(&m->pool_kf, N, 0) && m->alloc(&m->kf_tab, 2 * K, 0) && m->alloc(&m->keys, S, 0xFF) &&
            m->alloc(&m->cnt, S, 0) && m->alloc(&m->cl_xyz, 3 * N, 0) && m->alloc(&m->cl_rgb, 3 * N, 0) && m->alloc(&m->cl_kf, N, 0) && m->alloc(&m->cl_src, N, 0) &&
            m->alloc(&m->rank_min[0], S, 0x7F) && m->alloc(&m->rank_min[1], S, 0x7F) && m->alloc(&m->slot_of, N, 0) && m->alloc(&m->won, N, 0) && m->alloc(&m->cand, 3 * N, 0) &&
            m->alloc(&m->part, S / DM_THREADS + 2, 0) && m->alloc(&m->rp, 12 * K, 0) && m->alloc(&m->rp_ic, (size_t)12, 0) && m->alloc(&m->pose_d, 7 * K, 0) &&
            m->alloc(&m->ckeys, S, 0xFF) && m->alloc(&m->ccnt, S, 0) && m->alloc(&m->cstart, S, 0) && m->alloc(&m->cfill, S, 0) && m->alloc(&m->cslot, N, 0) && m->alloc(&m->keep_i, N, 0) &&
            m->alloc(&m->sorted, 3 * N, 0) && m->alloc(&m->out_xyz, 3 * N, 0) && m->alloc(&m->keep_b, N, 0) && m->alloc(&m->out_rgb, 3 * N, 0) && m->alloc(&m->meta, (size_t)DM_META, 0);
  if (!ok) { ctx_set_error(c, "gfbe_dmap_create: device allocation failed"); return GFBE_DEVICE_ERROR; }
  if (!m->alloc_pinned(&m->pose_h, 7 * K) || !m->create(&m->ev_pose) || !m->make_staging(c, "gfbe_dmap_create", 1 << 16, true)) return GFBE_DEVICE_ERROR;
  {
    Staged sg(c, m, 1024);
    const double *dex = sg.up(o.ex_cam, 7);
    if (!sg.ok) { ctx_set_error(c, "gfbe_dmap_create: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    hipLaunchKernelGGL(k_dm_poses, dim3(1), dim3(64), 0, st, 1, dex, m->rp_ic);
  }
  GFBE_CHECK(c, hipStreamSynchronize(st));
  GFBE_CHECK(c, hipGetLastError());
  guard.armed = false;
  *out = m;
  return GFBE_OK;
}

gfbe_status gfbe_dmap_add_keyframe(gfbe_ctx *c, gfbe_dmap *m, const double *pose7, int32_t n, const float *pts_cam, const uint8_t *rgb) {
  gfbe_status rc = dm_ready(c, m, "gfbe_dmap_add_keyframe");
  if (rc != GFBE_OK) return rc;
  if (!pose7 || n < 0 || (n > 0 && (!pts_cam || !rgb))) return GFBE_BAD_INPUT;
  if (n > m->pcap) { ctx_set_error(c, "gfbe_dmap_add_keyframe: more points in one call than point_capacity"); return GFBE_BAD_INPUT; }
  if (!dm_finite(pose7, 7)) { ctx_set_error(c, "gfbe_dmap_add_keyframe: the pose is not finite"); return GFBE_BAD_INPUT; }
  hipStream_t st = ctx_stream(c);
  if (m->n_kf >= m->kcap) {      // the keyframe table is full: the whole call is refused and counted
    hipLaunchKernelGGL(k_dm_refuse_all, dim3(1), dim3(1), 0, st, m->meta, (int)n);
    GFBE_CHECK(c, hipGetLastError());
    return GFBE_OK;
  }
  const size_t N = (size_t)n;
  {
    Staged sg(c, m, N * 15 + 2048, /*defer=*/true);
    const float *dp = sg.up(pts_cam, 3 * N);
    const uint8_t *dc = sg.up(rgb, 3 * N);
    const double *dpose = sg.up(pose7, 7);
    if (!sg.ok) { ctx_set_error(c, "gfbe_dmap_add_keyframe: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    const int G = dm_grid(n);
    hipLaunchKernelGGL(k_dm_poses, dim3(1), dim3(64), 0, st, 1, dpose, m->rp);
    hipLaunchKernelGGL(k_dm_begin, dim3(1), dim3(1), 0, st, m->meta, 0, (int)n, m->pcap, m->kcap);
    const VmDev T{m->keys, m->cnt, nullptr, m->slots - 1, 0, 0, nullptr};
    if (G > 0)
      hipLaunchKernelGGL(k_dm_point, dim3(G), dim3(DM_THREADS), 0, st, (const int *)m->meta, 0, dm_point_args(m, m->opt.add_cap), (const double *)m->rp,
                         (const double *)m->rp_ic, dp, (const int *)m->pool_kf, T, m->rank_min[0], m->slot_of, m->won, m->cand);
    dm_enqueue_cap(c, m, 0, m->opt.add_cap, G, dp, dc);
  }
  m->n_kf++;
  m->bound_stored = std::min<long long>(m->pcap, m->bound_stored + n);
  m->bound_cloud = std::min<long long>(m->pcap, m->bound_cloud + n);
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_dmap_rebuild(gfbe_ctx *c, gfbe_dmap *m, int32_t n_keyframes, const double *pose7) {
  gfbe_status rc = dm_ready(c, m, "gfbe_dmap_rebuild");
  if (rc != GFBE_OK) return rc;
  if (n_keyframes != m->n_kf) { ctx_set_error(c, "gfbe_dmap_rebuild: n_keyframes is not the number of keyframes held"); return GFBE_BAD_INPUT; }
  if (n_keyframes > 0 && !pose7) return GFBE_BAD_INPUT;
  if (!dm_finite(pose7, 7 * (size_t)n_keyframes)) { ctx_set_error(c, "gfbe_dmap_rebuild: a pose is not finite"); return GFBE_BAD_INPUT; }
  hipStream_t st = ctx_stream(c);
  const size_t K = (size_t)n_keyframes;
  if (m->pose_busy) GFBE_CHECK(c, hipEventSynchronize(m->ev_pose));      // (the pinned mirror of the last rebuild's poses: long copied by now)
  if (K) {
    std::memcpy(m->pose_h, pose7, sizeof(double) * 7 * K);
    GFBE_CHECK(c, hipMemcpyAsync(m->pose_d, m->pose_h, sizeof(double) * 7 * K, hipMemcpyHostToDevice, st));
    GFBE_CHECK(c, hipEventRecord(m->ev_pose, st));
    m->pose_busy = true;
    hipLaunchKernelGGL(k_dm_poses, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, (int)K, (const double *)m->pose_d, m->rp);
  }
  GFBE_CHECK(c, hipMemsetAsync(m->keys, 0xFF, sizeof(unsigned long long) * (size_t)m->slots, st));
  GFBE_CHECK(c, hipMemsetAsync(m->cnt, 0, sizeof(int) * (size_t)m->slots, st));
  hipLaunchKernelGGL(k_dm_begin, dim3(1), dim3(1), 0, st, m->meta, 1, 0, m->pcap, m->kcap);
  const int G = dm_grid(m->bound_stored);
  const VmDev T{m->keys, m->cnt, nullptr, m->slots - 1, 0, 0, nullptr};
  if (G > 0)
    hipLaunchKernelGGL(k_dm_point, dim3(G), dim3(DM_THREADS), 0, st, (const int *)m->meta, 1, dm_point_args(m, m->opt.rebuild_cap), (const double *)m->rp,
                       (const double *)m->rp_ic, (const float *)m->pool_xyz, (const int *)m->pool_kf, T, m->rank_min[0], m->slot_of, m->won, m->cand);
  dm_enqueue_cap(c, m, 1, m->opt.rebuild_cap, G, nullptr, nullptr);
  m->bound_cloud = m->bound_stored;
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_dmap_filter(gfbe_ctx *c, gfbe_dmap *m, uint8_t *keep, int32_t *n_keep, float *xyz_out, uint8_t *rgb_out) {
  gfbe_status rc = dm_ready(c, m, "gfbe_dmap_filter");
  if (rc != GFBE_OK) return rc;
  if ((xyz_out == nullptr) != (rgb_out == nullptr)) { ctx_set_error(c, "gfbe_dmap_filter: xyz_out and rgb_out go together"); return GFBE_BAD_INPUT; }
  hipStream_t st = ctx_stream(c);
  const int G = dm_grid(m->bound_cloud);
  int used = 64;      // a cell table of 2^k >= 2 n slots of the handle's
  while (used < 2 * m->bound_cloud && used < m->slots) used <<= 1;
  const int GS = dm_grid(used);
  const double side = dmap_cell_side(m->opt.filter_radius), r2 = m->opt.filter_radius * m->opt.filter_radius;
  const VmDev C{m->ckeys, m->ccnt, nullptr, used - 1, 0, 0, nullptr};
  hipLaunchKernelGGL(k_df_begin, dim3(1), dim3(1), 0, st, m->meta);
  if (G > 0) {
    GFBE_CHECK(c, hipMemsetAsync(m->ckeys, 0xFF, sizeof(unsigned long long) * (size_t)used, st));
    GFBE_CHECK(c, hipMemsetAsync(m->ccnt, 0, sizeof(int) * (size_t)used, st));
    hipLaunchKernelGGL(k_df_cell, dim3(G), dim3(DM_THREADS), 0, st, (const int *)m->meta, (const float *)m->cl_xyz, side, C, m->cslot);
    hipLaunchKernelGGL(k_dm_partial, dim3(GS), dim3(DM_THREADS), 0, st, used, (const int *)m->ccnt, m->part);
    hipLaunchKernelGGL(k_dm_offsets, dim3(1), dim3(DM_SCAN_THREADS), 0, st, m->meta, GS, m->part);
    hipLaunchKernelGGL(k_df_starts, dim3(GS), dim3(DM_THREADS), 0, st, used, (const int *)m->ccnt, (const int *)m->part, m->cstart, m->cfill);
    hipLaunchKernelGGL(k_df_scatter, dim3(G), dim3(DM_THREADS), 0, st, (const int *)m->meta, (const float *)m->cl_xyz, (const int *)m->cslot, (const int *)m->cstart,
                       m->cfill, m->sorted);
    hipLaunchKernelGGL(k_df_decide, dim3(G), dim3(DM_THREADS), 0, st, m->meta, (const float *)m->cl_xyz, (const int *)m->cslot, C, (const int *)m->cstart,
                       (const float *)m->sorted, side, r2, (int)m->opt.filter_min_neighbors, m->keep_i, m->keep_b, m->part);
    hipLaunchKernelGGL(k_dm_offsets, dim3(1), dim3(DM_SCAN_THREADS), 0, st, m->meta, G, m->part);
    if (xyz_out)
      hipLaunchKernelGGL(k_df_compact, dim3(G), dim3(DM_THREADS), 0, st, (const int *)m->meta, (const int *)m->keep_i, (const int *)m->part, (const float *)m->cl_xyz,
                         (const uint8_t *)m->cl_rgb, m->out_xyz, m->out_rgb);
  }
  GFBE_CHECK(c, hipGetLastError());
  int h[DM_META];
  if ((rc = dm_read_meta(c, m, h)) != GFBE_OK) return rc;      // the host wait: the counts
  const size_t n = (size_t)h[DM_NCLOUD], nk = (size_t)h[DM_TOTAL];
  if (n_keep) *n_keep = (int32_t)nk;
  if (keep && n) GFBE_CHECK(c, hipMemcpyAsync(keep, m->keep_b, n, hipMemcpyDeviceToHost, st));
  if (xyz_out && nk) {
    GFBE_CHECK(c, hipMemcpyAsync(xyz_out, m->out_xyz, sizeof(float) * 3 * nk, hipMemcpyDeviceToHost, st));
    GFBE_CHECK(c, hipMemcpyAsync(rgb_out, m->out_rgb, 3 * nk, hipMemcpyDeviceToHost, st));
  }
  GFBE_CHECK(c, hipStreamSynchronize(st));
  return GFBE_OK;
}

gfbe_status gfbe_dmap_size(gfbe_ctx *c, gfbe_dmap *m, int32_t *counts) {
  gfbe_status rc = dm_ready(c, m, "gfbe_dmap_size");
  if (rc != GFBE_OK) return rc;
  int h[DM_META];
  if ((rc = dm_read_meta(c, m, h)) != GFBE_OK) return rc;
  if (counts) {
    for (int a = 0; a < GFBE_DMAP_N_COUNTS - 1; a++) counts[a] = h[a];
    counts[GFBE_DMAP_N_COUNTS - 1] = h[DM_FAST];
  }
  return GFBE_OK;
}

gfbe_status gfbe_dmap_download_cloud(gfbe_ctx *c, gfbe_dmap *m, float *xyz, uint8_t *rgb, int32_t *kf, int32_t *src) {
  gfbe_status rc = dm_ready(c, m, "gfbe_dmap_download_cloud");
  if (rc != GFBE_OK) return rc;
  int h[DM_META];
  if ((rc = dm_read_meta(c, m, h)) != GFBE_OK) return rc;
  const size_t n = (size_t)h[DM_NCLOUD];
  if (n == 0) return GFBE_OK;
  hipStream_t st = ctx_stream(c);
  if (xyz) GFBE_CHECK(c, hipMemcpyAsync(xyz, m->cl_xyz, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, st));
  if (rgb) GFBE_CHECK(c, hipMemcpyAsync(rgb, m->cl_rgb, 3 * n, hipMemcpyDeviceToHost, st));
  if (kf) GFBE_CHECK(c, hipMemcpyAsync(kf, m->cl_kf, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  if (src) GFBE_CHECK(c, hipMemcpyAsync(src, m->cl_src, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  return GFBE_OK;
}

gfbe_status gfbe_dmap_download_keyframe(gfbe_ctx *c, gfbe_dmap *m, int32_t k, int32_t *n, float *pts, uint8_t *rgb) {
  gfbe_status rc = dm_ready(c, m, "gfbe_dmap_download_keyframe");
  if (rc != GFBE_OK) return rc;
  if (k < 0 || k >= m->n_kf) { ctx_set_error(c, "gfbe_dmap_download_keyframe: no such keyframe"); return GFBE_BAD_INPUT; }
  hipStream_t st = ctx_stream(c);
  int e[2];
  GFBE_CHECK(c, hipMemcpyAsync(e, m->kf_tab + 2 * (size_t)k, sizeof e, hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  if (n) *n = e[1];
  if (e[1] == 0 || (!pts && !rgb)) return GFBE_OK;
  if (pts) GFBE_CHECK(c, hipMemcpyAsync(pts, m->pool_xyz + 3 * (size_t)e[0], sizeof(float) * 3 * (size_t)e[1], hipMemcpyDeviceToHost, st));
  if (rgb) GFBE_CHECK(c, hipMemcpyAsync(rgb, m->pool_rgb + 3 * (size_t)e[0], 3 * (size_t)e[1], hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  return GFBE_OK;
}

}  // extern "C"
