// gfbe_scan.hip — one LiDAR scan held on the device from the driver's cloud to the registration: what the reference does on the host
// between CloudConvert and lidarodom::optimize, and the hand-over of the result to gfbe_vmap_register_scan / gfbe_vmap_add_scan_handle.
//
//   subSampleFrame            lio/src/apps/main_eskf.cpp:56-64, common/utility.cpp:34-54       gfbe_scan_subsample
//   Undistort / PoseInterp    liw/lio/lidarodom.cpp:1578-1600, common/math_utils.h:530-585      gfbe_scan_undistort
//   transformPoint            lidarodom.cpp:1301-1304, common/utility.cpp:91-111                gfbe_scan_keypoints
//   gridSampling              lidarodom.cpp:503-505, common/utility.cpp:56-71                   gfbe_scan_keypoints
//
// The handle holds the points (IMU frame), alpha, the time stamp and the index in the uploaded cloud in a ping-pong pair, and the
// keypoints beside them. The point count lives in device memory (meta): no operation but keypoints / size / download waits for it;
// grids are sized by the count of the last upload, every kernel reads the count it works on.
//
// One point per voxel (subsample on the points, keypoints on the world points): an open-addressing table of 2^k >= 2 n slots
// (vmap_hash, the compare-and-swap claim of the voxel map) with an integer atomicMin of the point index per key; a point survives
// when it is the minimum of its voxel. Survivors are compacted in ascending index by a two-level scan (per workgroup, then one
// workgroup over the partial counts): the result depends neither on the order the workgroups ran in nor on the slot a key landed in.
// undistort: the states are staged in LDS once per workgroup, a point finds its segment by bisection there (gfbe_scan.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"
#include "gfbe_scan.h"
#include "gfbe_handle.h"
#include "gfbe_vmap.h"
#include "gfbe_vmap_impl.h"

using namespace gfd;

namespace {
enum { SM_N = 0, SM_NKP, SM_SKIP, SM_SKIPKP, SM_NOLD, SC_META = 8 };
constexpr int SC_THREADS = 256, SC_SCAN_THREADS = 1024;
}  // namespace

struct gfbe_scan : gfbe_handle {
  int cap = 0, slots = 0;
  int *src[2] = {};                       // [cap] index in the uploaded cloud
  double *pts[2] = {}, *alpha[2] = {}, *ts[2] = {};      // [cap][3], [cap], [cap]
  int cur = 0;
  int *kp_src = nullptr;
  double *kp_pts = nullptr, *kp_alpha = nullptr, *kp_ts = nullptr;
  unsigned long long *keys = nullptr;     // [slots]
  int *minidx = nullptr;                  // [slots] lowest point index of the voxel
  int *slot_of = nullptr;                 // [cap] slot of a point's voxel, -1: no voxel
  int *part = nullptr;                    // [2][cap / SC_THREADS + 1] survivors / dropped points per workgroup, then their offsets
  double *world = nullptr;                // [cap][3]
  int *meta = nullptr;                    // [SC_META]
  int n_up = 0;                           // the count of the last upload: the host's upper bound of the point count
  bool has_ts = false, kp_valid = false, counts_known = true;
  int n_pts = 0, n_kp = 0;                // the host's copy of the counts (counts_known)
};

namespace {

struct ScCols { int *src; double *pts, *alpha, *ts; };

// the uploaded cloud into the handle's columns; til: the lidar-to-IMU transform (NULL: the points as they are)
__global__ __launch_bounds__(SC_THREADS) void k_sc_ingest(int n, const double *raw, const double *alpha, const double *ts, const double *til, ScCols O, int *meta) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i == 0) { meta[SM_N] = n; meta[SM_NKP] = 0; meta[SM_SKIP] = 0; meta[SM_SKIPKP] = 0; meta[SM_NOLD] = n; }
  if (i >= n) return;
  const double *p = raw + 3 * (size_t)i;
  double q[3] = {p[0], p[1], p[2]};
  if (til) scan_til_point(til, p, q);
  for (int a = 0; a < 3; a++) O.pts[3 * (size_t)i + a] = q[a];
  O.src[i] = i; O.alpha[i] = alpha[i]; O.ts[i] = ts ? ts[i] : 0.0;
}

// Undistort: one thread per point, the states in LDS
__global__ __launch_bounds__(SC_THREADS) void k_sc_undistort(const int *meta, int ns, const double *st_time, const double *st_pose, double *pts, const double *ts) {
  __shared__ double s_t[SC_MAX_STATES], s_p[7 * SC_MAX_STATES];
  for (int q = threadIdx.x; q < ns; q += SC_THREADS) s_t[q] = st_time[q];
  for (int q = threadIdx.x; q < 7 * ns; q += SC_THREADS) s_p[q] = st_pose[q];
  __syncthreads();
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= meta[SM_N]) return;
  double Ti[7], out[3];
  int seg;
  const double p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
  scan_pose_at(ns, s_t, s_p, ts[i], &seg, Ti);
  scan_undistort_point(s_p + 7 * (ns - 1), Ti, p, out);
  for (int a = 0; a < 3; a++) pts[3 * (size_t)i + a] = out[a];
}

// transformPoint: the world point of every point of the handle (the body of k_vm_world)
__global__ __launch_bounds__(SC_THREADS) void k_sc_world(const int *meta, int ct, const double *raw, const double *alpha, const double *pb, const double *pe, double *out) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= meta[SM_N]) return;
  lio_world_store(i, ct, raw, alpha, pb, pe, out);
}

// the voxel of every point and the lowest index met in it
__global__ __launch_bounds__(SC_THREADS) void k_sc_claim(const int *meta, const double *p, double size, VmDev T, int *minidx, int *slot_of) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= meta[SM_N]) return;
  uint64_t key;
  int slot = -1;
  if (vmap_key(p + 3 * (size_t)i, size, &key)) {
    bool fresh;
    slot = vm_claim(T, key, &fresh);      // (never -1: the table has twice as many slots as there are points)
    if (slot >= 0) atomicMin(minidx + slot, i);
  }
  slot_of[i] = slot;
}
__device__ __forceinline__ void sc_flags(int i, int n, const int *slot_of, const int *minidx, int *keep, int *drop) {
  *keep = 0; *drop = 0;
  if (i >= n) return;
  const int s = slot_of[i];
  if (s < 0) *drop = 1; else *keep = minidx[s] == i;
}
// first level: survivors and dropped points of each workgroup
__global__ __launch_bounds__(SC_THREADS) void k_sc_count(const int *meta, const int *slot_of, const int *minidx, int G, int *part) {
  __shared__ int lds[20];
  int keep, drop, tk, td;
  sc_flags(blockIdx.x * SC_THREADS + threadIdx.x, meta[SM_N], slot_of, minidx, &keep, &drop);
  (void)block_exclusive_scan<SC_THREADS>(keep, &tk, lds);
  (void)block_exclusive_scan<SC_THREADS>(drop, &td, lds);
  if (threadIdx.x == 0) { part[blockIdx.x] = tk; part[G + blockIdx.x] = td; }
}
// second level: one workgroup turns the G counts into offsets and writes the totals. subsample: the points' count (the old one
// stays in SM_NOLD for the compaction), dropped points added; keypoints: the keypoint count, dropped points of this call.
__global__ __launch_bounds__(SC_SCAN_THREADS) void k_sc_offsets(int *meta, int G, int *part, int keypoints) {
  __shared__ int lds[20];
  const int t = threadIdx.x, chunk = (G + SC_SCAN_THREADS - 1) / SC_SCAN_THREADS, b0 = min(G, t * chunk), b1 = min(G, b0 + chunk);
  int mine = 0, drop = 0, total, tdrop;
  for (int b = b0; b < b1; b++) { mine += part[b]; drop += part[G + b]; }
  int run = block_exclusive_scan<SC_SCAN_THREADS>(mine, &total, lds);
  (void)block_exclusive_scan<SC_SCAN_THREADS>(drop, &tdrop, lds);
  for (int b = b0; b < b1; b++) { const int c = part[b]; part[b] = run; run += c; }
  if (t == 0) {
    if (keypoints) { meta[SM_NKP] = total; meta[SM_SKIPKP] = tdrop; }
    else { meta[SM_NOLD] = meta[SM_N]; meta[SM_N] = total; meta[SM_NKP] = 0; meta[SM_SKIP] += tdrop; meta[SM_SKIPKP] = 0; }
  }
}
// the survivors in ascending index order; n_word: where the count of the compacted list is (SM_NOLD after a subsample's k_sc_offsets)
__global__ __launch_bounds__(SC_THREADS) void k_sc_compact(const int *meta, int n_word, const int *slot_of, const int *minidx, const int *part, ScCols I, ScCols O) {
  __shared__ int lds[20];
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  int keep, drop, tk;
  sc_flags(i, meta[n_word], slot_of, minidx, &keep, &drop);
  const int dst = part[blockIdx.x] + block_exclusive_scan<SC_THREADS>(keep, &tk, lds);
  if (!keep) return;
  O.src[dst] = I.src[i]; O.alpha[dst] = I.alpha[i]; O.ts[dst] = I.ts[i];
  for (int a = 0; a < 3; a++) O.pts[3 * (size_t)dst + a] = I.pts[3 * (size_t)i + a];
}

gfbe_status sc_ready(gfbe_ctx *c, gfbe_scan *s, const char *who) { return handle_ready(c, s, who, "scan handle"); }
ScCols sc_cols(const gfbe_scan *s, int half) { return ScCols{s->src[half], s->pts[half], s->alpha[half], s->ts[half]}; }
bool sc_pose_ok(const double *p) {
  for (int a = 0; a < 7; a++) if (!std::isfinite(p[a])) return false;
  return true;
}
// the host's copy of the counts (one 32-byte read and a wait when an operation changed them on the device since)
gfbe_status sc_counts(gfbe_ctx *c, gfbe_scan *s) {
  if (s->counts_known) return GFBE_OK;
  int h[SC_META];
  GFBE_CHECK(c, hipMemcpyAsync(h, s->meta, sizeof h, hipMemcpyDeviceToHost, ctx_stream(c)));
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  s->n_pts = h[SM_N]; s->n_kp = h[SM_NKP]; s->counts_known = true;
  return GFBE_OK;
}
// claim, two-level scan and compaction of the points of half `cur` keyed on keypts [n][3]; grids by the host's bound n_up
void sc_enqueue_sample(gfbe_ctx *c, gfbe_scan *s, const double *keypts, double size, bool keypoints, ScCols out) {
  hipStream_t st = ctx_stream(c);
  int used = 64;      // a table of 2^k >= 2 n_up slots of the handle's
  while (used < 2 * s->n_up) used <<= 1;
  used = std::min(used, s->slots);
  const int G = (s->n_up + SC_THREADS - 1) / SC_THREADS;
  (void)hipMemsetAsync(s->keys, 0xFF, sizeof(unsigned long long) * (size_t)used, st);
  (void)hipMemsetAsync(s->minidx, 0x7F, sizeof(int) * (size_t)used, st);
  const VmDev T{s->keys, nullptr, nullptr, used - 1, 0, 0, nullptr};
  if (G > 0) {
    hipLaunchKernelGGL(k_sc_claim, dim3(G), dim3(SC_THREADS), 0, st, (const int *)s->meta, keypts, size, T, s->minidx, s->slot_of);
    hipLaunchKernelGGL(k_sc_count, dim3(G), dim3(SC_THREADS), 0, st, (const int *)s->meta, (const int *)s->slot_of, (const int *)s->minidx, G, s->part);
  }
  hipLaunchKernelGGL(k_sc_offsets, dim3(1), dim3(SC_SCAN_THREADS), 0, st, s->meta, G, s->part, keypoints ? 1 : 0);
  if (G > 0)
    hipLaunchKernelGGL(k_sc_compact, dim3(G), dim3(SC_THREADS), 0, st, (const int *)s->meta, keypoints ? (int)SM_N : (int)SM_NOLD, (const int *)s->slot_of,
                       (const int *)s->minidx, (const int *)s->part, sc_cols(s, s->cur), out);
}

}  // namespace

extern "C" {

void gfbe_scan_destroy(gfbe_ctx *c, gfbe_scan *s) {
  if (!s) return;
  s->release(c);
  delete s;
}

gfbe_status gfbe_scan_create(gfbe_ctx *c, int32_t point_capacity, gfbe_scan **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  if (point_capacity < 1 || point_capacity > (1 << 21)) { ctx_set_error(c, "gfbe_scan_create: point_capacity outside 1 .. 2^21"); return GFBE_BAD_INPUT; }
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_scan_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  gfbe_scan *s = new gfbe_scan();
  CreateGuard<gfbe_scan> guard{c, s, gfbe_scan_destroy};
  s->owner = c; s->cap = point_capacity;
  int slots = 64;
  while (slots < 2 * point_capacity) slots <<= 1;
  s->slots = slots;
  const size_t N = (size_t)point_capacity, G = (N + SC_THREADS - 1) / SC_THREADS;
  bool ok = true;
  for (int b = 0; b < 2; b++) ok = ok && s->alloc(&s->src[b], N) && s->alloc(&s->pts[b], 3 * N) && s->alloc(&s->alpha[b], N) && s->alloc(&s->ts[b], N);
  ok = ok && s->alloc(&s->kp_src, N) && s->alloc(&s->kp_pts, 3 * N) && s->alloc(&s->kp_alpha, N) && s->alloc(&s->kp_ts, N) && s->alloc(&s->keys, (size_t)slots) &&
       s->alloc(&s->minidx, (size_t)slots) && s->alloc(&s->slot_of, N) && s->alloc(&s->part, 2 * G + 2) && s->alloc(&s->world, 3 * N) && s->alloc(&s->meta, (size_t)SC_META);
  if (!ok) { ctx_set_error(c, "gfbe_scan_create: device allocation failed"); return GFBE_DEVICE_ERROR; }
  if (!s->make_staging(c, "gfbe_scan_create", 1 << 16, true)) return GFBE_DEVICE_ERROR;
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  guard.armed = false;
  *out = s;
  return GFBE_OK;
}

gfbe_status gfbe_scan_upload(gfbe_ctx *c, gfbe_scan *s, int32_t n, const double *raw_pts, const double *alpha, const double *timestamp, const double *til) {
  gfbe_status st = sc_ready(c, s, "gfbe_scan_upload");
  if (st != GFBE_OK) return st;
  if (n < 0 || (n > 0 && (!raw_pts || !alpha))) return GFBE_BAD_INPUT;
  if (n > s->cap) { ctx_set_error(c, "gfbe_scan_upload: more points than the handle's capacity"); return GFBE_BAD_INPUT; }
  if (til && !sc_pose_ok(til)) { ctx_set_error(c, "gfbe_scan_upload: til is not finite"); return GFBE_BAD_INPUT; }
  const size_t N = (size_t)n;
  {
    Staged sg(c, s, N * 40 + 2048, /*defer=*/true);
    const double *draw = sg.up(raw_pts, 3 * N), *dal = sg.up(alpha, N), *dts = sg.up(timestamp, timestamp ? N : 0), *dtil = sg.up(til, til ? 7 : 0);
    if (!sg.ok) { ctx_set_error(c, "gfbe_scan_upload: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    s->cur = 0;
    hipLaunchKernelGGL(k_sc_ingest, dim3((unsigned)std::max<size_t>(1, (N + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, ctx_stream(c), n, draw, dal,
                       timestamp ? dts : nullptr, til ? dtil : nullptr, sc_cols(s, 0), s->meta);
  }
  s->n_up = n; s->has_ts = timestamp != nullptr; s->kp_valid = false;
  s->n_pts = n; s->n_kp = 0; s->counts_known = true;
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_scan_subsample(gfbe_ctx *c, gfbe_scan *s, double size_voxel) {
  gfbe_status st = sc_ready(c, s, "gfbe_scan_subsample");
  if (st != GFBE_OK) return st;
  if (!(size_voxel > 0.0) || !std::isfinite(size_voxel)) { ctx_set_error(c, "gfbe_scan_subsample: size_voxel must be finite and > 0"); return GFBE_BAD_INPUT; }
  s->kp_valid = false; s->counts_known = false;
  sc_enqueue_sample(c, s, s->pts[s->cur], size_voxel, false, sc_cols(s, 1 - s->cur));
  s->cur = 1 - s->cur;
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_scan_undistort(gfbe_ctx *c, gfbe_scan *s, int32_t n_states, const double *state_time, const double *state_pose) {
  gfbe_status st = sc_ready(c, s, "gfbe_scan_undistort");
  if (st != GFBE_OK) return st;
  if (n_states < 1 || n_states > SC_MAX_STATES || !state_time || !state_pose) return GFBE_BAD_INPUT;
  if (!s->has_ts) { ctx_set_error(c, "gfbe_scan_undistort: the scan was uploaded without time stamps"); return GFBE_BAD_INPUT; }
  for (int k = 0; k < n_states; k++)
    if (!std::isfinite(state_time[k]) || (k > 0 && state_time[k] < state_time[k - 1]) || !sc_pose_ok(state_pose + 7 * k)) {
      ctx_set_error(c, "gfbe_scan_undistort: state times must be finite and ascending, state poses finite");
      return GFBE_BAD_INPUT;
    }
  s->kp_valid = false;
  {
    Staged sg(c, s, (size_t)n_states * 64 + 1024, /*defer=*/true);
    const double *dt = sg.up(state_time, (size_t)n_states), *dp = sg.up(state_pose, 7 * (size_t)n_states);
    if (!sg.ok) { ctx_set_error(c, "gfbe_scan_undistort: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    const int G = (s->n_up + SC_THREADS - 1) / SC_THREADS;
    if (G > 0) hipLaunchKernelGGL(k_sc_undistort, dim3(G), dim3(SC_THREADS), 0, ctx_stream(c), (const int *)s->meta, (int)n_states, dt, dp, s->pts[s->cur], (const double *)s->ts[s->cur]);
  }
  GFBE_CHECK(c, hipGetLastError());
  return GFBE_OK;
}

gfbe_status gfbe_scan_keypoints(gfbe_ctx *c, gfbe_scan *s, int32_t ct, const double *pose_begin, const double *pose_end, double size_voxel, int32_t *n_keypoints) {
  gfbe_status st = sc_ready(c, s, "gfbe_scan_keypoints");
  if (st != GFBE_OK) return st;
  if (!pose_begin || (ct && !pose_end)) return GFBE_BAD_INPUT;
  if (!(size_voxel > 0.0) || !std::isfinite(size_voxel)) { ctx_set_error(c, "gfbe_scan_keypoints: size_voxel must be finite and > 0"); return GFBE_BAD_INPUT; }
  s->kp_valid = false;
  int h[SC_META] = {0};
  {
    Staged sg(c, s, 1024);
    const double *dpb = sg.up(pose_begin, 7), *dpe = sg.up(pose_end ? pose_end : pose_begin, 7);
    if (!sg.ok) { ctx_set_error(c, "gfbe_scan_keypoints: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    const int G = (s->n_up + SC_THREADS - 1) / SC_THREADS;
    if (G > 0)
      hipLaunchKernelGGL(k_sc_world, dim3(G), dim3(SC_THREADS), 0, ctx_stream(c), (const int *)s->meta, ct ? 1 : 0, (const double *)s->pts[s->cur],
                         (const double *)s->alpha[s->cur], dpb, dpe, s->world);
    sc_enqueue_sample(c, s, s->world, size_voxel, true, ScCols{s->kp_src, s->kp_pts, s->kp_alpha, s->kp_ts});
    sg.down(h, (const int *)s->meta, (size_t)SC_META);
    sg.finish();      // the host wait: the counts
  }
  GFBE_CHECK(c, hipGetLastError());
  s->n_pts = h[SM_N]; s->n_kp = h[SM_NKP]; s->counts_known = true; s->kp_valid = true;
  if (n_keypoints) *n_keypoints = h[SM_NKP];
  return GFBE_OK;
}

gfbe_status gfbe_scan_size(gfbe_ctx *c, gfbe_scan *s, int32_t *n_points, int32_t *n_keypoints, int32_t *n_skipped) {
  gfbe_status st = sc_ready(c, s, "gfbe_scan_size");
  if (st != GFBE_OK) return st;
  int h[SC_META];
  GFBE_CHECK(c, hipMemcpyAsync(h, s->meta, sizeof h, hipMemcpyDeviceToHost, ctx_stream(c)));
  GFBE_CHECK(c, hipStreamSynchronize(ctx_stream(c)));
  s->n_pts = h[SM_N]; s->n_kp = h[SM_NKP]; s->counts_known = true;
  if (n_points) *n_points = h[SM_N];
  if (n_keypoints) *n_keypoints = s->kp_valid ? h[SM_NKP] : 0;
  if (n_skipped) *n_skipped = h[SM_SKIP] + h[SM_SKIPKP];
  return GFBE_OK;
}

gfbe_status gfbe_scan_download(gfbe_ctx *c, gfbe_scan *s, int32_t which, int32_t *src, double *pts, double *alpha, double *timestamp) {
  gfbe_status st = sc_ready(c, s, "gfbe_scan_download");
  if (st != GFBE_OK) return st;
  if (which != 0 && which != 1) return GFBE_BAD_INPUT;
  if ((st = sc_counts(c, s)) != GFBE_OK) return st;
  const size_t n = (size_t)(which ? (s->kp_valid ? s->n_kp : 0) : s->n_pts);
  if (n == 0) return GFBE_OK;
  const ScCols C = which ? ScCols{s->kp_src, s->kp_pts, s->kp_alpha, s->kp_ts} : sc_cols(s, s->cur);
  hipStream_t q = ctx_stream(c);
  if (src) GFBE_CHECK(c, hipMemcpyAsync(src, C.src, sizeof(int) * n, hipMemcpyDeviceToHost, q));
  if (pts) GFBE_CHECK(c, hipMemcpyAsync(pts, C.pts, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, q));
  if (alpha) GFBE_CHECK(c, hipMemcpyAsync(alpha, C.alpha, sizeof(double) * n, hipMemcpyDeviceToHost, q));
  if (timestamp) GFBE_CHECK(c, hipMemcpyAsync(timestamp, C.ts, sizeof(double) * n, hipMemcpyDeviceToHost, q));
  GFBE_CHECK(c, hipStreamSynchronize(q));
  return GFBE_OK;
}

}  // extern "C"

// ---- the hand-over (gfbe_vreg.hip, gfbe_vmap.hip): the handle's columns where they are, with a count the host knows
namespace gfd {
gfbe_status scan_keypoints_view(gfbe_ctx *c, gfbe_scan *s, const char *who, ScanView *v) {
  const gfbe_status st = sc_ready(c, s, who);
  if (st != GFBE_OK) return st;
  if (!s->kp_valid) { ctx_set_error(c, (std::string(who) + ": no keypoints of the scan as it is now (call gfbe_scan_keypoints after the last change)").c_str()); return GFBE_BAD_INPUT; }
  *v = ScanView{s->n_kp, s->kp_pts, s->kp_alpha};      // (kp_valid: gfbe_scan_keypoints read the count back)
  return GFBE_OK;
}
gfbe_status scan_points_view(gfbe_ctx *c, gfbe_scan *s, const char *who, ScanView *v) {
  gfbe_status st = sc_ready(c, s, who);
  if (st != GFBE_OK) return st;
  if ((st = sc_counts(c, s)) != GFBE_OK) return st;
  *v = ScanView{s->n_pts, s->pts[s->cur], s->alpha[s->cur]};
  return GFBE_OK;
}
}  // namespace gfd
