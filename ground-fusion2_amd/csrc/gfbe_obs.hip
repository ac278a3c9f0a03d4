// gfbe_obs.hip — the frame observations on the held points of a tracker handle (gfbe_klt.hip): the second half of
// FeatureTracker::trackImage for n cameras, the hand-over of the frame to the feature tables (gfbe_ftab.hip), and the two calls that go
// back from the estimator to the tracker.
//
//   undistortedPts, ptsVelocity, the depth lookup, the id-ordered frame    vins_estimator/src/featureTracker/feature_tracker.cpp:210-372     k_obs_observe
//   removeOutliers                                                        :1029-1045                                                       k_obs_remove
//   predictPtsInNextFrame, setPrediction                                  estimator.cpp:3927-3946, feature_tracker.cpp:1006-1027           k_obs_predict
//
// The rules are in gfbe_obs.h and include/gfbe_obs.h; every per-point statement is the header's function, compiled here for the device.
// k_obs_observe: one workgroup per camera; every point is lifted into LDS, the (id, index) keys are ordered by a bitonic sort in LDS,
// row j of the frame belongs to the j-th key: equal neighbours raise the duplicate flag, the previous list (ascending in id, in the
// half the last call wrote) is searched by bisection, the depth pixel is gathered, the row, the id and the new previous list (the
// other half) are written. The counters are integer sums in LDS. k_obs_remove: the compaction of k_klt_decide with "the id is listed"
// as the decision. k_obs_predict: 256 held points a workgroup against the table's id list in LDS tiles, as k_ftab_match does, then the
// chain of O8 by the thread that owns the point. None of it is arithmetic-bound (a frame is 150 points a camera): what counts is that
// no list crosses the bus and that a call waits once. No communication between workgroups inside a launch, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gfbe_obs.h"
#include "gfbe_device.h"
#include "gfbe_klt_priv.h"
#include "gfbe_obs.h"
#include "gfbe_handle.h"

using namespace gfd;

static_assert(OBS_MAX_POINTS == GFBE_DET_MAX_POINTS, "the header's bound");
static_assert(OBS_OW == FT_OW, "a row of the frame is a row of the tables");

struct gfbe_obs : gfbe_handle {
  gfbe_klt *trk = nullptr;
  gfbe_obs_options opt;
  ObsCam *cams = nullptr;                      // [n_cam]
  uint16_t *depth_d = nullptr, *depth_h = nullptr;      // [n_cam][rows][cols] and its pinned mirror (depth_cam == 1)
  hipEvent_t ev_depth = nullptr;
  bool depth_busy = false;
  // the frame observe left: rows packed over the cameras
  int *f_off = nullptr, *f_id = nullptr;      // [n_cam + 1], [n_cam * cap]
  double *f_obs = nullptr;                     // [n_cam * cap][8]
  int frame_state = 0;                         // 0: none, 1: held, 2: added
  bool frame_dup = false;
  int frame_rows = 0, frame_max = 0;
  // the previous lists, ascending in id: two halves, camera k at rows k * cap
  int *p_ids[2] = {nullptr, nullptr}, *p_n[2] = {nullptr, nullptr};
  float *p_un[2] = {nullptr, nullptr};
  int phalf = 0;
  bool has_time = false;
  std::vector<double> prev_time;
};

namespace {
constexpr int OBS_THREADS = 256;
typedef unsigned long long u64;

// ascending bitonic sort of n = 2^k keys in LDS by the whole workgroup; the keys are complete and a barrier has passed
__device__ __forceinline__ void obs_bitonic(u64 *k, int n) {
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < n / 2; i += OBS_THREADS) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const u64 a = k[lo], b = k[hi];
        if ((a > b) == up) { k[lo] = b; k[hi] = a; }
      }
      __syncthreads();
    }
}

// ---- O3 .. O6 -------------------------------------------------------------------------------------------------------------------------
struct ObsObserveArgs {
  const ObsCam *cams;
  const int *seg_begin, *count_in;             // the tracker's held rows
  const float *pts;
  const int *ids;
  const int *off;                              // [n_cam + 1] the packed rows of the frame (the host's exact mirrors)
  const double *dt;                            // [n_cam]
  const uint16_t *depth;                       // nullptr: every depth -2.4
  int rows, cols, cap, n_cam;
  const int *prev_ids, *prev_n;
  const float *prev_un;
  int *next_ids, *next_n;
  float *next_un;
  int *f_off, *f_id;
  double *f_obs;
  int *counters;                               // [n_cam][4]
};
__global__ __launch_bounds__(OBS_THREADS) void k_obs_observe(ObsObserveArgs A) {
  __shared__ u64 s_key[OBS_MAX_POINTS];
  __shared__ float s_un[2 * OBS_MAX_POINTS];
  __shared__ int s_cnt[3];
  const int cam = blockIdx.x, t = threadIdx.x;
  const int out = A.off[cam], n = max(0, min(min(A.off[cam + 1] - out, A.count_in[cam]), min(A.cap, OBS_MAX_POINTS)));
  const size_t base = (size_t)A.seg_begin[cam], list = (size_t)cam * (size_t)A.cap;
  const ObsCam c = A.cams[cam];
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  if (t < 3) s_cnt[t] = 0;
  for (int i = t; i < np2; i += OBS_THREADS) {
    u64 key = ~0ull;      // (no key is all ones: an index is below 2048)
    if (i < n) {
      key = obs_key(A.ids[base + i], i);
      float ux, uy;
      obs_lift(c, A.pts[2 * (base + i)], A.pts[2 * (base + i) + 1], &ux, &uy);
      s_un[2 * i] = ux; s_un[2 * i + 1] = uy;
    }
    s_key[i] = key;
  }
  __syncthreads();
  obs_bitonic(s_key, np2);
  const int n_prev = max(0, min(A.prev_n[cam], A.cap));
  const int *prev_ids = A.prev_ids + list;
  const float *prev_un = A.prev_un + 2 * list;
  const double dt = A.dt[cam];
  int found = 0, outside = 0, dup = 0;
  for (int j = t; j < n; j += OBS_THREADS) {
    const u64 key = s_key[j];
    const int i = obs_key_index(key), id = obs_key_id(key);
    if (j > 0 && obs_key_id(s_key[j - 1]) == id) dup = 1;
    const float u = A.pts[2 * (base + i)], v = A.pts[2 * (base + i) + 1], ux = s_un[2 * i], uy = s_un[2 * i + 1];
    float vx = 0.f, vy = 0.f;
    const int q = obs_lower_bound(prev_ids, n_prev, id);
    if (q < n_prev && prev_ids[q] == id) {
      vx = obs_velocity(ux, prev_un[2 * q], dt); vy = obs_velocity(uy, prev_un[2 * q + 1], dt);
      found++;
    }
    double dep = obs_no_depth();
    if (A.depth) {
      int x, y;
      bool inside;
      obs_depth_index(u, v, A.cols, A.rows, &x, &y, &inside);
      dep = obs_depth_value(inside ? A.depth[((size_t)cam * (size_t)A.rows + (size_t)y) * (size_t)A.cols + (size_t)x] : (uint16_t)0);
      outside += inside ? 0 : 1;
    }
    const size_t r = (size_t)out + (size_t)j;
    obs_row(ux, uy, u, v, vx, vy, dep, A.f_obs + OBS_OW * r);
    A.f_id[r] = id;
    A.next_ids[list + j] = id; A.next_un[2 * (list + j)] = ux; A.next_un[2 * (list + j) + 1] = uy;
  }
  if (found) atomicAdd(&s_cnt[0], found);
  if (outside) atomicAdd(&s_cnt[1], outside);
  if (dup) atomicOr(&s_cnt[2], 1);
  __syncthreads();
  if (t == 0) {
    int *cn = A.counters + 4 * (size_t)cam;
    cn[0] = n; cn[1] = s_cnt[0]; cn[2] = s_cnt[1]; cn[3] = s_cnt[2];
    A.next_n[cam] = n;
    A.f_off[cam] = out;
    if (cam == A.n_cam - 1) A.f_off[A.n_cam] = A.off[A.n_cam];
  }
}

// ---- O7 -------------------------------------------------------------------------------------------------------------------------------
struct ObsRemoveArgs {
  const int *seg_begin, *count_in;
  const float *pts_in;
  const int *ids_in, *cnt_in;
  const int *ioff, *list;                      // the ids to drop: camera k at list[ioff[k] .. ioff[k + 1])
  uint8_t *dec;                                // [rows] scratch: a point's decision, formed once
  float *pts_out;                              // the tracker's other half, the survivors at the head of the camera's rows
  int *ids_out, *cnt_out, *count_out, *held;
};
__global__ __launch_bounds__(OBS_THREADS) void k_obs_remove(ObsRemoveArgs A) {
  __shared__ int lds[20];
  const int cam = blockIdx.x, t = threadIdx.x, n = A.count_in[cam];
  const size_t base = (size_t)A.seg_begin[cam];
  const int l0 = A.ioff[cam], l1 = A.ioff[cam + 1];
  const int chunk = (n + OBS_THREADS - 1) / OBS_THREADS, b0 = min(n, t * chunk), b1 = min(n, b0 + chunk);
  int kept = 0, total;
  for (int i = b0; i < b1; i++) {
    const int id = A.ids_in[base + i];
    int keep = 1;
    for (int q = l0; q < l1; q++) keep = A.list[q] == id ? 0 : keep;
    A.dec[base + i] = (uint8_t)keep;      // (read back by this thread only)
    kept += keep;
  }
  int dst = block_exclusive_scan<OBS_THREADS>(kept, &total, lds);
  for (int i = b0; i < b1; i++) {
    const size_t p = base + (size_t)i;
    if (!A.dec[p]) continue;
    const size_t q = base + (size_t)dst;
    A.pts_out[2 * q] = A.pts_in[2 * p]; A.pts_out[2 * q + 1] = A.pts_in[2 * p + 1];
    A.ids_out[q] = A.ids_in[p]; A.cnt_out[q] = A.cnt_in[p];
    dst++;
  }
  if (t == 0) { A.count_out[cam] = total; A.held[cam] = total; }
}

// ---- O8 -------------------------------------------------------------------------------------------------------------------------------
struct ObsPredictArgs {
  const ObsCam *cams;
  const int *seg_begin, *count_in;
  const float *pts;
  const int *ids;
  const int *off;                              // [n_cam + 1] the packed rows of predict_pts
  const int *frame_count;                      // [n_cam]
  const double *poses, *tic_ric, *next_pose;   // [n_cam][11][12], [n_cam][12], [n_cam][12]
  int tile;
  float *predict;                              // [n][2]
  int *n_pred;                                 // [n_cam], zero before the launch
};
__global__ __launch_bounds__(OBS_THREADS) void k_obs_predict(FtabDev T, int cur, ObsPredictArgs A) {
  extern __shared__ int s_id[];                // [tile]
  const int cam = blockIdx.y, t = threadIdx.x, i = blockIdx.x * OBS_THREADS + t;
  const int out = A.off[cam], n = max(0, min(A.off[cam + 1] - out, A.count_in[cam]));
  if ((int)blockIdx.x * OBS_THREADS >= n) return;       // (workgroup-uniform)
  const size_t base = (size_t)A.seg_begin[cam], tb = (size_t)cam * (size_t)T.F;
  const int nf = max(0, min(T.count[cam], T.F));
  const bool mine = i < n;
  const int want = mine ? A.ids[base + i] : 0;
  int hit = -1;
  for (int f0 = 0; f0 < nf; f0 += A.tile) {
    const int nt = min(nf - f0, A.tile);
    __syncthreads();
    for (int f = t; f < nt; f += OBS_THREADS) s_id[f] = T.id[cur][tb + f0 + f];
    __syncthreads();
    if (mine && hit < 0)
      for (int f = nt - 1; f >= 0; f--) hit = s_id[f] == want ? f0 + f : hit;     // (ids are unique inside a table)
  }
  if (!mine) return;
  float u = A.pts[2 * (base + i)], v = A.pts[2 * (base + i) + 1];
  if (hit >= 0) {
    const double depth = T.depth[cur][tb + hit];
    const int m = T.nobs[cur][tb + hit], s = T.start[cur][tb + hit];
    if (s >= 0 && s < FT_NOBS && obs_predicts(depth, m, s, A.frame_count[cam])) {
      float pu, pv;
      if (obs_predict(A.cams[cam], T.obs[cur] + (tb + hit) * FT_NOBS * FT_OW, depth, A.poses + 132 * (size_t)cam + 12 * (size_t)s, A.tic_ric + 12 * (size_t)cam,
                      A.next_pose + 12 * (size_t)cam, &pu, &pv)) {
        u = pu; v = pv;
        atomicAdd(&A.n_pred[cam], 1);
      }
    }
  }
  A.predict[2 * ((size_t)out + i)] = u; A.predict[2 * ((size_t)out + i) + 1] = v;
}

bool obs_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
const char *obs_options_error(const gfbe_obs_options *o) {
  if (o->struct_size != (int32_t)sizeof(gfbe_obs_options)) return "gfbe_obs_options.struct_size does not match this library (ABI mismatch)";
  if (o->depth_cam != 0 && o->depth_cam != 1) return "depth_cam outside 0 .. 1";
  if (!obs_pow2(o->match_tile) || o->match_tile < 64 || o->match_tile > 1024) return "match_tile is no power of two in 64 .. 1024";
  return nullptr;
}
// the packed rows of the held points over the cameras, from the tracker's exact mirrors
void obs_offsets(const gfbe_klt *k, std::vector<int> *off, int *most) {
  off->assign((size_t)k->n_cam + 1, 0);
  *most = 0;
  for (int q = 0; q < k->n_cam; q++) { (*off)[(size_t)q + 1] = (*off)[(size_t)q] + k->count_h[(size_t)q]; *most = std::max(*most, k->count_h[(size_t)q]); }
}

}  // namespace

extern "C" {

void gfbe_obs_default_options(gfbe_obs_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = (int32_t)sizeof *o;
  o->depth_cam = 1; o->match_tile = 256;
}

void gfbe_obs_destroy(gfbe_ctx *c, gfbe_obs *m) {
  if (!m) return;
  m->release(c);
  delete m;
}

gfbe_status gfbe_obs_create(gfbe_ctx *c, gfbe_klt *k, const double *cameras, const gfbe_obs_options *opt, gfbe_obs **out) {
  if (!c || !out) return GFBE_BAD_INPUT;
  *out = nullptr;
  gfbe_obs_options o;
  if (opt) o = *opt; else gfbe_obs_default_options(&o);
  if (const char *bad = obs_options_error(&o)) return handle_bad(c, "gfbe_obs_create", bad);
  if (ctx_device(c) < 0) { ctx_set_error(c, "gfbe_obs_create: HIP device context required (no CPU fallback)"); return GFBE_NO_DEVICE; }
  if (!k) return handle_bad(c, "gfbe_obs_create", "tracker NULL");
  if (k->owner != c) return handle_bad(c, "gfbe_obs_create", "the tracker belongs to another context");
  if (k->cap > OBS_MAX_POINTS) return handle_bad(c, "gfbe_obs_create", "the tracker's point_capacity is above GFBE_DET_MAX_POINTS");
  if (!cameras) return handle_bad(c, "gfbe_obs_create", "cameras NULL");
  const size_t C = (size_t)k->n_cam, N = C * (size_t)k->cap;
  std::vector<ObsCam> cams(C);
  for (size_t q = 0; q < C; q++) {
    if (!obs_camera_ok(cameras + 8 * q)) return handle_bad(c, "gfbe_obs_create", "a camera parameter is not finite, or fx / fy is 0");
    cams[q] = obs_camera(cameras + 8 * q);
  }
  gfbe_obs *m = new gfbe_obs();
  CreateGuard<gfbe_obs> guard{c, m, gfbe_obs_destroy};
  m->owner = c; m->trk = k; m->opt = o;
  m->prev_time.assign(C, 0.0);
  hipStream_t st = ctx_stream(c);
  const size_t px = C * (size_t)k->rows * (size_t)k->cols;
  bool ok = m->alloc(&m->cams, C) && m->alloc(&m->f_off, C + 1) && m->alloc(&m->f_id, N) && m->alloc(&m->f_obs, OBS_OW * N);
  for (int b = 0; b < 2; b++) ok = ok && m->alloc(&m->p_ids[b], N) && m->alloc(&m->p_n[b], C) && m->alloc(&m->p_un[b], 2 * N);
  if (o.depth_cam) ok = ok && m->alloc(&m->depth_d, px) && m->alloc_pinned(&m->depth_h, px) && m->create(&m->ev_depth);
  if (!ok) { ctx_set_error(c, "gfbe_obs_create: device allocation failed"); return GFBE_DEVICE_ERROR; }
  GFBE_CHECK(c, hipMemcpyAsync(m->cams, cams.data(), sizeof(ObsCam) * C, hipMemcpyHostToDevice, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));      // (cams leaves scope)
  guard.armed = false;
  *out = m;
  return GFBE_OK;
}

gfbe_status gfbe_obs_reset(gfbe_ctx *c, gfbe_obs *m) {
  gfbe_status rc = handle_ready(c, m, "gfbe_obs_reset");
  if (rc != GFBE_OK) return rc;
  const size_t C = (size_t)m->trk->n_cam;
  for (int b = 0; b < 2; b++) GFBE_CHECK(c, hipMemsetAsync(m->p_n[b], 0, sizeof(int) * C, ctx_stream(c)));
  m->has_time = false; m->frame_state = 0; m->frame_dup = false;
  return GFBE_OK;
}

gfbe_status gfbe_obs_observe(gfbe_ctx *c, gfbe_obs *m, const double *cur_time, const uint16_t *depth, int32_t *offset_out, int32_t *feature_id, double *obs8,
                             int32_t *counters) {
  gfbe_status rc = handle_ready(c, m, "gfbe_obs_observe");
  if (rc != GFBE_OK) return rc;
  gfbe_klt *k = m->trk;
  if (k->n_pushed < 1) return handle_bad(c, "gfbe_obs_observe", "no image has been pushed");
  if (!cur_time) return handle_bad(c, "gfbe_obs_observe", "cur_time NULL");
  const size_t C = (size_t)k->n_cam;
  std::vector<double> dt(C, 0.0);
  for (size_t q = 0; q < C; q++) {
    if (!std::isfinite(cur_time[q]) || (m->has_time && !(cur_time[q] > m->prev_time[q]))) return handle_bad(c, "gfbe_obs_observe", "a time is not finite or not greater than the camera's previous time");
    dt[q] = cur_time[q] - m->prev_time[q];
  }
  if (m->opt.depth_cam && !depth) return handle_bad(c, "gfbe_obs_observe", "depth_cam == 1 needs the depth images");
  std::vector<int> off;
  int most = 0;
  obs_offsets(k, &off, &most);
  const size_t n = (size_t)off[C];
  hipStream_t st = ctx_stream(c);
  std::vector<int32_t> cnts(4 * C, 0);
  {
    Staged sg(c, k, C * 32 + 8192);
    const int *d_off = sg.up((const int *)off.data(), C + 1);
    const double *d_dt = sg.up((const double *)dt.data(), C);
    int *o_cnts = sg.up((const int *)nullptr, 4 * C);
    if (!sg.ok) { ctx_set_error(c, "gfbe_obs_observe: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    if (m->opt.depth_cam) {
      const size_t px = C * (size_t)k->rows * (size_t)k->cols;
      if (m->depth_busy) GFBE_CHECK(c, hipEventSynchronize(m->ev_depth));      // (the mirror's last copy has left it)
      std::memcpy(m->depth_h, depth, px * sizeof(uint16_t));
      GFBE_CHECK(c, hipMemcpyAsync(m->depth_d, m->depth_h, px * sizeof(uint16_t), hipMemcpyHostToDevice, st));
      GFBE_CHECK(c, hipEventRecord(m->ev_depth, st));
      m->depth_busy = true;
    }
    const int ph = m->phalf, nh = ph ^ 1, hf = k->half;
    ObsObserveArgs A;
    std::memset(&A, 0, sizeof A);
    A.cams = m->cams; A.seg_begin = k->seg_begin; A.count_in = k->seg_count[hf]; A.pts = k->pts[hf]; A.ids = k->ids[hf]; A.off = d_off; A.dt = d_dt;
    A.depth = m->opt.depth_cam ? m->depth_d : nullptr; A.rows = k->rows; A.cols = k->cols; A.cap = k->cap; A.n_cam = k->n_cam;
    A.prev_ids = m->p_ids[ph]; A.prev_n = m->p_n[ph]; A.prev_un = m->p_un[ph]; A.next_ids = m->p_ids[nh]; A.next_n = m->p_n[nh]; A.next_un = m->p_un[nh];
    A.f_off = m->f_off; A.f_id = m->f_id; A.f_obs = m->f_obs; A.counters = o_cnts;
    hipLaunchKernelGGL(k_obs_observe, dim3(k->n_cam), dim3(OBS_THREADS), 0, st, A);
    sg.down(cnts.data(), (const int32_t *)o_cnts, 4 * C);
    if (n > 0) {      // (straight from the handle's frame; nothing of it is downloaded when the caller wants the counters alone)
      sg.down(feature_id, (const int32_t *)m->f_id, n);
      sg.down(obs8, (const double *)m->f_obs, OBS_OW * n);
    }
    sg.finish();      // the one wait
    GFBE_CHECK(c, hipGetLastError());
    m->phalf = nh;
  }
  m->has_time = true;
  bool dup = false;
  for (size_t q = 0; q < C; q++) { m->prev_time[q] = cur_time[q]; dup = dup || cnts[4 * q + 3] != 0; }
  m->frame_state = 1; m->frame_dup = dup; m->frame_rows = (int)n; m->frame_max = most;
  if (offset_out) std::memcpy(offset_out, off.data(), sizeof(int32_t) * (C + 1));
  if (counters) std::memcpy(counters, cnts.data(), sizeof(int32_t) * 4 * C);
  return GFBE_OK;
}

gfbe_status gfbe_obs_add_frame(gfbe_ctx *c, gfbe_obs *m, gfbe_ftab *t, const int32_t *frame_count, const double *td, int32_t *keyframe, int32_t *counters,
                               double *avg_parallax) {
  gfbe_status rc = handle_ready(c, m, "gfbe_obs_add_frame");
  if (rc != GFBE_OK) return rc;
  if (!t || !frame_count || !td) return handle_bad(c, "gfbe_obs_add_frame", "ftab, frame_count or td NULL");
  if (t->d.W != m->trk->n_cam) return handle_bad(c, "gfbe_obs_add_frame", "the table count is not the tracker's camera count");
  if (m->frame_state == 0) return handle_bad(c, "gfbe_obs_add_frame", "no frame is held: observe first");
  if (m->frame_state == 2) return handle_bad(c, "gfbe_obs_add_frame", "the frame was already added");
  if (m->frame_dup) return handle_bad(c, "gfbe_obs_add_frame", "the frame holds two points of a camera with the same id");
  rc = ftab_add_frame_device(c, t, frame_count, td, m->frame_rows, m->frame_max, m->f_off, m->f_id, m->f_obs, keyframe, counters, avg_parallax);
  if (rc == GFBE_OK || rc == GFBE_BAD_INPUT) m->frame_state = 2;      // (the kernels ran: BAD_INPUT here is a table's capacity)
  return rc;
}

gfbe_status gfbe_obs_remove_outliers(gfbe_ctx *c, gfbe_obs *m, const int32_t *offset, const int32_t *ids, int32_t *held_out) {
  gfbe_status rc = handle_ready(c, m, "gfbe_obs_remove_outliers");
  if (rc != GFBE_OK) return rc;
  gfbe_klt *k = m->trk;
  if (k->n_pushed < 1) return handle_bad(c, "gfbe_obs_remove_outliers", "no image has been pushed");
  const size_t C = (size_t)k->n_cam;
  if (!offset || offset[0] != 0) return handle_bad(c, "gfbe_obs_remove_outliers", "offsets that do not ascend from 0");
  for (size_t q = 0; q < C; q++)
    if (offset[q + 1] < offset[q]) return handle_bad(c, "gfbe_obs_remove_outliers", "offsets that do not ascend from 0");
  const size_t L = (size_t)offset[C];
  if (L > 0 && !ids) return handle_bad(c, "gfbe_obs_remove_outliers", "ids NULL");
  std::vector<int32_t> held(C, 0);
  {
    Staged sg(c, k, L * 4 + C * 8 + 8192);
    const int *d_off = sg.up((const int *)offset, C + 1), *d_ids = sg.up((const int *)ids, L);
    int *o_held = sg.up((const int *)nullptr, C);
    if (!sg.ok) { ctx_set_error(c, "gfbe_obs_remove_outliers: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    const int hf = k->half, nh = hf ^ 1;
    ObsRemoveArgs A;
    std::memset(&A, 0, sizeof A);
    A.seg_begin = k->seg_begin; A.count_in = k->seg_count[hf]; A.pts_in = k->pts[hf]; A.ids_in = k->ids[hf]; A.cnt_in = k->cnt[hf]; A.ioff = d_off; A.list = d_ids;
    A.dec = k->w_dec; A.pts_out = k->pts[nh]; A.ids_out = k->ids[nh]; A.cnt_out = k->cnt[nh]; A.count_out = k->seg_count[nh]; A.held = o_held;
    hipLaunchKernelGGL(k_obs_remove, dim3(k->n_cam), dim3(OBS_THREADS), 0, ctx_stream(c), A);
    sg.down(held.data(), (const int32_t *)o_held, C);
    sg.finish();      // the one wait: the tracker's host mirrors stay exact
    GFBE_CHECK(c, hipGetLastError());
    k->half = nh;
  }
  for (size_t q = 0; q < C; q++) k->count_h[q] = std::min(held[q], k->count_h[q]);      // (the rows of camera q stay at begin_h[q], as after a track)
  if (held_out) std::memcpy(held_out, held.data(), sizeof(int32_t) * C);
  return GFBE_OK;
}

gfbe_status gfbe_obs_predict(gfbe_ctx *c, gfbe_obs *m, gfbe_ftab *t, const int32_t *frame_count, const double *poses, const double *tic_ric, const double *next_pose,
                             float *predict_pts, int32_t *n_predicted) {
  gfbe_status rc = handle_ready(c, m, "gfbe_obs_predict");
  if (rc != GFBE_OK) return rc;
  gfbe_klt *k = m->trk;
  if (k->n_pushed < 1) return handle_bad(c, "gfbe_obs_predict", "no image has been pushed");
  if (!t || !frame_count || !poses || !tic_ric || !next_pose) return handle_bad(c, "gfbe_obs_predict", "ftab, frame_count, poses, tic_ric or next_pose NULL");
  if (t->d.W != k->n_cam) return handle_bad(c, "gfbe_obs_predict", "the table count is not the tracker's camera count");
  rc = ftab_ready(c, t);
  if (rc != GFBE_OK) return rc;
  const size_t C = (size_t)k->n_cam;
  std::vector<int> off;
  int most = 0;
  obs_offsets(k, &off, &most);
  const size_t n = (size_t)off[C];
  {
    Staged sg(c, k, n * 8 + C * (16 + 156 * 8) + 16384);
    const int *d_off = sg.up((const int *)off.data(), C + 1), *d_fc = sg.up((const int *)frame_count, C);
    const double *d_poses = sg.up(poses, 132 * C), *d_tr = sg.up(tic_ric, 12 * C), *d_next = sg.up(next_pose, 12 * C);
    int *o_np = sg.up((const int *)nullptr, C);
    float *o_pred = sg.up((const float *)nullptr, 2 * n);
    if (!sg.ok) { ctx_set_error(c, "gfbe_obs_predict: staging allocation failed"); return GFBE_DEVICE_ERROR; }
    sg.flush();
    GFBE_CHECK(c, hipMemsetAsync(o_np, 0, sizeof(int) * C, ctx_stream(c)));
    if (most > 0) {
      const int hf = k->half;
      ObsPredictArgs A;
      std::memset(&A, 0, sizeof A);
      A.cams = m->cams; A.seg_begin = k->seg_begin; A.count_in = k->seg_count[hf]; A.pts = k->pts[hf]; A.ids = k->ids[hf]; A.off = d_off; A.frame_count = d_fc;
      A.poses = d_poses; A.tic_ric = d_tr; A.next_pose = d_next; A.tile = m->opt.match_tile; A.predict = o_pred; A.n_pred = o_np;
      hipLaunchKernelGGL(k_obs_predict, dim3((most + OBS_THREADS - 1) / OBS_THREADS, k->n_cam), dim3(OBS_THREADS), sizeof(int) * (size_t)m->opt.match_tile, ctx_stream(c),
                         t->d, t->cur, A);
    }
    sg.down(n_predicted, (const int32_t *)o_np, C);
    sg.down(predict_pts, (const float *)o_pred, 2 * n);
    sg.finish();      // the one wait
    GFBE_CHECK(c, hipGetLastError());
  }
  return GFBE_OK;
}

gfbe_status gfbe_obs_download_prev(gfbe_ctx *c, gfbe_obs *m, int32_t camera, int32_t *n_out, int32_t *ids, float *un_pts) {
  gfbe_status rc = handle_ready(c, m, "gfbe_obs_download_prev");
  if (rc != GFBE_OK) return rc;
  gfbe_klt *k = m->trk;
  if (camera < 0 || camera >= k->n_cam) return handle_bad(c, "gfbe_obs_download_prev", "camera outside the handle's");
  if (!n_out) return handle_bad(c, "gfbe_obs_download_prev", "n_out NULL");
  hipStream_t st = ctx_stream(c);
  int n = 0;
  GFBE_CHECK(c, hipMemcpyAsync(&n, m->p_n[m->phalf] + camera, sizeof(int), hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  n = std::max(0, std::min(n, k->cap));
  const size_t list = (size_t)camera * (size_t)k->cap;
  if (ids && n) GFBE_CHECK(c, hipMemcpyAsync(ids, m->p_ids[m->phalf] + list, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
  if (un_pts && n) GFBE_CHECK(c, hipMemcpyAsync(un_pts, m->p_un[m->phalf] + 2 * list, sizeof(float) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
  GFBE_CHECK(c, hipStreamSynchronize(st));
  *n_out = n;
  return GFBE_OK;
}

}  // extern "C"
