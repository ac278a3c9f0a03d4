// gfbe_handle.h — the host side every device handle shares (gfbe_ftab, gfbe_ltab, gfbe_vmap, gfbe_scan, gfbe_dmap, gfbe_ldb, gfbe_klt,
// gfbe_det, gfbe_obs, gfbe_kfd, gfbe_pnp, gfbe_eq, gfbe_gate): the check of a HIP call, the base that owns what a handle holds on the device, the guard of a create, and the
// entry checks of a call. Host code only, for the translation units that see the HIP runtime; the headers the HIP-free shims of the
// tests include stay clear of it.
#pragma once
#include <string>
#include <vector>

#include "gfbe_tabstage.h"

namespace gfd {
// a failed HIP call leaves "<call>: <HIP's text>" in the context
inline bool hip_ok(gfbe_ctx *c, hipError_t e, const char *call) {
  if (e != hipSuccess) ctx_set_error(c, (std::string(call) + ": " + hipGetErrorString(e)).c_str());
  return e == hipSuccess;
}
}  // namespace gfd
// ... and the function returns GFBE_DEVICE_ERROR
#define GFBE_CHECK(c, call) do { if (!gfd::hip_ok(c, (call), #call)) return GFBE_DEVICE_ERROR; } while (0)
// ... or puts it into its `st` and goes on to its `done:` (the calls that free their own buffers there)
#define GFBE_CHECK_DONE(c, call) do { if (!gfd::hip_ok(c, (call), #call)) { st = GFBE_DEVICE_ERROR; goto done; } } while (0)

// What a handle holds on the device: every block, pinned block and event is recorded the moment it exists, so that one release()
// frees a finished handle and a half-built one alike. The staging chunk and ring of gfbe_tab_staging are optional (make_staging):
// gfbe_det and gfbe_obs stage through their tracker's.
struct gfbe_handle : gfbe_tab_staging {
  gfbe_ctx *owner = nullptr;      // set by create before the first alloc: the allocations are cleared on its stream
  std::vector<void *> dev, pinned;
  std::vector<hipEvent_t> events;

  // n elements (at least one) of device memory, every byte set to `fill`
  template <typename T>
  bool alloc(T **p, size_t n, int fill = 0) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    void *q = nullptr;
    if (!gfd::hip_ok(owner, hipMalloc(&q, bytes), "hipMalloc")) return false;
    dev.push_back(q);      // (recorded before anything else can fail)
    *p = (T *)q;
    return gfd::hip_ok(owner, hipMemsetAsync(q, fill, bytes, gfd::ctx_stream(owner)), "hipMemsetAsync");
  }
  template <typename T>
  bool alloc_pinned(T **p, size_t n) {
    void *q = nullptr;
    if (!gfd::hip_ok(owner, hipHostMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)), "hipHostMalloc")) return false;
    pinned.push_back(q);
    *p = (T *)q;
    return true;
  }
  bool create(hipEvent_t *e) {
    if (!gfd::hip_ok(owner, hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreateWithFlags")) return false;
    events.push_back(*e);
    return true;
  }
  // the staging chunk, sized for warm_bytes up front, and the ring of the operations nobody waits for
  bool make_staging(gfbe_ctx *c, const char *who, size_t warm_bytes, bool with_ring) {
    if (!gfd::Staged(c, this, warm_bytes).ok) { gfd::ctx_set_error(c, (std::string(who) + ": staging allocation failed").c_str()); return false; }
    if (!with_ring) return true;
    bool ok = alloc(&ring_d, (size_t)RING * RING_SLOT) && alloc_pinned(&ring_h, (size_t)RING * RING_SLOT);
    for (int k = 0; k < RING && ok; k++) ok = create(&ring_ev[k]);
    return ok;
  }
  // behind everything queued on the context's stream
  void release(gfbe_ctx *c) {
    if (c && gfd::ctx_device(c) >= 0) (void)hipStreamSynchronize(gfd::ctx_stream(c));
    for (void *p : dev) (void)hipFree(p);
    for (void *p : pinned) (void)hipHostFree(p);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    if (stage_d) (void)hipFree(stage_d);
    if (stage_h) (void)hipHostFree(stage_h);
  }
};

namespace gfd {

// destroys the handle a create is building unless the create reaches its end (armed = false): a failed allocation leaves nothing
// behind and *out stays null
template <class H>
struct CreateGuard {
  gfbe_ctx *c;
  H *h;
  void (*destroy)(gfbe_ctx *, H *);
  bool armed = true;
  ~CreateGuard() { if (armed) destroy(c, h); }
};

inline gfbe_status handle_bad(gfbe_ctx *c, const char *who, const char *what) {
  ctx_set_error(c, (std::string(who) + ": " + what).c_str());
  return GFBE_BAD_INPUT;
}
// the head of every call on a handle: a context, with a device, and a handle
inline gfbe_status handle_device(gfbe_ctx *c, const gfbe_handle *m, const char *who) {
  if (!c) return GFBE_BAD_INPUT;
  if (ctx_device(c) < 0) { ctx_set_error(c, (std::string(who) + ": HIP device context required (no CPU fallback)").c_str()); return GFBE_NO_DEVICE; }
  return m ? GFBE_OK : GFBE_BAD_INPUT;
}
// ... of this context (`noun`: what the text calls it). The feature, line and voxel tables stop at handle_device.
inline gfbe_status handle_ready(gfbe_ctx *c, const gfbe_handle *m, const char *who, const char *noun = "handle") {
  const gfbe_status st = handle_device(c, m, who);
  if (st != GFBE_OK) return st;
  return m->owner == c ? GFBE_OK : handle_bad(c, who, (std::string("the ") + noun + " belongs to another context").c_str());
}

}  // namespace gfd

// ---- the two table handles more than one translation unit reads (FtabDev, LtabDev: gfbe_device.h)
struct gfbe_ftab : gfbe_handle {
  gfd::FtabDev d;
  int cur = 0;
  // gfbe_batch_upload_tables reads the tables on the context's COPY stream, beside the solves queued on the main one: it waits for
  // ev_ops (recorded on the main stream behind every table operation) and leaves ev_read behind its last reader; the next table
  // operation waits for that one (read_pending)
  hipEvent_t ev_ops = nullptr, ev_read = nullptr;
  bool read_pending = false;
  bool err_seen = false;      // a table's sticky error flag (d.err) came back set from an add_frame: what gfbe_gate_* refuses without a copy
};

struct gfbe_ltab : gfbe_handle {
  gfd::LtabDev d;
  int cur = 0;
  gfd::DevBuf reduce_buf;        // gfbe_ltab_reduce's scratch and output staging, kept between calls (gfbe_line_reduce.hip)
  // the step half of a joint iteration (gfbe_ltab_keep_records / gfbe_ltab_step / gfbe_ltab_commit, gfbe_line_step.hip)
  unsigned long long gen = 0;    // bumped by every operation that may change the tables
  bool keep_records = false;
  gfd::DevBuf rec_buf;           // the per-line store of a solve-mode reduce: rec_off [W + 1], then Vinv, bl, W, V, failed per line slot
  bool rec_valid = false;
  unsigned long long rec_gen = 0;
  double rec_mu = 0.0;
  std::vector<double> rec_pose;  // [W][77] poses then [W][7] extrinsics of that reduce, bit for bit
  std::vector<int> rec_off, rec_ne;      // [W + 1] first slot of a table, [W] entering lines
  const double *rec_Vinv = nullptr, *rec_bl = nullptr, *rec_W = nullptr, *rec_V = nullptr;
  const unsigned char *rec_failed = nullptr;
  const int *rec_off_d = nullptr;
  gfd::DevBuf step_buf;          // gfbe_ltab_step's inputs, outputs and the candidates, kept between calls
  bool cand_valid = false;
  const double *cand_plk = nullptr;      // [slots][6]
  const int *cand_lineof = nullptr, *cand_ne = nullptr;      // [slots] line of a record, [W] entering lines
};
