// gfbe_tabstage.h — argument staging of the device handles' operations: the tables (gfbe_ftab, gfbe_ltab), the maps (gfbe_vmap, gfbe_scan,
// gfbe_dmap), the loop database (gfbe_ldb) and the tracker (gfbe_klt), whose chunk the detector and the observer borrow.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gfbe_device.h"

// argument staging of a device handle's operations (the part of gfbe_handle, gfbe_handle.h, that gfd::Staged below works on)
struct gfbe_tab_staging {
  // one device chunk + its pinned host mirror, grown on demand and kept (a hipMalloc / hipFree pair per argument cost more than the
  // kernels: 0.4 ms per call measured)
  char *stage_d = nullptr, *stage_h = nullptr;
  size_t stage_cap = 0;
  // the operations that return nothing (triangulate, setDepth, the erasing ones) do not wait for the device: their arguments go
  // through a ring of small staging slots, a slot is reused when the event recorded behind its operation has passed
  enum { RING = 8, RING_SLOT = 64 << 10 };
  char *ring_d = nullptr, *ring_h = nullptr;
  hipEvent_t ring_ev[RING] = {};
  bool ring_used[RING] = {};
  int ring_next = 0;
};

namespace gfd {

// Exclusive scan of one int per thread over a workgroup of THREADS threads (<= 1024) in thread order; *total = the sum. The
// survivor scan of the order-preserving erasures: every thread owns a contiguous chunk of the list and scans its survivor count.
template <int THREADS>
__device__ __forceinline__ int block_exclusive_scan(int v, int *total, int *lds /* >= 17 ints */) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
  if (lane == 63) lds[wave] = x;
  __syncthreads();
  if (t == 0) { int run = 0; for (int q = 0; q < THREADS / 64; q++) { const int c = lds[q]; lds[q] = run; run += c; } lds[16] = run; }
  __syncthreads();
  const int excl = lds[wave] + x - v;
  *total = lds[16];
  __syncthreads();
  return excl;
}

// Host arguments of one table operation -> the table's staging chunk (one pinned host mirror, ONE host-to-device copy before
// the launch, ONE device-to-host copy of the output range after it, one wait). `need` = upper bound of the staged bytes.
// `defer`: an operation without outputs — its arguments go through a slot of the table's ring and nobody waits; every
// operation runs on the context's stream, so whoever reads a result later (add_frame, check_outliers, size, the solver's
// hand-over) sees the tables after it.
struct Staged {
  gfbe_ctx *c;
  gfbe_tab_staging *t;
  char *bh = nullptr, *bd = nullptr;
  size_t cap = 0, off = 0, ulo = SIZE_MAX, uhi = 0, dlo = SIZE_MAX, dhi = 0;
  int slot = -1;
  bool ok = true;
  struct Out { void *h; size_t off, bytes; };
  std::vector<Out> outs;
  Staged(gfbe_ctx *ctx, gfbe_tab_staging *tab, size_t need, bool defer = false) : c(ctx), t(tab) {
    need += 4096;
    if (defer && t->ring_d && need <= (size_t)gfbe_tab_staging::RING_SLOT) {
      slot = t->ring_next;
      t->ring_next = (slot + 1) % gfbe_tab_staging::RING;
      if (t->ring_used[slot]) (void)hipEventSynchronize(t->ring_ev[slot]);
      bh = t->ring_h + (size_t)slot * gfbe_tab_staging::RING_SLOT; bd = t->ring_d + (size_t)slot * gfbe_tab_staging::RING_SLOT; cap = gfbe_tab_staging::RING_SLOT;
      return;
    }
    if (need > t->stage_cap) {
      (void)hipStreamSynchronize(ctx_stream(c));
      if (t->stage_d) (void)hipFree(t->stage_d);
      if (t->stage_h) (void)hipHostFree(t->stage_h);
      t->stage_d = t->stage_h = nullptr; t->stage_cap = 0;
      const size_t ncap = std::max<size_t>(2 * need, (size_t)1 << 20);
      if (hipMalloc((void **)&t->stage_d, ncap) != hipSuccess || hipHostMalloc((void **)&t->stage_h, ncap) != hipSuccess) { ok = false; return; }
      t->stage_cap = ncap;
    }
    bh = t->stage_h; bd = t->stage_d; cap = t->stage_cap;
  }
  ~Staged() { finish(); }
  template <typename T>
  T *up(const T *h, size_t n) {
    const size_t bytes = (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255;
    if (!ok || off + bytes > cap) { ok = false; return nullptr; }
    if (h && n) { std::memcpy(bh + off, h, n * sizeof(T)); ulo = std::min(ulo, off); uhi = std::max(uhi, off + n * sizeof(T)); }
    T *p = (T *)(bd + off);
    off += bytes;
    return p;
  }
  void flush() {   // before the launch
    if (ok && uhi > ulo) (void)hipMemcpyAsync(bd + ulo, bh + ulo, uhi - ulo, hipMemcpyHostToDevice, ctx_stream(c));
  }
  template <typename T>
  void down(T *h, const T *dptr, size_t n) {     // (operations with outputs are never deferred)
    if (!h || !n || !ok || slot >= 0) return;
    const char *p = (const char *)dptr;
    if (p >= bd && p < bd + cap) {
      const size_t o = (size_t)(p - bd);
      outs.push_back({h, o, n * sizeof(T)});
      dlo = std::min(dlo, o); dhi = std::max(dhi, o + n * sizeof(T));
    } else {
      (void)hipMemcpyAsync(h, dptr, n * sizeof(T), hipMemcpyDeviceToHost, ctx_stream(c));
    }
  }
  void finish() {
    if (slot >= 0) {     // deferred: mark the slot busy until the stream has passed this point
      (void)hipEventRecord(t->ring_ev[slot], ctx_stream(c));
      t->ring_used[slot] = true;
      slot = -2;
      return;
    }
    if (slot == -2 || !bh) return;
    if (dhi > dlo) (void)hipMemcpyAsync(bh + dlo, bd + dlo, dhi - dlo, hipMemcpyDeviceToHost, ctx_stream(c));
    (void)hipStreamSynchronize(ctx_stream(c));
    for (const Out &o : outs) std::memcpy(o.h, bh + o.off, o.bytes);
    outs.clear(); dlo = SIZE_MAX; dhi = 0;
  }
};

}  // namespace gfd
