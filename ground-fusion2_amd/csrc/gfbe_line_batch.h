// gfbe_line_batch.h — the host side gfbe_line.hip, gfbe_line_reduce.hip and gfbe_line_step.hip share: the validation and the packing of
// gfbe_line_window[] into a LineList (gfbe_line.h) on the device, the LineList of the line tables, and the small pieces of the
// hand-over (error check, aligned arena, kept allocations, downloads). Plain helpers: every entry point keeps its own argument
// checks, launch and outputs.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_handle.h"
#include "gfbe_line.h"

namespace gfd {

inline size_t up8(size_t b) { return (b + 255) & ~(size_t)255; }

// Arrays laid out one after another at 256-byte steps from `base`. From a null base nothing is addressed: the same layout code run
// twice gives first the size of the allocation, then the pointers into it.
struct Arena {
  char *base;
  size_t off = 0;
  explicit Arena(char *b) : base(b) {}
  template <class T>
  T *take(size_t n) {
    T *p = base ? (T *)(base + off) : nullptr;
    off += up8(sizeof(T) * n);
    return p;
  }
};

// b holds at least `need` bytes afterwards; its contents do not survive a growth (the stream is drained before the old block goes)
inline hipError_t grow(hipStream_t s, DevBuf &b, size_t need) {
  if (b.cap >= need) return hipSuccess;
  if (b.d) {
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    (void)hipFree(b.d);
    b.d = nullptr; b.cap = 0;
  }
  const hipError_t e = hipMalloc((void **)&b.d, need);
  if (e == hipSuccess) b.cap = need;
  return e;
}
// layout(base) -> bytes (an Arena over base): sized from a null base, b grown to it, then laid out in b
template <class Layout>
inline hipError_t lay_out(hipStream_t s, DevBuf &b, Layout layout) {
  const hipError_t e = grow(s, b, layout(nullptr));
  if (e == hipSuccess) (void)layout(b.d);
  return e;
}

// n elements from the device into v (at least one element long), behind the work queued on s
template <class T>
inline hipError_t download(std::vector<T> &v, const T *d, size_t n, hipStream_t s) {
  v.resize(std::max<size_t>(n, 1));
  return n ? hipMemcpyAsync(v.data(), d, sizeof(T) * n, hipMemcpyDeviceToHost, s) : hipSuccess;
}

// the current half of the line tables as a LineList (pose7 / ex_cam: on the device)
inline LineList ltab_line_list(const gfbe_ltab &t, const double *pose7, const double *ex_cam) {
  const int b = t.cur;
  LineList L{};
  L.count = t.d.count; L.nobs = t.d.nobs[b]; L.F = t.d.F;
  L.start = t.d.start[b]; L.tri = t.d.tri[b]; L.plk_in = t.d.plk[b]; L.obs = t.d.obs[b];
  L.pose = pose7; L.ex = ex_cam;
  return L;
}

// ---- gfbe_line_window[] -> LineList, in two phases (an entry point has checks of its own between them)
struct LineWindows {
  std::vector<int> line_off;      // [n_windows + 1] first line of a window in the batch
  std::vector<int> entering;      // [n_windows] lines that pass line_eligible (what a solve-mode reduce reports as n_eligible)
  size_t n_obs = 0;               // observations of the batch
  int n_lines() const { return line_off.back(); }
};
// Phase one, host only: sizes, frames and pointers of every window (observation VALUES are not looked at). `who`: the entry point,
// for the error text; max_lines: the bound of the batch's line count (the kernels' scratch per line must stay within 32-bit indices).
inline bool check_line_windows(gfbe_ctx *c, const char *who, int n_windows, const gfbe_line_window *const *win, size_t max_lines, LineWindows &B) {
  auto refuse = [&](const char *what) { ctx_set_error(c, (std::string(who) + what).c_str()); return false; };
  B.line_off.assign((size_t)n_windows + 1, 0);
  B.entering.assign((size_t)n_windows, 0);
  B.n_obs = 0;
  for (int w = 0; w < n_windows; w++) {
    const gfbe_line_window *L = win[w];
    if (!L || L->struct_size != (int32_t)sizeof(gfbe_line_window)) return refuse(": gfbe_line_window ABI mismatch");
    if (L->n_lines < 0 || (L->n_lines > 0 && (!L->start_frame || !L->n_obs || !L->is_triangulation || !L->line_plucker))) return false;
    size_t no = 0;
    for (int i = 0; i < L->n_lines; i++) {
      const int s = L->start_frame[i], k = L->n_obs[i];
      if (s < 0 || k < 0 || s + k > GFBE_NFRAMES) return refuse(": a line's observations run past the window");
      no += (size_t)k;
      B.entering[w] += (k >= 5 && s < GFBE_WINDOW_SIZE - 2 && L->is_triangulation[i]) ? 1 : 0;
    }
    if (no > 0 && !L->obs) return false;
    if ((size_t)B.line_off[w] + (size_t)L->n_lines > max_lines || B.n_obs + no > (size_t)INT32_MAX / 8) return false;
    B.line_off[w + 1] = B.line_off[w] + L->n_lines;
    B.n_obs += no;
  }
  return true;
}
// Phase two: ints (line_off, obs_off, start), then doubles (plucker, obs, poses, extrinsics), then the triangulation flags, packed on
// the host and copied into ONE device allocation with `extra` bytes of the caller's behind them. The copies are asynchronous: the
// structure (it owns the host buffers) lives until the stream is synchronised; the caller frees d.
struct LineUpload {
  std::vector<int> ints;
  std::vector<double> dbl;
  std::vector<unsigned char> tri;
  char *d = nullptr, *extra = nullptr;      // the allocation, the caller's region in it
  LineList L{};
};
inline hipError_t upload_line_windows(hipStream_t s, int n_windows, const gfbe_line_window *const *win, const LineWindows &B, size_t extra,
                                      LineUpload &U) {
  const int n_lines = B.n_lines();
  U.ints.resize((size_t)n_windows + 1 + 2 * (size_t)n_lines + 1);
  int *h_line_off = U.ints.data(), *h_obs_off = h_line_off + n_windows + 1, *h_start = h_obs_off + n_lines + 1;
  U.dbl.resize((size_t)6 * n_lines + 4 * B.n_obs + 84 * (size_t)n_windows);
  double *h_plk = U.dbl.data(), *h_obs = h_plk + 6 * (size_t)n_lines, *h_pose = h_obs + 4 * B.n_obs, *h_ex = h_pose + 77 * (size_t)n_windows;
  U.tri.resize(std::max(n_lines, 1));
  size_t o = 0;
  for (int w = 0; w < n_windows; w++) {
    const gfbe_line_window *L = win[w];
    h_line_off[w] = B.line_off[w];
    std::memcpy(h_pose + 77 * (size_t)w, L->pose, sizeof(double) * 77);
    std::memcpy(h_ex + 7 * (size_t)w, L->ex_cam, sizeof(double) * 7);
    size_t lo = 0;
    for (int i = 0; i < L->n_lines; i++) {
      const int l = B.line_off[w] + i;
      h_obs_off[l] = (int)o; h_start[l] = L->start_frame[i]; U.tri[l] = L->is_triangulation[i] ? 1 : 0;
      std::memcpy(h_plk + 6 * (size_t)l, L->line_plucker + 6 * (size_t)i, sizeof(double) * 6);
      if (L->n_obs[i] > 0) std::memcpy(h_obs + 4 * o, L->obs + 4 * lo, sizeof(double) * 4 * L->n_obs[i]);
      o += L->n_obs[i]; lo += L->n_obs[i];
    }
  }
  h_line_off[n_windows] = n_lines;
  h_obs_off[n_lines] = (int)o;
  Arena a(nullptr);
  (void)a.take<int>(U.ints.size()); (void)a.take<double>(U.dbl.size()); (void)a.take<unsigned char>(U.tri.size());
  hipError_t e = hipMalloc((void **)&U.d, a.off + extra);
  if (e != hipSuccess) return e;
  a = Arena(U.d);
  int *d_int = a.take<int>(U.ints.size());
  double *d_dbl = a.take<double>(U.dbl.size());
  unsigned char *d_tri = a.take<unsigned char>(U.tri.size());
  U.extra = U.d + a.off;
  U.L.line_off = d_int; U.L.obs_off = d_int + (h_obs_off - h_line_off); U.L.start = d_int + (h_start - h_line_off);
  U.L.plk_in = d_dbl; U.L.obs = d_dbl + (h_obs - h_plk); U.L.pose = d_dbl + (h_pose - h_plk); U.L.ex = d_dbl + (h_ex - h_plk);
  U.L.tri = d_tri;
  if ((e = hipMemcpyAsync(d_int, U.ints.data(), sizeof(int) * U.ints.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(d_dbl, U.dbl.data(), sizeof(double) * U.dbl.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  return hipMemcpyAsync(d_tri, U.tri.data(), U.tri.size(), hipMemcpyHostToDevice, s);
}

}  // namespace gfd
