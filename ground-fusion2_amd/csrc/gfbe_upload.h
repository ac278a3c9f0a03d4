// gfbe_upload.h — the host arithmetic of a batch upload, free of HIP calls: validation and landmark layout of the windows (plan_upload),
// the allocation sequence of the batch's slab (carve_slab: the upload region — upload_region —, the cleared arrays, the rest; both sets of the
// linearisation's outputs through one pair of helpers) and the packing of one window into the upload region (pack_window). gfbe_host.cpp
// runs these between its HIP calls (upload_one); tests/upload_host_shim.cpp and tests/upload_host_main.cpp run them against plain heap buffers.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gfbe_device.h"

namespace gfd {

// what the scan of one window's factor list leaves for the fill pass
struct WinScan {
  int L = 0, K = 0, slots = 0, n_tiles = 0;
  int sf_tile_begin[NF + 1];
  int pair_begin[NPAIR + 1];
  std::vector<int> slot_rel;      // ABI landmark -> slot relative to the window's first slot
  std::vector<unsigned char> lstart, lm;
  std::string err;
};

// The landmark layout rule: groups by start frame (tile aligned), inside a group longer tracks first. cnt / base hold one entry per
// (start frame s, factors m) bin at [s * stride + (m - m0)], m = m0 .. MAXOBS (the host's scan bins m = 0 .. 10, the device tables'
// histogram m = 3 .. 10 with stride 8); base receives the first slot of every bin, relative to the window's first slot.
inline void layout_landmarks(const int *cnt, int stride, int m0, int *base, WinScan &sc) {
  int slots = 0;
  for (int s = 0; s < NF; s++) {
    sc.sf_tile_begin[s] = slots / LM_TILE;
    int in_group = 0;
    for (int m = MAXOBS; m >= m0; m--) { base[s * stride + (m - m0)] = slots + in_group; in_group += cnt[s * stride + (m - m0)]; }
    slots += (in_group + LM_TILE - 1) / LM_TILE * LM_TILE;
  }
  sc.sf_tile_begin[NF] = slots / LM_TILE;
  sc.slots = slots; sc.n_tiles = slots / LM_TILE;
}
inline void pair_begin_of(const int *pair_cnt, WinScan &sc) {
  int run = 0;
  for (int p = 0; p < NPAIR; p++) { sc.pair_begin[p] = run; run += pair_cnt[p]; }
  sc.pair_begin[NPAIR] = run;
}

// Validates the visual factor list of one window and lays its landmarks out (layout_landmarks; ties in ABI order: a stable counting
// sort over the (start, m) bins).
inline bool scan_window(const gfbe_window &win, int w, WinScan &sc) {
  const int L = win.n_feature, K = win.vis.n_factor;
  sc.L = L; sc.K = K;
  auto fail = [&](const std::string &m) { sc.err = "window " + std::to_string(w) + ": " + m; return false; };
  if (L > 0 && !win.para_Feature) return fail("para_Feature is null");
  if (K > 0 && (!win.vis.feature_index || !win.vis.imu_i || !win.vis.imu_j || !win.vis.pts_i || !win.vis.pts_j || !win.vis.vel_i ||
                !win.vis.vel_j || !win.vis.td_i || !win.vis.td_j)) return fail("null visual factor array");
  sc.lstart.assign(L, 255); sc.lm.assign(L, 0);
  std::vector<unsigned short> mask(L, 0);
  int pair_cnt[NPAIR];
  for (int p = 0; p < NPAIR; p++) pair_cnt[p] = 0;
  for (int k = 0; k < K; k++) {
    const int l = win.vis.feature_index[k], i = win.vis.imu_i[k], j = win.vis.imu_j[k];
    if (l < 0 || l >= L || i < 0 || j <= i || j > win.frame_count) return fail("bad visual factor " + std::to_string(k));
    if (sc.lstart[l] == 255) sc.lstart[l] = (unsigned char)i;
    if (sc.lstart[l] != i) return fail("visual factors of one landmark must share imu_i");
    const unsigned short bit = (unsigned short)(1u << (j - i - 1));
    if (mask[l] & bit) return fail("two visual factors of one landmark on the same frame");
    mask[l] |= bit; sc.lm[l]++;
    pair_cnt[i * NF + j]++;
  }
  int bin_cnt[NF][MAXOBS + 1];
  for (int s = 0; s < NF; s++) for (int m = 0; m <= MAXOBS; m++) bin_cnt[s][m] = 0;
  for (int l = 0; l < L; l++) {
    if (sc.lstart[l] == 255) sc.lstart[l] = 0;
    const int m = sc.lm[l];
    if (m > MAXOBS) return fail("landmark with more than 10 factors");
    if (mask[l] != (unsigned short)((1u << m) - 1)) return fail("landmark track must be contiguous from start_frame (feature_per_frame order)");
    bin_cnt[sc.lstart[l]][m]++;
  }
  int bin_base[NF][MAXOBS + 1];
  layout_landmarks(&bin_cnt[0][0], MAXOBS + 1, 0, &bin_base[0][0], sc);
  sc.slot_rel.resize(L);
  for (int l = 0; l < L; l++) sc.slot_rel[l] = bin_base[sc.lstart[l]][sc.lm[l]]++;
  pair_begin_of(pair_cnt, sc);
  return true;
}

// The same layout for a window whose landmarks live in the device tables: counts = [L, K, FT_BINS bins] as launch_ftab_count leaves
// them, lay = the window's row of the layout table for the pack kernel (its first entry, lm_off, is set when the batch-wide offsets are).
inline void scan_table_counts(const int *counts, int *lay, WinScan &sc) {
  const int *cnt = counts + 2;
  sc.L = counts[0]; sc.K = counts[1];
  layout_landmarks(cnt, 8, 3, lay + FT_LAY_BIN, sc);
  for (int s = 0; s < NF; s++) lay[FT_LAY_GRP + s] = sc.sf_tile_begin[s] * LM_TILE;
  // factors of pair (s, s+1+k) = landmarks of start frame s with more than k factors
  int pair_cnt[NPAIR];
  for (int p = 0; p < NPAIR; p++) pair_cnt[p] = 0;
  for (int s = 0; s < NF; s++)
    for (int k = 0; k < MAXOBS && s + 1 + k < NF; k++)
      for (int m = std::max(k + 1, 3); m <= MAXOBS; m++) pair_cnt[s * NF + s + 1 + k] += cnt[s * 8 + (m - 3)];
  pair_begin_of(pair_cnt, sc);
  std::memcpy(&lay[FT_LAY_PAIR], sc.pair_begin, sizeof(int) * (NPAIR + 1));
}

// Upper bound of the tangent size of the prior a marginalisation of this window can return (MarginalizationInfo::n): the
// blocks the marginalisation set touches (k_marg builds the same table on the device) minus the dropped ones.
inline int prior_out_bound(const gfbe_window &win, const int *pair_begin, bool old) {
  bool touched[GFBE_BLK_COUNT];
  for (int q = 0; q < GFBE_BLK_COUNT; q++) touched[q] = false;
  const gfbe_prior *pr = (win.prior && win.prior->valid && win.prior->n > 0) ? win.prior : nullptr;
  if (pr) for (int q = 0; q < pr->n_blocks; q++) touched[pr->block_id[q]] = true;
  if (!old) return pr ? pr->n : 0;
  for (int k = 0; k < win.n_imu; k++) if (win.imu_frame[k] == 0) touched[0] = touched[GFBE_BLK_SB0] = touched[1] = touched[GFBE_BLK_SB0 + 1] = true;
  for (int k = 0; k < win.n_wheel; k++)
    if (win.wheel_frame[k] == 0) touched[0] = touched[1] = touched[GFBE_BLK_EX_WHEEL] = touched[GFBE_BLK_SX] = touched[GFBE_BLK_SY] = touched[GFBE_BLK_SW] = touched[GFBE_BLK_TD_WHEEL] = true;
  if (win.use_plane && win.frame_count > 0) touched[0] = touched[GFBE_BLK_EX_WHEEL] = touched[GFBE_BLK_PLANE_R] = touched[GFBE_BLK_PLANE_Z] = true;
  if (win.gnss_ready) {
    touched[0] = touched[GFBE_BLK_SB0] = touched[1] = touched[GFBE_BLK_SB0 + 1] = touched[GFBE_BLK_YAW_ENU] = touched[GFBE_BLK_ANC_ECEF] = true;
    for (int k = 0; k < 4; k++) touched[GFBE_BLK_RCV_DT0 + 4 + k] = true;
    touched[GFBE_BLK_RCV_DDT0 + 1] = true;
  }
  if (pair_begin) { for (int j = 1; j < NF; j++) if (pair_begin[j + 1] > pair_begin[j]) touched[0] = touched[j] = touched[GFBE_BLK_EX_CAM] = touched[GFBE_BLK_TD] = true; }
  else for (int q = 0; q < NF; q++) touched[q] = touched[GFBE_BLK_EX_CAM] = touched[GFBE_BLK_TD] = true;   // (table-fed: pair counts live on the device)
  int n = 0;
  for (int q = 0; q < GFBE_BLK_COUNT; q++) if (touched[q] && q != 0 && q != GFBE_BLK_SB0) n += blk_lsize(q);
  return std::min(n, (int)ND);
}

// the facts of the context a plan depends on
struct UploadContext {
  bool allreduce = false;       // an all-reduce hook is installed (gfbe_set_allreduce)
  bool want_records = false;    // gfbe_eval_factors: the block-CSR record array is allocated
  int rank = 0, world = 1;
};

// Everything about a batch that follows from its windows, the options and the context alone: sizes, offsets and the batch flags.
struct UploadPlan {
  int B = 0;
  bool table_fed = false;
  UploadContext cx;
  std::vector<WinScan> scan;
  std::vector<WinDesc> desc;      // (only the offset fields are set; pack_window completes the descriptors in the mirror)
  std::vector<int> tile_start, feat_off;
  std::vector<long long> j0_off;
  std::vector<unsigned char> anchor_only;   // window: MARGIN_SECOND_NEW meets an invalid prior that lists Pose[WINDOW_SIZE-1] (estimator.cpp:3622-3632)
  std::vector<int> tlayout;       // table-fed: the layout table for the pack kernel
  int tot_lm = 0, tot_rec = 0, tot_n0 = 0, n_imu_tot = 0, n_wheel_tot = 0, tot_lio = 0, tot_gnss = 0, gnss_max = 0, pn_max = 0, marg_nmax = 0;
  int max_tiles = 0, max_sf_tiles = 0;
  double algo_bytes = 0.0;
  int vis_full = 0, obs_compact = 0, any_plane = 0, prior_n_max = 0, any_gnss = 0, nu = 0, solve_big = 0, spec = 0, linschur = 0, schur_groups = 0;
  size_t pj_row() const { return (size_t)pn_max * pn_max; }   // J0 of the priors travels compactly: rows of pn_max^2 doubles, spread into the ND^2 slots on the device
};

// Validates the windows (ALL of it: packing cannot fail afterwards), lays their landmarks out and adds up the batch. tcounts: table-fed
// batches, the per-window [L, K, bins] counts fetched from the device (wins[w]->vis, n_feature, para_Feature, feature_const are then
// ignored); nullptr: host-fed. for_each_window(n, fn) runs fn(w) for w in [0, n), in parallel if it likes.
template <class ForEachWindow>
gfbe_status plan_upload(const gfbe_options &opt, const UploadContext &cx, int B, const gfbe_window *const *wins, const int *tcounts,
                        ForEachWindow &&for_each_window, UploadPlan &p, std::string &err) {
  const bool tabs = tcounts != nullptr;
  auto refuse = [&](int w, const std::string &m) { err = "window " + std::to_string(w) + ": " + m; return GFBE_BAD_INPUT; };
  for (int w = 0; w < B; w++) {
    const gfbe_window *win = wins[w];
    if (!win) return refuse(w, "null pointer");
    if (win->frame_count < 0 || win->frame_count > GFBE_WINDOW_SIZE || win->n_imu < 0 || win->n_imu > MAX_IMU || win->n_wheel < 0 || win->n_wheel > MAX_WHEEL ||
        (!tabs && (win->n_feature < 0 || win->vis.n_factor < 0)) || (win->n_imu > 0 && (!win->imu || !win->imu_frame)) ||
        (win->n_wheel > 0 && (!win->wheel || !win->wheel_frame))) return refuse(w, "bad sizes");
  }
  if (cx.allreduce && opt.max_solver_time_in_seconds > 0.0) {
    // (every rank would stop on its own clock: the replicated dense state would diverge between the ranks)
    err = "max_solver_time_in_seconds is not available with landmark sharding (gfbe_set_allreduce)"; return GFBE_BAD_INPUT;
  }
  p.B = B; p.table_fed = tabs; p.cx = cx;
  p.scan.resize(B);
  p.anchor_only.assign(B, 0);
  // ---- pass 1 (parallel over windows): validate the factor lists, lay the landmarks out
  if (tabs) {
    p.tlayout.assign((size_t)B * FT_LAY_STRIDE, 0);
    for (int w = 0; w < B; w++) {
      const int *counts = tcounts + (size_t)w * (FT_BINS + 2);
      if (counts[0] < 0 || counts[1] < 0) return refuse(w, "bad sizes");
      scan_table_counts(counts, &p.tlayout[(size_t)w * FT_LAY_STRIDE], p.scan[w]);
    }
  } else {
    std::atomic<int> bad(-1);
    for_each_window(B, [&](int w) { if (!scan_window(*wins[w], w, p.scan[w])) { int e = -1; bad.compare_exchange_strong(e, w); } });
    if (bad.load() >= 0) { err = p.scan[bad.load()].err; return GFBE_BAD_INPUT; }
  }
  // ---- serial: offsets of every window in the batch-wide arrays
  p.desc.resize(B);
  p.feat_off.assign(B + 1, 0);
  p.j0_off.assign(B + 1, 0);
  int gnss_dims = 0;
  for (int w = 0; w < B; w++) {
    const gfbe_window &win = *wins[w];
    const WinScan &sc = p.scan[w];
    WinDesc &ds = p.desc[w];
    std::memset(&ds, 0, sizeof ds);
    ds.L = sc.L; ds.K = sc.K; ds.frame_count = win.frame_count;
    ds.lm_off = p.tot_lm; ds.lm_slots = sc.slots; ds.n_tiles = sc.n_tiles; ds.tile_off = (int)p.tile_start.size();
    ds.rec_off = p.tot_rec;
    ds.vel_off = p.tot_n0;
    p.tot_n0 += tabs ? 0 : sc.pair_begin[NF];      // (records of the pairs (0, j): pair index i * NF + j, i-major)
    for (int s = 0; s < NF; s++) for (int t = sc.sf_tile_begin[s]; t < sc.sf_tile_begin[s + 1]; t++) p.tile_start.push_back(s);
    if (tabs) p.tlayout[(size_t)w * FT_LAY_STRIDE] = p.tot_lm;
    p.tot_lm += sc.slots; p.tot_rec += sc.K; p.max_tiles = std::max(p.max_tiles, sc.n_tiles);
    for (int s = 0; s < NF; s++) p.max_sf_tiles = std::max(p.max_sf_tiles, sc.sf_tile_begin[s + 1] - sc.sf_tile_begin[s]);
    ds.imu_off = p.n_imu_tot; ds.wheel_off = p.n_wheel_tot; ds.lio_off = p.tot_lio;
    p.n_imu_tot += win.n_imu; p.n_wheel_tot += win.n_wheel; p.tot_lio += win.lio.n > 0 ? win.lio.n : 0;
    for (int k = 0; k < win.n_imu; k++) if (win.imu_frame[k] < 0 || win.imu_frame[k] >= win.frame_count) return refuse(w, "bad imu_frame");
    for (int k = 0; k < win.n_wheel; k++) if (win.wheel_frame[k] < 0 || win.wheel_frame[k] >= win.frame_count) return refuse(w, "bad wheel_frame");
    if (win.lio.n > 0 && (win.lio.frame < 0 || win.lio.frame > win.frame_count || !win.lio.pts || !win.lio.normals || !win.lio.offsets)) return refuse(w, "bad lio block");
    if (win.gnss_ready) {
      if (win.n_gnss < 0 || (win.n_gnss > 0 && !win.gnss_obs)) return refuse(w, "gnss_ready without observations array");
      for (int k = 0; k < win.n_gnss; k++) {
        const gfbe_gnss_obs &o = win.gnss_obs[k];
        if (o.frame < 0 || o.frame > GFBE_WINDOW_SIZE || o.lower_idx < 0 || o.lower_idx >= GFBE_WINDOW_SIZE || (o.lower_idx != o.frame && o.lower_idx != o.frame - 1) ||
            o.sys_idx < 0 || o.sys_idx > 3 || !(o.pr_uura > 0.0) || !(o.dp_uura > 0.0))
          return refuse(w, "GNSS observation " + std::to_string(k) + " has an index or a deviation out of range");
      }
      ds.gnss_ready = 1; ds.n_gnss = win.n_gnss; ds.gnss_off = p.tot_gnss;
      p.tot_gnss += win.n_gnss; p.any_gnss = 1; p.gnss_max = std::max(p.gnss_max, win.n_gnss);
    }
    p.feat_off[w + 1] = p.feat_off[w] + sc.L;
    // MARGIN_SECOND_NEW with an INVALID last_marginalization_info that still lists Pose[WINDOW_SIZE-1] (estimator.cpp:3600, 3622-3632):
    // the reference marginalises a PoseAnchorFactor on Pose[0] with drop set {Pose[0]} — six dims dropped, nothing kept — and ends
    // with a valid, empty MarginalizationInfo. Nothing to compute: gfbe_batch_download hands back exactly that.
    if (win.prior && !win.prior->valid && win.frame_count == GFBE_WINDOW_SIZE && win.prior->n_blocks > 0 && win.prior->n_blocks <= GFBE_MAX_PRIOR_BLOCKS)
      for (int q = 0; q < win.prior->n_blocks; q++) if (win.prior->block_id[q] == GFBE_BLK_POSE0 + GFBE_WINDOW_SIZE - 1) p.anchor_only[w] = 1;
    if (win.prior && win.prior->valid && win.prior->n > 0) {
      const gfbe_prior &pr = *win.prior;
      if (pr.n > ND || pr.n_blocks < 0 || pr.n_blocks > GFBE_MAX_PRIOR_BLOCKS || !pr.J0 || !pr.r0) return refuse(w, "prior too large or without J0 / r0");
      bool seen[GFBE_BLK_COUNT];
      for (int q = 0; q < GFBE_BLK_COUNT; q++) seen[q] = false;
      int xo = 0;
      for (int q = 0; q < pr.n_blocks; q++) {
        const int id = pr.block_id[q];
        if (id < 0 || id >= GFBE_BLK_COUNT || pr.block_size[q] != blk_gsize(id) || seen[id] || pr.block_idx[q] < 0 || pr.block_idx[q] + blk_lsize(id) > pr.n)
          return refuse(w, "prior block table inconsistent (id, size, duplicate or offset out of range)");
        seen[id] = true; xo += pr.block_size[q];
        if (id >= GFBE_BLK_ANC_ECEF) gnss_dims = 1;
      }
      if (xo > (int)PRIOR_X0) { err = "prior x0 too large"; return GFBE_BAD_INPUT; }
      p.pn_max = std::max(p.pn_max, pr.n);
    }
    const int nb = std::max(prior_out_bound(win, tabs ? nullptr : sc.pair_begin, true), prior_out_bound(win, nullptr, false));
    p.j0_off[w + 1] = p.j0_off[w] + (long long)nb * nb;
    p.marg_nmax = std::max(p.marg_nmax, nb);
    p.algo_bytes += 108.0 * sc.K;   // 12 f64 + 3 i32 per visual residual block, J never re-read by the host
  }
  // ---- the batch flags
  p.schur_groups = B >= DENSE_SPLIT_MIN_B ? SCHUR_GROUPS : (cx.allreduce ? NF : 2 * NF);
  for (int w = 0; w < B; w++) if (!wins[w]->ex_cam_const || !wins[w]->td_const) p.vis_full = 1;
  // Host-fed batches that hold td and the camera extrinsic constant everywhere: the observations cross PCIe already shifted to the
  // window's td (two doubles per factor instead of five: k_expand would apply the same shift, projectionTwoFrameOneCamFactor.cpp:
  // 60-61, before anything reads them); velocity and td of an observation travel only for the landmarks that start in frame 0 — the
  // marginalisation's td / extrinsic columns are the only readers (estimator.cpp:3498-3531 takes the factors with imu_i == 0).
  // 378 -> ~200 KB of the 630 KB a 2000-landmark window uploads. (Not for gfbe_eval_factors: its records carry every td column.)
  p.obs_compact = (!tabs && !p.vis_full && !cx.want_records) ? 1 : 0;
  for (int w = 0; w < B; w++) if (wins[w]->use_plane || wins[w]->use_anchor) p.any_plane = 1;
  for (int w = 0; w < B; w++) if (wins[w]->prior && wins[w]->prior->valid) p.prior_n_max = std::max(p.prior_n_max, (int)wins[w]->prior->n);
  p.nu = (p.any_gnss || gnss_dims) ? (int)ND : (int)NC;       // a batch without GNSS blocks never touches the last 59 tangent dims
  p.solve_big = p.nu > NC;                                  // (decided per batch: k_solve / k_solve_chain hold the 187 core dims only)
  if (diag_getenv("GFBE_VIS_FULL")) p.vis_full = 1;   // (diagnostics build only: force the 20-column panel)
  // speculative linearisation (gfbe_options.speculative_linearization): every batch with landmarks gets a second set of the
  // linearisation's outputs (round 6: also with an all-reduce hook — the landmark-sharded solve: the candidate's pass linearises its own
  // tiles, the ranks' candidate costs travel as before; one evaluation pass less per iteration there too. The number of collectives per
  // iteration stays: DESIGN.md section 7)
  p.spec = (opt.speculative_linearization && p.max_tiles > 0) ? 1 : 0;
  // k_linschur (gfbe_options.merge_lin_schur): throughput batches on the 7 x 7 panel, every tile on this rank
  p.linschur = (opt.merge_lin_schur && B >= DENSE_SPLIT_MIN_B && !p.vis_full && !cx.allreduce && p.max_tiles > 0) ? 1 : 0;
  return GFBE_OK;
}

// the batch-level members of BatchDev a plan decides
inline void plan_to_batch(const UploadPlan &p, BatchDev &d) {
  d.tot_lm = p.tot_lm; d.max_tiles = p.max_tiles; d.tot_rec = p.tot_rec; d.tot_lio = p.tot_lio; d.max_sf_tiles = p.max_sf_tiles;
  d.rank = p.cx.rank; d.world = p.cx.world; d.sharded = p.cx.allreduce ? 1 : 0;
  d.schur_groups = p.schur_groups;
  d.vis_full = p.vis_full; d.obs_compact = p.obs_compact; d.any_plane = p.any_plane; d.prior_n_max = p.prior_n_max;
  d.any_gnss = p.any_gnss; d.tot_gnss = p.tot_gnss; d.gnss_max_obs = p.gnss_max; d.marg_nmax = p.marg_nmax;
  d.nu = p.nu; d.solve_big = p.solve_big; d.spec = p.spec; d.linschur = p.linschur;
}

// ---- the upload region: the arrays the host fills, first in the slab, with a mirror at the same offsets in one host buffer
// bytes an array of n elements takes in the slab
template <typename T>
inline size_t slab_bytes_of(size_t n) { return (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255; }
// the next array of an allocation sequence over `base` (nullptr: sizes only)
template <typename T>
inline void slab_take(char *base, size_t &off, T *&ptr, size_t n) { ptr = base ? (T *)(base + off) : nullptr; off += slab_bytes_of<T>(n); }

struct UploadMirror {
  WinDesc *desc; int *tile_start; double *x0;
  gfbe_imu_preint *imu; gfbe_wheel_preint *wheel; double *lio;
  double *prior_r0, *prior_x0;
  int *dl_feat_off; long long *dl_j0_off;
  gfbe_gnss_obs *gnss_obs;
  double *pJ0c;                   // the priors' J0, compact: [B][pj_row]
  int *lm_info, *lm_abi; double *lm_pts, *lam0, *fobs, *fvel;   // host-fed batches only (else nullptr: the pack kernel fills the landmark arrays)
  size_t bytes;                   // of the whole region
};
// The allocation sequence of the upload region over `base` (the slab or its host mirror; nullptr: sizes only).
inline UploadMirror upload_region(const UploadPlan &p, char *base) {
  UploadMirror m;
  std::memset(&m, 0, sizeof m);
  size_t off = 0;
  auto up = [&](auto *&ptr, size_t n) { slab_take(base, off, ptr, n); };
  const size_t B = p.B, TL = p.tot_lm;
  up(m.desc, B); up(m.tile_start, p.tile_start.size()); up(m.x0, B * NA);
  up(m.imu, p.n_imu_tot); up(m.wheel, p.n_wheel_tot); up(m.lio, (size_t)p.tot_lio * 8);
  up(m.prior_r0, B * ND); up(m.prior_x0, B * PRIOR_X0);
  up(m.dl_feat_off, B + 1); up(m.dl_j0_off, B + 1);
  up(m.gnss_obs, std::max(p.tot_gnss, 1));
  up(m.pJ0c, B * p.pj_row());
  if (!p.table_fed) {
    up(m.lm_info, TL); up(m.lm_abi, TL); up(m.lm_pts, 6 * TL); up(m.lam0, TL);
    up(m.fobs, (size_t)p.tot_rec * (p.obs_compact ? 2 : 5)); up(m.fvel, p.obs_compact ? (size_t)std::max(p.tot_n0, 1) * 3 : 1);
  }
  m.bytes = off;
  return m;
}
// the device side of the region: BatchDev's pointers over the slab (pJ0c has no member: it is the source of a device-to-device copy)
inline void point_upload_region(const UploadMirror &m, BatchDev &d) {
  d.desc = m.desc; d.tile_start = m.tile_start; d.x0 = m.x0; d.imu = m.imu; d.wheel = m.wheel; d.lio = m.lio;
  d.prior_r0 = m.prior_r0; d.prior_x0 = m.prior_x0; d.dl_feat_off = m.dl_feat_off; d.dl_j0_off = m.dl_j0_off; d.gnss_obs = m.gnss_obs;
  if (m.lm_info) { d.lm_info = m.lm_info; d.lm_abi = m.lm_abi; d.lm_pts = m.lm_pts; d.lam0 = m.lam0; d.fobs = m.fobs; d.fvel = m.fvel; }
}
// ---- the slab: every device array of a batch, carved from ONE allocation. Two passes over one allocation sequence (carve_slab): a dry
// pass over no base adds up the sizes, the slab comes from the context's cache (or hipMalloc), the second pass hands out the pointers.
// The arrays the host fills come FIRST ("upload region", upload_region above): they have a mirror at the same offsets in one pinned
// host buffer, the packing threads write straight into that mirror, and the whole region crosses PCIe as ONE hipMemcpyAsync. Then the
// arrays the kernels expect zeroed — only they are cleared (one hipMemsetAsync) —, then the ones that are written before they are read.
struct SlabArray { std::string name; size_t off, bytes; };
struct SlabLayout {
  // the whole slab; [0, up_end) upload region, [up_end, zero_end) cleared, the rest written before read; doubles of the [H | g | E | eg | xa] slab
  size_t bytes = 0, up_end = 0, zero_end = 0, slab_n = 0;
  UploadMirror up;                              // the upload region over the base
  std::vector<SlabArray> arrays;                // every array behind the upload region, by name (the second set's: lm_hP2, vis_part2, ...)
};
// One set of the linearisation's outputs (LinSet), once per set, through the carver `al(pointer, name, elements)` of carve_slab: the
// members that start as zeros ...
template <class Carver>
void carve_lin_cleared(Carver &al, const BatchDev &d, LinSet &s, const std::string &sfx, bool own_schur) {
  const size_t B = d.B, TL = d.tot_lm;
  al(s.lm_Hll, "lm_Hll" + sfx, TL); al(s.lm_gl, "lm_gl" + sfx, TL); al(s.lm_hC, "lm_hC" + sfx, (size_t)HC * TL); al(s.lm_sw, "lm_sw" + sfx, TL);
  if (own_schur) al(s.schur_part, "schur_part" + sfx, B * d.schur_groups * SCHUR_STRIDE); else s.schur_part = d.schur_part;
  al(s.imu_part, "imu_part" + sfx, B * MAX_IMU * IMU_PART); al(s.wheel_part, "wheel_part" + sfx, B * MAX_WHEEL * WHEEL_PART);
  al(s.plane_part, "plane_part" + sfx, d.any_plane ? B * MAX_PLANE * PLANE_PART : 1); al(s.anchor_part, "anchor_part" + sfx, d.any_plane ? B * ANCHOR_PART : 1);
  al(s.prior_g, "prior_g" + sfx, B * (ND + 2)); al(s.lio_part, "lio_part" + sfx, B * LIOW_WGS * LIOW_PART);
}
// ... and the members that are written before they are read. vis_stride: doubles per (tile, observation step) slot of vis_part.
template <class Carver>
void carve_lin_written(Carver &al, const BatchDev &d, LinSet &s, const std::string &sfx, size_t vis_stride) {
  const size_t B = d.B, TL = d.tot_lm, ng = std::max(d.tot_gnss, 1);
  al(s.lm_hP, "lm_hP" + sfx, (size_t)MAXOBS * 6 * TL);    // (k_vis writes the rows below a track's length, k_schur masks the others per landmark: 1.0 MB per window)
  al(s.vis_part, "vis_part" + sfx, B * std::max(d.max_tiles, 1) * MAXOBS * vis_stride);   // (a tile's steps below its longest track are written by k_vis, the others never read)
  al(s.gnss_J, "gnss_J" + sfx, ng * 36); al(s.gnss_r, "gnss_r" + sfx, ng * 2); al(s.gnss_cost, "gnss_cost" + sfx, B * 2);
}

// The allocation sequence of the whole slab over `base` (nullptr: sizes only, every pointer null). d: the batch as plan_to_batch left
// it (d.spec may have been taken back since: a slab that did not fit); receives the pointers, vs_blocks and solve_scratch_stride.
// chain_scratch_doubles = solve_chain_scratch_doubles(), sys_pack_doubles = sys_pack_doubles_host(nu, world) (sharded batches): the
// two sizes the kernels' translation units own.
inline SlabLayout carve_slab(const UploadPlan &p, BatchDev &d, char *base, size_t chain_scratch_doubles, size_t sys_pack_doubles) {
  SlabLayout lay;
  const size_t B = p.B, TL = p.tot_lm, tiles = std::max(p.max_tiles, 1);
  const bool small = p.B < DENSE_SPLIT_MIN_B;
  // -- upload region
  lay.up = upload_region(p, base);
  if (base) point_upload_region(lay.up, d);
  size_t off = lay.up_end = lay.up.bytes;
  auto al = [&](auto *&ptr, const std::string &name, size_t n) { const size_t o = off; slab_take(base, off, ptr, n); lay.arrays.push_back({name, o, off - o}); };
  // -- arrays the kernels expect zeroed at the start (rows past a track's length, partials of absent factors, ...)
  if (p.table_fed) { al(d.lm_info, "lm_info", TL); al(d.lm_abi, "lm_abi", TL); al(d.lm_pts, "lm_pts", 6 * TL); al(d.lam0, "lam0", TL); d.fobs = nullptr; d.fvel = nullptr; }
  al(d.raw_imu, "raw_imu", (size_t)MAX_IMU * (15 + 450) * 4 * ((B + 3) / 4)); al(d.raw_wheel, "raw_wheel", (size_t)MAX_WHEEL * (6 + 132) * 4 * ((B + 3) / 4));   // [factor][window / 4][value][window % 4]
  al(d.zero, "zero", 16); al(d.vis_H, "vis_H", B * NV * (NV + 1));
  d.vs_blocks = d.vis_full ? (int)VS_BLOCKS : 1;
  if (small && !d.sharded) al(d.vis_Hs, "vis_Hs", B * d.vs_blocks * NV * (NV + 1)); else d.vis_Hs = nullptr;
  al(d.ctl, "ctl", B);
  al(d.lam, "lam", 2 * TL); al(d.lm_sl, "lm_sl", TL); al(d.lm_yl, "lm_yl", TL); al(d.lm_vl, "lm_vl", TL);
  al(d.imu_sqrt, "imu_sqrt", (size_t)p.n_imu_tot * 225); al(d.wheel_sqrt, "wheel_sqrt", (size_t)p.n_wheel_tot * 36);
  al(d.pair_part, "pair_part", B * NF * VP_STRIDE);
  carve_lin_cleared(al, d, d, "", true);
  // (the second set, cleared like the first; its Schur partial is its own where the candidate's pass eliminates the landmarks too)
  if (d.spec) carve_lin_cleared(al, d, d.lin2, "2", d.linschur != 0); else d.lin2 = LinSet{};
  al(d.tile_cost, "tile_cost", B * tiles); al(d.tile_cand, "tile_cand", B * tiles * 4);
  al(d.tile_cnt, "tile_cnt", small ? B * tiles : 1); al(d.win_cnt, "win_cnt", small ? B * 2 : 1);
  al(d.tile_gram, "tile_gram", B * tiles * 8); al(d.dense_cand, "dense_cand", B * 4);
  al(d.xb, "xb", B * d.world * XCHG); al(d.xc, "xc", B * d.world * XCHG);
  if (d.sharded) { al(d.Er, "Er", B * (NV * NV + NV)); al(d.sys_pack, "sys_pack", B * sys_pack_doubles); } else { d.Er = nullptr; d.sys_pack = nullptr; }
  al(d.sp, "sp", B * ND); al(d.Dp, "Dp", B * ND); al(d.gts, "gts", B * ND); al(d.vp, "vp", B * ND); al(d.yp, "yp", B * ND); al(d.step, "step", B * ND);
  al(d.timing, "timing", (B + 1) * 32);   // (+ one block for the phase stamps of a diagnostics build)
  al(d.mmeta, "mmeta", B * (4 + 3 * GFBE_MAX_PRIOR_BLOCKS)); al(d.mx0, "mx0", B * PRIOR_X0);
  lay.zero_end = off;
  // -- written before they are read: no clearing (block-CSR records only exist for the inspection API)
  al(d.prior_J0, "prior_J0", B * ND * ND);     // (the n x n prior block arrives by copy; nothing reads past it)
  al(d.lm_obs, "lm_obs", (size_t)MAXOBS * 5 * TL); al(d.lm_rec, "lm_rec", (size_t)MAXOBS * TL);   // (k_expand / k_ftab_pack write the rows of a track; the evaluation uses a row only below the track's length: 0.9 of the 2.8 MB per window that used to be cleared)
  carve_lin_written(al, d, d, "", VP_STRIDE);
  // (the second set: the solve's linearisation only — its 7 x 7 partials take VPY_STRIDE doubles per step when no window frees the extrinsic / td)
  if (d.spec) carve_lin_written(al, d, d.lin2, "2", d.vis_full ? (size_t)VP_STRIDE : (size_t)VPY_STRIDE);
  al(d.mA, "mA", B * ND * ND); al(d.mb, "mb", B * ND); al(d.mJ0, "mJ0", B * ND * ND); al(d.mr0, "mr0", B * ND);   // (k_marg / k_marg_ldlt write what they and k_gather read)
  al(d.x, "x", B * 2 * NA); al(d.xout, "xout", B * NA);                 // (k_reset / k_reanchor write them before anything reads)
  al(d.pc, "pc", B * 3 * NPAIR * PAIR_CONST_DOUBLES);                   // (written by the kernels that produce a state)
  al(d.prior_H, "prior_H", B * ND * ND);      // (k_prep writes the n x n block k_assemble reads)
  // (k_assemble writes every entry of H (lower triangle) its table lists, g, E, eg it owns, k_visblock the exchange row: no clearing
  //  here — a batch on the compact table clears H once at upload)
  // the partial reduced system [H | g | E | eg | xa] is one slab: a single all-reduce per linearisation when the
  // landmarks are sharded over ranks
  const size_t nH = B * ND * ND, ng = B * ND, nE = B * NV * NV, ne = B * NV;
  al(d.H, "H", lay.slab_n = nH + ng + nE + ne + B * d.world * XCHG);
  if (base) { d.g = d.H + nH; d.E = d.g + ng; d.eg = d.E + nE; d.xa = d.eg + ne; }
  al(d.dbg_imu, "dbg_imu", B * MAX_IMU * 15 * 31); al(d.dbg_wheel, "dbg_wheel", B * MAX_WHEEL * 6 * 23); al(d.dbg_prior, "dbg_prior", B * ND);
  al(d.rec, "rec", p.cx.want_records ? (size_t)p.tot_rec * REC : 1); al(d.mV, "mV", B * ND * ND);
  al(d.vis_contrib, "vis_contrib", small ? B * tiles * MAXOBS * 16 * LM_TILE : 1);
  d.solve_scratch_stride = d.solve_big ? (size_t)BIG_LD * BIG_LD : chain_scratch_doubles;
  al(d.solveY, "solveY", d.solve_big ? 1 : B * chain_scratch_doubles);
  al(d.solveS, "solveS", d.solve_big ? B * BIG_LD * BIG_LD : 1);
  al(d.gnss_marg, "gnss_marg", d.any_gnss ? B * GN_MPART : 1);
  // (the results last and contiguous: [dl_fix | dl_feat | dl_J0] leave in one device-to-host copy)
  al(d.dl_fix, "dl_fix", B * DL_FIX); al(d.dl_feat, "dl_feat", p.feat_off[B]); al(d.dl_J0, "dl_J0", (size_t)p.j0_off[B]);
  lay.bytes = off;
  return lay;
}

// the batch-wide tables of the region (once per batch, before the windows are packed)
inline void pack_batch_tables(const UploadPlan &p, const UploadMirror &m) {
  if (!p.tile_start.empty()) std::memcpy(m.tile_start, p.tile_start.data(), sizeof(int) * p.tile_start.size());   // (no landmarks: data() may be null)
  std::memcpy(m.dl_feat_off, p.feat_off.data(), sizeof(int) * (p.B + 1));
  std::memcpy(m.dl_j0_off, p.j0_off.data(), sizeof(long long) * (p.B + 1));
}

// ---- pack_window: one window into the mirror. `used`: the parameter blocks some residual of the window touches.
// landmark scalars, observations; slot_of receives ABI landmark -> global slot. Returns the bytes written.
inline double pack_landmarks(const UploadPlan &p, const gfbe_window &win, const WinScan &sc, const WinDesc &ds, const UploadMirror &m,
                             std::vector<int> &slot_of) {
  const size_t TL = p.tot_lm;
  // landmark scalars: padding slots first (valid = 0, abi -1, lambda 1), then the landmarks
  const int o = ds.lm_off;
  for (int q = 0; q < sc.slots; q++) { m.lm_info[o + q] = 0; m.lm_abi[o + q] = -1; m.lam0[o + q] = 1.0; }
  for (int r = 0; r < 6; r++) std::memset(m.lm_pts + r * TL + o, 0, sizeof(double) * sc.slots);
  for (int l = 0; l < sc.L; l++) {
    const int slot = o + sc.slot_rel[l];
    const bool is_const = win.feature_const && win.feature_const[l];
    m.lm_info[slot] = sc.lstart[l] | (sc.lm[l] << 8) | ((is_const ? 1 : 0) << 16) | (1 << 24);
    m.lm_abi[slot] = l;
    m.lam0[slot] = win.para_Feature[l];
  }
  const bool compact = p.obs_compact != 0;
  double *fo = m.fobs + (size_t)ds.rec_off * (compact ? 2 : 5), *fv = compact ? m.fvel + (size_t)ds.vel_off * 3 : nullptr;
  const double tdw = win.state.para_Td;
  for (int k = 0; k < sc.K; k++) {
    const int l = win.vis.feature_index[k], i = win.vis.imu_i[k], j = win.vis.imu_j[k];
    const int rel = sc.slot_rel[l];
    const int rec = sc.pair_begin[i * NF + j] + (rel - sc.sf_tile_begin[i] * LM_TILE);
    if (compact) {
      // p' = p - (td - td_obs) v: k_expand's fused multiply-add (a correctly rounded std::fma is the same number; an observation
      // stamped with the window's td — the usual case — is not touched)
      const double dtj = tdw - win.vis.td_j[k];
      double *f = fo + (size_t)rec * 2;
      f[0] = dtj == 0.0 ? win.vis.pts_j[3 * k] : std::fma(-dtj, win.vis.vel_j[2 * k], win.vis.pts_j[3 * k]);
      f[1] = dtj == 0.0 ? win.vis.pts_j[3 * k + 1] : std::fma(-dtj, win.vis.vel_j[2 * k + 1], win.vis.pts_j[3 * k + 1]);
      if (i == 0) { double *v = fv + (size_t)rec * 3; v[0] = win.vis.vel_j[2 * k]; v[1] = win.vis.vel_j[2 * k + 1]; v[2] = win.vis.td_j[k]; }
    } else {
      double *f = fo + (size_t)rec * 5;
      f[0] = win.vis.pts_j[3 * k]; f[1] = win.vis.pts_j[3 * k + 1]; f[2] = win.vis.vel_j[2 * k]; f[3] = win.vis.vel_j[2 * k + 1]; f[4] = win.vis.td_j[k];
    }
    if (j == i + 1) {   // the landmark's first observation travels with its first factor
      const size_t slot = (size_t)o + rel;
      m.lm_pts[0 * TL + slot] = win.vis.pts_i[3 * k]; m.lm_pts[1 * TL + slot] = win.vis.pts_i[3 * k + 1]; m.lm_pts[2 * TL + slot] = win.vis.pts_i[3 * k + 2];
      m.lm_pts[3 * TL + slot] = win.vis.vel_i[2 * k]; m.lm_pts[4 * TL + slot] = win.vis.vel_i[2 * k + 1]; m.lm_pts[5 * TL + slot] = win.vis.td_i[k];
    }
  }
  slot_of.resize(sc.L);
  for (int l = 0; l < sc.L; l++) slot_of[l] = o + sc.slot_rel[l];
  return (double)sc.slots * (4 + 4 + 8 + 48) + (compact ? 16.0 * sc.K + 24.0 * sc.pair_begin[NF] : 40.0 * sc.K);
}

// dense state, inertial factors, and the optional in-window factors' descriptor fields: PlaneFactor on every pose i < frame_count
// (estimator.cpp:3214-3220), PoseAnchorFactor on Pose[0]
inline double pack_dense(int w, const gfbe_window &win, WinDesc &ds, const UploadMirror &m) {
  std::memcpy(m.x0 + (size_t)w * NA, &win.state, sizeof(double) * NA);
  for (int q = 0; q < NF; q++) ds.imu_of_frame[q] = ds.wheel_of_frame[q] = -1;
  ds.n_imu = win.n_imu;
  for (int k = 0; k < win.n_imu; k++) { m.imu[ds.imu_off + k] = win.imu[k]; ds.imu_frame[k] = win.imu_frame[k]; ds.imu_of_frame[win.imu_frame[k]] = k; }
  ds.n_wheel = win.n_wheel;
  for (int k = 0; k < win.n_wheel; k++) { m.wheel[ds.wheel_off + k] = win.wheel[k]; ds.wheel_frame[k] = win.wheel_frame[k]; ds.wheel_of_frame[win.wheel_frame[k]] = k; }
  ds.n_plane = win.use_plane ? std::min(win.frame_count, (int)MAX_PLANE) : 0;
  ds.use_anchor = win.use_anchor ? 1 : 0;
  for (int q = 0; q < 3; q++) ds.plane_noise_inv[q] = win.plane_noise_inv[q];
  for (int q = 0; q < 7; q++) ds.anchor_pose[q] = win.anchor_pose[q];
  ds.anchor_sqrt_info = win.anchor_sqrt_info;
  std::memcpy(ds.ex_cam_mask, win.ex_cam_mask, 6);
  std::memcpy(ds.ex_wheel_mask, win.ex_wheel_mask, 6);
  return sizeof(WinDesc) + sizeof(double) * NA + sizeof(gfbe_imu_preint) * win.n_imu + sizeof(gfbe_wheel_preint) * win.n_wheel;
}

// LiDAR factors on one pose
inline double pack_lio(const gfbe_window &win, WinDesc &ds, const UploadMirror &m) {
  ds.lio_n = win.lio.n > 0 ? win.lio.n : 0; ds.lio_frame = win.lio.frame;
  ds.lio_sqrt_info = win.lio.sqrt_info; ds.lio_huber = win.lio.huber_delta;
  double *lo = m.lio + (size_t)ds.lio_off * 8;
  for (int k = 0; k < ds.lio_n; k++) {
    for (int q = 0; q < 3; q++) { lo[8 * k + q] = win.lio.pts[3 * k + q]; lo[8 * k + 3 + q] = win.lio.normals[3 * k + q]; }
    lo[8 * k + 6] = win.lio.offsets[k];
    lo[8 * k + 7] = win.lio.weights ? win.lio.weights[k] : 1.0;
  }
  return 64.0 * ds.lio_n;
}

// prior (validated by plan_upload)
inline double pack_prior(const UploadPlan &p, int w, const gfbe_window &win, WinDesc &ds, const UploadMirror &m, bool *used) {
  const size_t pj_row = p.pj_row();
  for (int q = 0; q < ND; q++) ds.prior_map[q] = -1;
  std::memset(m.prior_r0 + (size_t)w * ND, 0, sizeof(double) * ND);
  std::memset(m.prior_x0 + (size_t)w * PRIOR_X0, 0, sizeof(double) * PRIOR_X0);
  if (pj_row) std::memset(m.pJ0c + (size_t)w * pj_row, 0, sizeof(double) * pj_row);
  if (!(win.prior && win.prior->valid && win.prior->n > 0)) return 0.0;
  const gfbe_prior &pr = *win.prior;
  ds.prior_n = pr.n; ds.prior_nblk = pr.n_blocks;
  int xo = 0;
  for (int q = 0; q < pr.n_blocks; q++) {
    const int id = pr.block_id[q];
    ds.prior_blk_id[q] = id; ds.prior_blk_size[q] = pr.block_size[q]; ds.prior_blk_idx[q] = pr.block_idx[q];
    ds.prior_x0_off[q] = xo; xo += pr.block_size[q];
    used[id] = true;
    for (int k = 0; k < blk_lsize(id); k++) ds.prior_map[blk_tan(id) + k] = pr.block_idx[q] + k;
  }
  std::memcpy(m.prior_x0 + (size_t)w * PRIOR_X0, pr.x0, sizeof(double) * xo);
  std::memcpy(m.pJ0c + (size_t)w * pj_row, pr.J0, sizeof(double) * pr.n * pr.n);
  std::memcpy(m.prior_r0 + (size_t)w * ND, pr.r0, sizeof(double) * pr.n);
  return 8.0 * ((double)pr.n * pr.n + pr.n + xo);
}

// GNSS (estimator.cpp:2965-3002, 3239-3291): the observations sorted by frame (stable: the reference's insertion order is
// frame-major already), the lowspeed gate from the window's velocities, the blocks the factors touch
inline double pack_gnss(const gfbe_window &win, WinDesc &ds, const UploadMirror &m, bool *used) {
  if (!ds.gnss_ready) return 0.0;
  int cnt[NF + 1];
  for (int q = 0; q <= NF; q++) cnt[q] = 0;
  for (int k = 0; k < win.n_gnss; k++) cnt[win.gnss_obs[k].frame + 1]++;
  for (int q = 0; q < NF; q++) cnt[q + 1] += cnt[q];
  for (int q = 0; q <= NF; q++) ds.gnss_frame_begin[q] = cnt[q];
  for (int k = 0; k < win.n_gnss; k++) m.gnss_obs[ds.gnss_off + cnt[win.gnss_obs[k].frame]++] = win.gnss_obs[k];
  ds.gnss_has_iono = win.gnss_iono ? 1 : 0;
  for (int q = 0; q < 8; q++) ds.gnss_iono[q] = win.gnss_iono ? win.gnss_iono[q] : 0.0;
  for (int q = 0; q < GFBE_WINDOW_SIZE; q++) ds.gnss_frame_dt[q] = win.gnss_frame_dt[q];
  ds.gnss_ddt_weight = win.gnss_ddt_weight;
  double ax = 0.0, ay = 0.0;
  for (int i = 0; i <= GFBE_WINDOW_SIZE; i++) { ax += std::fabs(win.state.para_SpeedBias[i][0]); ay += std::fabs(win.state.para_SpeedBias[i][1]); }
  ax /= GFBE_WINDOW_SIZE + 1; ay /= GFBE_WINDOW_SIZE + 1;
  ds.gnss_factors = !(std::sqrt(ax * ax + ay * ay) < 0.3);
  if (ds.gnss_factors) {
    for (int k = 0; k < win.n_gnss; k++) {
      const gfbe_gnss_obs &o = win.gnss_obs[k];
      used[o.lower_idx] = used[GFBE_BLK_SB0 + o.lower_idx] = used[o.lower_idx + 1] = used[GFBE_BLK_SB0 + o.lower_idx + 1] = true;
      used[GFBE_BLK_YAW_ENU] = used[GFBE_BLK_ANC_ECEF] = true;
    }
    for (int q = GFBE_BLK_RCV_DT0; q < GFBE_BLK_COUNT; q++) used[q] = true;     // DtDdtFactor / DdtSmoothFactor chains
  }
  return (double)(sizeof(gfbe_gnss_obs) * win.n_gnss);
}

// reduced program: blocks touched by a residual and not constant (Ceres drops the rest)
inline void pack_block_table(const gfbe_window &win, const WinScan &sc, WinDesc &ds, bool *used) {
  if (ds.lio_n > 0) used[ds.lio_frame] = true;
  for (int k = 0; k < win.n_imu; k++) { const int i = win.imu_frame[k]; used[i] = used[GFBE_BLK_SB0 + i] = used[i + 1] = used[GFBE_BLK_SB0 + i + 1] = true; }
  for (int k = 0; k < win.n_wheel; k++) {
    const int i = win.wheel_frame[k];
    used[i] = used[i + 1] = used[GFBE_BLK_EX_WHEEL] = used[GFBE_BLK_SX] = used[GFBE_BLK_SY] = used[GFBE_BLK_SW] = used[GFBE_BLK_TD_WHEEL] = true;
  }
  for (int p = 0; p < NPAIR; p++) if (sc.pair_begin[p + 1] > sc.pair_begin[p]) { used[p / NF] = used[p % NF] = used[GFBE_BLK_EX_CAM] = used[GFBE_BLK_TD] = true; }
  for (int i = 0; i < ds.n_plane; i++) used[i] = true;
  if (ds.n_plane > 0) used[GFBE_BLK_EX_WHEEL] = used[GFBE_BLK_PLANE_R] = used[GFBE_BLK_PLANE_Z] = true;
  if (ds.use_anchor) used[0] = true;
  for (int q = 0; q < GFBE_BLK_COUNT; q++) {
    bool cst;
    if (q < GFBE_BLK_SB0) cst = win.pose_const[q] || q > win.frame_count;
    else if (q < GFBE_BLK_EX_CAM) cst = win.sb_const[q - GFBE_BLK_SB0] || (q - GFBE_BLK_SB0) > win.frame_count;
    else if (q == GFBE_BLK_EX_CAM) cst = win.ex_cam_const;
    else if (q == GFBE_BLK_EX_WHEEL) cst = win.ex_wheel_const;
    else if (q == GFBE_BLK_TD) cst = win.td_const;
    else if (q == GFBE_BLK_TD_WHEEL) cst = win.td_wheel_const;
    else if (q == GFBE_BLK_PLANE_R || q == GFBE_BLK_PLANE_Z) cst = win.plane_const;
    else if (q == GFBE_BLK_YAW_ENU) cst = win.gnss_ready != 0;         // estimator.cpp:2991
    else if (q == GFBE_BLK_ANC_ECEF || q >= GFBE_BLK_RCV_DT0) cst = false;
    else cst = win.ix_wheel_const;
    ds.blk_free[q] = used[q] && !cst;
    if (ds.blk_free[q]) for (int k = 0; k < blk_lsize(q); k++) ds.act[blk_tan(q) + k] = 1;
  }
  ds.act[T_PLR + 3] = 0;   // the plane quaternion's 4th slot only exists in the prior (three tangent dims in the solve)
}

// Window w of a planned batch into the mirror: cannot fail. slot_of: host-fed batches, ABI landmark -> global slot (for the
// download). Returns the bytes the window contributes to the upload.
inline double pack_window(const UploadPlan &p, int w, const gfbe_window &win, const UploadMirror &m, std::vector<int> &slot_of) {
  const WinScan &sc = p.scan[w];
  WinDesc &ds = m.desc[w];
  ds = p.desc[w];
  std::memcpy(ds.sf_tile_begin, sc.sf_tile_begin, sizeof ds.sf_tile_begin);
  std::memcpy(ds.pair_begin, sc.pair_begin, sizeof ds.pair_begin);
  bool used[GFBE_BLK_COUNT];
  for (int q = 0; q < GFBE_BLK_COUNT; q++) used[q] = false;
  double bytes = 0.0;
  if (!p.table_fed) bytes += pack_landmarks(p, win, sc, ds, m, slot_of);
  bytes += pack_dense(w, win, ds, m);
  bytes += pack_lio(win, ds, m);
  bytes += pack_prior(p, w, win, ds, m, used);
  bytes += pack_gnss(win, ds, m, used);
  pack_block_table(win, sc, ds, used);
  return bytes;
}

}  // namespace gfd
