// TEST INFRASTRUCTURE. The host half of a batch upload (csrc/gfbe_upload.h) behind a C interface for tests/test_upload_host.py: plan B
// windows, lay the upload region out in a malloc'ed buffer of exactly the planned size, pack every window into it; carve the whole slab of
// the plan (carve_slab) into another one and look at a batch through lin_view. No HIP call.
#include "../ground-fusion2_amd/csrc/gfbe_upload.h"

#include <cstdio>

using namespace gfd;

namespace {
struct Packed {
  UploadPlan plan;
  UploadMirror m;
  char *buf = nullptr;
  std::vector<std::vector<int>> slot_of;
  std::vector<double> win_bytes;
};
// the slab of a plan: the dry pass, then the real one over a malloc'ed buffer of the dry pass's size
struct Carved {
  BatchDev d;
  SlabLayout dry, real;
  UploadMirror alone;       // what upload_region alone returns over the same buffer
  char *buf = nullptr;
};
enum { LIN_SLOTS = sizeof(LinSet) / sizeof(double *) };
static_assert(sizeof(LinSet) == LIN_SLOTS * sizeof(double *), "a LinSet is pointer slots and nothing else");
long long rel(const Carved *c, const void *q) { return q ? (long long)((const char *)q - c->buf) : -1; }
}  // namespace

extern "C" {

// status (gfbe_status) and, when it is not GFBE_OK, the message in err; the handle is null then. tcounts: [B][FT_BINS + 2] or null.
void *uh_pack(const gfbe_options *opt, int allreduce, int want_records, int B, const gfbe_window *const *wins, const int *tcounts, int *status,
              char *err, int errcap) {
  Packed *h = new Packed();
  std::string e;
  UploadContext cx;
  cx.allreduce = allreduce != 0; cx.want_records = want_records != 0;
  auto serial = [](int n, auto &&fn) { for (int w = 0; w < n; w++) fn(w); };
  *status = plan_upload(*opt, cx, B, wins, tcounts, serial, h->plan, e);
  snprintf(err, errcap, "%s", e.c_str());
  if (*status != GFBE_OK) { delete h; return nullptr; }
  const size_t bytes = upload_region(h->plan, nullptr).bytes;
  h->buf = (char *)malloc(bytes);
  h->m = upload_region(h->plan, h->buf);
  h->slot_of.resize(B); h->win_bytes.resize(B);
  pack_batch_tables(h->plan, h->m);
  for (int w = 0; w < B; w++) h->win_bytes[w] = pack_window(h->plan, w, *wins[w], h->m, h->slot_of[w]);
  return h;
}
void uh_free(void *hp) { Packed *h = (Packed *)hp; if (h) { free(h->buf); delete h; } }

// batch totals and flags, in the order of tests/test_upload_host.py::INFO
void uh_info(void *hp, long long *out) {
  const UploadPlan &p = ((Packed *)hp)->plan;
  const long long v[] = {p.tot_lm, p.tot_rec, p.tot_n0, p.n_imu_tot, p.n_wheel_tot, p.tot_lio, p.tot_gnss, p.gnss_max, p.pn_max, p.marg_nmax, p.max_tiles,
                         p.max_sf_tiles, p.vis_full, p.obs_compact, p.any_plane, p.prior_n_max, p.any_gnss, p.nu, p.solve_big, p.spec, p.linschur,
                         p.schur_groups, (long long)((Packed *)hp)->m.bytes, (long long)p.tile_start.size()};
  for (size_t k = 0; k < sizeof v / sizeof v[0]; k++) out[k] = v[k];
}
// the scan of window w: head = L, K, slots, n_tiles; slot_rel [L] (host-fed only)
void uh_scan(void *hp, int w, int *head, int *sf_tile_begin, int *pair_begin, int *slot_rel) {
  const WinScan &sc = ((Packed *)hp)->plan.scan[w];
  head[0] = sc.L; head[1] = sc.K; head[2] = sc.slots; head[3] = sc.n_tiles;
  std::memcpy(sf_tile_begin, sc.sf_tile_begin, sizeof sc.sf_tile_begin);
  std::memcpy(pair_begin, sc.pair_begin, sizeof sc.pair_begin);
  for (size_t l = 0; l < sc.slot_rel.size(); l++) slot_rel[l] = sc.slot_rel[l];
}
// the packed descriptor of window w: head = lm_off, rec_off, vel_off, tile_off, imu_off, wheel_off, lio_off, lio_n, gnss_off, n_gnss, gnss_factors,
// prior_n, n_plane, use_anchor
void uh_desc(void *hp, int w, int *head, unsigned char *act, unsigned char *blk_free, int *gnss_frame_begin, int *prior_map) {
  const WinDesc &ds = ((Packed *)hp)->m.desc[w];
  const int v[] = {ds.lm_off, ds.rec_off, ds.vel_off, ds.tile_off, ds.imu_off, ds.wheel_off, ds.lio_off, ds.lio_n, ds.gnss_off, ds.n_gnss, ds.gnss_factors,
                   ds.prior_n, ds.n_plane, ds.use_anchor};
  for (size_t k = 0; k < sizeof v / sizeof v[0]; k++) head[k] = v[k];
  std::memcpy(act, ds.act, ND);
  std::memcpy(blk_free, ds.blk_free, GFBE_BLK_COUNT);
  std::memcpy(gnss_frame_begin, ds.gnss_frame_begin, sizeof ds.gnss_frame_begin);
  std::memcpy(prior_map, ds.prior_map, sizeof ds.prior_map);
}
// an array of the packed region by name (null: not in this batch)
void *uh_array(void *hp, const char *name) {
  const UploadMirror &m = ((Packed *)hp)->m;
  const struct { const char *n; void *p; } tab[] = {
      {"tile_start", m.tile_start}, {"x0", m.x0}, {"lio", m.lio}, {"prior_r0", m.prior_r0}, {"prior_x0", m.prior_x0}, {"dl_feat_off", m.dl_feat_off},
      {"dl_j0_off", m.dl_j0_off}, {"gnss_obs", m.gnss_obs}, {"pJ0c", m.pJ0c}, {"lm_info", m.lm_info}, {"lm_abi", m.lm_abi}, {"lm_pts", m.lm_pts},
      {"lam0", m.lam0}, {"fobs", m.fobs}, {"fvel", m.fvel}, {"imu", m.imu}, {"wheel", m.wheel}};
  for (const auto &t : tab) if (!strcmp(t.n, name)) return t.p;
  return nullptr;
}
// ---- the slab of the plan. spec_off: with BatchDev::spec taken back (what carve_batch does when the slab does not fit); chain / pack: the two
// sizes the kernels' translation units own
void *uh_carve(void *hp, int spec_off, long long chain, long long pack) {
  const UploadPlan &p = ((Packed *)hp)->plan;
  Carved *c = new Carved();
  std::memset(&c->d, 0, sizeof c->d);
  c->d.B = p.B;
  plan_to_batch(p, c->d);
  if (spec_off) c->d.spec = 0;
  c->dry = carve_slab(p, c->d, nullptr, (size_t)chain, (size_t)pack);
  c->buf = (char *)malloc(c->dry.bytes);
  c->real = carve_slab(p, c->d, c->buf, (size_t)chain, (size_t)pack);
  c->alone = upload_region(p, c->buf);
  return c;
}
void uh_carve_free(void *cp) { Carved *c = (Carved *)cp; if (c) { free(c->buf); delete c; } }
// in the order of tests/test_upload_host.py::CARVE
void uh_carve_info(void *cp, long long *out) {
  const Carved *c = (const Carved *)cp;
  const BatchDev &d = c->d;
  const long long v[] = {(long long)c->dry.bytes, (long long)c->dry.up_end, (long long)c->dry.zero_end, (long long)c->real.bytes, (long long)c->real.up_end,
                         (long long)c->real.zero_end, (long long)c->real.slab_n, (long long)c->dry.slab_n, (long long)c->real.arrays.size(),
                         (long long)c->dry.arrays.size(), LIN_SLOTS, d.spec, d.linschur, d.vis_full, rel(c, d.H), rel(c, d.g), rel(c, d.E), rel(c, d.eg),
                         rel(c, d.xa), d.vs_blocks, (long long)d.solve_scratch_stride, VP_STRIDE, VPY_STRIDE};
  for (size_t k = 0; k < sizeof v / sizeof v[0]; k++) out[k] = v[k];
}
void uh_carve_array(void *cp, int dry, int k, char *name, int cap, long long *off, long long *bytes) {
  const SlabArray &a = (dry ? ((Carved *)cp)->dry : ((Carved *)cp)->real).arrays[k];
  snprintf(name, cap, "%s", a.name.c_str());
  *off = (long long)a.off; *bytes = (long long)a.bytes;
}
// the slots of set `set` (0: the batch's own, 1: lin2) as offsets into the buffer, -1 for a null slot
void uh_carve_slots(void *cp, int set, long long *out) {
  const Carved *c = (const Carved *)cp;
  double *const *slot = (double *const *)&c->d.lin_set(set);
  for (int k = 0; k < LIN_SLOTS; k++) out[k] = rel(c, slot[k]);
}
// the upload region's pointers of the carved batch, then what upload_region alone gives for the same members (offsets, -1: null)
int uh_carve_upload(void *cp, long long *got, long long *want) {
  const Carved *c = (const Carved *)cp;
  const BatchDev &d = c->d;
  const UploadMirror &m = c->alone, &u = c->real.up;
  const void *g[] = {d.desc, d.tile_start, d.x0, d.imu, d.wheel, d.lio, d.prior_r0, d.prior_x0, d.dl_feat_off, d.dl_j0_off, d.gnss_obs, u.pJ0c,
                     m.lm_info ? d.lm_info : nullptr, m.lm_info ? d.lm_abi : nullptr, m.lm_info ? d.lm_pts : nullptr, m.lm_info ? d.lam0 : nullptr, d.fobs, d.fvel};
  const void *w[] = {m.desc, m.tile_start, m.x0, m.imu, m.wheel, m.lio, m.prior_r0, m.prior_x0, m.dl_feat_off, m.dl_j0_off, m.gnss_obs, m.pJ0c,
                     m.lm_info, m.lm_abi, m.lm_pts, m.lam0, m.fobs, m.fvel};
  const int n = (int)(sizeof g / sizeof g[0]);
  for (int k = 0; k < n; k++) { got[k] = rel(c, g[k]); want[k] = rel(c, w[k]); }
  return u.bytes == m.bytes ? n : -1;
}
// lin_view(d, lb) of the carved batch, with BatchDev::spec as it is (spec < 0) or set to `spec`: the bytes of the batch it was called on and of
// the view. Returns sizeof(BatchDev); lay = offsets of the first set and of lin2 inside it, sizeof(LinSet).
int uh_lin_view(void *cp, int lb, int spec, unsigned char *of_d, unsigned char *of_view, int *lay) {
  BatchDev d = ((Carved *)cp)->d;
  if (spec >= 0) d.spec = spec;
  const BatchDev v = lin_view(d, lb);
  if (of_d) { std::memcpy(of_d, &d, sizeof d); std::memcpy(of_view, &v, sizeof v); }
  lay[0] = (int)((const char *)static_cast<const LinSet *>(&d) - (const char *)&d); lay[1] = (int)((const char *)&d.lin2 - (const char *)&d); lay[2] = (int)sizeof(LinSet);
  return (int)sizeof d;
}

// the table-fed entry of the layout rule on one window's [L, K, bins] counts
void uh_table_layout(const int *counts, int *head, int *sf_tile_begin, int *pair_begin, int *lay) {
  WinScan sc;
  scan_table_counts(counts, lay, sc);
  head[0] = sc.L; head[1] = sc.K; head[2] = sc.slots; head[3] = sc.n_tiles;
  std::memcpy(sf_tile_begin, sc.sf_tile_begin, sizeof sc.sf_tile_begin);
  std::memcpy(pair_begin, sc.pair_begin, sizeof sc.pair_begin);
}
int uh_prior_out_bound(const gfbe_window *win, const int *pair_begin, int old) { return prior_out_bound(*win, pair_begin, old != 0); }
void uh_default_options(gfbe_options *o) {   // (the fields a plan reads; the library's gfbe_default_options is not linked here)
  std::memset(o, 0, sizeof *o);
  o->struct_size = (int32_t)sizeof *o; o->speculative_linearization = 1;
}
int uh_sizes(int what) { return what == 0 ? (int)FT_BINS : what == 1 ? (int)FT_LAY_STRIDE : what == 2 ? (int)LM_TILE : (int)sizeof(gfbe_gnss_obs); }

}  // extern "C"
