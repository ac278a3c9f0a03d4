// TEST INFRASTRUCTURE. The host half of a batch upload (csrc/gfbe_upload.h) as a stand-alone program for the address and undefined-
// behaviour sanitizers (tests/test_upload_host.py::test_sanitized_stand_alone_program builds it with -fsanitize=address,undefined and
// runs it): a handful of windows built here, planned and packed into heap buffers of exactly the planned size — a wrong index in the
// packing is a heap overrun the sanitizer reports. Every plan's slab is carved too (carve_slab), dry and over a heap buffer of exactly the
// dry pass's size, and the first and last byte of every array it lists are written. No HIP call, no GPU.
#include "../ground-fusion2_amd/csrc/gfbe_upload.h"

#include <cstdio>
#include <memory>

using namespace gfd;

namespace {
// one window and the arrays its pointers alias
struct Win {
  gfbe_window w;
  std::vector<int32_t> idx, ii, jj, imu_frame, wheel_frame;
  std::vector<double> pi, pj, vi, vj, tdi, tdj, lam, J0, r0, lio_p, lio_n, lio_o;
  std::vector<uint8_t> fconst;
  std::vector<gfbe_imu_preint> imu;
  std::vector<gfbe_wheel_preint> wheel;
  std::vector<gfbe_gnss_obs> gnss;
  gfbe_prior prior;

  // tracks: (start frame, factors) per landmark; the window of examples/gfbe_minimal.c with inertial factors on every frame pair
  Win(const std::vector<std::pair<int, int>> &tracks, int frame_count = GFBE_WINDOW_SIZE) {
    std::memset(&w, 0, sizeof w);
    std::memset(&prior, 0, sizeof prior);
    w.frame_count = frame_count;
    for (int i = 0; i < GFBE_NFRAMES; i++) { w.state.para_Pose[i][0] = 0.1 * i; w.state.para_Pose[i][6] = 1.0; w.state.para_SpeedBias[i][0] = 1.0; }
    w.state.para_Ex_Pose[6] = w.state.para_Ex_Pose_wheel[6] = 1.0;
    w.ex_cam_const = w.ex_wheel_const = w.ix_wheel_const = w.td_const = w.td_wheel_const = 1;
    for (size_t l = 0; l < tracks.size(); l++) {
      lam.push_back(0.25 + 0.01 * l); fconst.push_back(l % 3 == 0);
      for (int k = 1; k <= tracks[l].second; k++) {
        idx.push_back((int32_t)l); ii.push_back(tracks[l].first); jj.push_back(tracks[l].first + k);
        for (int q = 0; q < 3; q++) { pi.push_back(0.1 * q + 0.01 * l); pj.push_back(0.1 * q - 0.01 * k); }
        for (int q = 0; q < 2; q++) { vi.push_back(0.02 * q); vj.push_back(0.03 + 0.01 * q); }
        tdi.push_back(0.0); tdj.push_back(k % 2 ? 0.0 : 0.004);
      }
    }
    imu.resize(frame_count); wheel.resize(frame_count);
    for (int k = 0; k < frame_count; k++) { imu_frame.push_back(k); wheel_frame.push_back(k); std::memset(&imu[k], 0, sizeof imu[k]); std::memset(&wheel[k], 0, sizeof wheel[k]); imu[k].sum_dt = 0.1 * (k + 1); }
    link();
  }
  void link() {
    w.n_feature = (int32_t)lam.size(); w.para_Feature = lam.data(); w.feature_const = fconst.data();
    w.vis.n_factor = (int32_t)idx.size(); w.vis.feature_index = idx.data(); w.vis.imu_i = ii.data(); w.vis.imu_j = jj.data();
    w.vis.pts_i = pi.data(); w.vis.pts_j = pj.data(); w.vis.vel_i = vi.data(); w.vis.vel_j = vj.data(); w.vis.td_i = tdi.data(); w.vis.td_j = tdj.data();
    w.n_imu = (int32_t)imu.size(); w.imu = imu.data(); w.imu_frame = imu_frame.data();
    w.n_wheel = (int32_t)wheel.size(); w.wheel = wheel.data(); w.wheel_frame = wheel_frame.data();
  }
  void add_prior(const std::vector<int> &blocks) {
    prior.valid = 1; prior.n_blocks = (int32_t)blocks.size();
    int n = 0, xo = 0;
    for (size_t q = 0; q < blocks.size(); q++) {
      prior.block_id[q] = blocks[q]; prior.block_size[q] = blk_gsize(blocks[q]); prior.block_idx[q] = n;
      n += blk_lsize(blocks[q]);
      for (int k = 0; k < prior.block_size[q]; k++) prior.x0[xo++] = 0.5 * k;
    }
    prior.n = n;
    J0.assign((size_t)n * n, 1.5); r0.assign(n, -0.5);     // (exactly n x n and n: a read past them is an overrun too)
    prior.J0 = J0.data(); prior.r0 = r0.data();
    w.prior = &prior;
  }
  void add_gnss(const std::vector<int> &frames) {
    for (size_t k = 0; k < frames.size(); k++) {
      gfbe_gnss_obs o;
      std::memset(&o, 0, sizeof o);
      o.frame = frames[k]; o.lower_idx = std::max(frames[k] - 1, 0); o.sys_idx = (int32_t)(k % 4); o.pr_uura = 1.0; o.dp_uura = 2.0; o.psr = 2e7 + k;
      gnss.push_back(o);
    }
    w.gnss_ready = 1; w.n_gnss = (int32_t)gnss.size(); w.gnss_obs = gnss.data();
  }
  void add_lio(int n) {
    lio_p.assign(3 * n, 1.0); lio_n.assign(3 * n, 0.5); lio_o.assign(n, 0.25);
    w.lio.n = n; w.lio.frame = w.frame_count; w.lio.pts = lio_p.data(); w.lio.normals = lio_n.data(); w.lio.offsets = lio_o.data(); w.lio.weights = nullptr;
    w.lio.sqrt_info = 20.0; w.lio.huber_delta = 0.5;
  }
};

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

// the slab of a plan, with the second set of the linearisation's outputs (where the plan has one) or without it
void carve(const UploadPlan &plan, int with_spec) {
  BatchDev d;
  std::memset(&d, 0, sizeof d);
  d.B = plan.B;
  plan_to_batch(plan, d);
  if (!with_spec) d.spec = 0;
  const size_t chain = 96 * 104, pack = 4321;     // (stand-ins for the sizes the kernels' translation units own)
  const SlabLayout dry = carve_slab(plan, d, nullptr, chain, pack);
  CHECK(d.lm_hP == nullptr && d.lin2.gnss_cost == nullptr && d.dl_J0 == nullptr);
  std::unique_ptr<char[]> buf(new char[dry.bytes]);
  const SlabLayout lay = carve_slab(plan, d, buf.get(), chain, pack);
  CHECK(lay.bytes == dry.bytes && lay.up_end == dry.up_end && lay.zero_end == dry.zero_end && lay.arrays.size() == dry.arrays.size());
  CHECK(lay.up_end == upload_region(plan, nullptr).bytes && lay.up_end <= lay.zero_end && lay.zero_end <= lay.bytes);
  for (const SlabArray &a : lay.arrays) {
    CHECK(a.off >= lay.up_end && a.bytes > 0 && a.off + a.bytes <= lay.bytes);
    buf[a.off] = 1; buf[a.off + a.bytes - 1] = 2;
  }
  double *const *s0 = (double *const *)&d.lin_set(0), *const *s1 = (double *const *)&d.lin_set(1);
  for (size_t k = 0; k < sizeof(LinSet) / sizeof(double *); k++) {
    CHECK(s0[k] != nullptr && (s1[k] != nullptr) == (d.spec != 0));
    *(char *)s0[k] = 3;
    if (s1[k]) *(char *)s1[k] = 4;
  }
  const BatchDev v = lin_view(d, 1);
  CHECK(v.lm_hP == (d.spec ? d.lin2.lm_hP : d.lm_hP) && v.gnss_cost == (d.spec ? d.lin2.gnss_cost : d.gnss_cost) && v.lam == d.lam);
  d.g[0] = 1.0; d.xa[(size_t)plan.B * d.world * XCHG - 1] = 2.0;      // the ends of the [H | g | E | eg | xa] slab's parts
}

// plan + pack into heap buffers of exactly the planned size; returns the status
gfbe_status run(const std::vector<Win *> &set, const int *tcounts, std::string &err) {
  gfbe_options opt;
  std::memset(&opt, 0, sizeof opt);
  opt.speculative_linearization = 1;
  std::vector<const gfbe_window *> wins;
  for (Win *x : set) wins.push_back(&x->w);
  UploadPlan plan;
  auto serial = [](int n, auto &&fn) { for (int w = 0; w < n; w++) fn(w); };
  const gfbe_status st = plan_upload(opt, UploadContext(), (int)wins.size(), wins.data(), tcounts, serial, plan, err);
  if (st != GFBE_OK) return st;
  const size_t bytes = upload_region(plan, nullptr).bytes;
  std::unique_ptr<char[]> buf(new char[bytes]);
  const UploadMirror m = upload_region(plan, buf.get());
  CHECK(m.bytes == bytes);
  pack_batch_tables(plan, m);
  std::vector<int> slot_of;
  for (size_t w = 0; w < wins.size(); w++) {
    pack_window(plan, (int)w, *wins[w], m, slot_of);
    CHECK(m.desc[w].L == plan.scan[w].L && m.desc[w].lm_slots % LM_TILE == 0);
    if (!tcounts) for (int l = 0; l < plan.scan[w].L; l++) CHECK(m.lm_abi[slot_of[l]] == l);
  }
  CHECK(m.dl_feat_off[wins.size()] == plan.feat_off.back());
  carve(plan, 1); carve(plan, 0);
  return GFBE_OK;
}
}  // namespace

int main() {
  std::vector<std::pair<int, int>> edge64(64, {2, 3}), edge65(65, {2, 3}), mix;
  for (int s = 0; s < 8; s++) for (int m = 3; m <= 10 - s; m++) mix.push_back({s, m});
  Win none({}), one({{0, 3}}), w64(edge64), w65(edge65), ten({{0, 10}, {0, 0}, {3, 1}}), small({{0, 3}, {1, 4}, {2, 2}}, 6), pr_a(mix), pr_b(mix), pr_sb(mix), gn(mix), lio(mix), free_td(mix),
      plane(mix);
  pr_a.add_prior({GFBE_BLK_SB0, 1, 2});
  pr_b.add_prior({GFBE_BLK_SB0, 1, 2, 3, 4, 5, GFBE_BLK_EX_WHEEL, GFBE_BLK_EX_CAM, GFBE_BLK_TD});
  pr_sb.add_prior({GFBE_BLK_SB0, GFBE_BLK_SB0 + 2, 1});
  gn.add_gnss({3, 0, 10, 3, 1, 0, 7, 10});
  lio.add_lio(37);
  free_td.w.td_const = 0;
  plane.w.use_plane = plane.w.use_anchor = 1;
  std::vector<Win *> all = {&none, &one, &w64, &w65, &ten, &small, &pr_a, &pr_b, &pr_sb, &gn, &lio, &plane};
  std::string err;
  for (Win *x : all) CHECK(run({x}, nullptr, err) == GFBE_OK);
  CHECK(run(all, nullptr, err) == GFBE_OK);          // compact observations, pn_max above most windows' n
  all.push_back(&free_td);
  CHECK(run(all, nullptr, err) == GFBE_OK);          // a free td: five doubles per observation
  // table-fed: the counts of `mix` (one landmark per (start, factors) bin), three windows
  std::vector<int> counts(3 * (FT_BINS + 2), 0);
  for (int w = 0; w < 3; w++) {
    int *cw = &counts[w * (FT_BINS + 2)];
    for (auto &t : mix) { cw[0]++; cw[1] += t.second; cw[2 + t.first * 8 + (t.second - 3)]++; }
  }
  CHECK(run({&pr_a, &gn, &lio}, counts.data(), err) == GFBE_OK);
  // refusals come before any buffer exists
  lio.w.lio.frame = 11;
  CHECK(run({&one, &lio}, nullptr, err) == GFBE_BAD_INPUT && err == "window 1: bad lio block");
  one.imu_frame[2] = 10;
  CHECK(run({&one}, nullptr, err) == GFBE_BAD_INPUT && err == "window 0: bad imu_frame");
  if (failures) return 1;
  printf("upload_host_main: ok\n");
  return 0;
}
