// tests/gate_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_gate.h for a sanitizer run
// (-fsanitize=address,undefined; never on code loaded into Python). argv[1] is the file tests/gate_cases.py dumps: every case with the
// model's expected outputs of gfbe_gate_frame. Each case is run through gate_frame_host and compared byte for byte, then every table
// through G8 for every (l, r) in both modes, with exact room and with none. Every array is allocated at its exact size, so a read or a
// write outside it stops the program. Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_gate.h"

using namespace gfd;

namespace {
FILE *g_f = nullptr;
template <typename T>
std::vector<T> rd(size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, g_f) != n) { printf("short file\n"); exit(2); }
  return v;
}
template <typename T>
bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
}  // namespace

int main(int argc, char **argv) {
  if (argc < 2 || !(g_f = fopen(argv[1], "rb"))) { printf("usage: gate_host_main CASES\n"); return 2; }
  const int n_cases = rd<int32_t>(1)[0];
  for (int k = 0; k < n_cases; k++) {
    const std::vector<int32_t> iopt = rd<int32_t>(4);
    const std::vector<double> dopt = rd<double>(10);
    GateParams G;
    G.use_wheel = iopt[0]; G.wdetect = iopt[1]; G.min_pair_count = iopt[2]; G.pad = 0;
    G.dis_threshold = dopt[0]; G.wheel_still_norm = dopt[1]; G.preint_still_norm = dopt[2]; G.var_still = dopt[3]; G.var_excited = dopt[4]; G.still_parallax_px = dopt[5];
    G.init_parallax_px = dopt[6]; G.parallax_focal = dopt[7]; G.depth_min = dopt[8]; G.depth_max = dopt[9];
    const size_t B = (size_t)rd<int32_t>(1)[0];
    const std::vector<int32_t> toff = rd<int32_t>(B + 1);
    const size_t N = (size_t)toff[B];
    const std::vector<int32_t> start = rd<int32_t>(N), nobs = rd<int32_t>(N);
    const std::vector<double> obs = rd<double>(N * GATE_NOBS * GATE_OW);
    const std::vector<int32_t> fc = rd<int32_t>(B), ioff = rd<int32_t>(B + 1);
    const std::vector<double> imu = rd<double>(7 * (size_t)ioff[B]), imu_first = rd<double>(6 * B);
    const std::vector<int32_t> woff = rd<int32_t>(B + 1);
    const std::vector<double> wheel = rd<double>(7 * (size_t)woff[B]), wheel_first = rd<double>(6 * B), pose = rd<double>(12 * B), vel_ba = rd<double>(6 * B);
    const double g_norm = rd<double>(1)[0];
    const std::vector<int32_t> sprev = rd<int32_t>(B), foff = rd<int32_t>(B + 1);
    const std::vector<double> frames = rd<double>(4 * (size_t)foff[B]);
    const std::vector<int32_t> e_flags = rd<int32_t>(B), e_ls = rd<int32_t>(B), e_li = rd<int32_t>(B), e_cnt = rd<int32_t>(GATE_NL * B);
    const std::vector<double> e_sum = rd<double>(GATE_NL * B), e_dpi = rd<double>(3 * B), e_dpw = rd<double>(3 * B), e_dis = rd<double>(B), e_var = rd<double>(B),
                              e_pose = rd<double>(12 * B), e_vel = rd<double>(3 * B);
    std::vector<int32_t> flags(B), ls(B), li(B), cnt(GATE_NL * B);
    std::vector<double> sum(GATE_NL * B), dpi(3 * B), dpw(3 * B), dis(B), var(B), po(12 * B), vo(3 * B);
    gate_frame_host(G, iopt[3], (int)B, toff.data(), start.data(), nobs.data(), obs.data(), fc.data(), ioff.data(), imu.data(), imu_first.data(),
                    G.use_wheel ? woff.data() : nullptr, G.use_wheel ? wheel.data() : nullptr, G.use_wheel ? wheel_first.data() : nullptr, pose.data(), vel_ba.data(), g_norm,
                    sprev.data(), foff.data(), frames.data(), flags.data(), ls.data(), li.data(), cnt.data(), sum.data(), dpi.data(), dpw.data(), dis.data(), var.data(), po.data(),
                    vo.data());
    if (!(same(flags, e_flags) && same(ls, e_ls) && same(li, e_li) && same(cnt, e_cnt) && same(sum, e_sum) && same(dpi, e_dpi) && same(dpw, e_dpw) && same(dis, e_dis) &&
          same(var, e_var) && same(po, e_pose) && same(vo, e_vel))) {
      printf("case %d differs from the model\n", k);
      return 1;
    }
    // a second time with every output null
    gate_frame_host(G, iopt[3], (int)B, toff.data(), start.data(), nobs.data(), obs.data(), fc.data(), ioff.data(), imu.data(), imu_first.data(),
                    G.use_wheel ? woff.data() : nullptr, G.use_wheel ? wheel.data() : nullptr, G.use_wheel ? wheel_first.data() : nullptr, pose.data(), vel_ba.data(), g_norm,
                    sprev.data(), foff.data(), frames.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    for (size_t b = 0; b < B; b++) {
      const int n = toff[b + 1] - toff[b];
      const int32_t *s = start.data() + toff[b], *nb = nobs.data() + toff[b];
      const double *o = obs.data() + (size_t)toff[b] * GATE_NOBS * GATE_OW;
      for (int mode = 0; mode < 2; mode++)
        for (int l = 0; l < GATE_NL; l++)
          for (int r = l + 1; r <= GATE_NL; r++) {
            const int c = gate_corres_host(G, mode, n, s, nb, o, l, r, 0, nullptr, nullptr);
            std::vector<double> a(3 * (size_t)c), bb(3 * (size_t)c);
            if (gate_corres_host(G, mode, n, s, nb, o, l, r, c, a.data(), bb.data()) != c || (r == GATE_NL && c != (mode == iopt[3] ? cnt[GATE_NL * b + l] : c))) {
              printf("case %d table %zu: G8 and G5 count differently\n", k, b);
              return 1;
            }
          }
    }
  }
  fclose(g_f);
  printf("ok\n");
  return 0;
}
