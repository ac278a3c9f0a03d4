// tests/obs_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host build of gfbe_obs.h for a sanitizer run
// (-fsanitize=address,undefined; never on code loaded into Python): points on every edge of the depth image, on halves, far outside,
// huge and non-finite; ids at both ends of the int32 range and equal ids; empty lists and an empty previous list; the sort at 0, 1, 2,
// 63, 64, 65 and 2048 ids; a prediction whose Z is 0 and a start frame at either end of the window. Every read lies inside its buffer
// or the address sanitizer stops the program. Prints "ok".
#include <stdio.h>

#include <limits>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_obs.h"

using namespace gfd;

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const int cols = 64, rows = 48;
  const double cams[3][8] = {{60.0, 61.0, 31.5, 23.25, 0, 0, 0, 0}, {605.687407, 607.16452123, 323.35155412, 236.66167004, 0.15860811, -0.34018021, -0.00180768, 0.00032313},
                             {58.0, 57.0, 30.0, 25.0, -0.4, 0.2, 0.01, -0.02}};
  // the keys: ascending in id over the whole int32 range, then in index; the parts come back
  if (!(obs_key(-5, 9) < obs_key(-4, 0)) || !(obs_key(-1, 0) < obs_key(0, 0)) || !(obs_key(INT32_MIN, 2047) < obs_key(INT32_MAX, 0)) || !(obs_key(7, 1) < obs_key(7, 2))) return 1;
  for (int32_t id : {INT32_MIN, -1, 0, 1, INT32_MAX}) if (obs_key_id(obs_key(id, 2047)) != id || obs_key_index(obs_key(id, 2047)) != 2047) return 2;
  // the rounding rule of O5
  {
    int x, y;
    bool in;
    obs_depth_index(10.5f, 11.5f, cols, rows, &x, &y, &in);
    if (!in || x != 11 || y != 12) return 3;
    obs_depth_index(-0.5f, 0.f, cols, rows, &x, &y, &in);
    if (in) return 4;      // round(-0.5) = -1
    obs_depth_index(-0.25f, 47.25f, cols, rows, &x, &y, &in);
    if (!in || x != 0 || y != 47) return 5;
  }
  std::vector<uint16_t> depth((size_t)cols * (size_t)rows);
  for (size_t i = 0; i < depth.size(); i++) depth[i] = (uint16_t)(i % 65536);
  std::vector<float> pts;
  const float xs[8] = {-40.f, -0.5f, 0.f, 10.5f, cols - 1.f, cols - 0.5f, cols - 0.75f, cols + 60.f}, ys[8] = {-40.f, -0.5f, 0.f, 11.5f, rows - 1.f, rows - 0.5f, rows - 0.75f, rows + 60.f};
  for (float x : xs) for (float y : ys) { pts.push_back(x); pts.push_back(y); }
  const float wild[6][2] = {{1e30f, 5.f}, {-1e30f, 5.f}, {5.f, 3e9f}, {inf, 2.f}, {3.f, -inf}, {nan, nan}};
  for (const auto &w : wild) { pts.push_back(w[0]); pts.push_back(w[1]); }
  const int n = (int)pts.size() / 2;
  std::vector<int32_t> ids((size_t)n);
  for (int i = 0; i < n; i++) ids[(size_t)i] = (i * 37) % 101 - 50;
  ids[0] = INT32_MAX; ids[1] = INT32_MIN; ids[5] = ids[9];
  for (const auto &cam : cams) {
    std::vector<int32_t> prev_ids, ids_out((size_t)n), cn(4);
    std::vector<float> prev_un, un((size_t)2 * n);
    std::vector<double> obs8((size_t)OBS_OW * n);
    for (int round = 0; round < 3; round++) {
      obs_host_observe(cam, n, pts.data(), ids.data(), (int)prev_ids.size(), prev_ids.data(), prev_un.data(), 0.1, round == 2 ? nullptr : depth.data(), cols, rows, ids_out.data(),
                       obs8.data(), un.data(), cn.data());
      if (cn[0] != n || cn[3] != 1 || cn[1] != (round ? n : 0) || (round == 2 ? cn[2] != 0 : cn[2] == 0)) return 6;
      for (int j = 1; j < n; j++) if (ids_out[(size_t)j] < ids_out[(size_t)j - 1]) return 7;
      prev_ids = ids_out; prev_un = un;
    }
    obs_host_observe(cam, 0, nullptr, nullptr, 0, nullptr, nullptr, 0.1, depth.data(), cols, rows, nullptr, nullptr, nullptr, cn.data());
    if (cn[0] || cn[1] || cn[2] || cn[3]) return 8;
  }
  for (int len : {0, 1, 2, 63, 64, 65, 2048}) {
    std::vector<int32_t> v((size_t)len);
    std::vector<int> order((size_t)len + 1);
    for (int i = 0; i < len; i++) v[(size_t)i] = (int32_t)(((long long)i * 7919) % 4099) - 2000;
    if (obs_host_sort(len, v.data(), order.data())) return 9;
    for (int i = 1; i < len; i++) if (v[(size_t)order[(size_t)i]] <= v[(size_t)order[(size_t)i - 1]]) return 10;
    if (len >= 2) { v[(size_t)len - 1] = v[0]; if (!obs_host_sort(len, v.data(), order.data())) return 11; }
  }
  // O8: a feature at either end of the window, Z == 0, 0 / 0, and the list walk
  {
    double poses[11 * 12] = {0}, tic_ric[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, next[12] = {0, 0, 2.0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int f = 0; f < 11; f++) { poses[12 * f + 3] = poses[12 * f + 7] = poses[12 * f + 11] = 1.0; poses[12 * f] = 0.1 * f; }
    const int32_t fid[4] = {3, 10, 17, 24}, start[4] = {0, 10, 0, 0}, nobs[4] = {7, 2, 7, 7};
    const double dep[4] = {2.0, 3.0, 2.0, 4.0};
    double obs0[4 * 8] = {0};
    for (int f = 0; f < 4; f++) { obs0[8 * f] = 0.1 * f; obs0[8 * f + 1] = -0.05; obs0[8 * f + 2] = 1.0; }
    const float held[5 * 2] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
    const int32_t hid[5] = {24, 3, 99, 17, 10};
    float out[10];
    int got = obs_host_predict(cams[2], 5, held, hid, 4, fid, start, nobs, dep, obs0, 6, poses, tic_ric, next, out);
    if (got != 1 || out[2] != 3.f || out[3] != 4.f || out[4] != 5.f || out[6] != 7.f || out[8] != 9.f) return 12;      // ids 3, 17: Z == 0; 99 unknown; 10 ends at 11; 24 predicts
    got = obs_host_predict(cams[0], 5, held, hid, 4, fid, start, nobs, dep, obs0, 11, poses, tic_ric, next, out);
    if (got != 1 || out[8] == 9.f) return 13;      // the feature that starts at frame 10
    if (obs_host_predict(cams[1], 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 6, poses, tic_ric, next, nullptr) != 0) return 14;
  }
  const double bad[8] = {600, 0.0, 1, 1, 0, 0, 0, (double)nan};
  if (obs_camera_ok(bad) || !obs_camera_ok(cams[1])) return 15;
  printf("ok\n");
  return 0;
}
