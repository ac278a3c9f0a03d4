// tests/vmap_host_shim.cpp — TEST HARNESS ONLY. Compiles the __host__ __device__ pieces of the voxel map
// (ground-fusion2_amd/csrc/gfbe_vmap.h: key, moments, eigenvector, a2D, weight) for the HOST so that tests/test_vmap_model.py can pin
// them against tests/vmap_np.py without a GPU, and holds a single-thread host restatement of the voxel map and the association on
// std::unordered_map (hmap_*), written from tests/vmap_np.py: the host leg of tools/diag_vmap_bench.py. Never loaded by the package.
#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_vmap.h"

using namespace gfd;

extern "C" {
// 1 and key [3] when the point has a voxel, 0 when a coordinate is out of the short range
int shim_vmap_key(const double *p, double size, int *key) {
  uint64_t k;
  if (!vmap_key(p, size, &k)) return 0;
  vmap_unpack(k, key, key + 1, key + 2);
  return 1;
}
// neighbours [k][3] -> covariance [6], normal [3]; returns a2D
double shim_vmap_plane(const double *nb, int k, double *cov, double *normal) {
  double bary[3];
  vmap_moments(nb, k, bary, cov);
  return vmap_normal_a2d(cov, normal);
}
void shim_vmap_eig3(const double *cov, double *lam, double *V) { vmap_eig3(cov, lam, V); }
double shim_vmap_weight(double a2d, double d0, double wa, double wn, double power, double max_plane, int min_nn) {
  return vmap_weight(a2d, d0, wa, wn, power, max_plane, min_nn);
}
}

// ---- the host restatement: a hash map of voxels, the sequential insert, the triple loop, a sorted k-nearest
namespace {
struct HMap {
  int P, v, K, min_nn, thr, ncn, max_res;
  double size, min_dist, max_dist, max_plane, power, w_alpha, w_nb;
  std::unordered_map<uint64_t, std::vector<double>> vox;      // points [count][3] in insertion order
};
struct Cand { double d; int visit; const double *p; };
void h_qrot(const double *q, double *R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
void h_world(int ct, const double *pb, const double *pe, double al, const double *p, double *pw) {
  double q[4] = {pb[3], pb[4], pb[5], pb[6]}, t[3] = {pb[0], pb[1], pb[2]}, R[9];
  if (ct) {
    const double *a = pb + 3, *b = pe + 3;
    const double d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    double s0, s1;
    if (std::fabs(d) >= 1.0 - 2.220446049250313e-16) { s0 = 1.0 - al; s1 = al; }
    else { const double th = std::acos(std::fabs(d)), st = std::sin(th); s0 = std::sin((1.0 - al) * th) / st; s1 = std::sin(al * th) / st; }
    if (d < 0) s1 = -s1;
    double nn = 0;
    for (int i = 0; i < 4; i++) { q[i] = s0 * a[i] + s1 * b[i]; nn += q[i] * q[i]; }
    nn = std::sqrt(nn);
    for (int i = 0; i < 4; i++) q[i] /= nn;
    for (int i = 0; i < 3; i++) t[i] = pb[i] * (1 - al) + pe[i] * al;
  }
  h_qrot(q, R);
  for (int i = 0; i < 3; i++) pw[i] = R[3 * i] * p[0] + R[3 * i + 1] * p[1] + R[3 * i + 2] * p[2] + t[i];
}
}  // namespace

extern "C" {
// iopt: max_num_points_in_voxel, voxel_neighborhood, max_number_neighbors, min_number_neighbors, threshold_voxel_occupancy,
// num_closest_neighbors, max_num_residuals; dopt: size_voxel_map, min_distance_points, max_distance, max_dist_to_plane_icp,
// power_planarity, weight_alpha, weight_neighborhood
void *hmap_create(const int *iopt, const double *dopt) {
  HMap *m = new HMap();
  m->P = iopt[0]; m->v = iopt[1]; m->K = iopt[2]; m->min_nn = iopt[3]; m->thr = iopt[4]; m->ncn = iopt[5]; m->max_res = iopt[6];
  m->size = dopt[0]; m->min_dist = dopt[1]; m->max_dist = dopt[2]; m->max_plane = dopt[3]; m->power = dopt[4]; m->w_alpha = dopt[5]; m->w_nb = dopt[6];
  return m;
}
void hmap_destroy(void *h) { delete (HMap *)h; }
void hmap_size(void *h, int *out) {
  HMap *m = (HMap *)h;
  size_t np = 0;
  for (auto &kv : m->vox) np += kv.second.size() / 3;
  out[0] = (int)m->vox.size(); out[1] = (int)np;
}
void hmap_add_points(void *h, int n, const double *pts, int min_num_points) {
  HMap *m = (HMap *)h;
  const double md2 = m->min_dist * m->min_dist;
  for (int i = 0; i < n; i++) {
    const double *p = pts + 3 * (size_t)i;
    uint64_t key;
    if (!vmap_key(p, m->size, &key)) continue;
    auto it = m->vox.find(key);
    if (it == m->vox.end()) {
      if (min_num_points <= 0) m->vox[key] = {p[0], p[1], p[2]};
      continue;
    }
    std::vector<double> &b = it->second;
    const int c = (int)b.size() / 3;
    if (c >= m->P) continue;
    double sq_min = 10 * m->size * m->size;
    for (int j = 0; j < c; j++) sq_min = std::min(sq_min, vmap_sqdist(&b[3 * j], p));
    if (sq_min > md2 && (min_num_points <= 0 || c >= min_num_points)) b.insert(b.end(), p, p + 3);
  }
}
void hmap_erase_far(void *h, const double *loc) {
  HMap *m = (HMap *)h;
  for (auto it = m->vox.begin(); it != m->vox.end();)
    if (vmap_sqdist(it->second.data(), loc) > m->max_dist * m->max_dist) it = m->vox.erase(it); else ++it;
}
// the loop body of addSurfCostFactor; returns n_res; outputs sized max_num_residuals
int hmap_associate(void *h, int ct, int n, const double *raw, const double *alpha, const double *pb, const double *pe, int frame_init, int *src,
                   double *pts, double *normals, double *offsets, double *alpha_out, double *weights) {
  HMap *m = (HMap *)h;
  const int v = frame_init ? 2 : m->v, thr = frame_init ? 1 : m->thr;
  std::vector<Cand> cand;
  std::vector<double> nb(3 * (size_t)m->K);
  int total = 0;
  for (int k = 0; k < n && total < m->max_res; k++) {
    const double *rp = raw + 3 * (size_t)k, al = ct ? alpha[k] : 0.0;
    double pw[3];
    h_world(ct, pb, pe, al, rp, pw);
    int key[3];
    if (!vmap_axis_key(pw[0], m->size, key) || !vmap_axis_key(pw[1], m->size, key + 1) || !vmap_axis_key(pw[2], m->size, key + 2)) continue;
    cand.clear();
    int visit = 0;
    for (int x = key[0] - v; x <= key[0] + v; x++)
      for (int y = key[1] - v; y <= key[1] + v; y++)
        for (int z = key[2] - v; z <= key[2] + v; z++) {
          if (std::abs(x) > 32767 || std::abs(y) > 32767 || std::abs(z) > 32767) continue;
          auto it = m->vox.find(vmap_pack(x, y, z));
          if (it == m->vox.end() || (int)it->second.size() / 3 < thr) continue;
          for (size_t j = 0; j < it->second.size(); j += 3) cand.push_back({std::sqrt(vmap_sqdist(&it->second[j], pw)), visit++, &it->second[j]});
        }
    const int nk = std::min<int>(m->K, (int)cand.size());
    if (nk < m->min_nn || nk == 0) continue;
    std::partial_sort(cand.begin(), cand.begin() + nk, cand.end(), [](const Cand &a, const Cand &b) { return a.d < b.d || (a.d == b.d && a.visit < b.visit); });
    for (int i = 0; i < nk; i++) for (int a = 0; a < 3; a++) nb[3 * i + a] = cand[i].p[a];
    double bary[3], cov[6], nrm[3];
    vmap_moments(nb.data(), nk, bary, cov);
    const double a2d = vmap_normal_a2d(cov, nrm);
    if (a2d != a2d) continue;
    if (nrm[0] * (pb[0] - rp[0]) + nrm[1] * (pb[1] - rp[1]) + nrm[2] * (pb[2] - rp[2]) < 0) for (int a = 0; a < 3; a++) nrm[a] = -nrm[a];
    const double w = vmap_weight(a2d, cand[0].d, m->w_alpha, m->w_nb, m->power, m->max_plane, m->min_nn);
    const double nn = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
    const double nv[3] = {nrm[0] / nn, nrm[1] / nn, nrm[2] / nn};
    double pt[3] = {rp[0], rp[1], rp[2]};
    if (!ct) {
      const double q2 = pb[3] * pb[3] + pb[4] * pb[4] + pb[5] * pb[5] + pb[6] * pb[6];
      const double qi[4] = {-pb[3] / q2, -pb[4] / q2, -pb[5] / q2, pb[6] / q2};
      double Ri[9];
      h_qrot(qi, Ri);
      for (int a = 0; a < 3; a++)
        pt[a] = (Ri[3 * a] * pw[0] + Ri[3 * a + 1] * pw[1] + Ri[3 * a + 2] * pw[2]) - (Ri[3 * a] * pb[0] + Ri[3 * a + 1] * pb[1] + Ri[3 * a + 2] * pb[2]);
    }
    for (int i = 0; i < m->ncn && i < nk && total < m->max_res; i++) {
      const double *q = &nb[3 * i];
      if (std::fabs((pw[0] - q[0]) * nrm[0] + (pw[1] - q[1]) * nrm[1] + (pw[2] - q[2]) * nrm[2]) >= m->max_plane) continue;
      src[total] = k; offsets[total] = -(nv[0] * q[0] + nv[1] * q[1] + nv[2] * q[2]); alpha_out[total] = al; weights[total] = w;
      for (int a = 0; a < 3; a++) { pts[3 * total + a] = pt[a]; normals[3 * total + a] = nv[a]; }
      total++;
    }
  }
  return total;
}
}
