// tests/ldb_host_shim.cpp — TEST HARNESS ONLY. The host build of ground-fusion2_amd/csrc/gfbe_ldb.h behind a C interface: the
// vocabulary check and plan, the one-thread walk (transform, query with the decision, add, match) that tests/test_ldb_model.py compares
// with the model tests/ldb_np.py and that tools/diag_ldb_bench.py times on one core.
#include <algorithm>
#include <cstring>

#include "../ground-fusion2_amd/csrc/gfbe_ldb.h"

using namespace gfd;

namespace {
struct Shim {
  LdbTree T;
  std::vector<LdbBow> db;
  std::vector<std::vector<uint64_t>> desc;
};
}  // namespace

extern "C" {

int shim_ldb_validate(int k, int L, int scoring, int weighting, int n_nodes, const int32_t *node_id, const int32_t *parent_id, const double *weight, const uint64_t *descriptor,
                      int n_words, const int32_t *word_id, const int32_t *word_node) {
  return ldb_plan_vocab(LdbVocabIn{k, L, scoring, weighting, n_nodes, node_id, parent_id, weight, descriptor, n_words, word_id, word_node}, nullptr);
}
const char *shim_ldb_vocab_error(int code) { return ldb_vocab_error(code); }

void *shim_ldb_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t *node_id, const int32_t *parent_id, const double *weight, const uint64_t *descriptor,
                      int n_words, const int32_t *word_id, const int32_t *word_node) {
  Shim *s = new Shim();
  if (ldb_plan_vocab(LdbVocabIn{k, L, scoring, weighting, n_nodes, node_id, parent_id, weight, descriptor, n_words, word_id, word_node}, &s->T) != LDB_V_OK) { delete s; return nullptr; }
  return s;
}
void shim_ldb_destroy(void *h) { delete (Shim *)h; }

int shim_ldb_hamming(const uint64_t *a, const uint64_t *b) { return ldb_hamming(a, b); }
double shim_ldb_repeated_sum(double w, int c) { return ldb_repeated_sum(w, c); }
int shim_ldb_fits(long long n_kf, long long kcap, long long n_desc, long long dcap, long long n) { return ldb_fits(n_kf, kcap, n_desc, dcap, n) ? 1 : 0; }
// the minimum over `walkers` strided walkers of one step's keys: what the kernel's sub-group computes
int shim_ldb_step(void *h, const uint64_t *f, int node, int walkers) {
  const LdbTree &T = ((Shim *)h)->T;
  int key = LDB_KEY_NONE;
  for (int w = 0; w < walkers; w++) key = std::min(key, ldb_step_key(f, T.desc.data(), T.child.data() + T.child_begin[(size_t)node], T.child_count[(size_t)node], w, walkers));
  return key;
}

int shim_ldb_transform(void *h, int n, const uint64_t *desc, int32_t *word_out, int32_t *bow_word, double *bow_value) {
  LdbBow v;
  ldb_host_transform(((Shim *)h)->T, n, desc, word_out, &v);
  for (size_t a = 0; a < v.word.size(); a++) { bow_word[a] = v.word[a]; bow_value[a] = v.value[a]; }
  return (int)v.word.size();
}

// detectLoop (detect != 0) or addKeyFrameIntoVoc: returns loop_index; o = max_results, query_gap, min_loop_frame; thr = score_first, score_other
int shim_ldb_add(void *h, int n, const uint64_t *desc, int detect, const int *o, const double *thr, int *n_results, int32_t *id, double *score) {
  Shim *s = (Shim *)h;
  LdbBow v;
  ldb_host_transform(s->T, n, desc, nullptr, &v);
  const int frame_index = (int)s->db.size();
  int loop = -1;
  *n_results = 0;
  if (detect) {
    *n_results = ldb_host_query(s->db, v, frame_index - o[1], o[0], id, score);
    loop = ldb_decide(*n_results, id, score, frame_index, thr[0], thr[1], o[2], nullptr);
  }
  s->db.push_back(v);
  s->desc.emplace_back(desc, desc + 4 * (size_t)n);
  return loop;
}

int shim_ldb_match(void *h, int old_index, int n_window, const uint64_t *win, int start, int max_dist, uint8_t *status, int32_t *best_index, int32_t *best_dist, int32_t *matched_src) {
  const std::vector<uint64_t> &old = ((Shim *)h)->desc[(size_t)old_index];
  return ldb_host_match((int)(old.size() / 4), old.data(), n_window, win, start, max_dist, status, best_index, best_dist, matched_src);
}

int shim_ldb_decide(int n, const int32_t *id, const double *score, int frame_index, double first_min, double other_min, int min_frame, int *find_loop) {
  return ldb_decide(n, id, score, frame_index, first_min, other_min, min_frame, find_loop);
}

}  // extern "C"
