// tests/ldb_host_main.cpp — TEST HARNESS ONLY. A stand-alone program around the host functions of gfbe_ldb.h for a sanitizer run
// (-fsanitize=address,undefined): the vocabulary check on arrays of exactly the stated sizes (a sound tree, and one broken rule at a
// time), the descent, the BoW vector, the query, the decision and the match on vectors sized to the element. Prints "ok".
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../ground-fusion2_amd/csrc/gfbe_ldb.h"

using namespace gfd;

namespace {
struct Voc {
  std::vector<int32_t> id, parent, word_id, word_node;
  std::vector<double> weight;
  std::vector<uint64_t> desc;
  LdbVocabIn in(int scoring = 0, int weighting = 0) const {
    return LdbVocabIn{3, 3, scoring, weighting, (int)id.size(), id.data(), parent.data(), weight.data(), desc.data(), (int)word_id.size(), word_id.data(), word_node.data()};
  }
};
uint64_t mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; return x ^ (x >> 33); }
// an unbalanced tree: node 1 a leaf at level 1, 2 and 3 with children, node 4 with one child
Voc sound() {
  Voc v;
  const int parents[] = {0, 0, 0, 2, 2, 3, 3, 3, 4};
  for (int i = 0; i < 9; i++) {
    v.id.push_back(i + 1); v.parent.push_back(parents[i]); v.weight.push_back(0.25 + 0.1 * i);
    for (int w = 0; w < 4; w++) v.desc.push_back(mix((uint64_t)(17 * i + w + 1)));
  }
  const int leaves[] = {1, 5, 6, 7, 8, 9};
  for (int w = 0; w < 6; w++) { v.word_id.push_back(w); v.word_node.push_back(leaves[w]); }
  return v;
}
}  // namespace

int main() {
  int bad = 0;
  const Voc ok = sound();
  LdbTree T;
  if (ldb_plan_vocab(ok.in(), &T) != LDB_V_OK) bad++;
  if (ldb_plan_vocab(ok.in(1, 0), nullptr) != LDB_V_MODE || ldb_plan_vocab(ok.in(0, 2), nullptr) != LDB_V_MODE || ldb_plan_vocab(ok.in(0, 1), nullptr) != LDB_V_OK) bad++;
  { Voc v = ok; v.id[4] = 4; if (ldb_plan_vocab(v.in(), nullptr) != LDB_V_NODE_ID) bad++; }
  { Voc v = ok; v.id[4] = 10; if (ldb_plan_vocab(v.in(), nullptr) != LDB_V_NODE_ID) bad++; }
  { Voc v = ok; v.parent[3] = 9; if (ldb_plan_vocab(v.in(), nullptr) != LDB_V_PARENT) bad++; }
  { Voc v = ok; v.weight[2] = -1.0; if (ldb_plan_vocab(v.in(), nullptr) != LDB_V_WEIGHT) bad++; }
  { Voc v = ok; v.weight[2] = NAN; if (ldb_plan_vocab(v.in(), nullptr) != LDB_V_WEIGHT) bad++; }
  { Voc v = ok; v.word_node[1] = 2; if (ldb_plan_vocab(v.in(), nullptr) != LDB_V_WORD) bad++; }
  { Voc v = ok; v.word_id[1] = 0; if (ldb_plan_vocab(v.in(), nullptr) != LDB_V_WORD) bad++; }
  { Voc v = ok; v.word_id.pop_back(); v.word_node.pop_back(); if (ldb_plan_vocab(v.in(), nullptr) != LDB_V_LEAF) bad++; }
  {      // a chain of 17 levels, and a root with 257 children
    Voc v;
    for (int i = 0; i < 17; i++) { v.id.push_back(i + 1); v.parent.push_back(i); v.weight.push_back(1.0); for (int w = 0; w < 4; w++) v.desc.push_back(mix((uint64_t)i)); }
    v.word_id.push_back(0); v.word_node.push_back(17);
    if (ldb_plan_vocab(v.in(), nullptr) != LDB_V_DEPTH) bad++;
    Voc w;
    for (int i = 0; i < 257; i++) { w.id.push_back(i + 1); w.parent.push_back(0); w.weight.push_back(1.0); for (int a = 0; a < 4; a++) w.desc.push_back(mix((uint64_t)i)); w.word_id.push_back(i); w.word_node.push_back(i + 1); }
    if (ldb_plan_vocab(w.in(), nullptr) != LDB_V_CHILDREN) bad++;
  }
  // keyframes of exactly n descriptors: each near a leaf; the database, the query, the decision
  std::vector<LdbBow> db;
  std::vector<std::vector<uint64_t>> held;
  for (int kf = 0; kf < 60; kf++) {
    const int n = kf == 3 ? 0 : 1 + (kf * 7) % 23;
    std::vector<uint64_t> d(4 * (size_t)n);
    for (int i = 0; i < n; i++)
      for (int w = 0; w < 4; w++) d[4 * (size_t)i + (size_t)w] = ok.desc[4 * (size_t)((kf + 3 * i) % 9) + (size_t)w] ^ (1ull << ((kf + i) % 64));
    std::vector<int> word((size_t)n);
    LdbBow v;
    ldb_host_transform(T, n, d.data(), word.data(), &v);
    for (int w : word) if (w < 0 || w >= 6) bad++;
    double sum = 0.0;
    for (double x : v.value) sum += x;
    if (n > 0 && !(sum > 0.999999 && sum < 1.000001)) bad++;
    for (int walkers : {1, 16}) {      // a step's key does not depend on how the children are shared out
      if (n == 0) break;
      int key = LDB_KEY_NONE;
      for (int w = 0; w < walkers; w++) key = std::min(key, ldb_step_key(d.data(), T.desc.data(), T.child.data() + T.child_begin[0], T.child_count[0], w, walkers));
      if (key != ldb_step_key(d.data(), T.desc.data(), T.child.data() + T.child_begin[0], T.child_count[0], 0, 1)) bad++;
    }
    std::vector<int> id(4);
    std::vector<double> score(4);
    const int nr = ldb_host_query(db, v, kf - 50, 4, id.data(), score.data());
    int found = 0;
    const int loop = ldb_decide(nr, id.data(), score.data(), kf, 0.05, 0.015, 50, &found);
    if (nr < 0 || nr > 4 || loop >= kf || (kf <= 50 && loop != -1)) bad++;
    for (int a = 1; a < nr; a++) if (score[(size_t)a] > score[(size_t)a - 1]) bad++;
    db.push_back(v);
    held.push_back(d);
  }
  // the match of every keyframe's descriptors against an earlier one, outputs sized to the element
  for (int kf = 1; kf < 60; kf += 7) {
    const std::vector<uint64_t> &win = held[(size_t)kf], &old = held[(size_t)kf - 1];
    const int nw = (int)win.size() / 4, no = (int)old.size() / 4;
    std::vector<uint8_t> status((size_t)nw);
    std::vector<int> bi((size_t)nw), bd((size_t)nw), src((size_t)nw);
    const int m = ldb_host_match(no, old.data(), nw, win.data(), 128, 80, status.data(), bi.data(), bd.data(), src.data());
    if (m < 0 || m > nw) bad++;
    for (int i = 0; i < nw; i++) if (bi[(size_t)i] >= no || (bi[(size_t)i] < 0) != (bd[(size_t)i] == 128)) bad++;
  }
  if (ldb_match_status(ldb_match_none(128), 80) || !ldb_match_status(ldb_match_key(79, 5), 80) || ldb_match_status(ldb_match_key(80, 5), 80)) bad++;
  if (!ldb_fits(2, 3, 90, 100, 10) || ldb_fits(3, 3, 0, 100, 1) || ldb_fits(0, 3, 91, 100, 10)) bad++;
  std::printf(bad ? "bad %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
