// Which nodes of a Merkle tree a set of queries opens, and which positions a FRI layer opens: stwo's
// MerkleProver::decommit / MerkleVerifier::verify, fold_positions, the pair expansion and Queries::generate (SURVEY.md
// Appendix A.4 / A.8; oracle/merkle.py, oracle/prover.py).  The host's ONE statement of each: the prover's plan
// (decommit.cpp), lmn_tree_decommit's (level2.cpp) and the verifier (verifier.cpp) are visitors of walk_openings.
// Host only: nothing of the device runtime is included, and every visitor inlines.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <set>
#include <vector>

namespace lmn {

// sorted, distinct positions (one log size's queries)
struct Positions {
  const uint32_t* p = nullptr;
  size_t n = 0;
};

// The opening walk.  Layer by layer from `max_log` up to the root, the nodes to open are the parents of the nodes opened
// in the layer below merged with the layer's own queries.  ncols_of_log and queries_of_log are indexed by log size,
// 0 .. max_log; a tree's columns stand in tree order (size descending), so a layer's columns are a run of indices.
// For every opened node, ascending within its layer, the visitor sees in this order
//   v.child(layer, child, opened)   below the deepest layer, for both children: `opened` if the walk opened the child
//                                   in `layer` (= the node's layer + 1), otherwise its hash comes from the hash witness
//   v.column(col, node, queried)    for each column of the node's layer, by index in tree order: its value at `node` is a
//                                   queried value if the node is a query, otherwise column witness
//   v.node(layer, node)             the node is complete
// Each returns whether to go on; the walk returns false where a visitor stopped it.  Its two node lists are reserved
// once: nothing is allocated per node (the prover plans between a proof's last two waits).
template <class V>
bool walk_openings(int max_log, const uint32_t* ncols_of_log, const Positions* queries_of_log, V&& v) {
  std::vector<uint32_t> prev, cur;
  prev.reserve(16);
  cur.reserve(16);
  uint32_t first_col = 0;
  for (int log = max_log; log >= 0; --log) {
    const uint32_t ncols = ncols_of_log[log];
    const Positions q = queries_of_log[log];
    size_t pi = 0, qi = 0;
    cur.clear();
    while (pi < prev.size() || qi < q.n) {
      uint32_t node;
      if (pi < prev.size() && qi < q.n)
        node = std::min(prev[pi] / 2, q.p[qi]);
      else
        node = pi < prev.size() ? prev[pi] / 2 : q.p[qi];
      if (log < max_log)
        for (uint32_t child = 2 * node; child <= 2 * node + 1; ++child) {
          const bool opened = pi < prev.size() && prev[pi] == child;
          if (opened) ++pi;
          if (!v.child(log + 1, child, opened)) return false;
        }
      const bool queried = qi < q.n && q.p[qi] == node;
      if (queried) ++qi;
      for (uint32_t c = 0; c < ncols; ++c)
        if (!v.column(first_col + c, node, queried)) return false;
      if (!v.node(log, node)) return false;
      cur.push_back(node);
    }
    first_col += ncols;
    prev.swap(cur);
  }
  return true;
}

// sorted positions folded to a domain 2^n times smaller: sorted and distinct again
inline std::vector<uint32_t> fold_positions(const std::vector<uint32_t>& p, int n) {
  std::vector<uint32_t> out;
  out.reserve(p.size());
  for (uint32_t v : p) {
    const uint32_t q = v >> n;
    if (out.empty() || out.back() != q) out.push_back(q);
  }
  return out;
}

// The sibling pairs a FRI layer opens at sorted, distinct positions (compute_decommitment_positions_and_witness_evals with
// fold_step = 1): every pair (2k, 2k + 1) that holds a position, ascending.  f(pos, is_query) sees both members of each
// pair in turn; one that is no query comes from the FRI witness.  f returns whether to go on.
template <class F>
bool for_each_pair_member(const std::vector<uint32_t>& qpos, F&& f) {
  for (size_t i = 0; i < qpos.size();) {
    const uint32_t even = qpos[i] & ~1u;
    bool is_query[2] = {false, false};
    while (i < qpos.size() && (qpos[i] & ~1u) == even) is_query[qpos[i++] & 1u] = true;
    if (!f(even, is_query[0]) || !f(even + 1, is_query[1])) return false;
  }
  return true;
}

// Queries::generate: n_queries positions, 8 per draw_random_words, masked to log_domain bits; ascending and distinct
template <class Ch>
std::vector<uint32_t> draw_query_positions(Ch& channel, uint64_t n_queries, uint32_t log_domain) {
  std::set<uint32_t> qs;
  const uint32_t mask = (uint32_t)((1ull << log_domain) - 1u);
  for (uint64_t cnt = 0; cnt < n_queries;) {
    const auto r = channel.draw_random_words();
    for (int i = 0; i < 8 && cnt < n_queries; ++i, ++cnt) qs.insert(r.w[i] & mask);
  }
  return std::vector<uint32_t>(qs.begin(), qs.end());
}

}  // namespace lmn
