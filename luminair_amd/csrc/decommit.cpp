// Decommitment planning (stwo MerkleProver::decommit / FRI witness order): turns the query
// positions into an ordered list of device references that ONE gather launch fetches (k_gather), recomputing the tree
// nodes a fused launch never wrote.
#include "prover_internal.h"

namespace lmn {

// ------------------------------------------------------------------------------------ decommit planning
// A run of device words to fetch.  owner < 0: every rank holds it; otherwise only rank `owner` does (row-block
// sharded column or Merkle layer) and ptr is meaningful on that rank alone.
static Ref col_ref(const ColRef& c, uint64_t row, int g) {
  if (!c.sharded) return {c.ptr + row, 1, -1};
  const int sh = c.log - g;
  return {c.ptr + (row & ((1ull << sh) - 1)), 1, (int)(row >> sh)};
}
static Ref node_ref(const DevMerkle& m, int layer, uint64_t node, std::vector<MerkleRecompute>& jobs) {
  if (!m.layers[layer]) {   // a level its launch kept in registers (MerkleCut)
    const MerkleCut* c = cut_holding(m.cuts, layer);
    if (!c) throw LmnError(LMN_ERR_INTERNAL, "merkle: layer without storage");
    jobs.push_back({c->prev, c->sg, c->ncols, 1u << c->start_log, c->below, c->below_ncols, (uint32_t)node, c->start_log - layer, 0u});
    return {nullptr, 8, -1, (int)jobs.size() - 1};
  }
  if (m.g == 0 || layer <= m.g) return {m.layers[layer] + node * 8, 8, -1};
  const int sh = layer - m.g;
  return {m.layers[layer] + (node & ((1ull << sh) - 1)) * 8, 8, (int)(node >> sh)};
}

void release_host_scratch(void* p) { delete static_cast<HostScratch*>(p); }

// MerkleProver::decommit (openings.h walk_openings): emits device references in output order
void plan_merkle_decommit(const DevMerkle& m, const std::vector<ColRef>& cols_sorted, int g,
                                 const std::map<int, std::vector<uint32_t>>& queries, std::vector<Ref>& queried,
                                 std::vector<Ref>& hash_wit, std::vector<Ref>& col_wit, std::vector<MerkleRecompute>& jobs) {
  if (m.max_log > (int)OPEN_MAX_LOG) throw LmnError(LMN_ERR_INTERNAL, "merkle: a tree larger than the planner takes");
  uint32_t ncols_of_log[OPEN_MAX_LOG + 1] = {};
  Positions queries_of_log[OPEN_MAX_LOG + 1];
  for (const ColRef& c : cols_sorted) ++ncols_of_log[c.log];
  for (auto& q : queries)
    if (q.first >= 0 && q.first <= m.max_log) queries_of_log[q.first] = {q.second.data(), q.second.size()};
  struct Plan {
    const DevMerkle& m;
    const std::vector<ColRef>& cols;
    int g;
    std::vector<Ref> &queried, &hash_wit, &col_wit;
    std::vector<MerkleRecompute>& jobs;
    bool child(int layer, uint32_t child, bool opened) {
      if (!opened) hash_wit.push_back(node_ref(m, layer, child, jobs));
      return true;
    }
    bool column(uint32_t col, uint32_t node, bool is_query) {
      (is_query ? queried : col_wit).push_back(col_ref(cols[col], node, g));
      return true;
    }
    bool node(int, uint32_t) { return true; }
  };
  walk_openings(m.max_log, ncols_of_log, queries_of_log, Plan{m, cols_sorted, g, queried, hash_wit, col_wit, jobs});
}

// compute_decommitment_positions_and_witness_evals with fold_step = 1; `cols` = the 4 coordinate columns
void plan_fri_witness(const ColRef (&cols)[4], int g, const std::vector<uint32_t>& qpos,
                             std::vector<uint32_t>& dec_pos, std::vector<Ref>& wit) {
  // (planning runs between the proof's last two waits: no allocation per pair)
  dec_pos.reserve(dec_pos.size() + 2 * qpos.size());
  for_each_pair_member(qpos, [&](uint32_t pos, bool is_query) {
    dec_pos.push_back(pos);
    if (!is_query)
      for (int k = 0; k < 4; ++k) wit.push_back(col_ref(cols[k], pos, g));
    return true;
  });
}

}  // namespace lmn
