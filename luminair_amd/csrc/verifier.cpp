// verify(proof, settings): host-side replacement for
// /root/reference/crates/verifiers/rust/src/verifier.rs:21-143 (replay the three commitments, check
// the logup sum `crates/air/src/utils.rs:29-57`, then stwo::core::verifier::verify) — SURVEY.md §8f-2.
// Pure host code (the reference verifier is CPU code too); no GPU work, no oracle dependency.
#include <algorithm>
#include <set>

#include "capi_internal.h"
#include "openings.h"

namespace lmn {

namespace {

constexpr int ERR_VERIFY = LMN_ERR_VERIFICATION;
[[noreturn]] void fail(const std::string& what) { throw LmnError(ERR_VERIFY, "StwoVerifierError: " + what); }

// ---- bincode reader
struct Reader {
  const uint8_t* p;
  size_t n, o = 0;
  void need(size_t k) {
    if (o + k > n) throw LmnError(LMN_ERR_SERIALIZATION, "SerializationError: truncated proof");
  }
  uint8_t u8() {
    need(1);
    return p[o++];
  }
  uint32_t u32() {
    need(4);
    uint32_t v = (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8) | ((uint32_t)p[o + 2] << 16) | ((uint32_t)p[o + 3] << 24);
    o += 4;
    return v;
  }
  uint64_t u64() {
    uint64_t lo = u32(), hi = u32();
    return lo | (hi << 32);
  }
  size_t len(size_t elem_bytes) {
    uint64_t l = u64();
    if (elem_bytes && l > (n - o) / elem_bytes + 1) throw LmnError(LMN_ERR_SERIALIZATION, "SerializationError: bad length");
    return (size_t)l;
  }
  // A field element on the wire is a canonical M31 word: anything >= P would make the 64-bit lazy arithmetic
  // below compute outside the field and give equal values several accepted encodings.
  uint32_t m31() {
    uint32_t v = u32();
    if (v >= P31) throw LmnError(LMN_ERR_SERIALIZATION, "SerializationError: field word is not a canonical M31");
    return v;
  }
  bool option_tag() {
    uint8_t t = u8();
    if (t > 1) throw LmnError(LMN_ERR_SERIALIZATION, "SerializationError: bad Option tag");
    return t == 1;
  }
  QM31 q() {
    QM31 v;
    v.a = m31();
    v.b = m31();
    v.c = m31();
    v.d = m31();
    return v;
  }
  Hash32 hash() {
    Hash32 h;
    for (int i = 0; i < 8; ++i) h.w[i] = u32();
    return h;
  }
  Decommitment decommit() {
    Decommitment d;
    size_t nh = len(32);
    for (size_t i = 0; i < nh; ++i) d.hash_witness.push_back(hash());
    size_t nc = len(4);
    for (size_t i = 0; i < nc; ++i) d.column_witness.push_back(m31());
    return d;
  }
  FriLayerProof layer() {
    FriLayerProof l;
    size_t nw = len(16);
    for (size_t i = 0; i < nw; ++i) l.fri_witness.push_back(q());
    l.decommitment = decommit();
    l.commitment = hash();
    return l;
  }
};

Proof parse_proof(const uint8_t* data, size_t n, int n_slots) {
  Reader r{data, n};
  Proof p;
  for (int i = 0; i < n_slots; ++i) {
    if (!r.option_tag()) {
      p.claim.push_back(-1);
      continue;
    }
    uint32_t ls = r.u32();
    if (ls > 26) throw LmnError(LMN_ERR_SERIALIZATION, "SerializationError: claim log_size out of range");
    p.claim.push_back((int)ls);
  }
  for (int i = 0; i < n_slots; ++i) {
    bool some = r.option_tag();
    p.interaction_claim.push_back({some, some ? r.q() : q_zero()});
  }
  p.pow_bits = r.u32();
  p.log_blowup = r.u32();
  p.log_last_layer = r.u32();
  p.n_queries = r.u64();
  size_t nc = r.len(32);
  for (size_t i = 0; i < nc; ++i) p.commitments.push_back(r.hash());
  size_t nt = r.len(8);
  for (size_t t = 0; t < nt; ++t) {
    std::vector<std::vector<QM31>> tree;
    size_t ncol = r.len(8);
    for (size_t c = 0; c < ncol; ++c) {
      std::vector<QM31> col;
      size_t np = r.len(16);
      for (size_t k = 0; k < np; ++k) col.push_back(r.q());
      tree.push_back(col);
    }
    p.sampled_values.push_back(tree);
  }
  size_t nd = r.len(16);
  for (size_t i = 0; i < nd; ++i) p.decommitments.push_back(r.decommit());
  size_t nq = r.len(8);
  for (size_t t = 0; t < nq; ++t) {
    std::vector<uint32_t> v;
    size_t k = r.len(4);
    for (size_t i = 0; i < k; ++i) v.push_back(r.m31());
    p.queried_values.push_back(v);
  }
  p.proof_of_work = r.u64();
  p.first_layer = r.layer();
  size_t ni = r.len(40);
  for (size_t i = 0; i < ni; ++i) p.inner_layers.push_back(r.layer());
  size_t nl = r.len(16);
  for (size_t i = 0; i < nl; ++i) p.last_layer_coeffs.push_back(r.q());
  p.last_layer_log_size = r.u32();
  if (r.o != n) throw LmnError(LMN_ERR_SERIALIZATION, "SerializationError: trailing bytes");
  return p;
}

// ---- MerkleVerifier::verify (openings.h walk_openings): every opened node's hash from its children's and its column
// values, pulled from the proof's lists in the walk's order; a list that runs out stops the walk
struct MerkleReplay {
  const std::vector<uint32_t>& queried;
  const Decommitment& d;
  size_t qi = 0, hi = 0, ci = 0;
  std::vector<Hash32> nodes;   // the opened nodes' hashes in the walk's order; a layer opens ALL nodes of the layer below as
  size_t taken = 0;            // children, in that order: nodes[taken] is the next opened child
  std::vector<uint32_t> words;
  bool child(int, uint32_t, bool opened) {
    if (!opened && hi >= d.hash_witness.size()) return false;
    const Hash32& h = opened ? nodes[taken++] : d.hash_witness[hi++];
    words.insert(words.end(), h.w, h.w + 8);
    return true;
  }
  bool column(uint32_t, uint32_t, bool is_query) {
    const std::vector<uint32_t>& from = is_query ? queried : d.column_witness;
    size_t& at = is_query ? qi : ci;
    if (at >= from.size()) return false;
    words.push_back(from[at++]);
    return true;
  }
  bool node(int, uint32_t) {
    nodes.push_back(b2_hash_words(words.data(), words.size()));
    words.clear();
    return true;
  }
};
bool merkle_verify(const Hash32& root, const std::vector<int>& col_logs, const std::map<int, std::vector<uint32_t>>& queries,
                   const std::vector<uint32_t>& queried, const Decommitment& d) {
  if (col_logs.empty()) {
    Hash32 e = b2_hash_words(nullptr, 0);
    return memcmp(e.w, root.w, 32) == 0 && queried.empty() && d.hash_witness.empty() && d.column_witness.empty();
  }
  const int max_log = *std::max_element(col_logs.begin(), col_logs.end());
  std::vector<uint32_t> ncols_of_log(max_log + 1, 0u);
  for (int l : col_logs) ncols_of_log[l]++;
  std::vector<Positions> queries_of_log(max_log + 1);
  for (auto& q : queries)
    if (q.first >= 0 && q.first <= max_log) queries_of_log[q.first] = {q.second.data(), q.second.size()};
  MerkleReplay v{queried, d};
  if (!walk_openings(max_log, ncols_of_log.data(), queries_of_log.data(), v)) return false;
  if (v.qi != queried.size() || v.hi != d.hash_witness.size() || v.ci != d.column_witness.size()) return false;
  // (all but the root were taken as children: exactly one node is left, and only where the walk opened any)
  return v.taken + 1 == v.nodes.size() && memcmp(v.nodes.back().w, root.w, 32) == 0;
}

// sibling pairs of a sparse evaluation: queried values come from `known`, the rest from the witness
bool rebuild_pairs(const std::vector<uint32_t>& qpos, const std::map<uint32_t, QM31>& known,
                   const std::vector<QM31>& witness, size_t& wi, std::vector<uint32_t>& dec_pos,
                   std::map<uint32_t, QM31>& vals) {
  return for_each_pair_member(qpos, [&](uint32_t pos, bool is_query) {
    dec_pos.push_back(pos);
    if (is_query) {
      auto it = known.find(pos);
      if (it == known.end()) return false;
      vals[pos] = it->second;
    } else {
      if (wi >= witness.size()) return false;
      vals[pos] = witness[wi++];
    }
    return true;
  });
}

// Where the verdicts of one pass over a proof go.
//   rep == nullptr: lmn_verify (the first failed check throws).  Otherwise lmn_verify_diagnose: a failed check is
//   recorded and the replay goes on as far as the proof's shape allows, so that one pass tells WHICH part of the
//   protocol disagrees (tools/pin_variant.py): the checks depend on different parts of the transcript and of the AIR.
//   stopped (lmn_verify_many, rep == nullptr): receives the LMN_CHECK_* bit of the check that throws.
struct Checks {
  lmn_verify_report* rep = nullptr;
  uint32_t* stopped = nullptr;
  // check(bit, ok, what): lmn_verify semantics without a report; with one, record and continue
  void check(uint32_t bit, bool ok, const std::string& what, int code = LMN_ERR_VERIFICATION) const {
    if (rep) {
      rep->checks_run |= bit;
      if (ok) {
        if (!(rep->checks_failed & bit)) rep->checks_passed |= bit;
      } else {
        rep->checks_passed &= ~bit;
        rep->checks_failed |= bit;
        if (!rep->first_failure[0]) snprintf(rep->first_failure, sizeof rep->first_failure, "%s", what.c_str());
      }
      return;
    }
    if (!ok) {
      if (stopped) *stopped |= bit;
      if (code == LMN_ERR_INVALID_LOGUP) throw LmnError(LMN_ERR_INVALID_LOGUP, what);
      ::lmn::fail(what);
    }
  }
  // a structural stop (the replay cannot go on): in diagnose mode it is recorded as a failed LMN_CHECK_SHAPE before the
  // throw, so that a plain config or shape mismatch is not read as a transcript-encoding disagreement (pinning.py)
  [[noreturn]] void fail(const std::string& what) const {
    if (rep) {
      rep->checks_run |= LMN_CHECK_SHAPE;
      rep->checks_passed &= ~LMN_CHECK_SHAPE;
      rep->checks_failed |= LMN_CHECK_SHAPE;
      if (!rep->first_failure[0]) snprintf(rep->first_failure, sizeof rep->first_failure, "%s", what.c_str());
    }
    if (stopped) *stopped |= LMN_CHECK_SHAPE;
    ::lmn::fail(what);
  }
  void step(uint32_t id, uint32_t index, const Channel& ch) const {
    if (!rep || rep->n_steps >= LMN_MAX_TRANSCRIPT_STEPS) return;
    lmn_transcript_step& st = rep->steps[rep->n_steps++];
    st.step = id;
    st.index = index;
    memcpy(st.digest, ch.digest().w, 32);
  }
};

void require_expected_config(const lmn_config& expect) {
  if (expect.protocol_variant & ~LMN_PV_ALL) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "bad protocol_variant (unknown LMN_PV_* bits)");
  if (expect.log_blowup < 1 || expect.log_blowup > 3 /* what the prover accepts (context.cpp); oracle/verifier.py alike */ || expect.n_queries == 0 || expect.n_queries > 1024 || expect.log_last_layer > 10 ||
      expect.pow_bits > 40)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "bad expected PCS config");
}

// What the front half of the verifier leaves for the back half: the proof, the layout its claim implies and everything
// drawn from the transcript up to the query positions.
struct VerifyFront {
  Proof p;
  int lb = 0, top = 0;
  std::vector<std::vector<int>> tree_logs;             // column log sizes of the four trace trees, tree order
  std::vector<std::vector<std::vector<QPt>>> pts;      // sample points per tree and column
  std::vector<int> sizes;                              // the LDE log sizes, descending
  QM31 quot_alpha{};
  std::vector<QM31> alphas;                            // the fold alphas: first layer, then the inner layers
  std::vector<uint32_t> queries;                       // ascending, distinct, in the domain of 2^top
  std::map<int, std::vector<uint32_t>> pos_by_log;     // the queries folded to every size
};

// The front: parse, config and shape checks, the settings cross-check, the logup sum, the transcript replay, the OODS
// identity, the last layer's shape, the proof of work, the query draw and the folded positions per size.
VerifyFront verify_front(const uint8_t* data, size_t len, const lmn_config& expect, const lmn_settings* settings,
                         const Checks& ck) {
  lmn_verify_report* const rep = ck.rep;
  auto check = [&](uint32_t bit, bool ok, const std::string& what, int code = LMN_ERR_VERIFICATION) { ck.check(bit, ok, what, code); };
  auto fail = [&](const std::string& what) { ck.fail(what); };
  auto step = [&](uint32_t id, uint32_t index, const Channel& ch) { ck.step(id, index, ch); };
  const uint32_t variant = expect.protocol_variant;
  require_expected_config(expect);
  const int n_slots = claim_slots(variant);
  if (rep) rep->checks_run |= LMN_CHECK_PARSE;
  VerifyFront f;
  Proof& p = f.p;
  try {
    p = parse_proof(data, len, n_slots);
  } catch (...) {
    if (ck.stopped) *ck.stopped |= LMN_CHECK_PARSE;
    throw;
  }
  if (rep) rep->checks_passed |= LMN_CHECK_PARSE;
  // The security parameters are the VERIFIER's (the reference builds PcsConfig::default() itself,
  // crates/verifiers/rust/src/verifier.rs:36, and never reads them from the proof): a proof that announces other
  // ones - fewer queries, no proof of work - is rejected, whatever else it contains.
  if (p.pow_bits != expect.pow_bits || p.log_blowup != expect.log_blowup || p.log_last_layer != expect.log_last_layer ||
      p.n_queries != expect.n_queries)
    fail("proof was made for a different PCS config than the verifier's");
  if (rep) rep->checks_run |= LMN_CHECK_SHAPE;
  if (p.last_layer_log_size != p.log_last_layer) fail("last layer degree bound");
  const int lb = f.lb = (int)p.log_blowup;
  if (p.commitments.size() != 4 || p.sampled_values.size() != 4 || p.decommitments.size() != 4 ||
      p.queried_values.size() != 4)
    fail("expected 4 commitment trees");

  // components in struct order; tree layouts implied by the claim (Claim::log_sizes, components/mod.rs:164-170)
  std::vector<Instance> inst;
  int m_off = 0, i_off = 0;
  for (int kind = 0; kind < n_slots; ++kind) {
    if (p.claim[kind] < 0) continue;
    const ComponentSpec* sp = component_spec(kind);
    if (!sp) fail("claim names a component outside the backend's scope");
    if (p.claim[kind] < 4 || p.claim[kind] > 26) fail("bad log_size");
    if (!p.interaction_claim[kind].first) fail("missing interaction claim");
    Instance ci{};
    ci.spec = sp;
    ci.log_size = p.claim[kind];
    ci.main_start = m_off;
    ci.inter_start = i_off;
    ci.claimed = p.interaction_claim[kind].second;
    m_off += sp->n_cols;
    i_off += 4 * sp->n_rel;
    inst.push_back(ci);
  }
  if (inst.empty()) fail("empty claim");
  for (int kind = 0; kind < n_slots; ++kind)
    if (p.claim[kind] < 0 && p.interaction_claim[kind].first) fail("interaction claim without claim");
  std::vector<std::vector<int>>& tree_logs = f.tree_logs;
  tree_logs.assign(4, {});
  tree_logs[0] = assign_preprocessed(inst);
  if (settings) {
    // verifier.rs:47-57 derives the preprocessed column sizes from `settings.lookups`; here they follow from the
    // claim (a LUT column has its lookup component's size), so the settings must describe the same layout
    uint32_t present = 0;
    for (const LookupKind& lk : kLookupKinds)
      if (lk.kind < n_slots && p.claim[lk.kind] >= 0) present |= lk.bit;
    // The sin / exp2 / log2 LUTs are named by the settings and must match exactly; the 8-bit range-check LUT is
    // generated by the library whenever LessThan is present, so settings may or may not announce it (the
    // pre-expanded `lookups` form does not) - it only must not be announced when the claim lacks it.
    const uint32_t lut_bits = LMN_LOOKUP_SIN | LMN_LOOKUP_EXP2 | LMN_LOOKUP_LOG2;
    if (settings->has_lookups & ~present) fail("settings announce a lookup the proof's claim lacks");
    if (settings->has_lookups && (settings->has_lookups & lut_bits) != (present & lut_bits))
      fail("settings.lookups do not match the proof's claim");
    require_luts_pointer(*settings);
    for (uint32_t i = 0; i < settings->n_luts; ++i) {
      const lmn_lut& l = settings->luts[i];
      if (l.kind > LMN_LUT_LOG2) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "bad LUT kind in settings");
      const int kind = kLookupKinds[l.kind].kind;
      if (kind >= n_slots || p.claim[kind] != (int)l.log_size) fail("settings LUT size does not match the proof's claim");
    }
  }
  int max_log = 0;
  for (auto& ci : inst) {
    for (int c = 0; c < ci.spec->n_cols; ++c) tree_logs[1].push_back(ci.log_size);
    for (int c = 0; c < 4 * ci.spec->n_rel; ++c) tree_logs[2].push_back(ci.log_size);
    max_log = std::max(max_log, ci.log_size);
  }
  for (int k = 0; k < 4; ++k) tree_logs[3].push_back(max_log + 1);

  // ---- transcript replay (verifier.rs:61-106)
  Channel ch(variant);
  ch.mix_root(p.commitments[0]);
  step(LMN_STEP_ROOT_PREPROCESSED, 0, ch);
  for (int kind = 0; kind < n_slots; ++kind)
    if (p.claim[kind] >= 0) ch.mix_u64((uint64_t)p.claim[kind]);
  step(LMN_STEP_CLAIM, 0, ch);
  ch.mix_root(p.commitments[1]);
  step(LMN_STEP_ROOT_MAIN, 0, ch);
  const RelElems elems = draw_relation_elements(ch, variant);
  for (auto& ci : inst)
    for (int j = 0; j < ci.spec->n_rel; ++j)
      if (!elems.drawn[ci.spec->rel_elems[j]]) fail("component needs relation elements this protocol variant does not draw");
  QM31 tot = q_zero();
  for (auto& ci : inst) tot = q_add(tot, ci.claimed);
  check(LMN_CHECK_LOGUP_SUM, q_is_zero(tot), "InvalidLogUp", LMN_ERR_INVALID_LOGUP);   // log_sum_valid, verifier.rs:97-99
  for (auto& ci : inst) ch.mix_felts({ci.claimed});
  step(LMN_STEP_INTERACTION_CLAIM, 0, ch);
  ch.mix_root(p.commitments[2]);
  step(LMN_STEP_ROOT_INTERACTION, 0, ch);
  const QM31 comp_alpha = ch.draw_felt();
  ch.mix_root(p.commitments[3]);
  step(LMN_STEP_ROOT_COMPOSITION, 0, ch);
  QM31 tt = ch.draw_felt();
  QM31 t2 = q_sqr(tt);
  QM31 tinv = q_inv(q_add_m(t2, 1u));
  QPt oods{q_mul(q_sub(q_one(), t2), tinv), q_mul(q_add(tt, tt), tinv)};

  // ---- sample points per column
  std::vector<std::vector<std::vector<QPt>>>& pts = f.pts;
  pts.assign(4, {});
  for (size_t c = 0; c < tree_logs[0].size(); ++c) pts[0].push_back({oods});
  for (size_t c = 0; c < tree_logs[1].size(); ++c) pts[1].push_back({oods});
  for (auto& ci : inst) {
    Pt stp = pt_of_index((0x80000000u - subgroup_gen_index(ci.log_size)) & 0x7fffffffu);
    QPt prev = qpt_add_m(oods, stp);
    int ni = 4 * ci.spec->n_rel;
    for (int c = 0; c < ni; ++c) {
      if (c >= ni - 4)
        pts[2].push_back({prev, oods});
      else
        pts[2].push_back({oods});
    }
  }
  for (int k = 0; k < 4; ++k) pts[3].push_back({oods});
  for (int t = 0; t < 4; ++t) {
    if (p.sampled_values[t].size() != pts[t].size()) fail("sampled values shape");
    for (size_t c = 0; c < pts[t].size(); ++c)
      if (p.sampled_values[t][c].size() != pts[t][c].size()) fail("sampled values shape");
  }
  // ---- OODS composition identity
  {
    auto& s3 = p.sampled_values[3];
    QM31 lhs = q_from_partial_evals(s3[0][0], s3[1][0], s3[2][0], s3[3][0]);
    QM31 rhs = eval_composition_at_point(inst, p.sampled_values, oods, elems, comp_alpha, variant);
    check(LMN_CHECK_OODS, q_eq(lhs, rhs), "OodsNotMatching");
  }
  {
    std::vector<QM31> flat;
    for (auto& t : p.sampled_values)
      for (auto& c : t)
        for (auto& v : c) flat.push_back(v);
    ch.mix_felts(flat);
    step(LMN_STEP_SAMPLED_VALUES, 0, ch);
  }
  f.quot_alpha = ch.draw_felt();

  // ---- FRI commit phase replay
  std::set<int, std::greater<int>> size_set;
  for (auto& t : tree_logs)
    for (int l : t) size_set.insert(l + lb);
  std::vector<int>& sizes = f.sizes;
  sizes.assign(size_set.begin(), size_set.end());
  const int top = f.top = sizes[0];
  ch.mix_root(p.first_layer.commitment);
  step(LMN_STEP_FRI_FIRST_LAYER, 0, ch);
  std::vector<QM31>& alphas = f.alphas;
  alphas.assign(1, ch.draw_felt());
  for (auto& l : p.inner_layers) {
    ch.mix_root(l.commitment);
    step(LMN_STEP_FRI_INNER_LAYER, (uint32_t)alphas.size() - 1u, ch);
    alphas.push_back(ch.draw_felt());
  }
  if ((int)p.inner_layers.size() != top - 1 - ((int)p.log_last_layer + lb)) fail("inner layer count");
  if (p.last_layer_coeffs.size() != (size_t)1 << p.log_last_layer) fail("last layer degree");
  ch.mix_felts(p.last_layer_coeffs);
  step(LMN_STEP_FRI_LAST_LAYER, 0, ch);
  if (rep && !(rep->checks_failed & LMN_CHECK_SHAPE)) rep->checks_passed |= LMN_CHECK_SHAPE;   // every shape the transcript depends on was as the claim implies
  check(LMN_CHECK_POW, ch.verify_pow_nonce(p.pow_bits, p.proof_of_work), "ProofOfWork");
  ch.mix_u64(p.proof_of_work);
  step(LMN_STEP_POW_NONCE, 0, ch);
  std::vector<uint32_t>& queries = f.queries;
  queries = draw_query_positions(ch, p.n_queries, (uint32_t)top);
  for (int ls : sizes) f.pos_by_log[ls] = fold_positions(queries, top - ls);
  return f;
}
// ---- FRI answers: which sampled columns make up the quotient of each LDE size (shared by the host's back half and by
// lmn_verify_many's stager, whose layout table is this plan in words)
struct QuotCol {
  int tree, size;    // the tree, and the index of the column's LDE size in VerifyFront::sizes
  size_t base;       // offset of this size-group inside queried_values[tree]
  int ncol, j;       // columns of that size in the tree, index of this column among them
  QM31 value;        // the sampled value
};
struct QuotBatch {
  int pt;            // indexes QuotPlan::pts
  std::vector<QuotCol> cols;
};
struct QuotPlan {
  std::vector<QPt> pts;
  std::vector<std::vector<QuotBatch>> by_size;   // per LDE size: the batches by point, first-appearance order
};
QuotPlan plan_quotients(const VerifyFront& f) {
  const Proof& p = f.p;
  const int lb = f.lb;
  struct ColRef {
    int tree, lde_log;
    size_t base;
    int ncol, j;
    std::vector<std::pair<int, QM31>> samples;  // (point id, value); point id indexes `pts`
  };
  QuotPlan plan;
  auto pt_id = [&](const QPt& q) {
    for (size_t i = 0; i < plan.pts.size(); ++i)
      if (q_eq(plan.pts[i].x, q.x) && q_eq(plan.pts[i].y, q.y)) return (int)i;
    plan.pts.push_back(q);
    return (int)plan.pts.size() - 1;
  };
  std::vector<ColRef> cols;
  for (int t = 0; t < 4; ++t) {
    std::map<int, std::pair<size_t, int>, std::greater<int>> group;  // lde log -> (base, ncol)
    for (int l : f.tree_logs[t]) group[l + lb].second++;
    size_t off = 0;
    for (auto& g : group) {
      g.second.first = off;
      off += (size_t)g.second.second * f.pos_by_log.at(g.first).size();
    }
    std::map<int, int> seen;
    for (size_t c = 0; c < f.tree_logs[t].size(); ++c) {
      int ls = f.tree_logs[t][c] + lb;
      ColRef cr{t, ls, group[ls].first, group[ls].second, seen[ls]++, {}};
      for (size_t k = 0; k < f.pts[t][c].size(); ++k) cr.samples.push_back({pt_id(f.pts[t][c][k]), p.sampled_values[t][c][k]});
      cols.push_back(cr);
    }
  }
  for (size_t si = 0; si < f.sizes.size(); ++si) {
    std::vector<QuotBatch> batches;
    for (auto& c : cols) {
      if (c.lde_log != f.sizes[si]) continue;
      for (auto& sm : c.samples) {
        size_t b = 0;
        while (b < batches.size() && batches[b].pt != sm.first) ++b;
        if (b == batches.size()) batches.push_back({sm.first, {}});
        batches[b].cols.push_back({c.tree, (int)si, c.base, c.ncol, c.j, sm.second});
      }
    }
    plan.by_size.push_back(std::move(batches));
  }
  return plan;
}

// The back: the four trace-tree decommitments, the FRI quotients at the queried positions, the FRI layers.
void verify_back(const VerifyFront& f, const Checks& ck) {
  lmn_verify_report* const rep = ck.rep;
  auto check = [&](uint32_t bit, bool ok, const std::string& what) { ck.check(bit, ok, what); };
  auto fail = [&](const std::string& what) { ck.fail(what); };
  const Proof& p = f.p;
  const int lb = f.lb, top = f.top;
  const std::vector<int>& sizes = f.sizes;
  const std::vector<QM31>& alphas = f.alphas;
  const std::vector<uint32_t>& queries = f.queries;
  const QM31 quot_alpha = f.quot_alpha;
  auto positions = [&](int ls) -> const std::vector<uint32_t>& { return f.pos_by_log.at(ls); };

  // ---- trace tree decommitments
  for (int t = 0; t < 4; ++t) {
    std::vector<int> logs;
    std::map<int, std::vector<uint32_t>> qmap;
    for (int l : f.tree_logs[t]) {
      logs.push_back(l + lb);
      qmap[l + lb] = positions(l + lb);
    }
    check(LMN_CHECK_TREE_DECOMMIT, merkle_verify(p.commitments[t], logs, qmap, p.queried_values[t], p.decommitments[t]),
          "Merkle tree " + std::to_string(t));
  }
  // With wrong query positions (a failed tree decommitment) the queried values do not line up with the positions
  // below: the remaining checks would only report shape errors.
  if (rep && (rep->checks_failed & LMN_CHECK_TREE_DECOMMIT)) return;

  // ---- FRI answers: quotient values at the queried positions, per LDE size
  const QuotPlan plan = plan_quotients(f);
  std::map<int, std::map<uint32_t, QM31>> quot_at;
  for (size_t si = 0; si < sizes.size(); ++si) {
    const int ls = sizes[si];
    const auto& qp = positions(ls);
    for (size_t qi = 0; qi < qp.size(); ++qi) {
      Pt dp = domain_point(ls, qp[qi]);
      QM31 acc = q_zero();
      for (const QuotBatch& batch : plan.by_size[si]) {
        const QPt& pt = plan.pts[batch.pt];
        QM31 alpha = q_one(), num = q_zero();
        for (const QuotCol& cr : batch.cols) {
          alpha = q_mul(alpha, quot_alpha);
          size_t idx = cr.base + qi * (size_t)cr.ncol + (size_t)cr.j;
          if (idx >= p.queried_values[cr.tree].size()) fail("queried values shape");
          uint32_t fv = p.queried_values[cr.tree][idx];
          QM31 val = cr.value;
          QM31 la = q_sub(q_conj(val), val);
          QM31 lc2 = q_sub(q_conj(pt.y), pt.y);
          QM31 lbb = q_sub(q_mul(val, lc2), q_mul(la, pt.y));
          num = q_add(num, q_mul(alpha, q_sub(q_mul_m(lc2, fv), q_add(q_mul_m(la, dp.y), lbb))));
        }
        CM31 prx{pt.x.a, pt.x.b}, pix{pt.x.c, pt.x.d}, pry{pt.y.a, pt.y.b}, piy{pt.y.c, pt.y.d};
        CM31 dx{m_sub(prx.a, dp.x), prx.b}, dy{m_sub(pry.a, dp.y), pry.b};
        CM31 den = c_sub(c_mul(dx, piy), c_mul(dy, pix));
        if (c_norm(den) == 0) fail("degenerate quotient denominator");
        acc = q_add(q_mul(acc, q_pow(quot_alpha, batch.cols.size())), q_mul_c(num, c_inv(den)));
      }
      quot_at[ls][qp[qi]] = acc;
    }
  }

  // ---- FRI first layer: rebuild sibling pairs, Merkle-check, fold circle -> line
  std::map<int, std::map<uint32_t, QM31>> first_vals;
  std::map<int, std::vector<uint32_t>> dec_by_log;
  {
    size_t wi = 0;
    for (int ls : sizes)
      if (!rebuild_pairs(positions(ls), quot_at[ls], p.first_layer.fri_witness, wi, dec_by_log[ls], first_vals[ls]))
        fail("first layer witness");
    if (wi != p.first_layer.fri_witness.size()) fail("first layer witness too long");
    std::vector<int> logs;
    std::vector<uint32_t> qv;
    for (int ls : sizes) {
      for (int k = 0; k < 4; ++k) logs.push_back(ls);
      for (uint32_t pos : dec_by_log[ls]) {
        QM31 v = first_vals[ls][pos];
        qv.insert(qv.end(), {v.a, v.b, v.c, v.d});
      }
    }
    check(LMN_CHECK_FRI_DECOMMIT, merkle_verify(p.first_layer.commitment, logs, dec_by_log, qv, p.first_layer.decommitment),
          "FRI first layer Merkle");
  }
  auto fold_circle = [&](const std::map<uint32_t, QM31>& vals, int ls, QM31 alpha) {
    std::map<uint32_t, QM31> out;
    for (auto& kv : vals) {
      if (kv.first & 1u) continue;
      QM31 a = kv.second, b = vals.at(kv.first + 1);
      uint32_t y = domain_point(ls, kv.first).y;
      out[kv.first >> 1] = q_add(q_add(a, b), q_mul(alpha, q_mul_m(q_sub(a, b), m_inv(y))));
    }
    return out;
  };
  int layer_log = top - 1;
  std::map<uint32_t, QM31> cur = fold_circle(first_vals[top], top, alphas[0]);
  std::vector<int> left(sizes.begin() + 1, sizes.end());
  std::vector<uint32_t> lq = fold_positions(queries, 1);
  for (size_t li = 0; li < p.inner_layers.size(); ++li) {
    const FriLayerProof& l = p.inner_layers[li];
    std::vector<uint32_t> dpos;
    std::map<uint32_t, QM31> vals;
    size_t wi = 0;
    if (!rebuild_pairs(lq, cur, l.fri_witness, wi, dpos, vals) || wi != l.fri_witness.size())
      fail("inner layer witness");
    std::vector<uint32_t> qv;
    for (uint32_t pos : dpos) {
      QM31 v = vals[pos];
      qv.insert(qv.end(), {v.a, v.b, v.c, v.d});
    }
    std::map<int, std::vector<uint32_t>> dq;
    dq[layer_log] = dpos;
    check(LMN_CHECK_FRI_DECOMMIT, merkle_verify(l.commitment, {layer_log, layer_log, layer_log, layer_log}, dq, qv, l.decommitment),
          "FRI inner layer " + std::to_string(li) + " Merkle");
    QM31 alpha = alphas[li + 1];
    std::map<uint32_t, QM31> nxt;
    for (uint32_t pos : dpos) {
      if (pos & 1u) continue;
      QM31 a = vals[pos], b = vals[pos + 1];
      uint32_t x = line_domain_x(layer_log, pos);
      nxt[pos >> 1] = q_add(q_add(a, b), q_mul(alpha, q_mul_m(q_sub(a, b), m_inv(x))));
    }
    layer_log -= 1;
    lq = fold_positions(lq, 1);
    for (auto it = left.begin(); it != left.end();) {
      if (*it - 1 == layer_log) {
        auto fc = fold_circle(first_vals[*it], *it, alpha);
        for (auto& kv : nxt) {
          auto hit = fc.find(kv.first);
          if (hit == fc.end()) fail("FRI column positions");
          kv.second = q_add(q_mul(kv.second, q_mul(alpha, alpha)), hit->second);
        }
        it = left.erase(it);
      } else {
        ++it;
      }
    }
    cur.swap(nxt);
  }
  if (!left.empty()) fail("unconsumed FRI columns");
  // ---- last layer: the polynomial must reproduce the folded values
  for (auto& kv : cur) {
    uint32_t x = line_domain_x(layer_log, kv.first);
    QM31 val = q_zero();
    for (size_t j = 0; j < p.last_layer_coeffs.size(); ++j) {
      QM31 term = p.last_layer_coeffs[j];
      uint32_t xx = x;
      for (size_t jj = j; jj; jj >>= 1) {
        if (jj & 1) term = q_mul_m(term, xx);
        xx = m_sub(m_dbl(m_sqr(xx)), 1u);
      }
      val = q_add(val, term);
    }
    check(LMN_CHECK_FRI_FOLDS, q_eq(val, kv.second), "FRI last layer");
  }
}

// ---- lmn_verify_many: what the stager hands to the device stage (kernels.h VmLayout / VmProof)
constexpr uint32_t VM_MAX_BUCKETS = 4;              // claims of different shapes one call takes to the device; further ones: stage 2
constexpr uint32_t VM_CHUNK_PROOFS = 256;           // proofs of one chunk: one transfer in, one out, one wait
constexpr size_t VM_CHUNK_WORDS = (size_t)4 << 20;  // and its block's words (16 MiB); a chunk closes at whichever comes first
constexpr size_t VM_MAX_PROOF_WORDS = (size_t)1 << 20;   // a proof whose bytes and scratch exceed this many words: stage 2

// The layout table of the proof's claim, as words: false = a shape the device stage does not take (stage 2).
bool build_layout(const VerifyFront& f, const QuotPlan& plan, std::vector<uint32_t>& words) {
  const size_t n_inner = f.p.inner_layers.size();
  if (f.sizes.size() > VM_MAX_SIZES || 5 + n_inner > VM_MAX_TREES || f.top > 29 || f.queries.size() > VM_MAX_POS) return false;
  VmLayout L;
  memset(&L, 0, sizeof L);
  L.n_sizes = (uint32_t)f.sizes.size();
  L.top = (uint32_t)f.top;
  L.n_inner = (uint32_t)n_inner;
  L.n_trees = (uint32_t)(5 + n_inner);
  std::vector<VmBatch> batches;
  std::vector<VmBatchCol> bcols;
  for (size_t si = 0; si < f.sizes.size(); ++si) {
    L.size_log[si] = (uint32_t)f.sizes[si];
    L.size_batch0[si] = (uint32_t)batches.size();
    for (const QuotBatch& b : plan.by_size[si]) {
      batches.push_back({(uint32_t)b.pt, (uint32_t)bcols.size(), (uint32_t)(bcols.size() + b.cols.size())});
      for (const QuotCol& c : b.cols) bcols.push_back({(uint32_t)c.tree, (uint32_t)c.size, (uint32_t)c.ncol, (uint32_t)c.j});
    }
  }
  for (size_t si = f.sizes.size(); si <= VM_MAX_SIZES; ++si) L.size_batch0[si] = (uint32_t)batches.size();
  L.n_batches = (uint32_t)batches.size();
  L.n_bcols = (uint32_t)bcols.size();
  for (uint32_t& j : L.join_of_layer) j = VM_NONE;
  for (size_t si = 1; si < f.sizes.size(); ++si) {
    const int li = f.top - 1 - f.sizes[si];   // its circle fold joins the line behind inner layer li
    if (li < 0 || li >= (int)n_inner) return false;   // ("unconsumed FRI columns": the host says so after everything else)
    L.join_of_layer[li] = (uint32_t)si;
  }
  for (uint32_t& m : L.tree_max_log) m = VM_NONE;
  auto add_col = [&](size_t t, int log) {
    if (L.tree_ncols[t][log] == 0xffffu) return false;
    ++L.tree_ncols[t][log];
    if (L.tree_max_log[t] == VM_NONE || (uint32_t)log > L.tree_max_log[t]) L.tree_max_log[t] = (uint32_t)log;
    return true;
  };
  for (size_t t = 0; t < 4; ++t)
    for (int l : f.tree_logs[t])
      if (!add_col(t, l + f.lb)) return false;
  for (int k = 0; k < 4; ++k) {
    for (int ls : f.sizes) add_col(4, ls);
    for (size_t li = 0; li < n_inner; ++li) add_col(5 + li, f.top - 1 - (int)li);
  }
  words.resize((sizeof L + batches.size() * sizeof(VmBatch) + bcols.size() * sizeof(VmBatchCol)) / 4);
  char* o = (char*)words.data();
  memcpy(o, &L, sizeof L);
  if (!batches.empty()) memcpy(o + sizeof L, batches.data(), batches.size() * sizeof(VmBatch));
  if (!bcols.empty()) memcpy(o + sizeof L + batches.size() * sizeof(VmBatch), bcols.data(), bcols.size() * sizeof(VmBatchCol));
  return true;
}

// words of scratch the FRI trees' leaf lists take: 8 per sibling pair, as the positions imply
void leaf_words(const VerifyFront& f, std::vector<uint32_t>& per_tree) {
  uint32_t first = 0;
  for (int ls : f.sizes) first += 8u * (uint32_t)fold_positions(f.pos_by_log.at(ls), 1).size();
  per_tree.assign(1, first);
  std::vector<uint32_t> lq = fold_positions(f.queries, 1);
  for (size_t li = 0; li < f.p.inner_layers.size(); ++li) {
    lq = fold_positions(lq, 1);
    per_tree.push_back(8u * (uint32_t)lq.size());
  }
}

// Appends the proof's lists to the chunk's words and describes them.  Every length in the descriptor is the length of
// what was appended here; the leaf spans and the verdict index are set when the chunk closes.
VmProof stage_proof(const VerifyFront& f, const QuotPlan& plan, std::vector<uint32_t>& data) {
  static_assert(sizeof(Hash32) == 32 && sizeof(QM31) == 16 && sizeof(QPt) == 32, "lists are staged as they lie in memory");
  const Proof& p = f.p;
  VmProof d;
  memset(&d, 0, sizeof d);
  auto put = [&](const void* src, size_t n_words, size_t n_elems) {
    VmSpan s{(uint32_t)data.size(), (uint32_t)n_elems};
    if (n_words) data.insert(data.end(), (const uint32_t*)src, (const uint32_t*)src + n_words);
    return s;
  };
  d.pos = put(f.queries.data(), f.queries.size(), f.queries.size());
  for (int t = 0; t < 4; ++t) d.queried[t] = put(p.queried_values[t].data(), p.queried_values[t].size(), p.queried_values[t].size());
  std::vector<const Decommitment*> dec;
  std::vector<const Hash32*> roots;
  for (int t = 0; t < 4; ++t) dec.push_back(&p.decommitments[t]), roots.push_back(&p.commitments[t]);
  dec.push_back(&p.first_layer.decommitment), roots.push_back(&p.first_layer.commitment);
  for (auto& l : p.inner_layers) dec.push_back(&l.decommitment), roots.push_back(&l.commitment);
  for (size_t t = 0; t < dec.size(); ++t) {
    d.hash_wit[t] = put(dec[t]->hash_witness.data(), dec[t]->hash_witness.size() * 8, dec[t]->hash_witness.size());
    d.col_wit[t] = put(dec[t]->column_witness.data(), dec[t]->column_witness.size(), dec[t]->column_witness.size());
  }
  d.fri_wit[0] = put(p.first_layer.fri_witness.data(), p.first_layer.fri_witness.size() * 4, p.first_layer.fri_witness.size());
  for (size_t li = 0; li < p.inner_layers.size(); ++li) {
    const auto& w = p.inner_layers[li].fri_witness;
    d.fri_wit[1 + li] = put(w.data(), w.size() * 4, w.size());
  }
  d.last = put(p.last_layer_coeffs.data(), p.last_layer_coeffs.size() * 4, p.last_layer_coeffs.size());
  d.roots = (uint32_t)data.size();
  for (const Hash32* r : roots) put(r->w, 8, 1);
  d.samples = (uint32_t)data.size();
  for (auto& batches : plan.by_size)
    for (auto& b : batches)
      for (auto& c : b.cols) {
        put(&c.value, 4, 1);
        d.qbase[c.tree][c.size] = (uint32_t)c.base;
      }
  d.points = (uint32_t)data.size();
  d.n_points = (uint32_t)plan.pts.size();
  put(plan.pts.data(), plan.pts.size() * 8, plan.pts.size());
  d.alphas = (uint32_t)data.size();
  put(&f.quot_alpha, 4, 1);
  put(f.alphas.data(), f.alphas.size() * 4, f.alphas.size());
  return d;
}

// one call's exception guard per proof: the code lmn_verify_with_config would return (capi_internal.h capi_guard)
template <typename F>
int proof_guard(std::string& text, F&& body) {
  try {
    body();
    return LMN_OK;
  } catch (...) {
    return current_exception_code(text);
  }
}

}  // namespace

void verify_proof(const uint8_t* data, size_t len, const lmn_config& expect, const lmn_settings* settings,
                  lmn_verify_report* rep) {
  if (expect.protocol_variant & ~LMN_PV_ALL) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "bad protocol_variant (unknown LMN_PV_* bits)");
  if (rep) memset(rep, 0, sizeof *rep);
  const Checks ck{rep, nullptr};
  const VerifyFront f = verify_front(data, len, expect, settings, ck);
  verify_back(f, ck);
}

// lmn_verify_many (luminair_hip.h): the front on the host per proof, the back on the device per chunk.
void Context::verify_many(const uint8_t* const* proofs, const size_t* lens, uint32_t n, const lmn_settings* settings,
                          const lmn_config& expect, lmn_verify_result* results, std::string& first_rejection) {
  const char* F = "verify_many: ";
  if (shard_.active)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, std::string(F) + "ctx is sharded (lmn_ctx_set_shard): proofs are verified on an unsharded context only");
  require_expected_config(expect);
  uint32_t first_index = n;
  auto reject = [&](uint32_t i, int rc, uint32_t bits, uint32_t stage, const std::string& text) {
    results[i] = lmn_verify_result{rc, bits, stage};
    if (i < first_index) {
      first_index = i;
      first_rejection = text;
    }
  };
  struct Pending {
    uint32_t index, bucket, n_pos;
    VmProof desc;
    std::vector<uint32_t> leaves;   // words per FRI tree
  };
  std::vector<std::vector<uint32_t>> bucket_layouts;   // the call's buckets, by layout table
  std::vector<uint32_t> data;
  std::vector<Pending> pend;
  size_t chunk_scratch = 0;

  auto flush = [&] {
    if (pend.empty()) return;
    std::stable_sort(pend.begin(), pend.end(), [](const Pending& a, const Pending& b) { return a.bucket < b.bucket; });
    struct Launch {
      uint32_t layout_off, proofs_off, n_proofs, n_trees, max_pos;
    };
    std::vector<Launch> launches;
    // the block: the proofs' lists | per bucket its layout table and descriptors | scratch | verdicts
    size_t staged = data.size();
    for (size_t a = 0; a < pend.size();) {
      size_t b = a;
      uint32_t max_pos = 0;
      while (b < pend.size() && pend[b].bucket == pend[a].bucket) max_pos = std::max(max_pos, pend[b++].n_pos);
      const std::vector<uint32_t>& lay = bucket_layouts[pend[a].bucket];
      const uint32_t n_trees = ((const VmLayout*)lay.data())->n_trees;
      launches.push_back({(uint32_t)staged, (uint32_t)(staged + lay.size()), (uint32_t)(b - a), n_trees, max_pos});
      staged += lay.size() + (b - a) * (sizeof(VmProof) / 4);
      a = b;
    }
    size_t at = staged;   // scratch, then verdicts
    for (Pending& pd : pend)
      for (size_t k = 0; k < pd.leaves.size(); ++k) {
        pd.desc.leaves[k] = VmSpan{(uint32_t)at, pd.leaves[k]};
        at += pd.leaves[k];
      }
    const size_t verdict0 = at;
    for (Pending& pd : pend) {
      pd.desc.verdict = (uint32_t)at;
      at += 1 + ((const VmLayout*)bucket_layouts[pd.bucket].data())->n_trees;
    }
    const size_t total = at, n_verdict = total - verdict0;
    if (total > 0xffffffffu / 4) throw LmnError(LMN_ERR_INTERNAL, std::string(F) + "a chunk's block exceeds its bound");
    data.reserve(staged);
    {
      size_t k = 0;
      for (const Launch& l : launches) {
        const std::vector<uint32_t>& lay = bucket_layouts[pend[k].bucket];
        data.insert(data.end(), lay.begin(), lay.end());
        for (uint32_t j = 0; j < l.n_proofs; ++j, ++k)
          data.insert(data.end(), (const uint32_t*)&pend[k].desc, (const uint32_t*)&pend[k].desc + sizeof(VmProof) / 4);
      }
    }
    set_device();
    // the context's verify buffers (not its arena): page-locked staged words | verdicts, and the device block
    const size_t host_bytes = (staged + n_verdict) * 4, dev_bytes = total * 4;
    if (host_bytes > vm_host_cap_) {
      if (vm_host_) lmn_host_free_pinned(vm_host_);
      vm_host_ = nullptr, vm_host_cap_ = 0;
      vm_host_ = (char*)lmn_host_alloc_pinned(host_bytes + host_bytes / 2);
      vm_host_cap_ = host_bytes + host_bytes / 2;
    }
    if (dev_bytes > vm_dev_cap_) {
      if (vm_dev_) lmn_dev_free(vm_dev_);
      vm_dev_ = nullptr, vm_dev_cap_ = 0;
      vm_dev_ = (char*)lmn_dev_malloc(dev_bytes + dev_bytes / 2);
      vm_dev_cap_ = dev_bytes + dev_bytes / 2;
    }
    memcpy(vm_host_, data.data(), staged * 4);
    uint32_t* h_verdict = (uint32_t*)vm_host_ + staged;
    memset(h_verdict, 0, n_verdict * 4);
    uint32_t* blk = (uint32_t*)vm_dev_;
    lmn_h2d(blk, vm_host_, staged * 4, stream_);
    for (const Launch& l : launches) {
      launch_verify_values(blk, l.layout_off, l.proofs_off, l.n_proofs, stream_, &verify_counters_[2]);
      const uint32_t tpb = 2 * l.max_pos <= 64 ? 64 : 2 * l.max_pos <= 128 ? 128 : 256;   // a level has at most two nodes per position
      launch_verify_trees(blk, l.layout_off, l.proofs_off, l.n_proofs, l.n_trees, tpb, stream_, &verify_counters_[2]);
    }
    lmn_d2h(h_verdict, blk + verdict0, n_verdict * 4, stream_);
    lmn_sync(stream_);
    ++verify_counters_[3];
    for (const Pending& pd : pend) {
      const uint32_t n_trees = ((const VmLayout*)bucket_layouts[pd.bucket].data())->n_trees;
      const uint32_t* v = h_verdict + (pd.desc.verdict - verdict0);
      for (uint32_t k = 0; k <= n_trees; ++k)
        if ((v[k] & VM_DONE_MASK) != VM_DONE) throw LmnError(LMN_ERR_INTERNAL, std::string(F) + "the device stage left a verdict word unwritten");
      ++verify_counters_[0];
      // diagnose's rule, applied to the verdict words: nothing behind a failed tree decommitment counts
      int bad_tree = -1, bad_layer = -1;
      for (uint32_t t = 0; t < n_trees; ++t)
        if (v[1 + t] & VM_FAIL_TREE) {
          if (t < 4 && bad_tree < 0) bad_tree = (int)t;
          if (t >= 4 && bad_layer < 0) bad_layer = (int)t - 4;
        }
      const uint32_t vv = v[0] & ~VM_DONE_MASK;
      if (bad_tree >= 0) {
        reject(pd.index, LMN_ERR_VERIFICATION, LMN_CHECK_TREE_DECOMMIT, 1, "StwoVerifierError: Merkle tree " + std::to_string(bad_tree));
      } else if (vv & ~VM_FAIL_FOLDS) {
        const char* what = vv & VM_FAIL_QUERIED_SHAPE ? "queried values shape"
                           : vv & VM_FAIL_DENOMINATOR ? "degenerate quotient denominator"
                           : vv & VM_FAIL_WITNESS_SHORT ? "FRI layer witness"
                           : vv & VM_FAIL_WITNESS_LONG ? "FRI layer witness too long"
                                                       : "FRI column positions";
        reject(pd.index, LMN_ERR_VERIFICATION, LMN_CHECK_SHAPE, 1, std::string("StwoVerifierError: ") + what);
      } else if (bad_layer >= 0 || vv) {
        const uint32_t bits = (bad_layer >= 0 ? LMN_CHECK_FRI_DECOMMIT : 0u) | (vv ? LMN_CHECK_FRI_FOLDS : 0u);
        reject(pd.index, LMN_ERR_VERIFICATION, bits, 1,
               bad_layer == 0  ? std::string("StwoVerifierError: FRI first layer Merkle")
               : bad_layer > 0 ? "StwoVerifierError: FRI inner layer " + std::to_string(bad_layer - 1) + " Merkle"
                               : std::string("StwoVerifierError: FRI last layer"));
      } else {
        results[pd.index] = lmn_verify_result{LMN_OK, 0u, 1u};
      }
    }
    pend.clear();
    data.clear();
    chunk_scratch = 0;
  };

  for (uint32_t i = 0; i < n; ++i) {
    results[i] = lmn_verify_result{LMN_ERR_INTERNAL, 0u, 0u};
    if (!proofs[i]) {
      reject(i, LMN_ERR_INVALID_ARGUMENT, 0u, 0u, std::string(F) + "proofs[" + std::to_string(i) + "] is null");
      continue;
    }
    VerifyFront f;
    uint32_t bit = 0;
    std::string text;
    int rc = proof_guard(text, [&] { f = verify_front(proofs[i], lens[i], expect, settings, Checks{nullptr, &bit}); });
    if (rc != LMN_OK) {
      reject(i, rc, bit, 0u, text);
      continue;
    }
    // the device stage, unless the proof is awkward for it: then the host's back half judges it (stage 2)
    const QuotPlan plan = plan_quotients(f);
    std::vector<uint32_t> layout, leaves;
    bool device = build_layout(f, plan, layout);
    size_t scratch = 0;
    if (device) {
      leaf_words(f, leaves);
      for (uint32_t w : leaves) scratch += w;
      device = lens[i] / 4 + layout.size() + sizeof(VmProof) / 4 + scratch <= VM_MAX_PROOF_WORDS;
    }
    uint32_t bucket = 0;
    if (device) {
      while (bucket < bucket_layouts.size() && bucket_layouts[bucket] != layout) ++bucket;
      if (bucket == bucket_layouts.size()) {
        if (bucket == VM_MAX_BUCKETS)
          device = false;
        else
          bucket_layouts.push_back(layout);
      }
    }
    if (!device) {
      ++verify_counters_[1];
      bit = 0;
      rc = proof_guard(text, [&] { verify_back(f, Checks{nullptr, &bit}); });
      if (rc != LMN_OK)
        reject(i, rc, bit, 2u, text);
      else
        results[i] = lmn_verify_result{LMN_OK, 0u, 2u};
      continue;
    }
    if (pend.size() == VM_CHUNK_PROOFS || data.size() + chunk_scratch + lens[i] / 4 + scratch > VM_CHUNK_WORDS) flush();
    Pending pd;
    pd.index = i;
    pd.bucket = bucket;
    pd.n_pos = (uint32_t)f.queries.size();
    pd.desc = stage_proof(f, plan, data);
    pd.leaves = std::move(leaves);
    chunk_scratch += scratch + 1 + VM_MAX_TREES + layout.size() + sizeof(VmProof) / 4;
    pend.push_back(std::move(pd));
  }
  flush();
}

}  // namespace lmn

extern "C" int lmn_verify_many(lmn_ctx* ctx, const uint8_t* const* proofs, const size_t* lens, uint32_t n,
                               const lmn_settings* settings, const lmn_config* expected, lmn_verify_result* results) {
  if (!ctx || !ctx->impl) return LMN_ERR_INVALID_ARGUMENT;
  if (n == 0) return LMN_OK;
  std::string first_rejection;
  const int rc = lmn::capi_guard(ctx, [&] {
    if (!proofs || !lens || !results)
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, std::string("verify_many: ") + (!proofs ? "proofs" : !lens ? "lens" : "results") +
                                                   " is null with n = " + std::to_string(n));
    lmn_config c;
    if (expected) {
      c = *expected;
    } else {
      lmn_default_config(&c);  // PcsConfig::default(), protocol variant 0
      c.protocol_variant = 0;
    }
    ctx->impl->verify_many(proofs, lens, n, settings, c, results, first_rejection);
  });
  if (rc == LMN_OK && !first_rejection.empty()) {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    ctx->last_error = first_rejection;
  }
  return rc;
}
