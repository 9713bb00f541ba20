// prove(), inside stwo::prover::prove: proof of work, query positions, and the decommitment of every tree and FRI layer
// through one planned gather launch; assembles the proof container.
#include "prove_run.h"

#include <array>

namespace lmn {

PowWords pow_words_of(const Channel& ch, uint32_t pow_bits, bool& kat) {
  const bool prefixed = (ch.flags() & LMN_PV_POW_PREFIXED) != 0;
  kat = !prefixed && !(ch.flags() & LMN_PV_MIX_U64_HASHED);
  PowWords w;
  const Hash32 src = prefixed ? ch.pow_prefixed_digest(pow_bits) : ch.digest();
  memcpy(w.w, src.w, sizeof w.w);
  return w;
}

// Proof of work on the device (k_pow_grind): windows of 2^wlog nonces in ascending order, POW_WINDOWS_PER_WAIT per wait,
// until one holds a passing nonce; its minimum is the host loop's answer (Channel::grind).  The window grows with
// pow_bits (about two expected hits per window) up to pow_window_log_, the cap that keeps one launch well under a
// millisecond (2^24 nonces: 0.24 ms measured), so that other contexts' launches interleave.
// (POW_WINDOWS_PER_WAIT launches per host wait: kernels.h)

int Context::grind_window_log(uint32_t pow_bits) const {
  return std::min(pow_window_log_, std::max(POW_MIN_WINDOW_LOG, (int)pow_bits + 1));
}

uint64_t Context::device_grind(const Channel& ch, uint32_t pow_bits) {
  bool kat;
  const PowWords w = pow_words_of(ch, pow_bits, kat);
#ifndef LMN_BATCH
  ++counters_[0];   // (the lock-step build counts in grind_many, where its grinds go)
#endif
  return device_grind_from(w, kat, pow_bits, 0);
}

uint64_t Context::device_grind_from(const PowWords& w, bool kat, uint32_t pow_bits, uint64_t base) {
#ifdef LMN_BATCH
  // lock-step members must issue identical sequences, and this loop's length depends on the digest: the members grind
  // together, in one collective (grind_many below); a thread outside any batch is a group of one.  (From nonce 0 on
  // whatever `base` says: the rounds are the collective's.)
  (void)base;
  return grind_many(&w, 1, kat, pow_bits)[0];
#else
  if (!pow_best_) pow_best_ = (unsigned long long*)lmn_dev_malloc(sizeof(unsigned long long));
  unsigned long long* found = (unsigned long long*)pin_alloc(sizeof(unsigned long long));
  const int wlog = grind_window_log(pow_bits);
  lmn_memset(pow_best_, 0xff, sizeof(unsigned long long), stream_);
  for (;;) {
    for (int k = 0; k < POW_WINDOWS_PER_WAIT; ++k, base += 1ull << wlog)
      launch_pow_grind(w, kat, base, wlog, pow_bits, pow_best_, stream_);
    lmn_d2h(found, pow_best_, sizeof(unsigned long long), stream_);
    lmn_sync(stream_);
    ++counters_[1];
    if (*found != ~0ull) return *found;
  }
#endif
}

// Many digests ground together (k_grind_many): every round uploads the table of the digests still pending, queues
// POW_WINDOWS_PER_WAIT launches of consecutive windows over all of them, downloads best[] and waits; digests with a hit
// leave the table and base advances by the whole round.  Invariant: every pending digest has been examined on exactly
// [0, base) - so a digest's first hit is the minimum over [0, end of its round), the host loop's answer, whatever the
// window was in each round.  The window shrinks with the number of pending digests so that ONE launch examines at most
// 2^pow_window_log_ nonces in all (the rule that keeps a grind launch short for the other contexts; the smallest window,
// one block per digest, is the floor) and grows again as digests finish.  Returns the host waits spent.
#ifdef LMN_BATCH
// (the batch build runs this inside a collective, on one member's thread while the others wait: transfers and waits
// go straight to the runtime instead of into the member's copy list and the group's rendezvous)
static void pow_h2d(void* d, const void* h, size_t n, lmn_stream_t s) {
  batch_check_hip(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s), "grind_many upload");
}
static void pow_d2h(void* h, const void* d, size_t n, lmn_stream_t s) {
  batch_check_hip(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, s), "grind_many download");
}
static void pow_wait(lmn_stream_t s) { batch_stream_wait(s); }
#else
static void pow_h2d(void* d, const void* h, size_t n, lmn_stream_t s) { lmn_h2d(d, h, n, s); }
static void pow_d2h(void* h, const void* d, size_t n, lmn_stream_t s) { lmn_d2h(h, d, n, s); }
static void pow_wait(lmn_stream_t s) { lmn_sync(s); }
#endif

uint64_t Context::grind_rounds(const PowWords* w, uint32_t n, bool kat, uint32_t pow_bits, uint64_t* nonces) {
  typedef unsigned long long u64;
  constexpr size_t PER_DIGEST = sizeof(PowWords) + sizeof(u64) + sizeof(uint32_t);   // digests | best | pending
  if (n > pow_many_cap_) {
    if (pow_many_dev_) lmn_dev_free(pow_many_dev_);
    if (pow_many_host_) lmn_host_free_pinned(pow_many_host_);
    pow_many_dev_ = pow_many_host_ = nullptr;
    pow_many_cap_ = 0;
    const uint32_t cap = std::max(64u, n);
    pow_many_dev_ = (char*)lmn_dev_malloc(cap * PER_DIGEST);
    pow_many_host_ = (char*)lmn_host_alloc_pinned(cap * PER_DIGEST);
    pow_many_cap_ = cap;
  }
  const size_t cap = pow_many_cap_;
  PowWords* d_w = (PowWords*)pow_many_dev_;
  u64* d_best = (u64*)(pow_many_dev_ + cap * sizeof(PowWords));
  uint32_t* d_pend = (uint32_t*)(pow_many_dev_ + cap * (sizeof(PowWords) + sizeof(u64)));
  PowWords* h_w = (PowWords*)pow_many_host_;
  u64* h_best = (u64*)(pow_many_host_ + cap * sizeof(PowWords));
  uint32_t* h_pend = (uint32_t*)(pow_many_host_ + cap * (sizeof(PowWords) + sizeof(u64)));
  memcpy(h_w, w, n * sizeof(PowWords));
  for (uint32_t i = 0; i < n; ++i) {
    h_best[i] = ~0ull;
    h_pend[i] = i;
  }
  pow_h2d(d_w, h_w, n * sizeof(PowWords), stream_);
  pow_h2d(d_best, h_best, n * sizeof(u64), stream_);
  uint64_t waits = 0;
  uint32_t n_pending = n;
  for (uint64_t base = 0; n_pending;) {
    int lg = 0;
    while ((1u << lg) < n_pending) ++lg;
    const int wlog = std::max(POW_MIN_WINDOW_LOG, std::min((int)pow_bits + 1, pow_window_log_ - lg));
    pow_h2d(d_pend, h_pend, n_pending * sizeof(uint32_t), stream_);
    for (int k = 0; k < POW_WINDOWS_PER_WAIT; ++k)
      launch_grind_many(d_w, d_pend, n_pending, kat, base + ((uint64_t)k << wlog), wlog, pow_bits, d_best, stream_);
    pow_d2h(h_best, d_best, n * sizeof(u64), stream_);
    pow_wait(stream_);
    ++waits;
    ++counters_[1];
    uint32_t kept = 0;   // (the table just uploaded is read by launches that have finished: it may be rewritten)
    for (uint32_t i = 0; i < n_pending; ++i)
      if (h_best[h_pend[i]] == ~0ull) h_pend[kept++] = h_pend[i];
    n_pending = kept;
    base += (uint64_t)POW_WINDOWS_PER_WAIT << wlog;
  }
  for (uint32_t i = 0; i < n; ++i) nonces[i] = h_best[i];
  return waits;
}

#ifdef LMN_BATCH
// the grind collective (batch.h): run by the member that completes the rendezvous, with the context of any present member
// (`arg`; the members of a batch share one config, hence pow_bits and form) over the digests of all of them
struct GrindJob {
  Context* ctx;
  bool kat;
  uint32_t pow_bits;
};
uint64_t Context::grind_collective(void* arg, const BatchCollectiveItem* items, int n_items, hipStream_t) {
  const GrindJob& job = *static_cast<const GrindJob*>(arg);
  std::vector<PowWords> all;
  for (int i = 0; i < n_items; ++i) {
    const PowWords* w = static_cast<const PowWords*>(items[i].in);
    all.insert(all.end(), w, w + items[i].n);
  }
  std::vector<uint64_t> nonces(all.size());
  const uint64_t waits = job.ctx->grind_rounds(all.data(), (uint32_t)all.size(), job.kat, job.pow_bits, nonces.data());
  size_t at = 0;
  for (int i = 0; i < n_items; at += items[i].n, ++i)
    memcpy(items[i].out, nonces.data() + at, items[i].n * sizeof(uint64_t));
  return waits;
}
#endif

std::vector<uint64_t> Context::grind_many(const PowWords* w, uint32_t n, bool kat, uint32_t pow_bits) {
  std::vector<uint64_t> nonces(n);
  if (n == 0) return nonces;
  ++counters_[0];
#ifdef LMN_BATCH
  GrindJob job{this, kat, pow_bits};
  batch_collective(&Context::grind_collective, &job, w, n, nonces.data(), stream_);
#else
  grind_rounds(w, n, kat, pow_bits, nonces.data());
#endif
  return nonces;
}

uint64_t Context::grind(const Channel& ch, uint32_t pow_bits) {
  if ((int)pow_bits >= pow_device_min_bits_) return device_grind(ch, pow_bits);
  return ch.grind(pow_bits);
}

void Context::run_queries(ProofRun& r) {
  LMN_RUN_ALIASES(r);
  // ---- proof of work + queries
  const int ls0 = quots[0].log;
  if (r.close.on) {   // closed on the device, replayed by run_fri_commit
    proof.proof_of_work = r.close.nonce;
    queries = r.close.positions;
  } else {
    proof.proof_of_work = grind(channel, cfg.pow_bits);
    channel.mix_u64(proof.proof_of_work);
    queries = draw_query_positions(channel, cfg.n_queries, (uint32_t)ls0);
  }
  pos_by_log.clear();
  for (int ls : sizes) pos_by_log[ls] = fold_positions(queries, ls0 - ls);

  hm.mark("pow+queries");
}

// LMN_DEVICE_DECOMMIT=1 (docs/SWITCHES.md; effective where the close runs on the device): the openings of every tree
// [first FRI tree, inner layers..., trees 0..3] planned by k_open_plan from the positions k_fri_queries left in the result
// block, fetched into a page-locked block sized from n_queries - all queued behind k_fri_queries, in front of the FRI wait.
// The descriptor table depends on nothing the device has yet to compute: layer and column pointers (arena, or the prepared
// slab: absolute pointers serve both), columns per size, and the MerkleCut of every layer its launch never stored.
void Context::enqueue_device_decommit(ProofRun& r) {
  LMN_RUN_ALIASES(r);
  const FriClose& fc = r.close;
  struct Item {
    const DevMerkle* m;
    std::vector<ColRef> cols;
    bool pairs;
  };
  std::vector<Item> its;
  its.push_back({&first_merkle, first_cols, true});
  for (auto& fl : inner) {
    Item it{&fl.merkle, {}, true};
    secure_columns(fl.vals, fl.log, fl.sharded, g, it.cols);
    its.push_back(std::move(it));
  }
  for (auto* t : trees) {
    Item it{&t->merkle, {}, false};
    for (auto& c : t->cols) it.cols.push_back({c.lde, c.log_size + lb, c.sharded});
    std::stable_sort(it.cols.begin(), it.cols.end(), [](auto& a, auto& b) { return a.log > b.log; });
    its.push_back(std::move(it));
  }
  if (its.size() > OPEN_MAX_ITEMS) return;   // (more FRI layers than a launch takes: the host plans)
  const uint32_t n_items = (uint32_t)its.size(), nq = fc.n_queries;
  std::vector<const uint32_t*> ptrs;
  std::vector<OpenItemDesc> descs(n_items);
  std::vector<MerkleRecompute> cuts;
  OpenTotals tot;
  for (uint32_t k = 0; k < n_items; ++k) {
    const DevMerkle& m = *its[k].m;
    if (m.max_log > (int)OPEN_MAX_LOG) throw LmnError(LMN_ERR_INTERNAL, "device decommit: a tree larger than the planner takes");
    std::vector<uint32_t> ncols_of_log(m.max_log + 1, 0u);
    for (auto& c : its[k].cols) {
      if (c.log < 0 || c.log > m.max_log) throw LmnError(LMN_ERR_INTERNAL, "device decommit: a column larger than its tree");
      ++ncols_of_log[c.log];
    }
    if (!append_open_item(m.max_log, m.layers.data(), ncols_of_log, its[k].cols, &m.cuts, nq, its[k].pairs ? OPEN_FRI_PAIRS : 0u,
                          ptrs, cuts, descs[k], tot))
      return;   // (more cuts than a launch takes: the host plans)
  }
  // What the plan takes beside the proof's own buffers: tables, headers and both entry tables in the arena, the tables'
  // staging, the headers' copy and the lists in page-locked memory.  Where either does not have it, the host plans.
  const size_t head_bytes = sizeof(OpenHeader) + n_items * sizeof(OpenItemHeader);
  const size_t ptr_bytes = ptrs.size() * sizeof(void*), desc_bytes = n_items * sizeof(OpenItemDesc);
  const size_t table_bytes = ptr_bytes + desc_bytes + (cuts.size() + 1) * sizeof(MerkleRecompute);
  const size_t ent_bytes = (tot.entries + 1) * sizeof(OpenEntry), job_bytes = (tot.jobs + 1) * sizeof(OpenEntry);
  // (room is left for what the proof still stages behind this point: the FRI results' download, and - should the grind
  // fall back - the host plan's own entry table and result block, which the same bound covers)
  const size_t slack = 1u << 20;
  const size_t arena_need = table_bytes + head_bytes + ent_bytes + job_bytes + slack;
  const size_t pin_need = table_bytes + head_bytes + 2 * (tot.words * 4) + tot.entries * sizeof(GatherEntry) + r.fri.out_bytes + slack;
  if (tot.words > 0xffffffffull || tot.entries > 0xffffffffull || arena_need > arena_.capacity() - arena_.used() ||
      pin_need > pin_cap_ - pin_off_)
    return;
  char* h_tab = (char*)pin_alloc(table_bytes);
  memcpy(h_tab, ptrs.data(), ptr_bytes);
  memcpy(h_tab + ptr_bytes, descs.data(), desc_bytes);
  if (!cuts.empty()) memcpy(h_tab + ptr_bytes + desc_bytes, cuts.data(), cuts.size() * sizeof(MerkleRecompute));
  char* d_tab = (char*)arena_.alloc_bytes(table_bytes);
  lmn_h2d(d_tab, h_tab, table_bytes, stream_);
  const uint32_t* const* d_ptrs = (const uint32_t* const*)d_tab;
  const OpenItemDesc* d_items = (const OpenItemDesc*)(d_tab + ptr_bytes);
  const MerkleRecompute* d_cuts = (const MerkleRecompute*)(d_tab + ptr_bytes + desc_bytes);
  OpenEntry* d_ent = (OpenEntry*)arena_.alloc_bytes(ent_bytes);
  OpenEntry* d_job = (OpenEntry*)arena_.alloc_bytes(job_bytes);
  // The headers stay in device memory, where every lane of the fetch reads them, and come back with one copy behind the
  // last launch; the lists are written straight to page-locked memory: nothing to download behind them.
  char* d_head = (char*)arena_.alloc_bytes(head_bytes);
  OpenHeader* head = (OpenHeader*)d_head;
  OpenItemHeader* heads = (OpenItemHeader*)(d_head + sizeof(OpenHeader));
  char* block = (char*)result_block(head_bytes + tot.words * 4);
  uint32_t* out = (uint32_t*)(block + head_bytes);
  const FriCloseHeader* fh = reinterpret_cast<const FriCloseHeader*>(fc.h_block);
  launch_open_plan(&fh->n_positions, fc.h_block + sizeof(FriCloseHeader) / 4, &fh->found, fc.log_query_domain, d_items, n_items,
                   heads, d_ent, d_job, stream_);
  launch_open_offsets(&fh->n_positions, head, heads, n_items, (uint32_t)tot.words, stream_);
  launch_open_fetch(d_ptrs, (uint32_t)ptrs.size(), d_items, n_items, (uint32_t)tot.max_cap, head, heads, d_ent, out, stream_);
  launch_open_recompute(d_cuts, (uint32_t)cuts.size(), d_items, n_items, (uint32_t)tot.max_job_cap, head, heads, d_job, out, stream_);
  lmn_d2h(block, d_head, head_bytes, stream_);
  r.open.on = true;
  r.open.n_items = n_items;
  r.open.h_block = block;
  r.open.head_bytes = head_bytes;
  r.open.cap_words = tot.words;
  ++dev_open_counters_[0];
}

// The host's plan: MerkleProver::decommit's walk for every tree (decommit.cpp), one gather launch, one wait.  Fills cnt per
// plan [first, inner..., tree0..3] - words of FRI witness, queried words, hashes, column witness words - and returns the
// gathered words in that order (`merged` keeps them alive for a sharded proof).
const uint32_t* Context::plan_and_gather_on_host(ProofRun& r, std::vector<std::array<size_t, 4>>& cnt, std::vector<uint32_t>& merged) {
  LMN_RUN_ALIASES(r);
  typedef DecommitPlan Plan;
  const uint32_t* gathered = nullptr;
  if (!host_scratch) host_scratch = new HostScratch();
  HostScratch& hs = *static_cast<HostScratch*>(host_scratch);
  hs.used = 0;
  hs.jobs.clear();
  hs.plans.reserve(inner.size() + 5);  // plans are handed out by reference: no reallocation while planning
  std::vector<Plan>& plans = hs.plans;  // [first, inner..., tree0..3]
  {
    Plan& p = hs.next();
    std::map<int, std::vector<uint32_t>> dec;
    for (size_t qk = 0; qk < quots.size(); ++qk) {
      const ColRef(&c4)[4] = *reinterpret_cast<const ColRef(*)[4]>(&first_cols[4 * qk]);
      plan_fri_witness(c4, g, pos_by_log[quots[qk].log], dec[quots[qk].log], p.fri_wit);
    }
    std::vector<Ref> dummy;
    plan_merkle_decommit(first_merkle, first_cols, g, dec, dummy, p.hash_wit, p.col_wit, hs.jobs);
  }
  std::vector<uint32_t> lq = fold_positions(queries, 1);
  for (auto& fl : inner) {
    Plan& p = hs.next();
    std::map<int, std::vector<uint32_t>> dec;
    std::vector<ColRef>& lc = hs.cols;
    lc.clear();
    secure_columns(fl.vals, fl.log, fl.sharded, g, lc);
    const ColRef(&c4)[4] = *reinterpret_cast<const ColRef(*)[4]>(lc.data());
    plan_fri_witness(c4, g, lq, dec[fl.log], p.fri_wit);
    std::vector<Ref> dummy;
    plan_merkle_decommit(fl.merkle, lc, g, dec, dummy, p.hash_wit, p.col_wit, hs.jobs);
    lq = fold_positions(lq, 1);
  }
  for (auto* t : trees) {
    Plan& p = hs.next();
    std::vector<ColRef>& sorted = hs.cols;
    sorted.clear();
    std::map<int, std::vector<uint32_t>> qmap;
    sorted.reserve(t->cols.size());
    for (auto& c : t->cols) {
      sorted.push_back({c.lde, c.log_size + lb, c.sharded});
      if (!qmap.count(c.log_size + lb)) qmap[c.log_size + lb] = pos_by_log[c.log_size + lb];
    }
    std::stable_sort(sorted.begin(), sorted.end(), [](auto& a, auto& b) { return a.log > b.log; });
    plan_merkle_decommit(t->merkle, sorted, g, qmap, p.queried, p.hash_wit, p.col_wit, hs.jobs);
  }
  // Every rank plans the same list; it fetches the runs it holds into its own slot of the output buffer, the
  // slots are all-gathered (a few KB per rank) and each run is then read from its owner's slot.
  std::vector<GatherEntry>& entries = hs.entries;
  entries.clear();
  std::vector<std::pair<int, uint32_t>>& runs = hs.runs;  // (owner, len) in output order
  runs.clear();
  uint32_t out_words = 0;
  const Prepared* const shared = r.prepared;
  auto add_refs = [&](const std::vector<Ref>& refs) {
    for (auto& r : refs) {
      if (r.job >= 0)
        hs.jobs[r.job].dst_off = out_words;   // unsharded proofs only: one output slot
      else if (shared && shared->holds(r.ptr))   // the prepared tree 0 lies outside the arena: its own base
        entries.push_back({GATHER_SHARED | shared->word_offset(r.ptr), r.len, out_words});
      else if (r.owner < 0 || r.owner == (int)shard_.rank)
        entries.push_back({arena_.word_offset(r.ptr), r.len, out_words});
      if (sh) runs.push_back({r.owner, r.len});
      out_words += r.len;
    }
  };
  for (size_t k = 0; k < hs.used; ++k) {
    Plan& p = plans[k];
    add_refs(p.fri_wit);
    add_refs(p.queried);
    add_refs(p.hash_wit);
    add_refs(p.col_wit);
  }
  if (out_words) {
    const uint32_t slots = sh ? shard_.world : 1u, mine = sh ? shard_.rank : 0u;
    for (auto& e : entries) e.dst_off += mine * out_words;
    // the entry table is read once, one entry per lane: the kernel takes it straight from pinned host memory
    GatherEntry* d_e = (GatherEntry*)pin_alloc((entries.size() + 1) * sizeof(GatherEntry));
    if (!entries.empty()) memcpy(d_e, entries.data(), entries.size() * sizeof(GatherEntry));
    if (!hs.jobs.empty() && sh) throw LmnError(LMN_ERR_INTERNAL, "sharded proofs keep whole trees");
    MerkleRecompute* d_j = (MerkleRecompute*)pin_alloc((hs.jobs.size() + 1) * sizeof(MerkleRecompute));
    if (!hs.jobs.empty()) memcpy(d_j, hs.jobs.data(), hs.jobs.size() * sizeof(MerkleRecompute));   // (memcpy from a null vector: UB even for 0 bytes)
    // an unsharded proof's gather writes straight to page-locked memory: nothing to download behind it
    uint32_t* d_o = sh ? arena_.alloc_words((size_t)slots * out_words) : (uint32_t*)result_block((size_t)out_words * 4);
    hm.mark("decommit planned");
    if (hm.on) fprintf(stderr, "[host] decommit: %zu runs gathered, %zu tree nodes recomputed\n", entries.size(), hs.jobs.size());
    launch_gather(arena_.base_words(), shared ? shared->base_words() : nullptr, d_e, (uint32_t)entries.size(), d_j, (uint32_t)hs.jobs.size(), d_o, stream_);
    if (sh) gather_columns(d_o, 0, 1, out_words);
    gathered = sh ? (const uint32_t*)stage_download(d_o, (size_t)slots * out_words * 4) : d_o;
    lmn_sync(stream_);
    hm.mark("gathered");
    if (sh) {
      merged.resize(out_words);
      uint32_t at = 0;
      for (auto& r : runs) {
        const uint32_t slot = r.first < 0 ? mine : (uint32_t)r.first;
        memcpy(&merged[at], gathered + (size_t)slot * out_words + at, (size_t)r.second * 4);
        at += r.second;
      }
      gathered = merged.data();
    }
  }
  for (size_t k = 0; k < hs.used; ++k)
    cnt.push_back({plans[k].fri_wit.size(), plans[k].queried.size(), plans[k].hash_wit.size(), plans[k].col_wit.size()});
  return gathered;
}

void Context::run_decommit(ProofRun& r) {
  LMN_RUN_ALIASES(r);
  // ---- decommitment: plan device references, gather once, distribute
  {
    StageTimer st(this, log, stream_, C_DECOMMIT);
    // per plan [first, inner..., tree0..3]: words of FRI witness, queried words, hashes, column witness words
    std::vector<std::array<size_t, 4>> cnt;
    const uint32_t* gathered = nullptr;
    std::vector<uint32_t> merged;
    // planned and fetched on the device, in front of the wait that has passed (enqueue_device_decommit) - unless the queued
    // grind windows held no nonce: then nothing behind the grind ran, and the host plans as it always did
    const bool dev_plan = r.open.on && r.close.found;
    if (r.open.on && !r.close.found) ++dev_open_counters_[1];
    if (dev_plan) {
      const OpenHeader& head = *(const OpenHeader*)r.open.h_block;
      const OpenItemHeader* heads = (const OpenItemHeader*)(r.open.h_block + sizeof(OpenHeader));
      if (head.overflow || r.open.n_items != inner.size() + 5)
        throw LmnError(LMN_ERR_INTERNAL, "device decommit: the plan exceeded the bounds it was launched with");
      uint64_t at = 0, n_entries = 0, n_jobs = 0;
      for (uint32_t k = 0; k < r.open.n_items; ++k) {
        const OpenItemHeader& h = heads[k];
        for (int l = 0; l < 4; ++l) {
          if (h.base[l] != at) throw LmnError(LMN_ERR_INTERNAL, "device decommit: the lists are not compact");
          at += (uint64_t)h.count[l] * (l == OPEN_LIST_HASH ? 8 : 1);
        }
        if (h.count[OPEN_LIST_FRI] % 4) throw LmnError(LMN_ERR_INTERNAL, "device decommit: a partial FRI witness");
        cnt.push_back({h.count[OPEN_LIST_FRI], h.count[OPEN_LIST_QUERIED], h.count[OPEN_LIST_HASH], h.count[OPEN_LIST_WITNESS]});
        n_entries += h.n_entries;
        n_jobs += h.n_jobs;
      }
      if (at > r.open.cap_words) throw LmnError(LMN_ERR_INTERNAL, "device decommit: the counts exceed the result block");
      gathered = (const uint32_t*)(r.open.h_block + r.open.head_bytes);
      hm.mark("decommit sliced (device plan)");
      if (hm.on)
        fprintf(stderr, "[host] decommit: device plan, %llu entries fetched, %llu tree nodes recomputed\n",
                (unsigned long long)n_entries, (unsigned long long)n_jobs);
    } else {
      gathered = plan_and_gather_on_host(r, cnt, merged);
    }
    size_t g = 0;
    // (runs behind the proof's last wait: whole runs are copied, not words)
    auto take_q = [&](size_t nrefs) {
      const QM31* b = reinterpret_cast<const QM31*>(gathered + g);
      g += nrefs / 4 * 4;
      return std::vector<QM31>(b, b + nrefs / 4);
    };
    auto take_u32 = [&](size_t n) {
      std::vector<uint32_t> v(gathered + g, gathered + g + n);
      g += n;
      return v;
    };
    auto skip = [&](size_t n) { g += n; };
    auto take_hashes = [&](size_t n) {
      const Hash32* b = reinterpret_cast<const Hash32*>(gathered + g);
      g += 8 * n;
      return std::vector<Hash32>(b, b + n);
    };
    size_t pi = 0;
    auto fill_layer = [&](FriLayerProof& lp, const Hash32& root) {
      const std::array<size_t, 4>& p = cnt[pi++];
      lp.fri_witness = take_q(p[0]);
      skip(p[1]);
      lp.decommitment.hash_witness = take_hashes(p[2]);
      lp.decommitment.column_witness = take_u32(p[3]);
      lp.commitment = root;
    };
    fill_layer(proof.first_layer, first_merkle.root);
    proof.inner_layers.resize(inner.size());
    for (size_t i = 0; i < inner.size(); ++i) fill_layer(proof.inner_layers[i], inner[i].merkle.root);
    for (int t = 0; t < 4; ++t) {
      const std::array<size_t, 4>& p = cnt[pi++];
      skip(p[0]);
      proof.queried_values.push_back(take_u32(p[1]));
      Decommitment d;
      d.hash_witness = take_hashes(p[2]);
      d.column_witness = take_u32(p[3]);
      proof.decommitments.push_back(d);
    }
  }
  hm.mark("decommit done");
  r.total_guard.reset();
  lmn_sync(stream_);
}

}  // namespace lmn
