// prove(), phases 0 and 1: the preprocessed tree (LUT columns, /root/reference/crates/prover/src/prover.rs:54-59) and the
// main trace - pad + AoS -> SoA, interpolate, extend, commit (prover.rs:70-179; add/witness.rs:33-108).
#include "prove_run.h"

namespace lmn {

void Context::run_preprocessed(ProofRun& r) {
  LMN_RUN_ALIASES(r);
  const lmn_settings* settings = r.settings;
  // ---- PHASE 0: preprocessed trace (prover.rs:54-59): empty tree (root = blake2s("")) unless a lookup
  // component is present.  Columns in PreProcessedTrace order (preprocessed.rs:157-179: sin, exp2, log2
  // LUT pairs from the settings, then the 8-bit range check whose row r holds r), stable-sorted by size
  // descending (PreProcessedTrace::new).
  for (auto& ti : infos) {
    Instance ci{};
    ci.spec = ti.spec;
    ci.log_size = ti.log_size;
    inst.push_back(ci);
  }
  if (r.prepared) {
    // Settings prepared once: tree 0 - columns, coefficients, LDE, Merkle layers, root - is the prepared object's, shared
    // read-only with every other proof that uses it.  Nothing is checked on the host, uploaded, transformed or hashed, and
    // the host does not wait: the root is known.
    const Prepared& pp = *r.prepared;
    const uint32_t present = lookups_present(infos);
    if (present & ~pp.lookups)
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, "the pie holds a lookup table the settings were not prepared for");
    if (pp.lookups & ~present)
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, "the settings were prepared for a lookup whose table is not in the pie");
    lmn_lut sized[3] = {};   // the prepared LUTs as lut_for_table reads them: their sizes (the columns are the object's)
    Luts luts;
    for (int k = 0; k < 3; ++k)
      if (pp.log_of_pre[2 * k] >= 0) {
        sized[k].log_size = (uint32_t)pp.log_of_pre[2 * k];
        luts.of[k] = &sized[k];
      }
    for (size_t t = 0; t < inst.size(); ++t) lut_for_table(t, *inst[t].spec, inst[t].log_size, luts, Refusal{});
    // (the same components of the same sizes: the same tree-0 order as the prepared object's)
    const std::vector<int> logs = assign_preprocessed(inst);
    if (logs.size() != pp.tree.cols.size()) throw LmnError(LMN_ERR_INTERNAL, "prepared settings: tree-0 layout differs");
    tree0.cols = pp.tree.cols;
    tree0.merkle = pp.tree.merkle;
    pre_evals = pp.evals;
    channel.mix_root(tree0.merkle.root);
    return;
  }
  {
    const Luts luts = luts_for_pie(settings, infos);
    std::vector<int> logs = assign_preprocessed(inst);
    tree0.cols.resize(logs.size());
    pre_evals.resize(logs.size(), nullptr);
    for (size_t t = 0; t < inst.size(); ++t) {
      Instance& ci = inst[t];
      const ComponentSpec* sp = ci.spec;
      const lmn_lut* l = lut_for_table(t, *sp, ci.log_size, luts, Refusal{});
      for (int k = 0; k < sp->n_pre; ++k) {
        const uint64_t n = 1ull << ci.log_size;
        uint32_t* evals;
        if (sp->pre_id[k] == PRE_RANGE_CHECK) {
          std::vector<uint32_t> lut(n);
          for (uint32_t r = 0; r < n; ++r) lut[r] = r;
          evals = upload_vec(lut);
        } else {
          const uint32_t* src = (sp->pre_id[k] & 1) ? l->col1 : l->col0;
          if (first_noncanonical(src, n) < n) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "LUT value is not a canonical M31");
          evals = arena_.alloc_words(n);
          lmn_h2d(evals, src, n * 4, stream_);
        }
        uint32_t* coeffs = arena_.alloc_words(n);
        launch_ifft(coeffs, n, evals, n, 1, ci.log_size, itw(ci.log_size), stream_);
        tree0.cols[ci.pre_idx[k]] = {ci.log_size, coeffs, nullptr};
        pre_evals[ci.pre_idx[k]] = evals;
      }
    }
    if (!tree0.cols.empty()) {
      lde_and_merkle(tree0);
      lmn_sync(stream_);
      tree0.merkle.finish_root();
    } else {
      build_merkle(tree0.merkle, {});
    }
  }
  channel.mix_root(tree0.merkle.root);
}

// ---- lmn_settings_prepare: PHASE 0 of every proof of one circuit, done once.  Runs on the private context of `out`
// (own stream, own arena: reserved here and never reset or grown, so the object's pointers stay valid for its lifetime).
Prepared::Prepared(int device_, const lmn_config& cfg, const lmn_settings* settings, uint32_t lookups_) {
  for (int& l : log_of_pre) l = -1;
  ctx_ = new Context(device_, cfg, 1u << 20);
  try {
    ctx_->build_prepared(*this, settings, lookups_);
  } catch (...) {
    delete ctx_;
    ctx_ = nullptr;
    throw;
  }
}
Prepared::~Prepared() { delete ctx_; }

void Context::build_prepared(Prepared& out, const lmn_settings* settings, uint32_t lookups) {
#ifndef LMN_EMU
  LMN_HIP_CHECK(hipSetDevice(device_));
#endif
  const int lb = (int)cfg.log_blowup;
  out.device = device_;
  out.lookups = lookups;
  out.log_blowup = cfg.log_blowup;
  if (lookups & ~(LMN_LOOKUP_SIN | LMN_LOOKUP_EXP2 | LMN_LOOKUP_LOG2 | LMN_LOOKUP_RANGE_CHECK))
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "lmn_settings_prepare: unknown bits in `lookups`");
  const Luts luts = parse_luts(settings);
  for (const lmn_lut* l : luts.of)
    // the bounds scan_tables puts on the lookup table that will have the LUT's size
    if (l && (l->log_size < 4 || l->log_size > 26 || (int)l->log_size + lb + 2 > MAX_LOG - 2))
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, "LUT log_size " + std::to_string(l->log_size) +
                                                   " is outside what the prover takes (at least 4, and at most what a trace table may have)");
  static const char* const kLookupName[3] = {"sin", "exp2", "log2"};
  std::vector<Instance> inst;   // the lookup components of the pies to come, in the order of a pie's tables (ascending kind)
  for (int k = 0; k < 4; ++k) {
    if (!(lookups & kLookupKinds[k].bit)) continue;
    Instance ci{};
    ci.spec = component_spec(kLookupKinds[k].kind);
    // the rows its table will have - the LUT's, the range check's 256 - so of the table's rules only the LUT's presence can fail
    ci.log_size = k < 3 && luts.of[k] ? (int)luts.of[k]->log_size : 8;
    lut_for_table(inst.size(), *ci.spec, ci.log_size, luts, Refusal{});
    inst.push_back(ci);
  }
  const std::vector<int> logs = assign_preprocessed(inst);
  if (logs.empty()) {
    build_merkle(out.tree.merkle, {});   // root = blake2s("")
    return;
  }
  size_t words = 1u << 18;   // the flag word, alignment, a scattered level's pointer table
  for (int lg : logs) words += (2ull << lg) + (1ull << (lg + lb));           // evals + coeffs + lde
  words += 16ull << (logs[0] + lb);                                          // every Merkle layer: 2 x 2^max_log nodes of 8 words
  ensure_twiddles(logs[0] + lb);
  arena_.reserve(words * 4);
  arena_.reset();
  pin_off_ = 0;
  out.base_ = arena_.base_words();
  out.bytes_ = arena_.capacity();
  uint32_t* flag = arena_.alloc_words(1);
  lmn_memset(flag, 0, 4, stream_);
  out.tree.cols.resize(logs.size());
  out.evals.assign(logs.size(), nullptr);
  PrepareCols pc{};
  int pc_col[PREPARE_MAX_LUT_COLS] = {0};   // PRE_* id of each LUT column handed to the check
  for (auto& ci : inst)
    for (int k = 0; k < ci.spec->n_pre; ++k) {
      const uint64_t n = 1ull << ci.log_size;
      const int id = ci.spec->pre_id[k];
      uint32_t* evals = arena_.alloc_words(n);
      if (id == PRE_RANGE_CHECK) {
        pc.range_check = evals;
        pc.range_n = (uint32_t)n;
      } else {
        const lmn_lut* l = luts.of[id / 2];
        lmn_h2d(evals, (id & 1) ? l->col1 : l->col0, n * 4, stream_);
        pc_col[pc.n_luts] = id;
        pc.lut[pc.n_luts] = evals;
        pc.n[pc.n_luts++] = (uint32_t)n;
      }
      out.log_of_pre[id] = ci.log_size;
      out.evals[ci.pre_idx[k]] = evals;
    }
  launch_settings_prepare(pc, flag, stream_);
  for (auto& ci : inst)
    for (int k = 0; k < ci.spec->n_pre; ++k) {
      const uint64_t n = 1ull << ci.log_size;
      uint32_t* coeffs = arena_.alloc_words(n);
      launch_ifft(coeffs, n, out.evals[ci.pre_idx[k]], n, 1, ci.log_size, itw(ci.log_size), stream_);
      out.tree.cols[ci.pre_idx[k]] = {ci.log_size, coeffs, nullptr};
    }
  lde_and_merkle(out.tree);
  const uint32_t* h_flag = (const uint32_t*)stage_download(flag, 4);
  lmn_sync(stream_);   // the one wait: later proofs, on whatever stream, start after it
  out.tree.merkle.finish_root();
  if (*h_flag) {
    const int id = pc_col[std::min<uint32_t>(*h_flag, (uint32_t)pc.n_luts) - 1];
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, std::string("LUT value is not a canonical M31 (") + kLookupName[id / 2] + "_lut_" +
                                                 std::to_string(id & 1) + ")");
  }
}

// Trace reuse, the accounting: `changed_words` = the comparing transposes' words as they came back with the verdict.  A
// candidate column whose word is not this proof's mark was skipped by all three of its transform launches; the counters and
// the timings' bytes and butterflies then say what ran (bench.py's roofline divides them by the measured time).  Both
// counters, the correction and the back-off's count move here, together: a proof that throws in front of its report has
// moved none of them.
// Under LMN_COMP_FULL_DOMAIN=1 the timings are left as interpolate_for_commit counted them: that switch exists for A/B runs
// of the composition, which compare fft_butterflies of two proofs of one context (tests/comp_half_checks.py) - the columns
// reuse skipped would otherwise be the larger part of the difference.
void Context::account_trace_reuse(ProofRun& r, const uint32_t* changed_words) {
  const bool correct_timings = env_int("LMN_COMP_FULL_DOMAIN", 0) == 0;
  for (const ProofRun::ReuseTable& t : r.reuse_tables) {
    uint64_t skipped = 0;
    for (int c = 0; c < 32; ++c)
      if (((t.candidate_mask >> c) & 1u) && changed_words[t.first_word + c] != r.bad_mark) ++skipped;
    reuse_counters_[0] += (uint64_t)__builtin_popcount(t.candidate_mask);
    reuse_counters_[1] += skipped;
    if (t.table < reuse_.tables.size()) {   // the back-off's count (TraceReuse::Table::misses)
      int& misses = reuse_.tables[t.table].misses;
      misses = skipped == 0 ? misses + 1 : 0;
    }
    if (!correct_timings) continue;
    const uint64_t n = 1ull << t.log_size;
    timings.fft_bytes -= skipped * 20ull * n;                                   // as interpolate_for_commit counted them
    timings.fft_butterflies -= skipped * (n / 2 + n) * (uint64_t)t.log_size;
  }
  r.reuse_tables.clear();
}

void Context::run_main_trace(ProofRun& r) {
  LMN_RUN_ALIASES(r);
  // ---- PHASE 1: main trace (prover.rs:70-179)
  // Persistent device word the transposes write when a table holds a word that is not a canonical M31.  Unsharded proofs
  // never reset it: every proof has its own mark (>= 2) and only that value counts, so the accepting and the rejecting
  // path issue the same launches / copies / waits - what the lock-step batch library needs from its members (a
  // rejected pie leaves its batch alone and the slot stays usable).  Sharded proofs gather the word across ranks, whose
  // counters are unrelated: their mark is 1 and the rejecting path clears it.
  uint32_t* d_bad = bad_flag_;
  if (++bad_epoch_ < 2u) bad_epoch_ = 2u;
  const uint32_t bad_mark = shard_.active ? 1u : bad_epoch_;
  const uint32_t* h_bad = nullptr;
  bool any_rows_front = false;
  // ---- Trace reuse (LMN_TRACE_REUSE, on by default; docs/SWITCHES.md).  One model is proved on many inputs: the id, index,
  // successor and multiplicity columns of a table are functions of the graph alone (constraints.h graph_only_columns) and
  // bit-identical from one proof of a context to the next, and the arena still holds the previous proof's evaluation,
  // coefficient and LDE blocks at the addresses this proof gets (Context::TraceReuse).  The transpose compares those
  // columns with what it is about to overwrite, word for word, and the three transform launches skip the ones that did not
  // change.  Off for sharded proofs, the lock-step batch library, row sinks read in place, LMN_ROWS_FUSION, log_blowup != 1
  // and sizes without the three-launch form.
#ifdef LMN_BATCH
  const bool reuse_cfg = false;
#else
  const bool reuse_cfg = env_int("LMN_TRACE_REUSE", 1) != 0 && !shard_.active && lb == 1 && env_int("LMN_ROWS_FUSION", 0) == 0;
#endif
  const bool reuse_live = reuse_.live && reuse_cfg;   // (validity was cleared when run_setup formed `live`)
  reuse_.live = false;
  std::vector<TraceReuse::Table> now(infos.size(), TraceReuse::Table{-1, 0, 0, 0, nullptr, nullptr, nullptr, 0});
  struct Compared {
    bool on = false;
    uint32_t first_word = 0, mask = 0;
  };
  std::vector<Compared> compared(infos.size());
  uint32_t* const d_changed = bad_flag_ + 2;
  uint32_t changed_words = 0;
  {
    StageTimer st(this, log, stream_, C_TRANSPOSE);
    for (size_t t = 0; t < infos.size(); ++t) {
      auto& ti = infos[t];
      uint64_t n = 1ull << ti.log_size;
      const bool rows_front = shard_rows_front(ti.log_size);
      // row-parallel front end of a sharded proof: only this rank's block of the (padded) rows is transposed - and, for
      // host tables, uploaded
      const uint64_t nb = rows_front ? n >> shard_.g : n, blk0 = rows_front ? (uint64_t)shard_.rank * nb : 0;
      const uint64_t up0 = std::min<uint64_t>(blk0, ti.n_rows), up1 = std::min<uint64_t>(blk0 + nb, ti.n_rows);
      if (ti.cols_on_device) {
        // a finished row sink (lmn_rows_finish): padded, checked and column-major already, and only read from here on -
        // no upload, no transpose launch, no copy into the arena
        inst[t].trace_evals = const_cast<uint32_t*>(ti.rows);
        inst[t].rows_n = ti.n_rows;
        proof.claim[ti.spec->kind] = ti.log_size;
        continue;
      }
      const uint32_t* d_rows = ti.rows;
      if (!ti.on_device) {
        uint32_t* stg = arena_.alloc_words(std::max<uint64_t>(up1 - up0, 1) * ti.spec->n_cols);
        if (up1 > up0) lmn_h2d(stg, ti.rows + up0 * ti.spec->n_cols, (up1 - up0) * ti.spec->n_cols * 4, stream_);
        d_rows = stg - up0 * ti.spec->n_cols;   // indexed by table row: only rows [up0, up1) are ever read
      }
      const PadRow pad = pad_row_of(*ti.spec);
      inst[t].rows_dev = d_rows;
      inst[t].rows_n = ti.n_rows;
      inst[t].pad = pad;
      // LMN_ROWS_FUSION=1 (a switch, off by default): big unsharded tables get no transpose launch - the first pass of the
      // interpolation reads the rows itself (fft_fixed.hip k_fft_rows_fx) and nothing is stored column-major before it;
      // logup fractions then read the table's rows.  Measured (docs/HISTORY.md, round 6): skipping the transpose outright is
      // worth 5 % proofs/s, but the pass that absorbs it costs what the two launches cost (54 us against 27 + 27 solo;
      // +0.4 % under load: inside the noise) - byte-identical proofs, kept for the next idea.  Components with
      // preprocessed (LUT) columns keep the plain path; LMN_ROWS_FUSION_MIN_LOG (default 18) lowers the size threshold.
      const bool try_fused = env_int("LMN_ROWS_FUSION", 0) != 0 && !shard_.active && lb == 1 && ti.spec->n_pre == 0 &&
                             fft_interp_extend_supported(ti.log_size) &&
                             ti.log_size >= std::max(13, env_int("LMN_ROWS_FUSION_MIN_LOG", 18)) && !env_set("LMN_NO_FFT_FIXED");
      if (try_fused) {
        inst[t].trace_evals = nullptr;
      } else {
        uint32_t* evals = arena_.alloc_words((size_t)ti.spec->n_cols * nb);
        // Only the graph's columns are compared.  A value column (lhs, rhs, out, ...) is transformed in every proof, even
        // where it repeats - a benchmark proves the same buffers again and again, a service never sees the same input twice -
        // so what reuse gains in a benchmark is what it gains in real use.
        const uint32_t mask = graph_only_columns(*ti.spec);
        const bool table_ok = reuse_cfg && mask != 0u && !rows_front && fft_interp_extend_supported(ti.log_size);
        if (table_ok) now[t] = {ti.spec->kind, ti.log_size, ti.spec->n_cols, ti.n_rows, evals, nullptr, nullptr, 0};
        const TraceReuse::Table* prev = reuse_live && t < reuse_.tables.size() ? &reuse_.tables[t] : nullptr;
        const bool same_table = table_ok && prev && prev->kind == ti.spec->kind && prev->log_size == ti.log_size &&
                                prev->n_cols == ti.spec->n_cols && prev->n_rows == ti.n_rows && prev->evals == evals;
        // back-off (TraceReuse::Table::misses): a backed-off table counts its proofs on and is compared again every
        // REUSE_RETRY-th of them - a context that has settled on one graph after several finds its way back
        const bool backed_off = same_table && prev->misses >= TraceReuse::REUSE_BACKOFF && prev->misses % TraceReuse::REUSE_RETRY != 0;
        if (same_table) now[t].misses = !backed_off ? prev->misses
                                        : prev->misses < 2 * TraceReuse::REUSE_RETRY ? prev->misses + 1
                                                                                     : prev->misses + 1 - TraceReuse::REUSE_RETRY;
        if (same_table && !backed_off && changed_words + (uint32_t)ti.spec->n_cols <= (uint32_t)CHANGED_WORDS) {
          compared[t].on = true;
          compared[t].first_word = changed_words;
          compared[t].mask = mask;
          changed_words += (uint32_t)ti.spec->n_cols;
          launch_transpose_pad_compare(d_rows, ti.n_rows, ti.spec->n_cols, ti.log_size, evals, pad, d_bad, bad_mark, mask,
                                       d_changed + compared[t].first_word, bad_mark, stream_);
        } else {
          launch_transpose_pad_rows(d_rows, ti.n_rows, ti.spec->n_cols, ti.log_size, evals, nb, blk0, nb, pad, d_bad, stream_, bad_mark);
        }
        inst[t].trace_evals = evals;
      }
      inst[t].rows_sharded = rows_front;
      any_rows_front = any_rows_front || rows_front;
      proof.claim[ti.spec->kind] = ti.log_size;
    }
  }
  {
    StageTimer st(this, log, stream_, C_MAIN_COMMIT);
    int off = 0;
    for (size_t t = 0; t < inst.size(); ++t) {
      Instance& ci = inst[t];
      uint64_t n = 1ull << ci.log_size;
      int nc = ci.spec->n_cols;
      uint32_t* coeffs = arena_.alloc_words((size_t)nc * n);
      CommitOut co;
      bool fused = false;
      if (!ci.trace_evals) {
        uint32_t* lde = arena_.alloc_words((size_t)nc * 2 * n);
        {
          StageTimer t(this, log, stream_, C_FFT);
          fused = launch_interp_extend_rows(coeffs, n, ci.rows_dev, ci.rows_n, ci.pad, d_bad, bad_mark, lde, 2 * n, nc, ci.log_size,
                                            itw(ci.log_size), tw(ci.log_size + 1), stream_);
        }
        if (fused) {
          timings.fft_launches += 3;
          timings.fft_bytes += (uint64_t)nc * 20ull * n;                         // as interpolate_for_commit counts the two transforms
          timings.fft_butterflies += (uint64_t)nc * (n / 2) * (uint64_t)ci.log_size + (uint64_t)nc * n * (uint64_t)ci.log_size;
          co.lde = lde;
          co.stride = 2 * n;
        } else {
          throw LmnError(LMN_ERR_INTERNAL, "main trace: no row pass for a size run_main_trace had chosen it for");
        }
      }
      if (!fused) {
        // the skip argument only where all three blocks lie where the previous proof left them; anything else: every column
        ColSkip skip{};
        const uint32_t* prev_lde = nullptr;
        if (compared[t].on && reuse_.tables[t].coeffs == coeffs) {
          skip = ColSkip{d_changed + compared[t].first_word, bad_mark, compared[t].mask};
          prev_lde = reuse_.tables[t].lde;
        }
        co = interpolate_for_commit(coeffs, ci.trace_evals, nc, ci.log_size, -1, ci.rows_sharded, skip.changed ? &skip : nullptr, prev_lde);
        if (co.skipped) {
          r.reuse_tables.push_back({compared[t].first_word, compared[t].mask, ci.log_size, t});
        }
        if (now[t].kind >= 0) {
          now[t].coeffs = coeffs;
          now[t].lde = co.lde;
        }
      }
      ci.main_start = off;
      off += nc;
      for (int c = 0; c < nc; ++c)
        tree1.cols.push_back({ci.log_size, coeffs + (uint64_t)c * n, co.lde ? co.lde + (uint64_t)c * co.stride : nullptr,
                              co.sharded, co.owner_of(c)});
    }
    // the last trace launch is enqueued: the record stands for the next proof (a proof that throws later leaves consistent
    // blocks - the stream still runs what was queued; one that threw above has left the record invalid)
    reuse_.tables = std::move(now);
    reuse_.valid = reuse_cfg;
    for (int k = 0; k < n_slots; ++k)  // LuminairClaim::mix_into (crates/air/src/lib.rs:52-104)
      if (proof.claim[k] >= 0) channel.mix_u64((uint64_t)proof.claim[k]);
    r.bad_mark = bad_mark;
    if (r.dev_fs) {
      // no wait: the launch that produces the root also mixes it and draws the relation elements (ChanStep kind 1); the
      // host replays the step in run_oods, where the non-canonical-word verdict is read as well
      r.d_chan = (DevChannel*)arena_.alloc_bytes(sizeof(DevChannel));
      r.d_report = (DevReport*)arena_.alloc_bytes(sizeof(DevReport));
      ChanStep step{};
      step.kind = 1;
      memcpy(step.start.digest, channel.digest().w, 32);
      step.start.n_sent = 0;
      step.start.variant = (cfg.protocol_variant & LMN_PV_DRAW_CTR_U32) ? 1u : 0u;
      step.bad_word = d_bad;
      step.changed_words = changed_words;   // the comparing transposes' marks come back with the verdict: no wait of their own
      int sets[CHAN_N_ELEMS];
      const int n_draws = relation_draw_sets(cfg.protocol_variant, sets);
      if (n_draws < 1 || n_draws > CHAN_N_ELEMS) throw LmnError(LMN_ERR_INTERNAL, "relation draws: bad count");
      step.sets.n = n_draws;
      for (int i = 0; i < n_draws; ++i) step.sets.set[i] = sets[i];
      step.rep = r.d_report;
      lde_and_merkle(tree1, false, r.d_chan, &step);
      for (int i = 0; i < n_draws; ++i)
        if (sets[i] >= 0) elems.drawn[sets[i]] = true;
      hm.mark("main trace enqueued (device transcript)");
      return;
    }
    lde_and_merkle(tree1);
    uint32_t n_flags = 1;
    if (any_rows_front) {   // every rank has only looked at its own rows: the ranks must agree on the verdict
      n_flags = shard_.world;
      uint32_t* flags = arena_.alloc_words(n_flags);
      lmn_d2d(flags + shard_.rank, d_bad, 4, stream_);
      gather_columns(flags, 0, 1, 1);
      h_bad = (const uint32_t*)stage_download(flags, 4 * n_flags);
    } else {
      h_bad = (const uint32_t*)stage_download(d_bad, 4 * (2 + (size_t)changed_words));
    }
    lmn_sync(stream_);
    if (!any_rows_front) account_trace_reuse(r, h_bad + 2);
    bool bad_any = false;
    for (uint32_t k = 0; k < n_flags; ++k) bad_any = bad_any || h_bad[k] == bad_mark;
    if (bad_any) {
      if (shard_.active) {
        const uint32_t zero = 0u;
        lmn_h2d(d_bad, &zero, 4, stream_);
        lmn_sync(stream_);
      }
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, "trace table holds a word that is not a canonical M31 (>= 2^31-1)");
    }
    tree1.merkle.finish_root();
    channel.mix_root(tree1.merkle.root);
  }
  hm.mark("sync1: root1 mixed");
}

}  // namespace lmn
