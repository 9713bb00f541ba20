// prove(): MI355X replacement for /root/reference/crates/prover/src/prover.rs:28-319.
// The Fiat-Shamir channel, proof assembly and (tiny) decommitment bookkeeping run on the host;
// every per-row / per-coefficient pass runs in the gfx950 kernels on trace data
// that stays resident in HBM from the first transpose to the last query gather.
#include "prove_run.h"

#include <exception>

namespace lmn {

// ------------------------------------------------------------------------------------ the prover's input rules
void Refusal::operator()(size_t t, int code, const std::string& why) const {
  if (!named) throw LmnError(code, why);
  throw LmnError(code, "table " + std::to_string(t) + " (kind " + std::to_string(named[t].kind) + "): " + why);
}

int scan_tables(const lmn_table* tables, size_t n_tables, const lmn_config& cfg, bool sharded, int device, lmn_stream_t stream,
                const Refusal& refuse, std::vector<TableInfo>& infos) {
  const int n_slots = claim_slots(cfg.protocol_variant), lb = (int)cfg.log_blowup;
  int max_log = 0, prev_kind = -1;
  for (size_t t = 0; t < n_tables; ++t) {
    const lmn_table& tb = tables[t];
    const ComponentSpec* sp = component_spec((int)tb.kind);
    if (!sp) refuse(t, LMN_ERR_INVALID_ARGUMENT, "unsupported component kind " + std::to_string(tb.kind));
    if ((int)tb.kind >= n_slots) refuse(t, LMN_ERR_INVALID_ARGUMENT, "component kind has no claim slot in this protocol variant");
    if ((int)tb.kind <= prev_kind)
      refuse(t, LMN_ERR_INVALID_ARGUMENT, "tables must be in gen_trace order (ascending kind, no duplicates)");
    prev_kind = (int)tb.kind;
    if (tb.n_rows == 0) refuse(t, LMN_ERR_EMPTY_TRACE, "TraceError::EmptyTrace");
    if (!tb.rows) refuse(t, LMN_ERR_INVALID_ARGUMENT, "null rows pointer");
    if (tb.n_rows > (1ull << 26)) refuse(t, LMN_ERR_INVALID_ARGUMENT, "trace table has more than 2^26 rows");
    const int ls = padded_log(tb.n_rows);
    if (ls + lb + 2 > MAX_LOG - 2) refuse(t, LMN_ERR_INVALID_ARGUMENT, "trace too large");
    // A column of 2^(ls + lb) evaluations joins the FRI line layer of 2^(ls + lb - 1); stwo's commit loop ends at the
    // last layer of 2^(log_last_layer + lb) values and asserts that every column has been consumed by then: a table
    // of 2^log_last_layer rows or fewer cannot be proved under this PcsConfig (the reference panics)
    if (ls <= (int)cfg.log_last_layer)
      refuse(t, LMN_ERR_INVALID_ARGUMENT, "a table needs more than 2^log_last_layer rows (after padding)");
    const bool cols = (tb.flags & LMN_TABLE_COLS_ON_DEVICE) != 0;
    if (cols) {
      if (tb.flags & LMN_TABLE_ROWS_ON_DEVICE)
        refuse(t, LMN_ERR_INVALID_ARGUMENT, "a table is LMN_TABLE_ROWS_ON_DEVICE or LMN_TABLE_COLS_ON_DEVICE, not both");
#ifdef LMN_BATCH
      refuse(t, LMN_ERR_INVALID_ARGUMENT, "LMN_TABLE_COLS_ON_DEVICE (row sinks) is not supported by the batch library");
#else
      if (sharded)
        refuse(t, LMN_ERR_INVALID_ARGUMENT, "LMN_TABLE_COLS_ON_DEVICE (row sinks) is not supported on a sharded context");
      try {
        rows_sink_attach(tb, device, stream);   // the stream waits for the sink's finish event; the host does not
      } catch (const LmnError& e) {
        refuse(t, e.code, e.what());
      }
#endif
    }
    infos.push_back({sp, tb.n_rows, ls, tb.rows, (tb.flags & LMN_TABLE_ROWS_ON_DEVICE) != 0, cols});
    max_log = std::max(max_log, ls);
  }
  return max_log;
}

uint32_t lookups_present(const std::vector<TableInfo>& infos) {
  uint32_t present = 0;
  for (const TableInfo& ti : infos)
    for (const LookupKind& lk : kLookupKinds)
      if (ti.spec->kind == lk.kind) present |= lk.bit;
  return present;
}

Luts parse_luts(const lmn_settings* settings) {
  Luts luts;
  if (!settings || !settings->n_luts) return luts;
  require_luts_pointer(*settings);
  for (uint32_t i = 0; i < settings->n_luts; ++i) {
    const lmn_lut& l = settings->luts[i];
    if (l.kind > LMN_LUT_LOG2 || !l.col0 || !l.col1 || luts.of[l.kind])
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, "bad or duplicate LUT in settings (unknown kind, null column, or a kind given twice)");
    luts.of[l.kind] = &l;
  }
  return luts;
}

Luts luts_for_pie(const lmn_settings* settings, const std::vector<TableInfo>& infos) {
  if (settings && (settings->has_lookups & ~lookups_present(infos)))
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "settings announce a lookup whose table is not in the pie");
  return parse_luts(settings);
}

const lmn_lut* lut_for_table(size_t t, const ComponentSpec& spec, int log_size, const Luts& luts, const Refusal& refuse) {
  if (spec.n_pre == 0) return nullptr;
  if (spec.pre_id[0] == PRE_RANGE_CHECK) {
    if (log_size != 8) refuse(t, LMN_ERR_INVALID_ARGUMENT, "RangeCheckLookup table must have exactly 256 rows");
    return nullptr;
  }
  const lmn_lut* l = luts.of[spec.pre_id[0] / 2];
  if (!l) refuse(t, LMN_ERR_INVALID_ARGUMENT, "lookup table present but settings carry no LUT columns for it");
  if ((int)l->log_size != log_size) refuse(t, LMN_ERR_INVALID_ARGUMENT, "lookup table rows must match the LUT column size");
  return l;
}

uint64_t first_noncanonical(const uint32_t* words, uint64_t n) {
  uint64_t i = 0;
  while (i < n && words[i] < P31) ++i;
  return i;
}

#ifdef LMN_BATCH
void Context::prepare_for(const lmn_table* tables, size_t n_tables) {
  LMN_HIP_CHECK(hipSetDevice(device_));
  if (!tables) return;
  int max_log = 0;
  for (size_t t = 0; t < n_tables; ++t) {
    if (tables[t].n_rows == 0 || tables[t].n_rows > (1ull << 26)) return;
    max_log = std::max(max_log, padded_log(tables[t].n_rows));
  }
  const int max_lde = max_log + 1 + (int)cfg.log_blowup;
  if (max_lde > MAX_LOG - 2) return;
  ensure_twiddles(max_lde);
}
#endif

// ------------------------------------------------------------------------------------ prove
// The phases of one proof, in transcript order; each is a Context member in the file named.
std::vector<uint8_t> Context::prove(const lmn_table* tables, size_t n_tables, const lmn_settings* settings,
                                    const Prepared* prepared) {
#ifndef LMN_EMU
  LMN_HIP_CHECK(hipSetDevice(device_));
#endif
  if (!tables || n_tables == 0) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "no trace tables");
  if (prepared) {   // refused before anything is launched, copied or exchanged
    if (shard_.active)
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, "prepared settings cannot be used on a sharded context (tree 0 is split into row blocks there)");
    if (prepared->device != device_)
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, "prepared settings live on device " + std::to_string(prepared->device) +
                                                   ", this context on device " + std::to_string(device_));
    if (prepared->log_blowup != cfg.log_blowup)
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, "prepared settings were extended by log_blowup " + std::to_string(prepared->log_blowup) +
                                                   ", this context proves with log_blowup " + std::to_string(cfg.log_blowup));
  }
  struct InFlight {
    InFlight() { g_proofs_in_flight.fetch_add(1, std::memory_order_relaxed); }
    ~InFlight() { g_proofs_in_flight.fetch_sub(1, std::memory_order_relaxed); }
  } in_flight;
  // A proof that ends in an exception may leave launches in flight that read plans from, or write results to, the
  // page-locked staging memory the next proof reuses from its start: drain the stream on that way out (not in a
  // lock-step batch, whose waits are rendezvous of all members), and close an upload group left open.
  struct FailureDrain {
    Context* c;
    int pending = std::uncaught_exceptions();
    ~FailureDrain() {
      if (std::uncaught_exceptions() <= pending) return;
      c->grp_pin_ = c->grp_dev_ = nullptr;
      c->grp_cap_ = c->grp_off_ = 0;
#if defined(LMN_BATCH) && !defined(LMN_EMU)
      // decided at run time: the batch library also exports the solo entry points (lmn_prove / lmn_prove_submit), whose
      // threads are outside any lock-step group and must drain like the main library's
      if (tls_batch_group == nullptr) (void)hipStreamSynchronize(c->stream_);
#elif !defined(LMN_EMU)
      (void)hipStreamSynchronize(c->stream_);
#endif
    }
  } failure_drain{this};
  ProofRun r(cfg.protocol_variant);
  r.tables = tables;
  r.n_tables = n_tables;
  r.settings = settings;
  r.prepared = prepared;
  r.lb = (int)cfg.log_blowup;
  r.n_slots = claim_slots(cfg.protocol_variant);
  r.log = g_log(this);
  r.log->reset();
  memset(&timings, 0, sizeof timings);
  // big trees are stored without the levels their fused launches keep in registers (MerkleCut); sharded proofs and the
  // level-2 ops (whose handles expose every layer) keep whole trees
  struct CutScope {
    bool& flag;
    ~CutScope() { flag = false; }
  } cut_scope{merkle_cut_};
  merkle_cut_ = !shard_.active && !env_set("LMN_MERKLE_FULL");

  // Device-resident Fiat-Shamir of the commitment phases - sharded proofs included since round 6 (every rank runs the same
  // steps behind the all-gather of the subtree roots); LMN_HOST_FS=1 keeps the transcript on the host (round 1-4
  // behaviour, for A/B measurements)
  r.dev_fs = !env_set("LMN_HOST_FS");
  run_setup(r);               // prove.cpp: validate the tables, size the arena, twiddles, transcript
  run_preprocessed(r);        // phase_trace.cpp: tree 0 (LUT columns)                      prover.rs:54-59
  run_main_trace(r);          // phase_trace.cpp: transpose + commit, claim mixed           prover.rs:70-179
  run_interaction(r);         // phase_logup.cpp: relation draws, logup columns + commit    prover.rs:186-298
  run_composition(r);         // phase_composition.cpp: constraint quotients + commit       prover.rs:312 (stwo::prover::prove)
  run_oods(r);                // phase_oods.cpp: OODS point, sampled values, self-check
  run_quotients(r);           // phase_oods.cpp: FRI quotient columns
  run_fri_commit(r);          // phase_fri.cpp: layers with the device-resident channel, last layer
  run_queries(r);             // phase_decommit.cpp: proof of work, query positions
  run_decommit(r);            // phase_decommit.cpp: one gather launch, proof assembly
  return run_finish(r);
}

void Context::run_setup(ProofRun& r) {
  LMN_RUN_ALIASES(r);
  // ---- validate (the input rules above), then size the arena
  const int max_log = scan_tables(r.tables, r.n_tables, cfg, shard_.active, device_, stream_, Refusal{}, infos);
  size_t words = 0;
  // a sharded context holds only its row block of every LDE / Merkle layer / large FRI layer
  const int size_g = shard_.active ? shard_.g : 0;
  auto row_split = [&](uint64_t w) { return size_g ? (w >> size_g) + 8192 : w; };
  for (const TableInfo& ti : infos) {
    const ComponentSpec* sp = ti.spec;
    const int ls = ti.log_size;
    uint64_t cells = (uint64_t)(sp->n_cols + 4 * sp->n_rel) << ls;
    words += cells * 2 + row_split(cells << lb);               // evals + coeffs + lde (this rank's row block)
    if (!ti.on_device && !ti.cols_on_device) words += ti.n_rows * sp->n_cols;  // staging
    if (!r.prepared) words += (uint64_t)sp->n_pre * ((2ull << ls) + row_split(2ull << ls));  // preprocessed columns: evals + coeffs + lde
    words += (4ull << ls) * 2;                                 // logup temps
    words += (4ull << (ls + 1)) * 3;                           // per-size composition scratch
    if (lb != 1) words += (uint64_t)(sp->n_cols + 4 * sp->n_rel + sp->n_pre) << (ls + 1);   // columns on the constraint domain
    if (shard_.active) words += (4ull << (ls + 1)) + 4096;     // halo rows of the last logup column group
    if (shard_rows_front(ls))                                  // received row blocks, gathered logup sums, scan output, coefficients
      words += (uint64_t)(sp->n_cols + 8 * sp->n_rel + 16) << ls;
    if (shard_all_to_all()) {                                  // own columns over all rows, packed copy, halo exchange
      const uint64_t G = shard_.world;
      words += 2 * (((uint64_t)sp->n_cols / G + 1) + ((uint64_t)(4 * sp->n_rel) / G + 1)) * (2ull << ls) + 6 * (2ull << ls);
    }
  }
  comp_log = max_log + 1;
  const int max_lde = comp_log + lb;
  words += (4ull << comp_log) * 2 + row_split(4ull << max_lde);  // composition values/coeffs + lde
  if (shard_all_to_all()) words += 2ull << max_lde;              // one composition column over all rows + its packed copy
  words += row_split((4ull << max_lde) * 3);                   // quotient columns (all sizes) + fri layers
  if (merkle_cut_ && max_lde >= 21)
    // trees without their register levels (MerkleCut): 1/8 of the nodes of a tree of 2^20 leaves and more
    // (bounds: up to four trees whose leaf level has more than 8 columns next to a smaller component's - that level is a
    // launch of its own and stays whole - and 1/8 + the block tops of everything else)
    words += 4 * (8ull << max_lde) + 7 * (3ull << max_lde) + (16ull << 20);
  else
    words += row_split(7 * (16ull << max_lde));                // merkle trees (4 trace + fri first + inner)
  if (shard_.active) words += 64ull << std::min(max_lde, std::max(shard_.fri_min_log, 12) + 2);  // replicated small FRI layers + their trees
  words += (16u << 20);                                        // slack: tables, partials, gather buffers
  ensure_twiddles(max_lde);
  // trace reuse: the previous proof's blocks are where it left them only if nothing but this reset has started over in
  // the arena since that proof's own; the record is spent here and stands again once this proof has enqueued its main trace
  const uint64_t gen_before = arena_.generation();
  arena_.reserve(words * 4);
  arena_.reset();
  reuse_.live = reuse_.valid && reuse_.generation == gen_before && arena_.generation() == gen_before + 1;
  reuse_.valid = false;
  reuse_.generation = arena_.generation();
  pin_off_ = 0;

  proof.claim.assign(n_slots, -1);
  proof.interaction_claim.assign(n_slots, {false, q_zero()});
  proof.pow_bits = cfg.pow_bits;
  proof.log_blowup = cfg.log_blowup;
  proof.log_last_layer = cfg.log_last_layer;
  proof.n_queries = cfg.n_queries;

  r.total_guard.reset(new StageTimer(this, log, stream_, C_TOTAL));
}

std::vector<uint8_t> Context::run_finish(ProofRun& r) {
  LMN_RUN_ALIASES(r);
  // ---- timings
  float acc[C_N] = {0};
  for (auto& sp : log->spans) acc[sp.cat] += lmn_event_elapsed_ms(sp.a, sp.b);
  timings.total_ms = acc[C_TOTAL];
  timings.transpose_ms = acc[C_TRANSPOSE];
  timings.main_commit_ms = acc[C_MAIN_COMMIT];
  timings.logup_ms = acc[C_LOGUP];
  timings.interaction_commit_ms = acc[C_INTER_COMMIT];
  timings.composition_ms = acc[C_COMPOSITION];
  timings.composition_commit_ms = acc[C_COMP_COMMIT];
  timings.oods_ms = acc[C_OODS];
  timings.quotients_ms = acc[C_QUOT];
  timings.fri_ms = acc[C_FRI];
  timings.decommit_ms = acc[C_DECOMMIT];
  timings.fft_ms = acc[C_FFT];
  timings.merkle_ms = acc[C_MERKLE];
  timings.merkle_fused_ms = acc[C_MERKLE_FUSED];
  std::vector<uint8_t> bytes = proof_to_bincode(proof);
  hm.mark("serialized");
  return bytes;
}

}  // namespace lmn
