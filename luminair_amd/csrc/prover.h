// Device-resident prover context and the `prove` orchestration that replaces
// /root/reference/crates/prover/src/prover.rs:28-319 on MI355X.
#pragma once
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/luminair_hip.h"

#include <array>
#include "constraints.h"
#include "host.h"
#include "kernels.h"

namespace lmn {

// kSpecs[kind] (constraints.h); nullptr for an unknown kind
const ComponentSpec* component_spec(int kind);
// The lookup components and the LMN_LOOKUP_* bit that announces each: the LUT-backed ones first, in LMN_LUT_* order (entry k
// reads the LUT of kind k and has bit 1 << k), then the 8-bit range check, whose column the library generates.
struct LookupKind {
  int kind;
  uint32_t bit;
};
constexpr LookupKind kLookupKinds[4] = {{LMN_KIND_SIN_LOOKUP, LMN_LOOKUP_SIN},
                                        {LMN_KIND_EXP2_LOOKUP, LMN_LOOKUP_EXP2},
                                        {LMN_KIND_LOG2_LOOKUP, LMN_LOOKUP_LOG2},
                                        {LMN_KIND_RANGE_CHECK_LOOKUP, LMN_LOOKUP_RANGE_CHECK}};
// settings that count LUTs point to them: the one rule on the LUT list that the prover and the verifier share
inline void require_luts_pointer(const lmn_settings& s) {
  if (s.n_luts && !s.luts) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "null luts pointer");
}
// the row a component's table is padded with: is_last = 1 and the spec's padding values, zero elsewhere
inline PadRow pad_row_of(const ComponentSpec& sp) {
  PadRow pad{};
  if (sp.is_last_col >= 0) pad.v[sp.is_last_col] = 1u;
  for (int k = 0; k < sp.n_pad; ++k) pad.v[sp.pad_col[k]] = sp.pad_val[k];
  return pad;
}
// relation element sets drawn after the main commitment (components/mod.rs:227-235, lookups/mod.rs:44-51)
struct RelElems {
  QM31 z[N_ELEMS], alpha[N_ELEMS];
  bool drawn[N_ELEMS] = {false, false, false, false, false};
};
class Channel;
RelElems draw_relation_elements(Channel& channel, uint32_t protocol_flags);
// the element set each draw_felts(2) of LuminairInteractionElements::draw fills, in draw order; returns the number of draws
int relation_draw_sets(uint32_t protocol_flags, int sets_out[5]);
inline int claim_slots(uint32_t protocol_flags) { return (protocol_flags & LMN_PV_CLAIM17) ? 17 : 8; }

// Constraint slots of a component under the protocol's constraint-form bits (LMN_PV_*_SLOT(S) / _NEG, luminair_hip.h).
// "Kernel slot" k = the k-th value of the component: what local_constraints<KIND> (constraints.h: the one statement that
// k_composition, k_trace_check and the host's evaluation at the OODS point all instantiate) emits, in `evaluate` order with
// the KAT-era shape (eval_fixed_mul: two slots; recip / sqrt / rem: one), then one per relation.
// The protocol may give a helper one slot more or less and the opposite sign; that only changes WHICH power of the
// composition randomness multiplies a kernel slot, so it is decided here on the host and the kernels never see the bits.
struct ConstraintLayout {
  int n_kernel = 0;      // n_local + n_rel
  int n_protocol = 0;    // constraints the component contributes to the composition polynomial (zero slots included)
  int proto_index[16];   // per kernel slot: index among the component's protocol constraints; -1 = no such constraint
  bool neg[16];          // the protocol's constraint is minus the kernel's value
};
ConstraintLayout constraint_layout(const ComponentSpec& sp, uint32_t protocol_flags);

// one component of a proof: shared by the prover and the host-side verifier
struct Instance {
  const ComponentSpec* spec;
  int log_size;
  int main_start, inter_start;  // column offsets inside trees 1 / 2
  QM31 claimed;
  uint32_t* halo = nullptr;               // sharded proofs with all_to_all: neighbour blocks of the last logup group
  const QM31* d_claimed_shift = nullptr;  // device [claimed, shift] (prover only)
  uint32_t* trace_evals = nullptr;        // device, n_cols x 2^log_size (prover only)
  bool rows_sharded = false;              // sharded proofs: trace_evals holds this rank's block of 2^(log_size - g) rows only
  // trace_evals == nullptr: the evaluations were never stored column-major (the transpose ran inside the interpolation,
  // fft_fixed.hip k_fft_rows_fx): readers take them from the table's rows on the device, padded beyond rows_n
  const uint32_t* rows_dev = nullptr;
  uint64_t rows_n = 0;
  PadRow pad{};
  int pre_idx[2] = {-1, -1};    // tree-0 column indices of the component's preprocessed columns
};
// sum_k c_k(oods)/Z_k(oods) * alpha^(N-1-k) from the sampled mask values
QM31 eval_composition_at_point(const std::vector<Instance>& inst, const std::vector<std::vector<std::vector<QM31>>>& sv,
                               QPt oods, const RelElems& elems, QM31 comp_alpha, uint32_t protocol_flags);
// tree-0 layout implied by the components present: fills Instance::pre_idx, returns the columns' log
// sizes in tree order (a LUT column has the log size of its lookup component)
std::vector<int> assign_preprocessed(std::vector<Instance>& inst);
// verify(proof, settings): crates/verifiers/rust/src/verifier.rs:21-143 (host only, no GPU work)
// `expect`: the verifier's own PcsConfig + protocol variant (a proof announcing another config is rejected);
// `settings` (may be null): cross-checked against the tree-0 layout the claim implies
void verify_proof(const uint8_t* data, size_t len, const lmn_config& expect, const lmn_settings* settings,
                  lmn_verify_report* report = nullptr);

// bump allocator over one device slab; reset per proof
class Arena {
 public:
  ~Arena();
  void reserve(size_t bytes);
  void reset() {
    off_ = 0;
    ++generation_;
  }
  // counts the resets and the growths: two equal readings mean that nobody has started over in the arena in between
  uint64_t generation() const { return generation_; }
  void* alloc_bytes(size_t bytes);
  uint32_t* alloc_words(size_t words) { return (uint32_t*)alloc_bytes(words * 4); }
  uint64_t word_offset(const void* p) const { return (uint64_t)((const char*)p - base_) / 4; }
  const uint32_t* base_words() const { return (const uint32_t*)base_; }
  size_t capacity() const { return cap_; }
  size_t used() const { return off_; }

 private:
  char* base_ = nullptr;
  size_t cap_ = 0, off_ = 0;
  uint64_t generation_ = 0;
};

struct DevColumn {
  int log_size;      // polynomial (coefficient) log size
  uint32_t* coeffs;  // 2^log_size
  uint32_t* lde;     // 2^(log_size + log_blowup), bit-reversed canonic-domain evaluations
  bool sharded = false;  // lde holds only this rank's block of 2^(log_size + log_blowup - g) rows
  int owner = -1;        // >= 0: the coefficients exist on that rank only (column-parallel interpolation)
};

// A column as the Merkle / decommitment code sees it.  sharded: ptr is this rank's aligned block of
// 2^(log - g) rows (row r of the column lives on rank r >> (log - g)); otherwise ptr holds all 2^log rows.
struct ColRef {
  const uint32_t* ptr;
  int log;
  bool sharded;
};

// A fused Merkle launch whose lanes kept their per-lane subtree in registers only: layers start_log, start_log - 1, ...,
// start_log - depth + 1 of the tree do not exist in HBM (7/8 of a big tree's 32-byte nodes, 1 GB of writes per 2^20-row
// proof, of which the decommitment reads a few dozen).  What the decommitment needs of them is recomputed from the
// launch's start level (MerkleRecompute, k_gather).
struct MerkleCut {
  int start_log, depth;
  const uint32_t* prev;
  MerkleSegs sg;
  int ncols;
  const uint32_t* below = nullptr;   // the launch hashed the leaf level under its start level itself (MerkleFold::below)
  int below_ncols = 0;
  bool leaf_from_above = false;      // this IS that leaf level: never hashed by a launch of its own, a node = the hash of its leaf
};

struct DevMerkle {
  int max_log = -1;
  // layers[k]: 2^k hashes of 8 words.  In a sharded tree (g > 0) the layers k > g hold only this rank's
  // 2^(k-g) nodes (node n lives on rank n >> (k - g)); layers k <= g are complete on every rank.
  // A null layer was not written: see `cuts`.
  std::vector<uint32_t*> layers;
  std::vector<MerkleCut> cuts;
  int g = 0;
  Hash32 root;
  const uint32_t* root_pinned = nullptr;  // pending async download of layers[0]
  void finish_root() {
    if (root_pinned) memcpy(root.w, root_pinned, 32);
    root_pinned = nullptr;
  }
};

struct DevTree {
  std::vector<DevColumn> cols;
  DevMerkle merkle;
};

// what lmn_tree_decommit hands to its caller: three buffers from malloc (released with lmn_free), null where empty
struct TreeOpening {
  uint32_t* queried_values = nullptr;
  size_t n_values = 0;
  uint8_t* hash_witness = nullptr;   // n_hashes x 32 bytes
  size_t n_hashes = 0;
  uint32_t* column_witness = nullptr;
  size_t n_column_words = 0;
};

// what lmn_col_fri_commit hands to its caller (lmn_fri_commit_result): buffers from malloc, released one by one on failure
struct FriCommitOut {
  lmn_fri_commit_result r{};
  ~FriCommitOut();                      // frees what release() has not handed over
  lmn_fri_commit_result release();
};

// what lmn_col_fri_close hands to its caller (lmn_fri_close_result)
struct FriCloseOut {
  lmn_fri_close_result r{};
  ~FriCloseOut();
  lmn_fri_close_result release();
};

// the caller-facing limits of one accumulate_quotients call (level2.cpp): LMN_ERR_INVALID_ARGUMENT past them
void check_quotient_limits(const uint32_t* sample_point, uint32_t nsamples);
// the sample points and each column's (point, value) list of such a call, as make_quotient_args takes them;
// LMN_ERR_INVALID_ARGUMENT for a sample that names a column or a point the call does not have
struct QuotientSamples {
  std::vector<QPt> points;
  std::vector<std::vector<std::pair<int, QM31>>> of_col;
};
QuotientSamples parse_quotient_samples(uint32_t ncols, const uint32_t* sample_col, const uint32_t* sample_point,
                                       const uint32_t* sample_values, uint32_t nsamples, const uint32_t* points_xy, uint32_t npoints);

// A trace table that a HOST producer fills chunk by chunk while it works (lmn_rows_*, trace_gen.cpp): column-major in
// HBM from the first push on, so that what is left between the last row and the proof is one chunk's transfer, the padding
// rows and one wait.  The columns come from lmn_dev_malloc, outside every context's per-proof arena; all device work runs
// on the sink's own stream, so a proof on the context it was opened on overlaps with its filling.  Calls on one sink are
// serialised by its own lock and never take the context's.
// A DEVICE producer may fill it too (lmn_rows_append_*, a Context producer with TraceTarget::into): the producer's column-form launch runs on
// the context's stream and writes the node's rows straight into the columns at the sink's current row count.  Such a call
// holds the context's lock and takes the sink's behind it - always in that order.  The two streams are tied by two events:
// `appended_` (recorded on the producer's stream behind every append; sync, finish, reset and the destructor make the sink's
// stream wait for it before anything else) and `cleared_` (recorded on the sink's stream behind the memset that clears
// `bad_`, at open and at every reset; the next append makes the producer's stream wait for it).
class RowSink {
 public:
  RowSink(int device, uint32_t kind, uint64_t capacity_rows);
  ~RowSink();
  RowSink(const RowSink&) = delete;
  RowSink& operator=(const RowSink&) = delete;
  // pinned: `host_rows` is page-locked and read by the GPU where it lies; otherwise it is copied through the staging ring
  void push(const uint32_t* host_rows, uint64_t n, bool pinned);
  void sync();
  void finish(lmn_table* table_out);
  void reset();
  uint64_t count() const;
  // One device append, between the producer's argument checks and its launch.  The constructor takes the sink's lock and
  // refuses (LMN_ERR_INVALID_ARGUMENT, text = `call`: `rows`: ...) a sink of another kind or device, one that is not filling,
  // and more rows than capacity - count; then makes `producer` wait for the last clearing of `bad_`.  cols() / stride() /
  // bad() are what the column-form launch takes.  done(): the launch is enqueued - records `appended_` behind it and adds the
  // rows to the count.  Without done() the sink is as it was.
  class Append {
   public:
    Append(RowSink& sink, const char* call, int device, lmn_stream_t producer, uint32_t kind, uint64_t n_rows);
    uint32_t* cols() const { return sink_.cols_ + sink_.count_; }
    uint64_t stride() const { return sink_.stride_; }
    uint32_t* bad() const { return sink_.bad_; }
    void done();

   private:
    RowSink& sink_;
    std::lock_guard<std::mutex> lock_;
    lmn_stream_t producer_;
    uint64_t n_rows_;
  };

 private:
  friend void rows_sink_attach(const lmn_table& tb, int device, lmn_stream_t proof_stream);
  void forget();   // no longer a finished table prove() accepts
  int device_;
  const ComponentSpec* spec_;
  uint64_t cap_, stride_, count_ = 0;
  enum { FILLING, FINISHED, FAILED } state_ = FILLING;
  PadRow pad_{};
  uint32_t* cols_ = nullptr;     // n_cols x stride_ words (n_cols x 2^log_size after a finish that compacted them)
  uint32_t* bad_ = nullptr;      // the sink's own device word: set by a chunk that held a non-canonical word
  uint32_t* h_bad_ = nullptr;    // page-locked: its copy, read after finish's one wait
  lmn_stream_t stream_{};
  lmn_event_t done_{};           // recorded behind finish's last launch: what a proof's stream waits for
  lmn_event_t appended_{};       // recorded on a producer's stream behind a device append (pending_: not yet waited for)
  lmn_event_t cleared_{};        // recorded on stream_ behind every clearing of bad_
  lmn_stream_t pending_on_{};    // the producer stream appended_ was last recorded on
  bool pending_ = false;
  void join_appends();           // stream_ waits for the pending appends (mu_ held)
  // Staging ring of lmn_rows_push (pageable rows), allocated by the first such push: SLOTS page-locked slots of SLOT_BYTES.
  // 4 MiB holds one of the 16 chunks of BASELINE config 2a (2^16 rows x 15 columns = 3.75 MiB) in ONE launch, and
  // is ~75 us of link time against ~400 us of the CPU copy that fills it: with 4 slots the copy never waits for the link.
  static constexpr int SLOTS = 4;
  static constexpr size_t SLOT_BYTES = 4u << 20;
  char* ring_ = nullptr;
  const char* ring_dev_ = nullptr;   // the ring as the chunk kernel addresses it
  lmn_event_t slot_done_[SLOTS] = {};
  int next_slot_ = 0;
  mutable std::mutex mu_;
};
// prove(): a LMN_TABLE_COLS_ON_DEVICE table must be the finished columns of a sink on this device (LMN_ERR_INVALID_ARGUMENT
// otherwise); the proof stream is made to wait for the sink's finish event - the host does not wait
void rows_sink_attach(const lmn_table& tb, int device, lmn_stream_t proof_stream);

// An operand of a trace producer as the C API hands it over: a device pointer, an optional strided view, and the member
// stride of the many-member forms
struct TraceIn {
  const void* p = nullptr;
  const lmn_view* view = nullptr;
  uint64_t ms = 0;
};
// Where a trace producer's rows and outputs go (Context::elementwise and its siblings): a table at row_offset
// (lmn_trace_*), n_members tables with their strides and counters (lmn_trace_many_*: `*_ms` of operands / outputs in
// elements, rows in rows of the kind, tables in words), or a row sink's columns at its current count (lmn_rows_append_*).
// `call`: the entry point's name, put in front of every rule's text; the integer table forms carry none.
// Refused elements are counted in *refused (may be null; the table form has none) - and fail a sink's finish.
struct TraceTarget {
  enum Form { TABLE, MANY, SINK } form;
  const char* call;
  uint32_t* rows;
  uint64_t row_offset, rows_ms;
  uint32_t n_members;
  RowSink* sink;
  int32_t* out;
  uint64_t out_ms;
  uint32_t* refused;
  static TraceTarget table(uint32_t* rows, uint64_t row_offset, int32_t* out, const char* call = nullptr) {
    return {TABLE, call, rows, row_offset, 0, 1, nullptr, out, 0, nullptr};
  }
  static TraceTarget many(const char* call, uint32_t n_members, uint32_t* rows, uint64_t row_offset, uint64_t rows_ms, int32_t* out,
                          uint64_t out_ms, uint32_t* refused) {
    return {MANY, call, rows, row_offset, rows_ms, n_members, nullptr, out, out_ms, refused};
  }
  static TraceTarget into(const char* call, RowSink& sink, int32_t* out, uint32_t* refused) {
    return {SINK, call, nullptr, 0, 0, 1, &sink, out, 0, refused};
  }
};

// Settings prepared once (lmn_settings_prepare): everything about tree 0 that does not depend on the pie - the LUT and
// range-check columns on their trace domain, their coefficients, their LDE, every Merkle layer and the root - in device
// memory of its own, immutable after construction and read by any number of proofs at once.  The memory is the arena of
// a private context that exists for this object alone (own stream; reserved once, never reset, so nothing moves).
class Context;
class Prepared {
 public:
  Prepared(int device, const lmn_config& cfg, const lmn_settings* settings, uint32_t lookups);
  ~Prepared();
  Prepared(const Prepared&) = delete;
  Prepared& operator=(const Prepared&) = delete;
  int device = 0;
  uint32_t lookups = 0;                // LMN_LOOKUP_* bits of the lookup components its pies contain
  uint32_t log_blowup = 0;
  int log_of_pre[N_PRE_IDS];           // log size of each preprocessed column present, -1 otherwise
  DevTree tree;                        // columns in tree-0 order (assign_preprocessed); no cut levels: every layer is in memory
  std::vector<uint32_t*> evals;        // the columns on their trace domain, tree-0 order
  // the one slab everything above lies in (k_gather's second base)
  const uint32_t* base_words() const { return base_; }
  bool holds(const void* p) const { return (const char*)p >= (const char*)base_ && (const char*)p < (const char*)base_ + bytes_; }
  uint64_t word_offset(const void* p) const { return (uint64_t)((const char*)p - (const char*)base_) / 4; }

 private:
  friend class Context;
  Context* ctx_ = nullptr;
  const uint32_t* base_ = nullptr;
  size_t bytes_ = 0;
};

struct StageTimer;

struct FriClose;   // the device chain that closes the FRI transcript (prove_run.h)
struct ProofRun;   // state of one proof across the phases of Context::prove (prove_run.h)

class Context {
 public:
  // pin_bytes: page-locked staging of the context (a proving context stages plans, tables and results of megabytes)
  Context(int device, const lmn_config& cfg, size_t pin_bytes = 32u << 20);
  ~Context();
  // prepared != nullptr (lmn_prove_prepared): tree 0 is the prepared object's, `settings` is not read
  std::vector<uint8_t> prove(const lmn_table* tables, size_t n_tables, const lmn_settings* settings,
                             const Prepared* prepared = nullptr);
  // lmn_settings_prepare, on the private context of `out`: checks, places, transforms and commits tree 0 once, then waits
  void build_prepared(Prepared& out, const lmn_settings* settings, uint32_t lookups);
#ifdef LMN_BATCH
  // lock-step batches (batch.h): every member context issues its work on the group's one stream
  void adopt_stream(lmn_stream_t s);
  // the set-up `prove` would do for these tables on its first call with such a shape (twiddle tables), done outside
  // lock-step; malformed tables are left for `prove` to report
  void prepare_for(const lmn_table* tables, size_t n_tables);
#endif

  // level-2 ops
  void op_interpolate(uint32_t* cols, uint32_t ncols, uint32_t log_size);
  void op_evaluate(const uint32_t* coeffs, uint32_t ncols, uint32_t log_coeffs, uint32_t log_domain, uint32_t* out);
  void op_evaluate_block(const uint32_t* coeffs, uint32_t ncols, uint32_t log_coeffs, uint32_t log_domain,
                         uint32_t log_blocks, uint32_t block, uint32_t* out);
  void op_merkle_root(const uint32_t* const* cols, const uint32_t* log_sizes, uint32_t ncols, uint8_t root[32]);
  void op_eval_at_point(const uint32_t* coeffs, uint32_t log_size, const uint32_t pt[8], uint32_t out[4]);
  void op_fft_selftest(uint32_t log_size, uint32_t ncols);
  void op_accumulate_quotients(uint32_t log_size, const uint32_t* const* cols, uint32_t ncols, const uint32_t* sample_col,
                               const uint32_t* sample_point, const uint32_t* sample_values, uint32_t nsamples,
                               const uint32_t* points_xy, uint32_t npoints, const uint32_t alpha[4], uint32_t* out);
  void op_fold(int circle, uint32_t* dst, const uint32_t* src, uint32_t log_src, const uint32_t alpha[4]);
  // GrindOps::grind on the device (lmn_ctx_grind): the smallest nonce the proof-of-work check of `variant` accepts
  uint64_t op_grind(const Hash32& digest, uint32_t pow_bits, uint32_t variant);
  // the same for n digests in one go (lmn_ctx_grind_many): nonces_out[i] for digests[32 * i ..]
  void op_grind_many(const uint8_t* digests, uint32_t n, uint32_t pow_bits, uint32_t variant, uint64_t* nonces_out);
  // n digests ground together on the device (k_grind_many): result[i] = Channel::grind's nonce for w[i].  In the lock-step
  // batch build this is a collective: the members' digests are ground in one go by whoever arrives last.
  std::vector<uint64_t> grind_many(const PowWords* w, uint32_t n, bool kat, uint32_t pow_bits);

  // single-proof sharding (lmn_ctx_set_shard / lmn_ctx_set_shard_rccl)
  static void check_shard_args(uint32_t rank, uint32_t world, uint32_t fri_min_log, const lmn_collective* coll);
  void set_shard(uint32_t rank, uint32_t world, uint32_t fri_min_log, const lmn_collective* coll);
  void set_shard_rccl(uint32_t rank, uint32_t world, uint32_t fri_min_log, const uint8_t* id);
  void clear_shard();

  // level-2 ops on device handles (level2.cpp)
  lmn_col* col_alloc(uint32_t ncols, uint32_t log_size, bool zero);
  lmn_col* col_from_cpu(const uint32_t* host, uint32_t ncols, uint32_t log_size);
  void col_to_cpu(const lmn_col* c, uint32_t* host);
  void col_free(lmn_col* c);
  lmn_col* col_view(const lmn_col* c, uint32_t first, uint32_t n);
  void col_bit_reverse(lmn_col* c);
  void col_precompute_twiddles(uint32_t log_size);
  void col_interpolate(lmn_col* c);
  lmn_col* col_evaluate(const lmn_col* coeffs, uint32_t log_domain);
  lmn_col* col_evaluate_block(const lmn_col* coeffs, uint32_t log_domain, uint32_t log_blocks, uint32_t block);
  lmn_col* col_extend(const lmn_col* coeffs, uint32_t log_size);
  void col_eval_at_point(const lmn_col* coeffs, uint32_t column, const uint32_t pt[8], uint32_t out[4]);
  lmn_tree* col_commit(const lmn_col* const* cols, uint32_t n);
  void tree_layer_to_cpu(const lmn_tree* t, uint32_t layer_log, uint8_t* out);
  void tree_free(lmn_tree* t);
  void tree_decommit(const lmn_tree* t, const lmn_col* const* cols, uint32_t n_cols, const uint32_t* query_logs,
                     const uint32_t* query_counts, uint32_t n_groups, const uint32_t* queries, TreeOpening& out);
  void col_gather(const lmn_col* c, const uint32_t* positions, uint32_t n, uint32_t* host_out);
  // FriProver::commit without the last layer's interpolation: prove()'s layer loop (fri_commit_layers) on column handles
  void col_fri_commit(const lmn_col* const* cols, uint32_t n, const uint8_t start_digest[32], FriCommitOut& out);
  // what FriProver::commit and the query phase do behind the layer loop, as one device chain (enqueue_fri_close): the last
  // layer's polynomial and degree check, mix_felts, the grind, mix_u64, Queries::generate
  // keep != nullptr (lmn_col_fri_close_keep): the positions also stay on the device, in a new handle
  void col_fri_close(const lmn_col* last_layer, const uint8_t start_digest[32], uint32_t log_query_domain, FriCloseOut& out,
                     lmn_positions** keep = nullptr);
  // query positions on the device and the openings planned there (lmn_positions_*, lmn_open_queries; kernels.h k_open_plan)
  lmn_positions* positions_from_cpu(const uint32_t* positions, uint32_t n, uint32_t log_domain);
  void positions_to_cpu(const lmn_positions* p, uint32_t* host, uint32_t* n_out);
  void positions_free(lmn_positions* p);
  void open_queries(const lmn_positions* p, const lmn_open_item* items, uint32_t n_items, lmn_opening* out);
  // lmn_verify_many (verifier.cpp): results[i] for every proof; first_rejection = the text of the first rejection in index order
  void verify_many(const uint8_t* const* proofs, const size_t* lens, uint32_t n, const lmn_settings* settings,
                   const lmn_config& expect, lmn_verify_result* results, std::string& first_rejection);
  void col_accumulate(lmn_col* dst, const lmn_col* src);
  lmn_col* col_accumulate_quotients(const lmn_col* const* cols, uint32_t n, const uint32_t* sample_col,
                                    const uint32_t* sample_point, const uint32_t* sample_values, uint32_t nsamples,
                                    const uint32_t* points_xy, uint32_t npoints, const uint32_t alpha[4]);
  lmn_col* col_fold_line(const lmn_col* src, const uint32_t alpha[4]);
  void col_fold_circle_into_line(lmn_col* dst, const lmn_col* src, const uint32_t alpha[4]);
  lmn_col* col_decompose(const lmn_col* f, uint32_t lambda_out[4]);
  // FieldOps::batch_inverse (M31, or QM31 on 4 coordinate columns): dst = src^-1 element by element, 0 for a zero element;
  // n_zero_out != nullptr waits and reports how many elements were zero
  void col_batch_inverse(const lmn_col* src, lmn_col* dst, bool secure, uint64_t* n_zero_out);
  lmn_col* col_logup(uint32_t kind, const lmn_col* main, const lmn_col* pre, const uint32_t* elems, uint32_t claimed_out[4]);
  void col_composition(uint32_t kind, const lmn_col* main_lde, const lmn_col* inter_lde, const lmn_col* pre_lde,
                       const uint32_t* elems, const uint32_t claimed[4], const uint32_t* coeffs, uint32_t n_coeffs,
                       lmn_col* acc);

  void* upload(const void* host, size_t bytes);
  void* device_alloc(size_t bytes);
  void upload_to(const void* host, size_t bytes, void* dst);
  void device_copy(void* dst, const void* src, size_t bytes);
  void download(const void* device, void* host, size_t bytes);
  // The trace producers (trace_gen.cpp): `process_trace` of a node on device tensors, one method per producer.  What it
  // computes is the method's; where the rows and outputs go is the TraceTarget's (the three forms of the C API).
  // Operands: member m of a many-member target reads p + m * ms elements (ms == 0 shares the operand).
  void elementwise(const TraceTarget& tg, uint32_t kind, const TraceIn& lhs, const TraceIn& rhs, uint64_t n,
                   const lmn_node_info& info, uint32_t* rc_mult = nullptr, uint64_t rc_ms = 0, int src_dtype = SRC_FIXED);
  void contiguous(const TraceTarget& tg, const TraceIn& input, uint64_t in_size, uint64_t out_size, const lmn_node_info& info);
  void reduce(const TraceTarget& tg, bool is_max, const TraceIn& input, uint64_t front, uint64_t dim, uint64_t back,
              const lmn_node_info& info);
  void lut(const TraceTarget& tg, uint32_t kind, const TraceIn& input, uint64_t n, const lmn_node_info& info,
           const uint32_t* lut_col1, const lmn_range* ranges, uint32_t n_ranges, uint32_t* mult, uint64_t mult_ms = 0);
  // graph inputs from raw float bits of `dtype` (src.ms in elements of the dtype)
  void inputs_float(const TraceTarget& tg, uint32_t dtype, const TraceIn& src, uint64_t n, const lmn_node_info& info);
  // lmn_eval_* (trace_gen.cpp): the producers' forward pass - values, their range, the refused elements; no rows
  void eval_elementwise(uint32_t kind, const int32_t* lhs, const lmn_view* lv, const int32_t* rhs, const lmn_view* rv, uint64_t n,
                        int32_t* out, int32_t* minmax, uint32_t* refused);
  void eval_reduce(bool is_max, const int32_t* input, uint64_t front, uint64_t dim, uint64_t back, int32_t* out, int32_t* minmax,
                   uint32_t* refused);
  void eval_lut(uint32_t kind, const int32_t* input, const lmn_view* view, uint64_t n, const uint32_t* lut_col1,
                const lmn_range* ranges, uint32_t n_ranges, int32_t* out, int32_t* minmax, uint32_t* refused);
  void tensor_range(const int32_t* buf, uint64_t n, int32_t* minmax);
  // lmn_eval_inputs_float / lmn_tensor_to_float (trace_gen.cpp): the float source's forward pass, outputs back to floats
  void eval_inputs_float(uint32_t dtype, const void* src, uint64_t n, int32_t* out, int32_t* minmax, uint32_t* refused);
  void tensor_to_float(uint32_t dtype, const int32_t* src, uint64_t n, void* dst);
  void device_free(void* p);
  // lmn_trace_check (trace_gen.cpp): the rows that break a local constraint and the logup tuples that do not balance
  void trace_check(const lmn_table* tables, size_t n_tables, const lmn_settings* settings, lmn_trace_report& report);

  int device() const { return device_; }
  // lmn_ctx_counter - 7: device grinds started, 8: host waits inside grind rounds, 9: proofs whose transcript was closed on
  // the device, 10: those among them that fell back to the host's grind rounds; 0 for any other number
  // 11, 12: proofs opened by the device plan, fallbacks among them; 13, 14, 15 (diagnostic): plan launches, fetch launches
  // and host waits of open_queries; 16 .. 19: verify_many's proofs judged by the device stage, stage-2 proofs, launches, waits
  // 20, 21 (trace reuse): candidate columns compared with the previous proof's, columns among them whose transforms were skipped
  // 22, 23 (diagnostic): proofs whose quotient tables k_quot_prepare made, unsharded device-transcript proofs that kept the host's wait
  uint64_t counter(int which) const {
    return which >= 7 && which <= 10    ? counters_[which - 7]
           : which >= 11 && which <= 12 ? dev_open_counters_[which - 11]
           : which >= 13 && which <= 15 ? open_counters_[which - 13]
           : which >= 16 && which <= 19 ? verify_counters_[which - 16]
           : which >= 20 && which <= 21 ? reuse_counters_[which - 20]
           : which >= 22 && which <= 23 ? quot_counters_[which - 22]
                                        : 0;
  }
  lmn_config cfg;
  lmn_timings timings{};
  bool profiling = false;  // record HIP events around stages/kernels (lmn_set_profiling)
  void* event_log = nullptr;  // EventLog (prover.cpp)
  void* host_scratch = nullptr;  // HostScratch (prover.cpp): decommit-planning storage reused across proofs
  std::string last_error;

 private:
  // the phases of prove(), in transcript order (prove.cpp, phase_*.cpp)
  void run_setup(ProofRun& r);
  void run_preprocessed(ProofRun& r);
  void run_main_trace(ProofRun& r);
  void run_interaction(ProofRun& r);
  void run_composition(ProofRun& r);
  void run_oods(ProofRun& r);
  void replay_device_transcript(ProofRun& r, const std::function<void(QM31)>& set_points);
  void set_sample_points(ProofRun& r, QM31 t);          // phase_oods.cpp: the OODS point of the draw t and the mask points
  void enqueue_quotient_tables(ProofRun& r, const QM31* d_vals);   // phase_oods.cpp: k_quot_prepare + the quotient launches' arguments
  void finish_oods_on_host(ProofRun& r);                 // phase_oods.cpp: the host's replay of everything from root 1 to the quotient randomness
  void check_composition_identity(ProofRun& r);          // phase_oods.cpp: stwo's OODS sanity check on the sampled values
  void run_quotients(ProofRun& r);
  void run_fri_commit(ProofRun& r);
  void fri_commit_layers(ProofRun& r);   // phase_fri.cpp: the layer loop, shared with col_fri_commit
  // phase_fri.cpp, shared with col_fri_close: the chain k_fri_close | grind windows | k_fri_queries behind what produces
  // `d_last` and leaves `d_ch` behind the last alpha; after the next wait, the host's replay on `channel` and its
  // cross-check.  `last_vals`: the last layer on the host, fetched only if no nonce lay in the queued windows.
  void enqueue_fri_close(FriClose& fc, const uint32_t* d_last, DevChannel* d_ch, uint32_t log_query_domain);
  void finish_fri_close(FriClose& fc, Channel& channel, const std::function<std::vector<QM31>()>& last_vals,
                        bool refuse_bad_degree);
  void run_queries(ProofRun& r);
  void run_decommit(ProofRun& r);
  void enqueue_device_decommit(ProofRun& r);   // behind enqueue_fri_close, in front of the FRI wait
  const uint32_t* plan_and_gather_on_host(ProofRun& r, std::vector<std::array<size_t, 4>>& cnt, std::vector<uint32_t>& merged);
  std::vector<uint8_t> run_finish(ProofRun& r);

  void ensure_twiddles(int max_domain_log);
  TwPtrs tw(int domain_log) const;
  TwPtrs itw(int domain_log) const;
  // evaluations -> coefficients (`coeffs` may equal `evals`).  Unsharded proofs of a supported size get the blown-up
  // evaluation in the same three launches (launch_interp_extend): returns the LDE (ncols x 2^(log + log_blowup),
  // arena) or nullptr when lde_and_merkle has to produce it.
  //   Sharded proofs whose collective offers all_to_all (SURVEY.md section 8e stages A / B): this rank interpolates and
  //   extends only its contiguous share of the columns and receives its row block of every column's LDE through one
  //   all-to-all; coefficients then exist on the owning rank only (CommitOut::first), and with halo_first >= 0 the two
  //   neighbouring row blocks of the 4 columns halo_first .. halo_first + 3 (mask offset -1 of the last logup column
  //   group) arrive through a second, small all-to-all.
  struct CommitOut {
    uint32_t* lde = nullptr;      // nullptr: lde_and_merkle produces it
    uint64_t stride = 0;          // words between the columns of `lde`
    bool sharded = false;         // `lde` holds this rank's row block only
    bool owned = false;           // column c's coefficients live on rank `owner_of(c)` only
    int first[9] = {0};           // columns [first[r], first[r + 1]) belong to rank r
    uint32_t* halo = nullptr;     // 4 columns x 2^(log + 1) words, the two neighbour blocks filled in
    bool skipped = false;         // the transforms ran with the caller's ColSkip
    int owner_of(int c) const {
      if (!owned) return -1;
      int r = 0;
      while (first[r + 1] <= c) ++r;
      return r;
    }
  };
  // evals_row_blocks: `evals` holds this rank's row block of every column (row-parallel transposes / logup); the blocks
  // travel to the columns' owners through one more all-to-all before stage A
  // skip (trace reuse, the three-launch form only): applied if the LDE block comes to lie at skip_lde, where the columns
  // it lets through unworked still hold their values; CommitOut::skipped says whether it was
  CommitOut interpolate_for_commit(uint32_t* coeffs, const uint32_t* evals, int ncols, int log_size, int halo_first = -1,
                                   bool evals_row_blocks = false, const ColSkip* skip = nullptr,
                                   const uint32_t* skip_lde = nullptr);
  bool shard_all_to_all() const;
  bool shard_a2a_columns(int log_size) const;   // stage A / B for columns of this size
  bool shard_rows_front(int log_size) const;    // row-parallel transposes and logup fractions for tables of this size
  // commit `cols` (coefficients already in place) -> LDE + Merkle (row-block sharded when a shard is set)
  // `step` (device-resident transcript): made by the launch that produces the root, or by launch_chan_step behind it
  void lde_and_merkle(DevTree& tree, bool fetch_root = true, DevChannel* step_ch = nullptr, const ChanStep* step = nullptr);
  // Merkle tree over columns sorted by size (descending, stable).  sharded: every rank hashes the subtree over its
  // row block, the subtree roots are all-gathered and the top log2(world) levels are hashed on every rank.
  // `fold` (unsharded FRI layers of more than 2^10 rows only): the leaf level computes the layer as the fold of the
  // previous one while hashing it (MerkleFold, kernels.h); cols_sorted then names the 4 columns it writes.
  void build_merkle(DevMerkle& m, const std::vector<ColRef>& cols_sorted, DevChannel* ch = nullptr,
                    QM31* alpha_out = nullptr, uint32_t* root_copy = nullptr, bool sharded = false,
                    const MerkleFold* fold = nullptr, const ChanStep* step = nullptr);
  // null entries of `layers` are allocated from the arena as the launches reach them; with `cuts` given, the levels a
  // fused launch keeps in registers stay null and are recorded there instead
  void build_merkle_levels(std::vector<uint32_t*>& layers, int max_log,
                           const std::vector<std::vector<const uint32_t*>>& per_level, DevChannel* ch, QM31* alpha_out,
                           uint32_t* root_copy, const MerkleFold* fold = nullptr, std::vector<MerkleCut>* cuts = nullptr,
                           const ChanStep* step = nullptr);
  // in-place all-gather of `ncols` columns `col_stride` words apart: rank r owns words [r*w, (r+1)*w) of each
  void gather_columns(uint32_t* base, uint64_t col_stride, int ncols, uint64_t words_per_rank);
  void merkle_layer_timed(const uint32_t* prev, const uint32_t* const* cols, int ncols, uint32_t size, uint32_t* out);
  void plan_fri_layout(struct ProofRun& r, int ls0, int smallest_quot_log);   // phase_fri.cpp
  void plan_fri_buffers(struct ProofRun& r);   // phase_fri.cpp
  void plan_sample_points(struct ProofRun& r);   // phase_oods.cpp
  void plan_eval_jobs(struct ProofRun& r);       // phase_oods.cpp
  void plan_oods_step(struct ProofRun& r, ChanStep& step);   // phase_oods.cpp: ChanStep kind 3 for the composition tree's root
  QuotientArgs make_quotient_args(int ls, const std::vector<const uint32_t*>& cols,
                                  const std::vector<std::vector<std::pair<int, QM31>>>& samples,
                                  const std::vector<QPt>& points, QM31 quot_alpha, bool alloc_out = true);
  // split: a sharded proof evaluates 1/world of every polynomial's coefficient chunks per rank and all-gathers the
  // partial sums (16 B per sample and rank)
  // d_maps (device, n_points x max(max_log, EVAL_LB) mappings, written by the ChanStep of kind 3) replaces `points` when given
  // d_jobs (device copy of `jobs`, already in place) saves the upload
  std::vector<QM31> eval_at_points(const std::vector<EvalJob>& jobs, const std::vector<QPt>& points, int max_log,
                                   bool split = false, const QM31* d_maps = nullptr, int n_points = 0,
                                   const EvalJob* d_jobs = nullptr, const QM31** device_out = nullptr);

  // pinned host staging (bump allocator, reset per proof): async H2D sources / D2H targets
  void begin_op();
  void set_device();
  void reset_event_log();
  void* pin_alloc(size_t bytes);
  void* stage_upload(const void* host, size_t bytes);           // -> device pointer (arena), async
  // Several small uploads as ONE transfer: between stage_group_begin and stage_group_end, stage_upload places its data
  // in a block reserved up front (same offsets on both sides) and nothing is transferred until the group ends.  What
  // does not fit the reservation is uploaded on its own as before.
  void stage_group_begin(size_t reserve_bytes);
  void stage_group_end();
  // a page-locked block that kernels write their (small) results into directly: no transfer behind the kernel, valid
  // after the next wait.  Unsharded proofs; the pointer is a device pointer as well (gather's entry table already
  // relies on that)
  void* result_block(size_t bytes) { return pin_alloc(bytes ? bytes : 4); }
  const void* stage_download(const void* dev, size_t bytes);    // -> pinned host pointer, valid after sync
  template <class T>
  T* upload_vec(const std::vector<T>& v) {
    return (T*)stage_upload(v.data(), v.size() * sizeof(T));
  }
  void fetch_root_async(DevMerkle& m);   // m.root_pinned valid after the next sync
  void eval_begin(int32_t* minmax);   // selects the device; the range words start at (INT32_MAX, INT32_MIN), on the stream
  uint32_t* bad_flag_ = nullptr;  // two device words: [0] marked when a trace table holds a non-canonical M31 word, [1] trace_lut's;
                                  // behind them the CHANGED_WORDS words of the comparing transposes (trace reuse)
  uint32_t bad_epoch_ = 1;        // the mark of the current unsharded proof (see Context::prove)
  // Trace reuse (phase_trace.cpp run_main_trace): where the previous proof left the evaluation, coefficient and LDE blocks
  // of its main trace.  The arena is not cleared between proofs and a pie of the same shape gets the same addresses, so a
  // column that is bit-identical to the previous proof's needs no transform.  The record may be trusted only while `valid`
  // (that proof enqueued its whole main-trace phase) and nobody but the next proof's own reset has started over in the
  // arena since (`generation`); `live` is that verdict, formed by run_setup and consumed by run_main_trace.
  struct TraceReuse {
    struct Table {
      int kind, log_size, n_cols;
      uint64_t n_rows;   // (where the padding begins: another count is another table, compared with nothing)
      const uint32_t *evals, *coeffs, *lde;
      // back-off: consecutive compared proofs of this table in which not one candidate column was unchanged.  From
      // REUSE_BACKOFF on the table is not compared - a context that proves another graph every time would pay for the
      // comparison (1.1 % proofs/s at 2^20 rows, profiles/trace_reuse_ab.json) and gain nothing - and the count goes on with
      // every proof; each time it reaches a multiple of REUSE_RETRY the table is compared once more, and a single unchanged
      // column ends the back-off.  Another signature (kind, sizes, addresses) starts from zero.
      int misses;
    };
    static constexpr int REUSE_BACKOFF = 2, REUSE_RETRY = 64;
    std::vector<Table> tables;
    bool valid = false, live = false;
    uint64_t generation = 0;
  } reuse_;
  uint64_t reuse_counters_[2] = {0, 0};   // counter() 20, 21
  uint64_t quot_counters_[2] = {0, 0};    // counter() 22, 23: run_oods's device path, and its host wait under the device transcript
  void account_trace_reuse(struct ProofRun& r, const uint32_t* changed_words);   // phase_trace.cpp
  char* pin_base_ = nullptr;
  size_t pin_cap_ = 0, pin_off_ = 0;
  char *grp_pin_ = nullptr, *grp_dev_ = nullptr;   // open upload group (stage_group_begin)
  size_t grp_cap_ = 0, grp_off_ = 0;

  struct Shard {
    bool active = false;
    uint32_t rank = 0, world = 1;
    int g = 0;             // log2(world)
    int fri_min_log = 16;  // FRI layers / quotient columns of at most 2^fri_min_log rows are replicated
    lmn_collective coll{};
    void* rccl = nullptr;  // built-in RCCL transport (RcclTransport in prover.cpp)
  } shard_;
  uint32_t block_rows(int log) const { return 1u << (log - shard_.g); }  // rows of a 2^log column held per rank

  int device_;
  lmn_stream_t stream_{};
  bool owns_stream_ = true;
  // proof of work: prove() grinds on the device from pow_bits >= pow_device_min_bits_ on (LMN_POW_DEVICE_MIN_BITS), on the
  // host below; one launch examines at most 2^pow_window_log_ nonces (LMN_POW_WINDOW_LOG)
  int pow_device_min_bits_ = 0, pow_window_log_ = 0;
  unsigned long long* pow_best_ = nullptr;   // device: the smallest passing nonce found so far (allocated on first use)
  uint64_t grind(const Channel& ch, uint32_t pow_bits);          // the proof's path: device or host by pow_device_min_bits_
  uint64_t device_grind(const Channel& ch, uint32_t pow_bits);
  // device_grind's rounds from nonce `base` on (every nonce below it has been examined and fails)
  uint64_t device_grind_from(const PowWords& w, bool kat, uint32_t pow_bits, uint64_t base);
  int grind_window_log(uint32_t pow_bits) const;   // the window of device_grind's launches
  uint64_t counters_[4] = {0, 0, 0, 0};            // counter()
  uint64_t open_counters_[3] = {0, 0, 0};          // counter() 13 .. 15
  uint64_t dev_open_counters_[2] = {0, 0};         // counter() 11, 12: proofs opened by the device plan, fallbacks among them
  uint64_t verify_counters_[4] = {0, 0, 0, 0};     // counter() 16 .. 19
  // verify_many's block, page-locked (staged words | verdicts) and on the device; grown on demand, never the arena
  char *vm_host_ = nullptr, *vm_dev_ = nullptr;
  size_t vm_host_cap_ = 0, vm_dev_cap_ = 0;
  // grind_many's rounds; its tables (digests | best | pending, device and page-locked host) grow on demand
  uint64_t grind_rounds(const PowWords* w, uint32_t n, bool kat, uint32_t pow_bits, uint64_t* nonces);
  char *pow_many_dev_ = nullptr, *pow_many_host_ = nullptr;
  uint32_t pow_many_cap_ = 0;
#ifdef LMN_BATCH
  static uint64_t grind_collective(void* arg, const BatchCollectiveItem* items, int n_items, hipStream_t s);
#endif
  bool merkle_cut_ = false;       // inside prove() of an unsharded proof: trees are stored without their register levels
  Arena arena_;
  int tw_max_log_ = 0;
  // twiddle tables: Y[m] (m>=1), X[k] (k>=2), forward + inverse, device pointers
  std::vector<uint32_t*> twY_, twX_, itwY_, itwX_;
  std::vector<uint32_t*> twY2_, twX2_, itwY2_, itwX2_;  // the same tables, entries doubled (TwPtrs::d)
  std::vector<void*> tw_allocs_;
  std::shared_ptr<void> tw_shared_;   // the device's twiddle set, shared by the contexts of a process (prover.cpp)
  friend struct StageTimer;
};

}  // namespace lmn
