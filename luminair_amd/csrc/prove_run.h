// State of one proof while Context::prove walks its phases (prove.cpp drives; the phases live in phase_*.cpp).
// The phases read and write it through LMN_RUN_ALIASES, so their bodies read like the single function they were
// carved out of.  Not part of any boundary.
#pragma once
#include "prover_internal.h"

namespace lmn {

struct TableInfo {
  const ComponentSpec* spec;
  uint64_t n_rows;
  int log_size;
  const uint32_t* rows;
  bool on_device;
  bool cols_on_device = false;   // LMN_TABLE_COLS_ON_DEVICE: `rows` = a finished row sink's padded columns, 2^log_size apart
};

// ---- The prover's input rules: which pie and which settings it takes.  Stated once (bodies in prove.cpp) for lmn_prove
// (run_setup, run_preprocessed), lmn_trace_check and lmn_settings_prepare (build_prepared).
// How a broken rule is answered: lmn_prove throws the rule's text as it is, lmn_trace_check names the table in front of it
// ("table T (kind K): ").  Only ever called on the refusing path: nothing is built where a pie is accepted.
struct Refusal {
  const lmn_table* named = nullptr;   // the pie whose tables the text names; null: the bare text
  [[noreturn]] void operator()(size_t t, int code, const std::string& why) const;
};
// log size of the padded table: the smallest power of two >= n_rows, and at least 2^4
inline int padded_log(uint64_t n_rows) {
  int ls = 4;
  while ((1ull << ls) < n_rows) ++ls;
  return ls;
}
// The rules on the tables, in table order; a row-sink table's columns are attached to `stream` (rows_sink_attach) when the
// table has passed, before the next one is looked at.  Fills `infos`, returns the largest log size.
int scan_tables(const lmn_table* tables, size_t n_tables, const lmn_config& cfg, bool sharded, int device, lmn_stream_t stream,
                const Refusal& refuse, std::vector<TableInfo>& infos);
uint32_t lookups_present(const std::vector<TableInfo>& infos);   // LMN_LOOKUP_* bits of the lookup tables in the pie
struct Luts {
  const lmn_lut* of[3] = {nullptr, nullptr, nullptr};   // by LMN_LUT_* kind
};
Luts parse_luts(const lmn_settings* settings);           // no null pointer, unknown kind, null column or kind given twice
Luts luts_for_pie(const lmn_settings* settings, const std::vector<TableInfo>& infos);   // and no lookup announced without its table
// the rules on one lookup table's size: 256 rows for the range check, the rows of its LUT (which the settings must carry)
// otherwise.  Returns that LUT; null for the range check and for a component without preprocessed columns.
const lmn_lut* lut_for_table(size_t t, const ComponentSpec& spec, int log_size, const Luts& luts, const Refusal& refuse);
uint64_t first_noncanonical(const uint32_t* words, uint64_t n);   // index of the first word >= 2^31 - 1; n: all are canonical

// one FRI quotient column (the columns of one LDE size accumulated)
struct Quot {
  int log;
  uint32_t* vals;  // 4 x 2^log, or 4 x 2^(log-g) (this rank's rows) when sharded
  bool sharded;
};
// one committed inner FRI layer
struct FriLayer {
  int log;
  uint32_t* vals;  // 4 x 2^log (line evaluation), or this rank's 4 x 2^(log-g) rows when sharded
  bool sharded;
  DevMerkle merkle;
};

// The close of the FRI transcript as a device chain (phase_fri.cpp enqueue_fri_close / finish_fri_close): what was
// enqueued, and - after the wait and the host's replay - what it found.  prove() and lmn_col_fri_close share it.
struct FriClose {
  bool on = false;
  int log_n = 0;                        // the last layer: 2^log_n values (log_last_layer + log_blowup)
  uint32_t n_queries = 0, log_query_domain = 0;
  bool kat = false;                     // the form the grind examines (k_grind_many<KAT>)
  int window_log = 0;                   // device_grind's window: POW_WINDOWS_PER_WAIT of them are queued
  FriCloseState* d_state = nullptr;
  const uint32_t* h_block = nullptr;    // page-locked result block (FriCloseHeader | positions | coefficients)
  // results
  bool found = false;                   // a nonce lay in the queued windows
  std::vector<QM31> coeffs;             // the first 2^log_last_layer
  uint32_t first_bad = 0xffffffffu;
  uint64_t nonce = 0;
  uint64_t grind_waits = 0;             // host waits spent grinding behind the chain's own wait (the fallback)
  std::vector<uint32_t> positions;
  Hash32 digest_after_coeffs{}, digest_after_nonce{};
  uint32_t n_sent_end = 0;
};

// The openings planned and fetched on the device behind k_fri_queries (phase_decommit.cpp enqueue_device_decommit,
// LMN_DEVICE_DECOMMIT=1): what was queued; the page-locked block holds OpenHeader | item headers | the lists.
struct DevOpen {
  bool on = false;
  uint32_t n_items = 0;
  const char* h_block = nullptr;
  size_t head_bytes = 0;
  uint64_t cap_words = 0;
};

struct ProofRun {
  explicit ProofRun(uint32_t protocol_flags) : channel(protocol_flags) {}
  // inputs (borrowed)
  const lmn_table* tables = nullptr;
  size_t n_tables = 0;
  const lmn_settings* settings = nullptr;
  const Prepared* prepared = nullptr;   // settings prepared once: tree 0 is read from it (run_preprocessed, run_decommit)
  // set-up
  int lb = 0, n_slots = 0, comp_log = 0;
  HostMarks hm;
  EventLog* log = nullptr;
  std::vector<TableInfo> infos;
  Channel channel;
  Proof proof;
  std::unique_ptr<StageTimer> total_guard;
  // commitments: preprocessed, main trace, interaction trace, composition
  DevTree tree0, tree1, tree2, tree3;
  DevTree* trees[4] = {&tree0, &tree1, &tree2, &tree3};
  std::vector<Instance> inst;
  std::vector<uint32_t*> pre_evals;  // tree-0 columns on their trace domain (logup denominators)
  RelElems elems;
  QM31 comp_alpha{};
  // Device-resident Fiat-Shamir of the commitment phases (unsharded proofs): the host enqueues everything up to the
  // sampled values without waiting; the k_chan_* kernels do the transcript steps in between and report back through
  // `d_report`, which the host reads at its first wait (run_oods) to replay and cross-check the same steps.
  bool dev_fs = false;
  DevChannel* d_chan = nullptr;
  DevReport* d_report = nullptr;
  const DevReport* h_report = nullptr;   // page-locked copy, valid after the wait in run_oods
  QM31* d_coeff = nullptr;               // 16 constraint-slot coefficients per component
  QM31* d_maps = nullptr;                // point mappings for launch_eval_tables
  std::vector<EvalJob> eval_jobs;        // one per (column, sample point), sampled_values order (plan_eval_jobs)
  EvalJob* d_eval_jobs = nullptr;        // device copy made by the OODS step's workgroup (device-resident transcript)
  uint32_t bad_mark = 0;                 // this proof's mark of the non-canonical-word verdict
  // trace reuse: the tables whose transforms got a skip argument - their changed[] words, candidate columns and size; the
  // words come back with the verdict and say what was skipped (Context::account_trace_reuse)
  struct ReuseTable {
    uint32_t first_word, candidate_mask;
    int log_size;
    size_t table;   // its place in the context's record
  };
  std::vector<ReuseTable> reuse_tables;
  // Unsharded proofs go on without the sampled values as well (round 6): k_quot_prepare mixes them, draws the quotient
  // randomness and writes the quotient kernels' tables on the device; the host's first wait is the one for the FRI results,
  // where it replays everything from root 1 on (finish_oods_on_host).  LMN_HOST_QUOT=1 keeps the wait in run_oods.
  bool quot_dev = false;
  const QM31* h_vals = nullptr;          // page-locked: the sampled values (eval_jobs order) + the device's quotient randomness
  std::vector<QuotientArgs> qargs;       // the quotient launches, one per LDE size (descending), laid out by run_oods
  // OODS: point 0 = the OODS point, then per trace size the point one trace step before it (plan_sample_points)
  std::map<int, int> prev_point_of_log;
  std::vector<Pt> neg_step;
  QPt oods{};
  std::vector<QPt> points;
  std::vector<std::vector<std::vector<int>>> spoints;     // sample point indices per tree / column, sampled_values order
  std::vector<std::vector<std::vector<QM31>>> sampled;
  // FRI
  QM31 quot_alpha{};
  bool sh = false;   // sharded proof
  int g = 0;         // log2 ranks
  int fri_T = 0;     // quotient columns / layers of more than 2^fri_T rows are split into row blocks
  std::vector<int> sizes;   // LDE log sizes present, descending
  std::vector<Quot> quots;
  DevMerkle first_merkle;
  std::vector<ColRef> first_cols;
  std::vector<FriLayer> inner;
  // What the FRI commit loop reads from and leaves on the device, laid out before the quotient kernels are launched
  // (plan_fri_buffers) so that its tables travel in the quotient phase's one upload and its results come back in one
  // download: roots | alphas | last layer in one block; the device channel's start state; for unsharded proofs the
  // layers of the single-block tail (k_fri_tail) with their trees and the table that names them.
  struct FriPlan {
    int max_layers = 0, last_size_log = 0;
    uint32_t* d_out = nullptr;      // max_layers x 8 root words | max_layers x QM31 alphas | 4 x 2^last_size_log last layer
    uint32_t* d_roots = nullptr;
    QM31* d_alphas = nullptr;
    uint32_t* d_last = nullptr;
    size_t out_bytes = 0;
    DevChannel* d_chan = nullptr;
    int tail_log = -1;              // first layer of the tail (-1: none planned)
    uint32_t* tail_first = nullptr; // that layer's values
    std::vector<FriLayer> tail_layers;
    std::vector<FriTailLayer> tail_table;   // host copy, staged by plan_fri_buffers
    FriTailLayer* d_tail = nullptr;
    int planned_ls0 = -1;           // plan_fri_layout ran for a first layer of this size
    std::vector<uint32_t> forms;    // per layer (inner layers, then the last): LMN_FRI_FOLD_* | LMN_FRI_TREE_* the loop took
  } fri;
  std::vector<QM31> last_vals;
  int last_log = 0;
  FriClose close;   // on: the transcript is closed on the device, in front of the FRI wait
  DevOpen open;     // on: the openings are planned and fetched there as well
  std::vector<uint32_t> queries;
  std::map<int, std::vector<uint32_t>> pos_by_log;
  bool sharded_log(int lg) const { return sh && lg > fri_T; }
  ProofRun(const ProofRun&) = delete;
  ProofRun& operator=(const ProofRun&) = delete;
};

// shared by the host's and the device's close of the transcript (phase_fri.cpp, phase_decommit.cpp)
std::vector<QM31> interpolate_last_layer(const std::vector<QM31>& last_vals, int last_log);
// the words one nonce is hashed with: the channel's digest, or its prefixed digest in the prefixed form
PowWords pow_words_of(const Channel& ch, uint32_t pow_bits, bool& kat);

// the four coordinate columns of a secure column as tree columns
inline void secure_columns(const uint32_t* vals, int lg, bool s, int g, std::vector<ColRef>& out) {
  const uint64_t stride = s ? (1ull << (lg - g)) : (1ull << lg);
  for (int k = 0; k < 4; ++k) out.push_back({vals + (uint64_t)k * stride, lg, s});
}

#define LMN_RUN_ALIASES(r)                                                                                              \
  HostMarks& hm = (r).hm; EventLog* const log = (r).log; const int lb = (r).lb, n_slots = (r).n_slots; int& comp_log = (r).comp_log; \
  std::vector<TableInfo>& infos = (r).infos; Channel& channel = (r).channel; Proof& proof = (r).proof;                  \
  DevTree &tree0 = (r).tree0, &tree1 = (r).tree1, &tree2 = (r).tree2, &tree3 = (r).tree3; DevTree* (&trees)[4] = (r).trees; \
  std::vector<Instance>& inst = (r).inst; std::vector<uint32_t*>& pre_evals = (r).pre_evals; RelElems& elems = (r).elems; \
  QM31& comp_alpha = (r).comp_alpha; QPt& oods = (r).oods; std::vector<QPt>& points = (r).points;                       \
  std::vector<std::vector<std::vector<int>>>& spoints = (r).spoints;                                                    \
  std::vector<std::vector<std::vector<QM31>>>& sampled = (r).sampled; QM31& quot_alpha = (r).quot_alpha;                \
  bool& sh = (r).sh; int &g = (r).g, &fri_T = (r).fri_T; std::vector<int>& sizes = (r).sizes;                           \
  std::vector<Quot>& quots = (r).quots; DevMerkle& first_merkle = (r).first_merkle;                                     \
  std::vector<ColRef>& first_cols = (r).first_cols; std::vector<FriLayer>& inner = (r).inner;                           \
  std::vector<QM31>& last_vals = (r).last_vals; int& last_log = (r).last_log; std::vector<uint32_t>& queries = (r).queries; \
  std::map<int, std::vector<uint32_t>>& pos_by_log = (r).pos_by_log;                                                    \
  (void)hm; (void)log; (void)lb; (void)n_slots; (void)comp_log; (void)infos; (void)channel; (void)proof; (void)tree0;   \
  (void)tree1; (void)tree2; (void)tree3; (void)trees; (void)inst; (void)pre_evals; (void)elems; (void)comp_alpha;       \
  (void)oods; (void)points; (void)spoints; (void)sampled; (void)quot_alpha; (void)sh; (void)g; (void)fri_T; (void)sizes; \
  (void)quots; (void)first_merkle; (void)first_cols; (void)inner; (void)last_vals; (void)last_log; (void)queries;       \
  (void)pos_by_log

}  // namespace lmn
