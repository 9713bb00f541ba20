// Level-2 ops on device handles (include/luminair_hip.h, `lmn_col_*` / `lmn_tree_*`): the stwo `Backend`-shaped
// surface a Rust `HipBackend` would bind (/root/reference/crates/prover/src/prover.rs:38-46,312,
// /root/reference/crates/air/src/utils.rs:112-128).  Columns live in HBM from lmn_col_from_cpu to lmn_col_to_cpu;
// every op is one or a few launches of the same gfx950 kernels `lmn_prove` uses, on the context's stream.
#include "capi_internal.h"
#include "prove_run.h"

#include <algorithm>

struct lmn_col {
  uint32_t* d;
  uint32_t ncols, log_size;
  bool view = false;  // aliases columns of another handle (lmn_col_view): does not own `d`
  uint64_t words() const { return (uint64_t)ncols << log_size; }
};
struct lmn_tree {
  uint32_t* slab;                 // all layers, root first
  std::vector<uint32_t*> layers;  // layers[k]: 2^k hashes
  int max_log;
  lmn::Hash32 root;
  std::vector<uint32_t> ncols_of_log;  // [log]: how many columns of 2^log rows it was committed from (lmn_tree_decommit)
};

struct lmn_positions {
  uint32_t* d;          // word 0: their number; words 1 .. 1024: the positions (k_open_plan's input)
  uint32_t log_domain;
  uint32_t n;           // what the host knows of their number: an upper bound for sizing, exact once a wait has passed
};

namespace lmn {

constexpr uint32_t COL_MAX_LOG = 27;  // 2^26-row traces have 2^27-row LDEs

static lmn_col* new_col(uint32_t ncols, uint32_t log_size) {
  if (ncols == 0 || ncols > 4096 || log_size > COL_MAX_LOG)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "column handle: bad shape");
  lmn_col* c = new lmn_col{nullptr, ncols, log_size, false};
  try {
    c->d = (uint32_t*)lmn_dev_malloc(c->words() * 4);
  } catch (const LmnError& e) {
    delete c;
    throw LmnError(LMN_ERR_OUT_OF_MEMORY, std::string("column allocation failed: ") + e.what());
  }
  return c;
}

// field words crossing the C ABI must be canonical M31 (< 2^31 - 1), as the verifier enforces for proof bytes
static void check_canonical(const uint32_t* w, uint64_t n, const char* what) {
  for (uint64_t i = 0; i < n; ++i)
    if (w[i] >= P31) throw LmnError(LMN_ERR_INVALID_ARGUMENT, std::string(what) + " is not a canonical M31 word");
}

// frees a freshly allocated handle when the op that fills it throws
struct ColGuard {
  lmn_col* c;
  explicit ColGuard(lmn_col* c_) : c(c_) {}
  ~ColGuard() {
    if (c) {
      lmn_dev_free(c->d);
      delete c;
    }
  }
  lmn_col* release() {
    lmn_col* r = c;
    c = nullptr;
    return r;
  }
};

lmn_col* Context::col_alloc(uint32_t ncols, uint32_t log_size, bool zero) {
  set_device();
  ColGuard c(new_col(ncols, log_size));
  if (zero) lmn_memset(c.c->d, 0, c.c->words() * 4, stream_);
  return c.release();
}
lmn_col* Context::col_from_cpu(const uint32_t* host, uint32_t ncols, uint32_t log_size) {
  set_device();
  ColGuard c(new_col(ncols, log_size));
  lmn_h2d(c.c->d, host, c.c->words() * 4, stream_);
  lmn_sync(stream_);  // the host buffer is borrowed only for the duration of the call
  return c.release();
}
void Context::col_to_cpu(const lmn_col* c, uint32_t* host) {
  set_device();
  lmn_d2h(host, c->d, c->words() * 4, stream_);
  lmn_sync(stream_);
}
void Context::col_free(lmn_col* c) {
  if (!c) return;
  if (c->view) {
    delete c;
    return;
  }
  set_device();
  lmn_sync(stream_);  // stream-ordered ops may still read it
  lmn_dev_free(c->d);
  delete c;
}
lmn_col* Context::col_view(const lmn_col* c, uint32_t first, uint32_t n) {
  if (n == 0 || first >= c->ncols || n > c->ncols - first) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "view: column range out of bounds");
  return new lmn_col{c->d + ((uint64_t)first << c->log_size), n, c->log_size, true};
}

void Context::col_bit_reverse(lmn_col* c) {
  set_device();
  launch_bit_reverse(c->d, 1ull << c->log_size, (int)c->ncols, (int)c->log_size, stream_);
}
void Context::col_precompute_twiddles(uint32_t log_size) {
  set_device();
  if (log_size > COL_MAX_LOG) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "precompute_twiddles: log size too large");
  ensure_twiddles((int)log_size);
}
void Context::col_interpolate(lmn_col* c) {
  set_device();
  if (c->log_size < 1) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "interpolate: log_size < 1");
  ensure_twiddles((int)c->log_size);
  const uint64_t n = 1ull << c->log_size;
  launch_ifft(c->d, n, c->d, n, (int)c->ncols, (int)c->log_size, itw((int)c->log_size), stream_);
}
lmn_col* Context::col_evaluate(const lmn_col* co, uint32_t log_domain) {
  set_device();
  if (log_domain < co->log_size || log_domain < 1) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "evaluate: domain smaller than the polynomial");
  lmn_col* out = new_col(co->ncols, log_domain);
  try {
    ensure_twiddles((int)log_domain);
    launch_fft(out->d, 1ull << log_domain, co->d, 1ull << co->log_size, (int)co->log_size, (int)co->ncols, (int)log_domain,
               tw((int)log_domain), stream_);
  } catch (...) {
    col_free(out);
    throw;
  }
  return out;
}
lmn_col* Context::col_evaluate_block(const lmn_col* co, uint32_t log_domain, uint32_t log_blocks, uint32_t block) {
  set_device();
  if (log_domain < co->log_size) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "evaluate_block: domain smaller than the polynomial");
  if (log_blocks < 1 || log_blocks > 3 || log_blocks >= log_domain || block >= (1u << log_blocks))
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "bad block specification");
  const uint32_t lb = log_domain - log_blocks;
  lmn_col* out = new_col(co->ncols, lb);
  try {
    ensure_twiddles((int)log_domain);
    launch_fft_block(out->d, 1ull << lb, co->d, 1ull << co->log_size, (int)co->log_size, (int)co->ncols, (int)log_domain,
                     (int)log_blocks, block, tw((int)log_domain), stream_);
  } catch (...) {
    col_free(out);
    throw;
  }
  return out;
}
lmn_col* Context::col_extend(const lmn_col* co, uint32_t log_size) {
  set_device();
  if (log_size < co->log_size) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "extend: target smaller than the polynomial");
  ColGuard out(new_col(co->ncols, log_size));
  launch_extend(co->d, 1ull << co->log_size, (int)co->log_size, out.c->d, 1ull << log_size, (int)log_size, (int)co->ncols, stream_);
  return out.release();
}
void Context::col_eval_at_point(const lmn_col* co, uint32_t column, const uint32_t pt[8], uint32_t out[4]) {
  check_canonical(pt, 8, "eval_at_point: point");
  if (column >= co->ncols) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "eval_at_point: column index out of range");
  arena_.reserve(8u << 20);
  begin_op();
  std::vector<QM31> r = eval_at_points({{co->d + ((uint64_t)column << co->log_size), (int)co->log_size, 0}}, {qpt_words(pt)},
                                       (int)co->log_size);
  store_words(out, r[0]);
}

// frees a tree handle (and its device slab) when the op that fills it throws
struct TreeGuard {
  lmn_tree* t;
  explicit TreeGuard(lmn_tree* t_) : t(t_) {}
  ~TreeGuard() {
    if (t) {
      if (t->slab) lmn_dev_free(t->slab);
      delete t;
    }
  }
  lmn_tree* release() {
    lmn_tree* r = t;
    t = nullptr;
    return r;
  }
};

lmn_tree* Context::col_commit(const lmn_col* const* cols, uint32_t n) {
  set_device();
  std::vector<ColRef> sorted;
  uint32_t max_log = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const lmn_col* c = cols[k];
    if (!c) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "commit: null column handle");
    for (uint32_t j = 0; j < c->ncols; ++j) sorted.push_back({c->d + ((uint64_t)j << c->log_size), (int)c->log_size, false});
    max_log = std::max(max_log, c->log_size);
  }
  if (sorted.empty()) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "commit: no columns");
  std::stable_sort(sorted.begin(), sorted.end(), [](auto& a, auto& b) { return a.log > b.log; });
  // the tree is hashed in the arena, then its layers move to a slab the handle owns
  arena_.reserve((16ull << max_log) * 4 + (4u << 20));
  begin_op();
  reset_event_log();
  DevMerkle m;
  build_merkle(m, sorted);
  TreeGuard tg(new lmn_tree{nullptr, {}, m.max_log, {}});
  lmn_tree* t = tg.t;
  try {
    t->slab = (uint32_t*)lmn_dev_malloc((16ull << m.max_log) * 4);
  } catch (const LmnError& e) {
    throw LmnError(LMN_ERR_OUT_OF_MEMORY, std::string("tree allocation failed: ") + e.what());
  }
  t->layers.assign(m.max_log + 1, nullptr);
  uint64_t off = 0;
  for (int l = 0; l <= m.max_log; ++l) {
    t->layers[l] = t->slab + off;
    lmn_d2d(t->layers[l], m.layers[l], (32ull << l), stream_);
    off += 8ull << l;
  }
  t->ncols_of_log.assign(m.max_log + 1, 0u);
  for (const ColRef& c : sorted) t->ncols_of_log[c.log]++;
  fetch_root_async(m);
  lmn_sync(stream_);
  m.finish_root();
  t->root = m.root;
  return tg.release();
}
void Context::tree_layer_to_cpu(const lmn_tree* t, uint32_t layer_log, uint8_t* out) {
  set_device();
  if ((int)layer_log > t->max_log) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "tree: no such layer");
  lmn_d2h(out, t->layers[layer_log], 32ull << layer_log, stream_);
  lmn_sync(stream_);
}
void Context::tree_free(lmn_tree* t) {
  if (!t) return;
  set_device();
  lmn_sync(stream_);
  lmn_dev_free(t->slab);
  delete t;
}

// ---- decommitment on the device (lmn_tree_decommit, lmn_col_gather): the host decides WHICH nodes an opening needs, one
// launch fetches them from the tree's slab and the column handles, one transfer brings them back.
constexpr size_t OPENING_MAX_BYTES = 12u << 20;   // of the plan and of the result, each: what the context's staging carries

static std::string u32s(uint64_t v) { return std::to_string(v); }

// MerkleProver::decommit's walk (openings.h walk_openings) as entries of the launch's plan.  The pointer table: layers
// 0 .. max_log, then the columns in tree order.
namespace {
struct OpeningPlan {
  std::vector<DecommitEntry> hashes, values, witness;
  uint32_t col_src0;
  bool child(int layer, uint32_t child, bool opened) {
    if (!opened) hashes.push_back({(uint32_t)layer, child});
    return true;
  }
  bool column(uint32_t col, uint32_t node, bool queried) {
    (queried ? values : witness).push_back({col_src0 + col, node});
    return true;
  }
  bool node(int, uint32_t) { return true; }
};
}  // namespace
static OpeningPlan plan_opening(int max_log, const std::vector<uint32_t>& ncols_of_log, const std::vector<Positions>& queries_of_log) {
  OpeningPlan pl{{}, {}, {}, (uint32_t)max_log + 1};
  walk_openings(max_log, ncols_of_log.data(), queries_of_log.data(), pl);
  return pl;
}

// The handles of an opening call must be the columns the tree was committed from: as many at each size.  -> the columns
// in tree order.  `A` names the argument in the refusals; also(log, n): the caller's own rule for a size's n columns.
template <class Refuse, class Also>
static std::vector<ColRef> columns_as_committed(const lmn_tree* t, const lmn_col* const* cols, uint32_t n_cols, const std::string& A,
                                                Refuse&& refuse, Also&& also) {
  const int max_log = t->max_log;
  std::vector<ColRef> sorted;
  std::vector<uint32_t> have(max_log + 1, 0u);
  for (uint32_t k = 0; k < n_cols; ++k) {
    const lmn_col* c = cols[k];
    if (!c) refuse(A + "[" + u32s(k) + "] is null");
    if ((int)c->log_size > max_log)
      refuse(A + "[" + u32s(k) + "] has log size " + u32s(c->log_size) + ", the tree's is " + u32s(max_log));
    for (uint32_t j = 0; j < c->ncols; ++j) sorted.push_back({c->d + ((uint64_t)j << c->log_size), (int)c->log_size, false});
    have[c->log_size] += c->ncols;
  }
  for (int log = max_log; log >= 0; --log) {
    if (have[log] != t->ncols_of_log[log])
      refuse(A + " holds " + u32s(have[log]) + " columns of log size " + u32s(log) + ", the tree was committed from " +
             u32s(t->ncols_of_log[log]));
    also(log, have[log]);
  }
  std::stable_sort(sorted.begin(), sorted.end(), [](auto& a, auto& b) { return a.log > b.log; });
  return sorted;
}

static uint32_t* malloc_words(size_t n) {
  if (n == 0) return nullptr;
  uint32_t* p = (uint32_t*)malloc(n * 4);
  if (!p) throw std::bad_alloc();
  return p;
}

void Context::tree_decommit(const lmn_tree* t, const lmn_col* const* cols, uint32_t n_cols, const uint32_t* query_logs,
                            const uint32_t* query_counts, uint32_t n_groups, const uint32_t* queries, TreeOpening& out) {
  const char* F = "tree_decommit: ";
  auto refuse = [&](const std::string& what) { throw LmnError(LMN_ERR_INVALID_ARGUMENT, F + what); };
  if (n_cols && !cols) refuse("cols is null with n_cols = " + u32s(n_cols));
  if (n_groups && !query_logs) refuse("query_logs is null with n_groups = " + u32s(n_groups));
  if (n_groups && !query_counts) refuse("query_counts is null with n_groups = " + u32s(n_groups));
  const int max_log = t->max_log;
  const std::vector<ColRef> sorted = columns_as_committed(t, cols, n_cols, "cols", refuse, [](int, uint32_t) {});
  // the queries
  std::vector<Positions> queries_of_log(max_log + 1);
  std::vector<bool> seen(max_log + 1, false);
  uint64_t at = 0;
  for (uint32_t g = 0; g < n_groups; ++g) {
    const uint32_t log = query_logs[g], n = query_counts[g];
    if ((int)log > max_log) refuse("query_logs[" + u32s(g) + "] = " + u32s(log) + " exceeds the tree's log size " + u32s(max_log));
    if (seen[log]) refuse("query_logs[" + u32s(g) + "] repeats log size " + u32s(log));
    seen[log] = true;
    if (n && !queries) refuse("queries is null with query_counts[" + u32s(g) + "] = " + u32s(n));
    const uint32_t* q = queries + at;
    for (uint32_t i = 0; i < n; ++i) {
      if (q[i] >> log)
        refuse("queries: position " + u32s(q[i]) + " of group " + u32s(g) + " is out of range for log size " + u32s(log));
      if (i && q[i] <= q[i - 1])
        refuse("queries: group " + u32s(g) + " is not strictly ascending at index " + u32s(i) + " (" + u32s(q[i - 1]) +
               " then " + u32s(q[i]) + ")");
    }
    queries_of_log[log] = {q, n};
    at += n;
  }
  const OpeningPlan pl = plan_opening(max_log, t->ncols_of_log, queries_of_log);
  const size_t nh = pl.hashes.size(), nv = pl.values.size(), nw = pl.witness.size();
  if (nh + nv + nw == 0) return;
  const size_t n_ptrs = (size_t)max_log + 1 + sorted.size();
  const size_t plan_bytes = n_ptrs * sizeof(void*) + (nh + nv + nw) * sizeof(DecommitEntry);
  const size_t out_bytes = nh * 32 + (nv + nw) * 4;
  if (plan_bytes > OPENING_MAX_BYTES || out_bytes > OPENING_MAX_BYTES)
    refuse("queries: the opening (" + u32s(out_bytes) + " bytes, a plan of " + u32s(plan_bytes) + ") exceeds the " +
           u32s(OPENING_MAX_BYTES) + " bytes one call carries");
  arena_.reserve(std::max<size_t>(8u << 20, plan_bytes + out_bytes + (1u << 20)));
  begin_op();
  // pointer table and plan: built in page-locked staging, ONE transfer
  char* h_plan = (char*)pin_alloc(plan_bytes);
  const uint32_t** h_ptrs = (const uint32_t**)h_plan;
  for (int l = 0; l <= max_log; ++l) h_ptrs[l] = t->layers[l];
  for (size_t c = 0; c < sorted.size(); ++c) h_ptrs[max_log + 1 + c] = sorted[c].ptr;
  DecommitEntry* h_e = (DecommitEntry*)(h_plan + n_ptrs * sizeof(void*));
  if (nh) memcpy(h_e, pl.hashes.data(), nh * sizeof(DecommitEntry));
  if (nv) memcpy(h_e + nh, pl.values.data(), nv * sizeof(DecommitEntry));
  if (nw) memcpy(h_e + nh + nv, pl.witness.data(), nw * sizeof(DecommitEntry));
  char* d_plan = (char*)arena_.alloc_bytes(plan_bytes);
  uint32_t* d_out = (uint32_t*)arena_.alloc_bytes(out_bytes);
  lmn_h2d(d_plan, h_plan, plan_bytes, stream_);
  launch_tree_decommit((const uint32_t* const*)d_plan, (const DecommitEntry*)(d_plan + n_ptrs * sizeof(void*)), (uint32_t)nh,
                       (uint32_t)(nv + nw), d_out, stream_);
  const uint32_t* got = (const uint32_t*)stage_download(d_out, out_bytes);
  // the caller's buffers are allocated under the transfer
  TreeOpening o;
  try {
    o.hash_witness = (uint8_t*)malloc_words(nh * 8);
    o.queried_values = malloc_words(nv);
    o.column_witness = malloc_words(nw);
  } catch (...) {
    lmn_sync(stream_);
    free(o.hash_witness);
    free(o.queried_values);
    throw;
  }
  lmn_sync(stream_);
  if (nh) memcpy(o.hash_witness, got, nh * 32);
  if (nv) memcpy(o.queried_values, got + nh * 8, nv * 4);
  if (nw) memcpy(o.column_witness, got + nh * 8 + nv, nw * 4);
  o.n_hashes = nh;
  o.n_values = nv;
  o.n_column_words = nw;
  out = o;
}

void Context::col_gather(const lmn_col* c, const uint32_t* positions, uint32_t n, uint32_t* host_out) {
  for (uint32_t i = 0; i < n; ++i)
    if (positions[i] >> c->log_size)
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, "col_gather: positions[" + u32s(i) + "] = " + u32s(positions[i]) +
                                                   " is out of range for columns of log size " + u32s(c->log_size));
  const size_t in_bytes = (size_t)n * 4, out_bytes = (size_t)n * c->ncols * 4;
  if (in_bytes > OPENING_MAX_BYTES || out_bytes > OPENING_MAX_BYTES)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "col_gather: n = " + u32s(n) + " positions of " + u32s(c->ncols) +
                                                 " columns exceed the " + u32s(OPENING_MAX_BYTES) + " bytes one call carries");
  arena_.reserve(std::max<size_t>(8u << 20, in_bytes + out_bytes + (1u << 20)));
  begin_op();
  const uint32_t* d_pos = (const uint32_t*)stage_upload(positions, in_bytes);
  uint32_t* d_out = (uint32_t*)arena_.alloc_bytes(out_bytes);
  launch_col_gather(c->d, c->log_size, c->ncols, d_pos, n, d_out, stream_);
  const void* got = stage_download(d_out, out_bytes);
  lmn_sync(stream_);
  memcpy(host_out, got, out_bytes);
}

// ---- query positions on the device, and openings planned there (lmn_positions_*, lmn_open_queries)
static lmn_positions* new_positions(uint32_t log_domain, uint32_t n) {
  lmn_positions* p = new lmn_positions{nullptr, log_domain, n};
  try {
    p->d = (uint32_t*)lmn_dev_malloc((1 + OPEN_MAX_POSITIONS) * 4);
  } catch (const LmnError& e) {
    delete p;
    throw LmnError(LMN_ERR_OUT_OF_MEMORY, std::string("positions allocation failed: ") + e.what());
  }
  return p;
}

lmn_positions* Context::positions_from_cpu(const uint32_t* positions, uint32_t n, uint32_t log_domain) {
  const char* F = "positions_from_cpu: ";
  auto refuse = [&](const std::string& what) { throw LmnError(LMN_ERR_INVALID_ARGUMENT, F + what); };
  if (log_domain > OPEN_MAX_LOG) refuse("log_domain is " + u32s(log_domain) + ", at most " + u32s(OPEN_MAX_LOG));
  if (n > OPEN_MAX_POSITIONS) refuse("n is " + u32s(n) + ", at most " + u32s(OPEN_MAX_POSITIONS) + " positions");
  if (n && !positions) refuse("positions is null with n = " + u32s(n));
  for (uint32_t i = 0; i < n; ++i) {
    if (positions[i] >> log_domain)
      refuse("positions[" + u32s(i) + "] = " + u32s(positions[i]) + " is out of range for log_domain " + u32s(log_domain));
    if (i && positions[i] <= positions[i - 1])
      refuse("positions is not strictly ascending at index " + u32s(i) + " (" + u32s(positions[i - 1]) + " then " +
             u32s(positions[i]) + ")");
  }
  set_device();
  lmn_positions* p = new_positions(log_domain, n);
  begin_op();
  uint32_t* h = (uint32_t*)pin_alloc((1 + (size_t)n) * 4);
  h[0] = n;
  if (n) memcpy(h + 1, positions, (size_t)n * 4);
  lmn_h2d(p->d, h, (1 + (size_t)n) * 4, stream_);
  lmn_sync(stream_);   // the staging memory is the next op's
  return p;
}
void Context::positions_to_cpu(const lmn_positions* p, uint32_t* host, uint32_t* n_out) {
  set_device();
  begin_op();
  const uint32_t* got = (const uint32_t*)stage_download(p->d, (1 + OPEN_MAX_POSITIONS) * 4);
  lmn_sync(stream_);
  const uint32_t n = std::min(got[0], OPEN_MAX_POSITIONS);
  if (n) memcpy(host, got + 1, (size_t)n * 4);
  *n_out = n;
}
void Context::positions_free(lmn_positions* p) {
  if (!p) return;
  set_device();
  lmn_sync(stream_);
  lmn_dev_free(p->d);
  delete p;
}

// (prover_internal.h)  What an item's plan and output can hold at most follows from the NUMBER of positions alone (k_open_plan checks both): with m
// nodes per layer at most - the positions, doubled by the pair expansion - a layer of 2^log nodes opens min(2^log, m) of
// them, each with its column values and at most both children's hashes; a size's pairs have at most as many members
// that are no positions as there are pairs.
bool append_open_item(int max_log, uint32_t* const* layers, const std::vector<uint32_t>& ncols_of_log,
                      const std::vector<ColRef>& cols_sorted, const std::vector<MerkleCut>* cuts, uint32_t n_positions,
                      uint32_t flags, std::vector<const uint32_t*>& ptrs, std::vector<MerkleRecompute>& recompute,
                      OpenItemDesc& d, OpenTotals& tot) {
  d = OpenItemDesc{};
  memset(d.cut_of_layer, (int)OPEN_STORED, sizeof d.cut_of_layer);
  d.ent_off = (uint32_t)tot.entries;
  d.job_off = (uint32_t)tot.jobs;
  if (max_log < 0) {
    d.flags = OPEN_EMPTY;
    return true;
  }
  d.max_log = (uint32_t)max_log;
  d.flags = flags;
  const bool pairs = (flags & OPEN_FRI_PAIRS) != 0;
  const uint64_t m = pairs ? 2ull * n_positions : n_positions;
  uint64_t entries = 0, words = 0, job_cap = 0;
  d.layer_src0 = (uint32_t)ptrs.size();
  for (int l = 0; l <= max_log; ++l) {
    const uint64_t nodes = std::min<uint64_t>(1ull << l, m);
    const uint64_t hashes = l < max_log ? 2 * nodes : 0;
    const uint64_t fri = pairs && ncols_of_log[l] ? 4 * std::min<uint64_t>(std::max<uint64_t>(1ull << l, 2) / 2, n_positions) : 0;
    entries += nodes * ncols_of_log[l] + hashes + fri;
    words += nodes * ncols_of_log[l] + 8 * hashes + fri;
    d.ncols[l] = ncols_of_log[l];
    ptrs.push_back(layers[l]);
    if (layers[l] || l == 0) continue;   // (an opening reads the children's hashes: layers 1 .. max_log)
    const MerkleCut* cut = cuts ? cut_holding(*cuts, l) : nullptr;
    if (!cut) throw LmnError(LMN_ERR_INTERNAL, "merkle: layer without storage");
    if (recompute.size() >= OPEN_STORED) return false;
    d.cut_of_layer[l] = (uint8_t)recompute.size();
    recompute.push_back({cut->prev, cut->sg, cut->ncols, 1u << cut->start_log, cut->below, cut->below_ncols, 0u, 0, 0u});
    job_cap += 2 * std::min<uint64_t>(1ull << (l - 1), m);
  }
  d.col_src0 = (uint32_t)ptrs.size();
  for (auto& c : cols_sorted) ptrs.push_back(c.ptr);
  d.ent_cap = (uint32_t)std::min<uint64_t>(entries, 0xffffffffu);
  d.job_cap = (uint32_t)job_cap;
  tot.entries += entries;
  tot.jobs += job_cap;
  tot.words += words;
  tot.max_cap = std::max(tot.max_cap, entries);
  tot.max_job_cap = std::max(tot.max_job_cap, job_cap);
  return true;
}

void Context::open_queries(const lmn_positions* p, const lmn_open_item* items, uint32_t n_items, lmn_opening* out) {
  const char* F = "open_queries: ";
  auto refuse = [&](const std::string& what) { throw LmnError(LMN_ERR_INVALID_ARGUMENT, F + what); };
  if (shard_.active) refuse("ctx is sharded (lmn_ctx_set_shard): openings are planned on an unsharded context only");
  if (!p) refuse("positions is null");
  if (n_items > OPEN_MAX_ITEMS) refuse("n_items is " + u32s(n_items) + ", at most " + u32s(OPEN_MAX_ITEMS));
  if (n_items && !items) refuse("items is null with n_items = " + u32s(n_items));
  if (n_items && !out) refuse("out is null with n_items = " + u32s(n_items));
  // the items: their columns as at commit time, the pointer table, the bounds
  std::vector<const uint32_t*> ptrs;
  std::vector<OpenItemDesc> descs(n_items);
  std::vector<MerkleRecompute> none;   // a level-2 tree keeps every layer
  OpenTotals tot;
  for (uint32_t k = 0; k < n_items; ++k) {
    const lmn_open_item& it = items[k];
    const std::string I = "items[" + u32s(k) + "]";
    if (!it.tree) refuse(I + ".tree is null");
    if (it.n_cols && !it.cols) refuse(I + ".cols is null with n_cols = " + u32s(it.n_cols));
    if (it.flags & ~LMN_OPEN_FRI_PAIRS) refuse(I + ".flags = " + u32s(it.flags) + " holds an unknown flag");
    const lmn_tree* t = it.tree;
    if (t->max_log > (int)p->log_domain)
      refuse(I + ".tree has log size " + u32s(t->max_log) + ", larger than the positions' log_domain " + u32s(p->log_domain));
    const bool pairs = (it.flags & LMN_OPEN_FRI_PAIRS) != 0;
    const std::vector<ColRef> sorted = columns_as_committed(t, it.cols, it.n_cols, I + ".cols", refuse, [&](int log, uint32_t n) {
      if (pairs && n != 0 && (n != 4 || log == 0))
        refuse(I + ".flags: LMN_OPEN_FRI_PAIRS needs exactly 4 columns at each of the tree's sizes and none of log size 0; it has " +
               u32s(n) + " of log size " + u32s(log));
    });
    append_open_item(t->max_log, t->layers.data(), t->ncols_of_log, sorted, nullptr, p->n, it.flags, ptrs, none, descs[k], tot);
    if (tot.words * 4 > OPENING_MAX_BYTES || tot.entries * sizeof(OpenEntry) > 4 * OPENING_MAX_BYTES)
      refuse("items: the upper bound of the opening (" + u32s(tot.words * 4) + " bytes up to " + I + ", for " + u32s(p->n) +
             " positions) exceeds the " + u32s(OPENING_MAX_BYTES) + " bytes one call carries");
  }
  if (n_items == 0 || p->n == 0) return;   // (out is zeroed by the caller)
  const size_t head_bytes = sizeof(OpenHeader) + n_items * sizeof(OpenItemHeader);
  const size_t table_bytes = ptrs.size() * sizeof(void*) + n_items * sizeof(OpenItemDesc);
  const size_t out_bytes = head_bytes + tot.words * 4;
  set_device();
  arena_.reserve(std::max<size_t>(8u << 20, table_bytes + out_bytes + tot.entries * sizeof(OpenEntry) + (1u << 20)));
  begin_op();
  // pointer table and descriptors: ONE transfer; nothing in them depends on the positions
  char* h_tab = (char*)pin_alloc(table_bytes);
  memcpy(h_tab, ptrs.data(), ptrs.size() * sizeof(void*));
  memcpy(h_tab + ptrs.size() * sizeof(void*), descs.data(), n_items * sizeof(OpenItemDesc));
  char* d_tab = (char*)arena_.alloc_bytes(table_bytes);
  lmn_h2d(d_tab, h_tab, table_bytes, stream_);
  const uint32_t* const* d_ptrs = (const uint32_t* const*)d_tab;
  const OpenItemDesc* d_items = (const OpenItemDesc*)(d_tab + ptrs.size() * sizeof(void*));
  char* d_out = (char*)arena_.alloc_bytes(out_bytes);   // header | item headers | the lists
  OpenHeader* d_head = (OpenHeader*)d_out;
  OpenItemHeader* d_heads = (OpenItemHeader*)(d_out + sizeof(OpenHeader));
  OpenEntry* d_ent = (OpenEntry*)arena_.alloc_bytes(std::max<size_t>(tot.entries, 1) * sizeof(OpenEntry));
  // (the wrappers count the launches they make: open_counters_)
  launch_open_plan(p->d, p->d + 1, nullptr, p->log_domain, d_items, n_items, d_heads, d_ent, d_ent, stream_, &open_counters_[0]);
  launch_open_offsets(p->d, d_head, d_heads, n_items, (uint32_t)tot.words, stream_);
  launch_open_fetch(d_ptrs, (uint32_t)ptrs.size(), d_items, n_items, (uint32_t)tot.max_cap, d_head, d_heads, d_ent,
                    (uint32_t*)(d_out + head_bytes), stream_, &open_counters_[1]);
  const char* got = (const char*)stage_download(d_out, out_bytes);
  lmn_sync(stream_);
  ++open_counters_[2];
  const OpenHeader& head = *(const OpenHeader*)got;
  const OpenItemHeader* heads = (const OpenItemHeader*)(got + sizeof(OpenHeader));
  const uint32_t* words = (const uint32_t*)(got + head_bytes);
  if (head.overflow) throw LmnError(LMN_ERR_INTERNAL, "open_queries: the device plan exceeded the bounds it was launched with");
  std::vector<lmn_opening> res(n_items, lmn_opening{});
  auto release = [&] {
    for (auto& o : res) {
      free(o.queried_values);
      free(o.hash_witness);
      free(o.column_witness);
      free(o.fri_witness);
    }
  };
  try {
    for (uint32_t k = 0; k < n_items; ++k) {
      const OpenItemHeader& h = heads[k];
      uint64_t end = 0;
      for (int l = 0; l < 4; ++l) end = std::max<uint64_t>(end, (uint64_t)h.base[l] + (uint64_t)h.count[l] * (l == OPEN_LIST_HASH ? 8 : 1));
      if (end > tot.words) throw LmnError(LMN_ERR_INTERNAL, "open_queries: the device plan's counts exceed the result block");
      lmn_opening& o = res[k];
      o.n_fri_words = h.count[OPEN_LIST_FRI];
      o.n_values = h.count[OPEN_LIST_QUERIED];
      o.n_hashes = h.count[OPEN_LIST_HASH];
      o.n_column_words = h.count[OPEN_LIST_WITNESS];
      o.fri_witness = malloc_words(o.n_fri_words);
      o.queried_values = malloc_words(o.n_values);
      o.hash_witness = (uint8_t*)malloc_words(o.n_hashes * 8);
      o.column_witness = malloc_words(o.n_column_words);
      if (o.n_fri_words) memcpy(o.fri_witness, words + h.base[OPEN_LIST_FRI], o.n_fri_words * 4);
      if (o.n_values) memcpy(o.queried_values, words + h.base[OPEN_LIST_QUERIED], o.n_values * 4);
      if (o.n_hashes) memcpy(o.hash_witness, words + h.base[OPEN_LIST_HASH], o.n_hashes * 32);
      if (o.n_column_words) memcpy(o.column_witness, words + h.base[OPEN_LIST_WITNESS], o.n_column_words * 4);
    }
  } catch (...) {
    release();
    throw;
  }
  memcpy(out, res.data(), n_items * sizeof(lmn_opening));
}

// ---- the FRI commit loop on handles (lmn_col_fri_commit): prove()'s own layer loop (phase_fri.cpp fri_commit_layers) on
// caller-given quotient columns, then everything it left in device memory brought to the host
FriCommitOut::~FriCommitOut() {
  free(r.roots);
  free(r.alphas);
  free(r.tree_logs);
  free(r.level_masks);
  free(r.forms);
  free(r.values);
  free(r.levels);
}
lmn_fri_commit_result FriCommitOut::release() {
  lmn_fri_commit_result o = r;
  r = lmn_fri_commit_result{};
  return o;
}

void Context::col_fri_commit(const lmn_col* const* cols, uint32_t n, const uint8_t start_digest[32], FriCommitOut& out) {
  const char* F = "fri_commit: ";
  auto refuse = [&](const std::string& what) { throw LmnError(LMN_ERR_INVALID_ARGUMENT, F + what); };
  if (shard_.active) refuse("ctx is sharded (lmn_ctx_set_shard): the layer loop on handles runs on an unsharded context only");
  if (!cols || n == 0) refuse("cols is empty");
  if (!start_digest) refuse("start_digest is null");
  const int lb = (int)cfg.log_blowup, last_log = (int)cfg.log_last_layer + lb;
  for (uint32_t k = 0; k < n; ++k) {
    const lmn_col* c = cols[k];
    if (!c) refuse("cols[" + u32s(k) + "] is null");
    if (c->ncols != 4) refuse("cols[" + u32s(k) + "] has " + u32s(c->ncols) + " columns, a secure column has 4 coordinate columns");
    if (k && c->log_size >= cols[k - 1]->log_size)
      refuse("cols[" + u32s(k) + "] has log size " + u32s(c->log_size) + " after cols[" + u32s(k - 1) + "] of log size " +
             u32s(cols[k - 1]->log_size) + ": sizes must be strictly decreasing");
  }
  const int ls0 = (int)cols[0]->log_size;
  if (ls0 - 1 < last_log)
    refuse("cols[0] has log size " + u32s(ls0) + ": its first line layer is smaller than the last layer of log size " +
           u32s(last_log) + " (log_last_layer + log_blowup)");
  for (uint32_t k = 1; k < n; ++k)
    if ((int)cols[k]->log_size - 1 < last_log)
      refuse("cols[" + u32s(k) + "] has log size " + u32s(cols[k]->log_size) + ": it would join below the last layer of log size " +
             u32s(last_log));
  set_device();
  ensure_twiddles(ls0);
  // first tree 16 << ls0 words, line layers 4 << ls0 in all, their trees 16 << ls0 in all; tables and alignment in the slack
  arena_.reserve(((size_t)48 << ls0) * 4 + (16u << 20));
  begin_op();
  reset_event_log();
  // as in prove(): trees are stored without the levels their fused launches keep in registers
  struct CutScope {
    bool& flag;
    ~CutScope() { flag = false; }
  } cut_scope{merkle_cut_};
  // lmn_get_timings keeps describing the last proof: the loop adds to the counters as it does inside prove()
  struct TimingsScope {
    lmn_timings& t;
    lmn_timings saved;
    ~TimingsScope() { t = saved; }
  } timings_scope{timings, timings};
  merkle_cut_ = !env_set("LMN_MERKLE_FULL");
  ProofRun r(cfg.protocol_variant);
  r.lb = lb;
  r.log = g_log(this);
  Hash32 d0;
  memcpy(d0.w, start_digest, 32);
  r.channel.set_digest(d0);
  for (uint32_t k = 0; k < n; ++k) r.quots.push_back({(int)cols[k]->log_size, cols[k]->d, false});
  try {
    plan_fri_buffers(r);
    fri_commit_layers(r);
  } catch (...) {
    lmn_sync(stream_);   // launches in flight read tables in the staging memory the next op reuses
    throw;
  }
  const ProofRun::FriPlan& fp = r.fri;
  const size_t n_trees = 1 + r.inner.size();
  if (fp.forms.size() != n_trees) throw LmnError(LMN_ERR_INTERNAL, "FRI: one form per layer expected");
  auto tree_of = [&](size_t t) -> const DevMerkle& { return t == 0 ? r.first_merkle : r.inner[t - 1].merkle; };
  uint64_t n_values = 0, n_levels = 0;
  for (size_t i = 0; i < n_trees; ++i) n_values += 4ull << (ls0 - 1 - (int)i);
  for (size_t t = 0; t < n_trees; ++t)
    for (int l = 0; l <= tree_of(t).max_log; ++l)
      if (tree_of(t).layers[l]) n_levels += 8ull << l;
  lmn_fri_commit_result& o = out.r;
  o.n_trees = (uint32_t)n_trees;
  o.roots = (uint8_t*)malloc_words(n_trees * 8);
  o.alphas = malloc_words(n_trees * 4);
  o.tree_logs = malloc_words(n_trees);
  o.level_masks = malloc_words(n_trees);
  o.forms = malloc_words(n_trees + 1);
  o.values = malloc_words(n_values);
  o.levels = malloc_words(n_levels);
  o.n_value_words = n_values;
  o.n_level_words = n_levels;
  lmn_d2h(o.roots, fp.d_roots, n_trees * 32, stream_);
  lmn_d2h(o.alphas, fp.d_alphas, n_trees * 16, stream_);
  uint64_t at = 0;
  for (size_t i = 0; i < n_trees; ++i) {
    const int lg = ls0 - 1 - (int)i;
    const uint32_t* vals = i + 1 < n_trees ? r.inner[i].vals : fp.d_last;
    if (i + 1 < n_trees && r.inner[i].log != lg) throw LmnError(LMN_ERR_INTERNAL, "FRI: a layer of an unexpected size");
    lmn_d2h(o.values + at, vals, 16ull << lg, stream_);
    at += 4ull << lg;
  }
  at = 0;
  for (size_t t = 0; t < n_trees; ++t) {
    const DevMerkle& m = tree_of(t);
    o.tree_logs[t] = (uint32_t)m.max_log;
    o.level_masks[t] = 0;
    for (int l = 0; l <= m.max_log; ++l) {
      if (!m.layers[l]) continue;
      o.level_masks[t] |= 1u << l;
      lmn_d2h(o.levels + at, m.layers[l], 32ull << l, stream_);
      at += 8ull << l;
    }
  }
  // build_merkle_levels marks the cut it makes where it hands a leaf level to the launch above it (MerkleFold::below)
  bool below = false;
  for (const MerkleCut& c : r.first_merkle.cuts) below |= c.leaf_from_above;
  o.forms[0] = below ? LMN_FRI_FIRST_TREE_BELOW : LMN_FRI_FIRST_TREE;
  for (size_t i = 0; i < n_trees; ++i) o.forms[1 + i] = fp.forms[i];
  lmn_sync(stream_);
}

// ---- the close of the FRI transcript on a handle (lmn_col_fri_close): prove()'s own chain (phase_fri.cpp
// enqueue_fri_close / finish_fri_close) on a caller-given last layer and start digest
FriCloseOut::~FriCloseOut() {
  free(r.coeffs);
  free(r.positions);
}
lmn_fri_close_result FriCloseOut::release() {
  lmn_fri_close_result o = r;
  r = lmn_fri_close_result{};
  return o;
}

void Context::col_fri_close(const lmn_col* last_layer, const uint8_t start_digest[32], uint32_t log_query_domain,
                            FriCloseOut& out, lmn_positions** keep) {
  const char* F = "fri_close: ";
  auto refuse = [&](const std::string& what) { throw LmnError(LMN_ERR_INVALID_ARGUMENT, F + what); };
  if (shard_.active) refuse("ctx is sharded (lmn_ctx_set_shard): the transcript is closed on an unsharded context only");
  if (!last_layer) refuse("last_layer is null");
  if (!start_digest) refuse("start_digest is null");
  if (log_query_domain > 31) refuse("log_query_domain is " + u32s(log_query_domain) + ", at most 31");
  const int last_log = (int)cfg.log_last_layer + (int)cfg.log_blowup;
  if (last_layer->ncols != 4 || (int)last_layer->log_size != last_log)
    refuse("last_layer has " + u32s(last_layer->ncols) + " columns of log size " + u32s(last_layer->log_size) +
           ": the last layer is 4 coordinate columns of log size " + u32s(last_log) + " (log_last_layer + log_blowup)");
  set_device();
  ensure_twiddles(last_log + 1);
  arena_.reserve(((size_t)8 << last_log) * 4 + (1u << 20));
  begin_op();
  reset_event_log();
  Channel channel(cfg.protocol_variant);
  Hash32 d0;
  memcpy(d0.w, start_digest, 32);
  channel.set_digest(d0);
  DevChannel hc{};
  memcpy(hc.digest, d0.w, 32);
  hc.n_sent = 0;
  hc.variant = (cfg.protocol_variant & LMN_PV_DRAW_CTR_U32) ? 1u : 0u;
  FriClose fc;
  lmn_positions* kept = keep ? new_positions(log_query_domain, 0) : nullptr;
  try {
    DevChannel* d_ch = (DevChannel*)stage_upload(&hc, sizeof hc);
    enqueue_fri_close(fc, last_layer->d, d_ch, log_query_domain);
    if (kept) {   // behind k_fri_queries, in front of the wait: the block's count and positions into the handle
      const FriCloseHeader* h = reinterpret_cast<const FriCloseHeader*>(fc.h_block);
      lmn_h2d(kept->d, &h->n_positions, 4, stream_);
      lmn_h2d(kept->d + 1, fc.h_block + sizeof(FriCloseHeader) / 4, (size_t)fc.n_queries * 4, stream_);
    }
    lmn_sync(stream_);
    finish_fri_close(fc, channel, [&] {
      const size_t n = (size_t)1 << last_log;
      const uint32_t* raw = (const uint32_t*)stage_download(last_layer->d, 16 * n);
      lmn_sync(stream_);
      std::vector<QM31> v(n);
      for (size_t i = 0; i < n; ++i) v[i] = QM31{raw[i], raw[n + i], raw[2 * n + i], raw[3 * n + i]};
      return v;
    }, false);
    if (kept) {
      kept->n = (uint32_t)fc.positions.size();
      if (!fc.found) {   // nothing behind the grind ran: the host's positions
        uint32_t* h = (uint32_t*)pin_alloc((1 + fc.positions.size()) * 4);
        h[0] = kept->n;
        if (kept->n) memcpy(h + 1, fc.positions.data(), fc.positions.size() * 4);
        lmn_h2d(kept->d, h, (1 + fc.positions.size()) * 4, stream_);
        lmn_sync(stream_);
      }
    }
  } catch (...) {
    lmn_sync(stream_);   // launches in flight read tables in the staging memory the next op reuses
    if (kept) {
      lmn_dev_free(kept->d);
      delete kept;
    }
    throw;
  }
  if (keep) *keep = kept;
  lmn_fri_close_result& o = out.r;
  o.n_coeffs = (uint32_t)fc.coeffs.size();
  o.first_bad = fc.first_bad;
  o.n_positions = (uint32_t)fc.positions.size();
  o.grind_rounds = (uint32_t)fc.grind_waits;
  o.nonce = fc.nonce;
  o.coeffs = malloc_words(4 * fc.coeffs.size());
  memcpy(o.coeffs, fc.coeffs.data(), 16 * fc.coeffs.size());
  o.positions = malloc_words(fc.positions.size());
  memcpy(o.positions, fc.positions.data(), 4 * fc.positions.size());
  memcpy(o.digest_after_coeffs, fc.digest_after_coeffs.w, 32);
  memcpy(o.digest_after_nonce, fc.digest_after_nonce.w, 32);
  memcpy(o.digest_end, fc.digest_after_nonce.w, 32);   // (draws leave the digest alone)
  o.n_sent_end = fc.n_sent_end;
}

void Context::col_accumulate(lmn_col* dst, const lmn_col* src) {
  set_device();
  if (dst->ncols != src->ncols || dst->log_size != src->log_size)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "accumulate: shapes differ");
  launch_secure_add(dst->d, src->d, dst->words(), stream_);
}

// at most QUOT_MAX_BATCH distinct sample points and QUOT_MAX_ENTRIES samples (include/luminair_hip.h): make_quotient_args
// sizes its batch and entry tables by them
void check_quotient_limits(const uint32_t* sample_point, uint32_t nsamples) {
  if (nsamples > (uint32_t)QUOT_MAX_ENTRIES)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "accumulate_quotients: more than 512 samples");
  uint32_t seen[QUOT_MAX_BATCH];
  int n = 0;
  for (uint32_t i = 0; i < nsamples; ++i) {
    if (std::find(seen, seen + n, sample_point[i]) != seen + n) continue;
    if (n == QUOT_MAX_BATCH) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "accumulate_quotients: more than 4 distinct sample points");
    seen[n++] = sample_point[i];
  }
}

QuotientSamples parse_quotient_samples(uint32_t ncols, const uint32_t* sample_col, const uint32_t* sample_point,
                                       const uint32_t* sample_values, uint32_t nsamples, const uint32_t* points_xy, uint32_t npoints) {
  QuotientSamples s{std::vector<QPt>(npoints), std::vector<std::vector<std::pair<int, QM31>>>(ncols)};
  for (uint32_t p = 0; p < npoints; ++p) s.points[p] = qpt_words(points_xy + 8 * p);
  for (uint32_t i = 0; i < nsamples; ++i) {
    if (sample_col[i] >= ncols || sample_point[i] >= npoints) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "bad sample index");
    s.of_col[sample_col[i]].push_back({(int)sample_point[i], q_words(sample_values + 4 * i)});
  }
  return s;
}

lmn_col* Context::col_accumulate_quotients(const lmn_col* const* cols, uint32_t n, const uint32_t* sample_col,
                                           const uint32_t* sample_point, const uint32_t* sample_values, uint32_t nsamples,
                                           const uint32_t* points_xy, uint32_t npoints, const uint32_t alpha[4]) {
  set_device();
  if (n == 0 || !cols[0]) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "accumulate_quotients: no columns / null column handle");
  const uint32_t log_size = cols[0]->log_size;
  if (log_size < 2) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "accumulate_quotients: domain too small");
  check_quotient_limits(sample_point, nsamples);
  std::vector<const uint32_t*> d_cols;
  for (uint32_t k = 0; k < n; ++k) {
    if (!cols[k] || cols[k]->log_size != log_size) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "accumulate_quotients: columns of one size only");
    for (uint32_t j = 0; j < cols[k]->ncols; ++j) d_cols.push_back(cols[k]->d + ((uint64_t)j << log_size));
  }
  const uint32_t ncols = (uint32_t)d_cols.size();
  check_canonical(points_xy, 8ull * npoints, "accumulate_quotients: point");
  check_canonical(sample_values, 4ull * nsamples, "accumulate_quotients: sample value");
  check_canonical(alpha, 4, "accumulate_quotients: alpha");
  const QuotientSamples smp = parse_quotient_samples(ncols, sample_col, sample_point, sample_values, nsamples, points_xy, npoints);
  ensure_twiddles((int)log_size);
  arena_.reserve(8u << 20);
  begin_op();
  lmn_col* out = new_col(4, log_size);
  try {
    QuotientArgs a = make_quotient_args((int)log_size, d_cols, smp.of_col, smp.points, q_words(alpha), false);
    a.out = out->d;
    launch_quotients(a, stream_);
    lmn_sync(stream_);  // the (pointer, coefficient) table lives in the arena, which the next op resets
  } catch (...) {
    col_free(out);
    throw;
  }
  return out;
}

static void check_secure(const lmn_col* c, const char* what) {
  if (c->ncols != 4) throw LmnError(LMN_ERR_INVALID_ARGUMENT, std::string(what) + ": a secure column has 4 coordinate columns");
}
lmn_col* Context::col_fold_line(const lmn_col* src, const uint32_t alpha[4]) {
  check_canonical(alpha, 4, "fold_line: alpha");
  check_secure(src, "fold_line");
  if (src->log_size < 1) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "fold_line: nothing to fold");
  ensure_twiddles((int)src->log_size + 1);
  arena_.reserve(8u << 20);
  begin_op();
  std::vector<QM31> av{q_words(alpha)};
  QM31* d_alpha = upload_vec(av);
  ColGuard out(new_col(4, src->log_size - 1));
  launch_fold_line(out.c->d, src->d, 1u << src->log_size, itwX_[src->log_size + 1], d_alpha, stream_);
  lmn_sync(stream_);  // alpha lives in the arena
  return out.release();
}
void Context::col_fold_circle_into_line(lmn_col* dst, const lmn_col* src, const uint32_t alpha[4]) {
  check_canonical(alpha, 4, "fold_circle_into_line: alpha");
  check_secure(src, "fold_circle_into_line");
  check_secure(dst, "fold_circle_into_line");
  if (src->log_size < 1 || dst->log_size + 1 != src->log_size)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "fold_circle_into_line: dst must be half the size of src");
  ensure_twiddles((int)src->log_size);
  arena_.reserve(8u << 20);
  begin_op();
  std::vector<QM31> av{q_words(alpha)};
  QM31* d_alpha = upload_vec(av);
  launch_fold_circle_into_line(dst->d, src->d, 1u << src->log_size, itwY_[src->log_size], d_alpha, 1, stream_);
  lmn_sync(stream_);
}
lmn_col* Context::col_decompose(const lmn_col* f, uint32_t lambda_out[4]) {
  check_secure(f, "decompose");
  if (f->log_size < 1) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "decompose: a circle domain has at least two points");
  arena_.reserve(8u << 20);
  begin_op();
  QM31* d_lambda = (QM31*)arena_.alloc_bytes(sizeof(QM31));
  QM31* scratch = (QM31*)arena_.alloc_bytes((size_t)decompose_num_blocks((int)f->log_size) * sizeof(QM31));
  ColGuard gg(new_col(4, f->log_size));
  lmn_col* g = gg.c;
  launch_decompose(f->d, (int)f->log_size, g->d, d_lambda, scratch, stream_);
  const QM31* l = (const QM31*)stage_download(d_lambda, sizeof(QM31));
  lmn_sync(stream_);
  store_words(lambda_out, *l);
  return gg.release();
}

// FieldOps::batch_inverse on handles.  Everything is refused before anything is launched; dst over exactly src's range is
// the in-place form (a lane of k_batch_inverse_* reads all it owns before it writes), any other overlap is refused.
void Context::col_batch_inverse(const lmn_col* src, lmn_col* dst, bool secure, uint64_t* n_zero_out) {
  const std::string F = secure ? "batch_inverse_secure: " : "batch_inverse: ";
  auto refuse = [&](const std::string& what) { throw LmnError(LMN_ERR_INVALID_ARGUMENT, F + what); };
  if (!src) refuse("src is null");
  if (!dst) refuse("dst is null");
  if (secure && src->ncols != 4) refuse("src has " + u32s(src->ncols) + " columns, a secure column has 4 coordinate columns");
  if (secure && dst->ncols != 4) refuse("dst has " + u32s(dst->ncols) + " columns, a secure column has 4 coordinate columns");
  if (dst->ncols != src->ncols || dst->log_size != src->log_size)
    refuse("dst is " + u32s(dst->ncols) + " x 2^" + u32s(dst->log_size) + ", src is " + u32s(src->ncols) + " x 2^" +
           u32s(src->log_size) + ": shapes differ");
  if (src->log_size > COL_MAX_LOG) refuse("src has log size " + u32s(src->log_size) + ", the largest is " + u32s(COL_MAX_LOG));
  const uint32_t *s0 = src->d, *s1 = s0 + src->words(), *d0 = dst->d, *d1 = d0 + dst->words();
  if (d0 != s0 && d0 < s1 && s0 < d1) refuse("dst overlaps src without being the same range");
  unsigned long long* d_zero = nullptr;
  if (n_zero_out) {
    arena_.reserve(8u << 20);
    begin_op();
    d_zero = (unsigned long long*)arena_.alloc_bytes(sizeof(unsigned long long));
    lmn_memset(d_zero, 0, sizeof(unsigned long long), stream_);
  } else {
    set_device();
  }
  if (secure)
    launch_batch_inverse_qm31(src->d, dst->d, (int)src->log_size, d_zero, stream_);
  else
    launch_batch_inverse_m31(src->d, dst->d, 1ull << src->log_size, (int)src->ncols, (int)src->log_size, d_zero, stream_);
  if (!n_zero_out) return;
  const unsigned long long* z = (const unsigned long long*)stage_download(d_zero, sizeof(unsigned long long));
  lmn_sync(stream_);
  *n_zero_out = *z;
}

// ---- the per-component stages on handles (the same launches Context::prove makes)
static const ComponentSpec* spec_or_throw(uint32_t kind, const char* what) {
  const ComponentSpec* sp = component_spec((int)kind);
  if (!sp) throw LmnError(LMN_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown component kind");
  return sp;
}
lmn_col* Context::col_logup(uint32_t kind, const lmn_col* main, const lmn_col* pre, const uint32_t* elems,
                            uint32_t claimed_out[4]) {
  set_device();
  const ComponentSpec* sp = spec_or_throw(kind, "logup");
  if ((int)main->ncols != sp->n_cols) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "logup: wrong number of trace columns for this kind");
  if (main->log_size < 4 || main->log_size > 26) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "logup: trace log size must be 4..26");
  if (sp->n_pre && (!pre || (int)pre->ncols != sp->n_pre || pre->log_size != main->log_size))
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "logup: this kind needs its preprocessed columns (same size as the trace)");
  check_canonical(elems, 8ull * N_ELEMS, "logup: relation element");
  const uint64_t n = 1ull << main->log_size;
  const int nic = 4 * sp->n_rel;
  const int nb = logup_num_blocks((uint32_t)n);
  arena_.reserve(n * sizeof(QM31) + (size_t)nb * 16 + (size_t)logup_scan_num_blocks((int)main->log_size) * sizeof(QM31) + (4u << 20));
  begin_op();
  ColGuard out(new_col((uint32_t)nic, main->log_size));
  LogupArgs a{};
  a.k = sp->n_rel;
  for (int j = 0; j < sp->n_rel; ++j) {
    auto column = [&](int idx) -> const uint32_t* { return (sp->rel_pre[j] ? pre->d : main->d) + (uint64_t)idx * n; };
    a.val[j] = column(sp->rel_val[j]);
    a.id[j] = sp->rel_id[j] >= 0 ? column(sp->rel_id[j]) : nullptr;
    a.mult[j] = main->d + (uint64_t)sp->rel_mult[j] * n;
    a.neg[j] = sp->rel_neg[j];
    a.z[j] = q_words(elems + 8 * sp->rel_elems[j]);
    a.alpha[j] = q_words(elems + 8 * sp->rel_elems[j] + 4);
  }
  a.inter = out.c->d;
  a.last_tmp = (QM31*)arena_.alloc_bytes(n * sizeof(QM31));
  a.partials = arena_.alloc_words((size_t)nb * 4);
  a.n = (uint32_t)n;
  launch_logup_fracs(a, stream_);
  QM31* d_cs = (QM31*)arena_.alloc_bytes(2 * sizeof(QM31));
  QM31* bsums = (QM31*)arena_.alloc_bytes((size_t)logup_scan_num_blocks((int)main->log_size) * sizeof(QM31));
  launch_logup_scan(a.last_tmp, d_cs, (int)main->log_size, out.c->d + (uint64_t)(nic - 4) * n, bsums, stream_, true,
                    m_inv((uint32_t)(n % P31)));
  const QM31* cs = (const QM31*)stage_download(d_cs, 2 * sizeof(QM31));
  lmn_sync(stream_);
  store_words(claimed_out, cs[0]);
  return out.release();
}

void Context::col_composition(uint32_t kind, const lmn_col* main_lde, const lmn_col* inter_lde, const lmn_col* pre_lde,
                              const uint32_t* elems, const uint32_t claimed[4], const uint32_t* coeffs, uint32_t n_coeffs,
                              lmn_col* acc) {
  set_device();
  const ComponentSpec* sp = spec_or_throw(kind, "composition");
  const int e = (int)main_lde->log_size, ls = e - 1;
  if (ls < 4 || ls > 26) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "composition: evaluation domain log size must be 5..27");
  if ((int)main_lde->ncols != sp->n_cols || (int)inter_lde->ncols != 4 * sp->n_rel || (int)inter_lde->log_size != e)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "composition: trace / interaction columns do not match this kind");
  if (sp->n_pre && (!pre_lde || (int)pre_lde->ncols != sp->n_pre || (int)pre_lde->log_size != e))
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "composition: this kind needs its preprocessed columns on the evaluation domain");
  if ((int)n_coeffs != sp->n_local + sp->n_rel) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "composition: one coefficient per constraint");
  if (acc->ncols != 4 || (int)acc->log_size != e) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "composition: accumulator must be 4 x 2^(k+1)");
  check_canonical(elems, 8ull * N_ELEMS, "composition: relation element");
  check_canonical(claimed, 4, "composition: claimed sum");
  check_canonical(coeffs, 4ull * n_coeffs, "composition: coefficient");
  arena_.reserve(4u << 20);
  begin_op();
  const uint64_t E = 1ull << e;
  CompositionArgs a{};
  a.kind = sp->kind;
  a.log_size = ls;
  a.eval_log = e;
  a.main = main_lde->d;
  a.inter = inter_lde->d;
  a.row0 = 0;
  a.n_rows = (uint32_t)E;
  a.stride = E;
  a.prev_last = a.inter + (uint64_t)(4 * (sp->n_rel - 1)) * E;
  a.out = acc->d;
  a.accumulate = 1;
  a.z = q_words(elems + 8 * ELEMS_NODE);
  a.alpha = q_words(elems + 8 * ELEMS_NODE + 4);
  for (int j = 0; j < sp->n_rel; ++j)
    if (sp->rel_elems[j] != ELEMS_NODE) {
      a.z2 = q_words(elems + 8 * sp->rel_elems[j]);
      a.alpha2 = q_words(elems + 8 * sp->rel_elems[j] + 4);
    }
  a.pre = sp->n_pre >= 1 ? pre_lde->d : nullptr;
  a.pre2 = sp->n_pre >= 2 ? pre_lde->d + E : nullptr;
  const QM31 cl = q_words(claimed);
  std::vector<QM31> cs{cl, q_mul_m(cl, m_inv((uint32_t)((1ull << ls) % P31)))};
  a.claimed_shift = upload_vec(cs);
  for (uint32_t k = 0; k < n_coeffs; ++k) a.coeff[k] = q_words(coeffs + 4 * k);
  for (int b = 0; b < 2; ++b) {
    Pt p = domain_point(e, (uint32_t)b << ls);
    uint32_t x = p.x;
    for (int k = 0; k < ls - 1; ++k) x = m_sub(m_dbl(m_sqr(x)), 1u);
    a.zinv[b] = m_inv(x);
  }
  launch_composition(a, stream_);
  lmn_sync(stream_);  // [claimed, shift] lives in the arena, which the next op resets
}

}  // namespace lmn

// ------------------------------------------------------------------------------------ extern "C"
namespace {
template <typename F>
int guard2(lmn_ctx* ctx, F&& f) {
  return lmn::capi_guard(ctx, std::forward<F>(f));
}
}  // namespace

extern "C" {
int lmn_col_alloc(lmn_ctx* ctx, uint32_t ncols, uint32_t log_size, lmn_col** out) {
  if (!ctx || !out) return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return guard2(ctx, [&] { *out = ctx->impl->col_alloc(ncols, log_size, true); });
}
int lmn_col_from_cpu(lmn_ctx* ctx, const uint32_t* host, uint32_t ncols, uint32_t log_size, lmn_col** out) {
  if (!ctx || !host || !out) return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return guard2(ctx, [&] { *out = ctx->impl->col_from_cpu(host, ncols, log_size); });
}
int lmn_col_to_cpu(lmn_ctx* ctx, const lmn_col* col, uint32_t* host) {
  if (!ctx || !col || !host) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->col_to_cpu(col, host); });
}
void lmn_col_free(lmn_ctx* ctx, lmn_col* col) {
  if (ctx && col) guard2(ctx, [&] { ctx->impl->col_free(col); });
}
uint32_t lmn_col_ncols(const lmn_col* col) { return col ? col->ncols : 0; }
uint32_t lmn_col_log_size(const lmn_col* col) { return col ? col->log_size : 0; }
void* lmn_col_device_ptr(const lmn_col* col) { return col ? col->d : nullptr; }
int lmn_col_bit_reverse(lmn_ctx* ctx, lmn_col* col) {
  if (!ctx || !col) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->col_bit_reverse(col); });
}
int lmn_col_precompute_twiddles(lmn_ctx* ctx, uint32_t log_size) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->col_precompute_twiddles(log_size); });
}
int lmn_col_interpolate(lmn_ctx* ctx, lmn_col* c) {
  if (!ctx || !c) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->col_interpolate(c); });
}
int lmn_col_evaluate(lmn_ctx* ctx, const lmn_col* coeffs, uint32_t log_domain, lmn_col** out) {
  if (!ctx || !coeffs || !out) return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return guard2(ctx, [&] { *out = ctx->impl->col_evaluate(coeffs, log_domain); });
}
int lmn_col_evaluate_block(lmn_ctx* ctx, const lmn_col* coeffs, uint32_t log_domain, uint32_t log_blocks, uint32_t block,
                           lmn_col** out) {
  if (!ctx || !coeffs || !out) return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return guard2(ctx, [&] { *out = ctx->impl->col_evaluate_block(coeffs, log_domain, log_blocks, block); });
}
int lmn_col_extend(lmn_ctx* ctx, const lmn_col* coeffs, uint32_t log_size, lmn_col** out) {
  if (!ctx || !coeffs || !out) return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return guard2(ctx, [&] { *out = ctx->impl->col_extend(coeffs, log_size); });
}
int lmn_col_eval_at_point(lmn_ctx* ctx, const lmn_col* coeffs, uint32_t column, const uint32_t point_xy[8],
                          uint32_t value_out[4]) {
  if (!ctx || !coeffs || !point_xy || !value_out) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->col_eval_at_point(coeffs, column, point_xy, value_out); });
}
int lmn_col_commit(lmn_ctx* ctx, const lmn_col* const* cols, uint32_t n, lmn_tree** tree_out) {
  if (!ctx || !cols || !tree_out) return LMN_ERR_INVALID_ARGUMENT;
  *tree_out = nullptr;
  return guard2(ctx, [&] { *tree_out = ctx->impl->col_commit(cols, n); });
}
int lmn_tree_root(lmn_ctx* ctx, const lmn_tree* tree, uint8_t root_out[32]) {
  if (!ctx || !tree || !root_out) return LMN_ERR_INVALID_ARGUMENT;
  memcpy(root_out, tree->root.w, 32);
  return LMN_OK;
}
uint32_t lmn_tree_log_size(const lmn_tree* tree) { return tree ? (uint32_t)tree->max_log : 0; }
int lmn_tree_layer_to_cpu(lmn_ctx* ctx, const lmn_tree* tree, uint32_t layer_log, uint8_t* hashes_out) {
  if (!ctx || !tree || !hashes_out) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->tree_layer_to_cpu(tree, layer_log, hashes_out); });
}
int lmn_tree_decommit(lmn_ctx* ctx, const lmn_tree* tree, const lmn_col* const* cols, uint32_t n_cols,
                      const uint32_t* query_logs, const uint32_t* query_counts, uint32_t n_groups, const uint32_t* queries,
                      uint32_t** queried_values, size_t* n_values, uint8_t** hash_witness, size_t* n_hashes,
                      uint32_t** column_witness, size_t* n_column_words) {
  if (queried_values) *queried_values = nullptr;
  if (hash_witness) *hash_witness = nullptr;
  if (column_witness) *column_witness = nullptr;
  if (n_values) *n_values = 0;
  if (n_hashes) *n_hashes = 0;
  if (n_column_words) *n_column_words = 0;
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] {
    if (!tree) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "tree_decommit: tree is null");
    if (!queried_values || !n_values || !hash_witness || !n_hashes || !column_witness || !n_column_words)
      throw LmnError(LMN_ERR_INVALID_ARGUMENT, "tree_decommit: an output pointer is null");
    lmn::TreeOpening o;
    ctx->impl->tree_decommit(tree, cols, n_cols, query_logs, query_counts, n_groups, queries, o);
    *queried_values = o.queried_values;
    *n_values = o.n_values;
    *hash_witness = o.hash_witness;
    *n_hashes = o.n_hashes;
    *column_witness = o.column_witness;
    *n_column_words = o.n_column_words;
  });
}
int lmn_col_gather(lmn_ctx* ctx, const lmn_col* col, const uint32_t* positions, uint32_t n, uint32_t* host_out) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] {
    if (!col) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "col_gather: col is null");
    if (n == 0) return;
    if (!positions) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "col_gather: positions is null with n = " + std::to_string(n));
    if (!host_out) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "col_gather: host_out is null with n = " + std::to_string(n));
    ctx->impl->col_gather(col, positions, n, host_out);
  });
}
int lmn_col_fri_commit(lmn_ctx* ctx, const lmn_col* const* cols, uint32_t n, const uint8_t start_digest[32],
                       lmn_fri_commit_result* result) {
  if (result) *result = lmn_fri_commit_result{};
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] {
    if (!result) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "fri_commit: result is null");
    lmn::FriCommitOut o;
    ctx->impl->col_fri_commit(cols, n, start_digest, o);
    *result = o.release();
  });
}
int lmn_col_fri_close(lmn_ctx* ctx, const lmn_col* last_layer, const uint8_t start_digest[32], uint32_t log_query_domain,
                      lmn_fri_close_result* result) {
  if (result) *result = lmn_fri_close_result{};
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] {
    if (!result) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "fri_close: result is null");
    lmn::FriCloseOut o;
    ctx->impl->col_fri_close(last_layer, start_digest, log_query_domain, o);
    *result = o.release();
  });
}
int lmn_col_fri_close_keep(lmn_ctx* ctx, const lmn_col* last_layer, const uint8_t start_digest[32], uint32_t log_query_domain,
                           lmn_fri_close_result* result, lmn_positions** positions_out) {
  if (result) *result = lmn_fri_close_result{};
  if (positions_out) *positions_out = nullptr;
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] {
    if (!result) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "fri_close: result is null");
    if (!positions_out) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "fri_close: positions_out is null");
    lmn::FriCloseOut o;
    lmn_positions* kept = nullptr;
    ctx->impl->col_fri_close(last_layer, start_digest, log_query_domain, o, &kept);
    *result = o.release();
    *positions_out = kept;
  });
}
int lmn_positions_from_cpu(lmn_ctx* ctx, const uint32_t* positions, uint32_t n, uint32_t log_domain, lmn_positions** out) {
  if (out) *out = nullptr;
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] {
    if (!out) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "positions_from_cpu: out is null");
    *out = ctx->impl->positions_from_cpu(positions, n, log_domain);
  });
}
int lmn_positions_to_cpu(lmn_ctx* ctx, const lmn_positions* positions, uint32_t* host, uint32_t* n_out) {
  if (n_out) *n_out = 0;
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] {
    if (!positions) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "positions_to_cpu: positions is null");
    if (!host) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "positions_to_cpu: host is null");
    if (!n_out) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "positions_to_cpu: n_out is null");
    ctx->impl->positions_to_cpu(positions, host, n_out);
  });
}
uint32_t lmn_positions_log_domain(const lmn_positions* positions) { return positions ? positions->log_domain : 0; }
void lmn_positions_free(lmn_ctx* ctx, lmn_positions* positions) {
  if (ctx && positions) guard2(ctx, [&] { ctx->impl->positions_free(positions); });
}
int lmn_open_queries(lmn_ctx* ctx, const lmn_positions* positions, const lmn_open_item* items, uint32_t n_items,
                     lmn_opening* out) {
  if (out)
    for (uint32_t k = 0; k < n_items; ++k) out[k] = lmn_opening{};
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->open_queries(positions, items, n_items, out); });
}
void lmn_tree_free(lmn_ctx* ctx, lmn_tree* tree) {
  if (ctx && tree) guard2(ctx, [&] { ctx->impl->tree_free(tree); });
}
int lmn_col_accumulate(lmn_ctx* ctx, lmn_col* dst, const lmn_col* src) {
  if (!ctx || !dst || !src) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->col_accumulate(dst, src); });
}
int lmn_col_accumulate_quotients(lmn_ctx* ctx, const lmn_col* const* cols, uint32_t n, const uint32_t* sample_col,
                                 const uint32_t* sample_point, const uint32_t* sample_values, uint32_t nsamples,
                                 const uint32_t* points_xy, uint32_t npoints, const uint32_t alpha[4], lmn_col** out) {
  if (!ctx || !cols || !sample_col || !sample_point || !sample_values || !points_xy || !alpha || !out)
    return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return guard2(ctx, [&] {
    *out = ctx->impl->col_accumulate_quotients(cols, n, sample_col, sample_point, sample_values, nsamples, points_xy, npoints, alpha);
  });
}
int lmn_col_fold_line(lmn_ctx* ctx, const lmn_col* src, const uint32_t alpha[4], lmn_col** out) {
  if (!ctx || !src || !alpha || !out) return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return guard2(ctx, [&] { *out = ctx->impl->col_fold_line(src, alpha); });
}
int lmn_col_fold_circle_into_line(lmn_ctx* ctx, lmn_col* dst, const lmn_col* src, const uint32_t alpha[4]) {
  if (!ctx || !dst || !src || !alpha) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->col_fold_circle_into_line(dst, src, alpha); });
}
int lmn_col_view(lmn_ctx* ctx, const lmn_col* col, uint32_t first, uint32_t n, lmn_col** out) {
  if (!ctx || !col || !out) return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  return guard2(ctx, [&] { *out = ctx->impl->col_view(col, first, n); });
}
int lmn_col_logup(lmn_ctx* ctx, uint32_t kind, const lmn_col* main, const lmn_col* pre, const uint32_t* elems,
                  lmn_col** interaction_out, uint32_t claimed_sum_out[4]) {
  if (!ctx || !main || !elems || !interaction_out || !claimed_sum_out) return LMN_ERR_INVALID_ARGUMENT;
  *interaction_out = nullptr;
  return guard2(ctx, [&] { *interaction_out = ctx->impl->col_logup(kind, main, pre, elems, claimed_sum_out); });
}
int lmn_col_composition(lmn_ctx* ctx, uint32_t kind, const lmn_col* main_lde, const lmn_col* inter_lde,
                        const lmn_col* pre_lde, const uint32_t* elems, const uint32_t claimed_sum[4],
                        const uint32_t* coeffs, uint32_t n_coeffs, lmn_col* acc) {
  if (!ctx || !main_lde || !inter_lde || !elems || !claimed_sum || !coeffs || !acc) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] {
    ctx->impl->col_composition(kind, main_lde, inter_lde, pre_lde, elems, claimed_sum, coeffs, n_coeffs, acc);
  });
}
uint32_t lmn_kind_constraints(uint32_t kind) {
  const lmn::ComponentSpec* s = lmn::component_spec((int)kind);
  return s ? (uint32_t)(s->n_local + s->n_rel) : 0u;
}
uint32_t lmn_kind_constraint_layout(uint32_t kind, uint32_t protocol_flags, int32_t proto_index_out[16], int32_t sign_out[16]) {
  const lmn::ComponentSpec* s = lmn::component_spec((int)kind);
  if (!s || !proto_index_out || !sign_out || (protocol_flags & ~LMN_PV_ALL)) return 0u;
  const lmn::ConstraintLayout L = lmn::constraint_layout(*s, protocol_flags);
  for (int k = 0; k < 16; ++k) {
    proto_index_out[k] = k < L.n_kernel ? L.proto_index[k] : -1;
    sign_out[k] = k < L.n_kernel && L.neg[k] ? -1 : 1;
  }
  return (uint32_t)L.n_protocol;
}
uint32_t lmn_kind_relations(uint32_t kind) {
  const lmn::ComponentSpec* s = lmn::component_spec((int)kind);
  return s ? (uint32_t)s->n_rel : 0u;
}
int lmn_col_decompose(lmn_ctx* ctx, const lmn_col* f, lmn_col** g_out, uint32_t lambda_out[4]) {
  if (!ctx || !f || !g_out || !lambda_out) return LMN_ERR_INVALID_ARGUMENT;
  *g_out = nullptr;
  return guard2(ctx, [&] { *g_out = ctx->impl->col_decompose(f, lambda_out); });
}
int lmn_col_batch_inverse(lmn_ctx* ctx, const lmn_col* src, lmn_col* dst, uint64_t* n_zero_out) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->col_batch_inverse(src, dst, false, n_zero_out); });
}
int lmn_col_batch_inverse_secure(lmn_ctx* ctx, const lmn_col* src, lmn_col* dst, uint64_t* n_zero_out) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard2(ctx, [&] { ctx->impl->col_batch_inverse(src, dst, true, n_zero_out); });
}
}  // extern "C"
