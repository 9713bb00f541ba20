// extern "C" boundary (include/luminair_hip.h): the entry points a Rust `extern "C"` block would
// bind in place of /root/reference/crates/prover/src/prover.rs:28-31.
#include "../../include/luminair_hip.h"

#include "capi_internal.h"

#include <algorithm>
#include <cmath>

using lmn::Context;
using lmn::TraceTarget;

namespace {
// for the entry points that need no context
template <class F>
static int host_guard(F&& f) {
  try {
    f();
    return LMN_OK;
  } catch (const LmnError& e) {
    return e.code;
  } catch (const std::bad_alloc&) {
    return LMN_ERR_OUT_OF_MEMORY;
  } catch (...) {
    return LMN_ERR_INTERNAL;
  }
}

template <typename F>
int guard(lmn_ctx* ctx, F&& f) {
  return lmn::capi_guard(ctx, std::forward<F>(f));
}
thread_local std::string g_create_error;
}  // namespace

namespace lmn {
const char prepared_tag = 0;
std::shared_ptr<const Prepared> prepared_ref(const lmn_prepared* p) {
  if (!p || !p->impl) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "null prepared settings");
  if (p->made_by != &prepared_tag)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "prepared settings were made by another library (the main and the batch library each prepare their own)");
  return p->impl;
}
}  // namespace lmn

extern "C" {

const char* lmn_strerror(int code) {
  switch (code) {
    case LMN_OK: return "ok";
    case LMN_ERR_EMPTY_TRACE: return "TraceError(EmptyTrace)";
    case LMN_ERR_MAIN_TRACE: return "MainTraceEvalGenError";
    case LMN_ERR_INTERACTION_TRACE: return "InteractionTraceEvalGenError";
    case LMN_ERR_CONSTRAINTS: return "ProverError(ConstraintsNotSatisfied)";
    case LMN_ERR_SERIALIZATION: return "SerializationError";
    case LMN_ERR_INVALID_ARGUMENT: return "invalid argument";
    case LMN_ERR_OUT_OF_MEMORY: return "out of memory";
    case LMN_ERR_NO_DEVICE: return "no HIP device (no CPU fallback exists)";
    case LMN_ERR_VERIFICATION: return "StwoVerifierError";
    case LMN_ERR_INVALID_LOGUP: return "InvalidLogUp";
    default: return "internal error";
  }
}

uint32_t lmn_abi_version(void) { return LMN_API_VERSION; }

const char* lmn_last_error(const lmn_ctx* ctx) { return ctx ? ctx->last_error.c_str() : g_create_error.c_str(); }

void lmn_default_config(lmn_config* cfg) {
  if (!cfg) return;
  cfg->pow_bits = 5;
  cfg->log_blowup = 1;
  cfg->log_last_layer = 0;
  cfg->n_queries = 3;
  cfg->fp_scale = 12;
  cfg->protocol_variant = LMN_VARIANT_KAT;
}

uint32_t lmn_kind_columns(uint32_t kind) {
  const lmn::ComponentSpec* s = lmn::component_spec((int)kind);
  return s ? (uint32_t)s->n_cols : 0u;
}

int lmn_kind_padding_row(uint32_t kind, uint32_t* out) {
  const lmn::ComponentSpec* s = lmn::component_spec((int)kind);
  if (!s || !out) return LMN_ERR_INVALID_ARGUMENT;
  const lmn::PadRow pad = lmn::pad_row_of(*s);
  for (int c = 0; c < s->n_cols; ++c) out[c] = pad.v[c];
  return LMN_OK;
}

int lmn_ctx_create(int device, const lmn_config* cfg, lmn_ctx** out) {
  if (!out) return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  lmn_config c;
  lmn_default_config(&c);
  if (cfg) c = *cfg;
  lmn_ctx* ctx = new lmn_ctx{nullptr, {}};
  int rc = guard(ctx, [&] { ctx->impl = new Context(device, c); });
  if (rc != LMN_OK) {
    g_create_error = ctx->last_error;
    delete ctx;
    return rc;
  }
  *out = ctx;
  return LMN_OK;
}

// error text written by the CALLING thread: under the context's own lock, like the worker's guard()
static int set_error(lmn_ctx* ctx, int code, const char* msg) {
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  ctx->last_error = msg;
  return code;
}

static void async_stop(lmn_ctx* ctx) {
  lmn_async* a = ctx->async;
  if (!a) return;
  {
    std::unique_lock<std::mutex> lk(a->m);
    a->cv.wait(lk, [&] { return a->state != lmn_async::SUBMITTED; });  // let a running proof finish
    a->state = lmn_async::QUIT;
  }
  a->cv.notify_all();
  if (a->worker.joinable()) a->worker.join();
  delete a;
  ctx->async = nullptr;
}

void lmn_ctx_destroy(lmn_ctx* ctx) {
  if (!ctx) return;
  async_stop(ctx);
  delete ctx->impl;
  delete ctx;
}

// ---- asynchronous form of lmn_prove: the reference's callers are single-threaded (SURVEY.md §8b "threading"); with
// submit / wait one thread keeps a proof in flight on each of several contexts
static int prove_submit(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_settings* settings,
                        std::shared_ptr<const lmn::Prepared> prepared) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  std::unique_lock<std::mutex> create_lock(ctx->async_mu);
  if (!ctx->async) {
    lmn_async* a = new lmn_async();
    ctx->async = a;
    a->worker = std::thread([ctx, a] {
      for (;;) {
        std::unique_lock<std::mutex> lk(a->m);
        a->cv.wait(lk, [&] { return a->state == lmn_async::SUBMITTED || a->state == lmn_async::QUIT; });
        if (a->state == lmn_async::QUIT) return;
        const lmn_table* t = a->tables;
        const size_t n = a->n_tables;
        const lmn_settings* st = a->settings;
        const std::shared_ptr<const lmn::Prepared> pp = a->prepared;
        lk.unlock();
        std::vector<uint8_t> bytes;
        const int rc = guard(ctx, [&] { bytes = ctx->impl->prove(t, n, st, pp.get()); });
        lk.lock();
        a->rc = rc;
        a->proof.swap(bytes);
        a->state = lmn_async::DONE;
        lk.unlock();
        a->cv.notify_all();
      }
    });
  }
  lmn_async* a = ctx->async;
  create_lock.unlock();
  bool busy = false;
  {
    std::lock_guard<std::mutex> lk(a->m);
    if (a->state != lmn_async::IDLE) {
      busy = true;
    } else {
      a->tables = tables;
      a->n_tables = n_tables;
      a->settings = settings;
      a->prepared = std::move(prepared);
      a->state = lmn_async::SUBMITTED;
    }
  }
  if (busy) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT,
                             "lmn_prove_submit: a submitted proof has not been collected with lmn_prove_wait");
  a->cv.notify_all();
  return LMN_OK;
}

int lmn_prove_submit(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_settings* settings) {
  return prove_submit(ctx, tables, n_tables, settings, nullptr);
}

int lmn_prove_wait(lmn_ctx* ctx, uint8_t** proof_bincode, size_t* proof_len) {
  if (!ctx || !proof_bincode || !proof_len) return LMN_ERR_INVALID_ARGUMENT;
  *proof_bincode = nullptr;
  *proof_len = 0;
  lmn_async* a;
  {
    std::lock_guard<std::mutex> create_lock(ctx->async_mu);
    a = ctx->async;
  }
  if (!a) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_prove_wait: nothing was submitted");
  std::unique_lock<std::mutex> lk(a->m);
  if (a->state == lmn_async::IDLE) {
    lk.unlock();
    return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_prove_wait: nothing was submitted");
  }
  a->cv.wait(lk, [&] { return a->state == lmn_async::DONE; });
  const int rc = a->rc;
  a->prepared.reset();
  if (rc == LMN_OK) {
    uint8_t* p = (uint8_t*)malloc(a->proof.size() ? a->proof.size() : 1);
    if (!p) {
      a->proof.clear();
      a->state = lmn_async::IDLE;
      return LMN_ERR_OUT_OF_MEMORY;
    }
    memcpy(p, a->proof.data(), a->proof.size());
    *proof_bincode = p;
    *proof_len = a->proof.size();
  }
  a->proof.clear();
  a->state = lmn_async::IDLE;
  return rc;
}

int lmn_prove(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_settings* settings,
              uint8_t** proof_bincode, size_t* proof_len) {
  if (!ctx || !proof_bincode || !proof_len) return LMN_ERR_INVALID_ARGUMENT;
  *proof_bincode = nullptr;
  *proof_len = 0;
  return guard(ctx, [&] {
    std::vector<uint8_t> bytes = ctx->impl->prove(tables, n_tables, settings);
    uint8_t* p = (uint8_t*)malloc(bytes.size());
    if (!p) throw std::bad_alloc();
    memcpy(p, bytes.data(), bytes.size());
    *proof_bincode = p;
    *proof_len = bytes.size();
  });
}

void lmn_free(void* p) { free(p); }

// ---- settings prepared once (prover.h Prepared)
int lmn_settings_prepare(int device, const lmn_config* cfg, const lmn_settings* settings, uint32_t lookups, lmn_prepared** out) {
  if (!out) return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  lmn_config c;
  lmn_default_config(&c);
  if (cfg) c = *cfg;
  lmn_ctx err{nullptr, {}};   // collects the error text only
  const int rc = guard(&err, [&] {
    auto impl = std::make_shared<const lmn::Prepared>(device, c, settings, lookups);
    *out = new lmn_prepared{std::move(impl), &lmn::prepared_tag};
  });
  if (rc != LMN_OK) g_create_error = err.last_error;
  return rc;
}

int lmn_prepared_root(const lmn_prepared* p, uint8_t root_out[32]) {
  if (!p || !p->impl || !root_out) return LMN_ERR_INVALID_ARGUMENT;
  memcpy(root_out, p->impl->tree.merkle.root.w, 32);
  return LMN_OK;
}

uint32_t lmn_prepared_lookups(const lmn_prepared* p) { return p && p->impl ? p->impl->lookups : 0u; }

void lmn_prepared_destroy(lmn_prepared* p) { delete p; }

int lmn_prove_prepared(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_prepared* prepared,
                       uint8_t** proof_bincode, size_t* proof_len) {
  if (!ctx || !proof_bincode || !proof_len) return LMN_ERR_INVALID_ARGUMENT;
  *proof_bincode = nullptr;
  *proof_len = 0;
  return guard(ctx, [&] {
    const std::shared_ptr<const lmn::Prepared> pp = lmn::prepared_ref(prepared);   // this proof's own reference
    std::vector<uint8_t> bytes = ctx->impl->prove(tables, n_tables, nullptr, pp.get());
    uint8_t* p = (uint8_t*)malloc(bytes.size());
    if (!p) throw std::bad_alloc();
    memcpy(p, bytes.data(), bytes.size());
    *proof_bincode = p;
    *proof_len = bytes.size();
  });
}

#ifndef LMN_BATCH
// batch objects exist in the batch library alone (batch.cpp defines this entry there): no handle this library could be given is one
int lmn_batch_prove_prepared(lmn_batch*, uint32_t n, const lmn_table* const*, size_t, const lmn_prepared*, uint8_t** proofs,
                             size_t* lens, int* rcs) {
  for (uint32_t i = 0; i < n && n <= 256; ++i) {
    if (proofs) proofs[i] = nullptr;
    if (lens) lens[i] = 0;
    if (rcs) rcs[i] = LMN_ERR_INVALID_ARGUMENT;
  }
  g_create_error = "lmn_batch_prove_prepared: lock-step batches are proved by libluminair_hip_batch.so";
  return LMN_ERR_INVALID_ARGUMENT;
}
#endif

int lmn_prove_submit_prepared(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_prepared* prepared) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  std::shared_ptr<const lmn::Prepared> pp;
  const int rc = guard(ctx, [&] { pp = lmn::prepared_ref(prepared); });
  if (rc != LMN_OK) return rc;
  return prove_submit(ctx, tables, n_tables, nullptr, std::move(pp));
}

int lmn_set_profiling(lmn_ctx* ctx, int enabled) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  ctx->impl->profiling = enabled != 0;
  return LMN_OK;
}

int lmn_get_timings(const lmn_ctx* ctx, lmn_timings* out) {
  if (!ctx || !out) return LMN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::recursive_mutex> lock(const_cast<lmn_ctx*>(ctx)->mu);
  *out = ctx->impl->timings;
  return LMN_OK;
}

int lmn_verify_with_config(const uint8_t* proof_bincode, size_t proof_len, const lmn_settings* settings,
                           const lmn_config* expected) {
  if (!proof_bincode || !expected) return LMN_ERR_INVALID_ARGUMENT;
  lmn_ctx tmp{nullptr, {}};
  int rc = guard(&tmp, [&] { lmn::verify_proof(proof_bincode, proof_len, *expected, settings); });
  g_create_error = tmp.last_error;
  return rc;
}

int lmn_verify_diagnose(const uint8_t* proof_bincode, size_t proof_len, const lmn_settings* settings,
                        const lmn_config* expected, lmn_verify_report* report) {
  if (!proof_bincode || !expected || !report) return LMN_ERR_INVALID_ARGUMENT;
  memset(report, 0, sizeof *report);
  lmn_ctx tmp{nullptr, {}};
  int rc = guard(&tmp, [&] { lmn::verify_proof(proof_bincode, proof_len, *expected, settings, report); });
  if (rc != LMN_OK && !report->first_failure[0]) snprintf(report->first_failure, sizeof report->first_failure, "%s", tmp.last_error.c_str());
  g_create_error = tmp.last_error;
  return rc;
}

int lmn_verify(const uint8_t* proof_bincode, size_t proof_len, const lmn_settings* settings, uint32_t protocol_variant) {
  lmn_config c;
  lmn_default_config(&c);  // PcsConfig::default(), as the reference verifier hard-codes it
  c.protocol_variant = protocol_variant;
  return lmn_verify_with_config(proof_bincode, proof_len, settings, &c);
}

// page-locked host memory for host-resident trace rows (no context: usable by every context of the process)
int lmn_host_alloc(size_t bytes, void** host_out) {
  if (!host_out || bytes == 0) return LMN_ERR_INVALID_ARGUMENT;
  *host_out = nullptr;
  return host_guard([&] { *host_out = lmn_host_alloc_pinned(bytes); });
}
void lmn_host_free(void* host) {
  if (host) lmn_host_free_pinned(host);
}
int lmn_host_register(void* host, size_t bytes) {
  if (!host || bytes == 0) return LMN_ERR_INVALID_ARGUMENT;
  return host_guard([&] { lmn_host_register_range(host, bytes); });
}
int lmn_host_unregister(void* host) {
  if (!host) return LMN_ERR_INVALID_ARGUMENT;
  return host_guard([&] { lmn_host_unregister_range(host); });
}

// ---- row sinks (trace_gen.cpp RowSink).  No call here takes the context's lock: a sink fills while its context proves.
}  // extern "C"
struct lmn_rows {
  lmn::RowSink sink;
  lmn_rows(int device, uint32_t kind, uint64_t capacity) : sink(device, kind, capacity) {}
};
namespace {
template <class F>
int rows_guard(F&& f) {
  lmn_ctx tmp{nullptr, {}};
  const int rc = guard(&tmp, std::forward<F>(f));
  if (rc != LMN_OK) g_create_error = tmp.last_error;
  return rc;
}
}  // namespace
extern "C" {
int lmn_rows_open(lmn_ctx* ctx, uint32_t kind, uint64_t capacity_rows, lmn_rows** out) {
  if (!ctx || !out) return LMN_ERR_INVALID_ARGUMENT;
  *out = nullptr;
#ifdef LMN_BATCH
  g_create_error = "row sinks are not part of the batch library (use libluminair_hip.so)";
  return LMN_ERR_INVALID_ARGUMENT;
#else
  const int device = ctx->impl->device();
  return rows_guard([&] { *out = new lmn_rows(device, kind, capacity_rows); });
#endif
}
int lmn_rows_push(lmn_rows* rows, const uint32_t* host_rows, uint64_t n) {
  if (!rows || !host_rows) return LMN_ERR_INVALID_ARGUMENT;
  return rows_guard([&] { rows->sink.push(host_rows, n, false); });
}
int lmn_rows_push_pinned(lmn_rows* rows, const uint32_t* host_rows, uint64_t n) {
  if (!rows || !host_rows) return LMN_ERR_INVALID_ARGUMENT;
  return rows_guard([&] { rows->sink.push(host_rows, n, true); });
}
int lmn_rows_sync(lmn_rows* rows) {
  if (!rows) return LMN_ERR_INVALID_ARGUMENT;
  return rows_guard([&] { rows->sink.sync(); });
}
int lmn_rows_finish(lmn_rows* rows, lmn_table* table_out) {
  if (!rows || !table_out) return LMN_ERR_INVALID_ARGUMENT;
  return rows_guard([&] { rows->sink.finish(table_out); });
}
uint64_t lmn_rows_count(const lmn_rows* rows) { return rows ? rows->sink.count() : 0; }
int lmn_rows_reset(lmn_rows* rows) {
  if (!rows) return LMN_ERR_INVALID_ARGUMENT;
  return rows_guard([&] { rows->sink.reset(); });
}
void lmn_rows_close(lmn_rows* rows) { delete rows; }

// ---- device producers that fill a sink (trace_gen.cpp: the Context producers with TraceTarget::into).  These do take the context's lock - the
// launch runs on its stream, as every lmn_trace_* launch does - and the sink's behind it.  Null pointers are refused where
// the single forms refuse them, with the argument's name in lmn_last_error(ctx).
}  // extern "C"
namespace {
template <class F>
int rows_append(lmn_ctx* ctx, lmn_rows* rows, const char* call, const char* null_arg /* the first null argument, if any */, F&& f) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  const std::string name = std::string(call) + ": ";
#ifdef LMN_BATCH
  (void)rows; (void)null_arg; (void)f;
  return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, (name + "rows: row sinks are not part of the batch library (use libluminair_hip.so)").c_str());
#else
  if (!rows) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, (name + "null rows").c_str());
  if (null_arg) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, (name + "null " + null_arg).c_str());
  return guard(ctx, [&] { f(rows->sink); });
#endif
}
}  // namespace
extern "C" {
int lmn_rows_append_elementwise_v(lmn_ctx* ctx, lmn_rows* rows, uint32_t kind, const int32_t* lhs_dev, const lmn_view* lhs_view,
                                  const int32_t* rhs_dev, const lmn_view* rhs_view, uint64_t n, const lmn_node_info* info,
                                  uint32_t* range_check_mult_dev, int32_t* out_dev, uint32_t* refused_dev) {
  const char* call = "lmn_rows_append_elementwise_v";
  return rows_append(ctx, rows, call, !lhs_dev ? "lhs_dev" : !info ? "info" : nullptr, [&](lmn::RowSink& sink) {
    ctx->impl->elementwise(TraceTarget::into(call, sink, out_dev, refused_dev), kind, {lhs_dev, lhs_view}, {rhs_dev, rhs_view}, n,
                           *info, range_check_mult_dev);
  });
}
int lmn_rows_append_contiguous(lmn_ctx* ctx, lmn_rows* rows, const int32_t* input_dev, uint64_t in_size, const lmn_view* view,
                               uint64_t out_size, const lmn_node_info* info, int32_t* out_dev, uint32_t* refused_dev) {
  const char* call = "lmn_rows_append_contiguous";
  return rows_append(ctx, rows, call, !input_dev ? "input_dev" : !info ? "info" : nullptr, [&](lmn::RowSink& sink) {
    ctx->impl->contiguous(TraceTarget::into(call, sink, out_dev, refused_dev), {input_dev, view}, in_size, out_size, *info);
  });
}
int lmn_rows_append_reduce(lmn_ctx* ctx, lmn_rows* rows, uint32_t is_max, const int32_t* input_dev, uint64_t front, uint64_t dim,
                           uint64_t back, const lmn_node_info* info, int32_t* out_dev, uint32_t* refused_dev) {
  const char* call = "lmn_rows_append_reduce";
  return rows_append(ctx, rows, call, !input_dev ? "input_dev" : !info ? "info" : nullptr, [&](lmn::RowSink& sink) {
    ctx->impl->reduce(TraceTarget::into(call, sink, out_dev, refused_dev), is_max != 0, {input_dev}, front, dim, back, *info);
  });
}
int lmn_rows_append_lut_ranges(lmn_ctx* ctx, lmn_rows* rows, uint32_t kind, const int32_t* input_dev, const lmn_view* view,
                               uint64_t n, const lmn_node_info* info, const uint32_t* lut_col1_dev, const lmn_range* ranges,
                               uint32_t n_ranges, uint32_t* mult_dev, int32_t* out_dev, uint32_t* refused_dev) {
  const char* call = "lmn_rows_append_lut_ranges";
  return rows_append(ctx, rows, call,
                     !input_dev ? "input_dev" : !info ? "info" : !lut_col1_dev ? "lut_col1_dev" : !mult_dev ? "mult_dev" : nullptr,
                     [&](lmn::RowSink& sink) {
                       ctx->impl->lut(TraceTarget::into(call, sink, out_dev, refused_dev), kind, {input_dev, view}, n, *info,
                                      lut_col1_dev, ranges, n_ranges, mult_dev);
                     });
}

// (a null src_dev is named by Context::inputs_float, behind an unknown dtype)
int lmn_rows_append_inputs_float(lmn_ctx* ctx, lmn_rows* rows, uint32_t dtype, const void* src_dev, uint64_t n,
                                 const lmn_node_info* info, int32_t* out_dev, uint32_t* refused_dev) {
  const char* call = "lmn_rows_append_inputs_float";
  return rows_append(ctx, rows, call, !info ? "info" : nullptr, [&](lmn::RowSink& sink) {
    ctx->impl->inputs_float(TraceTarget::into(call, sink, out_dev, refused_dev), dtype, {src_dev}, n, *info);
  });
}

int lmn_upload(lmn_ctx* ctx, const void* host, size_t bytes, void** device_out) {
  if (!ctx || !host || !device_out) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { *device_out = ctx->impl->upload(host, bytes); });
}

void lmn_device_free(lmn_ctx* ctx, void* p) {
  if (ctx && p) ctx->impl->device_free(p);
}

int lmn_op_interpolate(lmn_ctx* ctx, uint32_t* cols, uint32_t ncols, uint32_t log_size) {
  if (!ctx || !cols || ncols == 0 || log_size < 1) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->op_interpolate(cols, ncols, log_size); });
}

int lmn_op_evaluate(lmn_ctx* ctx, const uint32_t* coeffs, uint32_t ncols, uint32_t log_coeffs, uint32_t log_domain,
                    uint32_t* evals_out) {
  if (!ctx || !coeffs || !evals_out || ncols == 0 || log_domain < 1) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->op_evaluate(coeffs, ncols, log_coeffs, log_domain, evals_out); });
}

int lmn_op_merkle_root(lmn_ctx* ctx, const uint32_t* const* cols, const uint32_t* log_sizes, uint32_t ncols,
                       uint8_t root_out[32]) {
  if (!ctx || !root_out || (ncols && (!cols || !log_sizes))) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->op_merkle_root(cols, log_sizes, ncols, root_out); });
}

int lmn_op_eval_at_point(lmn_ctx* ctx, const uint32_t* coeffs, uint32_t log_size, const uint32_t point_xy[8],
                         uint32_t value_out[4]) {
  if (!ctx || !coeffs || !point_xy || !value_out) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->op_eval_at_point(coeffs, log_size, point_xy, value_out); });
}

int lmn_op_fft_selftest(lmn_ctx* ctx, uint32_t log_size, uint32_t ncols) {
  if (!ctx || log_size < 1 || ncols == 0) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->op_fft_selftest(log_size, ncols); });
}

}  // extern "C"

int lmn_op_accumulate_quotients(lmn_ctx* ctx, uint32_t log_size, const uint32_t* const* cols, uint32_t ncols,
                                const uint32_t* sample_col, const uint32_t* sample_point, const uint32_t* sample_values,
                                uint32_t nsamples, const uint32_t* points_xy, uint32_t npoints, const uint32_t alpha[4],
                                uint32_t* out) {
  if (!ctx || !cols || !sample_col || !sample_point || !sample_values || !points_xy || !alpha || !out)
    return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] {
    ctx->impl->op_accumulate_quotients(log_size, cols, ncols, sample_col, sample_point, sample_values, nsamples, points_xy,
                                       npoints, alpha, out);
  });
}

int lmn_op_fold_line(lmn_ctx* ctx, const uint32_t* src, uint32_t log_src, const uint32_t alpha[4], uint32_t* dst) {
  if (!ctx || !src || !alpha || !dst) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->op_fold(0, dst, src, log_src, alpha); });
}

int lmn_op_fold_circle_into_line(lmn_ctx* ctx, uint32_t* dst, const uint32_t* src, uint32_t log_src, const uint32_t alpha[4]) {
  if (!ctx || !src || !alpha || !dst) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->op_fold(1, dst, src, log_src, alpha); });
}

int lmn_op_grind(const uint8_t digest[32], uint32_t pow_bits, uint32_t protocol_variant, uint64_t* nonce_out) {
  if (!digest || !nonce_out || pow_bits > 40 || (protocol_variant & ~LMN_PV_ALL)) return LMN_ERR_INVALID_ARGUMENT;
  lmn::Channel ch(protocol_variant);
  lmn::Hash32 d;
  memcpy(d.w, digest, 32);
  ch.set_digest(d);
  *nonce_out = ch.grind(pow_bits);
  return LMN_OK;
}

int lmn_ctx_grind(lmn_ctx* ctx, const uint8_t digest[32], uint32_t pow_bits, uint32_t protocol_variant, uint64_t* nonce_out) {
  if (!ctx || !digest || !nonce_out || pow_bits > 40 || (protocol_variant & ~LMN_PV_ALL)) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] {
    lmn::Hash32 d;
    memcpy(d.w, digest, 32);
    *nonce_out = ctx->impl->op_grind(d, pow_bits, protocol_variant);
  });
}

uint64_t lmn_ctx_counter(const lmn_ctx* ctx, int which) { return ctx && ctx->impl ? ctx->impl->counter(which) : 0; }

int lmn_ctx_grind_many(lmn_ctx* ctx, const uint8_t* digests, uint32_t n, uint32_t pow_bits, uint32_t protocol_variant,
                       uint64_t* nonces_out) {
  if (!ctx) {
    g_create_error = "lmn_ctx_grind_many: ctx is null";
    return LMN_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) return LMN_OK;
  if (!digests) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_ctx_grind_many: digests is null");
  if (!nonces_out) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_ctx_grind_many: nonces_out is null");
  if (n > LMN_GRIND_MANY_MAX) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_ctx_grind_many: n exceeds LMN_GRIND_MANY_MAX");
  if (pow_bits > 40) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_ctx_grind_many: pow_bits exceeds 40");
  if (protocol_variant & ~LMN_PV_ALL)
    return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_ctx_grind_many: protocol_variant has unknown bits");
  return guard(ctx, [&] { ctx->impl->op_grind_many(digests, n, pow_bits, protocol_variant, nonces_out); });
}

int lmn_device_alloc(lmn_ctx* ctx, size_t bytes, void** device_out) {
  if (!ctx || !device_out) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { *device_out = ctx->impl->device_alloc(bytes); });
}

int lmn_download(lmn_ctx* ctx, const void* device, void* host, size_t bytes) {
  if (!ctx || !device || !host) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->download(device, host, bytes); });
}

int lmn_trace_elementwise(lmn_ctx* ctx, uint32_t kind, const int32_t* lhs_dev, const int32_t* rhs_dev, uint64_t n,
                          const lmn_node_info* info, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev) {
  return lmn_trace_elementwise_v(ctx, kind, lhs_dev, nullptr, rhs_dev, nullptr, n, info, rows_dev, row_offset, out_dev);
}

int lmn_trace_sum_reduce(lmn_ctx* ctx, const int32_t* input_dev, uint64_t front, uint64_t dim, uint64_t back,
                         const lmn_node_info* info, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev) {
  if (!ctx || !input_dev || !info || !rows_dev) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] {
    ctx->impl->reduce(TraceTarget::table(rows_dev, row_offset, out_dev), false, {input_dev}, front, dim, back, *info);
  });
}

int lmn_trace_elementwise_v(lmn_ctx* ctx, uint32_t kind, const int32_t* lhs_dev, const lmn_view* lhs_view,
                            const int32_t* rhs_dev, const lmn_view* rhs_view, uint64_t n, const lmn_node_info* info,
                            uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev) {
  if (!ctx || !lhs_dev || !info || !rows_dev || kind == LMN_KIND_LESS_THAN) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] {
    ctx->impl->elementwise(TraceTarget::table(rows_dev, row_offset, out_dev), kind, {lhs_dev, lhs_view}, {rhs_dev, rhs_view}, n,
                           *info);
  });
}

int lmn_trace_contiguous(lmn_ctx* ctx, const int32_t* input_dev, uint64_t in_size, const lmn_view* view, uint64_t out_size,
                         const lmn_node_info* info, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev) {
  if (!ctx || !input_dev || !info || !rows_dev) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] {
    ctx->impl->contiguous(TraceTarget::table(rows_dev, row_offset, out_dev), {input_dev, view}, in_size, out_size, *info);
  });
}

int lmn_trace_lut(lmn_ctx* ctx, uint32_t kind, const int32_t* input_dev, const lmn_view* view, uint64_t n,
                  const lmn_node_info* info, const uint32_t* lut_col1_dev, int32_t lo, uint32_t lut_len,
                  uint32_t* mult_dev, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev) {
  if (lut_len == 0) return LMN_ERR_INVALID_ARGUMENT;
  const lmn_range one{(int64_t)lo, (int64_t)lo + (int64_t)lut_len - 1};
  return lmn_trace_lut_ranges(ctx, kind, input_dev, view, n, info, lut_col1_dev, &one, 1, mult_dev, rows_dev, row_offset, out_dev);
}

int lmn_trace_lut_ranges(lmn_ctx* ctx, uint32_t kind, const int32_t* input_dev, const lmn_view* view, uint64_t n,
                         const lmn_node_info* info, const uint32_t* lut_col1_dev, const lmn_range* ranges, uint32_t n_ranges,
                         uint32_t* mult_dev, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev) {
  if (!ctx || !input_dev || !info || !lut_col1_dev || !mult_dev || !rows_dev) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] {
    ctx->impl->lut(TraceTarget::table(rows_dev, row_offset, out_dev), kind, {input_dev, view}, n, *info, lut_col1_dev, ranges,
                   n_ranges, mult_dev);
  });
}

int lmn_trace_less_than(lmn_ctx* ctx, const int32_t* lhs_dev, const lmn_view* lhs_view, const int32_t* rhs_dev,
                        const lmn_view* rhs_view, uint64_t n, const lmn_node_info* info, uint32_t* range_check_mult_dev,
                        uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev) {
  if (!ctx || !lhs_dev || !rhs_dev || !info || !range_check_mult_dev || !rows_dev) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] {
    ctx->impl->elementwise(TraceTarget::table(rows_dev, row_offset, out_dev), LMN_KIND_LESS_THAN, {lhs_dev, lhs_view},
                           {rhs_dev, rhs_view}, n, *info, range_check_mult_dev);
  });
}

int lmn_trace_max_reduce(lmn_ctx* ctx, const int32_t* input_dev, uint64_t front, uint64_t dim, uint64_t back,
                         const lmn_node_info* info, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev) {
  if (!ctx || !input_dev || !info || !rows_dev) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] {
    ctx->impl->reduce(TraceTarget::table(rows_dev, row_offset, out_dev), true, {input_dev}, front, dim, back, *info);
  });
}

// ---- the many-member producers: n_members == 0 is LMN_OK and touches nothing (as lmn_ctx_grind_many); null pointers are
// refused where the single forms refuse them, with the argument's name in lmn_last_error
namespace {
template <class F>
int producer_call(lmn_ctx* ctx, uint32_t n_members, const char* call, const char* null_arg /* the first null argument, if any */, F&& f) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  if (n_members == 0) return LMN_OK;
  if (null_arg) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, (std::string(call) + ": null " + null_arg).c_str());
  return guard(ctx, f);
}
}  // namespace
int lmn_trace_many_elementwise_v(lmn_ctx* ctx, uint32_t kind, const int32_t* lhs_dev, const lmn_view* lhs_view,
                                 uint64_t lhs_member_stride, const int32_t* rhs_dev, const lmn_view* rhs_view,
                                 uint64_t rhs_member_stride, uint64_t n, const lmn_node_info* info, uint32_t n_members,
                                 uint32_t* rows_dev, uint64_t row_offset, uint64_t rows_member_stride, int32_t* out_dev,
                                 uint64_t out_member_stride, uint32_t* range_check_mult_dev,
                                 uint64_t range_check_mult_member_stride, uint32_t* refused_dev) {
  const char* call = "lmn_trace_many_elementwise_v";
  return producer_call(ctx, n_members, call, !lhs_dev ? "lhs_dev" : !info ? "info" : !rows_dev ? "rows_dev" : nullptr, [&] {
    ctx->impl->elementwise(
        TraceTarget::many(call, n_members, rows_dev, row_offset, rows_member_stride, out_dev, out_member_stride, refused_dev), kind,
        {lhs_dev, lhs_view, lhs_member_stride}, {rhs_dev, rhs_view, rhs_member_stride}, n, *info, range_check_mult_dev,
        range_check_mult_member_stride);
  });
}

int lmn_trace_many_contiguous(lmn_ctx* ctx, const int32_t* input_dev, uint64_t input_member_stride, uint64_t in_size,
                              const lmn_view* view, uint64_t out_size, const lmn_node_info* info, uint32_t n_members,
                              uint32_t* rows_dev, uint64_t row_offset, uint64_t rows_member_stride, int32_t* out_dev,
                              uint64_t out_member_stride, uint32_t* refused_dev) {
  const char* call = "lmn_trace_many_contiguous";
  return producer_call(ctx, n_members, call, !input_dev ? "input_dev" : !info ? "info" : !rows_dev ? "rows_dev" : nullptr, [&] {
    ctx->impl->contiguous(
        TraceTarget::many(call, n_members, rows_dev, row_offset, rows_member_stride, out_dev, out_member_stride, refused_dev),
        {input_dev, view, input_member_stride}, in_size, out_size, *info);
  });
}

int lmn_trace_many_reduce(lmn_ctx* ctx, uint32_t is_max, const int32_t* input_dev, uint64_t input_member_stride, uint64_t front,
                          uint64_t dim, uint64_t back, const lmn_node_info* info, uint32_t n_members, uint32_t* rows_dev,
                          uint64_t row_offset, uint64_t rows_member_stride, int32_t* out_dev, uint64_t out_member_stride,
                          uint32_t* refused_dev) {
  const char* call = "lmn_trace_many_reduce";
  return producer_call(ctx, n_members, call, !input_dev ? "input_dev" : !info ? "info" : !rows_dev ? "rows_dev" : nullptr, [&] {
    ctx->impl->reduce(
        TraceTarget::many(call, n_members, rows_dev, row_offset, rows_member_stride, out_dev, out_member_stride, refused_dev),
        is_max != 0, {input_dev, nullptr, input_member_stride}, front, dim, back, *info);
  });
}

int lmn_trace_many_lut_ranges(lmn_ctx* ctx, uint32_t kind, const int32_t* input_dev, const lmn_view* view,
                              uint64_t input_member_stride, uint64_t n, const lmn_node_info* info, const uint32_t* lut_col1_dev,
                              const lmn_range* ranges, uint32_t n_ranges, uint32_t n_members, uint32_t* mult_dev,
                              uint64_t mult_member_stride, uint32_t* rows_dev, uint64_t row_offset, uint64_t rows_member_stride,
                              int32_t* out_dev, uint64_t out_member_stride, uint32_t* refused_dev) {
  const char* call = "lmn_trace_many_lut_ranges";
  const char* null_arg = !input_dev ? "input_dev" : !info ? "info" : !lut_col1_dev ? "lut_col1_dev" : !mult_dev ? "mult_dev"
                         : !rows_dev ? "rows_dev" : nullptr;
  return producer_call(ctx, n_members, call, null_arg, [&] {
    ctx->impl->lut(TraceTarget::many(call, n_members, rows_dev, row_offset, rows_member_stride, out_dev, out_member_stride, refused_dev),
                   kind, {input_dev, view, input_member_stride}, n, *info, lut_col1_dev, ranges, n_ranges, mult_dev,
                   mult_member_stride);
  });
}

int lmn_eval_elementwise_v(lmn_ctx* ctx, uint32_t kind, const int32_t* lhs_dev, const lmn_view* lhs_view, const int32_t* rhs_dev,
                           const lmn_view* rhs_view, uint64_t n, int32_t* out_dev, int32_t* minmax_dev, uint32_t* refused_dev) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  if (!lhs_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_eval_elementwise_v: null lhs_dev");
  if (!out_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_eval_elementwise_v: null out_dev");
  return guard(ctx, [&] {
    ctx->impl->eval_elementwise(kind, lhs_dev, lhs_view, rhs_dev, rhs_view, n, out_dev, minmax_dev, refused_dev);
  });
}

int lmn_eval_reduce(lmn_ctx* ctx, uint32_t is_max, const int32_t* input_dev, uint64_t front, uint64_t dim, uint64_t back,
                    int32_t* out_dev, int32_t* minmax_dev, uint32_t* refused_dev) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  if (!input_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_eval_reduce: null input_dev");
  if (!out_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_eval_reduce: null out_dev");
  return guard(ctx, [&] { ctx->impl->eval_reduce(is_max != 0, input_dev, front, dim, back, out_dev, minmax_dev, refused_dev); });
}

uint32_t lmn_eval_reduce_split(uint64_t dim, uint64_t back) { return lmn::eval_reduce_by_wave(dim, back) ? 1u : 0u; }

int lmn_eval_lut_ranges(lmn_ctx* ctx, uint32_t kind, const int32_t* input_dev, const lmn_view* view, uint64_t n,
                        const uint32_t* lut_col1_dev, const lmn_range* ranges, uint32_t n_ranges, int32_t* out_dev,
                        int32_t* minmax_dev, uint32_t* refused_dev) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  if (!input_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_eval_lut_ranges: null input_dev");
  if (!lut_col1_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_eval_lut_ranges: null lut_col1_dev");
  if (!out_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_eval_lut_ranges: null out_dev");
  return guard(ctx, [&] {
    ctx->impl->eval_lut(kind, input_dev, view, n, lut_col1_dev, ranges, n_ranges, out_dev, minmax_dev, refused_dev);
  });
}

int lmn_tensor_range(lmn_ctx* ctx, const int32_t* buf_dev, uint64_t n, int32_t* minmax_dev) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  if (!buf_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_tensor_range: null buf_dev");
  if (!minmax_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_tensor_range: null minmax_dev");
  return guard(ctx, [&] { ctx->impl->tensor_range(buf_dev, n, minmax_dev); });
}

// ---- float tensors in and out (trace_gen.cpp): every refusal names its argument; dtype, src_dev and n are checked by the
// context, in that order, in front of the sibling form's own rules
int lmn_trace_inputs_float(lmn_ctx* ctx, uint32_t dtype, const void* src_dev, uint64_t n, const lmn_node_info* info,
                           uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev) {
  const char* call = "lmn_trace_inputs_float";
  return producer_call(ctx, 1, call, !info ? "info" : !rows_dev ? "rows_dev" : nullptr, [&] {
    ctx->impl->inputs_float(TraceTarget::table(rows_dev, row_offset, out_dev, call), dtype, {src_dev}, n, *info);
  });
}

int lmn_trace_many_inputs_float(lmn_ctx* ctx, uint32_t dtype, const void* src_dev, uint64_t src_member_stride, uint64_t n,
                                const lmn_node_info* info, uint32_t n_members, uint32_t* rows_dev, uint64_t row_offset,
                                uint64_t rows_member_stride, int32_t* out_dev, uint64_t out_member_stride, uint32_t* refused_dev) {
  const char* call = "lmn_trace_many_inputs_float";
  return producer_call(ctx, n_members, call, !info ? "info" : !rows_dev ? "rows_dev" : nullptr, [&] {
    ctx->impl->inputs_float(
        TraceTarget::many(call, n_members, rows_dev, row_offset, rows_member_stride, out_dev, out_member_stride, refused_dev), dtype,
        {src_dev, nullptr, src_member_stride}, n, *info);
  });
}

int lmn_eval_inputs_float(lmn_ctx* ctx, uint32_t dtype, const void* src_dev, uint64_t n, int32_t* out_dev, int32_t* minmax_dev,
                          uint32_t* refused_dev) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  if (!out_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_eval_inputs_float: null out_dev");
  return guard(ctx, [&] { ctx->impl->eval_inputs_float(dtype, src_dev, n, out_dev, minmax_dev, refused_dev); });
}

int lmn_tensor_to_float(lmn_ctx* ctx, uint32_t dtype, const int32_t* src_dev, uint64_t n, void* dst_dev) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  if (!src_dev) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_tensor_to_float: null src_dev");
  return guard(ctx, [&] { ctx->impl->tensor_to_float(dtype, src_dev, n, dst_dev); });
}

int lmn_trace_check(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_settings* settings,
                    lmn_trace_report* report) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  if (!report) return set_error(ctx, LMN_ERR_INVALID_ARGUMENT, "lmn_trace_check: null report");
  memset(report, 0, sizeof *report);
  return guard(ctx, [&] { ctx->impl->trace_check(tables, n_tables, settings, *report); });
}

namespace lmn {
void rccl_unique_id(uint8_t* out);
}
int lmn_ctx_set_shard(lmn_ctx* ctx, uint32_t rank, uint32_t world, uint32_t fri_min_log, const lmn_collective* coll) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] {
    // validate first: a rejected call leaves the context's current sharding (and its RCCL transport) untouched
    lmn::Context::check_shard_args(rank, world, fri_min_log, coll);
    ctx->impl->clear_shard();  // releases a previous built-in RCCL transport, if any
    ctx->impl->set_shard(rank, world, fri_min_log, coll);
  });
}
int lmn_rccl_unique_id(uint8_t id_out[LMN_RCCL_ID_BYTES]) {
  if (!id_out) return LMN_ERR_INVALID_ARGUMENT;
  lmn_ctx tmp{nullptr, {}};
  int rc = guard(&tmp, [&] { lmn::rccl_unique_id(id_out); });
  g_create_error = tmp.last_error;
  return rc;
}
int lmn_ctx_set_shard_rccl(lmn_ctx* ctx, uint32_t rank, uint32_t world, uint32_t fri_min_log,
                           const uint8_t id[LMN_RCCL_ID_BYTES]) {
  if (!ctx || !id) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->set_shard_rccl(rank, world, fri_min_log, id); });
}
int lmn_ctx_clear_shard(lmn_ctx* ctx) {
  if (!ctx) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->clear_shard(); });
}

// ---- LUT columns from the reference's layouts (preprocessed.rs:34-46, 351-383, 434-466, 517-549)
static int lut_values(const lmn_range* ranges, uint32_t n, std::vector<int64_t>& vals) {
  if (!ranges || n == 0) return LMN_ERR_INVALID_ARGUMENT;
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (ranges[i].hi < ranges[i].lo || ranges[i].lo <= -(1ll << 30) || ranges[i].hi >= (1ll << 30)) return LMN_ERR_INVALID_ARGUMENT;
    total += (uint64_t)(ranges[i].hi - ranges[i].lo + 1);
    if (total > (1ull << 26)) return LMN_ERR_INVALID_ARGUMENT;
  }
  vals.reserve(total);
  for (uint32_t i = 0; i < n; ++i)
    for (int64_t v = ranges[i].lo; v <= ranges[i].hi; ++v) vals.push_back(v);
  std::sort(vals.begin(), vals.end());
  vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
  return LMN_OK;
}
int lmn_lut_log_size(const lmn_range* ranges, uint32_t n_ranges, uint32_t* log_size_out) {
  if (!log_size_out) return LMN_ERR_INVALID_ARGUMENT;
  // LookupLayout::new counts the values of the (already coalesced) ranges: value_count, preprocessed.rs:117-119
  uint64_t count = 0;
  if (!ranges || n_ranges == 0) return LMN_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < n_ranges; ++i) {
    // same bounds as lut_values(): Fixed<12> values inside (-2^30, 2^30), so hi - lo + 1 cannot overflow
    if (ranges[i].hi < ranges[i].lo || ranges[i].lo <= -(1ll << 30) || ranges[i].hi >= (1ll << 30)) return LMN_ERR_INVALID_ARGUMENT;
    count += (uint64_t)(ranges[i].hi - ranges[i].lo + 1);
    if (count > (1ull << 26)) return LMN_ERR_INVALID_ARGUMENT;
  }
  // calculate_log_size: ceil(count / 16) rounded up to a power of two, times 16 (LOG_N_LANES = 4)
  uint64_t packs = (count + 15) >> 4, p2 = 1;
  uint32_t lg = 0;
  while (p2 < packs) {
    p2 <<= 1;
    ++lg;
  }
  *log_size_out = lg + 4;
  return LMN_OK;
}
int lmn_lut_from_ranges(uint32_t lut_kind, const lmn_range* ranges, uint32_t n_ranges, uint32_t log_size, uint32_t* col0_out,
                        uint32_t* col1_out) {
  return lmn_lut_from_ranges_r(lut_kind, ranges, n_ranges, log_size, LMN_ROUND_HALF_AWAY, col0_out, col1_out);
}

int lmn_lut_from_ranges_r(uint32_t lut_kind, const lmn_range* ranges, uint32_t n_ranges, uint32_t log_size, uint32_t rounding,
                          uint32_t* col0_out, uint32_t* col1_out) {
  if (!col0_out || !col1_out || lut_kind > LMN_LUT_LOG2 || log_size > 26 || rounding > LMN_ROUND_FLOOR)
    return LMN_ERR_INVALID_ARGUMENT;
  std::vector<int64_t> vals;
  int rc = lut_values(ranges, n_ranges, vals);
  if (rc != LMN_OK) return rc;
  const uint64_t n = 1ull << log_size;
  if (vals.size() > n) return LMN_ERR_INVALID_ARGUMENT;
  const double scale = 4096.0;
  auto to_m31 = [](int64_t v) { return (uint32_t)(v >= 0 ? v : (int64_t)lmn::P31 + v); };  // Fixed::to_m31
  for (uint64_t i = 0; i < n; ++i) col0_out[i] = col1_out[i] = 0u;
  for (size_t i = 0; i < vals.size(); ++i) {
    const double x = (double)vals[i] / scale;
    double y;
    if (lut_kind == LMN_LUT_SIN) {
      y = std::sin(x);
    } else if (lut_kind == LMN_LUT_EXP2) {
      y = std::exp2(x);
    } else {
      // Divergence from the reference, on purpose: Log2PreProcessed::gen_column (preprocessed.rs:517-549) feeds
      // x <= 0 to f64::log2 and stores the saturated cast of NaN / -inf; such a row can never be looked up by a
      // valid trace (log2 of a non-positive input has no fixed-point value), so a layout that contains one is
      // rejected here instead of committing to a meaningless LUT row.
      if (vals[i] <= 0) return LMN_ERR_INVALID_ARGUMENT;
      y = std::log2(x);
    }
    const double ys = y * scale;
    const double r = rounding == LMN_ROUND_HALF_AWAY   ? std::round(ys)
                     : rounding == LMN_ROUND_HALF_EVEN ? std::nearbyint(ys)   // default FE_TONEAREST = ties to even
                     : rounding == LMN_ROUND_TRUNC     ? std::trunc(ys)
                                                       : std::floor(ys);
    if (!(std::fabs(r) < (double)(1ll << 30))) return LMN_ERR_INVALID_ARGUMENT;
    col0_out[i] = to_m31(vals[i]);
    col1_out[i] = to_m31((int64_t)r);
  }
  return LMN_OK;
}

int lmn_device_copy(lmn_ctx* ctx, void* device_dst, const void* device_src, size_t bytes) {
  if (!ctx || !device_dst || !device_src) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->device_copy(device_dst, device_src, bytes); });
}

int lmn_upload_to(lmn_ctx* ctx, const void* host, size_t bytes, void* device_dst) {
  if (!ctx || !host || !device_dst) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->upload_to(host, bytes, device_dst); });
}

int lmn_op_evaluate_block(lmn_ctx* ctx, const uint32_t* coeffs, uint32_t ncols, uint32_t log_coeffs, uint32_t log_domain,
                          uint32_t log_blocks, uint32_t block, uint32_t* evals_out) {
  if (!ctx || !coeffs || !evals_out || ncols == 0) return LMN_ERR_INVALID_ARGUMENT;
  return guard(ctx, [&] { ctx->impl->op_evaluate_block(coeffs, ncols, log_coeffs, log_domain, log_blocks, block, evals_out); });
}
