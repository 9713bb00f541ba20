// The step before the path: `process_trace` of the reference's operators on device-resident tensors
// (crates/graph/src/op/prim.rs), filling trace-table rows in HBM.  Host side of the lmn_trace_*, lmn_trace_many_*,
// lmn_rows_append_* and lmn_eval_* entry points: a producer (Context::elementwise, contiguous, reduce, lut, inputs_float)
// states what is computed and its argument rules once; a TraceTarget states where the rows and outputs go.
#include "prove_run.h"

#include <algorithm>
#include <optional>

namespace lmn {

static TraceNode trace_node(const lmn_node_info& info) {
  auto m31 = [](int64_t v) { return (uint32_t)(((v % (int64_t)P31) + (int64_t)P31) % (int64_t)P31); };
  TraceNode nd{};
  nd.node_id = info.node_id;
  nd.lhs_id = info.input_ids[0];
  nd.rhs_id = info.input_ids[1];
  nd.lhs_mult = m31(info.input_mults[0]);
  nd.rhs_mult = m31(info.input_mults[1]);
  nd.out_mult = info.is_final_output ? 0u : m31(info.num_consumers);
  return nd;
}

// ------------------------------------------------------------------------------------ the producers' argument rules
// Each rule is stated once.  The trace forms answer a broken rule with the reference's own codes and texts (trace_fail); the
// eval forms name the argument instead, so a rule set takes the caller's way to fail: fail(rule) does not return.
namespace {
struct RuleText {
  int code;
  const char* text;
};
[[noreturn]] void trace_fail(const RuleText& t) { throw LmnError(t.code, t.text); }
[[noreturn]] void bad_argument(const char* call, const std::string& why) {
  throw LmnError(LMN_ERR_INVALID_ARGUMENT, std::string(call) + ": " + why);
}
// the rules of `f`, with the entry point's name in front of the text (no name: the text as it is)
template <class F>
auto named_rules(const char* call, F&& f) {
  if (!call) return f();
  try {
    return f();
  } catch (const LmnError& e) {
    throw LmnError(e.code, std::string(call) + ": " + e.what());
  }
}

TraceView trace_view(const lmn_view* v, uint64_t n) {
  TraceView t{};
  if (!v) return t;
  if (v->ndim < 1 || v->ndim > 4) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "view: ndim must be 1..4");
  uint64_t prod = 1;
  t.ndim = v->ndim;
  for (uint32_t k = 0; k < v->ndim; ++k) {
    if (v->shape[k] == 0) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "view: empty dimension");
    t.shape[k] = v->shape[k];
    t.strides[k] = v->strides[k];
    prod *= v->shape[k];
  }
  if (v->offset < 0) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "view: negative offset");
  t.offset = v->offset;
  if (prod != n) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "view: shape does not match the element count");
  return t;
}

// the shape rules of the reduce producers
void check_reduce_shape(uint64_t front, uint64_t dim, uint64_t back) {
  if (front == 0 || dim == 0 || back == 0) throw LmnError(LMN_ERR_EMPTY_TRACE, "TraceError::EmptyTrace");
  if (front * back * dim >= (1ull << 31)) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "tensor too large");
}

// the argument rules of the LUT producers; lut_rows = the LUT rows the ranges enumerate
enum LutRule { LUT_KIND, LUT_EMPTY, LUT_TOO_LARGE, LUT_NO_RANGES, LUT_N_RANGES, LUT_ORDER, LUT_ROWS };
const RuleText kTraceLutRules[] = {
    {LMN_ERR_INVALID_ARGUMENT, "trace_lut: kind must be Sin, Exp2 or Log2"},
    {LMN_ERR_EMPTY_TRACE, "TraceError::EmptyTrace"},
    {LMN_ERR_INVALID_ARGUMENT, "bad sizes"},
    {LMN_ERR_INVALID_ARGUMENT, "trace_lut: 1..16 value ranges"},
    {LMN_ERR_INVALID_ARGUMENT, "trace_lut: 1..16 value ranges"},
    {LMN_ERR_INVALID_ARGUMENT, "trace_lut: ranges must be ascending, disjoint and inside (-2^30, 2^30)"},
    {LMN_ERR_INVALID_ARGUMENT, "trace_lut: LUT larger than 2^26 rows"}};
template <class Fail>
LutRanges lut_ranges(uint32_t kind, uint64_t n, const lmn_range* ranges, uint32_t n_ranges, uint64_t& lut_rows, Fail&& fail) {
  if (kind != LMN_KIND_SIN && kind != LMN_KIND_EXP2 && kind != LMN_KIND_LOG2) fail(LUT_KIND);
  if (n == 0) fail(LUT_EMPTY);
  if (n >= (1ull << 31)) fail(LUT_TOO_LARGE);
  if (!ranges) fail(LUT_NO_RANGES);
  if (n_ranges == 0 || n_ranges > (uint32_t)LUT_MAX_RANGES) fail(LUT_N_RANGES);
  LutRanges rg{};
  rg.n = (int)n_ranges;
  uint64_t base = 0;
  for (uint32_t k = 0; k < n_ranges; ++k) {
    // ascending, disjoint, inside the Fixed<12> range the LUT generator accepts (coalesce_ranges' output)
    if (ranges[k].hi < ranges[k].lo || ranges[k].lo <= -(1ll << 30) || ranges[k].hi >= (1ll << 30) ||
        (k > 0 && ranges[k].lo <= ranges[k - 1].hi))
      fail(LUT_ORDER);
    rg.lo[k] = (int32_t)ranges[k].lo;
    rg.hi[k] = (int32_t)ranges[k].hi;
    rg.base[k] = (uint32_t)base;
    base += (uint64_t)(ranges[k].hi - ranges[k].lo + 1);
    if (base > (1ull << 26)) fail(LUT_ROWS);
  }
  lut_rows = base;
  return rg;
}

// the argument rules of the elementwise producers
bool elementwise_binary(uint32_t kind) {
  return kind == LMN_KIND_ADD || kind == LMN_KIND_MUL || kind == LMN_KIND_REM || kind == LMN_KIND_LESS_THAN;
}
bool elementwise_unary(uint32_t kind) {
  return kind == LMN_KIND_RECIP || kind == LMN_KIND_SQRT || kind == LMN_KIND_CONTIGUOUS || kind == LMN_KIND_INPUTS;
}
enum ElemRule { ELEM_KIND, ELEM_RHS, ELEM_AUX, ELEM_EMPTY, ELEM_TOO_LARGE };
const RuleText kTraceElemRules[] = {
    {LMN_ERR_INVALID_ARGUMENT, "trace_elementwise: not an elementwise kind"},
    {LMN_ERR_INVALID_ARGUMENT, "trace_elementwise: missing right operand"},
    {LMN_ERR_INVALID_ARGUMENT, "trace_elementwise: LessThan needs the range-check multiplicity table"},
    {LMN_ERR_EMPTY_TRACE, "TraceError::EmptyTrace"},
    {LMN_ERR_INVALID_ARGUMENT, "tensor too large"}};
// aux_missing: the kind is LessThan and the form takes its multiplicity table, but got none
template <class Fail>
void check_elementwise(uint32_t kind, const void* rhs, bool aux_missing, uint64_t n, Fail&& fail) {
  const bool binary = elementwise_binary(kind);
  if (!component_spec((int)kind) || !(binary || elementwise_unary(kind))) fail(ELEM_KIND);
  if (binary && !rhs) fail(ELEM_RHS);
  if (aux_missing) fail(ELEM_AUX);
  if (n == 0) fail(ELEM_EMPTY);
  if (n >= (1ull << 31)) fail(ELEM_TOO_LARGE);
}

// the argument rules of the buffer-rule Contiguous producer; fills nd.phys_n / nd.out_n
TraceView check_contiguous(uint64_t in_size, const lmn_view* view, uint64_t out_size, TraceNode& nd) {
  if (in_size == 0 || out_size == 0) throw LmnError(LMN_ERR_EMPTY_TRACE, "TraceError::EmptyTrace");
  if (in_size >= (1ull << 31) || out_size >= (1ull << 31)) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "tensor too large");
  nd.phys_n = in_size;
  nd.out_n = out_size;
  const TraceView tv = trace_view(view, out_size);
  if (view)  // every element the view addresses must lie inside the buffer
    for (uint64_t corner = 0; corner < (1ull << view->ndim); ++corner) {
      int64_t off = view->offset;
      for (uint32_t k = 0; k < view->ndim; ++k)
        if (corner >> k & 1) off += (int64_t)(view->shape[k] - 1) * view->strides[k];
      if (off < 0 || (uint64_t)off >= in_size) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "contiguous: the view leaves the input buffer");
    }
  else if (out_size > in_size)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "contiguous: output larger than the input buffer without a view");
  return tv;
}

// the float source of the Inputs producers and the destination of lmn_tensor_to_float
void check_float_ptr(const char* call, uint32_t dtype, const void* p, const char* name) {
  if (dtype != LMN_F32 && dtype != LMN_F16 && dtype != LMN_BF16)
    bad_argument(call, "dtype " + std::to_string(dtype) + " is not LMN_F32, LMN_F16 or LMN_BF16");
  if (!p) bad_argument(call, std::string("null ") + name);
  if ((uintptr_t)p % (dtype == LMN_F32 ? 4u : 2u)) bad_argument(call, std::string(name) + " is not aligned to the dtype's element size");
}

// ------------------------------------------------------------------------------------ the destinations
// One producer call's place in its target, between the producer's own argument rules and its launch.  The constructor
// applies the form's rules - everything is refused here, before any launch, and the text names the argument - and gives
// the launcher its TraceOut; done() follows the launch.  No form waits.
//   a table (lmn_trace_*):        the node's rows start at row_offset.
//   many (lmn_trace_many_*):      member m works on base + m * member stride; the strides must hold the node.
//   a sink (lmn_rows_append_*):   the rows go straight into a row sink's columns at its current row count (no
//                                 array-of-structs table, no transpose in front of the proof), inside RowSink::Append.
// n_rows = the node's rows, out_n = elements of one member's output, shared_in = every operand the kind reads has stride 0
struct Placed {
  TraceOut o;
  std::optional<RowSink::Append> append;
  Placed(const TraceTarget& tg, int device, lmn_stream_t stream, uint32_t kind, uint64_t n_rows, uint64_t out_n, bool shared_in) {
    const uint64_t nc = (uint64_t)component_spec((int)kind)->n_cols;
    o.out = tg.out;
    o.refused = tg.refused;
    switch (tg.form) {
      case TraceTarget::TABLE:
        o.form = TraceOut::ROWS;
        o.rows = tg.rows + tg.row_offset * nc;
        break;
      case TraceTarget::MANY:
        if (tg.n_members > LMN_TRACE_MANY_MAX) bad_argument(tg.call, "n_members exceeds LMN_TRACE_MANY_MAX");
        if (tg.row_offset >= (1ull << 31) || tg.rows_ms >= (1ull << 40))
          bad_argument(tg.call, "row_offset / rows_member_stride: table too large");
        if (tg.rows_ms < tg.row_offset + n_rows)
          bad_argument(tg.call, "rows_member_stride is smaller than row_offset + the node's " + std::to_string(n_rows) + " rows");
        if (tg.out && tg.out_ms == 0 && !shared_in)
          bad_argument(tg.call, "out_member_stride 0 (a shared output tensor) needs every operand stride to be 0");
        if (tg.out && tg.out_ms != 0 && tg.out_ms < out_n)
          bad_argument(tg.call, "out_member_stride is smaller than the output's " + std::to_string(out_n) + " elements");
        o.form = TraceOut::MANY;
        o.rows = tg.rows + tg.row_offset * nc;
        o.rows_ms = tg.rows_ms * nc;
        o.n_members = tg.n_members;
        o.out_ms = tg.out_ms;
        break;
      case TraceTarget::SINK:
        append.emplace(*tg.sink, tg.call, device, stream, kind, n_rows);
        o.form = TraceOut::COLS;
        o.cols = append->cols();
        o.col_stride = append->stride();
        o.bad_word = append->bad();
        break;
    }
  }
  void done() {
    if (append) append->done();
  }
};
}  // namespace

// ------------------------------------------------------------------------------------ the producers
// Every producer: select the device, the producer's own rules, the target's, then one launch - stream-ordered with every
// later call on this context (lmn_prove, lmn_download).  Nothing is launched before all rules hold.

// `process_trace` of an Add / Mul / Recip / Sqrt / Rem / LessThan / Inputs node on device tensors (prim.rs:967-1013,
// :1090-1139, :388-431); rc_mult: LessThan's RangeCheckLookup multiplicities.  src_dtype: inputs_float's source.
void Context::elementwise(const TraceTarget& tg, uint32_t kind, const TraceIn& lhs, const TraceIn& rhs, uint64_t n,
                          const lmn_node_info& info, uint32_t* rc_mult, uint64_t rc_ms, int src_dtype) {
  lmn_set_device(device_);
  const bool binary = elementwise_binary(kind), lt = kind == LMN_KIND_LESS_THAN;
  named_rules(tg.call, [&] { check_elementwise(kind, rhs.p, lt && !rc_mult, n, [](ElemRule r) { trace_fail(kTraceElemRules[r]); }); });
  const TraceOperand l{(const int32_t*)lhs.p, named_rules(tg.call, [&] { return trace_view(lhs.view, n); }), lhs.ms};
  // (the table form has always held a unary kind's right view to the view rules as well)
  const TraceOperand r{binary ? (const int32_t*)rhs.p : nullptr,
                       binary || tg.form == TraceTarget::TABLE ? named_rules(tg.call, [&] { return trace_view(rhs.view, n); }) : TraceView{},
                       rhs.ms};
  Placed pl(tg, device_, stream_, kind, n, n, lhs.ms == 0 && (!binary || rhs.ms == 0));
  if (tg.form == TraceTarget::MANY && lt && rc_ms < 256)
    bad_argument(tg.call, "range_check_mult_member_stride is smaller than the table's 256 words");
  launch_trace_elementwise((int)kind, src_dtype, l, r, n, trace_node(info), lt ? rc_mult : nullptr, rc_ms, pl.o, stream_);
  pl.done();
}

// `LuminairContiguous::process_trace` in the reference's own row rule (prim.rs:229-301): max(in_size, out_size) rows
void Context::contiguous(const TraceTarget& tg, const TraceIn& input, uint64_t in_size, uint64_t out_size, const lmn_node_info& info) {
  lmn_set_device(device_);
  TraceNode nd = trace_node(info);
  const TraceOperand in{(const int32_t*)input.p, named_rules(tg.call, [&] { return check_contiguous(in_size, input.view, out_size, nd); }),
                        input.ms};
  const uint64_t n = std::max(in_size, out_size);
  Placed pl(tg, device_, stream_, LMN_KIND_CONTIGUOUS, n, out_size, input.ms == 0);
  launch_trace_elementwise(LMN_KIND_CONTIGUOUS, SRC_FIXED, in, TraceOperand{}, n, nd, nullptr, 0, pl.o, stream_);
  pl.done();
}

// `LuminairSumReduce::process_trace` (prim.rs:1450-1565), or MaxReduce, on a contiguous (front, dim, back) device tensor
void Context::reduce(const TraceTarget& tg, bool is_max, const TraceIn& input, uint64_t front, uint64_t dim, uint64_t back,
                     const lmn_node_info& info) {
  lmn_set_device(device_);
  named_rules(tg.call, [&] { check_reduce_shape(front, dim, back); });
  Placed pl(tg, device_, stream_, is_max ? LMN_KIND_MAX_REDUCE : LMN_KIND_SUM_REDUCE, front * dim * back, front * back, input.ms == 0);
  launch_trace_reduce(is_max, TraceOperand{(const int32_t*)input.p, TraceView{}, input.ms}, front, dim, back, trace_node(info), pl.o,
                      stream_);
  pl.done();
}

// `process_trace` of a Sin / Exp2 / Log2 node on a device tensor; fills the LUT multiplicity column too.  An input outside
// every range is a refused element of a many-member or sink target; the table form fails the call - the one wait here.
void Context::lut(const TraceTarget& tg, uint32_t kind, const TraceIn& input, uint64_t n, const lmn_node_info& info,
                  const uint32_t* lut_col1, const lmn_range* ranges, uint32_t n_ranges, uint32_t* mult, uint64_t mult_ms) {
  lmn_set_device(device_);
  uint64_t lut_rows = 0;
  const LutRanges rg = named_rules(tg.call, [&] {
    return lut_ranges(kind, n, ranges, n_ranges, lut_rows, [](LutRule r) { trace_fail(kTraceLutRules[r]); });
  });
  const TraceOperand in{(const int32_t*)input.p, named_rules(tg.call, [&] { return trace_view(input.view, n); }), input.ms};
  Placed pl(tg, device_, stream_, kind, n, n, input.ms == 0);
  if (tg.form == TraceTarget::MANY && mult_ms < lut_rows)
    bad_argument(tg.call, "mult_member_stride is smaller than the " + std::to_string(lut_rows) + " LUT rows the ranges enumerate");
  const bool table = tg.form == TraceTarget::TABLE;
  if (table) pl.o.err_flag = bad_flag_ + 1;   // zero between calls; the kernel sets it when an input misses every range
  launch_trace_lut(in, n, trace_node(info), lut_col1, rg, mult, mult_ms, pl.o, stream_);
  pl.done();
  if (!table) return;
  uint32_t err = 0;
  lmn_d2h(&err, bad_flag_ + 1, 4, stream_);
  lmn_sync(stream_);
  if (err) {
    const uint32_t zero = 0u;
    lmn_h2d(bad_flag_ + 1, &zero, 4, stream_);
    lmn_sync(stream_);
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "trace_lut: an input value lies outside the LUT's range");
  }
}

// `CopyToStwo` on raw float bits (prim.rs:52-101): the Inputs producer with the float -> Fixed<12> rule (kernels_trace.hip
// float_bits_to_fixed) inside the launch that writes the rows.  The float arguments are checked first, then Inputs' own
// rules apply, with their codes; every form's text carries the entry point's name.
void Context::inputs_float(const TraceTarget& tg, uint32_t dtype, const TraceIn& src, uint64_t n, const lmn_node_info& info) {
  lmn_set_device(device_);
  check_float_ptr(tg.call, dtype, src.p, "src_dev");
  if (n == 0) throw LmnError(LMN_ERR_EMPTY_TRACE, std::string(tg.call) + ": n is 0 (TraceError::EmptyTrace)");
  elementwise(tg, LMN_KIND_INPUTS, src, TraceIn{}, n, info, nullptr, 0, (int)dtype);
}

// ------------------------------------------------------------------------------------ lmn_eval_*
// `Operator::process` of the same operators: the forward pass in front of gen_trace (gen_circuit_settings' dry run,
// crates/graph/src/graph.rs:61-159).  Values only; every call also leaves the range of what it wrote and adds its refused
// elements to a counter, and none waits for the device.  The producers' rules, failing with the argument's name.
namespace {
TraceView eval_view(const char* call, const char* name, const lmn_view* v, uint64_t n) {
  return named_rules(call, [&] { return named_rules(name, [&] { return trace_view(v, n); }); });
}
}  // namespace

void Context::eval_begin(int32_t* minmax) {
  lmn_set_device(device_);
  if (minmax) launch_eval_init(minmax, stream_);
}

void Context::eval_elementwise(uint32_t kind, const int32_t* lhs, const lmn_view* lv, const int32_t* rhs, const lmn_view* rv,
                               uint64_t n, int32_t* out, int32_t* minmax, uint32_t* refused) {
  const char* call = "lmn_eval_elementwise_v";
  check_elementwise(kind, rhs, false, n, [&](ElemRule r) {
    bad_argument(call, r == ELEM_KIND    ? "kind " + std::to_string(kind) + " is not an elementwise kind"
                       : r == ELEM_RHS   ? "null rhs_dev for a binary kind"
                       : r == ELEM_EMPTY ? "n is 0"
                                         : "n: tensor too large");
  });
  const TraceView tlv = eval_view(call, "lhs_view", lv, n);
  const TraceView trv = elementwise_binary(kind) ? eval_view(call, "rhs_view", rv, n) : TraceView{};
  eval_begin(minmax);
  launch_eval_elementwise((int)kind, lhs, tlv, rhs, trv, n, out, minmax, refused, stream_);
}

void Context::eval_reduce(bool is_max, const int32_t* input, uint64_t front, uint64_t dim, uint64_t back, int32_t* out,
                          int32_t* minmax, uint32_t* refused) {
  const char* call = "lmn_eval_reduce";
  if (front == 0) bad_argument(call, "front is 0");
  if (dim == 0) bad_argument(call, "dim is 0");
  if (back == 0) bad_argument(call, "back is 0");
  if (front >= (1ull << 31) || dim >= (1ull << 31) || back >= (1ull << 31) || front * back >= (1ull << 31) ||
      front * back * dim >= (1ull << 31))
    bad_argument(call, "front * dim * back: tensor too large");
  eval_begin(minmax);
  launch_eval_reduce(is_max, input, front, dim, back, out, minmax, refused, stream_);
}

void Context::eval_lut(uint32_t kind, const int32_t* input, const lmn_view* view, uint64_t n, const uint32_t* lut_col1,
                       const lmn_range* ranges, uint32_t n_ranges, int32_t* out, int32_t* minmax, uint32_t* refused) {
  const char* call = "lmn_eval_lut_ranges";
  static const char* const why[] = {"kind must be Sin, Exp2 or Log2", "n is 0", "n: tensor too large", "null ranges",
                                    "n_ranges must be 1..16", "ranges must be ascending, disjoint and inside (-2^30, 2^30)",
                                    "ranges: LUT larger than 2^26 rows"};
  uint64_t lut_rows = 0;
  const LutRanges rg = lut_ranges(kind, n, ranges, n_ranges, lut_rows, [&](LutRule r) { bad_argument(call, why[r]); });
  const TraceView tv = eval_view(call, "view", view, n);
  eval_begin(minmax);
  launch_eval_lut(input, tv, n, lut_col1, rg, out, minmax, refused, stream_);
}

void Context::tensor_range(const int32_t* buf, uint64_t n, int32_t* minmax) {
  if (n == 0) bad_argument("lmn_tensor_range", "n is 0");
  if (n >= (1ull << 31)) bad_argument("lmn_tensor_range", "n: tensor too large");
  eval_begin(minmax);
  launch_tensor_range(buf, n, minmax, stream_);
}

void Context::eval_inputs_float(uint32_t dtype, const void* src, uint64_t n, int32_t* out, int32_t* minmax, uint32_t* refused) {
  const char* call = "lmn_eval_inputs_float";
  check_float_ptr(call, dtype, src, "src_dev");
  if (n == 0) bad_argument(call, "n is 0");
  if (n >= (1ull << 31)) bad_argument(call, "n: tensor too large");
  eval_begin(minmax);
  launch_eval_inputs_float(dtype, src, n, out, minmax, refused, stream_);
}

// `CopyFromStwo`: returns when dst is complete, as download does - a reader on another stream may use it at once
void Context::tensor_to_float(uint32_t dtype, const int32_t* src, uint64_t n, void* dst) {
  const char* call = "lmn_tensor_to_float";
  lmn_set_device(device_);
  check_float_ptr(call, dtype, dst, "dst_dev");
  if (n == 0) bad_argument(call, "n is 0");
  if (n >= (1ull << 31)) bad_argument(call, "n: tensor too large");
  launch_tensor_to_float(dtype, src, n, dst, stream_);
  lmn_sync(stream_);
}

// ------------------------------------------------------------------------------------ lmn_trace_check
// lmn_prove answers a bad trace with ProverError(ConstraintsNotSatisfied) after the FRI loop (phase_oods.cpp) and proves an
// unbalanced one all the same.  This pass names the rows and the tuples instead: one launch per table over the rows where
// they lie (kernels_trace.hip k_trace_check), one per element set to pick the unbalanced tuples out of its table.
namespace {
const char* const kKindNames[17] = {"Add", "Mul", "Recip", "Sin", "SinLookup", "SumReduce", "MaxReduce", "Sqrt", "Rem", "Exp2",
                                    "Exp2Lookup", "Log2", "Log2Lookup", "LessThan", "RangeCheckLookup", "Inputs", "Contiguous"};
const char* const kSetNames[N_ELEMS] = {"NodeElements", "RangeCheck", "Sin", "Exp2", "Log2"};
const char* kind_name(uint32_t kind) { return kind < 17 ? kKindNames[kind] : "?"; }

// device scratch of one call: everything is released when the call returns, whatever its outcome
struct TcScratch {
  std::vector<void*> ptrs;
  lmn_stream_t stream;
  explicit TcScratch(lmn_stream_t s) : stream(s) {}
  ~TcScratch() {
    if (ptrs.empty()) return;
    try {
      lmn_sync(stream);   // a launch of a failed call may still be reading them
    } catch (...) {
    }
    for (void* p : ptrs) lmn_dev_free(p);
  }
  void* get(size_t bytes, const char* what) {
    try {
      void* p = lmn_dev_malloc(bytes);
      ptrs.push_back(p);
      return p;
    } catch (const LmnError&) {
#ifndef LMN_EMU
      (void)hipGetLastError();   // the failed allocation must not surface at the next launch
#endif
      throw LmnError(LMN_ERR_OUT_OF_MEMORY, std::string("trace check: cannot allocate ") + std::to_string(bytes) + " bytes for " + what);
    }
  }
};
}  // namespace

void Context::trace_check(const lmn_table* tables, size_t n_tables, const lmn_settings* settings, lmn_trace_report& rep) {
#ifndef LMN_EMU
  LMN_HIP_CHECK(hipSetDevice(device_));
#endif
  if (!tables || n_tables == 0) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "no trace tables");
  // trace reuse trusts the previous proof's blocks only from one proof straight to the next: any other work of the context in
  // between ends the record (the scratch below is this call's own, not the arena - the rule is kept simple on purpose)
  reuse_.valid = false;
  // ---- lmn_prove's input rules (prove_run.h): the same calls in the same order, so the same rule is named with the
  // same code; the text names the table
  const Refusal refuse{tables};
  std::vector<TableInfo> infos;
  scan_tables(tables, n_tables, cfg, shard_.active, device_, stream_, refuse, infos);
  const Luts luts = luts_for_pie(settings, infos);
  for (size_t t = 0; t < n_tables; ++t) {
    const lmn_lut* l = lut_for_table(t, *infos[t].spec, infos[t].log_size, luts, refuse);
    const uint64_t n = 1ull << infos[t].log_size;
    if (l && (first_noncanonical(l->col0, n) < n || first_noncanonical(l->col1, n) < n))
      refuse(t, LMN_ERR_INVALID_ARGUMENT, "LUT value is not a canonical M31");
  }

  // ---- scratch: the counters, one tuple table per element set the pie uses, device copies of host rows and LUT columns
  TcScratch scratch(stream_);
  uint64_t bound[N_ELEMS] = {0, 0, 0, 0, 0};   // entries a set can get: every relation entry of every real row
  for (size_t t = 0; t < n_tables; ++t)
    for (int j = 0; j < infos[t].spec->n_rel; ++j) bound[infos[t].spec->rel_elems[j]] += tables[t].n_rows;
  // counters: [n_unbalanced, noncanon count, noncanon first, slot_first x n_tables x TC_MAX_SLOTS] u64, then the found
  // tuples, then slot_count u32; behind them the five sets' table descriptors as the kernels read them
  const size_t n_sl = n_tables * TC_MAX_SLOTS;
  const size_t off_found = (3 + n_sl) * 8, off_count = off_found + LMN_TRACE_REPORT_MAX * sizeof(TcFound);
  const size_t ctrl_bytes = (off_count + n_sl * 4 + 7) / 8 * 8, off_sets = ctrl_bytes;
  char* d_ctrl = (char*)scratch.get(ctrl_bytes + N_ELEMS * sizeof(TcSet), "the counters");
  unsigned long long* d_u64 = (unsigned long long*)d_ctrl;
  lmn_memset(d_ctrl, 0, ctrl_bytes, stream_);
  lmn_memset(d_u64 + 2, 0xff, (1 + n_sl) * 8, stream_);
  TcOut out{};
  out.slot_count = (uint32_t*)(d_ctrl + off_count);
  out.slot_first = d_u64 + 3;
  out.noncanon = d_u64 + 1;
  out.sets = (const TcSet*)(d_ctrl + off_sets);
  TcSet sets[N_ELEMS] = {};
  for (int e = 0; e < N_ELEMS; ++e) {
    if (!bound[e]) continue;
    uint64_t cap = 256;
    while (cap < 2 * bound[e]) cap <<= 1;
    unsigned long long* base = (unsigned long long*)scratch.get(cap * 24, "a tuple table");
    sets[e] = {base, base + 2 * cap, base + cap, cap - 1};   // keys | firsts | sums
    lmn_memset(base, 0xff, cap * 16, stream_);
    lmn_memset(base + 2 * cap, 0, cap * 8, stream_);
  }
  lmn_h2d(d_ctrl + off_sets, sets, sizeof sets, stream_);
  const uint32_t* d_lut[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
  for (size_t t = 0; t < n_tables; ++t) {
    const ComponentSpec* sp = infos[t].spec;
    TcTable tb{};
    tb.n_rows = tables[t].n_rows;
    tb.stride = 1ull << infos[t].log_size;
    tb.table = (uint32_t)t;
    if (infos[t].on_device || infos[t].cols_on_device) {
      tb.data = tables[t].rows;
    } else {
      const size_t bytes = (size_t)tb.n_rows * sp->n_cols * 4;
      uint32_t* d = (uint32_t*)scratch.get(bytes, "a copy of host rows");
      lmn_h2d(d, tables[t].rows, bytes, stream_);
      tb.data = d;
    }
    if (sp->n_pre == 2) {
      const int k = sp->pre_id[0] / 2;
      for (int h = 0; h < 2; ++h) {
        uint32_t* d = (uint32_t*)scratch.get((size_t)tb.n_rows * 4, "a LUT column");
        lmn_h2d(d, h ? luts.of[k]->col1 : luts.of[k]->col0, (size_t)tb.n_rows * 4, stream_);
        d_lut[k][h] = d;
      }
      tb.pre0 = d_lut[k][0];
      tb.pre1 = d_lut[k][1];
    }
    tb.n_rel = sp->n_rel;
    tb.slot0 = sp->n_local;
    for (int j = 0; j < sp->n_rel; ++j) {
      tb.rel_mult[j] = sp->rel_mult[j];
      tb.rel_val[j] = sp->rel_val[j];
      tb.rel_id[j] = sp->rel_id[j];
      tb.rel_set[j] = sp->rel_elems[j];
      tb.rel_neg[j] = sp->rel_neg[j];
      tb.rel_pre[j] = sp->rel_pre[j];
    }
    launch_trace_check(sp->kind, infos[t].cols_on_device, tb, out, stream_);
  }
  TcFound* d_found = (TcFound*)(d_ctrl + off_found);
  for (int e = 0; e < N_ELEMS; ++e)
    if (sets[e].keys) launch_trace_check_collect(sets[e], (uint32_t)e, d_u64, d_found, LMN_TRACE_REPORT_MAX, stream_);
  std::vector<char> h_ctrl(ctrl_bytes);
  lmn_d2h(h_ctrl.data(), d_ctrl, ctrl_bytes, stream_);
  lmn_sync(stream_);

  // ---- the report
  const unsigned long long* h_u64 = (const unsigned long long*)h_ctrl.data();
  const uint32_t* h_count = (const uint32_t*)(h_ctrl.data() + off_count);
  rep.n_unbalanced = h_u64[0];
  rep.n_noncanonical = h_u64[1];
  if (rep.n_noncanonical) {
    rep.nc_table = (uint32_t)(h_u64[2] >> 40);
    rep.nc_row = (h_u64[2] >> 8) & 0xffffffffull;
    rep.nc_column = (uint32_t)(h_u64[2] & 0xffu);
  }
  for (size_t t = 0; t < n_tables; ++t)
    for (int sl = 0; sl < infos[t].spec->n_local; ++sl) {
      const uint32_t cnt = h_count[t * TC_MAX_SLOTS + sl];
      if (!cnt) continue;
      if (rep.n_constraints < LMN_TRACE_REPORT_MAX)
        rep.constraints[rep.n_constraints++] = {(uint32_t)t, (uint32_t)infos[t].spec->kind, (uint32_t)sl, 0u, cnt,
                                                h_u64[3 + t * TC_MAX_SLOTS + sl]};
      ++rep.n_constraint_slots;
    }
  rep.constraints_truncated = rep.n_constraint_slots > rep.n_constraints ? 1u : 0u;
  std::vector<TcFound> found((size_t)std::min<uint64_t>(rep.n_unbalanced, LMN_TRACE_REPORT_MAX));
  if (!found.empty()) memcpy(found.data(), h_ctrl.data() + off_found, found.size() * sizeof(TcFound));
  auto val_of = [](const TcFound& f) { return (uint32_t)(f.key & P31); };
  auto id_of = [](const TcFound& f) { return (uint32_t)(f.key >> 31); };
  std::sort(found.begin(), found.end(), [&](const TcFound& a, const TcFound& b) {
    if (a.set != b.set) return a.set < b.set;
    if (id_of(a) != id_of(b)) return id_of(a) < id_of(b);
    return val_of(a) < val_of(b);
  });
  for (const TcFound& f : found)
    rep.tuples[rep.n_tuples++] = {f.set, val_of(f), id_of(f), f.net, (uint32_t)(f.first >> 40), (uint32_t)((f.first >> 32) & 0xffu),
                                  f.first & 0xffffffffull};
  rep.tuples_truncated = rep.n_unbalanced > rep.n_tuples ? 1u : 0u;
  rep.ok = rep.n_noncanonical == 0 && rep.n_constraint_slots == 0 && rep.n_unbalanced == 0 ? 1u : 0u;

  std::string text;
  auto part = [&](const std::string& p) { text += (text.empty() ? "" : "; ") + p; };
  if (rep.ok) {
    uint64_t rows = 0;
    for (size_t t = 0; t < n_tables; ++t) rows += tables[t].n_rows;
    part("ok: " + std::to_string(n_tables) + " tables, " + std::to_string(rows) + " rows, constraints hold and relations balance");
  }
  if (rep.n_noncanonical)
    part(std::to_string(rep.n_noncanonical) + " non-canonical words, first: table " + std::to_string(rep.nc_table) + " (" +
         kind_name(tables[rep.nc_table].kind) + ") row " + std::to_string(rep.nc_row) + " column " + std::to_string(rep.nc_column));
  if (rep.n_constraints) {
    const lmn_trace_constraint& c = rep.constraints[0];
    part("table " + std::to_string(c.table) + " (" + kind_name(c.kind) + ") row " + std::to_string(c.first_row) +
         ": constraint slot " + std::to_string(c.slot) + " non-zero" +
         (rep.n_constraint_slots > 1 ? " (" + std::to_string(rep.n_constraint_slots) + " violated slots in all)" : ""));
  }
  if (rep.n_unbalanced) {
    const lmn_trace_tuple& u = rep.tuples[0];
    const long long net = u.net > P31 / 2 ? (long long)u.net - (long long)P31 : (long long)u.net;
    part(std::to_string(rep.n_unbalanced) + " unbalanced tuples, first: " + kSetNames[u.set] + " id " + std::to_string(u.id) +
         " val " + std::to_string(u.val) + " net " + std::to_string(net));
  }
  snprintf(rep.summary, sizeof rep.summary, "%s", text.c_str());
}

// ------------------------------------------------------------------------------------ row sinks (lmn_rows_*)
// The reference builds its pie on the host, node by node (`table.add_row` in every operator's process_trace,
// crates/graph/src/op/prim.rs:75, 412, 992, 1117; prove takes it at crates/prover/src/prover.rs:28-31,70).  A sink takes
// each node's rows when the node is done and keeps the table column-major in HBM: transfer and transpose run under the
// producer's CPU work instead of in front of the proof.
namespace {
std::mutex g_sinks_mu;
std::map<const uint32_t*, RowSink*> g_sinks;   // finished sinks by the column block they handed out
}  // namespace

RowSink::RowSink(int device, uint32_t kind, uint64_t capacity_rows)
    : device_(device), spec_(component_spec((int)kind)), cap_(capacity_rows) {
  if (!spec_) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "row sink: unsupported component kind " + std::to_string(kind));
  if (spec_->n_cols > CHUNK_MAX_COLS) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "row sink: component has too many columns");
  if (cap_ == 0 || cap_ > (1ull << 26)) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "row sink: capacity must be 1 .. 2^26 rows");
  stride_ = 1ull << padded_log(cap_);
  pad_ = pad_row_of(*spec_);
  lmn_set_device(device_);
  try {
    cols_ = (uint32_t*)lmn_dev_malloc((size_t)spec_->n_cols * stride_ * 4);
    bad_ = (uint32_t*)lmn_dev_malloc(4);
  } catch (const LmnError& e) {
    if (cols_) lmn_dev_free(cols_);
    throw LmnError(LMN_ERR_OUT_OF_MEMORY, std::string("row sink: device allocation failed: ") + e.what());
  }
  h_bad_ = (uint32_t*)lmn_host_alloc_pinned(64);
  stream_ = lmn_stream_create();
  done_ = lmn_event_create_untimed();
  appended_ = lmn_event_create_untimed();
  cleared_ = lmn_event_create_untimed();
  for (auto& e : slot_done_) e = lmn_event_create_untimed();
  lmn_memset(bad_, 0, 4, stream_);
  lmn_event_record(cleared_, stream_);   // a device append's stream waits for it: the memset is in front of the producer
}

RowSink::~RowSink() {
  forget();
  try {
    lmn_set_device(device_);
    join_appends();   // a producer may still be writing the columns
    lmn_sync(stream_);
  } catch (...) {
  }
  lmn_event_destroy(done_);
  lmn_event_destroy(appended_);
  lmn_event_destroy(cleared_);
  for (auto e : slot_done_) lmn_event_destroy(e);
  lmn_stream_destroy(stream_);
  if (ring_) lmn_host_free_pinned(ring_);
  lmn_host_free_pinned(h_bad_);
  lmn_dev_free(bad_);
  lmn_dev_free(cols_);
}

void RowSink::forget() {
  std::lock_guard<std::mutex> lk(g_sinks_mu);
  auto it = g_sinks.find(cols_);
  if (it != g_sinks.end() && it->second == this) g_sinks.erase(it);
}

uint64_t RowSink::count() const {
  std::lock_guard<std::mutex> lk(mu_);
  return count_;
}

void RowSink::push(const uint32_t* host_rows, uint64_t n, bool pinned) {
  std::lock_guard<std::mutex> lk(mu_);
  if (state_ != FILLING)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "row sink: push after finish (lmn_rows_reset starts the next table)");
  if (!host_rows || n == 0) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "row sink: a chunk has at least one row");
  if (n > cap_ - count_) throw LmnError(LMN_ERR_INVALID_ARGUMENT, "row sink: more rows than the capacity it was opened with");
  const uint64_t row_bytes = (uint64_t)spec_->n_cols * 4;
  lmn_set_device(device_);
  if (pinned) {
    const uint32_t* view = (const uint32_t*)lmn_host_device_view(host_rows, n * row_bytes);
    if (!view)
      throw LmnError(LMN_ERR_INVALID_ARGUMENT,
                     "lmn_rows_push_pinned: the rows are not in page-locked memory (lmn_host_alloc / lmn_host_register)");
    launch_rows_chunk(view, count_, n, spec_->n_cols, cols_, stride_, pad_, bad_, stream_);
    count_ += n;
    return;
  }
  if (!ring_) {
    ring_ = (char*)lmn_host_alloc_pinned(SLOTS * SLOT_BYTES);
    ring_dev_ = (const char*)lmn_host_device_view(ring_, SLOTS * SLOT_BYTES);
    if (!ring_dev_) throw LmnError(LMN_ERR_INTERNAL, "row sink: the staging ring has no device address");
  }
  const uint64_t slot_rows = SLOT_BYTES / row_bytes;
  for (uint64_t done = 0; done < n;) {
    const uint64_t m = std::min(slot_rows, n - done);
    const size_t at = (size_t)next_slot_ * SLOT_BYTES;
    lmn_event_wait(slot_done_[next_slot_]);   // waits only when every slot of the ring is still in flight
    memcpy(ring_ + at, host_rows + done * spec_->n_cols, m * row_bytes);
    launch_rows_chunk((const uint32_t*)(ring_dev_ + at), count_, m, spec_->n_cols, cols_, stride_, pad_, bad_, stream_);
    lmn_event_record(slot_done_[next_slot_], stream_);
    next_slot_ = (next_slot_ + 1) % SLOTS;
    count_ += m;
    done += m;
  }
}

void RowSink::join_appends() {
  if (!pending_) return;
  lmn_stream_wait_event(stream_, appended_);
  pending_ = false;
}

RowSink::Append::Append(RowSink& sink, const char* call, int device, lmn_stream_t producer, uint32_t kind, uint64_t n_rows)
    : sink_(sink), lock_(sink.mu_), producer_(producer), n_rows_(n_rows) {
  auto refuse = [&](const std::string& why) { throw LmnError(LMN_ERR_INVALID_ARGUMENT, std::string(call) + ": rows: " + why); };
  if ((uint32_t)sink.spec_->kind != kind)
    refuse("the sink was opened for kind " + std::to_string(sink.spec_->kind) + ", the producer writes kind " + std::to_string(kind));
  if (sink.device_ != device)
    refuse("the sink lives on device " + std::to_string(sink.device_) + ", ctx on device " + std::to_string(device));
  if (sink.state_ != FILLING) refuse("the sink is finished or has failed (lmn_rows_reset starts the next table)");
  if (n_rows > sink.cap_ - sink.count_)
    refuse("the node's " + std::to_string(n_rows) + " rows exceed the " + std::to_string(sink.cap_ - sink.count_) +
           " left of the capacity the sink was opened with");
  // appended_ is one event: appends from another stream than the last one's must not lose that one's record
  if (sink.pending_ && sink.pending_on_ != producer) sink.join_appends();
  lmn_stream_wait_event(producer, sink.cleared_);   // the verdict word is clear before a producer can set it
}

void RowSink::Append::done() {
  lmn_event_record(sink_.appended_, producer_);
  sink_.pending_ = true;
  sink_.pending_on_ = producer_;
  sink_.count_ += n_rows_;
}

void RowSink::sync() {
  std::lock_guard<std::mutex> lk(mu_);
  lmn_set_device(device_);
  join_appends();
  lmn_sync(stream_);
}

void RowSink::finish(lmn_table* table_out) {
  std::lock_guard<std::mutex> lk(mu_);
  if (state_ != FILLING)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT, "row sink: finished already (lmn_rows_reset starts the next table)");
  if (count_ == 0) throw LmnError(LMN_ERR_EMPTY_TRACE, "TraceError::EmptyTrace");
  const uint64_t size = 1ull << padded_log(count_);   // as lmn_prove derives log_size from n_rows
  lmn_set_device(device_);
  join_appends();   // the compaction and the verdict below are behind every producer
  if (size > count_) launch_rows_chunk(nullptr, count_, size - count_, spec_->n_cols, cols_, stride_, pad_, bad_, stream_);
  // a sink opened for more rows than came: columns `size` apart, as the proof's phases index them.  stride_ >= 2 * size,
  // so column c's new place ends before its old one - and every later column's - begins
  if (size < stride_)
    for (int c = 1; c < spec_->n_cols; ++c)
      lmn_d2d(cols_ + (uint64_t)c * size, cols_ + (uint64_t)c * stride_, size * 4, stream_);
  lmn_d2h(h_bad_, bad_, 4, stream_);
  lmn_event_record(done_, stream_);
  lmn_sync(stream_);   // the one wait: every pushed buffer is free, and the verdict is here
  if (*h_bad_) {
    state_ = FAILED;
    throw LmnError(LMN_ERR_INVALID_ARGUMENT,
                   "row sink: a pushed word is not a canonical M31 (>= 2^31-1), or a device producer refused an element "
                   "(lmn_rows_append_*: its row carries that mark)");
  }
  state_ = FINISHED;
  {
    std::lock_guard<std::mutex> g(g_sinks_mu);
    g_sinks[cols_] = this;
  }
  table_out->kind = (uint32_t)spec_->kind;
  table_out->flags = LMN_TABLE_COLS_ON_DEVICE;
  table_out->n_rows = count_;
  table_out->rows = cols_;
}

void RowSink::reset() {
  std::lock_guard<std::mutex> lk(mu_);
  forget();
  lmn_set_device(device_);
  join_appends();                    // a producer of the table given up may still set the verdict word
  lmn_memset(bad_, 0, 4, stream_);   // ordered in front of the next table's chunks
  lmn_event_record(cleared_, stream_);   // ... and, through this, in front of its device appends
  count_ = 0;
  state_ = FILLING;
}

void rows_sink_attach(const lmn_table& tb, int device, lmn_stream_t proof_stream) {
  std::lock_guard<std::mutex> lk(g_sinks_mu);
  auto it = g_sinks.find(tb.rows);
  if (it == g_sinks.end() || (uint32_t)it->second->spec_->kind != tb.kind || it->second->count_ != tb.n_rows ||
      it->second->device_ != device)
    throw LmnError(LMN_ERR_INVALID_ARGUMENT,
                   "LMN_TABLE_COLS_ON_DEVICE: the table is not what lmn_rows_finish of a live sink on this device filled in");
  lmn_stream_wait_event(proof_stream, it->second->done_);
}

}  // namespace lmn
