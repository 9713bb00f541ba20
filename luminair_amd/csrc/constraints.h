// The 17 AIR components, stated once for the host, the kernels and the emulation build: the table of their shapes
// (column layouts, relation wiring, padding rows: crates/air/src/components/**/table.rs, component.rs) and their local
// constraints, generic over the value type - M31 words in k_composition and k_trace_check, QM31 values at the OODS point
// (components.cpp: the prover's self-check and the verifier).  The independent restatement is oracle/air.py.
#pragma once
#include <utility>

#include "../../include/luminair_hip.h"
#include "field.h"

namespace lmn {

constexpr int MAX_REL = 7;
constexpr int N_KINDS = 17;
struct ComponentSpec {
  int kind;
  int n_cols;
  int is_last_col;
  int n_rel;
  int rel_mult[MAX_REL], rel_val[MAX_REL], rel_id[MAX_REL];  // rel_id < 0: width-1 relation (value only)
  int n_local;                // number of local constraints (including zero slots)
  int rel_elems[MAX_REL];     // ELEMS_*: 0 NodeElements, 1 RangeCheckLookup, 2 SinLookup, 3 Exp2Lookup, 4 Log2Lookup
  int rel_neg[MAX_REL];       // numerator is -mult
  int rel_pre[MAX_REL];       // rel_val / rel_id index the component's preprocessed columns
  int n_pre;                  // preprocessed (tree 0) columns read (0..2)
  int pre_id[2];              // PRE_*: position in PreProcessedTrace order (preprocessed.rs:157-179)
  int n_pad;                  // extra non-zero padding cells besides is_last_col = 1
  int pad_col[4];
  uint32_t pad_val[4];
};
enum { ELEMS_NODE = 0, ELEMS_RANGE_CHECK = 1, ELEMS_SIN = 2, ELEMS_EXP2 = 3, ELEMS_LOG2 = 4, N_ELEMS = 5 };
// tree-0 column order before the stable size sort: sin_lut_0/1, exp2_lut_0/1, log2_lut_0/1, range_check_8
enum { PRE_SIN0 = 0, PRE_EXP20 = 2, PRE_LOG20 = 4, PRE_RANGE_CHECK = 6, N_PRE_IDS = 7 };

// kSpecs[kind].  Column layouts / relation wiring: crates/air/src/components/{add,mul,recip,inputs}/{table,component}.rs
inline constexpr ComponentSpec kSpecs[N_KINDS] = {
    // kind, n_cols, is_last, n_rel, rel_mult, rel_val, rel_id, n_local, rel_elems, rel_neg, rel_pre, n_pre, pre_id, n_pad, pad_col, pad_val
    {LMN_KIND_ADD, 15, 4, 3, {12, 13, 14}, {9, 10, 11}, {1, 2, 0}, 6, {0}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},
    {LMN_KIND_MUL, 16, 4, 3, {13, 14, 15}, {9, 10, 11}, {1, 2, 0}, 7, {0}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},
    {LMN_KIND_RECIP, 13, 3, 2, {11, 12}, {7, 8}, {1, 0}, 5, {0}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},
    // sin/component.rs:50-122 (exp2, log2 alike): node relations on input/out + LUT relation (lookup_mult, [input, out])
    {LMN_KIND_SIN, 12, 3, 3, {9, 10, 11}, {7, 8, 7}, {1, 0, 8}, 4, {0, 0, ELEMS_SIN}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},
    // lookups/sin/component.rs:40-59: (-multiplicity, [lut_0, lut_1]) over the two preprocessed columns
    {LMN_KIND_SIN_LOOKUP, 1, -1, 1, {0}, {0}, {1}, 0, {ELEMS_SIN}, {1}, {1}, 2, {PRE_SIN0, PRE_SIN0 + 1}, 0, {0}, {0}},
    // constraint forms fully visible in the reference (no numerair helper):
    {LMN_KIND_SUM_REDUCE, 14, 3, 2, {12, 13}, {7, 8}, {1, 0}, 7, {0}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},   // sum_reduce/component.rs:36-110
    {LMN_KIND_MAX_REDUCE, 15, 3, 2, {13, 14}, {7, 8}, {1, 0}, 9, {0}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},   // max_reduce/component.rs
    // numerair's eval_fixed_sqrt / eval_fixed_rem are un-vendored: natural fixed-point identities (unpinned)
    {LMN_KIND_SQRT, 13, 3, 2, {11, 12}, {7, 8}, {1, 0}, 5, {0}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},
    {LMN_KIND_REM, 16, 4, 3, {13, 14, 15}, {9, 10, 11}, {1, 2, 0}, 6, {0}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},
    {LMN_KIND_EXP2, 12, 3, 3, {9, 10, 11}, {7, 8, 7}, {1, 0, 8}, 4, {0, 0, ELEMS_EXP2}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},
    {LMN_KIND_EXP2_LOOKUP, 1, -1, 1, {0}, {0}, {1}, 0, {ELEMS_EXP2}, {1}, {1}, 2, {PRE_EXP20, PRE_EXP20 + 1}, 0, {0}, {0}},
    {LMN_KIND_LOG2, 12, 3, 3, {9, 10, 11}, {7, 8, 7}, {1, 0, 8}, 4, {0, 0, ELEMS_LOG2}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},
    {LMN_KIND_LOG2_LOOKUP, 1, -1, 1, {0}, {0}, {1}, 0, {ELEMS_LOG2}, {1}, {1}, 2, {PRE_LOG20, PRE_LOG20 + 1}, 0, {0}, {0}},
    // less_than/component.rs:48-185; padding row less_than/table.rs:47-72 (rhs=1, out=4096, diff=1, limb0=1)
    {LMN_KIND_LESS_THAN, 22, 4, 7, {18, 19, 20, 21, 21, 21, 21}, {9, 10, 11, 14, 15, 16, 17}, {1, 2, 0, -1, -1, -1, -1}, 9,
     {0, 0, 0, 1, 1, 1, 1}, {0}, {0}, 0, {0, 0}, 4, {10, 11, 12, 14}, {1u, 4096u, 1u, 1u}},
    // lookups/range_check/component.rs: (-multiplicity, [range_check_8_column_0])
    {LMN_KIND_RANGE_CHECK_LOOKUP, 1, -1, 1, {0}, {0}, {-1}, 0, {ELEMS_RANGE_CHECK}, {1}, {1}, 1, {PRE_RANGE_CHECK, 0}, 0, {0}, {0}},
    {LMN_KIND_INPUTS, 7, 2, 1, {6}, {5}, {0}, 3, {0}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},
    {LMN_KIND_CONTIGUOUS, 11, 3, 2, {9, 10}, {7, 8}, {1, 0}, 4, {0}, {0}, {0}, 0, {0, 0}, 0, {0}, {0}},    // contiguous/component.rs
};
// The columns of a spec that are functions of the graph alone - ids, idx, is_last, their next_* columns, and the
// multiplicities of the relations on main-trace columns - as a bit mask: the candidates of the trace reuse
// (phase_trace.cpp run_main_trace).  Everything else carries values of the input and is never a candidate; components
// without local constraints (the lookups: is_last_col < 0) have none.
constexpr uint32_t graph_only_columns(const ComponentSpec& sp) {
  if (sp.is_last_col < 0) return 0u;
  uint32_t mask = (1u << (2 * sp.is_last_col + 1)) - 1u;
  for (int j = 0; j < sp.n_rel; ++j)
    if (sp.rel_pre[j] == 0) mask |= 1u << sp.rel_mult[j];
  return mask;
}
static_assert(graph_only_columns(kSpecs[LMN_KIND_ADD]) == 0x71ffu && graph_only_columns(kSpecs[LMN_KIND_MUL]) == 0xe1ffu &&
                  graph_only_columns(kSpecs[LMN_KIND_INPUTS]) == 0x5fu && graph_only_columns(kSpecs[LMN_KIND_SIN_LOOKUP]) == 0u,
              "Add: 12 of 15, Mul: 12 of 16, Inputs: 6 of 7");

// k_composition is instantiated once per shape: Exp2 / Log2 run Sin's code, their lookups SinLookup's (the element set
// they differ in is a launch argument)
constexpr int composition_shape(int kind) {
  return kind == LMN_KIND_EXP2 || kind == LMN_KIND_LOG2                 ? LMN_KIND_SIN
         : kind == LMN_KIND_EXP2_LOOKUP || kind == LMN_KIND_LOG2_LOOKUP ? LMN_KIND_SIN_LOOKUP
                                                                        : kind;
}

// the operations the constraint bodies need, on M31 words and on QM31 values
LMN_HD constexpr uint32_t f_add(uint32_t a, uint32_t b) { return m_add(a, b); }
LMN_HD constexpr uint32_t f_sub(uint32_t a, uint32_t b) { return m_sub(a, b); }
LMN_HD constexpr uint32_t f_mul(uint32_t a, uint32_t b) { return m_mul(a, b); }
LMN_HD constexpr uint32_t f_sqr(uint32_t a) { return m_sqr(a); }
LMN_HD constexpr uint32_t f_mul_m(uint32_t a, uint32_t m) { return m_mul(a, m); }
LMN_HD constexpr uint32_t f_sub_m(uint32_t a, uint32_t m) { return m_sub(a, m); }
LMN_HD constexpr uint32_t f_one_minus(uint32_t a) { return m_sub(1u, a); }
LMN_HD QM31 f_add(QM31 a, QM31 b) { return q_add(a, b); }
LMN_HD QM31 f_sub(QM31 a, QM31 b) { return q_sub(a, b); }
LMN_HD QM31 f_mul(QM31 a, QM31 b) { return q_mul(a, b); }
LMN_HD QM31 f_sqr(QM31 a) { return q_sqr(a); }
LMN_HD QM31 f_mul_m(QM31 a, uint32_t m) { return q_mul_m(a, m); }
LMN_HD QM31 f_sub_m(QM31 a, uint32_t m) { return q_sub_m(a, m); }
LMN_HD QM31 f_one_minus(QM31 a) { return q_sub(q_one(), a); }
template <class F>
LMN_HD constexpr F f_bool(F b) { return f_mul(b, f_sub_m(b, 1u)); }

// The local constraints of component KIND on one row c[0 .. n_cols), in `evaluate` order
// (crates/air/src/components/*/component.rs): emit(value) once per "kernel slot" (prover.h ConstraintLayout), n_local
// times.  Every component with local constraints starts its row with N id columns, idx, is_last and their next_* columns,
// opens its list with the boolean on is_last and closes it with the transitions on those columns.
template <int KIND, class F, class Emit>
LMN_HD constexpr void local_constraints(const F* c, Emit&& emit) {
  constexpr int N = kSpecs[KIND].is_last_col - 1;
  if constexpr (N >= 0) {
    emit(f_bool(c[N + 1]));
    if constexpr (KIND == LMN_KIND_ADD) {                // node, lhs_id, rhs_id, idx, is_last, next_*, lhs, rhs, out
      emit(f_sub(c[11], f_add(c[9], c[10])));
    } else if constexpr (KIND == LMN_KIND_MUL) {         // ..., lhs, rhs, out, rem
      emit(f_sub(f_mul(c[9], c[10]), f_add(f_mul_m(c[11], 4096u), c[12])));
      emit(F{});  // second eval_fixed_mul slot: zero on rem == 0 (KAT-pinned form)
    } else if constexpr (KIND == LMN_KIND_REM) {         // ..., lhs, rhs, rem, quotient: lhs = rhs * quotient + rem
      emit(f_sub(c[9], f_add(f_mul(c[10], c[12]), c[11])));   // (unpinned natural identity)
    } else if constexpr (KIND == LMN_KIND_RECIP) {       // node, input_id, idx, is_last, next_*, input, out, rem, scale
      emit(f_sub(f_sqr(c[10]), f_add(f_mul(c[7], c[8]), c[9])));   // (unpinned natural identity)
    } else if constexpr (KIND == LMN_KIND_SQRT) {        // as Recip
      emit(f_sub(f_mul(c[7], c[10]), f_add(f_sqr(c[8]), c[9])));   // (unpinned natural identity)
    } else if constexpr (KIND == LMN_KIND_SUM_REDUCE) {  // ..., input, out, acc, next_acc, is_last_step
      emit(f_bool(c[11]));
      emit(f_sub(c[10], f_add(c[9], c[7])));
      emit(f_mul(f_sub(c[8], c[10]), c[11]));
    } else if constexpr (KIND == LMN_KIND_MAX_REDUCE) {  // ..., input, out, max, next_max, is_last_step, is_max
      emit(f_bool(c[11]));
      emit(f_bool(c[12]));
      emit(f_mul(c[12], f_sub(c[10], c[7])));
      emit(f_mul(f_one_minus(c[12]), f_sub(c[10], c[9])));
      emit(f_mul(f_sub(c[8], c[10]), c[11]));
    } else if constexpr (KIND == LMN_KIND_LESS_THAN) {   // less_than/component.rs:48-185: ..., lhs, rhs, out, diff, borrow, limb0..3
      emit(f_bool(c[13]));
      emit(f_sub(c[11], f_mul_m(f_one_minus(c[13]), 4096u)));
      emit(f_sub(f_add(c[9], c[12]), c[10]));  // - borrow * (2^31 - 1), which is 0 in M31
      emit(f_sub(c[12], f_add(f_add(f_mul_m(c[17], 1u << 24), f_mul_m(c[16], 1u << 16)), f_add(f_mul_m(c[15], 1u << 8), c[14]))));
    }  // Inputs, Contiguous, Sin, Exp2, Log2: the boolean and the transitions only (sin/component.rs:50-122: the function
       // value is enforced by the LUT relation)
    const F not_last = f_one_minus(c[N + 1]);
#pragma unroll
    for (int k = 0; k < N; ++k) emit(f_mul(not_last, f_sub(c[N + 2 + k], c[k])));
    emit(f_mul(not_last, f_sub_m(f_sub(c[2 * N + 2], c[N]), 1u)));
  }
}

template <int KIND>
constexpr int count_local_constraints() {
  const uint32_t row[32] = {};
  int n = 0;
  local_constraints<KIND>(row, [&n](uint32_t) { ++n; });
  return n;
}
template <int... K>
constexpr bool specs_match_constraints(std::integer_sequence<int, K...>) {
  return ((kSpecs[K].kind == K && count_local_constraints<K>() == kSpecs[K].n_local) && ...);
}
static_assert(specs_match_constraints(std::make_integer_sequence<int, N_KINDS>{}),
              "kSpecs: not in kind order, or n_local is not the number of values local_constraints emits");

}  // namespace lmn
