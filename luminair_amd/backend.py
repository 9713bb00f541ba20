"""ctypes binding of the C ABI in include/luminair_hip.h.

The product library is `luminair_amd/csrc/libluminair_hip.so` (hipcc, gfx950).  There is no CPU
fallback: loading fails loudly if the library was not built, and `Context()` fails with
LMN_ERR_NO_DEVICE when no HIP device is present.  (`Library(path)` accepts an explicit path so
the test-suite can load the test-only emulation build; the package itself never does.)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "csrc", "libluminair_hip.so")

LMN_OK = 0
ERR_EMPTY_TRACE, ERR_MAIN_TRACE, ERR_INTERACTION_TRACE, ERR_CONSTRAINTS = -1, -2, -3, -4
ERR_SERIALIZATION, ERR_INVALID_ARGUMENT, ERR_OUT_OF_MEMORY, ERR_NO_DEVICE, ERR_INTERNAL = -5, -6, -7, -8, -100
ERR_VERIFICATION, ERR_INVALID_LOGUP = -9, -10
# lmn_config.protocol_variant: OR of LMN_PV_* bits (include/luminair_hip.h).  All clear = the protocol of the reference's
# known-answer proof; VARIANT_PINNED = what the reference at HEAD is believed to run (transcript bits from memory of the
# un-vendored stwo: unpinned).  tools/pin_variant.py finds the combination a given proof was made with.
PV_CLAIM17, PV_LUT_DRAWS4, PV_MIX_U64_HASHED, PV_DRAW_CTR_U32, PV_POW_PREFIXED = 0x1, 0x2, 0x4, 0x8, 0x10
PV_MUL_ONE_SLOT, PV_RECIP_TWO_SLOTS, PV_RECIP_NEG, PV_SQRT_TWO_SLOTS, PV_SQRT_NEG, PV_REM_TWO_SLOTS, PV_REM_NEG = (
    0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x4000)
PV_TRANSCRIPT_MASK, PV_FORMS_MASK = 0x1f, 0x7f00
PV_NAMES = {PV_CLAIM17: "claim17", PV_LUT_DRAWS4: "lut_draws4", PV_MIX_U64_HASHED: "mix_u64_hashed",
            PV_DRAW_CTR_U32: "draw_ctr_u32", PV_POW_PREFIXED: "pow_prefixed", PV_MUL_ONE_SLOT: "mul_one_slot",
            PV_RECIP_TWO_SLOTS: "recip_two_slots", PV_RECIP_NEG: "recip_neg", PV_SQRT_TWO_SLOTS: "sqrt_two_slots",
            PV_SQRT_NEG: "sqrt_neg", PV_REM_TWO_SLOTS: "rem_two_slots", PV_REM_NEG: "rem_neg"}
VARIANT_KAT, VARIANT_PINNED = 0, PV_TRANSCRIPT_MASK
CHECK_PARSE, CHECK_SHAPE, CHECK_LOGUP_SUM, CHECK_OODS, CHECK_POW, CHECK_TREE_DECOMMIT, CHECK_FRI_DECOMMIT, CHECK_FRI_FOLDS = (
    1, 2, 4, 8, 16, 32, 64, 128)
CHECK_ALL = 0xff
CHECK_NAMES = {CHECK_PARSE: "parse", CHECK_SHAPE: "shape", CHECK_LOGUP_SUM: "logup_sum", CHECK_OODS: "oods",
               CHECK_POW: "pow", CHECK_TREE_DECOMMIT: "tree_decommit", CHECK_FRI_DECOMMIT: "fri_decommit",
               CHECK_FRI_FOLDS: "fri_folds"}
STEP_NAMES = ["root_preprocessed", "claim", "root_main", "interaction_claim", "root_interaction", "root_composition",
              "sampled_values", "fri_first_layer", "fri_inner_layer", "fri_last_layer", "pow_nonce"]
ROUND_HALF_AWAY, ROUND_HALF_EVEN, ROUND_TRUNC, ROUND_FLOOR = 0, 1, 2, 3
MAX_TRANSCRIPT_STEPS = 48
TABLE_ROWS_ON_DEVICE = 1
TABLE_COLS_ON_DEVICE = 2


class LmnConfig(C.Structure):
    _fields_ = [("pow_bits", C.c_uint32), ("log_blowup", C.c_uint32), ("log_last_layer", C.c_uint32),
                ("n_queries", C.c_uint32), ("fp_scale", C.c_uint32), ("protocol_variant", C.c_uint32)]


class LmnTable(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("n_rows", C.c_uint64), ("rows", C.c_void_p)]


class LmnLut(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("log_size", C.c_uint32), ("col0", C.c_void_p), ("col1", C.c_void_p)]


class LmnSettings(C.Structure):
    _fields_ = [("has_lookups", C.c_uint32), ("n_luts", C.c_uint32), ("luts", C.POINTER(LmnLut))]


LUT_KINDS = {"sin": 0, "exp2": 1, "log2": 2}   # LMN_LUT_*
LOOKUP_SIN, LOOKUP_EXP2, LOOKUP_LOG2, LOOKUP_RANGE_CHECK = 1, 2, 4, 8   # LMN_LOOKUP_*
LOOKUP_BITS = {"sin": LOOKUP_SIN, "exp2": LOOKUP_EXP2, "log2": LOOKUP_LOG2, "range_check": LOOKUP_RANGE_CHECK}


class LmnView(C.Structure):
    """Strided view of a device tensor (`lmn_view`): shape of the op's output, strides in elements, 0 = expanded."""
    _fields_ = [("ndim", C.c_uint32), ("shape", C.c_uint32 * 4), ("strides", C.c_int64 * 4), ("offset", C.c_int64)]

    @staticmethod
    def make(shape, strides, offset: int = 0) -> "LmnView":
        n = len(shape)
        if not 1 <= n <= 4:
            raise ValueError("views have 1..4 dimensions")
        return LmnView(n, (C.c_uint32 * 4)(*(list(shape) + [0] * (4 - n))),
                       (C.c_int64 * 4)(*(list(strides) + [0] * (4 - n))), int(offset))


class LmnNodeInfo(C.Structure):
    """`NodeInfo` fields `process_trace` reads (crates/graph/src/utils.rs / op/prim.rs:980-990)."""
    _fields_ = [("node_id", C.c_uint32), ("input_ids", C.c_uint32 * 2), ("num_consumers", C.c_uint32),
                ("is_final_output", C.c_uint32), ("input_mults", C.c_int32 * 2)]


class LmnRange(C.Structure):
    """`Range(Fixed, Fixed)`: inclusive range of Fixed<12> values (i64)."""
    _fields_ = [("lo", C.c_int64), ("hi", C.c_int64)]


# ---- what every producer wrapper marshals (Context.trace_* / trace_many_* / eval_*)
def _node_info(node_id: int, input_ids=(), num_consumers: int = 0, is_final_output: bool = False, input_mults=()) -> LmnNodeInfo:
    """ids and mults padded to two"""
    ids = list(input_ids) + [0] * (2 - len(input_ids))
    mults = list(input_mults) + [0] * (2 - len(input_mults))
    return LmnNodeInfo(node_id, (C.c_uint32 * 2)(*ids), num_consumers, 1 if is_final_output else 0, (C.c_int32 * 2)(*mults))


def _addr(b):
    """a DeviceBuffer's address, a device address as it is (an int: memory of another owner), None"""
    return b.ptr if isinstance(b, DeviceBuffer) else b


def _ref(v):
    """an optional struct argument"""
    return C.byref(v) if v is not None else None


def _range_array(ranges):
    return (LmnRange * max(len(ranges), 1))(*[LmnRange(int(a), int(b)) for a, b in ranges])


ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


ALL_TO_ALL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p,
                            C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_void_p)


class LmnCollective(C.Structure):
    """`lmn_collective`: the exchange primitives of a sharded proof - an in-place all-gather on device memory and
    (optional) the all-to-all that re-partitions column-parallel LDEs into row blocks."""
    _fields_ = [("user", C.c_void_p), ("all_gather", ALL_GATHER_FN), ("group_begin", C.c_void_p), ("group_end", C.c_void_p),
                ("all_to_all", ALL_TO_ALL_FN)]


RCCL_ID_BYTES = 128


class LmnTimings(C.Structure):
    _fields_ = [("total_ms", C.c_float)] + [(n, C.c_float) for n in (
        "transpose_ms", "main_commit_ms", "logup_ms", "interaction_commit_ms", "composition_ms",
        "composition_commit_ms", "oods_ms", "quotients_ms", "fri_ms", "decommit_ms", "fft_ms", "merkle_ms")] + [
        ("fft_bytes", C.c_uint64), ("merkle_bytes", C.c_uint64), ("fft_launches", C.c_uint32),
        ("merkle_launches", C.c_uint32), ("fft_butterflies", C.c_uint64), ("merkle_compressions", C.c_uint64),
        ("merkle_fused_ms", C.c_float), ("merkle_fused_launches", C.c_uint32), ("merkle_fused_bytes", C.c_uint64),
        ("merkle_fused_compressions", C.c_uint64), ("shard_a2a_bytes", C.c_uint64), ("shard_gather_bytes", C.c_uint64),
        ("shard_a2a_calls", C.c_uint32), ("shard_gather_calls", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class LmnTranscriptStep(C.Structure):
    _fields_ = [("step", C.c_uint32), ("index", C.c_uint32), ("digest", C.c_uint8 * 32)]


class LmnVerifyReport(C.Structure):
    """`lmn_verify_report`: which checks of the verifier a proof passes under one set of protocol flags, and the
    channel digest after every mix of the replay."""
    _fields_ = [("checks_run", C.c_uint32), ("checks_passed", C.c_uint32), ("checks_failed", C.c_uint32),
                ("n_steps", C.c_uint32), ("steps", LmnTranscriptStep * MAX_TRANSCRIPT_STEPS),
                ("first_failure", C.c_char * 128)]


# form codes of lmn_col_fri_commit (LMN_FRI_*)
FRI_FOLD_LAUNCH, FRI_FOLD_IN_LEAVES, FRI_FOLD_IN_LEAVES_JOIN, FRI_FOLD_MATERIALISED, FRI_FOLD_TAIL_FRONT, FRI_FOLD_IN_TAIL = 1, 2, 3, 4, 5, 6
FRI_FOLD_MASK, FRI_TREE_OWN, FRI_TREE_IN_TAIL = 0xff, 0x100, 0x200
FRI_FIRST_TREE, FRI_FIRST_TREE_BELOW = 0x10000, 0x10001


class LmnFriCommitResult(C.Structure):
    """`lmn_fri_commit_result`"""
    _fields_ = [("n_trees", C.c_uint32), ("reserved", C.c_uint32), ("roots", C.c_void_p), ("alphas", C.c_void_p),
                ("tree_logs", C.c_void_p), ("level_masks", C.c_void_p), ("forms", C.c_void_p), ("values", C.c_void_p),
                ("levels", C.c_void_p), ("n_value_words", C.c_uint64), ("n_level_words", C.c_uint64)]


@dataclass
class FriCommit:
    """What `Context.fri_commit` returns.  Trees t = 0 .. n-1 (the first tree, then one per inner layer); layers i = 0 .. n-1
    (inner layer i is committed by tree i + 1, the last one is the last layer)."""
    roots: List[bytes]
    alphas: List[Tuple[int, int, int, int]]
    tree_logs: List[int]
    tree_levels: List[List[Optional[np.ndarray]]]   # [tree][level] -> (2^level, 8) uint32, None: not written to device memory
    first_tree_form: int
    layer_logs: List[int]
    layer_values: List[np.ndarray]                  # (4, 2^log) uint32
    layer_forms: List[int]                          # FRI_FOLD_* | FRI_TREE_*


TRACE_REPORT_MAX = 64   # LMN_TRACE_REPORT_MAX
ELEM_SET_NAMES = ["NodeElements", "RangeCheck", "Sin", "Exp2", "Log2"]


class LmnTraceConstraint(C.Structure):
    _fields_ = [("table", C.c_uint32), ("kind", C.c_uint32), ("slot", C.c_uint32), ("reserved", C.c_uint32),
                ("count", C.c_uint64), ("first_row", C.c_uint64)]


class LmnTraceTuple(C.Structure):
    _fields_ = [("set", C.c_uint32), ("val", C.c_uint32), ("id", C.c_uint32), ("net", C.c_uint32),
                ("first_table", C.c_uint32), ("first_slot", C.c_uint32), ("first_row", C.c_uint64)]


class LmnTraceReport(C.Structure):
    """`lmn_trace_report`: what lmn_trace_check found in a trace."""
    _fields_ = [("ok", C.c_uint32), ("n_constraints", C.c_uint32), ("n_constraint_slots", C.c_uint32),
                ("constraints_truncated", C.c_uint32), ("n_tuples", C.c_uint32), ("tuples_truncated", C.c_uint32),
                ("n_unbalanced", C.c_uint64), ("n_noncanonical", C.c_uint64), ("nc_table", C.c_uint32),
                ("nc_column", C.c_uint32), ("nc_row", C.c_uint64), ("constraints", LmnTraceConstraint * TRACE_REPORT_MAX),
                ("tuples", LmnTraceTuple * TRACE_REPORT_MAX), ("summary", C.c_char * 256)]


@dataclass
class TraceReport:
    """`Context.check_trace`'s answer.  constraints: [(table, kind, slot, count, first_row)] sorted by (table, slot) -
    local kernel slots on which real rows are non-zero; tuples: [(set, val, id, net, first_table, first_slot, first_row)]
    sorted by (set, id, val) - logup tuples whose net multiplicity (an M31 word) is not zero, with the smallest
    (table, slot, row) that mentions each; first_noncanonical: (table, row, column) or None."""
    ok: bool
    summary: str
    n_noncanonical: int
    first_noncanonical: Optional[Tuple[int, int, int]]
    n_constraint_slots: int
    constraints: List[Tuple[int, int, int, int, int]]
    constraints_truncated: bool
    n_unbalanced: int
    tuples: List[Tuple[int, int, int, int, int, int, int]]
    tuples_truncated: bool

    @staticmethod
    def from_c(r: "LmnTraceReport") -> "TraceReport":
        cons = [(int(c.table), int(c.kind), int(c.slot), int(c.count), int(c.first_row))
                for c in r.constraints[:r.n_constraints]]
        tup = [(int(t.set), int(t.val), int(t.id), int(t.net), int(t.first_table), int(t.first_slot), int(t.first_row))
               for t in r.tuples[:r.n_tuples]]
        nc = (int(r.nc_table), int(r.nc_row), int(r.nc_column)) if r.n_noncanonical else None
        return TraceReport(bool(r.ok), r.summary.decode(), int(r.n_noncanonical), nc, int(r.n_constraint_slots), cons,
                           bool(r.constraints_truncated), int(r.n_unbalanced), tup, bool(r.tuples_truncated))


class LmnFriCloseResult(C.Structure):
    """`lmn_fri_close_result`"""
    _fields_ = [("n_coeffs", C.c_uint32), ("first_bad", C.c_uint32), ("n_positions", C.c_uint32), ("grind_rounds", C.c_uint32),
                ("nonce", C.c_uint64), ("coeffs", C.c_void_p), ("positions", C.c_void_p),
                ("digest_after_coeffs", C.c_uint8 * 32), ("digest_after_nonce", C.c_uint8 * 32), ("digest_end", C.c_uint8 * 32),
                ("n_sent_end", C.c_uint32), ("reserved", C.c_uint32)]


@dataclass
class FriClose:
    """What `Context.fri_close` returns: the last layer's coefficients, the degree check, the nonce, the query positions and
    the channel after each step."""
    coeffs: List[Tuple[int, int, int, int]]   # the first 2^log_last_layer
    first_bad: Optional[int]                  # lowest index past them of a non-zero coefficient, None: degree ok
    nonce: int
    grind_rounds: int                         # host waits spent grinding after the chain's own wait
    positions: List[int]                      # ascending, distinct
    digest_after_coeffs: bytes
    digest_after_nonce: bytes
    digest_end: bytes
    n_sent_end: int


class LmnOpenItem(C.Structure):
    """`lmn_open_item`"""
    _fields_ = [("tree", C.c_void_p), ("cols", C.POINTER(C.c_void_p)), ("n_cols", C.c_uint32), ("flags", C.c_uint32)]


class LmnOpening(C.Structure):
    """`lmn_opening`"""
    _fields_ = [("queried_values", C.c_void_p), ("hash_witness", C.c_void_p), ("column_witness", C.c_void_p),
                ("fri_witness", C.c_void_p), ("n_values", C.c_uint64), ("n_hashes", C.c_uint64),
                ("n_column_words", C.c_uint64), ("n_fri_words", C.c_uint64)]


OPEN_FRI_PAIRS = 1          # LMN_OPEN_FRI_PAIRS
OPEN_MAX_POSITIONS = 1024
OPEN_MAX_ITEMS = 64


class LmnVerifyResult(C.Structure):
    """`lmn_verify_result`"""
    _fields_ = [("rc", C.c_int32), ("checks_failed", C.c_uint32), ("stage", C.c_uint32)]


@dataclass
class VerifyResult:
    """One proof of `Library.verify_many`: `code` is what `lmn_verify_with_config` returns for the proof, `checks_failed`
    the LMN_CHECK_* bits, `stage` 0 (decided by the host front), 1 (by the device stage) or 2 (by the host verifier)."""
    ok: bool
    code: int
    checks_failed: int
    stage: int


@dataclass
class Opening:
    """One item of `Context.open_queries`: the three outputs of `Tree.decommit`, and - under OPEN_FRI_PAIRS - the FRI
    witness, one (a, b, c, d) per pair member that is no position itself."""
    queried_values: np.ndarray
    hash_witness: List[bytes]
    column_witness: np.ndarray
    fri_witness: List[Tuple[int, int, int, int]]


# lmn_ctx_counter
COUNTER_GRINDS, COUNTER_GRIND_WAITS, COUNTER_DEVICE_CLOSES, COUNTER_DEVICE_CLOSE_FALLBACKS = 7, 8, 9, 10
COUNTER_DEVICE_OPENINGS, COUNTER_DEVICE_OPENING_FALLBACKS = 11, 12
# diagnostic only (the tests' evidence of one plan launch, one fetch launch and one wait per lmn_open_queries call)
COUNTER_OPEN_PLAN_LAUNCHES, COUNTER_OPEN_FETCH_LAUNCHES, COUNTER_OPEN_WAITS = 13, 14, 15
# lmn_verify_many: proofs judged by the device stage, stage-2 proofs, verify launches, host waits
COUNTER_VERIFY_DEVICE, COUNTER_VERIFY_STAGE2, COUNTER_VERIFY_LAUNCHES, COUNTER_VERIFY_WAITS = 16, 17, 18, 19
# diagnostic only: proofs whose quotient tables k_quot_prepare made; unsharded device-transcript proofs that kept the host's wait
COUNTER_QUOT_DEVICE, COUNTER_QUOT_HOST_WAIT = 22, 23

API_VERSION = 6   # LMN_API_VERSION of include/luminair_hip.h

EXPORTS = ["lmn_abi_version", "lmn_kind_padding_row", "lmn_strerror", "lmn_last_error", "lmn_default_config", "lmn_kind_columns", "lmn_ctx_create",
           "lmn_ctx_destroy", "lmn_prove", "lmn_prove_submit", "lmn_prove_wait", "lmn_free", "lmn_get_timings", "lmn_set_profiling", "lmn_upload", "lmn_device_free", "lmn_verify",
           "lmn_host_alloc", "lmn_host_free", "lmn_host_register", "lmn_host_unregister",
           "lmn_op_interpolate", "lmn_op_evaluate", "lmn_op_merkle_root", "lmn_op_eval_at_point",
           "lmn_op_fft_selftest", "lmn_op_accumulate_quotients", "lmn_op_fold_line", "lmn_op_fold_circle_into_line",
           "lmn_op_grind", "lmn_ctx_grind", "lmn_ctx_grind_many", "lmn_device_alloc", "lmn_download", "lmn_trace_elementwise", "lmn_trace_sum_reduce",
           "lmn_trace_elementwise_v", "lmn_trace_contiguous", "lmn_trace_lut", "lmn_trace_lut_ranges", "lmn_trace_less_than", "lmn_trace_max_reduce", "lmn_upload_to", "lmn_device_copy", "lmn_op_evaluate_block",
           "lmn_verify_with_config", "lmn_verify_diagnose", "lmn_kind_constraint_layout", "lmn_lut_log_size", "lmn_lut_from_ranges", "lmn_lut_from_ranges_r", "lmn_col_alloc", "lmn_col_from_cpu", "lmn_col_to_cpu", "lmn_col_free", "lmn_col_ncols",
           "lmn_col_log_size", "lmn_col_device_ptr", "lmn_col_view", "lmn_col_bit_reverse", "lmn_col_precompute_twiddles",
           "lmn_col_interpolate", "lmn_col_evaluate", "lmn_col_evaluate_block", "lmn_col_extend", "lmn_col_eval_at_point",
           "lmn_col_commit", "lmn_tree_root", "lmn_tree_log_size", "lmn_tree_layer_to_cpu", "lmn_tree_free",
           "lmn_tree_decommit", "lmn_col_gather", "lmn_col_fri_commit", "lmn_col_fri_close", "lmn_ctx_counter",
           "lmn_col_accumulate", "lmn_col_accumulate_quotients", "lmn_col_fold_line", "lmn_col_fold_circle_into_line",
           "lmn_col_decompose", "lmn_col_batch_inverse", "lmn_col_batch_inverse_secure", "lmn_col_logup", "lmn_col_composition", "lmn_kind_constraints", "lmn_kind_relations", "lmn_ctx_set_shard", "lmn_rccl_unique_id", "lmn_ctx_set_shard_rccl", "lmn_ctx_clear_shard",
           "lmn_rows_open", "lmn_rows_push", "lmn_rows_push_pinned", "lmn_rows_sync", "lmn_rows_finish", "lmn_rows_count",
           "lmn_rows_reset", "lmn_rows_close", "lmn_trace_check",
           "lmn_rows_append_elementwise_v", "lmn_rows_append_contiguous", "lmn_rows_append_reduce", "lmn_rows_append_lut_ranges",
           "lmn_eval_elementwise_v", "lmn_eval_reduce", "lmn_eval_reduce_split", "lmn_eval_lut_ranges", "lmn_tensor_range",
           "lmn_trace_many_elementwise_v", "lmn_trace_many_contiguous", "lmn_trace_many_reduce", "lmn_trace_many_lut_ranges",
           "lmn_settings_prepare", "lmn_prepared_root", "lmn_prepared_lookups", "lmn_prepared_destroy", "lmn_prove_prepared",
           "lmn_prove_submit_prepared", "lmn_batch_prove_prepared",
           "lmn_positions_from_cpu", "lmn_positions_to_cpu", "lmn_positions_log_domain", "lmn_positions_free",
           "lmn_col_fri_close_keep", "lmn_open_queries", "lmn_verify_many",
           "lmn_trace_inputs_float", "lmn_trace_many_inputs_float", "lmn_rows_append_inputs_float", "lmn_eval_inputs_float",
           "lmn_tensor_to_float"]
TRACE_MANY_MAX = 1024   # LMN_TRACE_MANY_MAX
F32, F16, BF16 = 0, 1, 2   # LMN_F32 / LMN_F16 / LMN_BF16: the dtype of a float source or destination
FLOAT_BYTES = {F32: 4, F16: 2, BF16: 2}
FIXED_MAX = (1 << 30) - 1   # the producers' value range (include/luminair_hip.h, lmn_trace_elementwise)


def float_dtype_code(dtype) -> int:
    """LMN_F32 / LMN_F16 / LMN_BF16 for a numpy or torch float dtype, the string "bfloat16" (numpy has no bf16), or the code
    itself."""
    if isinstance(dtype, int) and not isinstance(dtype, bool) and dtype in FLOAT_BYTES:
        return dtype
    name = str(dtype).replace("torch.", "")
    if name in ("bfloat16", "bf16"):
        return BF16
    try:
        name = np.dtype(dtype).name
    except TypeError:
        pass
    if name == "float32":
        return F32
    if name == "float16":
        return F16
    raise ValueError("float tensors are float32, float16 or bfloat16, not %r" % (dtype,))


def _float_bits(x, code: Optional[int] = None):
    """(raw IEEE bits as int64, exponent bits, mantissa bits) of a float32 / float16 array; code=BF16: `x` holds bf16 bit
    patterns (uint16) already."""
    if code == BF16:
        return np.ascontiguousarray(x).view(np.uint16).astype(np.int64), 8, 7
    x = np.ascontiguousarray(x)
    if x.dtype == np.float32:
        return x.view(np.uint32).astype(np.int64), 8, 23
    if x.dtype == np.float16:
        return x.view(np.uint16).astype(np.int64), 5, 10
    raise ValueError("to_fixed takes float32 or float16 arrays (bfloat16 as uint16 bit patterns with dtype=BF16), not %s" % x.dtype)


def to_fixed(x, dtype: Optional[int] = None, refused: Optional[list] = None) -> np.ndarray:
    """Float -> Fixed<12>, the host mirror of the device rule (`CopyToStwo`: `Fixed::from_f64(d as f64)`, taken as
    round-to-nearest, ties away from zero - numerair is un-vendored, its rounding unpinned): the exact value x 4096 rounded
    to the nearest integer, computed from the bit pattern in integers.  +-0 and denormals give 0.  `x`: a float32 or
    float16 array, or uint16 bf16 bit patterns with dtype=BF16.  Raises ValueError for what the device refuses - NaN, +-Inf, a
    result outside [-(2^30-1), 2^30-1] - unless `refused` is a list: then the refused elements' flat indices are appended
    to it and those elements are 0, as in a device tensor.  Returns int32 of x's shape."""
    bits, eb, mb = _float_bits(x, dtype)
    shape = np.shape(x)
    bits = bits.reshape(-1)
    bias = (1 << (eb - 1)) - 1
    e = (bits >> mb) & ((1 << eb) - 1)
    sig = (bits & ((1 << mb) - 1)) | (1 << mb)
    sh = e - bias - mb + 12                                   # value * 4096 = sig * 2^sh
    up = sig << np.clip(sh, 0, 31)
    r = np.clip(-sh, 1, mb + 3)
    down = np.where(-sh > mb + 2, 0, (sig + (np.int64(1) << (r - 1))) >> r)
    mag = np.where(sh >= 0, up, down)
    bad = (e == (1 << eb) - 1) | (mag > FIXED_MAX)
    mag = np.where((e == 0) | bad, 0, mag)
    out = np.where((bits >> (eb + mb)) & 1 == 1, -mag, mag).astype(np.int32)
    if bad.any():
        if refused is None:
            raise ValueError("to_fixed: %d elements are NaN, infinite or outside [-(2^30-1), 2^30-1] after scaling "
                             "(first at flat index %d)" % (int(bad.sum()), int(np.flatnonzero(bad)[0])))
        refused.extend(int(i) for i in np.flatnonzero(bad))
    return out.reshape(shape)


def from_fixed(v, dtype=np.float32) -> np.ndarray:
    """Fixed<12> -> float, the host mirror of `lmn_tensor_to_float` (`CopyFromStwo`: `d.to_f64() as f32`): the exact value
    v / 4096 rounded once to the format, round-to-nearest-even, in integers.  dtype: np.float32, np.float16, or BF16 /
    "bfloat16" - then the result is the uint16 bf16 bit patterns (numpy has no bfloat16)."""
    code = float_dtype_code(dtype)
    eb, mb = {F32: (8, 23), F16: (5, 10), BF16: (8, 7)}[code]
    v = np.asarray(v).astype(np.int64)
    shape = v.shape
    v = v.reshape(-1)
    bias = (1 << (eb - 1)) - 1
    mag = np.abs(v)
    p = np.zeros_like(mag)                                    # the leading bit of mag
    for k in (16, 8, 4, 2, 1):
        big = (mag >> (p + k)) != 0
        p = np.where(big, p + k, p)
    r = np.clip(p - mb, 1, 32)
    rem, half, q_dn = mag & ((np.int64(1) << r) - 1), np.int64(1) << (r - 1), mag >> r
    q_dn = q_dn + ((rem > half) | ((rem == half) & (q_dn & 1 == 1)))
    q = np.where(p <= mb, mag << np.clip(mb - p, 0, 32), q_dn)
    bits = ((p - 12 + bias - 1) << mb) + q
    inf = ((1 << eb) - 1) << mb
    bits = np.where(bits >= inf, inf, bits)
    bits = np.where(mag == 0, 0, bits | np.where(v < 0, 1 << (eb + mb), 0))
    if code == F32:
        return bits.astype(np.uint32).view(np.float32).reshape(shape)
    out = bits.astype(np.uint16)
    return (out.view(np.float16) if code == F16 else out).reshape(shape)


class LuminairBackendError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__("%s (code %d)" % (message, code))
        self.code = code


class Library:
    def __init__(self, path: Optional[str] = None):
        path = path or DEFAULT_LIB
        if not os.path.exists(path):
            raise LuminairBackendError(ERR_NO_DEVICE, "HIP backend library not built: %s (run __graft_entry__.build())"
                                       % path)
        self.path = path
        lib = C.CDLL(path)
        self.lib = lib
        # the ctypes structures below mirror include/luminair_hip.h at this ABI version; a library built from another
        # header (e.g. a 56-byte lmn_view without `offset`) must be refused, not fed garbage
        try:
            lib.lmn_abi_version.restype = C.c_uint32
            got = int(lib.lmn_abi_version())
        except AttributeError:
            got = None
        if got != API_VERSION:
            raise LuminairBackendError(ERR_INVALID_ARGUMENT, "%s implements ABI version %s, this package binds version %d"
                                       % (path, got, API_VERSION))
        lib.lmn_strerror.restype = C.c_char_p
        lib.lmn_strerror.argtypes = [C.c_int]
        lib.lmn_last_error.restype = C.c_char_p
        lib.lmn_last_error.argtypes = [C.c_void_p]
        lib.lmn_default_config.argtypes = [C.POINTER(LmnConfig)]
        lib.lmn_kind_columns.restype = C.c_uint32
        lib.lmn_kind_columns.argtypes = [C.c_uint32]
        lib.lmn_kind_relations.restype = C.c_uint32
        lib.lmn_kind_relations.argtypes = [C.c_uint32]
        lib.lmn_kind_padding_row.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
        lib.lmn_ctx_create.argtypes = [C.c_int, C.POINTER(LmnConfig), C.POINTER(C.c_void_p)]
        lib.lmn_ctx_destroy.argtypes = [C.c_void_p]
        lib.lmn_prove.argtypes = [C.c_void_p, C.POINTER(LmnTable), C.c_size_t, C.POINTER(LmnSettings),
                                  C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
        lib.lmn_prove_submit.argtypes = [C.c_void_p, C.POINTER(LmnTable), C.c_size_t, C.POINTER(LmnSettings)]
        lib.lmn_prove_wait.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
        lib.lmn_settings_prepare.argtypes = [C.c_int, C.POINTER(LmnConfig), C.POINTER(LmnSettings), C.c_uint32,
                                             C.POINTER(C.c_void_p)]
        lib.lmn_prepared_root.argtypes = [C.c_void_p, C.c_void_p]
        lib.lmn_prepared_lookups.argtypes = [C.c_void_p]
        lib.lmn_prepared_lookups.restype = C.c_uint32
        lib.lmn_prepared_destroy.argtypes = [C.c_void_p]
        lib.lmn_prepared_destroy.restype = None
        lib.lmn_prove_prepared.argtypes = [C.c_void_p, C.POINTER(LmnTable), C.c_size_t, C.c_void_p,
                                           C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
        lib.lmn_prove_submit_prepared.argtypes = [C.c_void_p, C.POINTER(LmnTable), C.c_size_t, C.c_void_p]
        lib.lmn_batch_prove_prepared.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(LmnTable)), C.c_size_t, C.c_void_p,
                                                 C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        lib.lmn_free.argtypes = [C.c_void_p]
        lib.lmn_get_timings.argtypes = [C.c_void_p, C.POINTER(LmnTimings)]
        lib.lmn_set_profiling.argtypes = [C.c_void_p, C.c_int]
        lib.lmn_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        lib.lmn_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        lib.lmn_host_free.argtypes = [C.c_void_p]
        lib.lmn_host_register.argtypes = [C.c_void_p, C.c_size_t]
        lib.lmn_host_unregister.argtypes = [C.c_void_p]
        lib.lmn_device_free.argtypes = [C.c_void_p, C.c_void_p]
        lib.lmn_verify.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(LmnSettings), C.c_uint32]
        lib.lmn_verify_with_config.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(LmnSettings), C.POINTER(LmnConfig)]
        lib.lmn_op_interpolate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        lib.lmn_op_evaluate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.lmn_op_evaluate_block.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_uint32, C.c_void_p]
        lib.lmn_op_merkle_root.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_uint32,
                                           C.c_void_p]
        lib.lmn_op_eval_at_point.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.lmn_op_fft_selftest.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        lib.lmn_op_accumulate_quotients.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                    C.c_void_p, C.c_void_p]
        lib.lmn_op_fold_line.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.lmn_op_fold_circle_into_line.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.lmn_op_grind.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        lib.lmn_ctx_grind.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        lib.lmn_ctx_grind_many.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.POINTER(C.c_uint64)]
        lib.lmn_device_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        lib.lmn_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.lmn_upload_to.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.lmn_device_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.lmn_lut_log_size.argtypes = [C.POINTER(LmnRange), C.c_uint32, C.POINTER(C.c_uint32)]
        lib.lmn_lut_from_ranges.argtypes = [C.c_uint32, C.POINTER(LmnRange), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.lmn_lut_from_ranges_r.argtypes = [C.c_uint32, C.POINTER(LmnRange), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                              C.c_void_p]
        lib.lmn_verify_diagnose.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(LmnSettings), C.POINTER(LmnConfig),
                                            C.POINTER(LmnVerifyReport)]
        lib.lmn_kind_constraint_layout.restype = C.c_uint32
        lib.lmn_kind_constraint_layout.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        VP, U32 = C.c_void_p, C.c_uint32
        lib.lmn_col_alloc.argtypes = [VP, U32, U32, C.POINTER(VP)]
        lib.lmn_col_from_cpu.argtypes = [VP, VP, U32, U32, C.POINTER(VP)]
        lib.lmn_col_to_cpu.argtypes = [VP, VP, VP]
        lib.lmn_col_free.argtypes = [VP, VP]
        lib.lmn_col_free.restype = None
        lib.lmn_col_ncols.argtypes = [VP]
        lib.lmn_col_ncols.restype = U32
        lib.lmn_col_log_size.argtypes = [VP]
        lib.lmn_col_log_size.restype = U32
        lib.lmn_col_device_ptr.argtypes = [VP]
        lib.lmn_col_device_ptr.restype = VP
        lib.lmn_col_view.argtypes = [VP, VP, U32, U32, C.POINTER(VP)]
        lib.lmn_col_bit_reverse.argtypes = [VP, VP]
        lib.lmn_col_precompute_twiddles.argtypes = [VP, U32]
        lib.lmn_col_interpolate.argtypes = [VP, VP]
        lib.lmn_col_evaluate.argtypes = [VP, VP, U32, C.POINTER(VP)]
        lib.lmn_col_evaluate_block.argtypes = [VP, VP, U32, U32, U32, C.POINTER(VP)]
        lib.lmn_col_extend.argtypes = [VP, VP, U32, C.POINTER(VP)]
        lib.lmn_col_eval_at_point.argtypes = [VP, VP, U32, VP, VP]
        lib.lmn_col_commit.argtypes = [VP, C.POINTER(VP), U32, C.POINTER(VP)]
        lib.lmn_tree_root.argtypes = [VP, VP, VP]
        lib.lmn_tree_log_size.argtypes = [VP]
        lib.lmn_tree_log_size.restype = U32
        lib.lmn_tree_layer_to_cpu.argtypes = [VP, VP, U32, VP]
        lib.lmn_tree_decommit.argtypes = [VP, VP, C.POINTER(VP), U32, VP, VP, U32, VP, C.POINTER(VP), C.POINTER(C.c_size_t),
                                          C.POINTER(VP), C.POINTER(C.c_size_t), C.POINTER(VP), C.POINTER(C.c_size_t)]
        lib.lmn_col_gather.argtypes = [VP, VP, VP, U32, VP]
        lib.lmn_col_fri_commit.argtypes = [VP, C.POINTER(VP), U32, VP, C.POINTER(LmnFriCommitResult)]
        lib.lmn_col_fri_close.argtypes = [VP, VP, VP, U32, C.POINTER(LmnFriCloseResult)]
        lib.lmn_col_fri_close_keep.argtypes = [VP, VP, VP, U32, C.POINTER(LmnFriCloseResult), C.POINTER(VP)]
        lib.lmn_positions_from_cpu.argtypes = [VP, VP, U32, U32, C.POINTER(VP)]
        lib.lmn_positions_to_cpu.argtypes = [VP, VP, VP, C.POINTER(U32)]
        lib.lmn_positions_log_domain.argtypes = [VP]
        lib.lmn_positions_log_domain.restype = U32
        lib.lmn_positions_free.argtypes = [VP, VP]
        lib.lmn_positions_free.restype = None
        lib.lmn_open_queries.argtypes = [VP, VP, C.POINTER(LmnOpenItem), U32, C.POINTER(LmnOpening)]
        lib.lmn_verify_many.argtypes = [VP, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), U32, C.POINTER(LmnSettings),
                                        C.POINTER(LmnConfig), C.POINTER(LmnVerifyResult)]
        lib.lmn_ctx_counter.argtypes = [VP, C.c_int]
        lib.lmn_ctx_counter.restype = C.c_uint64
        lib.lmn_tree_free.argtypes = [VP, VP]
        lib.lmn_tree_free.restype = None
        lib.lmn_col_accumulate.argtypes = [VP, VP, VP]
        lib.lmn_col_accumulate_quotients.argtypes = [VP, C.POINTER(VP), U32, VP, VP, VP, U32, VP, U32, VP, C.POINTER(VP)]
        lib.lmn_col_fold_line.argtypes = [VP, VP, VP, C.POINTER(VP)]
        lib.lmn_col_fold_circle_into_line.argtypes = [VP, VP, VP, VP]
        lib.lmn_col_decompose.argtypes = [VP, VP, C.POINTER(VP), VP]
        lib.lmn_col_batch_inverse.argtypes = [VP, VP, VP, C.POINTER(C.c_uint64)]
        lib.lmn_col_batch_inverse_secure.argtypes = [VP, VP, VP, C.POINTER(C.c_uint64)]
        lib.lmn_col_logup.argtypes = [VP, U32, VP, VP, VP, C.POINTER(VP), VP]
        lib.lmn_col_composition.argtypes = [VP, U32, VP, VP, VP, VP, VP, VP, U32, VP]
        lib.lmn_kind_constraints.argtypes = [U32]
        lib.lmn_kind_constraints.restype = U32
        lib.lmn_kind_relations.argtypes = [U32]
        lib.lmn_kind_relations.restype = U32
        lib.lmn_ctx_set_shard.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(LmnCollective)]
        lib.lmn_rccl_unique_id.argtypes = [C.c_void_p]
        lib.lmn_ctx_set_shard_rccl.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.lmn_ctx_clear_shard.argtypes = [C.c_void_p]
        lib.lmn_rows_open.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]
        lib.lmn_rows_push.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        lib.lmn_rows_push_pinned.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        lib.lmn_rows_sync.argtypes = [C.c_void_p]
        lib.lmn_rows_finish.argtypes = [C.c_void_p, C.POINTER(LmnTable)]
        lib.lmn_rows_count.argtypes = [C.c_void_p]
        lib.lmn_rows_count.restype = C.c_uint64
        lib.lmn_rows_reset.argtypes = [C.c_void_p]
        lib.lmn_rows_close.argtypes = [C.c_void_p]
        lib.lmn_rows_close.restype = None
        lib.lmn_rows_append_elementwise_v.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(LmnView),
                                                      C.c_void_p, C.POINTER(LmnView), C.c_uint64, C.POINTER(LmnNodeInfo),
                                                      C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lmn_rows_append_contiguous.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(LmnView),
                                                   C.c_uint64, C.POINTER(LmnNodeInfo), C.c_void_p, C.c_void_p]
        lib.lmn_rows_append_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64,
                                               C.c_uint64, C.POINTER(LmnNodeInfo), C.c_void_p, C.c_void_p]
        lib.lmn_rows_append_lut_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(LmnView),
                                                   C.c_uint64, C.POINTER(LmnNodeInfo), C.c_void_p, C.POINTER(LmnRange),
                                                   C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lmn_trace_check.argtypes = [C.c_void_p, C.POINTER(LmnTable), C.c_size_t, C.POINTER(LmnSettings),
                                        C.POINTER(LmnTraceReport)]
        lib.lmn_trace_elementwise_v.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(LmnView), C.c_void_p,
                                                C.POINTER(LmnView), C.c_uint64, C.POINTER(LmnNodeInfo), C.c_void_p,
                                                C.c_uint64, C.c_void_p]
        lib.lmn_trace_contiguous.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(LmnView), C.c_uint64,
                                             C.POINTER(LmnNodeInfo), C.c_void_p, C.c_uint64, C.c_void_p]
        lib.lmn_trace_lut.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(LmnView), C.c_uint64,
                                      C.POINTER(LmnNodeInfo), C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_uint64, C.c_void_p]
        lib.lmn_trace_lut_ranges.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(LmnView), C.c_uint64,
                                             C.POINTER(LmnNodeInfo), C.c_void_p, C.POINTER(LmnRange), C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_uint64, C.c_void_p]
        lib.lmn_trace_less_than.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(LmnView), C.c_void_p, C.POINTER(LmnView),
                                            C.c_uint64, C.POINTER(LmnNodeInfo), C.c_void_p, C.c_void_p, C.c_uint64,
                                            C.c_void_p]
        lib.lmn_trace_max_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                             C.POINTER(LmnNodeInfo), C.c_void_p, C.c_uint64, C.c_void_p]
        lib.lmn_trace_sum_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                             C.POINTER(LmnNodeInfo), C.c_void_p, C.c_uint64, C.c_void_p]
        lib.lmn_trace_elementwise.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                              C.POINTER(LmnNodeInfo), C.c_void_p, C.c_uint64, C.c_void_p]
        lib.lmn_eval_elementwise_v.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(LmnView), C.c_void_p,
                                               C.POINTER(LmnView), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lmn_eval_reduce.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
        lib.lmn_eval_reduce_split.argtypes = [C.c_uint64, C.c_uint64]
        lib.lmn_eval_reduce_split.restype = C.c_uint32
        lib.lmn_eval_lut_ranges.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(LmnView), C.c_uint64, C.c_void_p,
                                            C.POINTER(LmnRange), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lmn_tensor_range.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        U64 = C.c_uint64
        lib.lmn_trace_many_elementwise_v.argtypes = [VP, U32, VP, C.POINTER(LmnView), U64, VP, C.POINTER(LmnView), U64, U64,
                                                     C.POINTER(LmnNodeInfo), U32, VP, U64, U64, VP, U64, VP, U64, VP]
        lib.lmn_trace_many_contiguous.argtypes = [VP, VP, U64, U64, C.POINTER(LmnView), U64, C.POINTER(LmnNodeInfo), U32, VP,
                                                  U64, U64, VP, U64, VP]
        lib.lmn_trace_many_reduce.argtypes = [VP, U32, VP, U64, U64, U64, U64, C.POINTER(LmnNodeInfo), U32, VP, U64, U64, VP,
                                              U64, VP]
        lib.lmn_trace_many_lut_ranges.argtypes = [VP, U32, VP, C.POINTER(LmnView), U64, U64, C.POINTER(LmnNodeInfo), VP,
                                                  C.POINTER(LmnRange), U32, U32, VP, U64, VP, U64, U64, VP, U64, VP]
        lib.lmn_trace_inputs_float.argtypes = [VP, U32, VP, U64, C.POINTER(LmnNodeInfo), VP, U64, VP]
        lib.lmn_trace_many_inputs_float.argtypes = [VP, U32, VP, U64, U64, C.POINTER(LmnNodeInfo), U32, VP, U64, U64, VP, U64, VP]
        lib.lmn_rows_append_inputs_float.argtypes = [VP, VP, U32, VP, U64, C.POINTER(LmnNodeInfo), VP, VP]
        lib.lmn_eval_inputs_float.argtypes = [VP, U32, VP, U64, VP, VP, VP]
        lib.lmn_tensor_to_float.argtypes = [VP, U32, VP, U64, VP]

    def eval_reduce_split(self, dim: int, back: int) -> int:
        """How `lmn_eval_reduce` maps (dim, back) onto lanes: 0 = one lane per output element, 1 = one wave per group."""
        return int(self.lib.lmn_eval_reduce_split(dim, back))

    def host_rows(self, shape, dtype=np.uint32) -> "PinnedArray":
        """A page-locked numpy array (`lmn_host_alloc`): trace rows written here reach the GPU by direct DMA."""
        return PinnedArray(self, shape, dtype)

    def host_register(self, arr: np.ndarray):
        """Page-lock an existing C-contiguous array in place (`lmn_host_register`); pair with host_unregister."""
        assert arr.flags["C_CONTIGUOUS"]
        rc = self.lib.lmn_host_register(arr.ctypes.data_as(C.c_void_p), arr.nbytes)
        if rc != LMN_OK:
            raise LuminairBackendError(rc, self.lib.lmn_strerror(rc).decode())

    def host_unregister(self, arr: np.ndarray):
        rc = self.lib.lmn_host_unregister(arr.ctypes.data_as(C.c_void_p))
        if rc != LMN_OK:
            raise LuminairBackendError(rc, self.lib.lmn_strerror(rc).decode())

    def default_config(self) -> LmnConfig:
        cfg = LmnConfig()
        self.lib.lmn_default_config(C.byref(cfg))
        return cfg

    def kind_columns(self, kind: int) -> int:
        return int(self.lib.lmn_kind_columns(kind))

    def lut_log_size(self, ranges: Sequence[Tuple[int, int]]) -> int:
        """`LookupLayout::new(ranges).log_size` (crates/air/src/preprocessed.rs:49-52)."""
        arr = (LmnRange * len(ranges))(*[LmnRange(int(a), int(b)) for a, b in ranges])
        out = C.c_uint32()
        rc = self.lib.lmn_lut_log_size(arr, len(ranges), C.byref(out))
        if rc != LMN_OK:
            raise LuminairBackendError(rc, "bad LUT ranges")
        return int(out.value)

    def lut_from_ranges(self, name: str, ranges: Sequence[Tuple[int, int]], log_size: Optional[int] = None):
        """The two preprocessed columns of a sin / exp2 / log2 LUT from the reference's `LookupLayout`
        (`SinPreProcessed::gen_column` and siblings).  Returns (col0, col1), uint32 arrays of 2^log_size words."""
        if log_size is None:
            log_size = self.lut_log_size(ranges)
        arr = (LmnRange * len(ranges))(*[LmnRange(int(a), int(b)) for a, b in ranges])
        c0 = np.empty(1 << log_size, dtype=np.uint32)
        c1 = np.empty(1 << log_size, dtype=np.uint32)
        rc = self.lib.lmn_lut_from_ranges(LUT_KINDS[name], arr, len(ranges), log_size, c0.ctypes.data, c1.ctypes.data)
        if rc != LMN_OK:
            raise LuminairBackendError(rc, "bad LUT ranges")
        return c0, c1

    def grind(self, digest: bytes, pow_bits: int, variant: int = VARIANT_KAT) -> int:
        """GrindOps::grind on a 32-byte channel digest."""
        out = C.c_uint64()
        rc = self.lib.lmn_op_grind(bytes(digest), pow_bits, variant, C.byref(out))
        if rc != LMN_OK:
            raise LuminairBackendError(rc, self.lib.lmn_strerror(rc).decode())
        return int(out.value)

    def verify(self, proof: bytes, variant: int = VARIANT_KAT, config: Optional[LmnConfig] = None,
               settings: Optional[LmnSettings] = None) -> None:
        """`verify(proof, settings)` on the host; raises LuminairBackendError on rejection.  `config` = the
        verifier's own PcsConfig (default: PcsConfig::default(), as the reference hard-codes)."""
        sp = C.byref(settings) if settings is not None else None
        if config is not None:
            rc = self.lib.lmn_verify_with_config(proof, len(proof), sp, C.byref(config))
        else:
            rc = self.lib.lmn_verify(proof, len(proof), sp, variant)
        if rc != LMN_OK:
            msg = self.lib.lmn_last_error(None).decode() or self.lib.lmn_strerror(rc).decode()
            raise LuminairBackendError(rc, msg)

    def verify_many(self, proofs: Sequence[bytes], variant: int = VARIANT_KAT, config: Optional[LmnConfig] = None,
                    settings: Optional[LmnSettings] = None, ctx: Optional["Context"] = None) -> List["VerifyResult"]:
        """`lmn_verify_many`: the verifier's front per proof on the host, its back for all of them on the device of `ctx`
        (default: a context on device 0 that lives for this call).  One `VerifyResult` per proof, whatever the verdicts;
        raises LuminairBackendError only when the call itself fails."""
        proofs = [bytes(p) for p in proofs]
        if not proofs:
            return []
        cfg = LmnConfig()
        if config is not None:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(LmnConfig))
        else:
            self.lib.lmn_default_config(C.byref(cfg))
            cfg.protocol_variant = variant
        own = ctx is None
        if own:
            ctx = Context(0, library=self)
        try:
            n = len(proofs)
            ptrs = (C.c_char_p * n)(*proofs)
            lens = (C.c_size_t * n)(*[len(p) for p in proofs])
            res = (LmnVerifyResult * n)()
            sp = C.byref(settings) if settings is not None else None
            ctx._check(self.lib.lmn_verify_many(ctx.handle, ptrs, lens, n, sp, C.byref(cfg), res))
            return [VerifyResult(r.rc == LMN_OK, int(r.rc), int(r.checks_failed), int(r.stage)) for r in res]
        finally:
            if own:
                ctx.close()

    def diagnose(self, proof: bytes, variant: int, config: Optional[LmnConfig] = None,
                 settings: Optional[LmnSettings] = None):
        """`lmn_verify_diagnose`: (return code, LmnVerifyReport) - which verifier checks `proof` passes under the
        protocol flags `variant`, without stopping at the first failure."""
        cfg = LmnConfig()
        if config is not None:
            C.memmove(C.byref(cfg), C.byref(config), C.sizeof(LmnConfig))
        else:
            self.lib.lmn_default_config(C.byref(cfg))
        cfg.protocol_variant = variant
        rep = LmnVerifyReport()
        sp = C.byref(settings) if settings is not None else None
        rc = self.lib.lmn_verify_diagnose(proof, len(proof), sp, C.byref(cfg), C.byref(rep))
        return rc, rep

    def constraint_layout(self, kind: int, variant: int):
        """(n_protocol, proto_index[16], sign[16]) of `lmn_kind_constraint_layout`."""
        pi, sg = (C.c_int32 * 16)(), (C.c_int32 * 16)()
        n = int(self.lib.lmn_kind_constraint_layout(kind, variant, pi, sg))
        return n, list(pi), list(sg)


_default_library: Optional[Library] = None


def default_library() -> Library:
    global _default_library
    if _default_library is None:
        _default_library = Library()
    return _default_library


class PinnedArray:
    """numpy view of an `lmn_host_alloc` buffer; `.array` is valid until `free()` (or garbage collection of this object)."""

    def __init__(self, library: "Library", shape, dtype=np.uint32):
        self.library = library
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        rc = library.lib.lmn_host_alloc(nbytes, C.byref(p))
        if rc != LMN_OK:
            raise LuminairBackendError(rc, library.lib.lmn_strerror(rc).decode())
        self.ptr = p.value
        buf = (C.c_uint8 * nbytes).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            self.library.lib.lmn_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBuffer:
    def __init__(self, ctx: "Context", ptr: int, nbytes: int, owned: bool = True):
        self.ctx, self.ptr, self.nbytes, self.owned = ctx, ptr, nbytes, owned

    def view(self, offset: int, nbytes: int) -> "DeviceBuffer":
        """A sub-range of this allocation (not owned: freeing it is a no-op)."""
        if offset < 0 or offset + nbytes > self.nbytes:
            raise ValueError("view outside the allocation")
        return DeviceBuffer(self.ctx, self.ptr + offset, nbytes, owned=False)

    def free(self):
        if self.ptr and self.owned:
            self.ctx.lib.lib.lmn_device_free(self.ctx.handle, self.ptr)
        self.ptr = 0


class RowSink:
    """`lmn_rows`: one trace table of a pie, filled chunk by chunk while the host produces its rows (the reference's
    `table.add_row` loop, one `push` at the end of every node) and kept column-major in HBM.  After `finish()` it stands
    where a `TraceTable` stands: in `LuminairPie.from_tables`, `Prover.prove`, `ProverPool.prove_many`, and as the rows of
    a `Context.prove_tables` entry.  It must stay open (and not be reset) until the proof that reads it has returned."""

    def __init__(self, ctx: "Context", kind: int, capacity_rows: int):
        self.ctx, self.kind, self.capacity = ctx, int(kind), int(capacity_rows)
        self.ncols = ctx.lib.kind_columns(self.kind)
        self.table: Optional[LmnTable] = None       # filled in by finish()
        self._keep = []                              # page-locked chunks the GPU may still be reading
        h = C.c_void_p()
        self._check(ctx.lib.lib.lmn_rows_open(ctx.handle, self.kind, self.capacity, C.byref(h)))
        self.handle = h

    @staticmethod
    def open(ctx: "Context", kind: int, capacity_rows: int) -> "RowSink":
        return RowSink(ctx, kind, capacity_rows)

    def _check(self, rc: int):
        if rc != LMN_OK:
            lib = self.ctx.lib.lib
            raise LuminairBackendError(rc, lib.lmn_last_error(None).decode() or lib.lmn_strerror(rc).decode())

    def _chunk(self, rows) -> np.ndarray:
        a = np.asarray(rows)
        if a.dtype != np.uint32 or not a.flags["C_CONTIGUOUS"] or a.size % max(self.ncols, 1):
            raise ValueError("a chunk is a C-contiguous uint32 array of whole rows (%d words each)" % self.ncols)
        return a

    def push(self, rows) -> "RowSink":
        """Rows in any host memory; they are free again when the call returns."""
        a = self._chunk(np.ascontiguousarray(rows, dtype=np.uint32))
        self._check(self.ctx.lib.lib.lmn_rows_push(self.handle, a.ctypes.data, a.size // self.ncols))
        return self

    def push_pinned(self, rows) -> "RowSink":
        """Rows in page-locked memory (a `PinnedArray`'s `.array` or a slice of it, or a `host_register`ed array): no CPU
        copy; the memory must stay untouched until `sync()` or `finish()` returns."""
        a = self._chunk(rows)
        self._check(self.ctx.lib.lib.lmn_rows_push_pinned(self.handle, a.ctypes.data, a.size // self.ncols))
        self._keep.append(a)
        return self

    def sync(self):
        self._check(self.ctx.lib.lib.lmn_rows_sync(self.handle))
        self._keep = []

    def finish(self) -> "RowSink":
        t = LmnTable()
        try:
            self._check(self.ctx.lib.lib.lmn_rows_finish(self.handle, C.byref(t)))
        finally:
            self._keep = []
        self.table = t
        return self

    def reset(self) -> "RowSink":
        self._check(self.ctx.lib.lib.lmn_rows_reset(self.handle))
        self.table = None
        return self

    @property
    def n_rows(self) -> int:
        return int(self.ctx.lib.lib.lmn_rows_count(self.handle))

    @property
    def rows(self) -> "RowSink":          # what a TraceTable's `rows` is to the prover wrappers
        return self

    def columns(self) -> np.ndarray:
        """The finished table as data: (ncols, 2^log_size) words, padding rows included."""
        if self.table is None:
            raise ValueError("the sink is not finished")
        size = max(16, 1 << max(int(self.table.n_rows) - 1, 0).bit_length())
        nbytes = self.ncols * size * 4
        return self.ctx.download(DeviceBuffer(self.ctx, self.table.rows, nbytes, owned=False)).reshape(self.ncols, size)

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.lib.lmn_rows_close(self.handle)
            self.handle = None
            self.table = None

    def __enter__(self) -> "RowSink":
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Col:
    """`lmn_col`: ncols columns of 2^log_size words resident in HBM (stwo `Col<B, _>` / `SecureColumnByCoords<B>`).
    Every method is one level-2 op on the device data; only `from_cpu` / `to_cpu` move bytes over PCIe."""

    def __init__(self, ctx: "Context", handle):
        self.ctx, self.handle = ctx, handle

    @property
    def ncols(self) -> int:
        return int(self.ctx.lib.lib.lmn_col_ncols(self.handle))

    @property
    def log_size(self) -> int:
        return int(self.ctx.lib.lib.lmn_col_log_size(self.handle))

    @property
    def device_ptr(self) -> int:
        return int(self.ctx.lib.lib.lmn_col_device_ptr(self.handle))

    def _new(self, fn, *args) -> "Col":
        out = C.c_void_p()
        self.ctx._check(fn(self.ctx.handle, self.handle, *args, C.byref(out)))
        return Col(self.ctx, out)

    def to_cpu(self) -> np.ndarray:
        host = np.empty((self.ncols, 1 << self.log_size), dtype=np.uint32)
        self.ctx._check(self.ctx.lib.lib.lmn_col_to_cpu(self.ctx.handle, self.handle, host.ctypes.data))
        return host

    def free(self):
        if self.handle:
            self.ctx.lib.lib.lmn_col_free(self.ctx.handle, self.handle)
            self.handle = None

    def view(self, first: int, n: int) -> "Col":
        """Non-owning handle over columns [first, first + n) (valid while this handle lives)."""
        return self._new(self.ctx.lib.lib.lmn_col_view, first, n)

    def bit_reverse(self) -> "Col":
        self.ctx._check(self.ctx.lib.lib.lmn_col_bit_reverse(self.ctx.handle, self.handle))
        return self

    def interpolate(self) -> "Col":
        """evaluations -> coefficients, in place"""
        self.ctx._check(self.ctx.lib.lib.lmn_col_interpolate(self.ctx.handle, self.handle))
        return self

    def evaluate(self, log_domain: int) -> "Col":
        return self._new(self.ctx.lib.lib.lmn_col_evaluate, log_domain)

    def evaluate_block(self, log_domain: int, log_blocks: int, block: int) -> "Col":
        return self._new(self.ctx.lib.lib.lmn_col_evaluate_block, log_domain, log_blocks, block)

    def extend(self, log_size: int) -> "Col":
        return self._new(self.ctx.lib.lib.lmn_col_extend, log_size)

    def eval_at_point(self, column: int, point_xy: Sequence[int]) -> Tuple[int, int, int, int]:
        pt = (C.c_uint32 * 8)(*[int(v) for v in point_xy])
        out = (C.c_uint32 * 4)()
        self.ctx._check(self.ctx.lib.lib.lmn_col_eval_at_point(self.ctx.handle, self.handle, column, pt, out))
        return tuple(int(v) for v in out)

    def accumulate(self, other: "Col") -> "Col":
        """self += other"""
        self.ctx._check(self.ctx.lib.lib.lmn_col_accumulate(self.ctx.handle, self.handle, other.handle))
        return self

    def fold_line(self, alpha) -> "Col":
        al = (C.c_uint32 * 4)(*[int(v) for v in alpha])
        return self._new(self.ctx.lib.lib.lmn_col_fold_line, al)

    def fold_circle_into_line(self, src: "Col", alpha) -> "Col":
        """self = self * alpha^2 + fold(src)"""
        al = (C.c_uint32 * 4)(*[int(v) for v in alpha])
        self.ctx._check(self.ctx.lib.lib.lmn_col_fold_circle_into_line(self.ctx.handle, self.handle, src.handle, al))
        return self

    def gather(self, positions) -> np.ndarray:
        """-> (ncols, n) array: every column at `positions` (any order, repeats allowed).  One launch, one transfer of
        the gathered words; the columns stay in HBM."""
        pos = np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1)
        out = np.empty((self.ncols, len(pos)), dtype=np.uint32)
        self.ctx._check(self.ctx.lib.lib.lmn_col_gather(self.ctx.handle, self.handle, pos.ctypes.data, len(pos),
                                                        out.ctypes.data))
        return out

    def decompose(self):
        """FriOps::decompose -> (g, lambda)"""
        out = C.c_void_p()
        lam = (C.c_uint32 * 4)()
        self.ctx._check(self.ctx.lib.lib.lmn_col_decompose(self.ctx.handle, self.handle, C.byref(out), lam))
        return Col(self.ctx, out), tuple(int(v) for v in lam)

    def _batch_inverse(self, fn, out, count_zeros):
        dst = self if out is None else out
        n_zero = C.c_uint64()
        self.ctx._check(fn(self.ctx.handle, self.handle, dst.handle, C.byref(n_zero) if count_zeros else None))
        return (dst, int(n_zero.value)) if count_zeros else dst

    def batch_inverse(self, out: Optional["Col"] = None, count_zeros: bool = False):
        """FieldOps<BaseField>::batch_inverse: out = self^-1 word by word in M31 (`out=None`: in place).  A zero word
        gives 0.  -> the destination, or (destination, number of zero words) with `count_zeros` (which waits)."""
        return self._batch_inverse(self.ctx.lib.lib.lmn_col_batch_inverse, out, count_zeros)

    def batch_inverse_secure(self, out: Optional["Col"] = None, count_zeros: bool = False):
        """FieldOps<SecureField>::batch_inverse on 4 coordinate columns: element i is (self[0][i], .., self[3][i]) in
        QM31.  A zero element gives 0; `count_zeros` counts QM31 elements."""
        return self._batch_inverse(self.ctx.lib.lib.lmn_col_batch_inverse_secure, out, count_zeros)


class Tree:
    """`lmn_tree`: a committed Merkle tree whose layers stay in HBM."""

    def __init__(self, ctx: "Context", handle):
        self.ctx, self.handle = ctx, handle

    def root(self) -> bytes:
        out = (C.c_uint8 * 32)()
        self.ctx._check(self.ctx.lib.lib.lmn_tree_root(self.ctx.handle, self.handle, out))
        return bytes(out)

    @property
    def log_size(self) -> int:
        return int(self.ctx.lib.lib.lmn_tree_log_size(self.handle))

    def layer(self, layer_log: int) -> List[bytes]:
        buf = (C.c_uint8 * (32 << layer_log))()
        self.ctx._check(self.ctx.lib.lib.lmn_tree_layer_to_cpu(self.ctx.handle, self.handle, layer_log, buf))
        raw = bytes(buf)
        return [raw[32 * i:32 * i + 32] for i in range(1 << layer_log)]

    def decommit(self, cols: Sequence[Col], queries_by_log) -> Tuple[np.ndarray, List[bytes], np.ndarray]:
        """MerkleProver::decommit on the device tree -> (queried values, hash witness, column witness).  `cols`: the
        handles the tree was committed from, same order; `queries_by_log`: {log_size: sorted positions}.  Only the
        opened words and hashes cross the link."""
        L = self.ctx.lib.lib
        groups = [(int(lg), np.ascontiguousarray(q, dtype=np.uint32).reshape(-1)) for lg, q in queries_by_log.items()]
        logs = np.array([lg for lg, _ in groups], dtype=np.uint32)
        counts = np.array([len(q) for _, q in groups], dtype=np.uint32)
        flat = np.concatenate([q for _, q in groups]) if groups else np.zeros(0, dtype=np.uint32)
        arr = (C.c_void_p * max(len(cols), 1))(*[c.handle for c in cols])
        vals, hashes, wit = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nv, nh, nw = C.c_size_t(), C.c_size_t(), C.c_size_t()
        try:
            self.ctx._check(L.lmn_tree_decommit(self.ctx.handle, self.handle, arr, len(cols), logs.ctypes.data,
                                                counts.ctypes.data, len(groups), flat.ctypes.data, C.byref(vals),
                                                C.byref(nv), C.byref(hashes), C.byref(nh), C.byref(wit), C.byref(nw)))

            def words(p, n):
                return np.frombuffer(C.string_at(p, 4 * n), dtype=np.uint32).copy() if n else np.zeros(0, dtype=np.uint32)
            raw = C.string_at(hashes, 32 * nh.value) if nh.value else b""
            return (words(vals, nv.value), [raw[32 * i:32 * i + 32] for i in range(nh.value)], words(wit, nw.value))
        finally:
            for p in (vals, hashes, wit):
                if p.value:
                    L.lmn_free(p)

    def free(self):
        if self.handle:
            self.ctx.lib.lib.lmn_tree_free(self.ctx.handle, self.handle)
            self.handle = None


class Positions:
    """`lmn_positions`: up to 1024 ascending distinct query positions of a domain of 2^log_domain rows, in device memory -
    what `Context.open_queries` reads.  Made by `Context.positions_from_cpu` or left behind by
    `Context.fri_close(..., keep=True)`."""

    def __init__(self, ctx: "Context", handle):
        self.ctx, self.handle = ctx, handle

    @property
    def log_domain(self) -> int:
        return int(self.ctx.lib.lib.lmn_positions_log_domain(self.handle))

    def to_cpu(self) -> List[int]:
        buf = np.zeros(OPEN_MAX_POSITIONS, dtype=np.uint32)
        n = C.c_uint32()
        self.ctx._check(self.ctx.lib.lib.lmn_positions_to_cpu(self.ctx.handle, self.handle, buf.ctypes.data, C.byref(n)))
        return [int(v) for v in buf[:n.value]]

    def free(self):
        if self.handle:
            self.ctx.lib.lib.lmn_positions_free(self.ctx.handle, self.handle)
            self.handle = None


class PreparedSettings:
    """`lmn_prepared`: a circuit's preprocessed tree (tree 0) - LUT and range-check columns, coefficients, low-degree
    extension, Merkle layers, root - built once on the device and shared read-only by every proof that names it with
    `prepared=` (`Context.prove_tables` / `prove_submit`, `Prover.prove`, `ProverPool.prove_many`, and - made with the batch
    library - `BatchProver.prove_batch`, `BatchPool.prove_many`).  The proofs are byte-identical to the ones made with the
    LUTs handed over per proof.

    luts: {"sin" | "exp2" | "log2": (col0, col1)} as `Context.prove_tables` takes them (free again when this returns);
    lookups: LOOKUP_* bits of the lookup components the pies will contain - LOOKUP_RANGE_CHECK for a graph with LessThan;
    None = the bits of `luts`.  A prepared object works with contexts of its own library, device and log_blowup."""

    def __init__(self, device: int = 0, config: Optional[LmnConfig] = None, luts=None, lookups: Optional[int] = None,
                 library: Optional[Library] = None):
        self.lib = library or default_library()
        self.device = device
        self.handle = None
        cfg = config or self.lib.default_config()
        luts = luts or {}
        if lookups is None:
            lookups = 0
            for name in luts:
                lookups |= LOOKUP_BITS[name]
        _arr, _n, settings, _keep = Context._marshal_tables(None, [], luts)
        h = C.c_void_p()
        rc = self.lib.lib.lmn_settings_prepare(device, C.byref(cfg), C.byref(settings), int(lookups), C.byref(h))
        if rc != LMN_OK:
            msg = self.lib.lib.lmn_last_error(None).decode() or self.lib.lib.lmn_strerror(rc).decode()
            raise LuminairBackendError(rc, msg)
        self.handle = h

    def _handle_for(self, library: Library):
        """the C handle, for a call into `library` (which must be the library that made it)"""
        if not self.handle:
            raise LuminairBackendError(ERR_INVALID_ARGUMENT, "the prepared settings are closed")
        if os.path.realpath(library.path) != os.path.realpath(self.lib.path):
            raise LuminairBackendError(ERR_INVALID_ARGUMENT, "prepared settings made by %s cannot be used with %s"
                                       % (self.lib.path, library.path))
        return self.handle

    @property
    def root(self) -> bytes:
        """the root of tree 0: `commitments[0]` of every proof made with this object"""
        out = (C.c_uint8 * 32)()
        rc = self.lib.lib.lmn_prepared_root(self._handle_for(self.lib), out)
        if rc != LMN_OK:
            raise LuminairBackendError(rc, self.lib.lib.lmn_strerror(rc).decode())
        return bytes(out)

    @property
    def lookups(self) -> int:
        return int(self.lib.lib.lmn_prepared_lookups(self._handle_for(self.lib)))

    def close(self):
        """drops this reference; proofs in flight keep the object alive until they have been returned"""
        if getattr(self, "handle", None):
            self.lib.lib.lmn_prepared_destroy(self.handle)
            self.handle = None

    def __enter__(self) -> "PreparedSettings":
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One prover context per GPU (`lmn_ctx`)."""

    def __init__(self, device: int = 0, config: Optional[LmnConfig] = None, library: Optional[Library] = None):
        self.lib = library or default_library()
        self.config = config or self.lib.default_config()
        self.device = device
        h = C.c_void_p()
        rc = self.lib.lib.lmn_ctx_create(device, C.byref(self.config), C.byref(h))
        if rc != LMN_OK:
            msg = self.lib.lib.lmn_last_error(None).decode() or self.lib.lib.lmn_strerror(rc).decode()
            raise LuminairBackendError(rc, msg)
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            slab = getattr(self, "_graph_slab", None)      # DeviceGraph's cached allocation (luminair_amd/graph.py)
            if slab is not None:
                slab.free()
                self._graph_slab = None
            self.lib.lib.lmn_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != LMN_OK:
            msg = self.lib.lib.lmn_last_error(self.handle).decode() or self.lib.lib.lmn_strerror(rc).decode()
            raise LuminairBackendError(rc, msg)

    # ---- level-2 ops on device handles (lmn_col_* / lmn_tree_*)
    def col_from_cpu(self, cols: np.ndarray) -> Col:
        a = np.ascontiguousarray(cols, dtype=np.uint32)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        ncols, n = a.shape
        if n & (n - 1) or n == 0:
            raise ValueError("column length must be a power of two")
        out = C.c_void_p()
        self._check(self.lib.lib.lmn_col_from_cpu(self.handle, a.ctypes.data, ncols, n.bit_length() - 1, C.byref(out)))
        return Col(self, out)

    def col_zeros(self, ncols: int, log_size: int) -> Col:
        out = C.c_void_p()
        self._check(self.lib.lib.lmn_col_alloc(self.handle, ncols, log_size, C.byref(out)))
        return Col(self, out)

    def precompute_twiddles(self, log_size: int):
        self._check(self.lib.lib.lmn_col_precompute_twiddles(self.handle, log_size))

    def commit(self, cols: Sequence[Col]) -> Tree:
        arr = (C.c_void_p * max(len(cols), 1))(*[c.handle for c in cols])
        out = C.c_void_p()
        self._check(self.lib.lib.lmn_col_commit(self.handle, arr, len(cols), C.byref(out)))
        return Tree(self, out)

    def fri_commit(self, cols: Sequence[Col], start_digest: bytes) -> FriCommit:
        """`lmn_col_fri_commit`: the FRI commit loop of `prove` (stwo FriProver::commit without the last layer's
        interpolation) on secure-column handles of strictly decreasing sizes, from the channel digest `start_digest`;
        roots, alphas, every layer's values, every tree level the loop wrote and the form each layer took."""
        L = self.lib.lib
        if len(start_digest) != 32:
            raise ValueError("start_digest is 32 bytes")
        arr = (C.c_void_p * max(len(cols), 1))(*[c.handle for c in cols])
        dig = (C.c_uint8 * 32)(*start_digest)
        res = LmnFriCommitResult()
        try:
            self._check(L.lmn_col_fri_commit(self.handle, arr, len(cols), dig, C.byref(res)))
            n = int(res.n_trees)

            def words(p, count):
                return np.frombuffer(C.string_at(p, 4 * count), dtype=np.uint32).copy() if count else np.zeros(0, dtype=np.uint32)
            raw = C.string_at(res.roots, 32 * n)
            alphas = words(res.alphas, 4 * n).reshape(n, 4)
            tree_logs = [int(v) for v in words(res.tree_logs, n)]
            masks = words(res.level_masks, n)
            forms = [int(v) for v in words(res.forms, n + 1)]
            values = words(res.values, int(res.n_value_words))
            levels = words(res.levels, int(res.n_level_words))
            layer_logs = [tree_logs[0] - 1 - i for i in range(n)]
            layer_values, at = [], 0
            for lg in layer_logs:
                layer_values.append(values[at:at + (4 << lg)].reshape(4, 1 << lg))
                at += 4 << lg
            assert at == len(values)
            tree_levels, at = [], 0
            for t in range(n):
                lv = []
                for l in range(tree_logs[t] + 1):
                    if (int(masks[t]) >> l) & 1:
                        lv.append(levels[at:at + (8 << l)].reshape(1 << l, 8))
                        at += 8 << l
                    else:
                        lv.append(None)
                tree_levels.append(lv)
            assert at == len(levels)
            return FriCommit([raw[32 * t:32 * t + 32] for t in range(n)], [tuple(int(v) for v in a) for a in alphas],
                             tree_logs, tree_levels, forms[0], layer_logs, layer_values, forms[1:])
        finally:
            for name in ("roots", "alphas", "tree_logs", "level_masks", "forms", "values", "levels"):
                p = getattr(res, name)
                if p:
                    L.lmn_free(p)

    def positions_from_cpu(self, positions, log_domain: int) -> Positions:
        """`lmn_positions_from_cpu`: at most 1024 strictly ascending positions < 2^log_domain"""
        pos = np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1)
        out = C.c_void_p()
        self._check(self.lib.lib.lmn_positions_from_cpu(self.handle, pos.ctypes.data if len(pos) else None, len(pos),
                                                        log_domain, C.byref(out)))
        return Positions(self, out)

    def open_queries(self, positions: Positions, items) -> List[Opening]:
        """`lmn_open_queries`: opens every item - (tree, the handles it was committed from[, flags]) - at `positions`
        with one plan launch, one fetch launch, one transfer and one wait; the walk that decides what an opening needs
        runs on the device."""
        L = self.lib.lib
        n = len(items)
        c_items = (LmnOpenItem * max(n, 1))()
        keep = []
        for k, it in enumerate(items):
            tree, cols = it[0], it[1]
            arr = (C.c_void_p * max(len(cols), 1))(*[c.handle for c in cols])
            keep.append(arr)
            c_items[k] = LmnOpenItem(tree.handle, arr, len(cols), int(it[2]) if len(it) > 2 else 0)
        res = (LmnOpening * max(n, 1))()
        try:
            self._check(L.lmn_open_queries(self.handle, positions.handle, c_items, n, res))

            def words(p, cnt):
                return np.frombuffer(C.string_at(p, 4 * cnt), dtype=np.uint32).copy() if cnt else np.zeros(0, dtype=np.uint32)
            out = []
            for k in range(n):
                r = res[k]
                raw = C.string_at(r.hash_witness, 32 * r.n_hashes) if r.n_hashes else b""
                fri = words(r.fri_witness, int(r.n_fri_words)).reshape(-1, 4)
                out.append(Opening(words(r.queried_values, int(r.n_values)),
                                   [raw[32 * i:32 * i + 32] for i in range(int(r.n_hashes))],
                                   words(r.column_witness, int(r.n_column_words)), [tuple(int(v) for v in q) for q in fri]))
            return out
        finally:
            for k in range(n):
                for name in ("queried_values", "hash_witness", "column_witness", "fri_witness"):
                    p = getattr(res[k], name)
                    if p:
                        L.lmn_free(p)

    def fri_close(self, col: Col, start_digest: bytes, log_query_domain: int, keep: bool = False):
        """`lmn_col_fri_close`: what stands between FRI's layer loop and the decommitment, on the device - the last layer's
        polynomial (`col`: 4 coordinate columns of 2^(log_last_layer + log_blowup) rows) and its degree check, mix_felts
        from the channel digest `start_digest`, the grind, mix_u64 and the query positions of a domain of
        2^log_query_domain rows.  keep=True (`lmn_col_fri_close_keep`): -> (FriClose, Positions) - the positions also stay
        on the device, in a handle `open_queries` reads."""
        L = self.lib.lib
        if len(start_digest) != 32:
            raise ValueError("start_digest is 32 bytes")
        dig = (C.c_uint8 * 32)(*start_digest)
        res = LmnFriCloseResult()
        kept = C.c_void_p()
        try:
            if keep:
                self._check(L.lmn_col_fri_close_keep(self.handle, col.handle, dig, log_query_domain, C.byref(res), C.byref(kept)))
            else:
                self._check(L.lmn_col_fri_close(self.handle, col.handle, dig, log_query_domain, C.byref(res)))
            nc, npos = int(res.n_coeffs), int(res.n_positions)
            coeffs = np.frombuffer(C.string_at(res.coeffs, 16 * nc), dtype=np.uint32).reshape(nc, 4)
            positions = np.frombuffer(C.string_at(res.positions, 4 * npos), dtype=np.uint32) if npos else []
            out = FriClose([tuple(int(v) for v in c) for c in coeffs],
                           None if res.first_bad == 0xffffffff else int(res.first_bad), int(res.nonce), int(res.grind_rounds),
                           [int(v) for v in positions], bytes(res.digest_after_coeffs), bytes(res.digest_after_nonce),
                           bytes(res.digest_end), int(res.n_sent_end))
            return (out, Positions(self, kept)) if keep else out
        finally:
            for name in ("coeffs", "positions"):
                p = getattr(res, name)
                if p:
                    L.lmn_free(p)

    def col_accumulate_quotients(self, cols: Sequence[Col], samples, points, alpha) -> Col:
        """As `accumulate_quotients`, on resident columns; returns the secure column (4 coordinate columns)."""
        arr = (C.c_void_p * len(cols))(*[c.handle for c in cols])
        sc = np.array([s[0] for s in samples], dtype=np.uint32)
        sp = np.array([s[1] for s in samples], dtype=np.uint32)
        sv = np.array([list(s[2]) for s in samples], dtype=np.uint32).reshape(-1)
        pts = np.array([list(p) for p in points], dtype=np.uint32).reshape(-1)
        al = (C.c_uint32 * 4)(*[int(v) for v in alpha])
        out = C.c_void_p()
        self._check(self.lib.lib.lmn_col_accumulate_quotients(
            self.handle, arr, len(cols), sc.ctypes.data, sp.ctypes.data, sv.ctypes.data, len(samples), pts.ctypes.data,
            len(points), al, C.byref(out)))
        return Col(self, out)

    N_ELEMS = 5   # LMN_N_ELEMS: NodeElements, RangeCheck, Sin, Exp2, Log2

    @staticmethod
    def _elems_words(elems):
        """elems: {set index: (z words, alpha words)} or a flat sequence of N_ELEMS * 8 words"""
        if isinstance(elems, dict):
            flat = [0] * (8 * Context.N_ELEMS)
            for e, (z, a) in elems.items():
                flat[8 * e:8 * e + 4] = [int(v) for v in z]
                flat[8 * e + 4:8 * e + 8] = [int(v) for v in a]
            elems = flat
        if len(elems) != 8 * Context.N_ELEMS:
            raise ValueError("elems: %d words expected" % (8 * Context.N_ELEMS))
        return (C.c_uint32 * (8 * Context.N_ELEMS))(*[int(v) for v in elems])

    def col_logup(self, kind: int, main: Col, pre: Optional[Col], elems) -> Tuple[Col, Tuple[int, int, int, int]]:
        """`write_interaction_trace` of component `kind` on resident columns -> (interaction columns, claimed sum)."""
        out = C.c_void_p()
        claimed = (C.c_uint32 * 4)()
        self._check(self.lib.lib.lmn_col_logup(self.handle, kind, main.handle, pre.handle if pre is not None else None,
                                               self._elems_words(elems), C.byref(out), claimed))
        return Col(self, out), tuple(int(v) for v in claimed)

    def col_composition(self, kind: int, main_lde: Col, inter_lde: Col, pre_lde: Optional[Col], elems, claimed, coeffs,
                        acc: Col) -> Col:
        """acc += sum_k constraint_k * coeffs[k] / Z of component `kind` on its evaluation domain."""
        cw = (C.c_uint32 * (4 * len(coeffs)))(*[int(v) for c in coeffs for v in c])
        cl = (C.c_uint32 * 4)(*[int(v) for v in claimed])
        self._check(self.lib.lib.lmn_col_composition(
            self.handle, kind, main_lde.handle, inter_lde.handle, pre_lde.handle if pre_lde is not None else None,
            self._elems_words(elems), cl, cw, len(coeffs), acc.handle))
        return acc

    # ---- single-proof sharding (lmn_ctx_set_shard*)
    def set_shard(self, rank: int, world: int, all_gather, fri_min_log: int = 0, all_to_all=None):
        """Shard every later `prove` over `world` contexts (one per GPU, one per process).  `all_gather(buf_ptr,
        bytes_per_rank, stream)` is the in-place all-gather of `lmn_collective` (device pointer as an int);
        `all_to_all(send_ptr, send_off, send_bytes, recv_ptr, recv_off, recv_bytes, stream)` (lists of `world` ints) the
        optional second primitive."""
        def _cb(_user, buf, nbytes, stream):
            try:
                all_gather(buf, nbytes, stream)
                return 0
            except Exception:   # never unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        def _a2a(_user, send, so, sb, recv, ro, rb, stream):
            try:
                all_to_all(send, [so[p] for p in range(world)], [sb[p] for p in range(world)], recv,
                           [ro[p] for p in range(world)], [rb[p] for p in range(world)], stream)
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        cb = ALL_GATHER_FN(_cb)
        cb2 = ALL_TO_ALL_FN(_a2a) if all_to_all is not None else ALL_TO_ALL_FN()
        coll = LmnCollective(None, cb, None, None, cb2)
        self._check(self.lib.lib.lmn_ctx_set_shard(self.handle, rank, world, fri_min_log, C.byref(coll)))
        # keep the trampolines alive as long as the context uses them (a rejected call keeps the previous ones)
        self._shard_cb, self._shard_coll = (cb, cb2), coll

    def rccl_unique_id(self) -> bytes:
        buf = (C.c_uint8 * RCCL_ID_BYTES)()
        rc = self.lib.lib.lmn_rccl_unique_id(buf)
        if rc != LMN_OK:
            raise LuminairBackendError(rc, self.lib.lib.lmn_last_error(None).decode() or "lmn_rccl_unique_id failed")
        return bytes(buf)

    def set_shard_rccl(self, rank: int, world: int, unique_id: bytes, fri_min_log: int = 0):
        """Built-in transport: RCCL over xGMI on the prover's own stream (`unique_id` from rank 0's rccl_unique_id)."""
        if len(unique_id) != RCCL_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % RCCL_ID_BYTES)
        buf = (C.c_uint8 * RCCL_ID_BYTES)(*unique_id)
        self._check(self.lib.lib.lmn_ctx_set_shard_rccl(self.handle, rank, world, fri_min_log, buf))

    def clear_shard(self):
        self._check(self.lib.lib.lmn_ctx_clear_shard(self.handle))
        self._shard_cb = self._shard_coll = None

    def upload(self, arr: np.ndarray) -> DeviceBuffer:
        arr = np.ascontiguousarray(arr)
        out = C.c_void_p()
        self._check(self.lib.lib.lmn_upload(self.handle, arr.ctypes.data, arr.nbytes, C.byref(out)))
        return DeviceBuffer(self, out.value, arr.nbytes)

    def alloc(self, nbytes: int) -> DeviceBuffer:
        out = C.c_void_p()
        self._check(self.lib.lib.lmn_device_alloc(self.handle, nbytes, C.byref(out)))
        return DeviceBuffer(self, out.value, nbytes)

    def upload_to(self, buf: DeviceBuffer, arr: np.ndarray) -> DeviceBuffer:
        arr = np.ascontiguousarray(arr)
        if arr.nbytes > buf.nbytes:
            raise ValueError("destination too small")
        self._check(self.lib.lib.lmn_upload_to(self.handle, arr.ctypes.data, arr.nbytes, buf.ptr))
        return buf

    def device_copy(self, dst_ptr: int, src_ptr: int, nbytes: int):
        """Stream-ordered device-to-device copy (returns without waiting)."""
        self._check(self.lib.lib.lmn_device_copy(self.handle, dst_ptr, src_ptr, nbytes))

    def download(self, buf: DeviceBuffer, dtype=np.uint32) -> np.ndarray:
        host = np.empty(buf.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        self._check(self.lib.lib.lmn_download(self.handle, buf.ptr, host.ctypes.data, buf.nbytes))
        return host

    def trace_elementwise(self, kind: int, lhs: DeviceBuffer, rhs: Optional[DeviceBuffer], n: int, node_id: int,
                          input_ids, num_consumers: int, is_final_output: bool = False, input_mults=(-1, -1),
                          rows: Optional[DeviceBuffer] = None, row_offset: int = 0,
                          lhs_view: Optional[LmnView] = None, rhs_view: Optional[LmnView] = None,
                          out: Optional[DeviceBuffer] = None, sink: Optional["RowSink"] = None,
                          refused: Optional[DeviceBuffer] = None):
        """`process_trace` of one Add / Mul / Recip node on device tensors (int32 Fixed<12> values).
        Returns (rows DeviceBuffer, out DeviceBuffer).
        sink= (every `trace_*` method takes it): the node's rows are appended to that `RowSink`'s columns at its current
        row count instead (`lmn_rows_append_*`; `rows` / `row_offset` are not used, and the sink is returned in place of the
        rows buffer); `refused` is then a uint32 counter on the device that grows by the refused elements.  Nothing waits."""
        L = self.lib.lib
        if rows is None and sink is None:
            rows = self.alloc((row_offset + n) * self.lib.kind_columns(kind) * 4)
        out = out or self.alloc(n * 4)
        info = _node_info(node_id, input_ids, num_consumers, is_final_output, input_mults)
        if sink is not None:
            self._check(L.lmn_rows_append_elementwise_v(self.handle, sink.handle, kind, lhs.ptr, _ref(lhs_view), _addr(rhs),
                                                        _ref(rhs_view), n, C.byref(info), None, out.ptr, _addr(refused)))
            return sink, out
        if lhs_view is None and rhs_view is None:
            self._check(L.lmn_trace_elementwise(self.handle, kind, lhs.ptr, _addr(rhs), n, C.byref(info), rows.ptr, row_offset,
                                                out.ptr))
        else:
            self._check(L.lmn_trace_elementwise_v(self.handle, kind, lhs.ptr, _ref(lhs_view), _addr(rhs), _ref(rhs_view), n,
                                                  C.byref(info), rows.ptr, row_offset, out.ptr))
        return rows, out

    def trace_contiguous(self, inp: DeviceBuffer, in_size: int, out_size: int, node_id: int, input_id: int,
                         num_consumers: int, is_final_output: bool = False, input_mult: int = -1,
                         view: Optional[LmnView] = None, rows: Optional[DeviceBuffer] = None, row_offset: int = 0,
                         out: Optional[DeviceBuffer] = None, sink: Optional["RowSink"] = None,
                         refused: Optional[DeviceBuffer] = None):
        """`LuminairContiguous::process_trace` in the reference's row rule: max(in_size, out_size) rows."""
        L = self.lib.lib
        if rows is None and sink is None:
            rows = self.alloc((row_offset + max(in_size, out_size)) * 11 * 4)
        out = out or self.alloc(out_size * 4)
        info = _node_info(node_id, (input_id,), num_consumers, is_final_output, (input_mult,))
        if sink is not None:
            self._check(L.lmn_rows_append_contiguous(self.handle, sink.handle, inp.ptr, in_size, _ref(view), out_size,
                                                     C.byref(info), out.ptr, _addr(refused)))
            return sink, out
        self._check(L.lmn_trace_contiguous(self.handle, inp.ptr, in_size, _ref(view), out_size, C.byref(info), rows.ptr,
                                           row_offset, out.ptr))
        return rows, out

    def trace_lut(self, kind: int, inp: DeviceBuffer, n: int, node_id: int, input_id: int, num_consumers: int,
                  lut_col1: DeviceBuffer, lo: int = 0, lut_len: int = 0, mult: DeviceBuffer = None,
                  is_final_output: bool = False, input_mult: int = -1, view: Optional[LmnView] = None,
                  rows: Optional[DeviceBuffer] = None, row_offset: int = 0, out: Optional[DeviceBuffer] = None,
                  ranges: Optional[Sequence[Tuple[int, int]]] = None, sink: Optional["RowSink"] = None,
                  refused: Optional[DeviceBuffer] = None):
        """`process_trace` of a Sin / Exp2 / Log2 node; `mult` (the lookup component's table) is updated in place.
        The LUT enumerates either the single range lo .. lo + lut_len - 1 or `ranges` (ascending, disjoint).
        With sink= an input outside every range is a refused element (marked, counted), not an error of the call."""
        L = self.lib.lib
        if rows is None and sink is None:
            rows = self.alloc((row_offset + n) * 12 * 4)
        out = out or self.alloc(n * 4)
        info = _node_info(node_id, (input_id,), num_consumers, is_final_output, (input_mult,))
        if sink is not None:
            rg = ranges if ranges is not None else [(lo, lo + lut_len - 1)]
            self._check(L.lmn_rows_append_lut_ranges(self.handle, sink.handle, kind, inp.ptr, _ref(view), n, C.byref(info),
                                                     lut_col1.ptr, _range_array(rg), len(rg), mult.ptr, out.ptr, _addr(refused)))
            return sink, out
        if ranges is None:
            self._check(L.lmn_trace_lut(self.handle, kind, inp.ptr, _ref(view), n, C.byref(info), lut_col1.ptr, lo, lut_len,
                                        mult.ptr, rows.ptr, row_offset, out.ptr))
        else:
            self._check(L.lmn_trace_lut_ranges(self.handle, kind, inp.ptr, _ref(view), n, C.byref(info), lut_col1.ptr,
                                               _range_array(ranges), len(ranges), mult.ptr, rows.ptr, row_offset, out.ptr))
        return rows, out

    def trace_sum_reduce(self, inp: DeviceBuffer, front: int, dim: int, back: int, node_id: int, input_id: int,
                         num_consumers: int, is_final_output: bool = False, input_mult: int = -1,
                         rows: Optional[DeviceBuffer] = None, row_offset: int = 0, maximum: bool = False,
                         out: Optional[DeviceBuffer] = None, sink: Optional["RowSink"] = None,
                         refused: Optional[DeviceBuffer] = None):
        """`LuminairSumReduce::process_trace` (or MaxReduce with maximum=True) on a contiguous
        (front, dim, back) int32 device tensor."""
        L = self.lib.lib
        if rows is None and sink is None:
            rows = self.alloc((row_offset + front * dim * back) * (15 if maximum else 14) * 4)
        out = out or self.alloc(front * back * 4)
        info = _node_info(node_id, (input_id,), num_consumers, is_final_output, (input_mult,))
        if sink is not None:
            self._check(L.lmn_rows_append_reduce(self.handle, sink.handle, 1 if maximum else 0, inp.ptr, front, dim, back,
                                                 C.byref(info), out.ptr, _addr(refused)))
            return sink, out
        fn = L.lmn_trace_max_reduce if maximum else L.lmn_trace_sum_reduce
        self._check(fn(self.handle, inp.ptr, front, dim, back, C.byref(info), rows.ptr, row_offset, out.ptr))
        return rows, out

    def trace_less_than(self, lhs: DeviceBuffer, rhs: DeviceBuffer, n: int, node_id: int, input_ids, num_consumers: int,
                        range_check_mult: DeviceBuffer, is_final_output: bool = False, input_mults=(-1, -1),
                        rows: Optional[DeviceBuffer] = None, row_offset: int = 0,
                        lhs_view: Optional[LmnView] = None, rhs_view: Optional[LmnView] = None,
                        out: Optional[DeviceBuffer] = None, sink: Optional["RowSink"] = None,
                        refused: Optional[DeviceBuffer] = None):
        """`LuminairLessThan::process_trace`; `range_check_mult` (256 words) is the RangeCheckLookup table."""
        L = self.lib.lib
        if rows is None and sink is None:
            rows = self.alloc((row_offset + n) * 22 * 4)
        out = out or self.alloc(n * 4)
        info = _node_info(node_id, input_ids, num_consumers, is_final_output, input_mults)
        if sink is not None:
            self._check(L.lmn_rows_append_elementwise_v(self.handle, sink.handle, 13, lhs.ptr, _ref(lhs_view), rhs.ptr,
                                                        _ref(rhs_view), n, C.byref(info), range_check_mult.ptr, out.ptr,
                                                        _addr(refused)))
            return sink, out
        self._check(L.lmn_trace_less_than(self.handle, lhs.ptr, _ref(lhs_view), rhs.ptr, _ref(rhs_view), n, C.byref(info),
                                          range_check_mult.ptr, rows.ptr, row_offset, out.ptr))
        return rows, out

    # ---- lmn_trace_many_*: one call (one launch) fills a node's rows for `n_members` pies of one shape.  Member m works on
    # base + m * stride: operand and `out` strides in elements (0 = shared), `rows_stride` in rows of the kind, multiplicity
    # strides in words.  `refused`: n_members uint32 counters on the device, grown by each member's refused elements.
    # rows / out must be given (the caller lays out the members' regions); nothing waits.
    def trace_many_elementwise(self, kind: int, lhs: DeviceBuffer, rhs: Optional[DeviceBuffer], n: int, n_members: int,
                               node_id: int, input_ids, num_consumers: int, rows: DeviceBuffer, rows_stride: int,
                               out: Optional[DeviceBuffer], out_stride: int, lhs_stride: int = 0, rhs_stride: int = 0,
                               is_final_output: bool = False, input_mults=(-1, -1), row_offset: int = 0,
                               lhs_view: Optional[LmnView] = None, rhs_view: Optional[LmnView] = None,
                               range_check_mult: Optional[DeviceBuffer] = None, range_check_mult_stride: int = 0,
                               refused: Optional[DeviceBuffer] = None):
        """`lmn_trace_many_elementwise_v`: every kind of `trace_elementwise`, and LessThan with `range_check_mult`."""
        info = _node_info(node_id, input_ids, num_consumers, is_final_output, input_mults)
        self._check(self.lib.lib.lmn_trace_many_elementwise_v(
            self.handle, kind, _addr(lhs), _ref(lhs_view), lhs_stride, _addr(rhs), _ref(rhs_view), rhs_stride, n, C.byref(info),
            n_members, _addr(rows), row_offset, rows_stride, _addr(out), out_stride, _addr(range_check_mult),
            range_check_mult_stride, _addr(refused)))
        return rows, out

    def trace_many_contiguous(self, inp: DeviceBuffer, in_size: int, out_size: int, n_members: int, node_id: int,
                              input_id: int, num_consumers: int, rows: DeviceBuffer, rows_stride: int,
                              out: Optional[DeviceBuffer], out_stride: int, inp_stride: int = 0,
                              is_final_output: bool = False, input_mult: int = -1, view: Optional[LmnView] = None,
                              row_offset: int = 0, refused: Optional[DeviceBuffer] = None):
        """`lmn_trace_many_contiguous`: the reference's buffer rule, max(in_size, out_size) rows per member."""
        info = _node_info(node_id, (input_id,), num_consumers, is_final_output, (input_mult,))
        self._check(self.lib.lib.lmn_trace_many_contiguous(
            self.handle, _addr(inp), inp_stride, in_size, _ref(view), out_size, C.byref(info), n_members, _addr(rows), row_offset,
            rows_stride, _addr(out), out_stride, _addr(refused)))
        return rows, out

    def trace_many_reduce(self, inp: DeviceBuffer, front: int, dim: int, back: int, n_members: int, node_id: int,
                          input_id: int, num_consumers: int, rows: DeviceBuffer, rows_stride: int,
                          out: Optional[DeviceBuffer], out_stride: int, inp_stride: int = 0, maximum: bool = False,
                          is_final_output: bool = False, input_mult: int = -1, row_offset: int = 0,
                          refused: Optional[DeviceBuffer] = None):
        """`lmn_trace_many_reduce`: SumReduce, or MaxReduce with maximum=True, of a (front, dim, back) tensor per member."""
        info = _node_info(node_id, (input_id,), num_consumers, is_final_output, (input_mult,))
        self._check(self.lib.lib.lmn_trace_many_reduce(
            self.handle, 1 if maximum else 0, _addr(inp), inp_stride, front, dim, back, C.byref(info), n_members, _addr(rows),
            row_offset, rows_stride, _addr(out), out_stride, _addr(refused)))
        return rows, out

    def trace_many_lut(self, kind: int, inp: DeviceBuffer, n: int, n_members: int, node_id: int, input_id: int,
                       num_consumers: int, lut_col1: DeviceBuffer, ranges: Sequence[Tuple[int, int]], mult: DeviceBuffer,
                       mult_stride: int, rows: DeviceBuffer, rows_stride: int, out: Optional[DeviceBuffer], out_stride: int,
                       inp_stride: int = 0, is_final_output: bool = False, input_mult: int = -1,
                       view: Optional[LmnView] = None, row_offset: int = 0, refused: Optional[DeviceBuffer] = None):
        """`lmn_trace_many_lut_ranges`: Sin / Exp2 / Log2 over `ranges` (one (lo, hi) pair for a single-range LUT);
        `lut_col1` is shared, `mult` holds one multiplicity table per member.  An input outside every range is a refused
        element (marked, counted), not an error."""
        info = _node_info(node_id, (input_id,), num_consumers, is_final_output, (input_mult,))
        self._check(self.lib.lib.lmn_trace_many_lut_ranges(
            self.handle, kind, _addr(inp), _ref(view), inp_stride, n, C.byref(info), _addr(lut_col1), _range_array(ranges),
            len(ranges), n_members, _addr(mult), mult_stride, _addr(rows), row_offset, rows_stride, _addr(out), out_stride,
            _addr(refused)))
        return rows, out

    # ---- lmn_eval_*: the producers' forward pass (values, their range, the refused elements; no rows, no waiting).
    # `minmax`: two int32 words on the device, set to the range of what the call wrote; `refused`: a uint32 counter on the
    # device that grows by the refused elements.  Both optional.  Returns the output DeviceBuffer.
    def eval_elementwise(self, kind: int, lhs: DeviceBuffer, rhs: Optional[DeviceBuffer], n: int,
                         lhs_view: Optional[LmnView] = None, rhs_view: Optional[LmnView] = None,
                         out: Optional[DeviceBuffer] = None, minmax: Optional[DeviceBuffer] = None,
                         refused: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """`Operator::process` of an elementwise node (LessThan included) on int32 Fixed<12> device tensors."""
        out = out or self.alloc(max(n, 1) * 4)
        self._check(self.lib.lib.lmn_eval_elementwise_v(self.handle, kind, _addr(lhs), _ref(lhs_view), _addr(rhs), _ref(rhs_view),
                                                        n, out.ptr, _addr(minmax), _addr(refused)))
        return out

    def eval_reduce(self, inp: DeviceBuffer, front: int, dim: int, back: int, maximum: bool = False,
                    out: Optional[DeviceBuffer] = None, minmax: Optional[DeviceBuffer] = None,
                    refused: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """SumReduce / MaxReduce of `dim` on a contiguous (front, dim, back) int32 device tensor."""
        out = out or self.alloc(max(front * back, 1) * 4)
        self._check(self.lib.lib.lmn_eval_reduce(self.handle, 1 if maximum else 0, _addr(inp), front, dim, back, out.ptr,
                                                 _addr(minmax), _addr(refused)))
        return out

    def eval_lut(self, kind: int, inp: DeviceBuffer, n: int, lut_col1: DeviceBuffer, ranges: Sequence[Tuple[int, int]],
                 view: Optional[LmnView] = None, out: Optional[DeviceBuffer] = None,
                 minmax: Optional[DeviceBuffer] = None, refused: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """Sin / Exp2 / Log2: out = lut_col1[find_index(input)] over `ranges`; an input outside them is refused."""
        out = out or self.alloc(max(n, 1) * 4)
        self._check(self.lib.lib.lmn_eval_lut_ranges(self.handle, kind, _addr(inp), _ref(view), n, _addr(lut_col1),
                                                     _range_array(ranges), len(ranges), out.ptr, _addr(minmax), _addr(refused)))
        return out

    def tensor_range(self, buf: DeviceBuffer, n: int, minmax: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """The (min, max) of an int32 device buffer that no eval call produced, left in `minmax` (two int32 words)."""
        minmax = minmax or self.alloc(8)
        self._check(self.lib.lib.lmn_tensor_range(self.handle, _addr(buf), n, minmax.ptr))
        return minmax

    # ---- float tensors in and out (`CopyToStwo` / `CopyFromStwo`): the Inputs producers reading raw float bits of `dtype`
    # (F32 / F16 / BF16), converted in the launch that writes the rows, and the way back.  `src` is a DeviceBuffer or a
    # device address (an int: memory of another owner, a torch tensor's data_ptr()); nothing but tensor_to_float waits.
    def trace_inputs_float(self, dtype: int, src, n: int, node_id: int, num_consumers: int, is_final_output: bool = False,
                           rows: Optional[DeviceBuffer] = None, row_offset: int = 0, out: Optional[DeviceBuffer] = None,
                           sink: Optional["RowSink"] = None, refused: Optional[DeviceBuffer] = None):
        """`lmn_trace_inputs_float`, or with sink= `lmn_rows_append_inputs_float`: `trace_elementwise(Inputs)` on a float
        source.  Returns (rows DeviceBuffer or the sink, out DeviceBuffer)."""
        if rows is None and sink is None:
            rows = self.alloc((row_offset + n) * 7 * 4)
        out = out or self.alloc(max(n, 1) * 4)
        info = _node_info(node_id, (), num_consumers, is_final_output)
        if sink is not None:
            self._check(self.lib.lib.lmn_rows_append_inputs_float(self.handle, sink.handle, dtype, _addr(src), n, C.byref(info),
                                                                  out.ptr, _addr(refused)))
            return sink, out
        self._check(self.lib.lib.lmn_trace_inputs_float(self.handle, dtype, _addr(src), n, C.byref(info), rows.ptr, row_offset,
                                                        out.ptr))
        return rows, out

    def trace_many_inputs_float(self, dtype: int, src, n: int, n_members: int, node_id: int, num_consumers: int,
                                rows: DeviceBuffer, rows_stride: int, out: Optional[DeviceBuffer], out_stride: int,
                                src_stride: int = 0, is_final_output: bool = False, row_offset: int = 0,
                                refused: Optional[DeviceBuffer] = None):
        """`lmn_trace_many_inputs_float`: `trace_many_elementwise(Inputs)` on a float source; `src_stride` in elements of
        `dtype` (0: one source shared by all members)."""
        info = _node_info(node_id, (), num_consumers, is_final_output)
        self._check(self.lib.lib.lmn_trace_many_inputs_float(
            self.handle, dtype, _addr(src), src_stride, n, C.byref(info), n_members, _addr(rows), row_offset, rows_stride,
            _addr(out), out_stride, _addr(refused)))
        return rows, out

    def eval_inputs_float(self, dtype: int, src, n: int, out: Optional[DeviceBuffer] = None,
                          minmax: Optional[DeviceBuffer] = None, refused: Optional[DeviceBuffer] = None) -> DeviceBuffer:
        """`lmn_eval_inputs_float`: `eval_elementwise(Inputs)` on a float source."""
        out = out or self.alloc(max(n, 1) * 4)
        self._check(self.lib.lib.lmn_eval_inputs_float(self.handle, dtype, _addr(src), n, out.ptr, _addr(minmax), _addr(refused)))
        return out

    def tensor_to_float(self, dtype: int, src, n: int, dst=None):
        """`lmn_tensor_to_float`: n Fixed<12> values -> floats of `dtype` in `dst` (a DeviceBuffer, a device address, or
        None: a new DeviceBuffer).  Returns `dst` when the result is complete."""
        dst = dst if dst is not None else self.alloc(max(n, 1) * FLOAT_BYTES.get(dtype, 4))
        self._check(self.lib.lib.lmn_tensor_to_float(self.handle, dtype, _addr(src), n, _addr(dst)))
        return dst

    def _marshal_tables(self, tables, luts):
        """-> (LmnTable array, n, LmnSettings, objects that must stay alive while the library reads them)"""
        n = len(tables)
        arr = (LmnTable * max(n, 1))()
        keep = []
        for i, (kind, rows, n_rows) in enumerate(tables):
            arr[i].kind = kind
            arr[i].n_rows = n_rows
            if isinstance(rows, RowSink):
                if rows.table is None:
                    raise LuminairBackendError(ERR_INVALID_ARGUMENT, "a RowSink must be finished before it is proved")
                arr[i].flags = TABLE_COLS_ON_DEVICE
                arr[i].n_rows = rows.table.n_rows
                arr[i].rows = rows.table.rows
                keep.append(rows)
            elif isinstance(rows, DeviceBuffer):
                arr[i].flags = TABLE_ROWS_ON_DEVICE
                arr[i].rows = rows.ptr
            else:
                a = np.ascontiguousarray(rows, dtype=np.uint32)
                keep.append(a)
                arr[i].flags = 0
                arr[i].rows = a.ctypes.data
        luts = luts or {}
        lut_arr = (LmnLut * max(len(luts), 1))()
        for i, (name, (c0, c1)) in enumerate(luts.items()):
            c0 = np.ascontiguousarray(c0, dtype=np.uint32)
            c1 = np.ascontiguousarray(c1, dtype=np.uint32)
            if len(c0) != len(c1) or len(c0) & (len(c0) - 1) or len(c0) == 0:
                raise LuminairBackendError(-2, "LUT columns must have equal power-of-two lengths")
            keep += [c0, c1]
            lut_arr[i] = LmnLut(LUT_KINDS[name], len(c0).bit_length() - 1, c0.ctypes.data, c1.ctypes.data)
        settings = LmnSettings(0, len(luts), lut_arr)
        keep += [arr, lut_arr, settings]
        return arr, n, settings, keep

    def row_sink(self, kind: int, capacity_rows: int) -> RowSink:
        """`lmn_rows_open`: a table of `kind` to be filled with up to `capacity_rows` rows while they are produced - host
        rows (`push`), or a device producer's (the `sink=` argument of the `trace_*` methods)."""
        return RowSink(self, kind, capacity_rows)

    def prove_tables(self, tables: Sequence[Tuple[int, object, int]], luts=None,
                     prepared: Optional[PreparedSettings] = None) -> bytes:
        """tables: [(kind, rows, n_rows)] where rows is a uint32 ndarray (host), a DeviceBuffer or a finished RowSink;
        luts: {"sin" | "exp2" | "log2": (col0, col1)} preprocessed LUT columns (uint32, 2^k words each);
        prepared: a `PreparedSettings` in place of `luts` (`lmn_prove_prepared`): tree 0 is read from it."""
        arr, n, settings, _keep = self._marshal_tables(tables, None if prepared is not None else luts)
        out = C.POINTER(C.c_uint8)()
        out_len = C.c_size_t()
        if prepared is not None:
            self._check(self.lib.lib.lmn_prove_prepared(self.handle, arr, n, prepared._handle_for(self.lib), C.byref(out),
                                                        C.byref(out_len)))
        else:
            self._check(self.lib.lib.lmn_prove(self.handle, arr, n, C.byref(settings), C.byref(out), C.byref(out_len)))
        data = C.string_at(out, out_len.value)
        self.lib.lib.lmn_free(out)
        return data

    def check_trace(self, tables: Sequence[Tuple[int, object, int]], luts=None) -> TraceReport:
        """`lmn_trace_check` on what `prove_tables` takes: which rows break a local constraint, which logup tuples do not
        balance, which words are no canonical M31.  Nothing is committed or drawn; raises only for what `prove_tables`
        itself refuses before it starts (the text names the table)."""
        arr, n, settings, _keep = self._marshal_tables(tables, luts)
        rep = LmnTraceReport()
        self._check(self.lib.lib.lmn_trace_check(self.handle, arr, n, C.byref(settings), C.byref(rep)))
        return TraceReport.from_c(rep)

    def prove_submit(self, tables: Sequence[Tuple[int, object, int]], luts=None,
                     prepared: Optional[PreparedSettings] = None):
        """`lmn_prove_submit` (`lmn_prove_submit_prepared` with `prepared=`): start the proof on the context's own worker
        thread and return; collect it with `prove_wait()`.  One thread keeps N proofs in flight with N contexts."""
        arr, n, settings, keep = self._marshal_tables(tables, None if prepared is not None else luts)
        if prepared is not None:
            self._check(self.lib.lib.lmn_prove_submit_prepared(self.handle, arr, n, prepared._handle_for(self.lib)))
        else:
            self._check(self.lib.lib.lmn_prove_submit(self.handle, arr, n, C.byref(settings)))
        self._pending = keep          # borrowed by the library until prove_wait returns

    def prove_wait(self) -> bytes:
        out = C.POINTER(C.c_uint8)()
        out_len = C.c_size_t()
        try:
            self._check(self.lib.lib.lmn_prove_wait(self.handle, C.byref(out), C.byref(out_len)))
        finally:
            self._pending = None
        data = C.string_at(out, out_len.value)
        self.lib.lib.lmn_free(out)
        return data

    def set_profiling(self, enabled: bool):
        self._check(self.lib.lib.lmn_set_profiling(self.handle, 1 if enabled else 0))

    def timings(self) -> dict:
        t = LmnTimings()
        self._check(self.lib.lib.lmn_get_timings(self.handle, C.byref(t)))
        return t.as_dict()

    # ---- level-2 ops (host buffers)
    def interpolate(self, cols: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(cols, dtype=np.uint32).copy()
        ncols, n = a.shape
        self._check(self.lib.lib.lmn_op_interpolate(self.handle, a.ctypes.data, ncols, n.bit_length() - 1))
        return a

    def evaluate(self, coeffs: np.ndarray, log_domain: int) -> np.ndarray:
        a = np.ascontiguousarray(coeffs, dtype=np.uint32)
        ncols, n = a.shape
        out = np.empty((ncols, 1 << log_domain), dtype=np.uint32)
        self._check(self.lib.lib.lmn_op_evaluate(self.handle, a.ctypes.data, ncols, n.bit_length() - 1, log_domain,
                                                 out.ctypes.data))
        return out

    def evaluate_block(self, coeffs: np.ndarray, log_domain: int, log_blocks: int, block: int) -> np.ndarray:
        """Rows of block `block` (of 2^log_blocks equal row blocks) of the evaluation of (ncols, 2^k) coefficient
        columns on the 2^log_domain domain."""
        a = np.ascontiguousarray(coeffs, dtype=np.uint32)
        ncols, n = a.shape
        out = np.empty((ncols, 1 << (log_domain - log_blocks)), dtype=np.uint32)
        self._check(self.lib.lib.lmn_op_evaluate_block(self.handle, a.ctypes.data, ncols, n.bit_length() - 1, log_domain,
                                                       log_blocks, block, out.ctypes.data))
        return out

    def merkle_root(self, cols: List[np.ndarray]) -> bytes:
        arrs = [np.ascontiguousarray(c, dtype=np.uint32) for c in cols]
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        logs = (C.c_uint32 * max(len(arrs), 1))(*[len(a).bit_length() - 1 for a in arrs])
        root = (C.c_uint8 * 32)()
        self._check(self.lib.lib.lmn_op_merkle_root(self.handle, ptrs, logs, len(arrs), root))
        return bytes(root)

    def eval_at_point(self, coeffs: np.ndarray, point_xy: Sequence[int]) -> Tuple[int, int, int, int]:
        a = np.ascontiguousarray(coeffs, dtype=np.uint32)
        pt = (C.c_uint32 * 8)(*[int(v) for v in point_xy])
        out = (C.c_uint32 * 4)()
        self._check(self.lib.lib.lmn_op_eval_at_point(self.handle, a.ctypes.data, len(a).bit_length() - 1, pt, out))
        return tuple(int(v) for v in out)

    def accumulate_quotients(self, cols, samples, points, alpha) -> np.ndarray:
        """QuotientOps::accumulate_quotients for equal-size columns.  cols: [2^k uint32 arrays];
        samples: [(col index, point index, (4 words))] in (column, mask position) order; points: [(8 words)];
        alpha: 4 words.  Returns the 4 coordinate columns, shape (4, 2^k)."""
        keep = [np.ascontiguousarray(c, dtype=np.uint32) for c in cols]
        L = len(keep[0])
        ptrs = (C.c_void_p * len(keep))(*[c.ctypes.data for c in keep])
        sc = np.array([s[0] for s in samples], dtype=np.uint32)
        sp = np.array([s[1] for s in samples], dtype=np.uint32)
        sv = np.array([list(s[2]) for s in samples], dtype=np.uint32).reshape(-1)
        pts = np.array([list(p) for p in points], dtype=np.uint32).reshape(-1)
        al = (C.c_uint32 * 4)(*[int(v) for v in alpha])
        out = np.empty((4, L), dtype=np.uint32)
        self._check(self.lib.lib.lmn_op_accumulate_quotients(
            self.handle, L.bit_length() - 1, ptrs, len(keep), sc.ctypes.data, sp.ctypes.data, sv.ctypes.data, len(samples),
            pts.ctypes.data, len(points), al, out.ctypes.data))
        return out

    def fold_line(self, src: np.ndarray, alpha) -> np.ndarray:
        """FriOps::fold_line on 4 coordinate columns (4, 2^k) -> (4, 2^(k-1))."""
        a = np.ascontiguousarray(src, dtype=np.uint32)
        L = a.shape[1]
        out = np.empty((4, L // 2), dtype=np.uint32)
        al = (C.c_uint32 * 4)(*[int(v) for v in alpha])
        self._check(self.lib.lib.lmn_op_fold_line(self.handle, a.ctypes.data, L.bit_length() - 1, al, out.ctypes.data))
        return out

    def fold_circle_into_line(self, dst: np.ndarray, src: np.ndarray, alpha) -> np.ndarray:
        """FriOps::fold_circle_into_line: returns dst * alpha^2 + fold(src)."""
        a = np.ascontiguousarray(src, dtype=np.uint32)
        d = np.ascontiguousarray(dst, dtype=np.uint32).copy()
        al = (C.c_uint32 * 4)(*[int(v) for v in alpha])
        self._check(self.lib.lib.lmn_op_fold_circle_into_line(self.handle, d.ctypes.data, a.ctypes.data,
                                                              a.shape[1].bit_length() - 1, al))
        return d

    def grind(self, digest: bytes, pow_bits: int, variant: int = VARIANT_KAT) -> int:
        """GrindOps::grind on the context's GPU (lmn_ctx_grind): the nonce Library.grind finds on the host."""
        digest = bytes(digest)
        if len(digest) != 32:
            raise ValueError("digest must be 32 bytes")
        out = C.c_uint64()
        self._check(self.lib.lib.lmn_ctx_grind(self.handle, digest, pow_bits, variant, C.byref(out)))
        return int(out.value)

    def counter(self, which: int) -> int:
        """`lmn_ctx_counter` - 7: device grinds started, 8: host waits inside grind rounds, 9: proofs whose transcript was
        closed on the device, 10: those among them that went on grinding on the host's rounds."""
        return int(self.lib.lib.lmn_ctx_counter(self.handle, which))

    def grind_many(self, digests, pow_bits: int, variant: int = VARIANT_KAT) -> List[int]:
        """GrindOps::grind for several 32-byte channel digests ground together on the context's GPU (lmn_ctx_grind_many):
        the nonces Library.grind finds for each of them, in order."""
        digests = [bytes(d) for d in digests]
        if any(len(d) != 32 for d in digests):
            raise ValueError("every digest must be 32 bytes")
        out = (C.c_uint64 * max(1, len(digests)))()
        self._check(self.lib.lib.lmn_ctx_grind_many(self.handle, b"".join(digests), len(digests), pow_bits, variant, out))
        return [int(v) for v in out[:len(digests)]]

    def fft_selftest(self, log_size: int, ncols: int = 2):
        self._check(self.lib.lib.lmn_op_fft_selftest(self.handle, log_size, ncols))
