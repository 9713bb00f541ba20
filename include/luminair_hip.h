/* luminair_hip.h — C ABI of the MI355X-native LuminAIR prover backend.
 *
 * Drop-in boundary for the reference's
 *     pub fn prove(pie: LuminairPie, settings: CircuitSettings)
 *         -> Result<LuminairProof<Blake2sMerkleHasher>, LuminairError>
 * (/root/reference/crates/prover/src/prover.rs:28-31).  A Rust shim flattens
 * `pie.trace_tables` (crates/air/src/pie.rs:31-66) into `lmn_table`s and deserialises the returned
 * bincode bytes with `LuminairProof::from_bincode` (crates/prover/src/lib.rs:36-43).
 *
 * Plain pointers and sizes only; no C++/torch types.  One context per GPU (or several per GPU to keep
 * proofs in flight).  Different contexts are independent and run concurrently.  Calls on ONE context
 * from several threads are serialised by an internal lock (a context owns one HIP stream, one device
 * arena and one pinned staging buffer): safe, but they do not overlap - use one context per thread.
 * Device buffers handed to a context (LMN_TABLE_ROWS_ON_DEVICE, lmn_col handles) must not be written
 * by another context while a call that reads them is running.
 */
#ifndef LUMINAIR_HIP_H
#define LUMINAIR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this header.  It is bumped whenever a struct crossing the boundary changes size or layout (4: lmn_view
 * gained `offset`, 56 -> 64 bytes; 6: `protocol_variant` became a set of LMN_PV_* bits, LMN_VARIANT_PINNED 1 -> 0x1f).  A caller compares LMN_API_VERSION (what it was compiled against) with
 * lmn_abi_version() (what the loaded library implements) once at start-up; luminair_amd/backend.py does.
 * Structs passed in (lmn_view, lmn_node_info, lmn_settings, lmn_config) must be zero-initialised before their fields
 * are set, so that fields added by a later version read as 0. */
#define LMN_API_VERSION 6
uint32_t lmn_abi_version(void);

/* Error codes mirror LuminairError (/root/reference/crates/utils/src/lib.rs:5-34). */
#define LMN_OK 0
#define LMN_ERR_EMPTY_TRACE (-1)          /* TraceError::EmptyTrace (add/witness.rs:39-41)      */
#define LMN_ERR_MAIN_TRACE (-2)           /* MainTraceEvalGenError                                */
#define LMN_ERR_INTERACTION_TRACE (-3)    /* InteractionTraceEvalGenError                         */
#define LMN_ERR_CONSTRAINTS (-4)          /* ProverError(ConstraintsNotSatisfied)                 */
#define LMN_ERR_SERIALIZATION (-5)        /* SerializationError                                   */
#define LMN_ERR_INVALID_ARGUMENT (-6)     /* malformed table / unsupported component / config     */
#define LMN_ERR_OUT_OF_MEMORY (-7)
#define LMN_ERR_NO_DEVICE (-8)            /* no HIP device: the library never falls back to CPU   */
#define LMN_ERR_VERIFICATION (-9)         /* StwoVerifierError (verify only)                      */
#define LMN_ERR_INVALID_LOGUP (-10)       /* InvalidLogUp: claimed sums do not cancel (verify)    */
#define LMN_ERR_INTERNAL (-100)

/* TraceTable kinds, in `enum TraceTable` order (crates/air/src/pie.rs:31-66). */
#define LMN_KIND_ADD 0
#define LMN_KIND_MUL 1
#define LMN_KIND_RECIP 2
#define LMN_KIND_SIN 3
#define LMN_KIND_SIN_LOOKUP 4
#define LMN_KIND_SUM_REDUCE 5
#define LMN_KIND_MAX_REDUCE 6
#define LMN_KIND_SQRT 7
#define LMN_KIND_REM 8
#define LMN_KIND_EXP2 9
#define LMN_KIND_EXP2_LOOKUP 10
#define LMN_KIND_LOG2 11
#define LMN_KIND_LOG2_LOOKUP 12
#define LMN_KIND_LESS_THAN 13
#define LMN_KIND_RANGE_CHECK_LOOKUP 14
#define LMN_KIND_INPUTS 15
#define LMN_KIND_CONTIGUOUS 16

/* Protocol flags (SURVEY.md §8c "known deltas KAT-era -> pinned rev"; Appendix A.3).  The reference's only known-answer
 * proof (ui/demo/public/proof) was made by an older LuminAIR / stwo than the sources at HEAD; every observable
 * difference between the two is ONE independent bit of `lmn_config.protocol_variant` (since ABI version 6; before, the
 * field was an enum 0 / 1), so that a proof made by any build of the reference can be pinned by search
 * (tools/pin_variant.py tries every combination through lmn_verify_diagnose).  All bits clear = the KAT protocol, every
 * byte of which is pinned.  LMN_VARIANT_PINNED = what the reference at HEAD is believed to run; its transcript bits are
 * from memory of the un-vendored stwo ("parity unpinned").
 *
 * Transcript bits:
 *   CLAIM17        LuminairClaim / LuminairInteractionClaim have 17 Option slots (crates/air/src/lib.rs:30-48) instead of 8
 *   LUT_DRAWS4     LookupElements::draw draws sin, exp2, log2, range_check (lookups/mod.rs:44-51) instead of one LUT relation
 *   MIX_U64_HASHED mix_u64(v) = blake2s(digest || lo32 LE || hi32 LE) instead of the bare compression function on [lo, hi, 0..]
 *   DRAW_CTR_U32   draw = blake2s(digest || counter u32 LE || 0x00) instead of digest || counter zero-padded to 32 bytes
 *   POW_PREFIXED   proof of work = trailing zeros of blake2s(blake2s(0x12345678 LE || 12 zero bytes || digest || pow_bits LE)
 *                  || nonce u64 LE), nonce then mixed with mix_u64 - instead of the trailing zeros of the digest after
 *                  mix_u64(nonce)
 * Constraint-form bits (numerair's `eval_fixed_*` helpers are un-vendored; the KAT pins eval_fixed_add and the first
 * eval_fixed_mul constraint, and that eval_fixed_mul occupies two constraint slots):
 *   MUL_ONE_SLOT   eval_fixed_mul emits one constraint (KAT: two, the second contributing zero whenever rem == 0)
 *   RECIP_/SQRT_/REM_TWO_SLOTS  the helper emits a second (zero) slot as KAT-era eval_fixed_mul does (default: one)
 *   RECIP_/SQRT_/REM_NEG        the helper's constraint has the opposite sign: input*out + rem - scale^2,
 *                  out^2 + rem - input*scale, rhs*quotient + rem - lhs (default: scale^2 - (input*out + rem), ...) */
#define LMN_PV_CLAIM17 0x0001u
#define LMN_PV_LUT_DRAWS4 0x0002u
#define LMN_PV_MIX_U64_HASHED 0x0004u
#define LMN_PV_DRAW_CTR_U32 0x0008u
#define LMN_PV_POW_PREFIXED 0x0010u
#define LMN_PV_MUL_ONE_SLOT 0x0100u
#define LMN_PV_RECIP_TWO_SLOTS 0x0200u
#define LMN_PV_RECIP_NEG 0x0400u
#define LMN_PV_SQRT_TWO_SLOTS 0x0800u
#define LMN_PV_SQRT_NEG 0x1000u
#define LMN_PV_REM_TWO_SLOTS 0x2000u
#define LMN_PV_REM_NEG 0x4000u
#define LMN_PV_TRANSCRIPT_MASK 0x001fu
#define LMN_PV_FORMS_MASK 0x7f00u
#define LMN_PV_ALL (LMN_PV_TRANSCRIPT_MASK | LMN_PV_FORMS_MASK)
#define LMN_VARIANT_KAT 0u
#define LMN_VARIANT_PINNED LMN_PV_TRANSCRIPT_MASK

/* Replaces PcsConfig::default() (prover.rs:36) + DEFAULT_FP_SCALE (crates/air/src/lib.rs:23-24). */
typedef struct lmn_config {
  uint32_t pow_bits;         /* default 5 */
  uint32_t log_blowup;       /* default 1 (= blow-up 2, PcsConfig::default()); 1..3 accepted, sharded proofs included */
  uint32_t log_last_layer;   /* default 0 */
  uint32_t n_queries;        /* default 3 */
  uint32_t fp_scale;         /* default 12 */
  uint32_t protocol_variant; /* OR of LMN_PV_* bits: LMN_VARIANT_KAT (0), LMN_VARIANT_PINNED, or any combination */
} lmn_config;

#define LMN_TABLE_ROWS_ON_DEVICE 1u

/* One trace table of a LuminairPie: AoS rows, one u32 (canonical M31) per column in the
 * component's `Column::index()` order (e.g. crates/air/src/components/add/table.rs:191-211). */
typedef struct lmn_table {
  uint32_t kind;        /* LMN_KIND_* */
  uint32_t flags;       /* LMN_TABLE_ROWS_ON_DEVICE: `rows` is a device pointer (lmn_upload);
                           LMN_TABLE_COLS_ON_DEVICE: a finished row sink's columns (lmn_rows_finish, below) */
  uint64_t n_rows;
  const uint32_t* rows; /* n_rows * n_columns(kind) words */
} lmn_table;

/* CircuitSettings (crates/air/src/settings.rs).  `has_lookups` is a bit per `Lookups` field in
 * draw order (crates/air/src/components/lookups/mod.rs:20-51).  The 8-bit range-check LUT
 * (`lookups.range_check`, crates/graph/src/graph.rs:142-146) is generated by the library (row r holds
 * r, crates/air/src/preprocessed.rs:289-296).  The sin / exp2 / log2 LUT columns come from f64 math on
 * the reference's host side (`SinPreProcessed::gen_column`, preprocessed.rs:351-383 and siblings), so
 * the caller hands them over as data: `luts[i]` carries the two preprocessed columns
 * (`<name>_lut_0` = inputs, `<name>_lut_1` = outputs), 2^log_size canonical M31 words each, exactly
 * as `lookups_to_preprocessed_column` + `gen_column_simd` produce them.  A LUT is required iff its
 * lookup table (LMN_KIND_*_LOOKUP) is in the pie; the lookup table must have 2^log_size rows. */
#define LMN_LOOKUP_SIN 1u
#define LMN_LOOKUP_EXP2 2u
#define LMN_LOOKUP_LOG2 4u
#define LMN_LOOKUP_RANGE_CHECK 8u
#define LMN_LUT_SIN 0u
#define LMN_LUT_EXP2 1u
#define LMN_LUT_LOG2 2u
typedef struct lmn_lut {
  uint32_t kind;        /* LMN_LUT_* */
  uint32_t log_size;
  const uint32_t* col0; /* host pointers, borrowed for the duration of the call */
  const uint32_t* col1;
} lmn_lut;
typedef struct lmn_settings {
  uint32_t has_lookups; /* OR of LMN_LOOKUP_* (informational; checked against the pie's tables) */
  uint32_t n_luts;
  const lmn_lut* luts;
} lmn_settings;

/* `LookupLayout` (crates/air/src/preprocessed.rs:34-46): inclusive ranges of Fixed<12> values (numerair's
 * `Fixed` is a newtype over i64) and the LUT's log size.  lmn_lut_log_size restates `LookupLayout::new` /
 * `calculate_log_size` (crates/air/src/utils.rs:22-27: the value count rounded up to a power of two, at least 16
 * rows).  lmn_lut_from_ranges restates `SinPreProcessed::gen_column` (preprocessed.rs:351-383; Exp2 :434-466, Log2
 * :517-549): all values of the ranges, sorted and de-duplicated, go to col0 as M31 words and f(value / 2^12) * 2^12
 * rounded to the nearest integer (ties away from zero, `f64::round`; numerair's `Fixed::from_f64` is un-vendored:
 * unpinned) to col1; the remaining rows are zero.  Host code (f64 libm, like the reference); needs no context.
 * col0_out / col1_out: 2^log_size words each.  Returns LMN_ERR_INVALID_ARGUMENT for an empty / inverted range, a
 * value outside (-2^30, 2^30), a log2 argument <= 0, or a log_size too small for the values. */
typedef struct lmn_range {
  int64_t lo, hi; /* Range(Fixed, Fixed), inclusive */
} lmn_range;
int lmn_lut_log_size(const lmn_range* ranges, uint32_t n_ranges, uint32_t* log_size_out);
int lmn_lut_from_ranges(uint32_t lut_kind /* LMN_LUT_* */, const lmn_range* ranges, uint32_t n_ranges, uint32_t log_size,
                        uint32_t* col0_out, uint32_t* col1_out);
/* The same with the f64 -> Fixed rounding stated (since ABI version 6; `Fixed::from_f64` is in the un-vendored numerair,
 * so the rule is one of the axes tools/pin_variant.py searches when it is given the reference's preprocessed root):
 * HALF_AWAY = `f64::round` (what lmn_lut_from_ranges uses), HALF_EVEN = round-half-to-even, TRUNC = `as i64` (towards
 * zero), FLOOR = `f64::floor`. */
#define LMN_ROUND_HALF_AWAY 0u
#define LMN_ROUND_HALF_EVEN 1u
#define LMN_ROUND_TRUNC 2u
#define LMN_ROUND_FLOOR 3u
int lmn_lut_from_ranges_r(uint32_t lut_kind, const lmn_range* ranges, uint32_t n_ranges, uint32_t log_size, uint32_t rounding,
                          uint32_t* col0_out, uint32_t* col1_out);

typedef struct lmn_ctx lmn_ctx;

/* Per-stage timings of the last lmn_prove call, milliseconds (HIP events on the prover stream). */
typedef struct lmn_timings {
  float total_ms;
  float transpose_ms, main_commit_ms, logup_ms, interaction_commit_ms, composition_ms, composition_commit_ms,
      oods_ms, quotients_ms, fri_ms, decommit_ms;
  float fft_ms;     /* all circle (i)FFT passes */
  float merkle_ms;  /* all Blake2s Merkle layer kernels */
  uint64_t fft_bytes;    /* algorithmic bytes moved by those FFT launches (8 B per element per transform) */
  uint64_t merkle_bytes; /* algorithmic bytes of the Merkle launches */
  uint32_t fft_launches, merkle_launches;
  uint64_t fft_butterflies;      /* M31 butterflies (1 mul + 1 add + 1 sub) executed by those FFT launches */
  uint64_t merkle_compressions;  /* Blake2s compression-function calls executed by the Merkle launches */
  /* the k_merkle_fused launches alone (the dominant kernel; excludes k_merkle_small / k_fri_tail) */
  float merkle_fused_ms;
  uint32_t merkle_fused_launches;
  uint64_t merkle_fused_bytes, merkle_fused_compressions;
  /* sharded proofs (since ABI version 5): bytes this rank RECEIVED from other ranks through all_to_all / all_gather */
  uint64_t shard_a2a_bytes, shard_gather_bytes;
  uint32_t shard_a2a_calls, shard_gather_calls;
} lmn_timings;

const char* lmn_strerror(int code);
const char* lmn_last_error(const lmn_ctx* ctx);
void lmn_default_config(lmn_config* cfg);
uint32_t lmn_kind_columns(uint32_t kind); /* 0 if the kind is not supported */
/* The rest of a component's boundary data, for bindings and for tests/test_reference_layout.py: the number of logup
 * relations (`TraceColumn::count().1`, e.g. add/table.rs:214-216: lmn_kind_relations, declared with level 2 below) and the padding row `write_trace` appends up to
 * the next power of two (`*TraceTableRow::padding()`, e.g. add/table.rs:40-58; less_than/table.rs:47-72):
 * out receives lmn_kind_columns(kind) words. */
int lmn_kind_padding_row(uint32_t kind, uint32_t* out);

int lmn_ctx_create(int device, const lmn_config* cfg, lmn_ctx** out);
void lmn_ctx_destroy(lmn_ctx* ctx);

/* Replaces prove(pie, settings).  On success *proof_bincode holds `LuminairProof::to_bincode()`
 * bytes owned by the library until lmn_free. */
int lmn_prove(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_settings* settings,
              uint8_t** proof_bincode, size_t* proof_len);
void lmn_free(void* p);
/* Asynchronous form: the reference's callers are single-threaded (prover.rs:28 is a plain function call), and one
 * MI355X wants about eight proofs in flight.  lmn_prove_submit hands the proof to the context's
 * own worker thread and returns; lmn_prove_wait blocks until it is done and returns what lmn_prove would have.  One
 * outstanding submission per context; `tables`, the row buffers and `settings` are borrowed until lmn_prove_wait
 * returns.  A caller keeps N proofs in flight from one thread with N contexts: submit on each, then wait on each. */
int lmn_prove_submit(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_settings* settings);
int lmn_prove_wait(lmn_ctx* ctx, uint8_t** proof_bincode, size_t* proof_len);

/* ---- Settings prepared once.  CircuitSettings are fixed per model, and so is everything about the preprocessed tree
 * (tree 0) of its proofs: the LUT columns, the 8-bit range-check column, their coefficients, their low-degree extension,
 * the Merkle layers and the root.  lmn_prove redoes that work for every proof - a host loop over the LUT words, an
 * upload, the transforms, the tree and a host wait for a root that is the same bytes every time.  lmn_settings_prepare
 * does it ONCE, on a stream of its own, and returns after waiting; the object it hands out is immutable, lives in device
 * memory of its own (no context's arena) and is shared read-only by every context, batch object and thread of its device
 * that proves with it.  The proofs are byte-identical to lmn_prove's.
 *  - lookups: the LMN_LOOKUP_* bits of the lookup components the pies WILL contain (LMN_LOOKUP_RANGE_CHECK when the
 *    graph has LessThan).  settings->luts must carry the columns of every sin / exp2 / log2 bit set (a LUT whose bit is
 *    clear is validated and left out); settings->has_lookups is not read.  lookups == 0 is valid (settings may then be
 *    NULL): the empty tree, root = blake2s("").
 *  - The LUT words are checked on the device (canonical M31) and the range-check column is written there; the caller's
 *    LUT arrays are free again as soon as the call returns.
 *  - LMN_ERR_INVALID_ARGUMENT (text: lmn_last_error(NULL) for prepare, the context's / batch's for the prove entries):
 *    a non-canonical LUT word (of a LUT in use), a lookup bit without its LUT, a duplicate LUT, a null column, a LUT of
 *    fewer than 2^4 rows or too large for the prover, unknown bits; at prove time a pie whose lookup tables are not
 *    exactly `lookups`, a lookup table whose padded size is not its LUT's, a context whose log_blowup or device differs
 *    from the object's, a sharded context (tree 0 has another layout there).  The context stays usable.
 *  - Lifetime: the library holds a reference from the start of a prove / submit / batch call until its proof has been
 *    returned (lmn_prove_wait for submits); lmn_prepared_destroy drops the caller's reference only, at any time.
 *  - lmn_prepared_root: the root of tree 0 = proof.commitments[0] of every proof made with the object. */
typedef struct lmn_prepared lmn_prepared;
int lmn_settings_prepare(int device, const lmn_config* cfg, const lmn_settings* settings, uint32_t lookups,
                         lmn_prepared** out);
int lmn_prepared_root(const lmn_prepared* p, uint8_t root_out[32]);
uint32_t lmn_prepared_lookups(const lmn_prepared* p);
void lmn_prepared_destroy(lmn_prepared* p);
int lmn_prove_prepared(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_prepared* prepared,
                       uint8_t** proof_bincode, size_t* proof_len);
/* collected with lmn_prove_wait, like lmn_prove_submit's */
int lmn_prove_submit_prepared(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_prepared* prepared);
/* The lock-step batch form (luminair_hip_batch.h: `batch`, n, tables, proofs, lens, rcs as lmn_batch_prove takes them) with the
 * settings prepared once by the batch library: every member reads the one prepared tree 0, so no member checks or uploads a
 * LUT, transforms or commits tree 0, or waits for its root - fewer launches, host waits and transfers per batch
 * (lmn_batch_counter 0, 1, 2 + 3), the same proof bytes.  Declared here, next to the other prepared entries, and exported by
 * both libraries so that one binding covers them; batch objects exist in libluminair_hip_batch.so alone, so the main
 * library answers LMN_ERR_INVALID_ARGUMENT. */
typedef struct lmn_batch lmn_batch;
int lmn_batch_prove_prepared(lmn_batch* batch, uint32_t n, const lmn_table* const* tables, size_t n_tables,
                             const lmn_prepared* prepared, uint8_t** proofs, size_t* lens, int* rcs);

/* Per-stage / per-kernel HIP-event timing is off by default (every event record costs a few
 * microseconds between dependent kernels); enable it for the proofs whose lmn_timings you want. */
int lmn_set_profiling(lmn_ctx* ctx, int enabled);
int lmn_get_timings(const lmn_ctx* ctx, lmn_timings* out);

/* Replaces `verify(proof, settings)` (/root/reference/crates/verifiers/rust/src/verifier.rs:21-143).
 * Host-only (the reference verifier is CPU code too); needs no context and no GPU.  Returns LMN_OK,
 * LMN_ERR_INVALID_LOGUP, LMN_ERR_VERIFICATION or LMN_ERR_SERIALIZATION; the message of the last
 * failure on this thread is available through lmn_last_error(NULL). */
int lmn_verify(const uint8_t* proof_bincode, size_t proof_len, const lmn_settings* settings, uint32_t protocol_variant /* LMN_PV_* bits */);
/* lmn_verify checks the proof against PcsConfig::default() (pow 5, blow-up 2, 3 queries, last layer degree 0), as
 * verifier.rs:36 does; a deployment with other parameters states them here.  The security parameters are the
 * verifier's: a proof whose embedded config differs from `expected` is rejected (LMN_ERR_VERIFICATION).  Field
 * elements that are not canonical M31 words, Option tags other than 0/1 and claim log sizes above 26 are
 * LMN_ERR_SERIALIZATION.  `settings` may be NULL; when given, `has_lookups` (if non-zero) and every LUT's
 * log_size must agree with the lookup components in the proof's claim (the LUT columns themselves are not read:
 * like the reference, the verifier takes the preprocessed root from the proof). */
int lmn_verify_with_config(const uint8_t* proof_bincode, size_t proof_len, const lmn_settings* settings,
                           const lmn_config* expected);

/* lmn_verify that does not stop at the first failed check (since ABI version 6): the replay goes on as far as the
 * proof's shape allows and reports which checks passed.  The checks depend on different parts of the protocol, which
 * is what makes a proof from an unknown build of the reference diagnosable (tools/pin_variant.py runs this for every
 * combination of LMN_PV_* bits):
 *   PARSE          the bytes deserialize under the claim layout (CLAIM17) - LMN_ERR_SERIALIZATION otherwise
 *   SHAPE          tree / sampled-value / FRI-layer counts are what the claim implies
 *   LOGUP_SUM      the claimed sums cancel (no transcript dependence)
 *   OODS           composition identity at the OODS point: transcript up to the OODS draw (claim mix, relation draws,
 *                  composition randomness) AND every constraint form of the components present
 *   POW            proof-of-work nonce: the whole transcript up to the nonce; pow_bits bits of evidence only
 *   TREE_DECOMMIT  the four trace trees' decommitments at the drawn query positions: the whole transcript including
 *                  the query draw, and the Merkle hashing; independent of the constraint forms
 *   FRI_DECOMMIT   the FRI layers' decommitments (same dependence)
 *   FRI_FOLDS      FRI quotients from sampled + queried values fold to the last layer: OODS point, quotient and fold
 *                  randomness; independent of the constraint forms
 * `steps` records the channel digest after every mix of the replay, in order (a maintainer prints the same digests from
 * the Rust prover to find the first diverging step).  Returns LMN_OK when the replay ran to the end (whatever the checks
 * said), else the error that stopped it (its text in `first_failure` if no check had failed before).  `report` is
 * always filled as far as the replay got. */
#define LMN_CHECK_PARSE 0x0001u
#define LMN_CHECK_SHAPE 0x0002u
#define LMN_CHECK_LOGUP_SUM 0x0004u
#define LMN_CHECK_OODS 0x0008u
#define LMN_CHECK_POW 0x0010u
#define LMN_CHECK_TREE_DECOMMIT 0x0020u
#define LMN_CHECK_FRI_DECOMMIT 0x0040u
#define LMN_CHECK_FRI_FOLDS 0x0080u
#define LMN_CHECK_ALL 0x00ffu
#define LMN_STEP_ROOT_PREPROCESSED 0u /* mix_root(commitments[0]), prover.rs:59 */
#define LMN_STEP_CLAIM 1u             /* LuminairClaim::mix_into, crates/air/src/lib.rs:52-104 */
#define LMN_STEP_ROOT_MAIN 2u         /* prover.rs:179 */
#define LMN_STEP_INTERACTION_CLAIM 3u /* mix_felts(claimed_sum) per component, components/mod.rs:209-211 */
#define LMN_STEP_ROOT_INTERACTION 4u  /* prover.rs:298 */
#define LMN_STEP_ROOT_COMPOSITION 5u  /* inside stwo::prover::prove, prover.rs:312 */
#define LMN_STEP_SAMPLED_VALUES 6u
#define LMN_STEP_FRI_FIRST_LAYER 7u
#define LMN_STEP_FRI_INNER_LAYER 8u   /* index = layer number */
#define LMN_STEP_FRI_LAST_LAYER 9u
#define LMN_STEP_POW_NONCE 10u
#define LMN_MAX_TRANSCRIPT_STEPS 48
typedef struct lmn_transcript_step {
  uint32_t step;  /* LMN_STEP_* */
  uint32_t index;
  uint8_t digest[32];
} lmn_transcript_step;
typedef struct lmn_verify_report {
  uint32_t checks_run;    /* LMN_CHECK_* bits of the checks the replay reached */
  uint32_t checks_passed; /* ... that held */
  uint32_t checks_failed; /* ... that did not (a check with several parts fails if any part does) */
  uint32_t n_steps;
  lmn_transcript_step steps[LMN_MAX_TRANSCRIPT_STEPS];
  char first_failure[128]; /* text of the first failed check or of the error that stopped the replay */
} lmn_verify_report;
int lmn_verify_diagnose(const uint8_t* proof_bincode, size_t proof_len, const lmn_settings* settings,
                        const lmn_config* expected, lmn_verify_report* report);

/* Verifies n proofs in one call: the front of lmn_verify_with_config (parse, config and shape checks, the settings
 * cross-check, logup sum, transcript replay, OODS identity, last-layer shape, proof of work, query draw) runs on the host per
 * proof, the back (the four trace-tree decommitments, the FRI quotients at the queried positions, the FRI layers: 77 % to
 * 94 % of lmn_verify's time) on the device for all proofs that passed the front.
 *  - Returns LMN_OK when every proof was judged, whatever the verdicts; otherwise the error that stopped the call (null
 *    arguments with n > 0, a bad `expected`, a sharded context, out of memory, a device error), its text in
 *    lmn_last_error(ctx).  n = 0 returns LMN_OK and touches nothing.  After LMN_OK, lmn_last_error(ctx) carries the text
 *    of the first rejection in index order, if there was one.
 *  - results[i].rc is what lmn_verify_with_config(proofs[i], lens[i], settings, expected) returns.
 *  - stage 0: decided by the front; checks_failed holds the bit of the check that failed (a structural stop:
 *    LMN_CHECK_SHAPE; bytes that do not parse: LMN_CHECK_PARSE).
 *    stage 1: decided by the device stage; a rejection is LMN_ERR_VERIFICATION and checks_failed holds
 *    lmn_verify_diagnose's TREE_DECOMMIT | FRI_DECOMMIT | FRI_FOLDS bits (nothing behind a failed tree decommitment is
 *    looked at), or LMN_CHECK_SHAPE for a structural stop of that region (a witness list too short or too long, the
 *    queried-values shape, a degenerate denominator).
 *    stage 2: judged by the host's back half, with the same verdict - a proof the device stage does not take is never
 *    refused: more than 128 distinct query positions, more than 8 column sizes or 36 trees, column sizes that no FRI
 *    layer consumes, more than 4 MiB of lists and scratch, or a claim beyond the 4 different claims (kinds present and
 *    their log sizes) that one call buckets.
 *  - Proofs are staged in chunks of at most 256 proofs or 16 MiB: one transfer in, two launches per claim, one transfer
 *    out and one host wait per chunk.
 *  - Any unsharded context; in the batch library outside a batch.  The context's arena is not used.
 *  - lmn_ctx_counter 16: proofs judged by the device stage, 17: stage-2 proofs, 18: verify launches, 19: host waits. */
struct lmn_verify_result {
  int32_t rc;             /* what lmn_verify_with_config returns for these bytes */
  uint32_t checks_failed; /* LMN_CHECK_* bits */
  uint32_t stage;         /* 0: decided on the host before the device stage, 1: decided by the device stage,
                             2: judged entirely by the host verifier (fallback) */
};
typedef struct lmn_verify_result lmn_verify_result;
int lmn_verify_many(lmn_ctx* ctx, const uint8_t* const* proofs, const size_t* lens, uint32_t n,
                    const lmn_settings* settings, const lmn_config* expected /* NULL: PcsConfig::default(), variant 0 */,
                    lmn_verify_result* results /* n */);

/* Page-locked host memory for tables handed over as HOST buffers (`lmn_table.rows` without LMN_TABLE_ROWS_ON_DEVICE -
 * the reference's own calling convention: `prove(pie, settings)` takes the pie by value in host memory,
 * /root/reference/crates/prover/src/prover.rs:28-31,70).  Rows in ordinary pageable memory are copied through the
 * runtime's staging buffers (≈ 20 - 28 GB/s, the calling thread blocked meanwhile); rows in page-locked memory are
 * fetched by the GPU's DMA engines directly at PCIe rate and the call returns at once.  The binding's `flatten`
 *  can write the pie's rows straight into an `lmn_host_alloc` buffer, or page-lock the vectors it
 * already owns with `lmn_host_register`.  No context needed; the memory is usable by every context of the process. */
int lmn_host_alloc(size_t bytes, void** host_out);
void lmn_host_free(void* host);
int lmn_host_register(void* host, size_t bytes);   /* page-lock [host, host + bytes) in place */
int lmn_host_unregister(void* host);

/* Device residency helpers for callers that keep trace tables in HBM. */
int lmn_upload(lmn_ctx* ctx, const void* host, size_t bytes, void** device_out);
void lmn_device_free(lmn_ctx* ctx, void* device_ptr);

int lmn_device_alloc(lmn_ctx* ctx, size_t bytes, void** device_out);
int lmn_download(lmn_ctx* ctx, const void* device, void* host, size_t bytes);
int lmn_upload_to(lmn_ctx* ctx, const void* host, size_t bytes, void* device_dst); /* into an existing allocation */
/* device-to-device copy enqueued on the context's stream (ordered with every other call on this context; returns
 * without waiting) */
int lmn_device_copy(lmn_ctx* ctx, void* device_dst, const void* device_src, size_t bytes);

/* ---- The step before the path: `LuminairOperator::process_trace` of the
 * elementwise primitives on device-resident tensors (crates/graph/src/op/prim.rs:967-1013 Add,
 * :1090-1139 Mul, :388-431 Recip): executes the fixed-point op and fills the node's trace-table rows in
 * HBM, ready for lmn_prove with LMN_TABLE_ROWS_ON_DEVICE.  Tensors are contiguous int32 arrays of
 * Fixed<12> values; Mul: out = floor(lhs*rhs / 4096), rem = lhs*rhs - out*4096; Recip (input > 0):
 * out = floor(4096^2 / input), rem = 4096^2 - input*out (numerair's sign conventions are unpinned,
 * DESIGN.md §2).  out_mult = is_final_output ? 0 : num_consumers; input_mults are -1 at HEAD
 * (prim.rs:1005-1006), 0 for graph initializers in the KAT era. */
typedef struct lmn_node_info {
  uint32_t node_id;
  uint32_t input_ids[2];
  uint32_t num_consumers;
  uint32_t is_final_output;
  int32_t input_mults[2];
} lmn_node_info;
/* kind: LMN_KIND_ADD | LMN_KIND_MUL | LMN_KIND_REM (prim.rs:1323-1421, lhs >= 0, rhs > 0) | unary (rhs_dev ignored):
 * LMN_KIND_RECIP | LMN_KIND_SQRT (prim.rs:573-660) | LMN_KIND_CONTIGUOUS (prim.rs:229-301) | LMN_KIND_INPUTS
 * (`CopyToStwo`, prim.rs:52-88: rows of a graph input, multiplicity = num_consumers).  rows_dev receives
 * n * lmn_kind_columns(kind) words starting at row `row_offset` of the node's table (several nodes of one
 * kind share a table: prim.rs appends); out_dev (may be NULL) receives the n output values.
 *
 * The producers' contract (every lmn_trace_* call; the rows go to lmn_prove unchecked otherwise):
 *  - Value range: a Fixed<12> tensor value lies in [-(2^30-1), 2^30-1], the signed M31 range (the one
 *    lmn_trace_lut_ranges enforces for LUT ranges).  It holds for every operand a producer reads and every output
 *    value it writes; only the running sums inside SumReduce may leave it.
 *  - Row words: every row word is the exact integer value reduced mod P, canonical, equal to Python's `v % P` for the
 *    exact int64 intermediate - running sums, rem, quo and diff included.
 *  - Preconditions: Recip needs input > 0, Sqrt input >= 0, Rem lhs >= 0 and rhs > 0.
 *  - An element outside the contract gets the non-canonical word P in its row's output-value column (Add / Mul / Rem /
 *    LessThan out or rem, Recip / Sqrt / Contiguous out, Inputs val, SumReduce / MaxReduce out - the group result on
 *    its last step, or the row of an input outside the range - and Sin / Exp2 / Log2 out), the other derived words of
 *    that row (Mul / Recip / Sqrt rem, Rem quo, LessThan diff, borrow and limbs) are 0, its operand words stay exact,
 *    and 0 goes to the output tensor; LessThan adds nothing to the range-check multiplicities for it.  lmn_prove of a
 *    table holding such a row fails with LMN_ERR_INVALID_ARGUMENT (non-canonical word).  The other elements of the
 *    launch keep their exact rows, no call waits for the device to find out, and no lane does value-dependent work
 *    for a refused element (no division by zero, no square root of a negative number). */
int lmn_trace_elementwise(lmn_ctx* ctx, uint32_t kind, const int32_t* lhs_dev, const int32_t* rhs_dev, uint64_t n,
                          const lmn_node_info* info, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev);

/* Strided view of a device tensor, the part of luminal's ShapeTracker the elementwise ops need: element
 * (i_0 .. i_{ndim-1}) of the op's (row-major) output shape reads tensor[offset + sum_k i_k * strides[k]]; an
 * expanded ("fake") dimension has stride 0, a slice a non-zero offset.  NULL = contiguous. */
typedef struct lmn_view {
  uint32_t ndim; /* 1..4 */
  uint32_t shape[4];
  int64_t strides[4]; /* in elements */
  int64_t offset;     /* in elements: first element of the view (slices) */
} lmn_view;
/* lmn_trace_elementwise with a view per operand (crates/graph/src/op/prim.rs `get_index` with the
 * ShapeTracker's index expression); the product of view shapes must equal n. */
int lmn_trace_elementwise_v(lmn_ctx* ctx, uint32_t kind, const int32_t* lhs_dev, const lmn_view* lhs_view,
                            const int32_t* rhs_dev, const lmn_view* rhs_view, uint64_t n, const lmn_node_info* info,
                            uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev);

/* `LuminairContiguous::process_trace` in the reference's own row rule (crates/graph/src/op/prim.rs:229-301): the
 * reference zips the input BUFFER with the output, so row idx carries the idx-th buffer element (consumed with
 * multiplicity -1; zero past the buffer's end) and the idx-th output element (the view's element; past the output's
 * end the index wraps - luminal's own out-of-range index expression is un-vendored, unpinned), max(in_size, out_size)
 * rows, is_last_idx on the buffer's last element.  This is the rule under which a slice or permutation of the input
 * balances its logup (crates/graph/src/tests/ops.rs test_contiguous).  `view` NULL = identity.  For a view with
 * expanded dimensions (out_size > in_size) the reference's rule cannot balance; use lmn_trace_elementwise_v
 * (LMN_KIND_CONTIGUOUS), which consumes the view's element per output row. */
int lmn_trace_contiguous(lmn_ctx* ctx, const int32_t* input_dev, uint64_t in_size, const lmn_view* view, uint64_t out_size,
                         const lmn_node_info* info, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev);

/* `process_trace` of the LUT ops Sin / Exp2 / Log2 (prim.rs:663-760 and siblings; rows per
 * crates/air/src/components/sin/table.rs): out = LUT[input] for a LUT that enumerates the single value range
 * lo..lo+lut_len-1 (`lut_col1_dev` = its preprocessed output column, M31 words), one lookup per row
 * (lookup multiplicity 1), and the LUT's multiplicity column `mult_dev[input - lo]` incremented per use -
 * `mult_dev` (2^k words, zero-initialised by the caller) IS the SinLookup / Exp2Lookup / Log2Lookup trace table.
 * kind: LMN_KIND_SIN | LMN_KIND_EXP2 | LMN_KIND_LOG2.  Inputs outside the range fail with LMN_ERR_INVALID_ARGUMENT. */
int lmn_trace_lut(lmn_ctx* ctx, uint32_t kind, const int32_t* input_dev, const lmn_view* view, uint64_t n,
                  const lmn_node_info* info, const uint32_t* lut_col1_dev, int32_t lo, uint32_t lut_len,
                  uint32_t* mult_dev, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev);
/* The same for a LUT that enumerates SEVERAL value ranges - what `gen_circuit_settings` produces when a graph applies
 * the function on disjoint input ranges (one padded range per op, `coalesce_ranges`, crates/graph/src/graph.rs:61-159,
 * 665-691): `ranges` ascending and disjoint (at most 16), LUT row of a value = `LookupLayout::find_index`
 * (crates/air/src/preprocessed.rs:60-77); `lut_col1_dev` / `mult_dev` are the columns lmn_lut_from_ranges lays out
 * for the same ranges. */
int lmn_trace_lut_ranges(lmn_ctx* ctx, uint32_t kind, const int32_t* input_dev, const lmn_view* view, uint64_t n,
                         const lmn_node_info* info, const uint32_t* lut_col1_dev, const lmn_range* ranges, uint32_t n_ranges,
                         uint32_t* mult_dev, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev);

/* `LuminairLessThan::process_trace` (prim.rs:1203-1295): out = 1.0 iff lhs < rhs, diff = rhs - lhs (+ P with
 * borrow) split into four 8-bit limbs; `range_check_mult_dev` (256 words, zero-initialised by the caller) is the
 * RangeCheckLookup trace table and is incremented once per limb. */
int lmn_trace_less_than(lmn_ctx* ctx, const int32_t* lhs_dev, const lmn_view* lhs_view, const int32_t* rhs_dev,
                        const lmn_view* rhs_view, uint64_t n, const lmn_node_info* info, uint32_t* range_check_mult_dev,
                        uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev);
/* `LuminairMaxReduce::process_trace` (prim.rs:1591-1734): as lmn_trace_sum_reduce with the running maximum. */
int lmn_trace_max_reduce(lmn_ctx* ctx, const int32_t* input_dev, uint64_t front, uint64_t dim, uint64_t back,
                         const lmn_node_info* info, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev);

/* `LuminairSumReduce::process_trace` (prim.rs:1450-1565) on a contiguous device tensor of shape
 * (front, dim, back), reducing `dim`: front*back*dim rows in (i, j, k) order with the running sums
 * acc / next_acc; out_dev (may be NULL) receives the front*back sums. */
int lmn_trace_sum_reduce(lmn_ctx* ctx, const int32_t* input_dev, uint64_t front, uint64_t dim, uint64_t back,
                         const lmn_node_info* info, uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev);

/* ---- The many-member producers: one call - one launch - fills the rows of ONE graph node for n_members pies of one shape, the
 * producers in front of a lock-step batch, which proves the same graph on many input sets (luminair_hip_batch.h; with the
 * single forms above that costs one call per node per pie).  Every call takes the arguments of its single form, plus n_members, one
 * member stride per device pointer and a trailing refused_dev; member m works on `base + m * member_stride`.  `info`, the
 * views, the sizes and `row_offset` are common to all members (a lock-step batch needs identical shapes anyway).
 *  - Strides: operands and output tensors in elements, rows_dev in ROWS of the kind (so a member's table holds
 *    rows_member_stride rows), multiplicity tables in words.
 *  - Shared operands: an operand stride of 0 means that all members read the same operand (weights, constants).  Rows are
 *    still written per member: the Inputs rows of a shared weight tensor appear in every pie.
 *  - Shared output tensors: out_member_stride == 0 is accepted only when every operand stride the kind reads is 0; out_dev is
 *    then ONE tensor, stored by member 0 alone (no racing stores).  Any other out stride of 0 is LMN_ERR_INVALID_ARGUMENT.
 *    out_dev may be NULL as in the single forms (its stride is then ignored).
 *  - Refused before any launch, with the argument named by lmn_last_error: n_members > LMN_TRACE_MANY_MAX; a
 *    rows_member_stride smaller than row_offset + the node's row count; an out stride smaller than the output's element
 *    count (unless it is 0 as above); a multiplicity stride smaller than the table (256 words for the range check, the LUT
 *    rows the ranges enumerate for a LUT), 0 included; null pointers where the single form refuses them; and the single
 *    forms' own shape errors with their codes (a view whose shape product is not n, n = 0: LMN_ERR_EMPTY_TRACE, ...).
 *  - n_members == 0 is LMN_OK and touches nothing (as lmn_ctx_grind_many).
 *  - The producers' contract (lmn_trace_elementwise above) holds per element, unchanged: a refused element gets the word P in
 *    its row's output-value column, zeros in the other derived words, 0 in the output tensor, and adds nothing to any
 *    multiplicity table.  Here a Sin / Exp2 / Log2 input outside every range is such a refused element too - marked and
 *    counted, the call neither fails nor waits (as lmn_eval_lut_ranges; the single lmn_trace_lut* forms wait once per call to
 *    report it, and keep doing so).
 *  - refused_dev (n_members uint32_t counters on the device, may be NULL): counter m grows by member m's refused elements.
 *    Never reset by a call: one set of counters is accumulated over a whole graph and downloaded once.
 *  - No call waits for the device; all are ordered on the context's stream with every other call of that context. */
#define LMN_TRACE_MANY_MAX 1024 /* the largest n_members */
/* the kinds of lmn_trace_elementwise_v; LMN_KIND_LESS_THAN too, with range_check_mult_dev (256 zero-initialised words per
 * member, ignored for the other kinds) as in lmn_trace_less_than */
int lmn_trace_many_elementwise_v(lmn_ctx* ctx, uint32_t kind, const int32_t* lhs_dev, const lmn_view* lhs_view,
                                 uint64_t lhs_member_stride, const int32_t* rhs_dev, const lmn_view* rhs_view,
                                 uint64_t rhs_member_stride, uint64_t n, const lmn_node_info* info, uint32_t n_members,
                                 uint32_t* rows_dev, uint64_t row_offset, uint64_t rows_member_stride, int32_t* out_dev,
                                 uint64_t out_member_stride, uint32_t* range_check_mult_dev,
                                 uint64_t range_check_mult_member_stride, uint32_t* refused_dev);
/* the reference's buffer rule, as lmn_trace_contiguous: max(in_size, out_size) rows per member */
int lmn_trace_many_contiguous(lmn_ctx* ctx, const int32_t* input_dev, uint64_t input_member_stride, uint64_t in_size,
                              const lmn_view* view, uint64_t out_size, const lmn_node_info* info, uint32_t n_members,
                              uint32_t* rows_dev, uint64_t row_offset, uint64_t rows_member_stride, int32_t* out_dev,
                              uint64_t out_member_stride, uint32_t* refused_dev);
/* lmn_trace_sum_reduce (is_max = 0) / lmn_trace_max_reduce: front * dim * back rows and front * back outputs per member */
int lmn_trace_many_reduce(lmn_ctx* ctx, uint32_t is_max, const int32_t* input_dev, uint64_t input_member_stride, uint64_t front,
                          uint64_t dim, uint64_t back, const lmn_node_info* info, uint32_t n_members, uint32_t* rows_dev,
                          uint64_t row_offset, uint64_t rows_member_stride, int32_t* out_dev, uint64_t out_member_stride,
                          uint32_t* refused_dev);
/* lmn_trace_lut_ranges (the single range of lmn_trace_lut is one range): lut_col1_dev is shared by all members, mult_dev is
 * per member (mult_member_stride words apart, zero-initialised by the caller) */
int lmn_trace_many_lut_ranges(lmn_ctx* ctx, uint32_t kind, const int32_t* input_dev, const lmn_view* view,
                              uint64_t input_member_stride, uint64_t n, const lmn_node_info* info, const uint32_t* lut_col1_dev,
                              const lmn_range* ranges, uint32_t n_ranges, uint32_t n_members, uint32_t* mult_dev,
                              uint64_t mult_member_stride, uint32_t* rows_dev, uint64_t row_offset, uint64_t rows_member_stride,
                              int32_t* out_dev, uint64_t out_member_stride, uint32_t* refused_dev);

/* ---- The eval forms of the producers: `Operator::process`, the forward pass that `gen_circuit_settings` runs in front
 * of gen_trace (crates/graph/src/graph.rs:61-159) because a Sin / Exp2 / Log2 node's LUT range is the min..max of its
 * source buffer (crates/graph/src/utils.rs:44-82).  Each call computes the node's output tensor exactly as the
 * lmn_trace_* call of the same operands leaves it in out_dev - the same kernels' value rules, the producers' contract above -
 * and writes no rows.  In the same launch:
 *  - minmax_dev (int32_t[2] on the device, may be NULL) receives the minimum and maximum of the n values written; the
 *    call sets it to (INT32_MAX, INT32_MIN) first.  A refused element's 0 takes part: the buffer holds it.
 *  - refused_dev (a uint32_t counter on the device, may be NULL) grows by the number of refused elements - the rows whose
 *    output-value column the trace call marks with P.  It is never reset by a call: one counter serves a whole graph.
 * No call waits for the device.  Argument errors (null pointers, a view whose shape product is not n, more than 16
 * ranges, n = 0) return LMN_ERR_INVALID_ARGUMENT and lmn_last_error names the argument. */
/* every elementwise kind of lmn_trace_elementwise_v, and LMN_KIND_LESS_THAN (no multiplicity table is touched) */
int lmn_eval_elementwise_v(lmn_ctx* ctx, uint32_t kind, const int32_t* lhs_dev, const lmn_view* lhs_view, const int32_t* rhs_dev,
                           const lmn_view* rhs_view, uint64_t n, int32_t* out_dev, int32_t* minmax_dev, uint32_t* refused_dev);
/* SumReduce (is_max = 0) / MaxReduce of `dim` on a contiguous (front, dim, back) tensor: front * back values.  The running
 * sum is kept in 64 bits; only an input or a group result outside the value range is refused. */
int lmn_eval_reduce(lmn_ctx* ctx, uint32_t is_max, const int32_t* input_dev, uint64_t front, uint64_t dim, uint64_t back,
                    int32_t* out_dev, int32_t* minmax_dev, uint32_t* refused_dev);
/* how lmn_eval_reduce maps (dim, back) onto lanes: 0 = one lane per output element, 1 = one wave per reduction group */
uint32_t lmn_eval_reduce_split(uint64_t dim, uint64_t back);
/* out = lut_col1[LookupLayout::find_index(input)] over `ranges` (as lmn_trace_lut_ranges; no multiplicities).  An input
 * outside every range is a refused element (0 written, counted), not an error: a dry run does not wait per node. */
int lmn_eval_lut_ranges(lmn_ctx* ctx, uint32_t kind, const int32_t* input_dev, const lmn_view* view, uint64_t n,
                        const uint32_t* lut_col1_dev, const lmn_range* ranges, uint32_t n_ranges, int32_t* out_dev,
                        int32_t* minmax_dev, uint32_t* refused_dev);
/* the range of a buffer that no eval call produced */
int lmn_tensor_range(lmn_ctx* ctx, const int32_t* buf_dev, uint64_t n, int32_t* minmax_dev);

/* ---- Row sinks: host trace rows streamed to the GPU while they are produced.  The reference builds its pie on the
 * host node by node - every operator's `process_trace` appends with `table.add_row(...)`
 * (crates/graph/src/op/prim.rs:75, 412, 992, 1117) - and hands `prove` the finished pie (crates/prover/src/prover.rs:28-31,
 * 70).  A caller that keeps `process_trace` on the CPU opens one sink per table and pushes each node's rows when the node
 * is done: transfer and AoS -> SoA transpose then run under its own CPU work, and what is left in front of the proof is
 * the last chunk, the padding rows and one wait.  lmn_prove on plain host rows is unchanged.
 *
 * The contract:
 *  - Rows: lmn_kind_columns(kind) words each, in `Column::index()` order, as in lmn_table.  A chunk has ANY length >= 1
 *    (one node's rows), chunks arrive in table order.  More than `capacity_rows` (1 .. 2^26) in total is
 *    LMN_ERR_INVALID_ARGUMENT and the sink keeps what it had.  A sink never grows and never reallocates: its columns
 *    (capacity rounded up to a power of two, at least 16 rows) are allocated by lmn_rows_open, outside the context's
 *    per-proof arena.
 *  - lmn_rows_push returns when the library no longer needs `host_rows`: they went through the sink's own page-locked
 *    staging ring (4 slots of 4 MiB, allocated by the first such push; a push waits only when every slot is still in
 *    flight).  lmn_rows_push_pinned makes no CPU copy - the GPU reads the rows where they lie, once - and the buffer must
 *    stay untouched until lmn_rows_sync or lmn_rows_finish returns; memory the runtime does not know as page-locked
 *    (lmn_host_alloc / lmn_host_register) is refused with LMN_ERR_INVALID_ARGUMENT, never copied slowly instead.
 *  - Neither push waits for the device.  All device work of a sink runs on a stream of its own, not on the context's
 *    proof stream, and no lmn_rows_* call takes the context's lock: a proof of the previous pie on the same context
 *    (lmn_prove_submit, or lmn_prove on another thread) overlaps with the filling of the next sink.  Calls on ONE sink
 *    are serialised by the sink.
 *  - lmn_rows_finish writes the padding rows (lmn_kind_padding_row; rows [count, 2^log_size), log_size as lmn_prove
 *    derives it from n_rows: the next power of two, at least 16 rows), waits ONCE, and returns LMN_ERR_INVALID_ARGUMENT
 *    if any pushed word was >= 2^31 - 1 (or a device producer refused an element, lmn_rows_append_* below), LMN_ERR_EMPTY_TRACE if no row was pushed.  If 2^log_size is smaller than the
 *    column stride chosen at open, the columns are compacted so that table_out->rows has stride 2^log_size.  After an
 *    error the sink can be reset and the context is usable.  Pushing or finishing again without lmn_rows_reset is
 *    LMN_ERR_INVALID_ARGUMENT.
 *  - table_out = {kind, LMN_TABLE_COLS_ON_DEVICE, count, device pointer}.  lmn_prove / lmn_prove_submit accept such tables
 *    mixed freely with the two other kinds in one pie, on any context of the sink's device, with log_blowup 1, 2 or 3.
 *    The proof only READS the columns: proving the same finished sink twice gives the same bytes.  The sink must outlive
 *    the proof (lmn_prove_wait for submitted ones) and must not be reset or closed before; a table whose `rows` is not
 *    the columns of a live finished sink is LMN_ERR_INVALID_ARGUMENT.
 *  - Refused with LMN_ERR_INVALID_ARGUMENT and a text that says so: a LMN_TABLE_COLS_ON_DEVICE table on a sharded context
 *    (lmn_ctx_set_shard), and everything of this block in libluminair_hip_batch.so - lmn_rows_open there, and such a
 *    table in its lmn_batch_* AND in its solo lmn_prove.
 *  - The text of a failed lmn_rows_* call is available through lmn_last_error(NULL) on the calling thread. */
typedef struct lmn_rows lmn_rows;          /* a table being filled: column-major, in HBM, owned by the sink */
#define LMN_TABLE_COLS_ON_DEVICE 2u        /* `rows` = device pointer to n_columns(kind) columns of 2^log_size words each,
                                              padded, canonical: what lmn_rows_finish writes into table_out */
int lmn_rows_open(lmn_ctx* ctx, uint32_t kind, uint64_t capacity_rows, lmn_rows** out);
int lmn_rows_push(lmn_rows* rows, const uint32_t* host_rows, uint64_t n);         /* any host memory */
int lmn_rows_push_pinned(lmn_rows* rows, const uint32_t* host_rows, uint64_t n);  /* lmn_host_alloc / lmn_host_register memory */
int lmn_rows_sync(lmn_rows* rows);                         /* everything pushed so far has left the caller's buffers */
int lmn_rows_finish(lmn_rows* rows, lmn_table* table_out); /* pad, verdict on non-canonical words, fill table_out */
uint64_t lmn_rows_count(const lmn_rows* rows);
int lmn_rows_reset(lmn_rows* rows);                        /* same capacity, zero rows: the next proof's table */
void lmn_rows_close(lmn_rows* rows);

/* ---- Device producers that fill a row sink (lmn_rows_append_*): the four single producers - lmn_trace_elementwise_v (and
 * lmn_trace_less_than), lmn_trace_contiguous, lmn_trace_sum_reduce / _max_reduce, lmn_trace_lut_ranges, of which every other
 * single form is a special case - writing the node's rows straight into a sink's COLUMNS.  A pie built this way reaches
 * lmn_prove as LMN_TABLE_COLS_ON_DEVICE tables: no array-of-structs rows in HBM, and no transpose launch in front of the
 * proof.  The arguments are those of the single forms, with the sink in place of rows_dev / row_offset and a refused-element
 * counter behind them (lmn_rows_append_elementwise_v takes LessThan too: range_check_mult_dev is its 256-word table, ignored
 * for every other kind).
 *
 * The contract:
 *  - Rows: exactly the rows the corresponding lmn_trace_* call writes - n, max(in_size, out_size), front * dim * back and n of
 *    them - appended at the sink's current row count, in table order, as prim.rs appends.  There is no row_offset.
 *    lmn_rows_count has grown by that number when the call returns.  The values follow the producers' contract
 *    (lmn_trace_elementwise): out_dev receives what the row form writes, 0 for a refused element, and a refused element adds
 *    nothing to a multiplicity table.
 *  - Refused before any launch, with LMN_ERR_INVALID_ARGUMENT and a text in lmn_last_error(ctx) that names the argument, the
 *    sink keeping its count and content: a null sink; a sink whose kind is not the producer's (LMN_KIND_CONTIGUOUS for
 *    lmn_rows_append_contiguous, LMN_KIND_SUM_REDUCE / LMN_KIND_MAX_REDUCE for lmn_rows_append_reduce); a sink that is not
 *    filling (finished, or failed, without lmn_rows_reset); more rows than capacity - count; a context on another device
 *    than the sink's.  Each single form's own argument errors keep their own codes (n == 0: LMN_ERR_EMPTY_TRACE; a view whose
 *    shape product is not n: LMN_ERR_INVALID_ARGUMENT; ...).  libluminair_hip_batch.so exports the four entry points, and -
 *    as no sink can exist there - they refuse in the same way.
 *  - No call waits for the device.  An element outside the producers' contract - a LUT input outside every range included,
 *    as in lmn_trace_many_lut_ranges and lmn_eval_lut_ranges - is a refused element: its row carries the non-canonical word
 *    2^31 - 1 in the output-value column, the sink's verdict word is set, and *refused_dev (a uint32 device word, may be
 *    NULL, never reset by a call) grows by one.  lmn_rows_finish of such a sink returns LMN_ERR_INVALID_ARGUMENT.
 *  - A call takes the context's lock, as every lmn_trace_* call does, and then the sink's - always in that order.  The other
 *    lmn_rows_* calls still never take a context's lock.
 *  - Stream order: the launch runs on the context's stream, ordered with the tensors it reads and writes, and the sink
 *    records an event on that stream behind each append.  lmn_rows_sync, lmn_rows_finish, lmn_rows_reset and lmn_rows_close
 *    make the sink's own stream wait for that event before they do anything else, so lmn_rows_sync after appends means the
 *    producers have finished (operand tensors may be freed).  lmn_rows_reset records an event behind the clearing of the
 *    verdict word, and the next append makes the context's stream wait for it: a failed table followed by a clean one can
 *    neither lose nor inherit the verdict.
 *  - Host pushes and device appends may be mixed in one sink, in any order: they write disjoint rows, and the finish waits
 *    for both.
 *  - lmn_rows_finish is unchanged in shape - padding rows, compaction when 2^log_size is below the stride chosen at open, one
 *    wait, the verdict - and table_out is the same LMN_TABLE_COLS_ON_DEVICE table, accepted wherever such tables are. */
int lmn_rows_append_elementwise_v(lmn_ctx* ctx, lmn_rows* rows, uint32_t kind, const int32_t* lhs_dev, const lmn_view* lhs_view,
                                  const int32_t* rhs_dev, const lmn_view* rhs_view, uint64_t n, const lmn_node_info* info,
                                  uint32_t* range_check_mult_dev /* LessThan only */, int32_t* out_dev, uint32_t* refused_dev);
int lmn_rows_append_contiguous(lmn_ctx* ctx, lmn_rows* rows, const int32_t* input_dev, uint64_t in_size, const lmn_view* view,
                               uint64_t out_size, const lmn_node_info* info, int32_t* out_dev, uint32_t* refused_dev);
int lmn_rows_append_reduce(lmn_ctx* ctx, lmn_rows* rows, uint32_t is_max, const int32_t* input_dev, uint64_t front, uint64_t dim,
                           uint64_t back, const lmn_node_info* info, int32_t* out_dev, uint32_t* refused_dev);
int lmn_rows_append_lut_ranges(lmn_ctx* ctx, lmn_rows* rows, uint32_t kind, const int32_t* input_dev, const lmn_view* view,
                               uint64_t n, const lmn_node_info* info, const uint32_t* lut_col1_dev, const lmn_range* ranges,
                               uint32_t n_ranges, uint32_t* mult_dev, int32_t* out_dev, uint32_t* refused_dev);

/* ---- Float tensors in and out: `CopyToStwo` / `CopyFromStwo` on the device (crates/graph/src/op/prim.rs:52-101).  The
 * reference's user-facing tensor is `Vec<f32>`: a graph input becomes Fixed<12> through `StwoData::from_f32`
 * (`Fixed::from_f64(d as f64)` per element, crates/graph/src/data.rs:17-31) and an output leaves as `d.to_f64() as f32`.
 * These calls state both rules once, in integers, for float tensors that already lie in HBM.
 *
 * Float -> Fixed<12> (dtype LMN_F32 / LMN_F16 / LMN_BF16; the source holds raw IEEE bits, 4 or 2 bytes per element):
 *  - the exact real value x 4096, rounded to the nearest integer, ties away from zero (`f64::round`; numerair is un-vendored,
 *    so its rounding is unpinned - DESIGN.md section 2 - as for lmn_lut_from_ranges).  Widening f16 / bf16 is exact, so this
 *    is what the reference's `d as f64` route gives for the widened value.  +-0 and every denormal give 0.
 *  - Refused: a NaN of any payload or sign, +-Inf, and a rounded value outside [-(2^30-1), 2^30-1].  A refused element is
 *    handled as the producers' contract (lmn_trace_elementwise) says: the word P in the Inputs row's val, 0 in the output
 *    tensor, counted where the form has a counter, and no lane does value-dependent work for it.
 * Fixed<12> -> float: the exact value v / 4096 rounded once to the format, round-to-nearest-even (bf16 is NOT rounded
 * through f32); an f16 magnitude above 65504 becomes +-Inf as IEEE says.  A source word outside [-(2^30-1), 2^30-1] cannot
 * occur in a tensor a producer wrote: its result is unspecified, the call stays memory-safe.
 *
 * The four input forms are lmn_trace_elementwise(LMN_KIND_INPUTS, ...), lmn_trace_many_elementwise_v, lmn_rows_append_elementwise_v
 * and lmn_eval_elementwise_v with the conversion in front, in the SAME launch: rows, output tensor, marks, counters, strides
 * (0 = shared, with the shared-output rule), stream order, locks and "no call waits" are exactly what those forms document,
 * and rows and out_dev are word for word what the integer form writes for the converted integers.  src_dev is contiguous;
 * src_member_stride is in elements of dtype.  Refused before any launch, the argument named by lmn_last_error: an unknown
 * dtype, a null src_dev, n = 0 (LMN_ERR_EMPTY_TRACE for the three trace forms, LMN_ERR_INVALID_ARGUMENT for the eval form,
 * as their siblings), a src_dev that is not aligned to the element size, and every error of the sibling form.
 * libluminair_hip_batch.so exports all five; the sink form refuses there as every lmn_rows_append_* does.
 *
 * lmn_tensor_to_float converts n contiguous values and returns when dst_dev is complete, as lmn_download does: a reader on
 * another stream may use dst_dev at once.  dst_dev is aligned to the element size. */
#define LMN_F32 0u
#define LMN_F16 1u
#define LMN_BF16 2u
int lmn_trace_inputs_float(lmn_ctx* ctx, uint32_t dtype, const void* src_dev, uint64_t n, const lmn_node_info* info,
                           uint32_t* rows_dev, uint64_t row_offset, int32_t* out_dev);
int lmn_trace_many_inputs_float(lmn_ctx* ctx, uint32_t dtype, const void* src_dev, uint64_t src_member_stride, uint64_t n,
                                const lmn_node_info* info, uint32_t n_members, uint32_t* rows_dev, uint64_t row_offset,
                                uint64_t rows_member_stride, int32_t* out_dev, uint64_t out_member_stride, uint32_t* refused_dev);
int lmn_rows_append_inputs_float(lmn_ctx* ctx, lmn_rows* rows, uint32_t dtype, const void* src_dev, uint64_t n,
                                 const lmn_node_info* info, int32_t* out_dev, uint32_t* refused_dev);
int lmn_eval_inputs_float(lmn_ctx* ctx, uint32_t dtype, const void* src_dev, uint64_t n, int32_t* out_dev, int32_t* minmax_dev,
                          uint32_t* refused_dev);
int lmn_tensor_to_float(lmn_ctx* ctx, uint32_t dtype, const int32_t* src_dev, uint64_t n, void* dst_dev);

/* ---- lmn_trace_check: which rows and which logup tuples break a trace.  lmn_prove answers a bad trace once, at the end of
 * a whole proof, with LMN_ERR_CONSTRAINTS - no table, no row, no constraint - and a trace whose logup relations do not
 * balance is proved all the same (only lmn_verify says LMN_ERR_INVALID_LOGUP).  This call is the prover-side counterpart of
 * lmn_verify_diagnose: it commits, transforms and draws nothing; it reads the tables where they lie and reports.
 *
 * The contract (exact and deterministic; tests compare for equality with the oracle):
 *  - Input: `tables` in exactly the forms lmn_prove takes (host rows, LMN_TABLE_ROWS_ON_DEVICE, LMN_TABLE_COLS_ON_DEVICE of
 *    a finished sink), validated by lmn_prove's own setup rules (supported kind with a claim slot, ascending kinds, at most
 *    2^26 rows, a LUT for each lookup table, a lookup table whose padded size is the LUT's).  What lmn_prove's setup refuses
 *    is refused here with the same code, and the text (lmn_last_error) names the table: "table 2 (kind 4): ...".
 *  - Scope: only the n_rows real rows.  The padding rows are the library's own and carry multiplicity 0.
 *  - Non-canonical words: a word >= 2^31 - 1.  `n_noncanonical` counts them all; nc_table / nc_row / nc_column name the
 *    smallest (table, row, column).  A row that holds one is left out of the two checks below.
 *  - Local constraints: for every table and every local kernel slot - the component's local constraints in `evaluate`
 *    order, the first lmn_kind_constraints(kind) - lmn_kind_relations(kind) slots in lmn_kind_constraint_layout's indexing;
 *    Mul's slot 2 is identically zero - the number of real rows on which the slot is non-zero and the smallest such row.
 *    The constraint-form bits (LMN_PV_*_NEG, LMN_PV_*_SLOT(S)) do not change which rows violate: no flags.  Evaluated in
 *    M31 on the row's own words (every constraint is row-local: the next_* values are columns of the row).
 *    `n_constraint_slots` (table, slot) pairs are violated; the first LMN_TRACE_REPORT_MAX of them, sorted by (table, slot),
 *    are listed, `constraints_truncated` says whether that was all.
 *  - Relation balance: every relation entry of every row whose multiplicity word is non-zero contributes +mult (-mult where
 *    the component's relation is subtracted: the lookup tables) to the tuple (element set, val, id) - element sets as in
 *    LMN_N_ELEMS below (0 NodeElements, 1 RangeCheck, 2 Sin, 3 Exp2, 4 Log2), id = 0 for width-1 relations, lookup tables
 *    take val and id from the LUT columns of `settings`, the range check takes val from the row index.  A tuple is
 *    unbalanced when its net sum is non-zero mod P.  `n_unbalanced` is their exact number; up to LMN_TRACE_REPORT_MAX are
 *    listed with the net as an M31 word and the smallest (table, slot, row) that mentions the tuple (slot = the relation's
 *    kernel slot, local slots first).  With at most LMN_TRACE_REPORT_MAX unbalanced tuples all are listed, sorted by (set, id,
 *    val); with more, `tuples_truncated` is set and every listed entry is still a true one.  An exact multiset check - no
 *    randomness, no soundness parameter.
 *  - Returns LMN_OK when the check ran, whatever it found (as lmn_verify_diagnose does); report->ok = 1 iff all three findings
 *    are empty; report->summary is one line of text.  LMN_ERR_OUT_OF_MEMORY when a tuple table cannot be allocated.
 *  - Takes the context's lock, runs on its stream, frees all its scratch before it returns and leaves the context usable
 *    after any outcome.  No collective: works on a sharded context (for the table forms lmn_prove accepts there) and in
 *    libluminair_hip_batch.so's solo path. */
#define LMN_TRACE_REPORT_MAX 64
struct lmn_trace_constraint {
  uint32_t table;      /* index into `tables` */
  uint32_t kind;       /* LMN_KIND_* of that table */
  uint32_t slot;       /* local kernel slot */
  uint32_t reserved;
  uint64_t count;      /* real rows on which the slot is non-zero */
  uint64_t first_row;  /* the smallest of them */
};
typedef struct lmn_trace_constraint lmn_trace_constraint;
struct lmn_trace_tuple {
  uint32_t set;          /* element set 0..4 */
  uint32_t val, id;      /* the tuple; id = 0 for width-1 relations */
  uint32_t net;          /* net multiplicity, an M31 word != 0 */
  uint32_t first_table;  /* smallest (table, slot, row) that mentions the tuple */
  uint32_t first_slot;
  uint64_t first_row;
};
typedef struct lmn_trace_tuple lmn_trace_tuple;
struct lmn_trace_report {
  uint32_t ok;                     /* 1 iff no non-canonical word, no violated slot, no unbalanced tuple */
  uint32_t n_constraints;          /* entries of `constraints` */
  uint32_t n_constraint_slots;     /* violated (table, slot) pairs in all */
  uint32_t constraints_truncated;
  uint32_t n_tuples;               /* entries of `tuples` */
  uint32_t tuples_truncated;
  uint64_t n_unbalanced;           /* unbalanced tuples in all */
  uint64_t n_noncanonical;         /* words >= 2^31 - 1 in all */
  uint32_t nc_table, nc_column;    /* the smallest (table, row, column) holding one (n_noncanonical != 0) */
  uint64_t nc_row;
  lmn_trace_constraint constraints[LMN_TRACE_REPORT_MAX];
  lmn_trace_tuple tuples[LMN_TRACE_REPORT_MAX];
  char summary[256];
};
typedef struct lmn_trace_report lmn_trace_report;
int lmn_trace_check(lmn_ctx* ctx, const lmn_table* tables, size_t n_tables, const lmn_settings* settings,
                    lmn_trace_report* report);

/* ---- Single-proof sharding over the GPUs of one node (BASELINE.json configs 4 and 5).
 * One context per GPU, world = 1, 2, 4 or 8 ranks.  Every rank calls lmn_prove with the SAME tables and gets the
 * SAME proof bytes as an unsharded context would produce.  What is split: every rank evaluates only its aligned
 * block of rows of each LDE (the commitment `tree_builder.commit`, /root/reference/crates/prover/src/prover.rs:179,
 * 298, and stwo's commit of the composition polynomial behind prover.rs:312), hashes the Merkle subtree over that
 * block, evaluates constraint quotients, FRI quotients and FRI pair-folds on its rows.  What is exchanged, all
 * through ONE primitive, an in-place all-gather on device memory: the world subtree roots of every committed tree
 * (32 B per rank), the composition evaluations (16 B per eval-domain row in total) before their interpolation,
 * FRI layers / quotient columns of at most 2^fri_min_log rows (finished on every rank), and the few KB of
 * decommitted values.  The trace-sized transposes / interpolations / logup columns are recomputed on every rank:
 * cheaper than moving the coefficients over xGMI.
 *
 * `all_gather` must be stream-ordered on `stream` (a hipStream_t): `buf_dev` holds world * bytes_per_rank bytes,
 * this rank's part is already at offset rank * bytes_per_rank, and on completion every part is filled in (the
 * in-place form of ncclAllGather).  Return 0 on success. */
typedef struct lmn_collective {
  void* user;
  int (*all_gather)(void* user, void* buf_dev, size_t bytes_per_rank, void* stream);
  /* optional (may be NULL): bracket a batch of all_gather calls that may be fused into one launch
   * (ncclGroupStart / ncclGroupEnd); the 4 coordinate columns of a secure column are gathered as one batch */
  int (*group_begin)(void* user);
  int (*group_end)(void* user);
  /* optional (may be NULL; since ABI version 5): the second exchange primitive, SURVEY.md section 8(e) stage B.  With it
   * every rank interpolates and extends only 1/world of the columns of a commitment (stage A) and the extended columns
   * are re-partitioned into row blocks by ONE stream-ordered all-to-all: this rank sends send_bytes[p] bytes at
   * send_dev + send_off[p] to every rank p and receives recv_bytes[p] bytes from p at recv_dev + recv_off[p]
   * (arrays of `world` entries, p = rank included: a local copy).  Grouped ncclSend / ncclRecv in the built-in
   * transport.  Without it the columns are interpolated on every rank (round 2-3 behaviour). */
  int (*all_to_all)(void* user, const void* send_dev, const size_t* send_off, const size_t* send_bytes, void* recv_dev,
                    const size_t* recv_off, const size_t* recv_bytes, void* stream);
} lmn_collective;
/* fri_min_log = 0 selects the default (16: every all-gather of a small FRI layer's subtree roots costs a
 * collective's latency, hashing a 2^16-row layer on every rank does not).  world = 1 is allowed (the collective is
 * still called). */
int lmn_ctx_set_shard(lmn_ctx* ctx, uint32_t rank, uint32_t world, uint32_t fri_min_log, const lmn_collective* coll);
/* Built-in transport: RCCL over xGMI (librccl is dlopen'ed on first use, the library has no link-time dependency
 * on it).  Rank 0 creates the id, the caller hands the 128 bytes to the other ranks by any means. */
#define LMN_RCCL_ID_BYTES 128
int lmn_rccl_unique_id(uint8_t id_out[LMN_RCCL_ID_BYTES]);
int lmn_ctx_set_shard_rccl(lmn_ctx* ctx, uint32_t rank, uint32_t world, uint32_t fri_min_log,
                           const uint8_t id[LMN_RCCL_ID_BYTES]);
int lmn_ctx_clear_shard(lmn_ctx* ctx);

/* ---- Level 2, host-buffer convenience forms (each call: H2D -> kernel -> D2H; the device-handle forms a
 * `HipBackend` would use are the lmn_col_* functions at the end of this header).  Columns are `ncols` arrays of
 * 2^log_size words. */
int lmn_op_interpolate(lmn_ctx* ctx, uint32_t* cols, uint32_t ncols, uint32_t log_size);           /* PolyOps::interpolate */
int lmn_op_evaluate(lmn_ctx* ctx, const uint32_t* coeffs, uint32_t ncols, uint32_t log_coeffs,
                    uint32_t log_domain, uint32_t* evals_out);                                     /* PolyOps::evaluate */
int lmn_op_merkle_root(lmn_ctx* ctx, const uint32_t* const* cols, const uint32_t* log_sizes, uint32_t ncols,
                       uint8_t root_out[32]);                                                      /* MerkleOps::commit_on_layer chain */
int lmn_op_eval_at_point(lmn_ctx* ctx, const uint32_t* coeffs, uint32_t log_size, const uint32_t point_xy[8],
                         uint32_t value_out[4]);                                                   /* PolyOps::eval_at_point */
/* QuotientOps::accumulate_quotients for the columns of ONE LDE size: `cols[c]` = 2^log_size evaluations
 * (bit-reversed canonic domain); sample i = (column sample_col[i], point sample_point[i], value
 * sample_values[4i..4i+4)), in (column, mask-position) order; points_xy = npoints x 8 words (x then y);
 * out = 4 coordinate columns x 2^log_size.  Limits of one call (also of lmn_col_accumulate_quotients): at most 4
 * distinct sample_point indices and at most 512 samples; beyond either the call returns LMN_ERR_INVALID_ARGUMENT. */
int lmn_op_accumulate_quotients(lmn_ctx* ctx, uint32_t log_size, const uint32_t* const* cols, uint32_t ncols,
                                const uint32_t* sample_col, const uint32_t* sample_point, const uint32_t* sample_values,
                                uint32_t nsamples, const uint32_t* points_xy, uint32_t npoints, const uint32_t alpha[4],
                                uint32_t* out);
/* FriOps::fold_line: src = 4 coordinate columns x 2^log_src on LineDomain(half_odds(log_src)); dst gets 2^(log_src-1). */
int lmn_op_fold_line(lmn_ctx* ctx, const uint32_t* src, uint32_t log_src, const uint32_t alpha[4], uint32_t* dst);
/* FriOps::fold_circle_into_line: dst (4 x 2^(log_src-1), in/out) = dst * alpha^2 + fold(src), src on the
 * canonic circle domain of log_src. */
int lmn_op_fold_circle_into_line(lmn_ctx* ctx, uint32_t* dst, const uint32_t* src, uint32_t log_src, const uint32_t alpha[4]);
/* GrindOps::grind: smallest nonce accepted by the proof-of-work check of `protocol_variant` (LMN_PV_POW_PREFIXED,
 * LMN_PV_MIX_U64_HASHED) on channel state `digest` (host). */
int lmn_op_grind(const uint8_t digest[32], uint32_t pow_bits, uint32_t protocol_variant, uint64_t* nonce_out);
/* lmn_ctx_grind returns the same nonce as lmn_op_grind, found on the context's GPU (serialised with its proofs). */
int lmn_ctx_grind(lmn_ctx* ctx, const uint8_t digest[32], uint32_t pow_bits, uint32_t protocol_variant,
                  uint64_t* nonce_out);                                                            /* GrindOps::grind on the device */
/* The same for n channel digests ground together, one kernel over all of them: nonces_out[i] is lmn_op_grind's nonce
 * for digests[32 * i .. 32 * i + 32).  n == 0 is LMN_OK and touches nothing; a null pointer, n > LMN_GRIND_MANY_MAX,
 * pow_bits > 40 or unknown variant bits are LMN_ERR_INVALID_ARGUMENT, and lmn_last_error names the argument. */
#define LMN_GRIND_MANY_MAX 1024
int lmn_ctx_grind_many(lmn_ctx* ctx, const uint8_t* digests /* 32 * n bytes */, uint32_t n, uint32_t pow_bits,
                       uint32_t protocol_variant, uint64_t* nonces_out /* n */);
/* PolyOps::evaluate restricted to one aligned block of rows (single-commitment sharding over GPUs):
 * rows [block * 2^(log_domain - log_blocks), (block + 1) * 2^(log_domain - log_blocks)) of every column's
 * evaluation on the 2^log_domain domain, computed from the coefficients alone (1 <= log_blocks <= 3).
 * evals_out: ncols x 2^(log_domain - log_blocks) words. */
int lmn_op_evaluate_block(lmn_ctx* ctx, const uint32_t* coeffs, uint32_t ncols, uint32_t log_coeffs, uint32_t log_domain,
                          uint32_t log_blocks, uint32_t block, uint32_t* evals_out);
int lmn_op_fft_selftest(lmn_ctx* ctx, uint32_t log_size, uint32_t ncols);  /* tiled vs single-layer kernels */

/* ---- Level 2 on device handles ("Each takes device handles (lmn_col*) so columns stay resident").
 * This is what a Rust `HipBackend` would bind in place of `SimdBackend` behind
 * /root/reference/crates/prover/src/prover.rs:38-46,312 and the `TreeBuilder` shim
 * /root/reference/crates/air/src/utils.rs:112-128: stwo's `Col<B, BaseField>` becomes an `lmn_col` with ncols = 1,
 * a `SecureColumnByCoords<B>` an `lmn_col` with ncols = 4 (coordinate-major), a batch of equal-size columns one
 * `lmn_col` with ncols = n.  Data moves between host and HBM only in lmn_col_from_cpu / lmn_col_to_cpu (stwo's
 * `Column::to_cpu` / `FromIterator`); every op below runs on HBM-resident data on the context's stream and returns
 * after enqueueing (ops on one context are stream-ordered; lmn_col_to_cpu and the ops that return values to the
 * host synchronise).  stwo trait and method names are from the un-vendored dependency (unverified here, SURVEY.md
 * §8b); each op is checked against the oracle's restatement of the same operation (tests/level2_checks.py). */
typedef struct lmn_col lmn_col;   /* ncols columns of 2^log_size canonical-M31 words, contiguous, stride 2^log_size */
typedef struct lmn_tree lmn_tree; /* a committed Merkle tree: every layer stays in HBM for decommitment */

int lmn_col_alloc(lmn_ctx* ctx, uint32_t ncols, uint32_t log_size, lmn_col** out);            /* Column::zeros       */
int lmn_col_from_cpu(lmn_ctx* ctx, const uint32_t* host, uint32_t ncols, uint32_t log_size, lmn_col** out);
int lmn_col_to_cpu(lmn_ctx* ctx, const lmn_col* col, uint32_t* host);                          /* Column::to_cpu      */
void lmn_col_free(lmn_ctx* ctx, lmn_col* col);
uint32_t lmn_col_ncols(const lmn_col* col);
uint32_t lmn_col_log_size(const lmn_col* col);
void* lmn_col_device_ptr(const lmn_col* col);                                                  /* for lmn_table.rows etc. */
/* Non-owning handle over columns [first, first + n) of `col` (stwo holds one `Col` per column; here a batch of
 * equal-size columns is one allocation, and a single column / one component's columns are views of it).  Valid
 * while `col` lives; released with lmn_col_free (which then frees nothing on the device). */
int lmn_col_view(lmn_ctx* ctx, const lmn_col* col, uint32_t first, uint32_t n, lmn_col** out);

int lmn_col_bit_reverse(lmn_ctx* ctx, lmn_col* col);                         /* ColumnOps::bit_reverse_column, in place  */
int lmn_col_precompute_twiddles(lmn_ctx* ctx, uint32_t log_size);            /* PolyOps::precompute_twiddles (cached in the ctx) */
int lmn_col_interpolate(lmn_ctx* ctx, lmn_col* evals_to_coeffs);             /* PolyOps::interpolate(_columns), in place */
int lmn_col_evaluate(lmn_ctx* ctx, const lmn_col* coeffs, uint32_t log_domain, lmn_col** evals_out);  /* PolyOps::evaluate(_polynomials) */
int lmn_col_evaluate_block(lmn_ctx* ctx, const lmn_col* coeffs, uint32_t log_domain, uint32_t log_blocks, uint32_t block,
                           lmn_col** evals_out);                             /* row block `block` of 2^log_blocks (sharded commit) */
int lmn_col_extend(lmn_ctx* ctx, const lmn_col* coeffs, uint32_t log_size, lmn_col** out);   /* PolyOps::extend: zero-padded coefficients */
int lmn_col_eval_at_point(lmn_ctx* ctx, const lmn_col* coeffs, uint32_t column, const uint32_t point_xy[8],
                          uint32_t value_out[4]);                            /* PolyOps::eval_at_point */
/* MerkleOps::commit_on_layer for every layer: columns of any mix of sizes (each lmn_col contributes its ncols
 * columns), sorted by size descending (stable) as `MerkleProver::commit` does. */
int lmn_col_commit(lmn_ctx* ctx, const lmn_col* const* cols, uint32_t n, lmn_tree** tree_out);
int lmn_tree_root(lmn_ctx* ctx, const lmn_tree* tree, uint8_t root_out[32]);
uint32_t lmn_tree_log_size(const lmn_tree* tree);
int lmn_tree_layer_to_cpu(lmn_ctx* ctx, const lmn_tree* tree, uint32_t layer_log, uint8_t* hashes_out); /* 32 * 2^layer_log bytes */
/* MerkleProver::decommit on a device tree: the walk that decides which nodes an opening needs runs on the host, ONE launch
 * fetches them from the tree's layers and the column handles, ONE transfer brings them back - the columns and the layers
 * themselves never leave HBM.  `cols`: the handles the tree was committed from, same order (views are fine).
 * Queries: n_groups groups; group g holds query_counts[g] positions for columns of size 2^query_logs[g], flat in
 * `queries`, each group strictly ascending, every position < 2^query_logs[g], query_logs distinct and <= the tree's
 * log size (a log size at which the tree has no columns is allowed).  Outputs are allocated by the library and released
 * with lmn_free (an empty one is NULL with count 0): queried values and column witness as words, hash witness as 32-byte
 * hashes.  Order of all three = MerkleProver::decommit's: layer by layer from the leaves up, node-ascending, a layer's
 * columns in size-sorted tree order.  Zero groups give the root-only walk's result: three empty outputs.
 * LMN_ERR_INVALID_ARGUMENT, with a text that names the argument, and all six outputs NULL / 0: columns whose sizes differ
 * from what the tree was committed from, unsorted or repeated positions, a position out of range, a repeated or too large
 * query log size, a null pointer where a count is non-zero, an opening of more than 12 MiB.  Context and tree stay usable. */
int lmn_tree_decommit(lmn_ctx* ctx, const lmn_tree* tree, const lmn_col* const* cols, uint32_t n_cols,
                      const uint32_t* query_logs, const uint32_t* query_counts, uint32_t n_groups,
                      const uint32_t* queries,
                      uint32_t** queried_values, size_t* n_values,
                      uint8_t** hash_witness, size_t* n_hashes,
                      uint32_t** column_witness, size_t* n_column_words);
/* host_out[j * n + i] = column j of `col` at positions[i]; any order, repeats allowed, every position < 2^log_size
 * (else LMN_ERR_INVALID_ARGUMENT before anything is launched).  One launch, one transfer back, one wait; works on views;
 * n = 0 returns LMN_OK and writes nothing; at most 12 MiB of positions and of values per call.  What FriProver::decommit
 * needs for its witness evaluations, and the queried values of a secure column. */
int lmn_col_gather(lmn_ctx* ctx, const lmn_col* col, const uint32_t* positions, uint32_t n, uint32_t* host_out);
void lmn_tree_free(lmn_ctx* ctx, lmn_tree* tree);
/* FriProver::commit without the last layer's interpolation: the layer loop of lmn_prove's FRI commit phase - the same
 * function, so the same launches - on secure-column handles, with everything it left in device memory brought to the host.
 * `cols`: n >= 1 handles of 4 coordinate columns each (the FRI quotient columns, bit-reversed circle-domain evaluations), of
 * strictly decreasing log sizes; they need not be low-degree.  cols[0] is folded (circle to line) with the alpha drawn after
 * the first tree's root; cols[k] joins the line layer of half its size.  `start_digest`: the channel's 32-byte digest before
 * the first root is mixed.  The context's log_last_layer, log_blowup and the LMN_PV_DRAW_CTR_U32 bit of protocol_variant
 * apply: the loop ends at the layer of 2^(log_last_layer + log_blowup) values.
 * Result (every pointer from malloc, each released with lmn_free; the struct itself is the caller's):
 *   trees    t = 0 .. n_trees-1: the first tree (over all of `cols`), then one per inner layer.  roots[32 t], alphas[4 t] (the
 *            alpha drawn after root t), tree_logs[t], level_masks[t] (bit l set: level l of 2^l hashes was written to device
 *            memory; clear: a fused launch kept it in registers, or the leaf level was hashed by the launch of the level
 *            above it), `levels`: the written levels of tree 0, then of tree 1, ..., each tree's from level 0 upwards,
 *            8 words per hash.
 *   layers   i = 0 .. n_trees-1: inner layer i (log size tree_logs[0] - 1 - i, committed by tree i + 1), the last one being
 *            the last layer (no tree).  `values`: 4 x 2^log words per layer, coordinate-major, one layer after the other.
 *   forms    n_trees + 1 words.  forms[0]: LMN_FRI_FIRST_TREE, or LMN_FRI_FIRST_TREE_BELOW when the first tree's leaf level
 *            was hashed by the launch of the level above it.  forms[1 + i]: how layer i's values were produced
 *            (LMN_FRI_FOLD_*) or'ed with how it was committed (LMN_FRI_TREE_*; neither for the last layer).
 * LMN_ERR_INVALID_ARGUMENT with a text naming the argument, the result zeroed, context and handles usable: a null
 * pointer, n = 0, a handle that is not 4 columns, sizes not strictly decreasing, a first line layer smaller than the last
 * layer, a column that would join below the last layer, a sharded context. */
#define LMN_FRI_FOLD_LAUNCH 1u          /* plain fold launch(es): k_fold (a joining column: one more launch each) */
#define LMN_FRI_FOLD_IN_LEAVES 2u       /* inside the layer's own leaf hashing (k_merkle_fused<3>) */
#define LMN_FRI_FOLD_IN_LEAVES_JOIN 3u  /* the same, with a joining quotient column */
#define LMN_FRI_FOLD_MATERIALISED 4u    /* a fold left for the leaf hashing, made by k_fold after all (layer <= 2^10, or the last) */
#define LMN_FRI_FOLD_TAIL_FRONT 5u      /* by the tail's launch, in front of its first layer (k_fri_tail) */
#define LMN_FRI_FOLD_IN_TAIL 6u         /* inside the tail's launch */
#define LMN_FRI_FOLD_MASK 0xffu
#define LMN_FRI_TREE_OWN 0x100u         /* committed by launches of its own */
#define LMN_FRI_TREE_IN_TAIL 0x200u     /* committed inside the tail's launch */
#define LMN_FRI_FIRST_TREE 0x10000u
#define LMN_FRI_FIRST_TREE_BELOW 0x10001u
struct lmn_fri_commit_result {
  uint32_t n_trees;
  uint32_t reserved;
  uint8_t* roots;          /* n_trees x 32 bytes */
  uint32_t* alphas;        /* n_trees x 4 words */
  uint32_t* tree_logs;     /* n_trees */
  uint32_t* level_masks;   /* n_trees */
  uint32_t* forms;         /* n_trees + 1 */
  uint32_t* values;        /* n_value_words */
  uint32_t* levels;        /* n_level_words */
  uint64_t n_value_words;
  uint64_t n_level_words;
};
typedef struct lmn_fri_commit_result lmn_fri_commit_result;
int lmn_col_fri_commit(lmn_ctx* ctx, const lmn_col* const* cols, uint32_t n, const uint8_t start_digest[32],
                       lmn_fri_commit_result* result);
/* What FriProver::commit and the query phase do BEHIND the layer loop, on the device and in one call: the last layer's
 * polynomial (line interpolation of `last_layer`: 4 coordinate columns of 2^(log_last_layer + log_blowup) rows, bit-reversed
 * over LineDomain(half_odds), as lmn_col_fri_commit leaves the last layer), its degree check, Channel::mix_felts over the
 * first 2^log_last_layer coefficients starting from `start_digest` (the channel behind the last folding alpha), the proof
 * of work (GrindOps::grind at the context's pow_bits), Channel::mix_u64 of the nonce, and Queries::generate: n_queries
 * positions drawn 8 per draw_random_words, masked to log_query_domain bits, ascending and distinct.  The context's
 * log_last_layer, log_blowup, pow_bits, n_queries and protocol_variant apply.  The chain is k_fri_close, 8 grind windows
 * and k_fri_queries behind ONE host wait, whatever LMN_POW_DEVICE_MIN_BITS says (as lmn_ctx_grind); a nonce beyond the
 * queued windows is found by further grind rounds (grind_rounds counts their host waits) and the rest replayed on the host.
 * A layer of too high a degree is LMN_OK with first_bad set: the transcript goes on over the truncated coefficients, and
 * the caller decides.  LMN_ERR_INVALID_ARGUMENT with a text naming the argument, the result zeroed, context and handles
 * usable: a null pointer, a handle that is not 4 columns of 2^(log_last_layer + log_blowup) rows, log_query_domain > 31, a
 * sharded context.  coeffs and positions are released with lmn_free. */
struct lmn_fri_close_result {
  uint32_t n_coeffs;      /* 2^log_last_layer */
  uint32_t first_bad;     /* lowest index >= n_coeffs of a non-zero coefficient; 0xffffffff: degree ok */
  uint32_t n_positions;   /* distinct query positions */
  uint32_t grind_rounds;  /* host waits spent grinding after the chain's own wait (0: found in the queued windows) */
  uint64_t nonce;
  uint32_t* coeffs;       /* 4 words per coefficient (a,b,c,d), as proof.last_layer_coeffs; lmn_free */
  uint32_t* positions;    /* ascending, distinct; lmn_free */
  uint8_t digest_after_coeffs[32], digest_after_nonce[32], digest_end[32];
  uint32_t n_sent_end, reserved;
};
typedef struct lmn_fri_close_result lmn_fri_close_result;
int lmn_col_fri_close(lmn_ctx* ctx, const lmn_col* last_layer, const uint8_t start_digest[32],
                      uint32_t log_query_domain /* 0..31 */, lmn_fri_close_result* result);
/* Query positions in device memory: at most 1024 ascending distinct positions < 2^log_domain (log_domain <= 31).  A
 * handle is what lmn_open_queries reads; it is made from host positions (lmn_positions_from_cpu: LMN_ERR_INVALID_ARGUMENT
 * with a text naming the argument for a null pointer with n > 0, n > 1024, log_domain > 31, a position out of range or
 * not strictly above its predecessor) or left behind by lmn_col_fri_close_keep, behind the same single wait as the
 * close itself.  lmn_positions_to_cpu writes the positions to `host` (room for 1024 words) and their number
 * to *n_out.  lmn_positions_free waits for the context's stream first; a null handle is ignored. */
typedef struct lmn_positions lmn_positions;
int lmn_positions_from_cpu(lmn_ctx* ctx, const uint32_t* positions, uint32_t n, uint32_t log_domain, lmn_positions** out);
int lmn_positions_to_cpu(lmn_ctx* ctx, const lmn_positions* positions, uint32_t* host, uint32_t* n_out);
uint32_t lmn_positions_log_domain(const lmn_positions* positions);
void lmn_positions_free(lmn_ctx* ctx, lmn_positions* positions);
/* lmn_col_fri_close with the positions kept on the device as well: the same chain behind the same single wait (one
 * implementation behind both entry points), with one copy queued behind k_fri_queries that moves the positions from the
 * chain's page-locked result block - where k_fri_queries writes them for the host - into a new handle of log_domain =
 * log_query_domain: they cross the link once more, in front of the wait, and no host code touches them.  When the nonce lay beyond the queued windows
 * the handle is filled from the host's positions.  On any error *positions_out is NULL and the result zeroed. */
int lmn_col_fri_close_keep(lmn_ctx* ctx, const lmn_col* last_layer, const uint8_t start_digest[32],
                           uint32_t log_query_domain, lmn_fri_close_result* result, lmn_positions** positions_out);
/* Opens up to 64 trees at the positions of a handle with ONE plan launch (k_open_plan, one workgroup per item, followed
 * by a one-workgroup offset step), ONE fetch launch, one transfer and one wait: MerkleProver::decommit's walk and FRI's
 * pair expansion run on the device, no walk runs on the host, and the host need not know the positions at all.
 * An item is a tree with the handles it was committed from (`cols`, as for lmn_tree_decommit).  Its groups are, for every
 * log size at which the tree has columns, fold_positions(positions, log_domain - log size) (csrc/openings.h): without flags its three
 * Merkle outputs equal lmn_tree_decommit's for those groups.  LMN_OPEN_FRI_PAIRS (a FRI layer's tree: 4 coordinate
 * columns at each of its sizes) first expands every group to sibling pairs - position p contributes 2 floor(p / 2) and
 * 2 floor(p / 2) + 1, FriProver::decommit's rule at fold step 1 - and fri_witness receives 4 words (a, b, c, d) per
 * pair member that is no position itself, sizes descending, members ascending.  out: n_items results, every pointer
 * from malloc and released with lmn_free, NULL with count 0 where empty.  Zero positions or zero items: LMN_OK, empty
 * outputs, nothing launched.
 * LMN_ERR_INVALID_ARGUMENT with a text naming the argument, all outputs zeroed, nothing launched, context and handles
 * usable: a null pointer where a count is non-zero, more than 64 items, a tree larger than 2^log_domain, columns that
 * differ from what the tree was committed from, LMN_OPEN_FRI_PAIRS (or an unknown flag) on a tree that does not have
 * exactly 4 columns at each of its sizes or has columns of log size 0, an upper bound of the opening (computed from the
 * number of positions, before they are looked at) above the 12 MiB one call carries, a sharded context. */
#define LMN_OPEN_FRI_PAIRS 1u
struct lmn_open_item {
  const lmn_tree* tree;
  const lmn_col* const* cols;
  uint32_t n_cols;
  uint32_t flags;
};
typedef struct lmn_open_item lmn_open_item;
struct lmn_opening {
  uint32_t* queried_values;
  uint8_t* hash_witness;     /* 32 bytes per hash */
  uint32_t* column_witness;
  uint32_t* fri_witness;
  uint64_t n_values, n_hashes, n_column_words, n_fri_words;
};
typedef struct lmn_opening lmn_opening;
int lmn_open_queries(lmn_ctx* ctx, const lmn_positions* positions, const lmn_open_item* items, uint32_t n_items,
                     lmn_opening* out /* n_items */);
/* Counters of a context since its creation, in lmn_batch_counter's numbering where it applies - 7: proof-of-work grinds
 * started on the device, 8: host waits spent inside grind rounds, 9: proofs whose transcript was closed on the device
 * (lmn_prove under LMN_DEVICE_FRI_CLOSE=1 at pow_bits >= LMN_POW_DEVICE_MIN_BITS, unsharded), 10: those among them whose nonce
 * lay beyond the queued windows (the host went on grinding), 11: proofs whose openings were planned on the device
 * (LMN_DEVICE_DECOMMIT=1 where 9 counts), 12: those among them that fell back to the host plan (no nonce in the queued
 * windows).  Diagnostic only, outside lmn_batch_counter's numbering and not part of what a binding needs - 13: k_open_plan
 * launches made for lmn_open_queries (counted where the launch is made), 14: its k_open_fetch launches, 15: its host
 * waits; 16 - 19: lmn_verify_many's proofs judged by the device stage, stage-2 proofs, launches and host waits;
 * 22: proofs whose quotient tables were made on the device (k_quot_prepare), 23: unsharded proofs with the device
 * transcript that kept the host's wait for the sampled values instead (LMN_HOST_QUOT=1, or more distinct LDE sizes or
 * samples than the kernel plans for).  Any other number, or a null context: 0. */
uint64_t lmn_ctx_counter(const lmn_ctx* ctx, int which);
int lmn_col_accumulate(lmn_ctx* ctx, lmn_col* dst, const lmn_col* src);     /* AccumulationOps::accumulate: dst += src (same shape) */
/* FieldOps<BaseField>::batch_inverse and FieldOps<SecureField>::batch_inverse on whole columns, on the device.
 *   lmn_col_batch_inverse:        dst[j][i] = src[j][i]^-1 in M31 for every column j and row i.
 *   lmn_col_batch_inverse_secure: src, dst = 4 coordinate columns (SecureColumnByCoords); element i is
 *                                 (src[0][i], src[1][i], src[2][i], src[3][i]) in QM31.
 * Shape: dst has src's ncols and log_size; the secure form needs ncols == 4; every log size from 0 to 27 is accepted;
 *   views (lmn_col_view) are accepted on either side.
 * Aliasing: dst may be src itself, or a handle over exactly the same device range (the in-place form), or disjoint from
 *   src; ranges that overlap without being identical are refused.
 * Zero: stwo's inverse() panics on zero; a device op cannot panic per element, so a zero element's result is 0, it
 *   changes no other element's result, and zero elements are counted.  n_zero_out == NULL: the call enqueues the work on
 *   the context's stream and returns, as the other column ops do.  n_zero_out != NULL: the call waits and writes the
 *   number of zero elements - words for the M31 form, QM31 elements for the secure form (an element is zero exactly when
 *   its norm down to M31 is zero: QM31 is a field).
 * Words: inputs are canonical by the handle's contract; every output word is canonical (< 2^31 - 1).
 * Errors: a null handle, a shape mismatch, a secure form on a handle that is not 4 columns, a partial overlap give
 *   LMN_ERR_INVALID_ARGUMENT with a text (lmn_last_error) that names the argument; they are raised before anything is
 *   launched, nothing is written, and the context and the handles stay usable. */
int lmn_col_batch_inverse(lmn_ctx* ctx, const lmn_col* src, lmn_col* dst, uint64_t* n_zero_out);
int lmn_col_batch_inverse_secure(lmn_ctx* ctx, const lmn_col* src, lmn_col* dst, uint64_t* n_zero_out);
/* QuotientOps::accumulate_quotients (one LDE size; samples and limits as in lmn_op_accumulate_quotients: at most 4
 * distinct sample points and 512 samples, else LMN_ERR_INVALID_ARGUMENT): out = 4 coordinate columns */
int lmn_col_accumulate_quotients(lmn_ctx* ctx, const lmn_col* const* cols, uint32_t n, const uint32_t* sample_col,
                                 const uint32_t* sample_point, const uint32_t* sample_values, uint32_t nsamples,
                                 const uint32_t* points_xy, uint32_t npoints, const uint32_t alpha[4], lmn_col** out);
int lmn_col_fold_line(lmn_ctx* ctx, const lmn_col* src, const uint32_t alpha[4], lmn_col** out);       /* FriOps::fold_line */
int lmn_col_fold_circle_into_line(lmn_ctx* ctx, lmn_col* dst, const lmn_col* src, const uint32_t alpha[4]); /* FriOps::fold_circle_into_line */
/* FriOps::decompose: f = g + lambda * v_n on a circle domain in bit-reversed order; lambda = (sum of the first
 * half - sum of the second half) / 2^log_size, g = f - lambda on the first half and f + lambda on the second. */
int lmn_col_decompose(lmn_ctx* ctx, const lmn_col* f, lmn_col** g_out, uint32_t lambda_out[4]);

/* ---- The two per-component stages of `prove` that stwo's constraint framework runs on the backend's columns:
 * with these, the level-2 surface alone reproduces a proof (tests/test_level2_only_prove.py proves examples/simple
 * with lmn_col_* / lmn_tree_* and a host channel and gets the reference's 4 876 known-answer bytes).
 *
 * `elems`: the relation element sets drawn after the main commitment, LMN_N_ELEMS x 8 words: for set e (0 NodeElements,
 * 1 RangeCheck, 2 Sin, 3 Exp2, 4 Log2 - crates/air/src/components/mod.rs:216-235, lookups/mod.rs:44-51) z at
 * elems[8e .. 8e+4) and alpha at elems[8e+4 .. 8e+8).  Sets the component does not use are ignored. */
#define LMN_N_ELEMS 5
/* InteractionClaimGenerator::write_interaction_trace (/root/reference/crates/air/src/components/add/witness.rs:126-167
 * and its 16 siblings) = stwo `LogupTraceGenerator::{new_col, write_frac, finalize_col, finalize_last}` for the
 * relations of component `kind` (LMN_KIND_*): `main` = the component's trace columns on the trace domain (n_cols x 2^k,
 * `Column::index()` order), `pre` = its preprocessed columns (lookup components; NULL otherwise).  Returns the
 * interaction trace (4 base columns per relation, the last group prefix-summed in coset order) and its claimed sum. */
int lmn_col_logup(lmn_ctx* ctx, uint32_t kind, const lmn_col* main, const lmn_col* pre, const uint32_t* elems,
                  lmn_col** interaction_out, uint32_t claimed_sum_out[4]);
/* FrameworkComponent::evaluate_constraint_quotients_on_domain for component `kind`
 * (/root/reference/crates/air/src/components/add/component.rs:38-116 and siblings; components/mod.rs:122,530): on the
 * evaluation domain of log size k + 1 (= the committed LDE at blow-up 2), every constraint of the component times its
 * power of the composition randomness times 1/Z, accumulated into `acc` (4 coordinate columns x 2^(k+1), `acc += ...`:
 * DomainEvaluationAccumulator's column for that size).  `main_lde` / `inter_lde` / `pre_lde`: the component's trace,
 * interaction and preprocessed columns on that domain; `coeffs`: n_coeffs x 4 words, the power of alpha that multiplies
 * constraint i of this component (local constraints in `evaluate` order, then one per relation);
 * `claimed_sum`: the component's claimed logup sum. */
int lmn_col_composition(lmn_ctx* ctx, uint32_t kind, const lmn_col* main_lde, const lmn_col* inter_lde,
                        const lmn_col* pre_lde, const uint32_t* elems, const uint32_t claimed_sum[4],
                        const uint32_t* coeffs, uint32_t n_coeffs, lmn_col* acc);
/* number of constraint slots the kernels of component `kind` emit (local + one per relation; the KAT-era shape:
 * eval_fixed_mul two slots, eval_fixed_recip / _sqrt / _rem one) and of its relations */
uint32_t lmn_kind_constraints(uint32_t kind);
uint32_t lmn_kind_relations(uint32_t kind);
/* Those slots under the constraint-form bits of `protocol_flags` (LMN_PV_*_SLOT(S), LMN_PV_*_NEG; since ABI version 6):
 * proto_index_out[k] = index of kernel slot k among the component's constraints in the protocol (-1: the protocol has no
 * such constraint, its coefficient is 0), sign_out[k] = +1 / -1 (the coefficient of slot k is sign * alpha^(N-1-i) for
 * global constraint index i); 16 entries each.  Returns the number of constraints the component contributes to the
 * composition polynomial under these flags (0: unsupported kind).  What lmn_col_composition's caller builds `coeffs` from. */
uint32_t lmn_kind_constraint_layout(uint32_t kind, uint32_t protocol_flags, int32_t proto_index_out[16], int32_t sign_out[16]);

#ifdef __cplusplus
}
#endif
#endif /* LUMINAIR_HIP_H */
