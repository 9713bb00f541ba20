// Launch wrappers for the gfx950 kernels of the prove hot path.
// All pointers are device pointers; all launches are asynchronous on `s`.
#pragma once
#include "blake2s.h"
#include "field.h"

namespace lmn {

constexpr int MAX_LOG = 30;

// Per-layer twiddle pointers of one canonic circle domain (layer 0 = circle/y layer).  d[i] = the same table with
// every entry doubled (2w < 2^32): the fixed-shape FFT kernels multiply by 2w so that the 64-bit product splits into
// floor(x w / 2^31) (high word) and 2 (x w mod 2^31) (low word) without a funnel shift (fft_fixed.hip).
struct TwPtrs {
  const uint32_t* l[MAX_LOG];
  const uint32_t* d[MAX_LOG];
};

// ---- a3: AoS rows -> padded SoA columns (write_trace / pack_values)
struct PadRow {
  uint32_t v[32];  // the component's padding row (e.g. add/table.rs:40-58)
};
// Trace reuse (phase_trace.cpp run_main_trace): which columns of a launch may keep what the previous proof left in their
// blocks.  Column c is skipped when it is a candidate (bit c of candidate_mask) and changed[c] != epoch; the comparing
// transpose stores `epoch` into changed[c] when a word of a candidate column differs from the word it is about to
// overwrite.  changed == nullptr: every column is worked on.
struct ColSkip {
  const uint32_t* changed = nullptr;
  uint32_t epoch = 0;
  uint32_t candidate_mask = 0;
};
// In a kernel: column c keeps what the previous proof left in its blocks.  c is workgroup-uniform (it comes from blockIdx),
// so the mark arrives through a uniform load and every lane of the workgroup takes the same branch.
LMN_HD bool col_skipped(const ColSkip& k, int c) {
  return k.changed != nullptr && ((k.candidate_mask >> c) & 1u) != 0u && k.changed[c] != k.epoch;
}
constexpr int CHANGED_WORDS = 128;   // a proof's changed[] words, all tables together (tables beyond them are not compared)
void launch_transpose_pad(const uint32_t* rows, uint64_t n_rows, int ncols, int log_size, uint32_t* cols,
                          const PadRow& pad, uint32_t* bad_flag /* device word, set when a value >= P */, lmn_stream_t s);
// only rows [blk_row0, blk_row0 + blk_rows) of the padded table (blk_row0 a multiple of 64); columns out_stride apart
void launch_transpose_pad_rows(const uint32_t* rows, uint64_t n_rows, int ncols, int log_size, uint32_t* cols,
                               uint64_t out_stride, uint64_t blk_row0, uint64_t blk_rows, const PadRow& pad, uint32_t* bad_flag,
                               lmn_stream_t s,
                               uint32_t bad_value = 1u /* what a non-canonical word writes to *bad_flag */);
// The comparing form, whole tables only (`cols` hold the previous proof's columns): a word of a column of `cmp_mask` is
// read before it is stored and stored only if it differs; a wave that saw a difference writes `epoch` to changed[column].
// Columns outside the mask are stored as launch_transpose_pad stores them.
void launch_transpose_pad_compare(const uint32_t* rows, uint64_t n_rows, int ncols, int log_size, uint32_t* cols,
                                  const PadRow& pad, uint32_t* bad_flag, uint32_t bad_value, uint32_t cmp_mask,
                                  uint32_t* changed, uint32_t epoch, lmn_stream_t s);
// Row sinks (lmn_rows_*): one CHUNK of rows - its row 0 is table row r0, any r0, any length n >= 1 - transposed into
// columns `stride` words apart.  `chunk` may be page-locked HOST memory in its device view (read over the link, once).
// chunk == nullptr: rows [r0, r0 + n) receive the padding row instead.  A non-canonical word sets *bad_word to 1.
constexpr int CHUNK_ROWS = 256;      // table rows per workgroup, aligned in the DESTINATION: every full tile stores 1 KB runs
constexpr int CHUNK_MAX_COLS = 30;   // CHUNK_ROWS * (ncols | 1) * 4 B of LDS <= 31 744 B: two workgroups per CU and more
void launch_rows_chunk(const uint32_t* chunk, uint64_t r0, uint64_t n, int ncols, uint32_t* cols, uint64_t stride,
                       const PadRow& pad, uint32_t* bad_word, lmn_stream_t s);
// lmn_settings_prepare: the tree-0 columns of a prepared settings object, checked and completed where they lie.  Column
// c < n_luts (a LUT column of n[c] words): *flag = c + 1 if it holds a word that is not a canonical M31 (any such column
// may win).  range_check (may be null): row r of its range_n rows is set to r.
constexpr int PREPARE_MAX_LUT_COLS = 6;
struct PrepareCols {
  const uint32_t* lut[PREPARE_MAX_LUT_COLS];
  uint32_t n[PREPARE_MAX_LUT_COLS];
  int n_luts;
  uint32_t* range_check;
  uint32_t range_n;
};
void launch_settings_prepare(const PrepareCols& cols, uint32_t* flag, lmn_stream_t s);

// ---- a4: circle FFT passes.  data = ncols columns of 2^log_n words at stride col_stride.
// dst may equal src (in place).  launch_fft zero-extends src (2^log_src words) to 2^log_n (LDE).
// Both return the number of pass kernels launched.
int launch_ifft(uint32_t* dst, uint64_t dst_stride, const uint32_t* src, uint64_t src_stride, int ncols, int log_n,
                const TwPtrs& itw, lmn_stream_t s);
int launch_fft(uint32_t* dst, uint64_t dst_stride, const uint32_t* src, uint64_t src_stride, int log_src, int ncols,
               int log_n, const TwPtrs& tw, lmn_stream_t s);
// interpolate + extend by one bit in three launches (the strided passes of both transforms fused): evals (2^log_n) ->
// coeffs (2^log_n, kept) and lde (2^(log_n+1)).  itw: inverse twiddles of domain log_n; tw_ext: twiddles of log_n + 1.
bool fft_interp_extend_supported(int log_n);
// skip.changed != nullptr: the workgroups of a skipped column (ColSkip) leave all three launches before their first load.
int launch_interp_extend(uint32_t* coeffs, uint64_t coeff_stride, const uint32_t* evals, uint64_t evals_stride, uint32_t* lde,
                         uint64_t lde_stride, int ncols, int log_n, const TwPtrs& itw, const TwPtrs& tw_ext, lmn_stream_t s,
                         const ColSkip& skip = ColSkip{});
// The same for a polynomial of 2^log_half coefficients given by its evaluations on storage rows [0, 2^log_half) of the
// 2^(log_half + 1)-point domain (itw_full: that domain's inverse tables), extended onto the 2^(log_half + 2)-point domain
// (tw_ext): the inverse low pass and the strided pass that writes four quarters (2 launches); launch_interp_extend_half_finish
// is the forward low pass (1 launch).  Between the two, element 0 of the coefficients can still be changed: add the change to
// the words at multiples of 2^12 of each quarter.  Sizes: fft_interp_extend_supported(log_half).
int launch_interp_extend_half(uint32_t* coeffs, uint64_t coeff_stride, const uint32_t* evals, uint64_t evals_stride,
                              uint32_t* lde, uint64_t lde_stride, int ncols, int log_half, const TwPtrs& itw_full,
                              const TwPtrs& tw_ext, lmn_stream_t s);
int launch_interp_extend_half_finish(uint32_t* lde, uint64_t lde_stride, int ncols, int log_half, const TwPtrs& tw_ext,
                                     lmn_stream_t s);
// The same from the table's AoS rows (transpose fused into the inverse low pass; launch_transpose_pad's padding and
// canonical-word check included).  false: not applicable to this size / build (transpose first, then launch_interp_extend).
struct PadRow;
bool launch_interp_extend_rows(uint32_t* coeffs, uint64_t coeff_stride, const uint32_t* rows, uint64_t n_rows, const PadRow& pad,
                               uint32_t* bad_flag, uint32_t bad_value, uint32_t* lde, uint64_t lde_stride, int ncols, int log_n,
                               const TwPtrs& itw, const TwPtrs& tw_ext, lmn_stream_t s);
// forward transform restricted to block `block` of 2^log_blocks equal row blocks of the 2^log_n domain (tw = the
// twiddles of the whole domain); dst receives 2^(log_n - log_blocks) words per column
int launch_fft_block(uint32_t* dst, uint64_t dst_stride, const uint32_t* src, uint64_t src_stride, int log_src, int ncols,
                     int log_n, int log_blocks, uint32_t block, const TwPtrs& tw, lmn_stream_t s);
// Row blocks of `ncols` columns (column stride src_stride, blocks of block_rows rows) packed per destination rank for
// the all-to-all of a sharded commitment: dst[((s * ncols + c) * nsel + h) * block_rows + i] =
// src[c * src_stride + sel.blk[s][h] * block_rows + i] for s < world, h < nsel.
struct PackSel {
  uint32_t blk[8][2];
};
void launch_pack_blocks(const uint32_t* src, uint64_t src_stride, uint32_t* dst, uint32_t block_rows, int ncols, int nsel,
                        int world, const PackSel& sel, lmn_stream_t s);
// the inverse with one block per rank: cols[c * col_stride + r * block_rows + i] = packed[(r * ncols + c) * block_rows + i]
void launch_unpack_blocks(const uint32_t* packed, uint32_t* cols, uint64_t col_stride, uint32_t block_rows, int ncols, int world,
                          lmn_stream_t s);
// single-layer reference kernels (debug / self-test only)
void launch_fft_simple(uint32_t* data, uint64_t col_stride, int ncols, int log_n, const TwPtrs& tw, bool inverse,
                       lmn_stream_t s);
// dst (2^log_dst per column) <- src coefficients (2^log_src per column) zero-extended
void launch_extend(const uint32_t* src, uint64_t src_stride, int log_src, uint32_t* dst, uint64_t dst_stride,
                   int log_dst, int ncols, lmn_stream_t s);

// ---- level-2 column ops (stwo ColumnOps / FriOps pieces that `prove` itself never needs as separate passes)
// in-place bit-reversal permutation of every column (ColumnOps::bit_reverse_column)
void launch_bit_reverse(uint32_t* data, uint64_t col_stride, int ncols, int log_n, lmn_stream_t s);
// FriOps::decompose of a secure column f (4 x 2^log_n): lambda_out[0] = (sum of first half - sum of second half) / 2^log_n;
// g = f - lambda on the first half, f + lambda on the second.  scratch: decompose_num_blocks(log_n) QM31 values.
int decompose_num_blocks(int log_n);
void launch_decompose(const uint32_t* f, int log_n, uint32_t* g, QM31* lambda_out, QM31* scratch, lmn_stream_t s);
// FieldOps::batch_inverse of whole columns: dst[j][i] = src[j][i]^-1 for ncols columns of 2^log_n words col_stride words
// apart (M31), or of ONE secure column given as 4 coordinate columns 2^log_n words apart (QM31).  A zero element gives 0
// and is added to *n_zero (a device word the caller cleared; nullptr: not counted).  dst == src is the in-place form.
void launch_batch_inverse_m31(const uint32_t* src, uint32_t* dst, uint64_t col_stride, int ncols, int log_n,
                              unsigned long long* n_zero, lmn_stream_t s);
void launch_batch_inverse_qm31(const uint32_t* src, uint32_t* dst, int log_n, unsigned long long* n_zero, lmn_stream_t s);

// ---- a4: Blake2s Merkle layer.  out[i] = H(prev[2i] || prev[2i+1] || cols[0][i] .. cols[ncols-1][i])
void launch_merkle_layer(const uint32_t* prev, const uint32_t* const* cols, int ncols, uint32_t size, uint32_t* out,
                         lmn_stream_t s);

// ---- device-resident channel (FRI commit loop): digest <- H(digest || root); alpha <- draw_felt()
struct DevChannel {
  uint32_t digest[8];
  uint32_t n_sent;
  uint32_t variant;   // draw encoding: 0 = digest || counter padded to 32 bytes (KAT), 1 = digest || u32 counter || 0x00 (LMN_PV_DRAW_CTR_U32)
};
void launch_chan_mix_root_draw(DevChannel* ch, const uint32_t* root, QM31* out_alpha, uint32_t* root_copy,
                               lmn_stream_t s);

// ---- device-resident Fiat-Shamir of the commitment phases (phase_trace / _logup / _composition / _oods.cpp): the host
// enqueues a whole proof up to the sampled values without waiting; these single-workgroup kernels do the transcript steps
// in between on a DevChannel and leave what the next kernels need in device memory.  The host replays the same steps on
// its own Channel once the values have arrived and cross-checks every draw.
constexpr int CHAN_N_ELEMS = 5;              // relation element sets (prover.h ELEMS_*)
struct DevElems {                            // z / alpha of every set, written by the ChanStep of kind 1 (or uploaded by the host)
  QM31 z[CHAN_N_ELEMS], alpha[CHAN_N_ELEMS];
};
// Everything the host needs back from the device-resident steps, in one place: ONE download at the proof's first wait
struct DevReport {
  DevElems elems;
  QM31 comp_alpha, t;
  QM31 claimed[17];
  uint32_t roots[3][8];                      // main, interaction, composition tree
  uint32_t bad;                              // copy of the transposes' non-canonical-word verdict
  uint32_t pad[3];
  // trace reuse: copy of the first ChanStep::changed_words words behind the verdict's two.  The words beyond them are never
  // written and never read: they hold whatever the arena held (the last step copies the whole report, 0.5 KB of it this)
  uint32_t changed[CHANGED_WORDS];
};
struct ChanElemSets {
  int n;
  int set[CHAN_N_ELEMS];                     // relation element set of each draw_felts(2); negative: drawn and discarded
};
constexpr int CHAN_MAX_INST = 17;
struct ChanCoeffPlan {
  int n_inst, n_total;
  const QM31* claimed[CHAN_MAX_INST];        // device [claimed, shift] of each component, struct order
  int16_t k0[CHAN_MAX_INST];
  int8_t n_kernel[CHAN_MAX_INST];
  int8_t proto_index[CHAN_MAX_INST][16];
  uint16_t neg[CHAN_MAX_INST];               // bit k: the protocol's constraint is minus kernel slot k
};
constexpr int CHAN_MAX_POINTS = 24;
struct ChanOodsPlan {
  int n_points, n_maps;
  uint32_t step_x[CHAN_MAX_POINTS], step_y[CHAN_MAX_POINTS];
};
// One transcript step of the commitment phases, made by the launch that produces the tree's root (launch_merkle_small)
// or by a launch of its own (launch_chan_step):
//  kind 1  the channel starts at `start` (a launch argument instead of an upload); mix_root(root 1); one draw_felts(2) per
//          entry of `sets` -> rep->elems; rep->bad = *bad_word; rep->changed[k] = bad_word[2 + k] for k < changed_words
//  kind 2  mix_felts([claimed_i]) per component, mix_root(root 2), draw_felt() = the composition randomness alpha; then the
//          coefficient of every kernel constraint slot of every component: sign * alpha^(n_total - 1 - (k0 + proto_index)),
//          0 for a slot the protocol lacks (Context's constraint_layout) - 16 per component at coeff_out + 16 * i
//  kind 3  mix_root(root 3), t = draw_felt(), the OODS point ((1 - t^2) / (1 + t^2), 2t / (1 + t^2)), the points
//          oods + step_i (i >= 1; step_0 unused) and per point the mappings y, x, pi(x), pi^2(x), ... that
//          launch_eval_tables expands -> maps_out (n_points x n_maps); the finished report is copied to rep_host
//          (page-locked memory) by the kernel itself - no download behind it
//  kind 0  none (launch_merkle_small with a channel: mix_root + the draw of a folding alpha, the FRI layers' step)
struct ChanStep {
  int kind;
  DevChannel start;
  const uint32_t* bad_word;
  ChanElemSets sets;
  ChanCoeffPlan coeff;
  QM31* coeff_out;
  ChanOodsPlan oods;
  QM31* maps_out;
  uint32_t* rep_host;
  DevReport* rep;
  // kind 3 also copies `copy_words` words from page-locked memory to device memory (the evaluation kernels' job table)
  const uint32_t* copy_src;
  uint32_t* copy_dst;
  uint32_t copy_words;
  uint32_t changed_words;   // kind 1
};
// The kernels take the step as a device-visible pointer (+ its kind by value) and fetch it into LDS with one load per lane:
// page-locked host memory serves (one round trip, behind the launch's first loads).  check_chan_step validates a plan.
void check_chan_step(const ChanStep& step);
void launch_chan_step(DevChannel* ch, const ChanStep* step, int step_kind, const uint32_t* root, lmn_stream_t s);

// fused subtree variants: start level (children hashes and/or its own columns) + plain levels above.
// The start level's columns are given as runs of contiguous equal-size columns.
constexpr int MERKLE_MAX_SEG = 4;
constexpr int MERKLE_MAX_SUB = 3;     // per-lane register subtree: 2^3 start nodes
constexpr int MERKLE_MAX_FUSED = 11;  // levels above the start level covered by one launch
struct MerkleSegs {
  const uint32_t* base[MERKLE_MAX_SEG];
  int n[MERKLE_MAX_SEG];
};
struct MerkleLevels {
  uint32_t* p[MERKLE_MAX_FUSED + 1];  // p[0] = start level output, p[l] = l levels above it
};
// FRI layers: the leaves of a layer's tree are the fold of the previous layer.  With `fold` given, the start level
// computes leaf i = fold(src[2i], src[2i+1]) itself (FriOps::fold_line / fold_circle_into_line without an
// accumulator), writes it to dst (the layer's 4 coordinate columns, which later steps read) and hashes it - one
// launch and one pass over the layer less than fold kernel + leaf hashing.
struct MerkleFold {
  const uint32_t* src;   // previous layer / quotient column: 4 coordinate columns of 2*size words, stride 2*size
  const uint32_t* itw;   // inverse twiddles of the fold (one per leaf)
  const QM31* alpha;     // device: the folding randomness drawn by the previous layer's channel step
  uint32_t* dst;         // this layer: 4 coordinate columns of `size` words, stride `size`
  // A quotient column of 2*size rows that joins this layer (fold_circle_into_line with accumulation, same alpha):
  // leaf i = fold(src)[i] * alpha^2 + fold(src2)[i]; null if none
  const uint32_t* src2;
  const uint32_t* itw2;
  // Not a fold - a tree whose largest level (2*size leaves of `below_ncols` <= 8 contiguous columns, no children) sits
  // directly under a level with columns of its own: the start level hashes its two leaves itself instead of reading
  // their hashes, so the leaf level is neither written nor read back (2 x 32 B per leaf) and needs no launch.
  const uint32_t* below;
  int below_ncols;
};
void launch_merkle_fused(const uint32_t* prev, const MerkleSegs& sg, int ncols, uint32_t size,
                         const MerkleLevels& outs, int sub, int nfused, lmn_stream_t s, const MerkleFold* fold = nullptr);
// one block, size <= 1024 start nodes, nfused <= 10
// If `ch` is given and this launch reaches the root, it also makes the transcript step that consumes the root: without
// `step`, mix_root and the draw of the next felt (saves a launch per FRI layer); with it, that ChanStep.
void launch_merkle_small(const uint32_t* prev, const MerkleSegs& sg, int ncols, uint32_t size,
                         const MerkleLevels& outs, int nfused, DevChannel* ch, QM31* alpha_out, uint32_t* root_copy,
                         lmn_stream_t s, const ChanStep* step = nullptr, int step_kind = 0);

// FRI tail: layers of log size first_log, first_log-1, ... (n_layers of them, all <= 2^10) committed
// and folded in one single-block launch.  layers[li].next is the evaluation buffer of the next layer.
struct FriTailLayer {
  const uint32_t* vals;        // 4 x 2^L line evaluation (coordinate-major)
  uint32_t* next;              // 4 x 2^(L-1): fold output
  const uint32_t* itw;         // 1/x twiddles of the line domain of log size L
  uint32_t* merkle[11];        // merkle[l]: 2^l hashes, l = 0..L
};
// What the tail does at its two ends besides its layers.
// In front (src != null): its first layer does not exist yet - it is the line fold of `src` (2^(first_log+1) values,
// 1/x twiddles `itw`, folding randomness *alpha), computed by the tail itself (and written to layers[0].vals).
// Behind (out_mirror != null): when the tail is done it copies the FRI loop's result block (`out_words` words at out_block:
// roots | alphas | last layer, written by this and the earlier launches) to page-locked memory - no download behind it
struct FriTailIo {
  const uint32_t* src;
  const uint32_t* itw;
  const QM31* alpha;
  const uint32_t* out_block;
  uint32_t* out_mirror;
  uint32_t out_words;
};
void launch_fri_tail(DevChannel* ch, const FriTailLayer* layers, int n_layers, int first_log, QM31* alphas_out,
                     uint32_t* roots_out, lmn_stream_t s, const FriTailIo* io = nullptr);

// ---- twiddle tables on the device (a11): entry h of a table of 2^bits entries is the y (coord 0) or x (coord 1)
// coordinate of the point init + bit_reverse(h, bits) * step of a half coset; sx / sy = step * 2^k.  Four forms are written:
// the value, its inverse, and both doubled (TwPtrs::d).
struct TwGen {
  uint32_t ix, iy;
  uint32_t sx[30], sy[30];
};
void launch_twiddles(int bits, const TwGen& g, int coord, uint32_t* tw, uint32_t* itw, uint32_t* tw2, uint32_t* itw2,
                     lmn_stream_t s);

// ---- gather: out[dst_off[e] + k] = base[src_off[e] + k], k < len[e]; base = the context's arena, or - for an entry whose
// src_off carries GATHER_SHARED - the slab of the proof's prepared settings (lmn_settings_prepare), which lies outside
// every arena
constexpr uint64_t GATHER_SHARED = 1ull << 63;
struct GatherEntry {
  uint64_t src_off;  // word offset into the arena, or GATHER_SHARED | word offset into the shared slab
  uint32_t len;      // words
  uint32_t dst_off;  // word offset into out
};
// A Merkle node that was never written (a fused launch leaves the levels its lanes keep in registers - 7/8 of a big
// tree's hashes, of which a proof reads a few dozen - out of HBM): recomputed for the decommitment from the launch's
// start level.  node = index at `depth` (0..2) levels above that start level; the 8 words go to out[dst_off..].
struct MerkleRecompute {
  const uint32_t* prev;  // start level of the launch that skipped the node (as given to launch_merkle_fused)
  MerkleSegs sg;
  int ncols;
  uint32_t size;
  const uint32_t* below; // MerkleFold::below of that launch (children = hashes of two leaves), or null
  int below_ncols;
  uint32_t node;
  int depth;
  uint32_t dst_off;
};
void launch_gather(const uint32_t* arena, const uint32_t* shared, const GatherEntry* entries, uint32_t n_entries,
                   const MerkleRecompute* jobs, uint32_t n_jobs, uint32_t* out, lmn_stream_t s);

// ---- decommitment of a level-2 tree (lmn_tree_decommit): the tree's slab and the column handles are separate
// allocations, so an entry names its source through a table of base pointers instead of an arena offset.  The plan holds
// n_hashes hash entries, then n_words word entries; out = n_hashes x 8 words, then n_words words:
//   hash entry t:  out[8t .. 8t+8)        = src[plan[t].src][8 * idx .. 8 * idx + 8)   (src[..] and out 32-byte aligned)
//   word entry t:  out[8 * n_hashes + t'] = src[plan[t].src][idx],  t' = t - n_hashes
struct DecommitEntry {
  uint32_t src;  // index into the pointer table: a tree layer (hash entries) or a column in tree order (word entries)
  uint32_t idx;  // node
};
void launch_tree_decommit(const uint32_t* const* src, const DecommitEntry* plan, uint32_t n_hashes, uint32_t n_words,
                          uint32_t* out, lmn_stream_t s);
// out[j * n + i] = cols[j * 2^log_size + positions[i]], j < ncols (lmn_col_gather)
void launch_col_gather(const uint32_t* cols, uint32_t log_size, uint32_t ncols, const uint32_t* positions, uint32_t n,
                       uint32_t* out, lmn_stream_t s);

// ---- openings planned on the device (lmn_open_queries): MerkleProver::decommit's walk and FRI's pair expansion, restated
// as a kernel that reads the query positions where they were born - in device memory - so that no host walk stands
// between the positions and the fetch.  Three launches behind each other, no wait in between:
//   k_open_plan     one workgroup per item (a tree to open): walks the layers, writes the item's four counts and its
//                   entries (OpenEntry) into the item's region of the plan table
//   k_open_offsets  one workgroup: the items' counts -> compact word offsets in the proof's order (per item: FRI
//                   witness, queried values, hash witness, column witness; items in launch order)
//   k_open_fetch    one lane per entry over the host's upper bound; an item's entry count is read from device memory
//                   and surplus workgroups return at once
constexpr uint32_t OPEN_MAX_POSITIONS = 1024;   // = FRI_CLOSE_MAX_QUERIES
constexpr uint32_t OPEN_MAX_NODES = 2048;       // a layer's node set: the positions, pair-expanded
constexpr uint32_t OPEN_MAX_ITEMS = 64;
constexpr uint32_t OPEN_MAX_LOG = 31;
constexpr uint32_t OPEN_FRI_PAIRS = 1u;         // = LMN_OPEN_FRI_PAIRS
constexpr uint32_t OPEN_EMPTY = 1u << 31;       // an item without a tree (a proof's tree 0 without lookups): four empty lists
constexpr uint32_t OPEN_STORED = 0xffu;         // OpenItemDesc::cut_of_layer: the layer lies in memory
enum { OPEN_LIST_FRI = 0, OPEN_LIST_QUERIED = 1, OPEN_LIST_HASH = 2, OPEN_LIST_WITNESS = 3 };
// what the host knows of an item before the positions exist
struct OpenItemDesc {
  uint32_t max_log, flags;
  uint32_t layer_src0;   // pointer-table index of layer 0; layer l is layer_src0 + l
  uint32_t col_src0;     // pointer-table index of the first column, columns in tree order (size descending)
  uint32_t ent_off, ent_cap;           // the item's region of the plan table, in entries
  uint32_t job_off, job_cap;           // its region of the recompute table (hashes of layers a fused launch never stored)
  uint32_t ncols[OPEN_MAX_LOG + 1];    // columns per log size
  uint8_t cut_of_layer[OPEN_MAX_LOG + 1];   // OPEN_STORED, or the index of the layer's MerkleCut in the launch's cut table
};
// what the device writes per item: count[list] in words (hashes: in hashes), then - by k_open_offsets - base[list], the
// word offset of the list in the output
struct OpenItemHeader {
  uint32_t count[4];
  uint32_t n_entries, overflow, n_jobs, pad;
  uint32_t base[4];
  uint32_t pad2[4];
};
struct OpenHeader {        // in front of the items' headers; the output's first bytes
  uint32_t overflow;       // an item's plan exceeded its region or the node set, or the lists exceed out_cap_words
  uint32_t total_words, n_positions, pad;
};
struct OpenEntry {
  uint32_t src;   // index into the pointer table
  uint32_t idx;   // node (hash entries: 8 words at 8 * idx) or row
  uint32_t dst;   // word offset inside the item's list
  uint32_t list;  // OPEN_LIST_*
};
// *count = the number of positions (clamped to OPEN_MAX_POSITIONS), positions = ascending and distinct; found (may be null):
// the plan is made only if *found == 1 (FriCloseHeader::found: without a nonce k_fri_queries wrote no positions).
// A hash of a layer that is not stored goes to `jobs` instead of `entries`: src = the cut's index, idx = the node,
// list = OPEN_LIST_HASH | depth << 8 (levels above the cut's start level), fetched by launch_open_recompute from `cuts`
// (MerkleRecompute templates: node, depth and dst_off unused).  *n_launched (may be null) counts the launches made.
void launch_open_plan(const uint32_t* count, const uint32_t* positions, const uint32_t* found, uint32_t log_domain,
                      const OpenItemDesc* items, uint32_t n_items, OpenItemHeader* headers, OpenEntry* entries, OpenEntry* jobs,
                      lmn_stream_t s, uint64_t* n_launched = nullptr);
void launch_open_offsets(const uint32_t* count, OpenHeader* header, OpenItemHeader* headers, uint32_t n_items,
                         uint32_t out_cap_words, lmn_stream_t s);
void launch_open_fetch(const uint32_t* const* src, uint32_t n_src, const OpenItemDesc* items, uint32_t n_items, uint32_t max_cap,
                       OpenHeader* header, const OpenItemHeader* headers, const OpenEntry* entries, uint32_t* out,
                       lmn_stream_t s, uint64_t* n_launched = nullptr);
struct MerkleRecompute;
void launch_open_recompute(const MerkleRecompute* cuts, uint32_t n_cuts, const OpenItemDesc* items, uint32_t n_items,
                           uint32_t max_job_cap, OpenHeader* header, const OpenItemHeader* headers, const OpenEntry* jobs,
                           uint32_t* out, lmn_stream_t s);

// ---- proofs verified in batches (lmn_verify_many; kernels_verify.h): the part of the verifier behind the query draw - the
// four trace-tree decommitments, the FRI quotients at the queried positions, the FRI layers - for many proofs at once.
// The host stages a chunk of proofs into ONE block of 32-bit words (verifier.cpp): per bucket (proofs of one claim) a
// layout table, per proof a descriptor of offsets and lengths into the block.  Two launches per bucket:
//   k_verify_values  one wave per proof: quotients, sibling pairs, folds, last layer; writes the FRI trees' leaf words
//                    into the proof's scratch region of the block and the proof's values verdict
//   k_verify_trees   one workgroup per (proof, tree): MerkleVerifier::verify; writes the tree's verdict
// Every length a kernel uses is a descriptor field that the stager bounded against the block; no length is read from
// proof content, and every counter is compared with its list's length before it becomes an address.
constexpr uint32_t VM_MAX_POS = 128;     // distinct query positions of a proof the device stage takes
constexpr uint32_t VM_MAX_SIZES = 8;     // distinct column sizes of a claim
constexpr uint32_t VM_MAX_TREES = 36;    // 4 trace trees + the first FRI layer + the inner layers
constexpr uint32_t VM_MAX_NODES = 2 * VM_MAX_POS;   // a level's node set: the positions, pair-expanded
constexpr uint32_t VM_NONE = 0xffffffffu;
// A verdict word is VM_DONE | failure bits: a word without the tag was never written (the host refuses it).
constexpr uint32_t VM_DONE = 0x564d0000u, VM_DONE_MASK = 0xffff0000u;
enum : uint32_t {
  VM_FAIL_FOLDS = 1u,            // values: the last layer's polynomial does not reproduce a folded value
  VM_FAIL_QUERIED_SHAPE = 2u,    // values: a queried value lies beyond its list
  VM_FAIL_DENOMINATOR = 4u,      // values: degenerate quotient denominator
  VM_FAIL_WITNESS_SHORT = 8u,    // values: a FRI witness ran out
  VM_FAIL_WITNESS_LONG = 16u,    // values: a FRI witness has elements left over
  VM_FAIL_POSITIONS = 32u,       // values: a layer's positions do not line up with the values folded so far
  VM_FAIL_TREE = 1u,             // trees: the decommitment does not lead to the root (or a list ran out / has words left)
};
struct VmSpan {
  uint32_t off, len;   // word offset in the chunk's block; len in the list's elements (words, hashes or QM31s)
};
struct VmProof {
  VmSpan pos;                           // ascending distinct query positions in the largest domain
  VmSpan queried[4];                    // words
  VmSpan hash_wit[VM_MAX_TREES];        // hashes; trees 0-3, then the first FRI layer, then the inner layers
  VmSpan col_wit[VM_MAX_TREES];         // words
  VmSpan fri_wit[VM_MAX_TREES - 4];     // QM31s; layer 0 = the first layer
  VmSpan leaves[VM_MAX_TREES - 4];      // scratch (words): the FRI tree's queried values, as long as the positions imply
  VmSpan last;                          // QM31s: the last layer's coefficients
  uint32_t roots;                       // n_trees x 8 words
  uint32_t samples;                     // n_bcols x 4 words: the sampled values in the layout's batch-column order
  uint32_t points, n_points;            // n_points x 8 words (x, y)
  uint32_t alphas;                      // 4 words quot_alpha, then 4 words per FRI layer's fold alpha
  uint32_t qbase[4][VM_MAX_SIZES];      // offset of a size's group inside queried[tree]
  uint32_t verdict;                     // the proof's verdict words: [values, tree 0, tree 1, ...]
};
// one sampled column of a batch: queried value = queried[tree][qbase[tree][size] + query * ncol + j]
struct VmBatchCol {
  uint32_t tree, size, ncol, j;
};
struct VmBatch {
  uint32_t point, col0, col1;   // batch columns [col0, col1), the k-th of which is sampled at samples[k]
};
// What proofs of one claim share; in the block it is followed by n_batches VmBatch and n_bcols VmBatchCol.
struct VmLayout {
  uint32_t n_sizes, top, n_inner, n_trees, n_batches, n_bcols;
  uint32_t size_log[VM_MAX_SIZES];            // the LDE sizes, descending; size_log[0] == top
  uint32_t size_batch0[VM_MAX_SIZES + 1];     // batches of size s: [size_batch0[s], size_batch0[s + 1])
  uint32_t join_of_layer[VM_MAX_TREES];       // inner layer l: the size whose columns join behind its fold, or VM_NONE
  uint32_t tree_max_log[VM_MAX_TREES];        // VM_NONE: a tree without columns
  uint16_t tree_ncols[VM_MAX_TREES][32];      // columns per log size
};
// proofs: n_proofs descriptors; blk: the chunk's block (staged words | scratch | verdicts); tpb: 64, 128 or 256 lanes per
// (proof, tree), from the largest number of distinct positions.  *n_launched (may be null) counts the launches made.
void launch_verify_values(uint32_t* blk, uint32_t layout_off, uint32_t proofs_off, uint32_t n_proofs, lmn_stream_t s,
                          uint64_t* n_launched = nullptr);
void launch_verify_trees(uint32_t* blk, uint32_t layout_off, uint32_t proofs_off, uint32_t n_proofs, uint32_t n_trees,
                         uint32_t tpb, lmn_stream_t s, uint64_t* n_launched = nullptr);

// ---- proof-of-work grind (GrindOps on the device): one launch examines the nonces [base, base + 2^window_log) and
// lowers *best (device, u64) to the smallest of them that passes, if it is below what *best holds.  A block whose nonces
// all lie above *best at its start returns at once, so launches queued behind the one that found a nonce cost nothing
// and the first window with a hit yields the global minimum.  kat: the KAT form (bare compression, h = w, m0/m1 = nonce,
// t = 0, no final flag); otherwise blake2s(w || nonce LE), i.e. the hashed mix (w = digest) or the prefixed form (w = pre).
constexpr uint32_t POW_TPB = 256;       // lanes per block
constexpr uint32_t POW_NPT = 8;         // nonces per lane and launch
constexpr int POW_MIN_WINDOW_LOG = 11;  // one block: POW_TPB * POW_NPT nonces
constexpr int POW_WINDOW_LOG = 24;      // default cap of one launch's window (Context: LMN_POW_WINDOW_LOG)
constexpr int POW_DEVICE_MIN_BITS = 11; // prove() grinds on the device from this pow_bits on (LMN_POW_DEVICE_MIN_BITS; measured crossover)
// Launches queued per host wait, in device_grind, in grind_many's rounds and behind k_fri_close: one behind the launch that
// found a nonce returns at once (every block sees the smaller nonce at its start), so the queue costs a few us of launches
// and saves waits while nothing has been found.  (grind_many on 64 digests at pow_bits 20: 4 is within the spread of 8, 16
// is 5 - 8 % slower.)
constexpr int POW_WINDOWS_PER_WAIT = 8;
struct PowWords {
  uint32_t w[8];
};
void launch_pow_grind(const PowWords& w, bool kat, uint64_t base, int window_log, uint32_t pow_bits,
                      unsigned long long* best, lmn_stream_t s);
// The same for many digests at once: one launch examines [base, base + 2^window_log) for the digests
// digests[pending[y]], y < n_pending (<= 65535), and lowers best[pending[y]] (one u64 per digest, device).  A digest whose
// best already lies below a block's nonces costs that block one load.  digests, pending and best are device memory that
// nothing else writes during the launch.
void launch_grind_many(const PowWords* digests, const uint32_t* pending, uint32_t n_pending, bool kat, uint64_t base,
                       int window_log, uint32_t pow_bits, unsigned long long* best, lmn_stream_t s);

// ---- the close of the FRI transcript on the device (phase_fri.cpp enqueue_fri_close): what stands between the last
// folding alpha and the decommitment - the last layer's polynomial, its degree check, mix_felts, the proof of work, mix_u64
// and the query positions - as a chain of single-workgroup kernels with launch_grind_many's windows in between:
//   k_fri_close | POW_WINDOWS_PER_WAIT x k_grind_many (one digest) | k_fri_queries
constexpr int FRI_CLOSE_MAX_LOG = 13;        // the last layer: at most 2^(10 + 3) values (log_last_layer + log_blowup)
constexpr int FRI_CLOSE_LDS_LOG = 11;        // up to this size the interpolation's passes stay in LDS, above in `scratch`
constexpr int FRI_CLOSE_MAX_BOUND_LOG = 10;  // log_last_layer
constexpr uint32_t FRI_CLOSE_MAX_QUERIES = 1024;
struct FriCloseItw {
  const uint32_t* p[FRI_CLOSE_MAX_LOG + 1];  // p[d], d >= 1: the 1/x twiddles of the line domain of log size d (fold_line's)
};
// device memory between the kernels of the chain
struct FriCloseState {
  PowWords pow;              // what the grind hashes: the digest behind mix_felts, or its prefixed digest
  unsigned long long best;   // the grind's answer, ~0 while there is none
  uint32_t pending;          // the grind's pending table: its one entry, 0
  uint32_t first_bad;        // lowest index >= 2^log_bound of a non-zero coefficient, 0xffffffff: none
  uint32_t digest_after_coeffs[8];
};
// the result block (page-locked): this header, n_queries words of positions, then 4 words per coefficient
struct FriCloseHeader {
  uint32_t found;            // 0: no nonce in the queued windows - nothing else is written
  uint32_t first_bad, n_positions, n_sent_end;
  uint32_t nonce_lo, nonce_hi, pad[2];
  uint32_t digest_after_coeffs[8], digest_after_nonce[8], digest_end[8];
};
// last: 4 coordinate columns of 2^log_n words, bit-reversed over the line domain (FriPlan::d_last).  Interpolates (the
// butterflies of fold_line, scale n_inv = 1/2^log_n), writes all 2^log_n coefficients to coeffs (4 words each), checks the
// degree against 2^log_bound, runs Channel::mix_felts over the first 2^log_bound coefficients on *ch and fills *st.
// scratch: 4 x 2^log_n words of device memory when log_n > FRI_CLOSE_LDS_LOG, unused otherwise.
void launch_fri_close(DevChannel* ch, const uint32_t* last, int log_n, int log_bound, const FriCloseItw& itw, uint32_t n_inv,
                      uint32_t* scratch, uint32_t* coeffs, bool pow_prefixed, uint32_t pow_bits, FriCloseState* st,
                      lmn_stream_t s);
// behind the grind: with a nonce in st->best, mix_u64 (hashed: LMN_PV_MIX_U64_HASHED), n_queries positions drawn 8 per
// draw_random_words and masked with pos_mask, sorted and made distinct; header, positions and the first n_coeff_words of
// coeffs go to `out` (FriCloseHeader's layout).  Without one: out->found = 0.
void launch_fri_queries(DevChannel* ch, const FriCloseState* st, const uint32_t* coeffs, uint32_t n_coeff_words,
                        bool hashed, uint32_t n_queries, uint32_t pos_mask, uint32_t* out, lmn_stream_t s);

// ---- trace generation for the elementwise primitives (the producer of the hot path's input)
struct TraceNode {
  uint32_t node_id, lhs_id, rhs_id;
  uint32_t lhs_mult, rhs_mult, out_mult;  // canonical M31
  // Contiguous in the reference's own row rule (prim.rs:253-296, zip_longest over the input BUFFER and the output):
  // phys_n = elements of the input buffer (0: the view rule), out_n = elements of the output
  uint64_t phys_n = 0, out_n = 0;
};
struct TraceView {  // strided view; ndim == 0: contiguous
  uint32_t ndim;
  uint32_t shape[4];
  int64_t strides[4];
  int64_t offset;
};
// An operand of a producer: member m of a many-member launch reads p + m * ms elements (ms == 0 shares it; a float source:
// elements of its dtype); the reduce producers read it contiguous and take no view
struct TraceOperand {
  const int32_t* p;
  TraceView view;
  uint64_t ms;
};
// Where a producer's rows and values go, as the launchers take it (the host side of the kernels' TraceDst).
//   ROWS: `rows` is the node's first row in an array-of-structs table (lmn_trace_*).
//   COLS: the column form (lmn_rows_append_*) - word c of the node's row r goes to cols[c * col_stride + r], so `cols` is
//         column 0 at the node's FIRST TABLE ROW (the sink's row count, any value: no alignment is asked of it).  One dword
//         per lane per column, no LDS tile (the reduce kernels keep the LDS of their scan).  A refused element is marked as
//         in the row forms, sets *bad_word (the sink's verdict word) to 1 and is added to *refused (may be null).
//   MANY: one launch fills the node's rows for n_members pies (lmn_trace_many_*), grid.y = the member: member m works on
//         base + m * stride (operands and `out` in elements, rows / aux / mult in WORDS here - the host side converts row
//         strides); out_ms == 0 stores the shared output from member 0 only.  refused (n_members counters, may be null)
//         grows by each member's refused elements.
// A LUT input outside every range is a refused element in COLS and MANY; ROWS sets *err_flag (a device word) instead.
struct TraceOut {
  enum Form { ROWS, COLS, MANY } form = ROWS;
  uint32_t* rows = nullptr;       // ROWS, MANY
  uint64_t rows_ms = 0;           // MANY
  uint32_t* cols = nullptr;       // COLS
  uint64_t col_stride = 0;
  uint32_t* bad_word = nullptr;
  uint32_t n_members = 1;
  int32_t* out = nullptr;         // the node's output tensor (may be null)
  uint64_t out_ms = 0;
  uint32_t* refused = nullptr;    // COLS, MANY
  uint32_t* err_flag = nullptr;   // ROWS of the LUT producer
};
constexpr int SRC_FIXED = -1;     // src_dtype of an int32 Fixed<12> source; LMN_F32 / LMN_F16 / LMN_BF16: raw float bits
// One launcher per family, the kernel picked by o.form.  src_dtype != SRC_FIXED: the Inputs kind reading raw float bits of
// that dtype (kernels_trace.hip float_bits_to_fixed), the conversion inside the launch that writes the rows.
// aux: LessThan's range-check multiplicities (256 words per member, aux_ms apart).
void launch_trace_elementwise(int kind, int src_dtype, const TraceOperand& lhs, const TraceOperand& rhs, uint64_t n,
                              const TraceNode& nd, uint32_t* aux, uint64_t aux_ms, const TraceOut& o, lmn_stream_t s);
// The value ranges a LUT enumerates, ascending and disjoint (`LookupLayout::ranges` after `coalesce_ranges`,
// crates/graph/src/graph.rs:665-691): LUT row of value v in range r = base[r] + (v - lo[r])
// (`LookupLayout::find_index`, crates/air/src/preprocessed.rs:60-77).
constexpr int LUT_MAX_RANGES = 16;
struct LutRanges {
  int n;
  int32_t lo[LUT_MAX_RANGES], hi[LUT_MAX_RANGES];
  uint32_t base[LUT_MAX_RANGES];
};
// LUT op rows + LUT multiplicities (lut_col1 is shared by all members, the multiplicity atomics go to the member's own
// table, mult_ms words apart)
void launch_trace_lut(const TraceOperand& input, uint64_t n, const TraceNode& nd, const uint32_t* lut_col1,
                      const LutRanges& ranges, uint32_t* mult, uint64_t mult_ms, const TraceOut& o, lmn_stream_t s);
void launch_trace_reduce(bool is_max, const TraceOperand& input, uint64_t front, uint64_t dim, uint64_t back,
                         const TraceNode& nd, const TraceOut& o, lmn_stream_t s);

// ---- the eval forms of the producers (lmn_eval_*): values only, plus the range of what was written in minmax[0 .. 1]
// (atomicMin / atomicMax: initialise with launch_eval_init) and the refused elements added to *refused; both may be null
void launch_eval_init(int32_t* minmax, lmn_stream_t s);
void launch_eval_elementwise(int kind, const int32_t* lhs, const TraceView& lv, const int32_t* rhs, const TraceView& rv,
                             uint64_t n, int32_t* out, int32_t* minmax, uint32_t* refused, lmn_stream_t s);
void launch_eval_lut(const int32_t* input, const TraceView& view, uint64_t n, const uint32_t* lut_col1, const LutRanges& ranges,
                     int32_t* out, int32_t* minmax, uint32_t* refused, lmn_stream_t s);
// true: one wave per reduction group; false: one lane per output element (back large enough for coalesced steps)
bool eval_reduce_by_wave(uint64_t dim, uint64_t back);
void launch_eval_reduce(bool is_max, const int32_t* input, uint64_t front, uint64_t dim, uint64_t back, int32_t* out,
                        int32_t* minmax, uint32_t* refused, lmn_stream_t s);
void launch_tensor_range(const int32_t* buf, uint64_t n, int32_t* minmax, lmn_stream_t s);
// Float tensors in and out (kernels_trace.hip float_bits_to_fixed / fixed_to_float_bits): the eval form of the float
// Inputs producer, and the way back
void launch_eval_inputs_float(uint32_t dtype, const void* src, uint64_t n, int32_t* out, int32_t* minmax, uint32_t* refused,
                              lmn_stream_t s);
void launch_tensor_to_float(uint32_t dtype, const int32_t* src, uint64_t n, void* dst, lmn_stream_t s);

// ---- lmn_trace_check (trace_gen.cpp): which rows break a local constraint, which logup tuples do not balance.
// One open-addressing table per relation element set: entry i = {keys[i] = val | id << 31 (TC_EMPTY: free), sums[i] = the
// sum of the signed multiplicity words (u64: below 2^26 rows x 7 relations x 2^31 it cannot overflow), firsts[i] = the
// smallest mention, table << 40 | slot << 32 | row}.  mask + 1 = a power of two of at least twice the entries the set can get.
constexpr unsigned long long TC_EMPTY = ~0ull;
constexpr int TC_MAX_SLOTS = 16;   // local slots per table in the counters (at most 9 are used)
struct TcSet {
  unsigned long long *keys, *sums, *firsts;   // null: no table of the pie uses the set
  uint64_t mask;
};
struct TcOut {
  uint32_t* slot_count;             // [table * TC_MAX_SLOTS + slot]: real rows on which the slot is non-zero
  unsigned long long* slot_first;   // ... and the smallest of them (TC_EMPTY: none)
  unsigned long long* noncanon;     // [0] words >= P in all, [1] the smallest table << 40 | row << 8 | column
  const TcSet* sets;                // device: the tuple table of each of the 5 element sets (read through the scalar cache)
};
struct TcTable {
  const uint32_t* data;        // row-major: n_rows x n_cols words; column-major: n_cols columns `stride` words apart
  uint64_t n_rows, stride;
  uint32_t table;              // index in the caller's table list
  const uint32_t *pre0, *pre1; // lookup tables: the LUT columns val / id come from (range check: null, val = the row index)
  int n_rel, slot0;            // relations; kernel slot of the first (= the component's number of local slots)
  int rel_mult[7], rel_val[7], rel_id[7], rel_set[7], rel_neg[7], rel_pre[7];   // as ComponentSpec's
};
struct TcFound {   // one unbalanced tuple, as k_trace_check_collect compacts it
  uint64_t key, first;
  uint32_t set, net;
};
void launch_trace_check(int kind, bool cols_layout, const TcTable& tb, const TcOut& out, lmn_stream_t s);
// counts the entries of `set` whose sum is non-zero mod P into *n_unbalanced and writes the first `cap` of them to `found`
void launch_trace_check_collect(const TcSet& set, uint32_t set_index, unsigned long long* n_unbalanced, TcFound* found,
                                uint32_t cap, lmn_stream_t s);

// ---- a6: logup
constexpr int LOGUP_MAX_REL = 7;
struct LogupArgs {
  int k;                       // number of relations (1..7)
  const uint32_t* val[LOGUP_MAX_REL];   // value column
  const uint32_t* id[LOGUP_MAX_REL];    // tensor-id column, nullptr for width-1 relations
  const uint32_t* mult[LOGUP_MAX_REL];  // multiplicity column
  int neg[LOGUP_MAX_REL];      // numerator is -mult
  QM31 z[LOGUP_MAX_REL], alpha[LOGUP_MAX_REL];  // element set of each relation (used when d_elems is null)
  const DevElems* d_elems;     // device-resident draws (ChanStep kind 1): relation j uses set es[j]
  int es[LOGUP_MAX_REL];
  // rows != nullptr: the component's evaluations were never stored column-major (the transpose ran inside the
  // interpolation): the relation's cells are read from the table's rows - row r at rows + r * row_words, columns
  // vcol / icol (-1: none) / mcol - and from the padding row's values beyond n_real
  const uint32_t* rows;
  uint32_t row_words, n_real;
  int vcol[LOGUP_MAX_REL], icol[LOGUP_MAX_REL], mcol[LOGUP_MAX_REL];
  uint32_t pad_val[LOGUP_MAX_REL], pad_id[LOGUP_MAX_REL], pad_mult[LOGUP_MAX_REL];
  uint32_t* inter;             // interaction eval columns (4k columns, stride n)
  QM31* last_tmp;              // S_{k-1} per row (AoS), n entries
  uint32_t* partials;          // per-block partial sums, 4 words each
  uint32_t n;                  // rows
};
int logup_num_blocks(uint32_t n);
void launch_logup_fracs(const LogupArgs& a, lmn_stream_t s);
// claimed_out[0] = sum of partials; claimed_out[1] = shift = claimed * n_inv
void launch_logup_reduce(const uint32_t* partials, int nblocks, uint32_t n_inv, QM31* claimed_out, lmn_stream_t s);
// prefix sum of (last_tmp - shift) in coset order, written to the last 4 interaction columns.
// derive_claim: claimed_shift is OUTPUT - the claimed sum (= sum of last_tmp) and shift = claimed * n_inv come out of the
// scan of the block totals itself (no launch_logup_reduce in front); otherwise it is read.
void launch_logup_scan(const QM31* last_tmp, QM31* claimed_shift, int log_size, uint32_t* out_cols /*4 x n*/,
                       QM31* blocksums, lmn_stream_t s, bool derive_claim = false, uint32_t n_inv = 0);
int logup_scan_num_blocks(int log_size);

// ---- a7: constraint quotients on the eval domain (log_size + 1)
struct CompositionArgs {
  int kind;                    // TraceTable kind (LMN_KIND_*)
  int log_size;                // trace log size
  int eval_log;                // eval domain log size
  // Rows [row0, row0 + n_rows) of the eval domain are evaluated (the whole domain, or one rank's block of a
  // sharded proof).  main / inter / pre / pre2 hold exactly those rows, columns `stride` words apart; `out` and
  // `prev_last` span the whole domain (stride 2^eval_log, indexed by the global storage index).
  uint32_t row0, n_rows;
  uint64_t stride;
  const uint32_t* main;        // main columns on the eval domain
  const uint32_t* inter;       // interaction columns on the eval domain
  const uint32_t* prev_last;   // last 4 interaction columns where the mask offset -1 reads them (other row blocks)
  uint32_t* out;               // 4 coordinate columns, stride 2^eval_log
  int accumulate;              // out += instead of out =
  QM31 z, alpha;               // NodeElements
  QM31 z2, alpha2;             // the component's LUT element set (range check / sin / exp2 / log2)
  const DevElems* d_elems;     // when set: the four values above are read from here (sets 0 and es2) instead
  int es2;
  const uint32_t* pre;         // preprocessed columns on the eval domain (lookup components)
  const uint32_t* pre2;
  const QM31* claimed_shift;   // device: [claimed, shift]
  QM31 coeff[16];              // alpha^(N-1-k) for this component's constraints, in order
  const QM31* d_coeff;         // when set: the 16 coefficients are read from device memory (ChanStep kind 2) instead
  uint32_t zinv[2];            // 1/Z for rows with (s >> log_size) == 0 / 1
};
void launch_composition(const CompositionArgs& a, lmn_stream_t s);
// out (4 x n) += in (4 x n)
void launch_secure_add(uint32_t* out, const uint32_t* in, uint64_t n_words, lmn_stream_t s);
// the first n words of ncols columns: out[c * out_stride + i] += in[c * in_stride + i]
void launch_add_cols(uint32_t* out, uint64_t out_stride, const uint32_t* in, uint64_t in_stride, uint64_t n, int ncols,
                     lmn_stream_t s);

// ---- a7: the composition polynomial from half of its evaluation domain (phase_composition.cpp).
// The quotient p has N + 1 coefficients on its 2N-point domain (N = 2^log_half): [lo_0 .. lo_{N-1}, c].  The top layer's
// basis function is +w on storage rows [0, N) and -w on [N, 2N), so g = the N-coefficient polynomial that agrees with p on
// the first half differs from p by the constant 2wc on the second half: one evaluation of p there (the probe, row N) gives c.
struct ProbeMaps {
  uint32_t m[MAX_LOG];   // y, x, pi(x), pi^2(x), ... of the probe's domain point
};
constexpr int PROBE_CHUNK_LOG = 12;
inline uint32_t probe_dot_blocks(int log_n) { return log_n > PROBE_CHUNK_LOG ? 1u << (log_n - PROBE_CHUNK_LOG) : 1u; }
// partial[c * probe_dot_blocks(log_n) + b] = the share of run b of 2^PROBE_CHUNK_LOG coefficients in (column c)(point), 4 columns;
// tail_out != nullptr: tail_out[c] = the word behind column c's 2^log_n coefficients (where the probe row's evaluation lies)
void launch_probe_dot(const uint32_t* coeffs, uint64_t stride, int log_n, const ProbeMaps& pm, uint32_t* partial,
                      uint32_t* tail_out, lmn_stream_t s);
struct CompHalfFix {
  uint32_t* coeffs;            // 4 columns, 2^(log_half + 1) words each: g in the lower half
  uint64_t coeff_stride;
  uint32_t* lde;               // 4 columns of 4 quarters behind the strided pass, or nullptr (a size that is folded into a larger one)
  uint64_t lde_stride;
  int log_half;
  const uint32_t* part_g;      // launch_probe_dot of g: 4 x n_g
  uint32_t n_g;
  const uint32_t* part_f;      // ... of the smaller sizes' polynomial folded into this one (n_f = 0: none)
  uint32_t n_f;
  const uint32_t* probe;       // 4 words: this size's constraint quotients at the probe row (launch_probe_dot's tail_out)
  const uint32_t* w_top;       // top-layer table of the 2N-point domain: w = w_top[0]
  const uint32_t* w_ext;       // layer log_half of the 4N-point domain: the quarters' twiddles w_ext[0], w_ext[1]
};
// c = (g(probe) - (p(probe) - folded(probe))) / 2w per column; coefficient 0 -= wc, coefficient N = c, the rest of the upper
// half = 0; every word at a multiple of 2^12 of quarter h of the LDE += c * ((-1)^h w_ext[h >> 1] - w)
void launch_comp_half_fix(const CompHalfFix& f, lmn_stream_t s);

// ---- a9: OODS evaluation of coefficient columns
struct EvalJob {
  const uint32_t* coeffs;
  int log_n;
  int point;                   // which point table (0 = oods, 1.. = shifted points)
  int owner = -1;              // sharded proofs: -1 = the coefficient chunks are split over the ranks; r = only rank r
                               // holds the coefficients (column-parallel interpolation) and evaluates all chunks
};
constexpr int EVAL_LB = 10;
// tables: for point p: lo table at lo_tab + p*2^EVAL_LB, hi table at hi_tab + p*hi_stride
// shard_world > 1: only the chunks this rank owns are evaluated (zeros elsewhere): the reduction is a partial sum
void launch_eval_at_point(const EvalJob* jobs, int njobs, const QM31* lo_tab, const QM31* hi_tab, uint32_t hi_stride,
                          int max_log, QM31* partial_out /* njobs x max_chunks */, int max_chunks, lmn_stream_t s,
                          uint32_t shard_rank = 0, uint32_t shard_world = 1);
int eval_num_chunks(int log_n);
void launch_eval_tables(const QM31* maps, int maps_stride, int npoints, QM31* lo_tab, QM31* hi_tab, uint32_t hi_n,
                        int hi_bits, lmn_stream_t s);
void launch_eval_reduce(const EvalJob* jobs, int njobs, const QM31* partial, int max_chunks, QM31* out,
                        lmn_stream_t s);

// ---- a9: FRI quotients
constexpr int QUOT_MAX_BATCH = 4;
constexpr int QUOT_MAX_ENTRIES = 512;
struct QuotEntry {
  const uint32_t* col;         // column of 2^log_size words
  QM31 c;                      // alpha^k * c for this (batch, column) sample
};
// Per sample batch b (the columns sampled at one point p_b): A = sum_k alpha^k a_k, B = sum_k alpha^k b_k of the batch's
// line coefficients, batch_coeff = alpha^|batch|, and the point's coordinates split into their CM31 halves
// (x = prx + u pix, y = pry + u piy).  In device memory: uploaded by the host, or - unsharded proofs - written by
// k_quot_prepare behind the point evaluations, so that no host round trip stands in front of the quotient kernels.
struct QuotDev {
  QM31 A[QUOT_MAX_BATCH], B[QUOT_MAX_BATCH], batch_coeff[QUOT_MAX_BATCH];
  CM31 prx[QUOT_MAX_BATCH], pry[QUOT_MAX_BATCH], pix[QUOT_MAX_BATCH], piy[QUOT_MAX_BATCH];
};
struct QuotientArgs {
  int log_size;                // log size of the whole LDE domain
  // rows [row0, row0 + 2^log_rows) are computed; entries[].col and out hold exactly those rows
  uint32_t row0;
  int log_rows;
  uint64_t out_stride;         // words between the 4 coordinate columns of out
  int nbatch;
  int batch_start[QUOT_MAX_BATCH + 1];  // range into entries
  const QuotEntry* entries;    // device
  const QuotDev* dev;          // device: the batches' line sums, powers and sample points (uploaded, or written by k_quot_prepare)
  const uint32_t* tw_y;        // layer-0 twiddles of the domain (y at storage 2h)
  const uint32_t* tw_x;        // layer-1 twiddles (x at storage 4h)
  uint32_t* out;               // 4 coordinate columns
};
void launch_quotients(const QuotientArgs& a, lmn_stream_t s);

// ---- a9: the transcript step and the tables in front of the FRI quotient kernels, on the device (unsharded proofs).
// Behind the point evaluations one workgroup mixes the sampled values into the device-resident channel
// (Channel::mix_felts: one Blake2s over digest || values, quad-cooperative), draws the quotient randomness alpha, and
// writes what QuotientOps::accumulate_quotients' host side (quotients.cpp make_quotient_args) would have uploaded: per LDE
// size the (column, alpha^k * c_k) entries and the batches' QuotDev.  The host enqueues the quotient kernels and the whole
// FRI commit loop without waiting for the sampled values; it replays this step (and checks the composition identity) when
// the FRI results arrive.  With one table per kind a proof has fewer samples than QUOT_PREP_MAX_SAMPLES (all 17 kinds
// make about 424), so lmn_prove reaches the host's fallback through the size count or LMN_HOST_QUOT only.
constexpr int QUOT_PREP_MAX_SIZES = 8;
constexpr int QUOT_PREP_MAX_SAMPLES = 496;   // 8 + 4 x 496 message words = 125 Blake2s blocks
struct QuotPrepEntry {
  const uint32_t* col;         // the column's LDE on the device
  uint32_t sample;             // index of its sampled value (sampled_values order)
  uint16_t size, batch;        // LDE size (index into QuotPrepPlan::size) and sample batch inside it
};
struct QuotPrepSize {
  int n_entries, n_batch;
  int batch_start[QUOT_MAX_BATCH + 1];   // into this size's entries
  int point[QUOT_MAX_BATCH];             // sample point of each batch (row of `maps`)
  uint32_t first_entry, pad_;            // the size's first entry in the plan's list
  QuotEntry* entries_out;                // device, n_entries
  QuotDev* dev_out;                      // device
};
struct QuotPrepPlan {
  int n_sizes, n_samples, n_maps, n_entries;
  QuotPrepSize size[QUOT_PREP_MAX_SIZES];
  const QuotPrepEntry* entries;          // page-locked, n_entries (sizes in order, batches in order inside a size)
  const QM31* vals;                      // device: the sampled values (k_eval_reduce)
  QM31* vals_host;                       // page-locked: n_samples values + the drawn alpha, for the host's replay
  const QM31* maps;                      // device: per sample point y, x, pi(x), ... (ChanStep kind 3), n_maps apart
  const uint32_t* copy_src;              // also copies copy_words words from page-locked to device memory (the FRI tail's table)
  uint32_t* copy_dst;
  uint32_t copy_words, pad_;
};
void launch_quot_prepare(DevChannel* ch, const QuotPrepPlan* plan /* device-visible */, lmn_stream_t s);

// ---- a9: FRI folds.  Secure columns are 4 coordinate arrays at stride = length.
// alpha is read from device memory (written by the device-resident channel).
// src holds src_len rows (a whole layer or one rank's block; itw_* then points at the block's first twiddle);
// dst_stride = words between dst's coordinate columns (0: src_len / 2, i.e. dst is exactly the folded rows).
void launch_fold_circle_into_line(uint32_t* dst, const uint32_t* src, uint32_t src_len, const uint32_t* itw_y,
                                  const QM31* alpha, int accumulate, lmn_stream_t s, uint64_t dst_stride = 0);
void launch_fold_line(uint32_t* dst, const uint32_t* src, uint32_t src_len, const uint32_t* itw_x, const QM31* alpha,
                      lmn_stream_t s, uint64_t dst_stride = 0);

}  // namespace lmn
