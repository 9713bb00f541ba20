// gfx950 kernels, part 1: the AoS -> SoA transpose of `write_trace`, device-side trace
// generation (`process_trace`, section 8f-3) and the level-2 column ops (bit reversal, decompose).  One wavefront = 64 lanes;
// global accesses are laid out so that consecutive lanes touch consecutive 4-byte words of a column.
#include "kernels_common.h"
#include "constraints.h"

namespace lmn {

// =============================================================================================
// a3  AoS -> SoA transpose with padding rows (is_last_idx = 1, everything else 0)
// =============================================================================================
// Rows [blk_row0, blk_row0 + blk_rows) of the padded table are produced (the whole table, or one rank's row block of a
// sharded proof); row r of column c lands at cols[c * out_stride + (r - blk_row0)].
// ROWS rows per workgroup: 256 (a lane has `ncols` independent loads in flight and every column gets a 1 KB run) wherever
// the row block allows, 64 for smaller blocks.
// CMP, the comparing form (trace reuse, phase_trace.cpp run_main_trace): `cols` still hold the previous proof's columns.  A
// lane reads the word of a column of `cmp_mask` that it is about to overwrite and stores only if the two differ (an unchanged
// column costs its 4 bytes per cell of reads instead of writes); a wave that saw a difference - its 64 words belong to one
// column - has one lane store `epoch` into changed[column].  Every word is compared: a column counts as unchanged only if
// it is identical.  Columns outside the mask and the canonical-word check are as in the plain form.
template <int ROWS, bool CMP = false>
LMN_KERNEL k_transpose_pad(const uint32_t* __restrict__ rows, uint64_t n_rows, int ncols, uint64_t size,
                           uint32_t* __restrict__ cols, PadRow pad, uint32_t* __restrict__ bad_flag, uint32_t magic,
                           uint64_t out_stride, uint64_t blk_row0, uint32_t bad_value, uint32_t cmp_mask,
                           uint32_t* __restrict__ changed, uint32_t epoch) {
  LMN_DYN_SMEM(uint32_t, tile);  // ROWS x stride
  // odd row stride: the column-major read below walks rows at that stride, and an even one (16 words for the 15 columns of
  // Add) maps the rows of a column onto 2 of the 32 LDS banks
  const int stride = ncols | 1;
  const uint64_t row0 = blk_row0 + (uint64_t)blockIdx.x * ROWS;
  const int total = ROWS * ncols;
  constexpr int BATCH = 8;   // loads issued before the first of them is used
  for (int k0 = threadIdx.x; k0 < total; k0 += BATCH * TPB) {
    uint32_t v[BATCH];
    int rr[BATCH], cc[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int k = k0 + j * TPB;
      // k / ncols by the precomputed reciprocal (exact for k < 2^16): a runtime integer division is ~30 VALU ops
      const int r = magic ? (int)(((uint64_t)(uint32_t)k * magic) >> 32) : k, c = k - r * ncols;  // magic 0: one column
      rr[j] = r;
      cc[j] = c;
      const uint64_t gr = row0 + r;
      v[j] = 0u;
      if (k < total) v[j] = gr < n_rows ? rows[gr * (uint64_t)ncols + c] : pad.v[c];
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      if (k0 + j * TPB >= total) break;
      if (v[j] >= P31) *bad_flag = bad_value;  // the boundary takes raw u32 words: reject non-canonical M31 values
      tile[rr[j] * stride + cc[j]] = v[j];
    }
  }
  __syncthreads();
  if constexpr (CMP) {
    static_assert(ROWS % 64 == 0, "a wave's 64 words lie in one column");
    // (every lane makes every trip: the vote below is taken by whole waves)
    for (int k0 = 0; k0 < total; k0 += TPB) {
      const int k = k0 + (int)threadIdx.x;
      const bool on = k < total;
      const int c = on ? k / ROWS : 0, r = k - c * ROWS;
      bool differs = false;
      if (on && row0 + r < size) {
        uint32_t* dst = cols + (uint64_t)c * out_stride + (row0 - blk_row0) + r;
        const uint32_t v = tile[r * stride + c];
        differs = ((cmp_mask >> c) & 1u) == 0u || *dst != v;
        if (differs) *dst = v;
        differs = differs && ((cmp_mask >> c) & 1u) != 0u;
      }
      if (lmn_ballot(differs) != 0ull && (threadIdx.x & 63u) == 0u) changed[c] = epoch;
    }
  } else {
    for (int k = threadIdx.x; k < total; k += TPB) {
      const int c = k / ROWS, r = k - c * ROWS;
      if (row0 + r < size) cols[(uint64_t)c * out_stride + (row0 - blk_row0) + r] = tile[r * stride + c];
    }
  }
}

void launch_transpose_pad_rows(const uint32_t* rows, uint64_t n_rows, int ncols, int log_size, uint32_t* cols,
                               uint64_t out_stride, uint64_t blk_row0, uint64_t blk_rows, const PadRow& pad, uint32_t* bad_flag,
                               lmn_stream_t s, uint32_t bad_value) {
  uint64_t size = 1ull << log_size;
  const bool big = blk_row0 % 256 == 0 && blk_rows % 256 == 0;
  const unsigned tr_rows = big ? 256u : 64u;
  if (blk_row0 % tr_rows || blk_row0 + blk_rows > size) throw LmnError(-100, "transpose: bad row block");
  unsigned grid = cdiv(blk_rows, tr_rows);
  size_t smem = (size_t)tr_rows * (ncols + 1) * 4;
  if (ncols > 32 || ncols < 1) throw LmnError(-100, "transpose: bad column count");
  const uint32_t magic = ncols == 1 ? 0u : (uint32_t)((0x100000000ull + (uint64_t)ncols - 1) / (uint64_t)ncols);  // ceil(2^32 / ncols)
  uint32_t* const no_changed = nullptr;   // (the plain form compares nothing)
  // rows beyond the block are cut off by treating its end as the table's size
  if (big)
    LMN_LAUNCH(k_transpose_pad<256>, dim3(grid), dim3(TPB), smem, s, rows, n_rows, ncols, blk_row0 + blk_rows, cols, pad, bad_flag,
               magic, out_stride, blk_row0, bad_value, 0u, no_changed, 0u);
  else
    LMN_LAUNCH(k_transpose_pad<64>, dim3(grid), dim3(TPB), smem, s, rows, n_rows, ncols, blk_row0 + blk_rows, cols, pad, bad_flag,
               magic, out_stride, blk_row0, bad_value, 0u, no_changed, 0u);
}
void launch_transpose_pad_compare(const uint32_t* rows, uint64_t n_rows, int ncols, int log_size, uint32_t* cols,
                                  const PadRow& pad, uint32_t* bad_flag, uint32_t bad_value, uint32_t cmp_mask,
                                  uint32_t* changed, uint32_t epoch, lmn_stream_t s) {
  const uint64_t size = 1ull << log_size;
  if (ncols > 32 || ncols < 1) throw LmnError(-100, "transpose: bad column count");
  if (size % 256 || !changed || (ncols < 32 && (cmp_mask >> ncols) != 0u)) throw LmnError(-100, "comparing transpose: bad arguments");
  const size_t smem = (size_t)256 * (ncols + 1) * 4;
  const uint32_t magic = ncols == 1 ? 0u : (uint32_t)((0x100000000ull + (uint64_t)ncols - 1) / (uint64_t)ncols);  // ceil(2^32 / ncols)
  LMN_LAUNCH((k_transpose_pad<256, true>), dim3(cdiv(size, 256)), dim3(TPB), smem, s, rows, n_rows, ncols, size, cols, pad, bad_flag,
             magic, size, (uint64_t)0, bad_value, cmp_mask, changed, epoch);
}
void launch_transpose_pad(const uint32_t* rows, uint64_t n_rows, int ncols, int log_size, uint32_t* cols,
                          const PadRow& pad, uint32_t* bad_flag, lmn_stream_t s) {
  launch_transpose_pad_rows(rows, n_rows, ncols, log_size, cols, 1ull << log_size, 0, 1ull << log_size, pad, bad_flag, s);
}

// a3 for a row sink: the rows arrive in chunks while the caller produces them.  Against k_transpose_pad: the chunk starts at
// an arbitrary table row r0, so the tiles are cut in the DESTINATION - workgroup b owns table rows [t0, t0 + CHUNK_ROWS)
// with t0 = (r0 rounded down to CHUNK_ROWS) + b * CHUNK_ROWS, of which the first and the last workgroup hold only the
// chunk's head and tail - and every full tile stores aligned 1 KB runs per column whatever r0 is.  The tile's words are
// one contiguous run of the chunk (rows are AoS), read with consecutive lanes on consecutive words, 8 loads in flight per
// lane before the first is used; the run may lie in page-locked host memory (one pass over the link, no staging copy on
// the device).  chunk == nullptr (launch-uniform): the padding row is written instead.
LMN_KERNEL k_rows_chunk(const uint32_t* __restrict__ chunk, uint64_t r0, uint64_t n, int ncols, uint32_t magic,
                        uint32_t* __restrict__ cols, uint64_t col_stride, PadRow pad, uint32_t* __restrict__ bad_word) {
  LMN_DYN_SMEM(uint32_t, tile);  // CHUNK_ROWS x stride, indexed by (table row - t0)
  const int stride = ncols | 1;  // odd: the column-major read below walks rows at that stride (k_transpose_pad)
  const uint64_t t0 = (r0 & ~(uint64_t)(CHUNK_ROWS - 1)) + (uint64_t)blockIdx.x * CHUNK_ROWS;
  const uint64_t lo = t0 > r0 ? t0 : r0, hi = t0 + CHUNK_ROWS < r0 + n ? t0 + CHUNK_ROWS : r0 + n;
  const int first = (int)(lo - t0), total = (int)(hi - lo) * ncols;   // rows [lo, hi) of the table: total <= 7 680 words
  const uint32_t* __restrict__ src = chunk ? chunk + (lo - r0) * (uint64_t)ncols : nullptr;
  constexpr int BATCH = 8;   // loads issued before the first of them is used
  for (int k0 = threadIdx.x; k0 < total; k0 += BATCH * TPB) {
    uint32_t v[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int k = k0 + j * TPB;
      v[j] = 0u;
      if (src && k < total) v[j] = src[k];
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int k = k0 + j * TPB;
      if (k >= total) break;
      // k / ncols by the precomputed reciprocal (exact for k < 2^16); magic 0: one column
      const int r = magic ? (int)(((uint64_t)(uint32_t)k * magic) >> 32) : k, c = k - r * ncols;
      const uint32_t w = src ? v[j] : pad.v[c];
      if (w >= P31) *bad_word = 1u;  // the boundary takes raw u32 words: reject non-canonical M31 values
      tile[(first + r) * stride + c] = w;
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < CHUNK_ROWS * ncols; k += TPB) {
    const int c = k / CHUNK_ROWS, r = k - c * CHUNK_ROWS;
    if (t0 + r >= lo && t0 + r < hi) cols[(uint64_t)c * col_stride + t0 + r] = tile[r * stride + c];
  }
}

void launch_rows_chunk(const uint32_t* chunk, uint64_t r0, uint64_t n, int ncols, uint32_t* cols, uint64_t stride,
                       const PadRow& pad, uint32_t* bad_word, lmn_stream_t s) {
  if (ncols > CHUNK_MAX_COLS || ncols < 1) throw LmnError(-100, "row chunk: bad column count");
  if (n == 0 || r0 + n > stride) throw LmnError(-100, "row chunk: rows outside the columns");
  const uint64_t t0 = r0 & ~(uint64_t)(CHUNK_ROWS - 1);
  const unsigned grid = cdiv(r0 + n - t0, CHUNK_ROWS);
  const size_t smem = (size_t)CHUNK_ROWS * (ncols | 1) * 4;
  const uint32_t magic = ncols == 1 ? 0u : (uint32_t)((0x100000000ull + (uint64_t)ncols - 1) / (uint64_t)ncols);  // ceil(2^32 / ncols)
  LMN_LAUNCH(k_rows_chunk, dim3(grid), dim3(TPB), smem, s, chunk, r0, n, ncols, magic, cols, stride, pad, bad_word);
}

// =============================================================================================
// gen_trace for Add / Mul / Recip nodes (crates/graph/src/op/prim.rs:967-1013, :1090-1139, :388-431):
// one lane per tensor element computes the fixed-point op and its row; the block stages its rows in LDS
// and writes them out as one contiguous, coalesced run of words.
// The producers' contract (include/luminair_hip.h, lmn_trace_elementwise): every value read or written lies in
// [-FIXED_MAX, FIXED_MAX], every row word is the exact value mod P, and an element outside the contract (range or an
// op's precondition) gets the non-canonical word P in its row's output-value column and 0 in the output tensor, so that
// lmn_prove refuses the table.  No lane does value-dependent work for such an element (no division by zero, no isqrt
// of a negative number).
// =============================================================================================
constexpr int64_t FIXED_MAX = (1ll << 30) - 1;
LMN_HD bool fixed_ok(int64_t v) { return v >= -FIXED_MAX && v <= FIXED_MAX; }
// v mod P for any int64 (Python's v % P): |v| folded twice on 2^31 = 1 (mod P), then negated
LMN_HD uint32_t fixed_to_m31(int64_t v) {
  const uint64_t m = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
  uint64_t x = (m & P31) + (m >> 31);  // < 2^34
  x = (x & P31) + (x >> 31);           // < 2^31 + 8
  uint32_t w = (uint32_t)x;
  if (w >= P31) w -= P31;
  return v < 0 && w ? P31 - w : w;
}

// ---- Float tensors in and out (`CopyToStwo` / `CopyFromStwo`, crates/graph/src/op/prim.rs:52-101: `StwoData::from_f32` is
// `Fixed::from_f64(d as f64)` per element, crates/graph/src/data.rs:17-31, and the way back is `d.to_f64() as f32`).  Both
// rules are integer decodes of the IEEE bit pattern - EB exponent bits, MB mantissa bits: f32 <8, 23>, f16 <5, 10>,
// bf16 <8, 7> - so the library still does no floating point and the result cannot depend on a wave's denormal or rounding
// mode.
// Float -> Fixed<12>: the exact value x 4096 rounded to the nearest integer, ties away from zero (`f64::round`; numerair is
// un-vendored, its rounding unpinned).  +-0 and every denormal give 0 (the largest f16 denormal x 4096 is below 1/4).  A NaN,
// an infinity and a rounded value outside fixed_ok are refused: FLOAT_REFUSED, which no range check accepts, so the element
// takes the producers' ordinary refusal (P in the row, 0 in the tensor, counted).  Straight-line code: a refused element does
// the same work as any other.
constexpr int64_t FLOAT_REFUSED = INT64_MIN;
template <int EB, int MB>
LMN_HD int64_t float_bits_to_fixed(uint32_t bits) {
  constexpr int BIAS = (1 << (EB - 1)) - 1;
  const uint32_t e = (bits >> MB) & ((1u << EB) - 1u);
  const uint64_t sig = (uint64_t)((bits & ((1u << MB) - 1u)) | (1u << MB));   // 1.m as an integer: value = sig * 2^(e - BIAS - MB)
  const int sh = (int)e - BIAS - MB + 12;                                     // value * 4096 = sig * 2^sh
  uint64_t mag;
  if (sh >= 0) mag = sig << (sh < 31 ? sh : 31);                              // >= 2^31 from sh = 31 - MB on: refused below
  else if (-sh > MB + 2) mag = 0;                                             // below 1/4
  else mag = (sig + (1ull << (-sh - 1))) >> -sh;                              // floor(x + 1/2): ties away from zero
  const bool refused = e == (1u << EB) - 1u || mag > (uint64_t)FIXED_MAX;     // Inf / NaN, or outside the value range
  if (e == 0u) mag = 0;                                                       // zero and the denormals
  return refused ? FLOAT_REFUSED : (bits >> (EB + MB)) & 1u ? -(int64_t)mag : (int64_t)mag;
}
// Fixed<12> -> float: the exact value v / 4096 rounded ONCE to the format, round-to-nearest-even (for f32 what
// `d.to_f64() as f32` gives: v / 4096 is exact in f64).  Every |v| >= 1 is 2^-12 or more, a normal number in all three
// formats; a magnitude above the format's largest finite value becomes +-Inf (f16 only).  Defined for every 32-bit word
// - a word outside fixed_ok cannot occur in a tensor a producer wrote; its result is unspecified.
template <int EB, int MB>
LMN_HD uint32_t fixed_to_float_bits(int32_t v) {
  constexpr int BIAS = (1 << (EB - 1)) - 1;
  const uint32_t sign = v < 0 ? 1u << (EB + MB) : 0u;
  const uint32_t mag = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
  if (mag == 0u) return 0u;
  int p = 31;   // the leading bit: mag = 1.xxx * 2^p, the value 1.xxx * 2^(p - 12)
  while (!(mag >> p)) --p;
  uint32_t q;   // 1.m as an integer of MB + 1 bits (MB + 2 when the rounding carries)
  if (p <= MB) {
    q = mag << (MB - p);
  } else {
    const int r = p - MB;
    const uint32_t rem = mag & ((1u << r) - 1u), half = 1u << (r - 1);
    q = mag >> r;
    q += rem > half || (rem == half && (q & 1u)) ? 1u : 0u;
  }
  uint32_t bits = ((uint32_t)(p - 12 + BIAS - 1) << MB) + q;   // the leading 1 of q - or its carry - counts the exponent up
  if ((bits >> MB) >= (1u << EB) - 1u) bits = ((1u << EB) - 1u) << MB;
  return sign | bits;
}
// Where a producer's operand comes from: an int32 Fixed<12> tensor, or raw float bits of dtype LMN_F32 / LMN_F16 / LMN_BF16
// (SRC = the dtype) converted as they are read.  The float forms hand their source's address through the operand's
// `const int32_t*` parameter; src_at and src_value give it its element size back.  (SRC_FIXED: kernels.h)
template <int SRC>
LMN_HD const int32_t* src_at(const int32_t* base, uint64_t elems) {
  constexpr uint64_t BYTES = SRC == SRC_FIXED || SRC == 0 ? 4 : 2;
  return (const int32_t*)((const char*)base + elems * BYTES);
}
template <int SRC>
LMN_HD int64_t src_value(const int32_t* __restrict__ base, uint64_t i) {
  static_assert(SRC >= SRC_FIXED && SRC <= 2, "LMN_F32, LMN_F16 or LMN_BF16");
  if (SRC == 0) return float_bits_to_fixed<8, 23>(((const uint32_t*)base)[i]);
  if (SRC == 1) return float_bits_to_fixed<5, 10>(((const uint16_t*)base)[i]);
  if (SRC == 2) return float_bits_to_fixed<8, 7>(((const uint16_t*)base)[i]);
  return base[i];
}

LMN_D uint64_t view_offset(const TraceView& v, uint64_t r) {
  if (v.ndim == 0) return r;
  int64_t off = v.offset;
  for (int k = (int)v.ndim - 1; k >= 0; --k) {
    const uint64_t d = v.shape[k];
    off += (int64_t)(r % d) * v.strides[k];
    r /= d;
  }
  return (uint64_t)off;
}

LMN_HD constexpr int trace_ncols(int kind) {
  return kind == 0 ? 15 : kind == 1 ? 16 : kind == 2 ? 13 : kind == 7 ? 13 : kind == 8 ? 16 : kind == 13 ? 22
                                                                                       : kind == 16 ? 11 : 7;
}
// the output-value column of a kind's row: where a refused element carries the word P
LMN_HD constexpr int trace_mark_col(int kind) { return kind == 0 || kind == 1 || kind == 8 || kind == 13 ? 11 : kind == 15 ? 5 : 8; }
// floor(sqrt(v)) for 0 <= v < 2^44, exact (double sqrt + one correction step each way)
LMN_D int64_t isqrt_u64(int64_t v) {
  int64_t r = (int64_t)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

// The value rule of one element, stated once for the trace form (k_trace_elementwise: rows + output) and the eval form
// (k_eval_elementwise: output only).  out = what the output tensor receives (0 for a refused element), aux = the kind's
// second derived word as an exact integer (Mul: low 12 bits of the product, Recip / Sqrt: rem, Rem: quo, LessThan: diff;
// 0 for a refused element).  No value-dependent work for a refused element: it divides by 1, takes the root of 0.
struct ElemValue {
  bool ok;
  int64_t out, aux;
};
template <int KIND>
LMN_D ElemValue elem_value(int64_t a, int64_t b) {
  if (KIND == 16 || KIND == 15) {   // Contiguous (prim.rs:229-301), CopyToStwo / Inputs (prim.rs:52-88): out = input
    const bool ok = fixed_ok(a);
    return {ok, ok ? a : 0, 0};
  } else if (KIND == 7) {
    // Sqrt (prim.rs:573-660): out = floor(sqrt(input * scale)), rem = input * scale - out^2 (natural identity; numerair's
    // form is unpinned).  input >= 0: a refused element takes the square root of 0
    const bool ok = a >= 0 && a <= FIXED_MAX;
    const int64_t x = ok ? a * 4096ll : 0, o = isqrt_u64(x);
    return {ok, o, x - o * o};
  } else if (KIND == 8) {
    // Rem (prim.rs:1323-1421), lhs >= 0, rhs > 0: lhs = rhs * quotient + rem; the out relation carries rem.
    // A refused element divides 0 by 1.
    const bool ok = a >= 0 && a <= FIXED_MAX && b > 0 && b <= FIXED_MAX;
    const uint32_t num = ok ? (uint32_t)a : 0u, den = ok ? (uint32_t)b : 1u;
    const uint32_t quo = num / den, rem = num - quo * den;
    return {ok, (int64_t)rem, (int64_t)quo};
  } else if (KIND == 13) {
    // LessThan (prim.rs:1203-1295): out = 1.0 iff lhs < rhs; diff = rhs - lhs (+ P with borrow)
    // (a refused element has zero diff)
    const bool ok = fixed_ok(a) && fixed_ok(b), lt = ok && a < b;
    const int64_t diff = ok ? b - a + (lt ? 0 : (int64_t)P31) : 0;  // 1 .. 2^31 - 2, or P for equal operands
    return {ok, lt ? 4096 : 0, diff};
  } else if (KIND == 2) {
    // Recip: input > 0 (4096^2 / input and its remainder fit 32 bits): a refused element divides by 1
    const bool ok = a > 0 && a <= FIXED_MAX;
    const uint32_t sc2 = 4096u * 4096u, den = ok ? (uint32_t)a : 1u;
    const uint32_t o = sc2 / den, rem = sc2 - den * o;
    return {ok, ok ? (int64_t)o : 0, ok ? (int64_t)rem : 0};
  } else {
    const int64_t prod = a * b, o = KIND == 0 ? a + b : prod >> 12;  // Mul: floor
    const bool ok = fixed_ok(a) && fixed_ok(b) && fixed_ok(o);
    return {ok, ok ? o : 0, KIND == 1 && ok ? (prod & 4095) : 0};
  }
}

LMN_D uint32_t wave_count(bool pred) { return (uint32_t)__builtin_popcountll(lmn_ballot(pred)); }
// the refused elements of a many-member launch: one atomicAdd per wave that holds any, to the member's counter.  Reached by
// all TPB lanes.
LMN_D void trace_count_refused(bool bad, uint32_t* __restrict__ refused) {
  const uint32_t c = wave_count(bad);
  if (refused && c && (threadIdx.x & 63u) == 0u) atomicAdd(refused, c);
}

// Where a producer's rows go, and how a block's rows leave.  The ROW form (COLS false): `p` is the node's first row of an
// array-of-structs table; a lane builds its row in the block's LDS tile and the block writes the tile out as one contiguous,
// coalesced run of words.  The COLUMN form (a row sink's columns, lmn_rows_append_*): `p` is column 0 at the node's first
// table row - any row, aligned to nothing - and word c of the node's row r goes to p[c * col_stride + r]: the row is built in
// registers and stored column by column, one dword per lane per column (a 256-byte run per wave store), with no LDS tile.
// A lane whose row carries the mark sets *bad, the sink's verdict word (the word k_rows_chunk sets for a pushed word >= P).
struct TraceDst {
  uint32_t* p;
  uint64_t col_stride;   // column form only
  uint32_t* bad;         // column form only
};
template <int NC, bool COLS, int ST = (NC | 1)>   // ST: the tile's row stride, odd: conflict-free column writes
struct RowOut {   // the row form
  uint32_t* tile;
  uint32_t* t;    // this lane's row
  LMN_D RowOut() {
    LMN_SHARED uint32_t s_tile[TPB * ST];
    tile = s_tile;
    t = s_tile + threadIdx.x * ST;
  }
  // reached by all TPB lanes: the block holds rows [row0, min(row0 + TPB, n)) of the node's n rows
  LMN_D void store(const TraceDst& d, uint64_t row0, uint64_t n, bool, bool) {
    __syncthreads();
    const uint64_t rows_here = n - row0 < (uint64_t)TPB ? n - row0 : (uint64_t)TPB;
    const uint32_t words = (uint32_t)rows_here * NC;
    uint32_t* dst = d.p + row0 * NC;
    for (uint32_t w = threadIdx.x; w < words; w += TPB) dst[w] = tile[(w / NC) * ST + (w % NC)];
  }
};
template <int NC, int ST>
struct RowOut<NC, true, ST> {   // the column form
  uint32_t t[NC];
  LMN_D void store(const TraceDst& d, uint64_t row0, uint64_t n, bool on, bool bad) {
    if (!on) return;
    uint32_t* col = d.p + row0 + threadIdx.x;
#pragma unroll
    for (int c = 0; c < NC; ++c) col[(uint64_t)c * d.col_stride] = t[c];
    if (bad) *d.bad = 1u;
  }
};

// The row rule of the elementwise kinds, stated once for k_trace_elementwise (one tensor per launch) and
// k_trace_many_elementwise (blockIdx.y = the member): the pointers are the launch's own or the member's bases, blockIdx.x is
// the tile of TPB rows in both.  MANY or COLS: the refused elements are counted in *refused (may be null).  COLS: the
// column form of the single launch (k_sink_elementwise), see TraceDst.  SRC: what `lhs` holds (src_value; a float source is
// Inputs' alone - k_trace_inputs_float and its siblings: the conversion happens where the row is built, the converted
// tensor is never read back).
template <int KIND, bool MANY, bool COLS = false, int SRC = SRC_FIXED>
LMN_D void trace_elementwise_rows(const int32_t* __restrict__ lhs, const TraceView& lv, const int32_t* __restrict__ rhs,
                                  const TraceView& rv, uint64_t n, const TraceNode& nd, const TraceDst& dst,
                                  int32_t* __restrict__ out, uint32_t* __restrict__ aux, uint32_t* __restrict__ refused) {
  static_assert(!(MANY && COLS), "the many-member forms keep rows only");
  static_assert(SRC == SRC_FIXED || KIND == 15, "float sources feed graph inputs only");
  constexpr int NC = trace_ncols(KIND);
  RowOut<NC, COLS> ro;
  const uint64_t row0 = (uint64_t)blockIdx.x * TPB;
  const uint64_t r = row0 + threadIdx.x;
  bool bad = false;   // this lane's element is refused (its row carries the mark)
  if (r < n) {
    uint32_t* t = ro.t;
    const bool ref_contig = KIND == 16 && nd.phys_n != 0;
    const int64_t a = src_value<SRC>(lhs, view_offset(lv, ref_contig ? r % nd.out_n : r));
    const uint32_t idx = (uint32_t)r, last = r + 1 == (ref_contig ? nd.phys_n : n) ? 1u : 0u;
    if (ref_contig) {
      // LuminairContiguous::process_trace as the reference writes it (prim.rs:253-296): row idx pairs the idx-th
      // element of the input BUFFER (zero past its end) with the idx-th element of the OUTPUT (the view; past the
      // output's end the index expression wraps), is_last_idx marks the buffer's last element.  Every buffer
      // element is consumed exactly once, so slices and permutations of the input balance.
      const int64_t in = r < nd.phys_n ? (int64_t)lhs[r] : 0;
      const bool ok = fixed_ok(in) && fixed_ok(a);
      t[0] = nd.node_id; t[1] = nd.lhs_id; t[2] = idx; t[3] = last;
      t[4] = nd.node_id; t[5] = nd.lhs_id; t[6] = idx + 1u;
      t[7] = fixed_to_m31(in);
      t[8] = ok ? fixed_to_m31(a) : P31; t[9] = nd.lhs_mult; t[10] = nd.out_mult;
      if (out && r < nd.out_n) out[r] = ok ? (int32_t)a : 0;
    } else if (KIND == 16 || KIND == 7) {
      // Contiguous: input, out.  Sqrt: input, out, rem, scale
      const ElemValue e = elem_value<KIND>(a, 0);
      t[0] = nd.node_id; t[1] = nd.lhs_id; t[2] = idx; t[3] = last;
      t[4] = nd.node_id; t[5] = nd.lhs_id; t[6] = idx + 1u;
      t[7] = fixed_to_m31(a);
      t[8] = e.ok ? fixed_to_m31(e.out) : P31;
      if (KIND == 16) {
        t[9] = nd.lhs_mult; t[10] = nd.out_mult;
      } else {
        t[9] = fixed_to_m31(e.aux); t[10] = 4096u;
        t[11] = nd.lhs_mult; t[12] = nd.out_mult;
      }
      if (out) out[r] = (int32_t)e.out;
    } else if (KIND == 8 || KIND == 13) {
      const int64_t b = rhs[view_offset(rv, r)];
      t[0] = nd.node_id; t[1] = nd.lhs_id; t[2] = nd.rhs_id; t[3] = idx; t[4] = last;
      t[5] = nd.node_id; t[6] = nd.lhs_id; t[7] = nd.rhs_id; t[8] = idx + 1u;
      t[9] = fixed_to_m31(a); t[10] = fixed_to_m31(b);
      const ElemValue e = elem_value<KIND>(a, b);
      t[11] = e.ok ? (uint32_t)e.out : P31;   // Rem: rem; LessThan: 1.0 or 0
      if (KIND == 8) {
        t[12] = (uint32_t)e.aux;              // quo
        t[13] = nd.lhs_mult; t[14] = nd.rhs_mult; t[15] = nd.out_mult;
      } else {
        // diff in four range-checked 8-bit limbs; aux = the RangeCheckLookup multiplicity column (256 entries)
        // (a refused element has zero diff, borrow and limbs and adds nothing to the multiplicities)
        const bool ok = e.ok;
        const int64_t diff = e.aux;
        t[12] = fixed_to_m31(diff);
        t[13] = ok && e.out == 0 ? 1u : 0u;   // borrow: not less
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t limb = (uint32_t)(diff >> (8 * k)) & 0xFFu;
          t[14 + k] = limb;
          if (ok) atomicAdd(&aux[limb], 1u);
        }
        t[18] = nd.lhs_mult; t[19] = nd.rhs_mult; t[20] = nd.out_mult; t[21] = 1u;
      }
      if (out) out[r] = (int32_t)e.out;
    } else if (KIND == 15) {
      // CopyToStwo / Inputs (prim.rs:52-88): node, idx, is_last, next_node, next_idx, val, multiplicity
      const ElemValue e = elem_value<KIND>(a, 0);
      t[0] = nd.node_id; t[1] = idx; t[2] = last; t[3] = nd.node_id; t[4] = idx + 1u;
      t[5] = e.ok ? fixed_to_m31(a) : P31; t[6] = nd.out_mult;
      if (out) out[r] = (int32_t)e.out;
    } else if (KIND == 2) {
      // node, input, idx, is_last, next_node, next_input, next_idx, input, out, rem, scale, in_mult, out_mult
      const ElemValue e = elem_value<KIND>(a, 0);
      t[0] = nd.node_id; t[1] = nd.lhs_id; t[2] = idx; t[3] = last;
      t[4] = nd.node_id; t[5] = nd.lhs_id; t[6] = idx + 1u;
      t[7] = fixed_to_m31(a); t[8] = e.ok ? (uint32_t)e.out : P31; t[9] = (uint32_t)e.aux; t[10] = 4096u;
      t[11] = nd.lhs_mult; t[12] = nd.out_mult;
      if (out) out[r] = (int32_t)e.out;
    } else {
      const int64_t b = rhs[view_offset(rv, r)];
      t[0] = nd.node_id; t[1] = nd.lhs_id; t[2] = nd.rhs_id; t[3] = idx; t[4] = last;
      t[5] = nd.node_id; t[6] = nd.lhs_id; t[7] = nd.rhs_id; t[8] = idx + 1u;
      t[9] = fixed_to_m31(a); t[10] = fixed_to_m31(b);
      const ElemValue e = elem_value<KIND>(a, b);
      t[11] = e.ok ? fixed_to_m31(e.out) : P31;
      if (KIND == 0) {
        t[12] = nd.lhs_mult; t[13] = nd.rhs_mult; t[14] = nd.out_mult;
      } else {
        t[12] = (uint32_t)e.aux;
        t[13] = nd.lhs_mult; t[14] = nd.rhs_mult; t[15] = nd.out_mult;
      }
      if (out) out[r] = (int32_t)e.out;
    }
    if constexpr (MANY || COLS) bad = t[trace_mark_col(KIND)] == P31;
  }
  if constexpr (MANY || COLS) trace_count_refused(bad, refused);
  ro.store(dst, row0, n, r < n, bad);
}

template <int KIND>
LMN_KERNEL k_trace_elementwise(const int32_t* __restrict__ lhs, TraceView lv, const int32_t* __restrict__ rhs,
                               TraceView rv, uint64_t n, TraceNode nd, uint32_t* __restrict__ rows,
                               int32_t* __restrict__ out, uint32_t* __restrict__ aux) {
  trace_elementwise_rows<KIND, false>(lhs, lv, rhs, rv, n, nd, TraceDst{rows, 0, nullptr}, out, aux, nullptr);
}
// the column form: cols = column 0 at the node's first table row, columns col_stride words apart (TraceDst)
template <int KIND>
LMN_KERNEL k_sink_elementwise(const int32_t* __restrict__ lhs, TraceView lv, const int32_t* __restrict__ rhs,
                                    TraceView rv, uint64_t n, TraceNode nd, uint32_t* __restrict__ cols, uint64_t col_stride,
                                    int32_t* __restrict__ out, uint32_t* __restrict__ aux, uint32_t* __restrict__ bad_word,
                                    uint32_t* __restrict__ refused) {
  trace_elementwise_rows<KIND, false, true>(lhs, lv, rhs, rv, n, nd, TraceDst{cols, col_stride, bad_word}, out, aux, refused);
}

// Member m of a many-member launch works on base + m * member stride (blockIdx.y is uniform over the workgroup: the bases are
// formed once, as 64-bit scalars, in front of the per-lane work).  A stride of 0 shares an operand; a shared output tensor
// (out_ms == 0, all operands shared) is stored by member 0 alone.
LMN_D int32_t* many_out_base(int32_t* out, uint64_t out_ms, uint64_t m) {
  return !out ? nullptr : out_ms ? out + m * out_ms : m == 0 ? out : nullptr;
}
template <int KIND>
LMN_KERNEL k_trace_many_elementwise(const int32_t* __restrict__ lhs, TraceView lv, uint64_t lhs_ms,
                                    const int32_t* __restrict__ rhs, TraceView rv, uint64_t rhs_ms, uint64_t n, TraceNode nd,
                                    uint32_t* __restrict__ rows, uint64_t rows_ms, int32_t* __restrict__ out, uint64_t out_ms,
                                    uint32_t* __restrict__ aux, uint64_t aux_ms, uint32_t* __restrict__ refused) {
  const uint64_t m = blockIdx.y;
  trace_elementwise_rows<KIND, true>(lhs + m * lhs_ms, lv, rhs ? rhs + m * rhs_ms : nullptr, rv, n, nd,
                                     TraceDst{rows + m * rows_ms, 0, nullptr}, many_out_base(out, out_ms, m), aux ? aux + m * aux_ms : nullptr,
                                     refused ? refused + m : nullptr);
}

// SumReduce rows (prim.rs:1486-1510, 1536-1561): row r = (i*back + j)*dim + k holds input[i, k, j], the
// running sum before and after it, and the output on the group's last step.  One lane per row; the prefix
// inside a group comes from a block-wide segmented scan (plus one cooperative carry-in for the group that straddles
// the block's first row), rows leave through LDS.
// MAX: MaxReduce rows (prim.rs:1591-1734): the running maximum starts at the group's first element, is_max marks
// the rows whose input becomes the new maximum (strict comparison).
// (the row rule once, for k_trace_reduce and k_trace_many_reduce: `input` is the launch's or the member's own tensor, so the
// cooperative carry-in reads the member's own input.  COLS: the column form - the scan keeps its LDS, the rows are not
// staged)
template <bool MAX, bool MANY, bool COLS = false>
LMN_D void trace_reduce_rows(const int32_t* __restrict__ input, uint64_t dim, uint64_t back, uint64_t n_rows, uint64_t n_out,
                             const TraceNode& nd, const TraceDst& dst, int32_t* __restrict__ out,
                             uint32_t* __restrict__ refused) {
  static_assert(!(MANY && COLS), "the many-member forms keep rows only");
  constexpr int NC = MAX ? 15 : 14, ST = MAX ? 17 : 15;
  RowOut<NC, COLS, ST> ro;
  LMN_SHARED int64_t scan[TPB];   // inclusive segmented scan of the block's inputs (segment = reduction group)
  LMN_SHARED uint32_t head[TPB];  // distance (in lanes) back to the segment's first lane inside this block
  const uint64_t row0 = (uint64_t)blockIdx.x * TPB;
  const uint64_t r = row0 + threadIdx.x;
  const bool on = r < n_rows;
  const uint64_t g = on ? r / dim : 0, k = on ? r % dim : 0;  // output index (i*back + j), reduction step
  const uint64_t i = g / back, j = g % back;
  const int32_t* p = input + i * dim * back + j;
  const int64_t v = on ? (int64_t)p[k * back] : 0;
  auto op = [](int64_t a, int64_t b) { return MAX ? (a > b ? a : b) : a + b; };
  // carry-in of the group that straddles the block's first row: steps [0, k0) of that group, reduced cooperatively
  // (the block's first lane has k = k0); every other group starts inside the block
  const uint64_t k0 = row0 % dim;
  {
    const uint64_t g0 = row0 / dim, i0 = g0 / back, j0 = g0 % back;
    const int32_t* p0 = input + i0 * dim * back + j0;
    int64_t part = MAX ? INT64_MIN : 0;
    for (uint64_t kk = threadIdx.x; kk < k0; kk += TPB) part = op(part, (int64_t)p0[kk * back]);
    scan[threadIdx.x] = part;
    __syncthreads();
    for (int st = TPB / 2; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) scan[threadIdx.x] = op(scan[threadIdx.x], scan[threadIdx.x + st]);
      __syncthreads();
    }
  }
  const int64_t carry = scan[0];
  __syncthreads();
  // Hillis-Steele segmented inclusive scan: lane t combines with lane t - d only while that lane is still inside
  // the same group (head[t] = lanes back to the group's first lane in this block)
  const uint32_t dist = (uint32_t)(k < (uint64_t)threadIdx.x ? k : threadIdx.x);
  scan[threadIdx.x] = v;
  head[threadIdx.x] = dist;
  __syncthreads();
  for (uint32_t d = 1; d < TPB; d <<= 1) {
    int64_t add = 0;
    const bool take = d <= dist;
    if (take) add = scan[threadIdx.x - d];
    __syncthreads();
    if (take) scan[threadIdx.x] = op(scan[threadIdx.x], add);
    __syncthreads();
  }
  bool bad = false;   // this lane's row carries the mark
  if (on) {
    // exclusive value: everything of the group before step k (inside the block, plus the carry for the straddling group)
    const bool first_seg = k == k0 + threadIdx.x;  // this lane's group began before the block
    int64_t acc;
    if (k == 0) {
      acc = MAX ? v : 0;
    } else {
      const bool has_prev = dist > 0;
      const int64_t inside = has_prev ? scan[threadIdx.x - 1] : (MAX ? INT64_MIN : 0);
      acc = first_seg ? (has_prev ? op(carry, inside) : carry) : inside;
    }
    const int64_t next = op(acc, v);
    const bool last_step = k + 1 == dim;
    // running values may leave the value range (exact words mod P); an input outside it, or a group result outside it
    // on the last step, marks the row's output-value column
    const bool ok = fixed_ok(v) && (!last_step || fixed_ok(next));
    uint32_t* t = ro.t;
    t[0] = nd.node_id; t[1] = nd.lhs_id; t[2] = (uint32_t)g; t[3] = g + 1 == n_out ? 1u : 0u;
    t[4] = nd.node_id; t[5] = nd.lhs_id; t[6] = (uint32_t)g + 1u;
    t[7] = fixed_to_m31(v); t[8] = !ok ? P31 : last_step ? fixed_to_m31(next) : 0u;
    t[9] = fixed_to_m31(acc); t[10] = fixed_to_m31(next); t[11] = last_step ? 1u : 0u;
    if (MAX) {
      t[12] = v > acc ? 1u : 0u; t[13] = nd.lhs_mult; t[14] = last_step ? nd.out_mult : 0u;
    } else {
      t[12] = nd.lhs_mult; t[13] = last_step ? nd.out_mult : 0u;
    }
    if (last_step && out) out[g] = ok ? (int32_t)next : 0;
    bad = !ok;
  }
  if constexpr (MANY || COLS) trace_count_refused(bad, refused);
  ro.store(dst, row0, n_rows, on, bad);
}

template <bool MAX>
LMN_KERNEL k_trace_reduce(const int32_t* __restrict__ input, uint64_t dim, uint64_t back, uint64_t n_rows,
                          uint64_t n_out, TraceNode nd, uint32_t* __restrict__ rows, int32_t* __restrict__ out) {
  trace_reduce_rows<MAX, false>(input, dim, back, n_rows, n_out, nd, TraceDst{rows, 0, nullptr}, out, nullptr);
}
template <bool MAX>
LMN_KERNEL k_sink_reduce(const int32_t* __restrict__ input, uint64_t dim, uint64_t back, uint64_t n_rows, uint64_t n_out,
                               TraceNode nd, uint32_t* __restrict__ cols, uint64_t col_stride, int32_t* __restrict__ out,
                               uint32_t* __restrict__ bad_word, uint32_t* __restrict__ refused) {
  trace_reduce_rows<MAX, false, true>(input, dim, back, n_rows, n_out, nd, TraceDst{cols, col_stride, bad_word}, out, refused);
}
template <bool MAX>
LMN_KERNEL k_trace_many_reduce(const int32_t* __restrict__ input, uint64_t in_ms, uint64_t dim, uint64_t back, uint64_t n_rows,
                               uint64_t n_out, TraceNode nd, uint32_t* __restrict__ rows, uint64_t rows_ms,
                               int32_t* __restrict__ out, uint64_t out_ms, uint32_t* __restrict__ refused) {
  const uint64_t m = blockIdx.y;
  trace_reduce_rows<MAX, true>(input + m * in_ms, dim, back, n_rows, n_out, nd, TraceDst{rows + m * rows_ms, 0, nullptr},
                               many_out_base(out, out_ms, m), refused ? refused + m : nullptr);
}

// One launcher per family: the destination's form (TraceOut, kernels.h) picks the kernel in front of the same row rule
void launch_trace_reduce(bool is_max, const TraceOperand& input, uint64_t front, uint64_t dim, uint64_t back,
                         const TraceNode& nd, const TraceOut& o, lmn_stream_t s) {
  const uint64_t n_out = front * back, n_rows = n_out * dim;
  const dim3 g(cdiv(n_rows, TPB), o.form == TraceOut::MANY ? o.n_members : 1), b(TPB);
  switch (o.form) {
    case TraceOut::ROWS:
      if (is_max) LMN_LAUNCH(k_trace_reduce<true>, g, b, 0, s, input.p, dim, back, n_rows, n_out, nd, o.rows, o.out);
      else LMN_LAUNCH(k_trace_reduce<false>, g, b, 0, s, input.p, dim, back, n_rows, n_out, nd, o.rows, o.out);
      break;
    case TraceOut::COLS:
      if (is_max)
        LMN_LAUNCH(k_sink_reduce<true>, g, b, 0, s, input.p, dim, back, n_rows, n_out, nd, o.cols, o.col_stride, o.out, o.bad_word,
                   o.refused);
      else
        LMN_LAUNCH(k_sink_reduce<false>, g, b, 0, s, input.p, dim, back, n_rows, n_out, nd, o.cols, o.col_stride, o.out, o.bad_word,
                   o.refused);
      break;
    case TraceOut::MANY:
      if (is_max)
        LMN_LAUNCH(k_trace_many_reduce<true>, g, b, 0, s, input.p, input.ms, dim, back, n_rows, n_out, nd, o.rows, o.rows_ms, o.out,
                   o.out_ms, o.refused);
      else
        LMN_LAUNCH(k_trace_many_reduce<false>, g, b, 0, s, input.p, input.ms, dim, back, n_rows, n_out, nd, o.rows, o.rows_ms, o.out,
                   o.out_ms, o.refused);
      break;
  }
}

// The float forms of the Inputs producers (lmn_trace_inputs_float and its many and sink siblings): k_trace_elementwise<15>,
// k_sink_elementwise<15> and k_trace_many_elementwise<15> with a float source - the same row rule, RowOut and TraceDst, the
// conversion where the row is built.  A member's source is src_ms elements of the dtype behind the previous member's.
template <int SRC>
LMN_KERNEL k_trace_inputs_float(const int32_t* __restrict__ src, uint64_t n, TraceNode nd, uint32_t* __restrict__ rows,
                                int32_t* __restrict__ out) {
  trace_elementwise_rows<15, false, false, SRC>(src, TraceView{}, nullptr, TraceView{}, n, nd, TraceDst{rows, 0, nullptr}, out,
                                                nullptr, nullptr);
}
template <int SRC>
LMN_KERNEL k_sink_inputs_float(const int32_t* __restrict__ src, uint64_t n, TraceNode nd, uint32_t* __restrict__ cols,
                               uint64_t col_stride, int32_t* __restrict__ out, uint32_t* __restrict__ bad_word,
                               uint32_t* __restrict__ refused) {
  trace_elementwise_rows<15, false, true, SRC>(src, TraceView{}, nullptr, TraceView{}, n, nd, TraceDst{cols, col_stride, bad_word},
                                               out, nullptr, refused);
}
template <int SRC>
LMN_KERNEL k_trace_many_inputs_float(const int32_t* __restrict__ src, uint64_t src_ms, uint64_t n, TraceNode nd,
                                     uint32_t* __restrict__ rows, uint64_t rows_ms, int32_t* __restrict__ out, uint64_t out_ms,
                                     uint32_t* __restrict__ refused) {
  const uint64_t m = blockIdx.y;
  trace_elementwise_rows<15, true, false, SRC>(src_at<SRC>(src, m * src_ms), TraceView{}, nullptr, TraceView{}, n, nd,
                                               TraceDst{rows + m * rows_ms, 0, nullptr}, many_out_base(out, out_ms, m), nullptr,
                                               refused ? refused + m : nullptr);
}
// The elementwise kinds and the float dtypes, each stated once for every launcher that picks an instantiation by them:
// X(K) launches one
#define LMN_ELEMENTWISE_KINDS(kind, what, X)                  \
  switch (kind) {                                             \
    case 0: X(0); break;                                      \
    case 1: X(1); break;                                      \
    case 2: X(2); break;                                      \
    case 7: X(7); break;                                      \
    case 8: X(8); break;                                      \
    case 13: X(13); break;                                    \
    case 15: X(15); break;                                    \
    case 16: X(16); break;                                    \
    default: throw LmnError(-100, what ": unsupported kind"); \
  }
#define LMN_FLOAT_DTYPES(dtype, what, X)                       \
  switch (dtype) {                                             \
    case 0: X(0); break;                                       \
    case 1: X(1); break;                                       \
    case 2: X(2); break;                                       \
    default: throw LmnError(-100, what ": unsupported dtype"); \
  }
void launch_trace_elementwise(int kind, int src_dtype, const TraceOperand& lhs, const TraceOperand& rhs, uint64_t n,
                              const TraceNode& nd, uint32_t* aux, uint64_t aux_ms, const TraceOut& o, lmn_stream_t s) {
  const dim3 g(cdiv(n, TPB), o.form == TraceOut::MANY ? o.n_members : 1), b(TPB);
  if (src_dtype == SRC_FIXED) switch (o.form) {
      case TraceOut::ROWS:
#define LMN_X(K) LMN_LAUNCH(k_trace_elementwise<K>, g, b, 0, s, lhs.p, lhs.view, rhs.p, rhs.view, n, nd, o.rows, o.out, aux)
        LMN_ELEMENTWISE_KINDS(kind, "trace_elementwise", LMN_X)
#undef LMN_X
        break;
      case TraceOut::COLS:
#define LMN_X(K)                                                                                                          \
  LMN_LAUNCH(k_sink_elementwise<K>, g, b, 0, s, lhs.p, lhs.view, rhs.p, rhs.view, n, nd, o.cols, o.col_stride, o.out, aux, \
             o.bad_word, o.refused)
        LMN_ELEMENTWISE_KINDS(kind, "trace_elementwise_cols", LMN_X)
#undef LMN_X
        break;
      case TraceOut::MANY:
#define LMN_X(K)                                                                                                             \
  LMN_LAUNCH(k_trace_many_elementwise<K>, g, b, 0, s, lhs.p, lhs.view, lhs.ms, rhs.p, rhs.view, rhs.ms, n, nd, o.rows, o.rows_ms, \
             o.out, o.out_ms, aux, aux_ms, o.refused)
        LMN_ELEMENTWISE_KINDS(kind, "trace_many_elementwise", LMN_X)
#undef LMN_X
        break;
    }
  else switch (o.form) {   // the float source is Inputs' alone
      case TraceOut::ROWS:
#define LMN_X(S) LMN_LAUNCH(k_trace_inputs_float<S>, g, b, 0, s, lhs.p, n, nd, o.rows, o.out)
        LMN_FLOAT_DTYPES(src_dtype, "trace_inputs_float", LMN_X)
#undef LMN_X
        break;
      case TraceOut::COLS:
#define LMN_X(S) LMN_LAUNCH(k_sink_inputs_float<S>, g, b, 0, s, lhs.p, n, nd, o.cols, o.col_stride, o.out, o.bad_word, o.refused)
        LMN_FLOAT_DTYPES(src_dtype, "trace_inputs_float_cols", LMN_X)
#undef LMN_X
        break;
      case TraceOut::MANY:
#define LMN_X(S) \
  LMN_LAUNCH(k_trace_many_inputs_float<S>, g, b, 0, s, lhs.p, lhs.ms, n, nd, o.rows, o.rows_ms, o.out, o.out_ms, o.refused)
        LMN_FLOAT_DTYPES(src_dtype, "trace_many_inputs_float", LMN_X)
#undef LMN_X
        break;
    }
}

// LookupLayout::find_index: the LUT row of the range that holds `a`, -1 when no range does (few ranges: a linear scan of
// block-uniform bounds)
LMN_D int64_t lut_find_index(const LutRanges& rg, int64_t a) {
  int64_t li = -1;
  for (int k = 0; k < rg.n; ++k)
    if (a >= (int64_t)rg.lo[k] && a <= (int64_t)rg.hi[k]) li = (int64_t)rg.base[k] + (a - (int64_t)rg.lo[k]);
  return li;
}
// a LUT output word as the tensor value it stands for
LMN_D int32_t lut_out_value(uint32_t ow) { return ow > (P31 >> 1) ? (int32_t)ow - (int32_t)P31 : (int32_t)ow; }

// Sin / Exp2 / Log2 rows (sin/table.rs: node, input, idx, is_last, next_node, next_input, next_idx, input, out,
// input_mult, out_mult, lookup_mult) with out read from the LUT's output column, plus the LUT multiplicities.
// (the row rule once, for k_trace_lut and k_trace_many_lut.  An input outside every range: its row is marked; the single form
// also raises *err_flag - the call fails - the many form and the column form count it as a refused element in *refused)
template <bool MANY, bool COLS = false>
LMN_D void trace_lut_rows(const int32_t* __restrict__ input, const TraceView& view, uint64_t n, const TraceNode& nd,
                          const uint32_t* __restrict__ lut1, const LutRanges& rg, uint32_t* __restrict__ mult,
                          const TraceDst& dst, int32_t* __restrict__ out, uint32_t* __restrict__ err_flag,
                          uint32_t* __restrict__ refused) {
  static_assert(!(MANY && COLS), "the many-member forms keep rows only");
  constexpr int NC = 12;
  RowOut<NC, COLS> ro;
  const uint64_t row0 = (uint64_t)blockIdx.x * TPB;
  const uint64_t r = row0 + threadIdx.x;
  bool bad = false;
  if (r < n) {
    const int64_t a = input[view_offset(view, r)];
    const int64_t li = lut_find_index(rg, a);
    uint32_t ow = P31;  // an input outside every range
    if (li < 0) {
      bad = true;
      if constexpr (!MANY && !COLS) *err_flag = 1u;
    } else {
      ow = lut1[li];
      atomicAdd(&mult[li], 1u);
    }
    uint32_t* t = ro.t;
    t[0] = nd.node_id; t[1] = nd.lhs_id; t[2] = (uint32_t)r; t[3] = r + 1 == n ? 1u : 0u;
    t[4] = nd.node_id; t[5] = nd.lhs_id; t[6] = (uint32_t)r + 1u;
    t[7] = fixed_to_m31(a); t[8] = ow; t[9] = nd.lhs_mult; t[10] = nd.out_mult; t[11] = 1u;
    if (out) out[r] = lut_out_value(ow);
  }
  if constexpr (MANY || COLS) trace_count_refused(bad, refused);
  ro.store(dst, row0, n, r < n, bad);
}

LMN_KERNEL k_trace_lut(const int32_t* __restrict__ input, TraceView view, uint64_t n, TraceNode nd,
                       const uint32_t* __restrict__ lut1, LutRanges rg, uint32_t* __restrict__ mult,
                       uint32_t* __restrict__ rows, int32_t* __restrict__ out, uint32_t* __restrict__ err_flag) {
  trace_lut_rows<false>(input, view, n, nd, lut1, rg, mult, TraceDst{rows, 0, nullptr}, out, err_flag, nullptr);
}
LMN_KERNEL k_sink_lut(const int32_t* __restrict__ input, TraceView view, uint64_t n, TraceNode nd,
                            const uint32_t* __restrict__ lut1, LutRanges rg, uint32_t* __restrict__ mult,
                            uint32_t* __restrict__ cols, uint64_t col_stride, int32_t* __restrict__ out,
                            uint32_t* __restrict__ bad_word, uint32_t* __restrict__ refused) {
  trace_lut_rows<false, true>(input, view, n, nd, lut1, rg, mult, TraceDst{cols, col_stride, bad_word}, out, nullptr, refused);
}
// lut1 is shared by all members; the multiplicity atomics go to the member's own table
LMN_KERNEL k_trace_many_lut(const int32_t* __restrict__ input, TraceView view, uint64_t in_ms, uint64_t n, TraceNode nd,
                            const uint32_t* __restrict__ lut1, LutRanges rg, uint32_t* __restrict__ mult, uint64_t mult_ms,
                            uint32_t* __restrict__ rows, uint64_t rows_ms, int32_t* __restrict__ out, uint64_t out_ms,
                            uint32_t* __restrict__ refused) {
  const uint64_t m = blockIdx.y;
  trace_lut_rows<true>(input + m * in_ms, view, n, nd, lut1, rg, mult + m * mult_ms, TraceDst{rows + m * rows_ms, 0, nullptr},
                       many_out_base(out, out_ms, m), nullptr, refused ? refused + m : nullptr);
}

void launch_trace_lut(const TraceOperand& input, uint64_t n, const TraceNode& nd, const uint32_t* lut_col1,
                      const LutRanges& ranges, uint32_t* mult, uint64_t mult_ms, const TraceOut& o, lmn_stream_t s) {
  const dim3 g(cdiv(n, TPB), o.form == TraceOut::MANY ? o.n_members : 1), b(TPB);
  switch (o.form) {
    case TraceOut::ROWS:
      LMN_LAUNCH(k_trace_lut, g, b, 0, s, input.p, input.view, n, nd, lut_col1, ranges, mult, o.rows, o.out, o.err_flag);
      break;
    case TraceOut::COLS:
      LMN_LAUNCH(k_sink_lut, g, b, 0, s, input.p, input.view, n, nd, lut_col1, ranges, mult, o.cols, o.col_stride, o.out,
                 o.bad_word, o.refused);
      break;
    case TraceOut::MANY:
      LMN_LAUNCH(k_trace_many_lut, g, b, 0, s, input.p, input.view, input.ms, n, nd, lut_col1, ranges, mult, mult_ms, o.rows,
                 o.rows_ms, o.out, o.out_ms, o.refused);
      break;
  }
}

// =============================================================================================
// The eval forms (`Operator::process`, the forward pass in front of gen_trace): the same value rules, no rows.  Every launch
// also leaves the minimum and maximum of the values it wrote in minmax[0 .. 1] - the range of a buffer is known when the
// buffer is produced (`buffer.min_max()` of gen_circuit_settings, crates/graph/src/utils.rs:44-82) - and adds the number
// of refused elements to *refused; a refused element's 0 takes part in the range, the buffer holds it.
// =============================================================================================
LMN_D int32_t wave_min_i32(int32_t v) {
  for (int m = 32; m > 0; m >>= 1) {
    const int32_t o = (int32_t)lmn_shfl_xor((uint32_t)v, m);
    v = o < v ? o : v;
  }
  return v;
}
LMN_D int32_t wave_max_i32(int32_t v) {
  for (int m = 32; m > 0; m >>= 1) {
    const int32_t o = (int32_t)lmn_shfl_xor((uint32_t)v, m);
    v = o > v ? o : v;
  }
  return v;
}
LMN_D uint32_t wave_sum_u32(uint32_t v) {
  for (int m = 32; m > 0; m >>= 1) v += (uint32_t)lmn_shfl_xor(v, m);
  return v;
}
// End of every eval kernel, reached by all TPB lanes: lo / hi = the lane's own range (INT32_MAX / INT32_MIN for a lane that
// wrote nothing), wave_bad = the wave's refused elements (wave-uniform).  Per wave by xor shuffles, per workgroup through
// LDS, then one atomicMin, one atomicMax and - only when something was refused - one atomicAdd per workgroup.
LMN_D void eval_finish(int32_t lo, int32_t hi, uint32_t wave_bad, int32_t* __restrict__ minmax, uint32_t* __restrict__ refused) {
  LMN_SHARED int32_t s_lo[TPB / 64], s_hi[TPB / 64];
  LMN_SHARED uint32_t s_bad[TPB / 64];
  lo = wave_min_i32(lo);
  hi = wave_max_i32(hi);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0u) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
    s_bad[wave] = wave_bad;
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t bad = 0u;
    for (int w = 0; w < TPB / 64; ++w) {
      lo = s_lo[w] < lo ? s_lo[w] : lo;
      hi = s_hi[w] > hi ? s_hi[w] : hi;
      bad += s_bad[w];
    }
    if (minmax && lo <= hi) {
      atomicMin(&minmax[0], lo);
      atomicMax(&minmax[1], hi);
    }
    if (refused && bad) atomicAdd(refused, bad);
  }
}

LMN_KERNEL k_eval_init(int32_t* __restrict__ minmax) {
  if (blockIdx.x == 0u && threadIdx.x == 0u) {
    minmax[0] = INT32_MAX;
    minmax[1] = INT32_MIN;
  }
}
void launch_eval_init(int32_t* minmax, lmn_stream_t s) { LMN_LAUNCH(k_eval_init, dim3(1), dim3(64), 0, s, minmax); }

// One lane per element, operands through their views, coalesced int32 stores; no LDS tile, and LessThan touches no
// multiplicity table.
// (the body once, for k_eval_elementwise and k_eval_inputs_float: SRC as in trace_elementwise_rows)
template <int KIND, int SRC = SRC_FIXED>
LMN_D void eval_elementwise_values(const int32_t* __restrict__ lhs, const TraceView& lv, const int32_t* __restrict__ rhs,
                                   const TraceView& rv, uint64_t n, int32_t* __restrict__ out, int32_t* __restrict__ minmax,
                                   uint32_t* __restrict__ refused) {
  constexpr bool BINARY = KIND == 0 || KIND == 1 || KIND == 8 || KIND == 13;
  const uint64_t r = (uint64_t)blockIdx.x * TPB + threadIdx.x;
  const bool on = r < n;
  int32_t o = 0;
  bool bad = false;
  if (on) {
    const int64_t a = src_value<SRC>(lhs, view_offset(lv, r));
    const int64_t b = BINARY ? (int64_t)rhs[view_offset(rv, r)] : 0;
    const ElemValue e = elem_value<KIND>(a, b);
    o = (int32_t)e.out;
    bad = !e.ok;
    out[r] = o;
  }
  eval_finish(on ? o : INT32_MAX, on ? o : INT32_MIN, wave_count(bad), minmax, refused);
}
template <int KIND>
LMN_KERNEL k_eval_elementwise(const int32_t* __restrict__ lhs, TraceView lv, const int32_t* __restrict__ rhs, TraceView rv,
                              uint64_t n, int32_t* __restrict__ out, int32_t* __restrict__ minmax,
                              uint32_t* __restrict__ refused) {
  eval_elementwise_values<KIND>(lhs, lv, rhs, rv, n, out, minmax, refused);
}
template <int SRC>
LMN_KERNEL k_eval_inputs_float(const int32_t* __restrict__ src, uint64_t n, int32_t* __restrict__ out, int32_t* __restrict__ minmax,
                               uint32_t* __restrict__ refused) {
  eval_elementwise_values<15, SRC>(src, TraceView{}, nullptr, TraceView{}, n, out, minmax, refused);
}

void launch_eval_elementwise(int kind, const int32_t* lhs, const TraceView& lv, const int32_t* rhs, const TraceView& rv,
                             uint64_t n, int32_t* out, int32_t* minmax, uint32_t* refused, lmn_stream_t s) {
  dim3 g(cdiv(n, TPB)), b(TPB);
#define LMN_X(K) LMN_LAUNCH(k_eval_elementwise<K>, g, b, 0, s, lhs, lv, rhs, rv, n, out, minmax, refused)
  LMN_ELEMENTWISE_KINDS(kind, "eval_elementwise", LMN_X)
#undef LMN_X
}

void launch_eval_inputs_float(uint32_t dtype, const void* src, uint64_t n, int32_t* out, int32_t* minmax, uint32_t* refused,
                              lmn_stream_t s) {
  const dim3 g(cdiv(n, TPB)), b(TPB);
  const int32_t* lhs = (const int32_t*)src;
#define LMN_X(S) LMN_LAUNCH(k_eval_inputs_float<S>, g, b, 0, s, lhs, n, out, minmax, refused)
  LMN_FLOAT_DTYPES(dtype, "eval_inputs_float", LMN_X)
#undef LMN_X
}

// lmn_tensor_to_float (`CopyFromStwo`): one lane per element, fixed_to_float_bits, coalesced 4- or 2-byte stores
template <int DT>
LMN_KERNEL k_tensor_to_float(const int32_t* __restrict__ src, uint64_t n, void* __restrict__ dst) {
  const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int32_t v = src[i];
  if (DT == 0) ((uint32_t*)dst)[i] = fixed_to_float_bits<8, 23>(v);
  else if (DT == 1) ((uint16_t*)dst)[i] = (uint16_t)fixed_to_float_bits<5, 10>(v);
  else ((uint16_t*)dst)[i] = (uint16_t)fixed_to_float_bits<8, 7>(v);
}
void launch_tensor_to_float(uint32_t dtype, const int32_t* src, uint64_t n, void* dst, lmn_stream_t s) {
  const dim3 g(cdiv(n, TPB)), b(TPB);
#define LMN_X(S) LMN_LAUNCH(k_tensor_to_float<S>, g, b, 0, s, src, n, dst)
  LMN_FLOAT_DTYPES(dtype, "tensor_to_float", LMN_X)
#undef LMN_X
}
#undef LMN_FLOAT_DTYPES
#undef LMN_ELEMENTWISE_KINDS

// out = lut_col1[find_index(input)]; an input outside every range is a refused element (the trace form fails the call
// instead: a dry run must not wait per node).  No multiplicity increments.
LMN_KERNEL k_eval_lut(const int32_t* __restrict__ input, TraceView view, uint64_t n, const uint32_t* __restrict__ lut1,
                      LutRanges rg, int32_t* __restrict__ out, int32_t* __restrict__ minmax, uint32_t* __restrict__ refused) {
  const uint64_t r = (uint64_t)blockIdx.x * TPB + threadIdx.x;
  const bool on = r < n;
  int32_t o = 0;
  bool bad = false;
  if (on) {
    const int64_t li = lut_find_index(rg, (int64_t)input[view_offset(view, r)]);
    bad = li < 0;
    if (!bad) o = lut_out_value(lut1[li]);
    out[r] = o;
  }
  eval_finish(on ? o : INT32_MAX, on ? o : INT32_MIN, wave_count(bad), minmax, refused);
}
void launch_eval_lut(const int32_t* input, const TraceView& view, uint64_t n, const uint32_t* lut_col1, const LutRanges& ranges,
                     int32_t* out, int32_t* minmax, uint32_t* refused, lmn_stream_t s) {
  LMN_LAUNCH(k_eval_lut, dim3(cdiv(n, TPB)), dim3(TPB), 0, s, input, view, n, lut_col1, ranges, out, minmax, refused);
}

// The group rule of SumReduce / MaxReduce, as k_trace_reduce's rows state it: an input outside the value range marks its
// row, the last step's row is marked when its input or the group result is outside it, and only then 0 is written; the
// running sum (int64) may leave the range.  The refused count is the number of marked rows.
template <bool MAX>
LMN_D int64_t reduce_op(int64_t a, int64_t b) { return MAX ? (a > b ? a : b) : a + b; }

// One lane per output element g = i * back + j, walking its group at stride `back`: consecutive lanes read consecutive
// words on every step.  For back >= 64 (a whole wave on one run of words).
template <bool MAX>
LMN_KERNEL k_eval_reduce_lane(const int32_t* __restrict__ input, uint64_t dim, uint64_t back, uint64_t n_out,
                              int32_t* __restrict__ out, int32_t* __restrict__ minmax, uint32_t* __restrict__ refused) {
  const uint64_t g = (uint64_t)blockIdx.x * TPB + threadIdx.x;
  const bool on = g < n_out;
  int32_t o = 0;
  uint32_t bad = 0u;
  if (on) {
    const int32_t* p = input + (g / back) * dim * back + g % back;
    int64_t acc = MAX ? INT64_MIN : 0;
    int64_t v = 0;
    for (uint64_t k = 0; k < dim; ++k) {
      v = (int64_t)p[k * back];
      acc = reduce_op<MAX>(acc, v);
      if (!fixed_ok(v) && k + 1 < dim) ++bad;
    }
    const bool ok = fixed_ok(v) && fixed_ok(acc);
    if (!ok) ++bad;
    o = ok ? (int32_t)acc : 0;
    out[g] = o;
  }
  eval_finish(on ? o : INT32_MAX, on ? o : INT32_MIN, wave_sum_u32(bad), minmax, refused);
}
// One wave per group: lane l reduces steps l, l + 64, ... (back words apart: for a small `back` a wave's 64 loads fall into
// a few cache lines), the wave combines by xor shuffles - the int64 partial as two words.
template <bool MAX>
LMN_KERNEL k_eval_reduce_wave(const int32_t* __restrict__ input, uint64_t dim, uint64_t back, uint64_t n_out,
                              int32_t* __restrict__ out, int32_t* __restrict__ minmax, uint32_t* __restrict__ refused) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t g = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);   // wave-uniform
  const bool on = g < n_out;
  int64_t acc = MAX ? INT64_MIN : 0;
  uint32_t bad = 0u;
  bool last_ok = true;
  if (on) {
    const int32_t* p = input + (g / back) * dim * back + g % back;
    for (uint64_t k = lane; k < dim; k += 64) {
      const int64_t v = (int64_t)p[k * back];
      acc = reduce_op<MAX>(acc, v);
      if (k + 1 < dim) bad += fixed_ok(v) ? 0u : 1u;
      else last_ok = fixed_ok(v);
    }
  }
  for (int m = 32; m > 0; m >>= 1) {
    const uint32_t lo = (uint32_t)lmn_shfl_xor((uint32_t)(uint64_t)acc, m), hi = (uint32_t)lmn_shfl_xor((uint32_t)((uint64_t)acc >> 32), m);
    acc = reduce_op<MAX>(acc, (int64_t)((uint64_t)hi << 32 | lo));
  }
  bad = wave_sum_u32(bad);
  const bool ok = wave_count(!last_ok) == 0u && fixed_ok(acc);
  const int32_t o = ok ? (int32_t)acc : 0;
  const bool writer = on && lane == 0u;
  if (writer) out[g] = o;
  eval_finish(writer ? o : INT32_MAX, writer ? o : INT32_MIN, on ? bad + (ok ? 0u : 1u) : 0u, minmax, refused);
}

bool eval_reduce_by_wave(uint64_t dim, uint64_t back) { return back < 64; }

void launch_eval_reduce(bool is_max, const int32_t* input, uint64_t front, uint64_t dim, uint64_t back, int32_t* out,
                        int32_t* minmax, uint32_t* refused, lmn_stream_t s) {
  const uint64_t n_out = front * back;
  if (eval_reduce_by_wave(dim, back)) {
    const dim3 g(cdiv(n_out, TPB / 64)), b(TPB);
    if (is_max) LMN_LAUNCH(k_eval_reduce_wave<true>, g, b, 0, s, input, dim, back, n_out, out, minmax, refused);
    else LMN_LAUNCH(k_eval_reduce_wave<false>, g, b, 0, s, input, dim, back, n_out, out, minmax, refused);
  } else {
    const dim3 g(cdiv(n_out, TPB)), b(TPB);
    if (is_max) LMN_LAUNCH(k_eval_reduce_lane<true>, g, b, 0, s, input, dim, back, n_out, out, minmax, refused);
    else LMN_LAUNCH(k_eval_reduce_lane<false>, g, b, 0, s, input, dim, back, n_out, out, minmax, refused);
  }
}

// lmn_tensor_range: the range of a buffer no eval call produced.  Grid-stride over at most 1024 workgroups.
LMN_KERNEL k_tensor_range(const int32_t* __restrict__ buf, uint64_t n, int32_t* __restrict__ minmax) {
  int32_t lo = INT32_MAX, hi = INT32_MIN;
  for (uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TPB) {
    const int32_t v = buf[i];
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  eval_finish(lo, hi, 0u, minmax, nullptr);
}
void launch_tensor_range(const int32_t* buf, uint64_t n, int32_t* minmax, lmn_stream_t s) {
  const unsigned blocks = cdiv(n, TPB);
  LMN_LAUNCH(k_tensor_range, dim3(blocks < 1024u ? blocks : 1024u), dim3(TPB), 0, s, buf, n, minmax);
}

// =============================================================================================
// lmn_trace_check: the rows that break a local constraint, the logup tuples that do not balance
// =============================================================================================
// add `w` to the tuple `key` of one element set and lower its first mention: linear probing, the slot claimed by a 64-bit
// compare-and-swap on the key.  The plain reads in front of the atomics can only be stale towards "free" and "larger", in
// which case the atomic decides; the table holds at most half as many keys as slots, so the walk ends.
LMN_D void tc_insert(const TcSet S, unsigned long long key, unsigned long long w, unsigned long long mention) {
  unsigned long long x = (key ^ (key >> 29)) * 0x9E3779B97F4A7C15ull;
  uint64_t h = (x >> 24) & S.mask;
  for (;;) {
    unsigned long long k = S.keys[h];
    if (k == TC_EMPTY) k = atomicCAS(&S.keys[h], TC_EMPTY, key);
    if (k == TC_EMPTY || k == key) break;
    h = (h + 1) & S.mask;
  }
  atomicAdd(&S.sums[h], w);
  if (S.firsts[h] > mention) atomicMin(&S.firsts[h], mention);
}

// One lane per real row.  COLS: the table is column-major (a finished row sink) and a lane's words are coalesced column
// reads; otherwise the workgroup's TPB x NC words are one contiguous run of the row-major table, staged through LDS with
// an odd row pitch (a row is 7 .. 22 words: per-lane global reads of it would be 28 .. 88-byte strides).  Per local slot: a
// wave ballot, and only when it is non-zero one atomicAdd of its population count and one atomicMin of the wave's smallest
// row, by the leader - a clean trace issues no atomic here.  Relation entries with a non-zero multiplicity go to their
// element set's tuple table; LessThan's limbs (4 per row on the 256 keys of the range check) are summed per workgroup in
// LDS, direct-indexed, and reach the table once per workgroup.
template <int KIND, bool COLS>
LMN_KERNEL k_trace_check(TcTable tb, TcOut out) {
  constexpr int NC = kSpecs[KIND].n_cols, NL = kSpecs[KIND].n_local, ST = NC | 1;
  LMN_SHARED uint32_t tile[COLS ? 1 : TPB * ST];
  LMN_SHARED unsigned long long rc_sum[KIND == 13 ? 256 : 1], rc_first[KIND == 13 ? 256 : 1];
  const uint64_t row0 = (uint64_t)blockIdx.x * TPB;
  const uint64_t r = row0 + threadIdx.x;
  const bool on = r < tb.n_rows;
  uint32_t c[NC];
  if constexpr (COLS) {
#pragma unroll
    for (int k = 0; k < NC; ++k) c[k] = on ? tb.data[(uint64_t)k * tb.stride + r] : 0u;
  } else {
    const uint64_t rows_here = tb.n_rows - row0 < (uint64_t)TPB ? tb.n_rows - row0 : (uint64_t)TPB;
    const uint32_t words = (uint32_t)rows_here * NC;
    const uint32_t* __restrict__ src = tb.data + row0 * NC;
    for (uint32_t w = threadIdx.x; w < words; w += TPB) tile[(w / NC) * ST + (w % NC)] = src[w];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NC; ++k) c[k] = on ? tile[threadIdx.x * ST + k] : 0u;
  }
  if constexpr (KIND == 13) {
    rc_sum[threadIdx.x] = 0ull;       // TPB == 256 keys
    rc_first[threadIdx.x] = TC_EMPTY;
    __syncthreads();
  }
  // words that are no canonical M31: counted, the smallest (table, row, column) kept, and the row is out of both checks
  uint32_t n_bad = 0u, first_bad = 0u;
#pragma unroll
  for (int k = NC - 1; k >= 0; --k)
    if (c[k] >= P31) {
      ++n_bad;
      first_bad = (uint32_t)k;
    }
  if (n_bad) {
    atomicAdd(&out.noncanon[0], (unsigned long long)n_bad);
    atomicMin(&out.noncanon[1], (unsigned long long)tb.table << 40 | r << 8 | first_bad);
  }
  const bool live = on && n_bad == 0u;
  const unsigned lane = threadIdx.x & 63u;
  if constexpr (NL > 0) {
    uint32_t v[NL];   // the component's local constraints on this row, one per slot (constraints.h)
    int n = 0;
    local_constraints<KIND>(c, [&](uint32_t x) { v[n++] = x; });
#pragma unroll
    for (int sl = 0; sl < NL; ++sl) {
      const unsigned long long bal = lmn_ballot(live && v[sl] != 0u);
      if (bal != 0ull && lane == (unsigned)__builtin_ctzll(bal)) {   // the leader holds the wave's smallest violating row
        atomicAdd(&out.slot_count[tb.table * TC_MAX_SLOTS + sl], (uint32_t)__builtin_popcountll(bal));
        atomicMin(&out.slot_first[tb.table * TC_MAX_SLOTS + sl], (unsigned long long)r);
      }
    }
  }
  auto word = [&](int col) -> uint32_t {   // a relation's column is launch-uniform data, not a register index: read it again
    if constexpr (COLS) return tb.data[(uint64_t)col * tb.stride + r];
    else return tile[threadIdx.x * ST + col];
  };
  // (the relation wiring is read from the argument block at constant offsets - a loop over it would be indexed by a register
  // and the block copied to scratch)
  auto relation = [&](int j, int mult_col, int val_col, int id_col, int set, int neg, int pre) {
    if (j >= tb.n_rel || !live) return;
    const uint32_t mult = word(mult_col);
    if (mult == 0u) return;
    uint32_t val, id = 0u;
    if (pre) {
      val = tb.pre0 ? tb.pre0[r] : (uint32_t)r;
      if (id_col >= 0) id = tb.pre1[r];
    } else {
      val = word(val_col);
      if (id_col >= 0) id = word(id_col);
    }
    const unsigned long long w = neg ? P31 - mult : mult;
    const unsigned long long mention = (unsigned long long)tb.table << 40 | (unsigned long long)(tb.slot0 + j) << 32 | r;
    if (KIND == 13 && set == 1 && val < 256u) {
      atomicAdd(&rc_sum[val], w);
      atomicMin(&rc_first[val], mention);
    } else {
      tc_insert(out.sets[set], (unsigned long long)val | (unsigned long long)id << 31, w, mention);
    }
  };
#define LMN_TC_REL(J) relation(J, tb.rel_mult[J], tb.rel_val[J], tb.rel_id[J], tb.rel_set[J], tb.rel_neg[J], tb.rel_pre[J])
  LMN_TC_REL(0); LMN_TC_REL(1); LMN_TC_REL(2); LMN_TC_REL(3); LMN_TC_REL(4); LMN_TC_REL(5); LMN_TC_REL(6);
#undef LMN_TC_REL
  if constexpr (KIND == 13) {
    __syncthreads();
    if (rc_first[threadIdx.x] != TC_EMPTY) tc_insert(out.sets[1], threadIdx.x, rc_sum[threadIdx.x], rc_first[threadIdx.x]);
  }
}

void launch_trace_check(int kind, bool cols_layout, const TcTable& tb, const TcOut& out, lmn_stream_t s) {
  if (tb.n_rows == 0 || tb.n_rows > (1ull << 26)) throw LmnError(-100, "trace check: bad row count");
  if (cols_layout && tb.n_rows > tb.stride) throw LmnError(-100, "trace check: rows outside the columns");
  const dim3 g(cdiv(tb.n_rows, TPB)), b(TPB);
#define LMN_TC_CASE(K)                                                             \
  case K:                                                                          \
    if (cols_layout) LMN_LAUNCH((k_trace_check<K, true>), g, b, 0, s, tb, out);    \
    else LMN_LAUNCH((k_trace_check<K, false>), g, b, 0, s, tb, out);               \
    break;
  switch (kind) {
    LMN_TC_CASE(0) LMN_TC_CASE(1) LMN_TC_CASE(2) LMN_TC_CASE(3) LMN_TC_CASE(4) LMN_TC_CASE(5) LMN_TC_CASE(6) LMN_TC_CASE(7)
    LMN_TC_CASE(8) LMN_TC_CASE(9) LMN_TC_CASE(10) LMN_TC_CASE(11) LMN_TC_CASE(12) LMN_TC_CASE(13) LMN_TC_CASE(14)
    LMN_TC_CASE(15) LMN_TC_CASE(16)
    default: throw LmnError(-100, "trace check: unsupported kind");
  }
#undef LMN_TC_CASE
}

// One lane per slot of a tuple table: the sum reduced mod P, the non-zero ones counted (one atomicAdd per wave) and the
// first `cap` of them compacted into `found`.
LMN_KERNEL k_trace_check_collect(TcSet S, uint32_t set_index, unsigned long long* __restrict__ n_unbalanced,
                                 TcFound* __restrict__ found, uint32_t cap) {
  LMN_SHARED unsigned long long wave_base[TPB / 64];
  const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
  unsigned long long key = TC_EMPTY;
  if (i <= S.mask) key = S.keys[i];
  uint32_t net = 0u;
  if (key != TC_EMPTY) net = m_red64(S.sums[i]);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long bal = lmn_ballot(net != 0u);
  if (bal != 0ull && lane == (unsigned)__builtin_ctzll(bal))
    wave_base[wave] = atomicAdd(n_unbalanced, (unsigned long long)__builtin_popcountll(bal));
  __syncthreads();
  if (net != 0u) {
    const unsigned long long at = wave_base[wave] + (unsigned long long)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
    if (at < cap) {
      TcFound f;
      f.key = key;
      f.first = S.firsts[i];
      f.set = set_index;
      f.net = net;
      found[at] = f;
    }
  }
}
void launch_trace_check_collect(const TcSet& set, uint32_t set_index, unsigned long long* n_unbalanced, TcFound* found,
                                uint32_t cap, lmn_stream_t s) {
  LMN_LAUNCH(k_trace_check_collect, dim3(cdiv(set.mask + 1, TPB)), dim3(TPB), 0, s, set, set_index, n_unbalanced, found, cap);
}

// =============================================================================================
// lmn_settings_prepare: blockIdx.y selects the column.  A LUT column is only read - a word that is not a canonical M31
// names its column in the object's flag word (plain stores; whichever offender stores last wins, any of them refuses the
// settings) - and the 8-bit range-check column, the last y, is written: row r holds r (preprocessed.rs:289-296).
// =============================================================================================
LMN_KERNEL k_settings_prepare(PrepareCols p, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int c = (int)blockIdx.y;
  if (c < p.n_luts) {
    if (i < p.n[c] && p.lut[c][i] >= P31) *flag = (uint32_t)c + 1u;
  } else if (p.range_check && i < p.range_n) {
    p.range_check[i] = (uint32_t)i;
  }
}
void launch_settings_prepare(const PrepareCols& cols, uint32_t* flag, lmn_stream_t s) {
  if (cols.n_luts < 0 || cols.n_luts > PREPARE_MAX_LUT_COLS) throw LmnError(-100, "settings_prepare: bad column count");
  uint32_t longest = cols.range_check ? cols.range_n : 0u;
  for (int c = 0; c < cols.n_luts; ++c) longest = std::max(longest, cols.n[c]);
  const int ny = cols.n_luts + (cols.range_check ? 1 : 0);
  if (ny == 0 || longest == 0) return;
  LMN_LAUNCH(k_settings_prepare, dim3(cdiv(longest, TPB), ny), dim3(TPB), 0, s, cols, flag);
}

// =============================================================================================
// level-2 column ops: bit reversal, FriOps::decompose, FieldOps::batch_inverse
// =============================================================================================
LMN_KERNEL k_bit_reverse(uint32_t* __restrict__ data, uint64_t col_stride, int log_n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1ull << log_n)) return;
  const uint64_t j = log_n == 0 ? 0 : (uint64_t)(__brev((uint32_t)i) >> (32 - log_n));
  if (i >= j) return;  // each unordered pair is swapped once, by its smaller index
  uint32_t* col = data + (uint64_t)blockIdx.y * col_stride;
  const uint32_t a = col[i], b = col[j];
  col[i] = b;
  col[j] = a;
}
void launch_bit_reverse(uint32_t* data, uint64_t col_stride, int ncols, int log_n, lmn_stream_t s) {
  if (log_n > 32) throw LmnError(-100, "bit_reverse: column too large");
  LMN_LAUNCH(k_bit_reverse, dim3(cdiv(1ull << log_n, TPB), ncols), dim3(TPB), 0, s, data, col_stride, log_n);
}

int decompose_num_blocks(int log_n) { return log_n < 1 ? 1 : (int)cdiv(1ull << (log_n - 1), TPB); }

// partial[b] = sum over the block's i < n/2 of f[i] - f[i + n/2]
LMN_KERNEL k_decompose_partial(const uint32_t* __restrict__ f, int log_n, QM31* __restrict__ partial) {
  LMN_SHARED QM31 red[TPB];
  const uint64_t n = 1ull << log_n, half = n >> 1;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  QM31 v = q_zero();
  if (i < half) {
    const QM31 a = load_secure_col(f, n, i), b = load_secure_col(f, n, i + half);
    v = q_sub(a, b);
  }
  red[threadIdx.x] = v;
  __syncthreads();
  for (int st = TPB / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] = q_add(red[threadIdx.x], red[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
// lambda = (sum of partials) * n_inv
LMN_KERNEL k_decompose_lambda(const QM31* __restrict__ partial, int nblocks, uint32_t n_inv, QM31* __restrict__ lambda) {
  LMN_SHARED QM31 red[TPB];
  QM31 acc = q_zero();
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) acc = q_add(acc, partial[b]);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int st = TPB / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] = q_add(red[threadIdx.x], red[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *lambda = q_mul_m(red[0], n_inv);
}
LMN_KERNEL k_decompose_apply(const uint32_t* __restrict__ f, int log_n, uint32_t* __restrict__ g,
                             const QM31* __restrict__ lambda) {
  const uint64_t n = 1ull << log_n;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const QM31 l = *lambda, v = load_secure_col(f, n, i);
  const QM31 r = i >= (n >> 1) ? q_add(v, l) : q_sub(v, l);
  g[i] = r.a;
  g[n + i] = r.b;
  g[2 * n + i] = r.c;
  g[3 * n + i] = r.d;
}
void launch_decompose(const uint32_t* f, int log_n, uint32_t* g, QM31* lambda_out, QM31* scratch, lmn_stream_t s) {
  if (log_n < 1) throw LmnError(-100, "decompose: a circle domain has at least two points");
  const int nb = decompose_num_blocks(log_n);
  LMN_LAUNCH(k_decompose_partial, dim3(nb), dim3(TPB), 0, s, f, log_n, scratch);
  int e = (31 - (log_n % 31)) % 31;  // 2^-log_n mod P
  LMN_LAUNCH(k_decompose_lambda, dim3(1), dim3(TPB), 0, s, scratch, nb, 1u << e, lambda_out);
  LMN_LAUNCH(k_decompose_apply, dim3(cdiv(1ull << log_n, TPB)), dim3(TPB), 0, s, f, log_n, g, lambda_out);
}

// ---- FieldOps::batch_inverse (lmn_col_batch_inverse / _secure): Montgomery's trick inside a lane.  A workgroup owns a tile
// of TPB * E consecutive words of one column (blockIdx.y: the flat index of ncols << log_n words is never formed); lane t
// owns the words t, t + TPB, ... of it, so every load and store of a wave is one contiguous run of 64 dwords.  The lane
// reads its E elements, multiplies them up (E - 1 products), inverts the total once (m_inv: 37 products) and walks back
// (2 products per element): 3 + 37 / E products per element instead of 37.  A zero enters the chain as 1 and leaves as 0,
// and so does a word past the column's end, which is neither stored nor counted.  Every store of a lane depends on the
// one inverse, which depends on all of its loads: a lane has read all it owns before it writes, so dst may be src.
// E: profiles/field_ops_rate.json (tools/field_ops_rate.py; docs/HISTORY.md has the sweep).
constexpr int BATCH_INV_E_M31 = 16;
constexpr int BATCH_INV_E_QM31 = 8;

// the zeros the lanes of a workgroup saw, reached by all TPB lanes: per wave by xor shuffles, per workgroup through LDS,
// then - only when there was one - one atomicAdd per workgroup (as eval_finish)
LMN_D void zero_count_finish(uint32_t lane_zeros, unsigned long long* n_zero) {
  LMN_SHARED uint32_t s_zeros[TPB / 64];
  const uint32_t wave_zeros = wave_sum_u32(lane_zeros);
  if ((threadIdx.x & 63u) == 0u) s_zeros[threadIdx.x >> 6] = wave_zeros;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t z = 0u;
    for (int w = 0; w < TPB / 64; ++w) z += s_zeros[w];
    if (z) atomicAdd(n_zero, (unsigned long long)z);
  }
}

// x[0 .. E) non-zero -> their inverses, in place
template <int E>
LMN_D void m_inv_chain(uint32_t (&x)[E]) {
  uint32_t pre[E];  // pre[e] = x[0] * ... * x[e]
  pre[0] = x[0];
#pragma unroll
  for (int e = 1; e < E; ++e) pre[e] = m_mul(pre[e - 1], x[e]);
  uint32_t inv = m_inv(pre[E - 1]);  // (x[0] * ... * x[e])^-1 while the walk is at e
#pragma unroll
  for (int e = E - 1; e > 0; --e) {
    const uint32_t r = m_mul(inv, pre[e - 1]);
    inv = m_mul(inv, x[e]);
    x[e] = r;
  }
  x[0] = inv;
}

template <int E>
LMN_KERNEL k_batch_inverse_m(const uint32_t* src, uint32_t* dst, uint64_t col_stride, uint32_t n, unsigned long long* n_zero) {
  const uint32_t* s = src + (uint64_t)blockIdx.y * col_stride;
  uint32_t* d = dst + (uint64_t)blockIdx.y * col_stride;
  const uint32_t i0 = blockIdx.x * (uint32_t)(TPB * E) + threadIdx.x;  // n <= 2^27: no wrap
  uint32_t x[E];
  uint32_t zero_mask = 0u, zeros = 0u;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t i = i0 + (uint32_t)e * TPB;
    const bool in = i < n;
    const uint32_t v = in ? ld_ub(s, i) : 0u;
    const bool zero = v == 0u;
    zeros += in && zero ? 1u : 0u;
    zero_mask |= (zero ? 1u : 0u) << e;
    x[e] = zero ? 1u : v;
  }
  m_inv_chain<E>(x);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t i = i0 + (uint32_t)e * TPB;
    if (i < n) st_ub(d, i, (zero_mask >> e) & 1u ? 0u : x[e]);
  }
  if (n_zero) zero_count_finish(zeros, n_zero);
}

// QM31 through the norms (q_inv's own route, its one m_inv shared by the lane's E elements): per element
// den = A^2 - (2 + i) B^2 in CM31 and nrm = |den|^2 in M31; the norms go through the chain; then den^-1 = conj(den) / nrm
// and the result is (A den^-1, -B den^-1).  QM31 is a field, so nrm == 0 exactly for the zero element.  All words are
// canonical, so the bytes are q_inv's whatever E is.
template <int E>
LMN_KERNEL k_batch_inverse_q(const uint32_t* src, uint32_t* dst, uint32_t n, unsigned long long* n_zero) {
  const uint32_t i0 = blockIdx.x * (uint32_t)(TPB * E) + threadIdx.x;
  CM31 A[E], B[E], den[E];
  uint32_t nrm[E];
  uint32_t zero_mask = 0u, zeros = 0u;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t i = i0 + (uint32_t)e * TPB;
    const bool in = i < n;
    const QM31 v = in ? load_secure_ub(src, n, i) : q_zero();
    A[e] = {v.a, v.b};
    B[e] = {v.c, v.d};
    den[e] = c_sub(c_mul(A[e], A[e]), c_mul_r(c_mul(B[e], B[e])));
    const uint32_t nn = c_norm(den[e]);
    const bool zero = nn == 0u;
    zeros += in && zero ? 1u : 0u;
    zero_mask |= (zero ? 1u : 0u) << e;
    nrm[e] = zero ? 1u : nn;
  }
  m_inv_chain<E>(nrm);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const uint32_t i = i0 + (uint32_t)e * TPB;
    if (i >= n) continue;
    const CM31 di{m_mul(den[e].a, nrm[e]), m_mul(m_neg(den[e].b), nrm[e])};
    const CM31 lo = c_mul(A[e], di), hi = c_mul(B[e], di);
    const bool zero = (zero_mask >> e) & 1u;
    st_ub(dst, i, zero ? 0u : lo.a);
    st_ub(dst + n, i, zero ? 0u : lo.b);
    st_ub(dst + 2ull * n, i, zero ? 0u : m_neg(hi.a));
    st_ub(dst + 3ull * n, i, zero ? 0u : m_neg(hi.b));
  }
  if (n_zero) zero_count_finish(zeros, n_zero);
}

void launch_batch_inverse_m31(const uint32_t* src, uint32_t* dst, uint64_t col_stride, int ncols, int log_n,
                              unsigned long long* n_zero, lmn_stream_t s) {
  if (log_n < 0 || log_n > 27 || ncols < 1 || ncols > 65535) throw LmnError(-100, "batch_inverse: bad shape");
  constexpr int E = BATCH_INV_E_M31;
  LMN_LAUNCH(k_batch_inverse_m<E>, dim3(cdiv(1ull << log_n, TPB * E), ncols), dim3(TPB), 0, s, src, dst, col_stride,
             1u << log_n, n_zero);
}
void launch_batch_inverse_qm31(const uint32_t* src, uint32_t* dst, int log_n, unsigned long long* n_zero, lmn_stream_t s) {
  if (log_n < 0 || log_n > 27) throw LmnError(-100, "batch_inverse_secure: bad shape");
  constexpr int E = BATCH_INV_E_QM31;
  LMN_LAUNCH(k_batch_inverse_q<E>, dim3(cdiv(1ull << log_n, TPB * E)), dim3(TPB), 0, s, src, dst, 1u << log_n, n_zero);
}

}  // namespace lmn
