// gfx950 kernels, part 3: Blake2s Merkle trees in fused subtree launches, the device-resident channel of the FRI commit
// loop, the single-block FRI tail and the decommitment gather.
#include "kernels_common.h"

namespace lmn {

// =============================================================================================
// a4  Blake2s Merkle layer: one lane per node; a wave reads 64 consecutive rows of each column.
// =============================================================================================
LMN_KERNEL k_merkle_layer(const uint32_t* __restrict__ prev, const uint32_t* const* __restrict__ cols, int ncols,
                          uint32_t size, uint32_t* __restrict__ out) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= size) return;
  const int npre = prev ? 16 : 0;
  const int nwords = npre + ncols;
  const int nblocks = (nwords + 15) / 16;
  uint32_t h[8];
  b2_init(h);
  for (int b = 0; b < nblocks; ++b) {
    uint32_t m[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      int w = b * 16 + k;
      uint32_t v = 0u;
      if (w < npre)
        v = prev[(uint64_t)i * 16 + w];
      else if (w < nwords)
        v = cols[w - npre][i];
      m[k] = v;
    }
    bool last = b + 1 == nblocks;
    b2_compress(h, m, last ? (uint32_t)(4 * nwords) : (uint32_t)(64 * (b + 1)), last ? 0xffffffffu : 0u);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) out[(uint64_t)i * 8 + k] = h[k];
}

void launch_merkle_layer(const uint32_t* prev, const uint32_t* const* cols, int ncols, uint32_t size, uint32_t* out,
                         lmn_stream_t s) {
  if (!prev && ncols == 0) throw LmnError(-100, "merkle layer with no input");
  LMN_LAUNCH(k_merkle_layer, dim3(cdiv(size, TPB)), dim3(TPB), 0, s, prev, cols, ncols, size, out);
}

// Fused Merkle subtree.  Every lane owns 2^sub consecutive start-level nodes and reduces them to one
// subtree root in registers (post-order, private LDS slots as the merge stack: all 64 lanes of a
// wave stay busy on every compression); the block's subtree roots then climb further levels
// through LDS.  All levels are written to HBM (decommitment needs them).
// Start-level columns are described as up to MERKLE_MAX_SEG runs of contiguous columns
// (column c of a run lives at base + c*size), so no per-column pointer loads are needed.
LMN_D const uint32_t* merkle_col_ptr(const MerkleSegs& sg, int c, uint64_t size) {
  // c is compile-time after unrolling; the comparisons are wave-uniform scalar work
  int n0 = sg.n[0], n1 = n0 + sg.n[1], n2 = n1 + sg.n[2];
  if (c < n0) return sg.base[0] + (uint64_t)c * size;
  if (c < n1) return sg.base[1] + (uint64_t)(c - n0) * size;
  if (c < n2) return sg.base[2] + (uint64_t)(c - n1) * size;
  return sg.base[3] + (uint64_t)(c - n2) * size;
}
// First 16 message words of start-level node i: the two child hashes when the level has a `prev`
// layer, else its first 16 columns (zero padded).  Split from the hashing so that callers can issue the
// loads of the next node before compressing the current one.
LMN_D void merkle_load_first(const uint32_t* __restrict__ prev, const MerkleSegs& sg, int ncols, uint32_t size,
                             uint32_t i, uint32_t m[16]) {
  if (prev) {
    const uint4* p4 = reinterpret_cast<const uint4*>(prev) + (uint64_t)i * 4;
    uint4 a = p4[0], b = p4[1], c = p4[2], d = p4[3];
    m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w;
    m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
    m[8] = c.x; m[9] = c.y; m[10] = c.z; m[11] = c.w;
    m[12] = d.x; m[13] = d.y; m[14] = d.z; m[15] = d.w;
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = k < ncols ? merkle_col_ptr(sg, k, size)[i] : 0u;
  }
}

// Hash of start-level node i given its first 16 message words (merkle_load_first).
LMN_D void merkle_hash_from(const uint32_t* __restrict__ prev, const MerkleSegs& sg, int ncols, uint32_t size,
                            uint32_t i, uint32_t m[16], uint32_t h[8]) {
  b2_init(h);
  const uint32_t total = (prev ? 64u : 0u) + 4u * (uint32_t)ncols;
  int c0 = prev ? 0 : 16;  // first column not yet consumed
  if (c0 >= ncols) {
    b2_compress(h, m, total, 0xffffffffu);
    return;
  }
  b2_compress(h, m, 64u, 0u);
  uint32_t done = 64u;
  while (c0 < ncols) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      int c = c0 + k;
      m[k] = c < ncols ? merkle_col_ptr(sg, c, size)[i] : 0u;
    }
    c0 += 16;
    bool last = c0 >= ncols;
    done += 64u;
    b2_compress(h, m, last ? total : done, last ? 0xffffffffu : 0u);
  }
}

LMN_D void merkle_hash_start(const uint32_t* __restrict__ prev, const MerkleSegs& sg, int ncols, uint32_t size,
                             uint32_t i, uint32_t h[8]) {
  uint32_t m[16];
  merkle_load_first(prev, sg, ncols, size, i, m);
  merkle_hash_from(prev, sg, ncols, size, i, m, h);
}

// MerkleFold::below: raw words of leaves 2i (m[0..7]) and 2i+1 (m[8..15]) of the level under the start level
LMN_D void merkle_load_below(const uint32_t* __restrict__ below, int below_ncols, uint32_t size, uint32_t i, uint32_t m[16]) {
  const uint64_t L = 2ull * size;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k < below_ncols) {
      ld_ub_pair(below + (uint64_t)k * L, i, m[k], m[8 + k]);   // leaves 2i and 2i+1 of column k: one 8-byte access
    } else {
      m[k] = 0u;
      m[8 + k] = 0u;
    }
  }
}
// start node i = H(H(leaf 2i) || H(leaf 2i+1) || own columns) from the raw leaf words of merkle_load_below
LMN_D void merkle_hash_below(const MerkleSegs& sg, int ncols, uint32_t size, int below_ncols, uint32_t i, const uint32_t m[16],
                             uint32_t h[8]) {
  uint32_t ml[16], mr[16], hl[8], hr[8];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    ml[k] = k < 8 ? m[k] : 0u;
    mr[k] = k < 8 ? m[8 + k] : 0u;
  }
  b2_compress_fresh_nz<8>(hl, ml, 4u * (uint32_t)below_ncols);
  b2_compress_fresh_nz<8>(hr, mr, 4u * (uint32_t)below_ncols);
  uint32_t m2[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    m2[k] = hl[k];
    m2[8 + k] = hr[k];
  }
  // merkle_hash_from only asks whether the node HAS children; their hashes are in m2
  merkle_hash_from(reinterpret_cast<const uint32_t*>(sg.base[0]), sg, ncols, size, i, m2, h);
}

LMN_D void store_hash(uint32_t* __restrict__ o, const uint32_t h[8]) {
  uint4* o4 = reinterpret_cast<uint4*>(o);
  o4[0] = make_uint4(h[0], h[1], h[2], h[3]);
  o4[1] = make_uint4(h[4], h[5], h[6], h[7]);
}

// Quad-cooperative Blake2s of one 64-byte final block (a Merkle parent): lane q of a quad owns column q
// of the 4x4 state (a, b, c, d = rows), so the four G functions of a half-round run on four lanes; the
// diagonal step rotates rows b, c, d by 1, 2, 3 lanes with DPP quad_perm.  Message words are fetched from
// LDS by per-lane sigma offsets.  ~400 issue slots instead of ~1000: single-hash latency 0.93 us vs 2.0 us
// on MI355X (round 2's single-hash microbenchmark, docs/HISTORY.md) - used where a level is too narrow to fill lanes anyway.
// Returns words q and 4+q of the digest.  Must be executed by all four lanes of the quad.
// WS = 0: the 16 message words are contiguous at msg; WS > 0: the two child hashes live in a word-major node array
// (word k of node j at base[k * WS + j]): message word w = msg[(w & 7) * WS + (w >> 3)] with msg = base + 2 * parent.
template <uint32_t WS = 0u>
LMN_D void b2_quad_parent(const uint32_t* msg, uint32_t q, uint32_t& o_lo, uint32_t& o_hi, uint32_t t0 = 64u) {
#define LMN_B2_QW(w) (WS ? msg[((w) & 7u) * WS + ((w) >> 3)] : msg[(w)])
#ifdef LMN_EMU
  // CPU emulation (tests only): a cross-lane rendezvous per DPP move would be a block-wide fiber switch;
  // every lane hashes the block alone and keeps its two words.  The DPP path is checked on the GPU.
  uint32_t h[8], m[16];
  for (uint32_t k = 0; k < 16; ++k) m[k] = LMN_B2_QW(k);
  b2_compress_fresh(h, m, t0);
  o_lo = h[q];
  o_hi = h[4 + q];
  return;
#endif
  const uint32_t iv_lo = q == 0 ? 0x6A09E667u : q == 1 ? 0xBB67AE85u : q == 2 ? 0x3C6EF372u : 0xA54FF53Au;
  const uint32_t iv_hi = q == 0 ? 0x510E527Fu : q == 1 ? 0x9B05688Cu : q == 2 ? 0x1F83D9ABu : 0x5BE0CD19u;
  const uint32_t h_lo = q == 0 ? (0x6A09E667u ^ 0x01010020u) : iv_lo;
  uint32_t a = h_lo, b = iv_hi, c = iv_lo, d = iv_hi ^ (q == 0 ? t0 : q == 2 ? 0xffffffffu : 0u);
  const uint32_t sh8 = 8u * q;
#define LMN_B2_QUAD_ROUND(...)                                            \
  {                                                                       \
    const uint64_t S = LMN_B2_SIGMA_PACK(__VA_ARGS__);                    \
    const uint32_t lo = (uint32_t)(S >> sh8), hi = (uint32_t)(S >> (32u + sh8)); \
    const uint32_t x0 = LMN_B2_QW(lo & 15u), y0 = LMN_B2_QW((lo >> 4) & 15u); \
    const uint32_t x1 = LMN_B2_QW(hi & 15u), y1 = LMN_B2_QW((hi >> 4) & 15u); \
    LMN_B2_G(a, b, c, d, x0, y0)                                          \
    b = lmn_quad_perm(b, 0x39);                                           \
    c = lmn_quad_perm(c, 0x4E);                                           \
    d = lmn_quad_perm(d, 0x93);                                           \
    LMN_B2_G(a, b, c, d, x1, y1)                                          \
    b = lmn_quad_perm(b, 0x93);                                           \
    c = lmn_quad_perm(c, 0x4E);                                           \
    d = lmn_quad_perm(d, 0x39);                                           \
  }
  LMN_B2_QUAD_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  LMN_B2_QUAD_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
  LMN_B2_QUAD_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
  LMN_B2_QUAD_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
  LMN_B2_QUAD_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
  LMN_B2_QUAD_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
  LMN_B2_QUAD_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
  LMN_B2_QUAD_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
  LMN_B2_QUAD_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
  LMN_B2_QUAD_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
#undef LMN_B2_QUAD_ROUND
  o_lo = h_lo ^ a ^ c;
  o_hi = iv_hi ^ b ^ d;
#undef LMN_B2_QW
}

// The same for ANY block of a hash in progress: lane q of the quad holds words q and 4 + q of the chaining value
// (hl, hh: updated); t0 = bytes hashed so far including this block, f0 = the finalisation word (0xffffffff on the last block).
LMN_D void b2_quad_compress(const uint32_t* msg, uint32_t q, uint32_t& hl, uint32_t& hh, uint32_t t0, uint32_t f0) {
  const uint32_t iv_lo = q == 0 ? 0x6A09E667u : q == 1 ? 0xBB67AE85u : q == 2 ? 0x3C6EF372u : 0xA54FF53Au;
  const uint32_t iv_hi = q == 0 ? 0x510E527Fu : q == 1 ? 0x9B05688Cu : q == 2 ? 0x1F83D9ABu : 0x5BE0CD19u;
  uint32_t a = hl, b = hh, c = iv_lo, d = iv_hi ^ (q == 0 ? t0 : q == 2 ? f0 : 0u);
  const uint32_t sh8 = 8u * q;
#define LMN_B2_QUAD_ROUND(...)                                            \
  {                                                                       \
    const uint64_t S = LMN_B2_SIGMA_PACK(__VA_ARGS__);                    \
    const uint32_t lo = (uint32_t)(S >> sh8), hi = (uint32_t)(S >> (32u + sh8)); \
    const uint32_t x0 = msg[lo & 15u], y0 = msg[(lo >> 4) & 15u];         \
    const uint32_t x1 = msg[hi & 15u], y1 = msg[(hi >> 4) & 15u];         \
    LMN_B2_G(a, b, c, d, x0, y0)                                          \
    b = lmn_quad_perm(b, 0x39);                                           \
    c = lmn_quad_perm(c, 0x4E);                                           \
    d = lmn_quad_perm(d, 0x93);                                           \
    LMN_B2_G(a, b, c, d, x1, y1)                                          \
    b = lmn_quad_perm(b, 0x93);                                           \
    c = lmn_quad_perm(c, 0x4E);                                           \
    d = lmn_quad_perm(d, 0x39);                                           \
  }
  LMN_B2_QUAD_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  LMN_B2_QUAD_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
  LMN_B2_QUAD_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
  LMN_B2_QUAD_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
  LMN_B2_QUAD_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
  LMN_B2_QUAD_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
  LMN_B2_QUAD_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
  LMN_B2_QUAD_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
  LMN_B2_QUAD_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
  LMN_B2_QUAD_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
#undef LMN_B2_QUAD_ROUND
  hl ^= a ^ c;
  hh ^= b ^ d;
}

// One level of an in-LDS Merkle climb.  The block's nodes live WORD-MAJOR in sh (word k of node j at sh[k * BLOCK + j]:
// lanes that walk nodes touch consecutive banks - the node-major form, 8 or 16 words per lane, put a whole wave on two
// banks): the children of this block's `n_par` parents are nodes 0 .. 2 * n_par - 1, parent j replaces node j and is
// written to out[(node0 + j)*8 ..].  Levels with at most 128 parents (two quad-waves per SIMD of the CU) use four lanes
// per hash, which is faster there; wider levels are throughput-bound inside the CU and keep one lane per hash.
// Block-uniform arguments; ends WITHOUT a barrier.
template <int BLOCK>
LMN_D void merkle_lds_level(uint32_t* sh, uint32_t* __restrict__ out, uint32_t node0, uint32_t n_par) {
  __syncthreads();
  if (n_par * 4u <= (uint32_t)BLOCK && n_par <= 128u) {
    const uint32_t g = threadIdx.x >> 2, q = threadIdx.x & 3u;
    const bool on = g < n_par;
    uint32_t o_lo = 0u, o_hi = 0u;
    const bool wave_on = ((threadIdx.x & ~63u) >> 2) < n_par;  // wave-uniform
    if (wave_on) b2_quad_parent<(uint32_t)BLOCK>(sh + 2u * g, q, o_lo, o_hi);
    __syncthreads();
    if (on) {
      sh[q * BLOCK + g] = o_lo;
      sh[(4u + q) * BLOCK + g] = o_hi;
      uint32_t* o = out + (uint64_t)(node0 + g) * 8;
      o[q] = o_lo;
      o[4u + q] = o_hi;
    }
  } else {
    const bool on = threadIdx.x < n_par;
    uint32_t cur[8];
    if (on) {
      uint32_t m[16];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        m[k] = sh[k * BLOCK + 2u * threadIdx.x];
        m[8 + k] = sh[k * BLOCK + 2u * threadIdx.x + 1u];
      }
      b2_compress_fresh(cur, m, 64u);
      store_hash(out + (uint64_t)(node0 + threadIdx.x) * 8, cur);
    }
    __syncthreads();
    if (on) {
#pragma unroll
      for (int k = 0; k < 8; ++k) sh[k * BLOCK + threadIdx.x] = cur[k];
    }
  }
}

// LDS climb shared by the Merkle kernels: `lvl_size` hashes of the whole level exist, this block's share
// sits in sh[idx*8..]; levels first..last are produced.
template <int BLOCK>
LMN_D void merkle_lds_climb(uint32_t* sh, const MerkleLevels& outs, int first, int last, uint32_t lvl_size) {
  for (int l = first; l <= last; ++l) {
    lvl_size >>= 1;
    const uint32_t active = (uint32_t)BLOCK >> (l - first + 1);
    const uint32_t node0 = blockIdx.x * active;
    const uint32_t n_par = node0 >= lvl_size ? 0u : (lvl_size - node0 < active ? lvl_size - node0 : active);
    merkle_lds_level<BLOCK>(sh, outs.p[l], node0, n_par);
  }
}

// MODE 1: leaf level of a single-size tree (no child layer, one contiguous run of <= 16 columns: one
// compression per leaf); MODE 2: pure inner level (children only); MODE 0: anything else.  The special modes
// drop the run selection and the multi-block loop from the hot loop.
// ZT: the caller keeps the message words this mode never loads at zero (set once, outside its leaf loop), so they are not
// rewritten for every leaf
template <int MODE, bool ZT = false>
LMN_D void merkle_load_mode(const uint32_t* __restrict__ prev, const MerkleSegs& sg, int ncols, uint32_t size,
                            uint32_t i, uint32_t m[16], const MerkleFold& fold = MerkleFold{}) {
  if (MODE == 3) {
    // leaf i of a FRI layer = fold of the pair (2i, 2i+1) of the previous layer (same arithmetic as k_fold); the layer's
    // coordinate columns are block-uniform bases, the pair is one 8-byte buffer access per coordinate (kernels_common.h)
    const uint64_t L = 2ull * size;
    QM31 a, b;
    ld_ub_pair(fold.src, i, a.a, b.a);
    ld_ub_pair(fold.src + L, i, a.b, b.b);
    ld_ub_pair(fold.src + 2 * L, i, a.c, b.c);
    ld_ub_pair(fold.src + 3 * L, i, a.d, b.d);
    const QM31 alpha = *fold.alpha;
    QM31 r = q_add(q_add(a, b), q_mul(alpha, q_mul_m(q_sub(a, b), ld_ub(fold.itw, i))));
    if (fold.src2) {   // block-uniform: a quotient column joins this layer (k_fold with accumulate = 1)
      QM31 c, d;
      ld_ub_pair(fold.src2, i, c.a, d.a);
      ld_ub_pair(fold.src2 + L, i, c.b, d.b);
      ld_ub_pair(fold.src2 + 2 * L, i, c.c, d.c);
      ld_ub_pair(fold.src2 + 3 * L, i, c.d, d.d);
      const QM31 rc = q_add(q_add(c, d), q_mul(alpha, q_mul_m(q_sub(c, d), ld_ub(fold.itw2, i))));
      r = q_add(q_mul(r, q_mul(alpha, alpha)), rc);
    }
    st_ub(fold.dst, i, r.a);
    st_ub(fold.dst + (uint64_t)size, i, r.b);
    st_ub(fold.dst + 2ull * size, i, r.c);
    st_ub(fold.dst + 3ull * size, i, r.d);
    m[0] = r.a;
    m[1] = r.b;
    m[2] = r.c;
    m[3] = r.d;
    if (!ZT) {
#pragma unroll
      for (int k = 4; k < 16; ++k) m[k] = 0u;
    }
  } else if (MODE == 1) {
    const uint32_t* __restrict__ base = sg.base[0];   // block-uniform column bases + the leaf as a 32-bit lane offset
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k < ncols)
        m[k] = ld_col(base, k, size, i);
      else if (!ZT)
        m[k] = 0u;
    }
  } else if (MODE == 2) {
    const uint4* p4 = reinterpret_cast<const uint4*>(prev) + (uint64_t)i * 4;
    uint4 a = p4[0], b = p4[1], c = p4[2], d = p4[3];
    m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w;
    m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
    m[8] = c.x; m[9] = c.y; m[10] = c.z; m[11] = c.w;
    m[12] = d.x; m[13] = d.y; m[14] = d.z; m[15] = d.w;
  } else if (MODE == 4) {
    merkle_load_below(fold.below, fold.below_ncols, size, i, m);
  } else {
    merkle_load_first(prev, sg, ncols, size, i, m);
  }
}
// NZ (MODE 1): the leaf has at most NZ columns - message words NZ..15 are zero at compile time (b2_compress_fresh_nz)
template <int MODE, int NZ = 16>
LMN_D void merkle_hash_mode(const uint32_t* __restrict__ prev, const MerkleSegs& sg, int ncols, uint32_t size,
                            uint32_t i, uint32_t m[16], uint32_t h[8], const MerkleFold& fold = MerkleFold{}) {
  if (MODE == 4) {
    merkle_hash_below(sg, ncols, size, fold.below_ncols, i, m, h);
  } else if (MODE == 3) {
    b2_compress_fresh_nz<4>(h, m, 16u);
  } else if (MODE == 1) {
    b2_compress_fresh_nz<NZ>(h, m, 4u * (uint32_t)ncols);
  } else if (MODE == 2) {
    b2_compress_fresh(h, m, 64u);
  } else {
    merkle_hash_from(prev, sg, ncols, size, i, m, h);
  }
}

template <int MODE, int NZ = 16>
LMN_KERNEL k_merkle_fused(const uint32_t* __restrict__ prev, MerkleSegs sg, int ncols, uint32_t size,
                          MerkleLevels outs, int sub, int nfused, MerkleFold fold) {
  // Wave-cooperative subtree: in batch j lane l hashes start node W0 + 64*j + l (coalesced column
  // loads and hash stores).  Siblings sit in neighbouring lanes, so after every second batch the
  // lanes swap one hash with lane^1 and ALL 64 lanes compress one level-1 parent (even lanes for the
  // older batch, odd lanes for the newer one); after every fourth batch the same with lane^2, etc.
  // Each lane keeps its pending hash per level in private LDS slots (word 8 = node index).
  LMN_SHARED uint32_t stack[MERKLE_MAX_SUB * 8 * TPB];  // [level][word][thread]
  uint32_t* sh = stack;  // the climb buffer reuses the stack storage once the batch loop is over
  const uint32_t per = 1u << sub;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t W0 = (t >> 6) * (64u << sub);
  uint32_t cur[8];
  uint32_t cur_idx = 0;
  // software pipeline: the next batch's loads are in flight while this batch is compressed (only ~2 waves share a SIMD
  // here, too few to hide HBM latency by occupancy alone).  Two message buffers alternate (the loop body handles an even and
  // an odd batch), so the prefetched words are hashed where they were loaded - no 16-register copy per leaf.
  uint32_t mA[16], mB[16];
  constexpr bool ZT = MODE == 1 || MODE == 3;   // the words beyond a leaf's columns stay zero for the whole kernel
  if (ZT) {
#pragma unroll
    for (int k = 0; k < 16; ++k) mA[k] = mB[k] = 0u;
  }
  merkle_load_mode<MODE, ZT>(prev, sg, ncols, size, W0 + lane, mA, fold);
  auto leaf = [&](uint32_t j, uint32_t (&mc)[16], uint32_t (&mn)[16]) {
    const uint32_t node = W0 + 64u * j + lane;
    cur_idx = node;
    if (j + 1 < per) merkle_load_mode<MODE, ZT>(prev, sg, ncols, size, node + 64u, mn, fold);
    merkle_hash_mode<MODE, NZ>(prev, sg, ncols, size, node, mc, cur, fold);
    if (outs.p[0]) store_hash(outs.p[0] + (uint64_t)node * 8, cur);
  };
  for (uint32_t j = 0; j < per; j += 2) {
    leaf(j, mA, mB);
    if (per == 1) break;                       // sub = 0: one leaf per lane, nothing to merge in registers
#pragma unroll
    for (int k = 0; k < 8; ++k) stack[k * TPB + threadIdx.x] = cur[k];   // level-0 slot: the even batch waits for its sibling
    leaf(j + 1, mB, mA);
    uint32_t jj = j + 1;
    int lvl = 0;
    while (jj & 1u) {
      const bool b = ((lane >> lvl) & 1u) != 0u;
      uint32_t m[16];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t st = stack[(lvl * 8 + k) * TPB + threadIdx.x];
        const uint32_t recv = lmn_shfl_xor(b ? st : cur[k], 1 << lvl);
        m[k] = b ? recv : st;
        m[8 + k] = b ? cur[k] : recv;
      }
      // the pending (older) node of this lane sits exactly 64 nodes before the newer one at every level
      cur_idx = (b ? cur_idx : cur_idx - 64u) >> 1;
      b2_compress_fresh(cur, m, 64u);
      jj >>= 1;
      ++lvl;
      if (outs.p[lvl]) store_hash(outs.p[lvl] + (uint64_t)cur_idx * 8, cur);
    }
    if (lvl < sub) {
#pragma unroll
      for (int k = 0; k < 8; ++k) stack[(lvl * 8 + k) * TPB + threadIdx.x] = cur[k];
    }
  }
  __syncthreads();  // every lane is done with its stack slots before they are overwritten
  {
    const uint32_t local = cur_idx - blockIdx.x * TPB;  // this block owns level-`sub` nodes [b*TPB, (b+1)*TPB)
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[k * TPB + local] = cur[k];   // word-major (merkle_lds_level)
  }
  merkle_lds_climb<TPB>(sh, outs, sub + 1, nfused, size >> sub);
}

LMN_D void chan_draw_words(DevChannel* ch, uint32_t out[8]) {
  uint32_t m[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) m[k] = ch->digest[k];
  m[8] = ch->n_sent;
#pragma unroll
  for (int k = 9; k < 16; ++k) m[k] = 0u;
  b2_init(out);
  // KAT encoding: digest || u64 counter zero-padded to 32 bytes (64-byte message);
  // LMN_PV_DRAW_CTR_U32: digest || u32 counter || 0x00 (37-byte message)
  b2_compress(out, m, ch->variant == 0u ? 64u : 37u, 0xffffffffu);
  ch->n_sent += 1u;
}

// digest <- H(digest || root); alpha <- draw_felt(); executed by ONE lane
LMN_D void chan_mix_root_draw(DevChannel* ch, const uint32_t* root, QM31* out_alpha, uint32_t* root_copy) {
  uint32_t m[16], h[8];
  for (int k = 0; k < 8; ++k) {
    m[k] = ch->digest[k];
    m[8 + k] = root[k];
    root_copy[k] = root[k];
  }
  b2_compress_fresh(h, m, 64u);
  for (int k = 0; k < 8; ++k) ch->digest[k] = h[k];
  ch->n_sent = 0u;
  for (;;) {
    uint32_t w[8];
    chan_draw_words(ch, w);
    bool ok = true;
    for (int k = 0; k < 8; ++k) ok = ok && (w[k] < 2u * P31);
    if (!ok) continue;
    QM31 a;
    a.a = w[0] >= P31 ? w[0] - P31 : w[0];
    a.b = w[1] >= P31 ? w[1] - P31 : w[1];
    a.c = w[2] >= P31 ? w[2] - P31 : w[2];
    a.d = w[3] >= P31 ? w[3] - P31 : w[3];
    *out_alpha = a;
    break;
  }
}

// Block-cooperative form of chan_mix_root_draw for kernels that already hold the root in LDS: called by ALL
// threads of the block (block-uniform control flow); the hashing runs on the first quad with the
// quad-cooperative Blake2s (0.9 us per hash instead of 2 us).  `scratch`: 28 words of LDS that do not
// overlap the root's 8 words.  Ends with a barrier and returns the drawn alpha to every thread.
// `dg` (lanes 0..7: word `lane` of the channel's digest) and `variant` are loaded by the caller - at its start, so that
// the round trip to memory is hidden behind its hashing; `dg` is updated (a kernel that makes several steps never
// reads the channel back), and the channel in memory as well (for the next launch).
LMN_D QM31 chan_mix_root_draw_block(DevChannel* ch, uint32_t& dg, uint32_t variant, const uint32_t* root,
                                    uint32_t root_stride, uint32_t* scratch, QM31* out_alpha, uint32_t* root_copy) {
  uint32_t* msg = scratch;       // 16 words: digest || root, then digest || counter
  uint32_t* wbuf = scratch + 16;  // 8 words: drawn words
  const uint32_t tid = threadIdx.x, q = tid & 3u;
  const uint32_t t_draw = variant == 0u ? 64u : 37u;
  __syncthreads();
  if (tid < 8u) {
    msg[tid] = dg;
    const uint32_t r = root[tid * root_stride];   // word k of the root at root[k * root_stride] (word-major node array)
    msg[8u + tid] = r;
    root_copy[tid] = r;
  }
  __syncthreads();
  uint32_t lo = 0u, hi = 0u;
  if (tid < 64u) b2_quad_parent(msg, q, lo, hi);
  __syncthreads();
  if (tid < 4u) {
    msg[q] = lo;
    msg[4u + q] = hi;
    ch->digest[q] = lo;
    ch->digest[4u + q] = hi;
  }
  for (uint32_t n_sent = 0;; ++n_sent) {
    if (tid >= 8u && tid < 16u) msg[tid] = tid == 8u ? n_sent : 0u;
    __syncthreads();
    if (tid < 64u) b2_quad_parent(msg, q, lo, hi, t_draw);
    if (tid < 4u) {
      wbuf[q] = lo;
      wbuf[4u + q] = hi;
    }
    __syncthreads();
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) ok = ok && (wbuf[k] < 2u * P31);
    if (ok) {  // block-uniform
      if (tid == 0u) {
        QM31 a;
        a.a = wbuf[0] >= P31 ? wbuf[0] - P31 : wbuf[0];
        a.b = wbuf[1] >= P31 ? wbuf[1] - P31 : wbuf[1];
        a.c = wbuf[2] >= P31 ? wbuf[2] - P31 : wbuf[2];
        a.d = wbuf[3] >= P31 ? wbuf[3] - P31 : wbuf[3];
        *out_alpha = a;
        ch->n_sent = n_sent + 1u;
        scratch[24] = a.a;
        scratch[25] = a.b;
        scratch[26] = a.c;
        scratch[27] = a.d;
      }
      break;
    }
    __syncthreads();  // everyone has read wbuf before the next draw overwrites it
  }
  if (tid < 8u) dg = msg[tid];   // the digest after the mix (the draws leave it alone)
  __syncthreads();
  return QM31{scratch[24], scratch[25], scratch[26], scratch[27]};
}

constexpr int CHAN_STEP_SCRATCH = 32 + 4 * CHAN_MAX_INST;   // LDS words a ChanStep works in (layout: chan_step_* below)
constexpr int CHAN_STEP_WORDS = (int)(sizeof(ChanStep) / 4);
static_assert(sizeof(ChanStep) % 8 == 0 && CHAN_STEP_WORDS <= 1024, "a ChanStep is fetched by one word per lane of a block");
LMN_D void chan_step_run(uint32_t* scr, DevChannel* ch, uint32_t dg, uint32_t variant, uint32_t root_word, const ChanStep& st);

// Small trees / tree tops: one node per lane, one block of up to 1024 lanes, up to 10 LDS levels.
// The launch that produces the root also makes the transcript step that consumes it when `ch` is given: mix_root and
// the draw of a folding alpha (step.kind 0, the FRI layers), or one of the commitment phases' steps (ChanStep, kernels.h).
constexpr int MERKLE_SMALL_BLOCK = 1024;
template <int MODE>
LMN_KERNEL k_merkle_small(const uint32_t* __restrict__ prev, MerkleSegs sg, int ncols, uint32_t size,
                          MerkleLevels outs, int nfused, DevChannel* ch, QM31* alpha_out, uint32_t* root_copy,
                          const ChanStep* __restrict__ step, int step_kind) {
  LMN_SHARED uint32_t sh[MERKLE_SMALL_BLOCK * 8];
  LMN_SHARED alignas(16) uint32_t sh_step[CHAN_STEP_WORDS];
  const uint32_t i = threadIdx.x;
  // when this launch produces the root, it also runs the device-resident Fiat-Shamir step: fetch the channel now
  const bool fs = ch != nullptr && (size >> nfused) == 1u;
  uint32_t dg = 0u, variant = 0u;
  if (fs && step_kind != 1) {   // (kind 1 starts the channel from step.start)
    if (i < 8u) dg = ch->digest[i];
    variant = ch->variant;
  }
  uint32_t cur[8];
  uint32_t m[16];
  if (i < size) merkle_load_mode<MODE>(prev, sg, ncols, size, i, m);
  // the step's plan lies in page-locked host memory: fetched behind the node loads (one round trip over the link, over
  // by the time the first compression is), kept in LDS
  uint32_t step_word = 0u;
  const bool step_lane = fs && step_kind != 0 && i < (uint32_t)CHAN_STEP_WORDS;
  if (step_lane) step_word = reinterpret_cast<const uint32_t*>(step)[i];
  if (i < size) {
    merkle_hash_mode<MODE>(prev, sg, ncols, size, i, m, cur);
    store_hash(outs.p[0] + (uint64_t)i * 8, cur);
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[k * MERKLE_SMALL_BLOCK + i] = cur[k];   // word-major (merkle_lds_level)
  }
  if (step_lane) sh_step[i] = step_word;
  merkle_lds_climb<MERKLE_SMALL_BLOCK>(sh, outs, 1, nfused, size);
  if (fs && step_kind == 0) chan_mix_root_draw_block(ch, dg, variant, sh, MERKLE_SMALL_BLOCK, sh + 16, alpha_out, root_copy);
  if (fs && step_kind != 0) {
    __syncthreads();   // the root's words (the climb ends without a barrier) and the plan
    const uint32_t root_word = i < 8u ? sh[i * MERKLE_SMALL_BLOCK] : 0u;
    // sh[16 .. 16 + CHAN_STEP_SCRATCH): word 0 of dead nodes
    chan_step_run(sh + 16, ch, dg, variant, root_word, *reinterpret_cast<const ChanStep*>(sh_step));
  }
}

void launch_merkle_fused(const uint32_t* prev, const MerkleSegs& sg, int ncols, uint32_t size,
                         const MerkleLevels& outs, int sub, int nfused, lmn_stream_t s, const MerkleFold* fold) {
  if (!prev && ncols == 0) throw LmnError(-100, "merkle level with no input");
  if (nfused > MERKLE_MAX_FUSED || sub > MERKLE_MAX_SUB || sub > nfused || nfused - sub > 8 ||
      size % ((uint32_t)TPB << sub) != 0)
    throw LmnError(-100, "merkle_fused: bad arguments");
  const dim3 g(cdiv(size >> sub, TPB)), b(TPB);
  const MerkleFold none{};
  // a null p[l] (l < sub only: the levels a lane keeps in registers) is a level the caller does not want written
  for (int l = sub; l <= nfused; ++l)
    if (!outs.p[l]) throw LmnError(-100, "merkle_fused: only the per-lane levels may be left unwritten");
  if (fold && fold->below) {
    if (prev || fold->src || ncols < 1 || fold->below_ncols < 1 || fold->below_ncols > 8)
      throw LmnError(-100, "merkle_fused: a start level over its own leaf level has columns, no stored children and <= 8 leaf columns");
    LMN_LAUNCH(k_merkle_fused<4>, g, b, 0, s, prev, sg, ncols, size, outs, sub, nfused, *fold);
  } else if (fold) {
    if (prev || ncols != 4) throw LmnError(-100, "merkle_fused: a folded level is a leaf level of 4 coordinate columns");
    LMN_LAUNCH(k_merkle_fused<3>, g, b, 0, s, prev, sg, ncols, size, outs, sub, nfused, *fold);
  } else if (!prev && ncols <= 16 && sg.n[0] == ncols) {
    // the leaf's zero message words are compile-time zeros of the instantiation (blake2s.h b2_compress_fresh_nz)
    if (ncols <= 4)
      LMN_LAUNCH((k_merkle_fused<1, 4>), g, b, 0, s, prev, sg, ncols, size, outs, sub, nfused, none);
    else if (ncols <= 8)
      LMN_LAUNCH((k_merkle_fused<1, 8>), g, b, 0, s, prev, sg, ncols, size, outs, sub, nfused, none);
    else if (ncols <= 12)
      LMN_LAUNCH((k_merkle_fused<1, 12>), g, b, 0, s, prev, sg, ncols, size, outs, sub, nfused, none);
    else if (ncols <= 15)
      LMN_LAUNCH((k_merkle_fused<1, 15>), g, b, 0, s, prev, sg, ncols, size, outs, sub, nfused, none);
    else
      LMN_LAUNCH((k_merkle_fused<1, 16>), g, b, 0, s, prev, sg, ncols, size, outs, sub, nfused, none);
  } else if (prev && ncols == 0)
    LMN_LAUNCH(k_merkle_fused<2>, g, b, 0, s, prev, sg, ncols, size, outs, sub, nfused, none);
  else
    LMN_LAUNCH(k_merkle_fused<0>, g, b, 0, s, prev, sg, ncols, size, outs, sub, nfused, none);
}

void launch_merkle_small(const uint32_t* prev, const MerkleSegs& sg, int ncols, uint32_t size,
                         const MerkleLevels& outs, int nfused, DevChannel* ch, QM31* alpha_out, uint32_t* root_copy,
                         lmn_stream_t s, const ChanStep* step, int step_kind) {
  if (!prev && ncols == 0) throw LmnError(-100, "merkle level with no input");
  if (size > (uint32_t)MERKLE_SMALL_BLOCK || nfused > 10) throw LmnError(-100, "merkle_small: bad arguments");
  static_assert(16 + CHAN_STEP_SCRATCH <= MERKLE_SMALL_BLOCK, "the step's scratch lies inside word 0 of the node array");
  const dim3 g(1), b(MERKLE_SMALL_BLOCK);
  if (!step) step_kind = 0;
  if (step_kind < 0 || step_kind > 3) throw LmnError(-100, "merkle_small: bad transcript step");
  if (step_kind != 0 && (!ch || (size >> nfused) != 1u)) throw LmnError(-100, "merkle_small: a transcript step needs the root and a channel");
  if (!prev && ncols <= 16 && sg.n[0] == ncols)
    LMN_LAUNCH(k_merkle_small<1>, g, b, 0, s, prev, sg, ncols, size, outs, nfused, ch, alpha_out, root_copy, step, step_kind);
  else if (prev && ncols == 0)
    LMN_LAUNCH(k_merkle_small<2>, g, b, 0, s, prev, sg, ncols, size, outs, nfused, ch, alpha_out, root_copy, step, step_kind);
  else
    LMN_LAUNCH(k_merkle_small<0>, g, b, 0, s, prev, sg, ncols, size, outs, nfused, ch, alpha_out, root_copy, step, step_kind);
}

// =============================================================================================
// Device-resident Fiat-Shamir steps for the FRI commit loop (no host round trip per layer)
// =============================================================================================
LMN_KERNEL k_chan_mix_root_draw(DevChannel* ch, const uint32_t* __restrict__ root, QM31* out_alpha,
                                uint32_t* root_copy) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  chan_mix_root_draw(ch, root, out_alpha, root_copy);
}

void launch_chan_mix_root_draw(DevChannel* ch, const uint32_t* root, QM31* out_alpha, uint32_t* root_copy,
                               lmn_stream_t s) {
  LMN_LAUNCH(k_chan_mix_root_draw, dim3(1), dim3(64), 0, s, ch, root, out_alpha, root_copy);
}

// =============================================================================================
// Device-resident Fiat-Shamir of the commitment phases (kernels.h): the transcript steps between the big kernels of a
// proof - two to eight dependent compressions each - instead of a host round trip (30 - 45 us of idle GPU each).
// Block-cooperative: every thread of the block calls these with block-uniform arguments; the compressions run on the
// first quad (b2_quad_parent: 0.9 us per hash against 2 us on one lane).  They are the last thing the launch that
// produces the tree's root does (k_merkle_small), or a launch of their own where no such launch exists (k_chan_step).
// Scratch (LDS, CHAN_STEP_SCRATCH words): msg 16 | drawn words 8 | point 8 | claimed sums 4 x CHAN_MAX_INST.
// =============================================================================================
// digest (msg[0..8)) <- H(digest || msg[8..8+n)); the caller has written msg[8..16) (zero-padded).  No barrier at the end.
LMN_D void qchan_mix(uint32_t* msg, uint32_t n_words) {
  const uint32_t tid = threadIdx.x, q = tid & 3u;
  __syncthreads();
  uint32_t lo = 0u, hi = 0u;
  if (tid < 64u) b2_quad_parent(msg, q, lo, hi, 32u + 4u * n_words);
  __syncthreads();
  if (tid < 4u) {
    msg[q] = lo;
    msg[4u + q] = hi;
  }
}
// Channel::draw_base_felts: 8 M31 from one hash of digest || counter, redrawn while a word is >= 2P; every thread gets them
LMN_D void qchan_draw_felts8(uint32_t* msg, uint32_t* wbuf, uint32_t& n_sent, uint32_t t_draw, uint32_t f[8]) {
  const uint32_t tid = threadIdx.x, q = tid & 3u;
  for (;;) {
    if (tid >= 8u && tid < 16u) msg[tid] = tid == 8u ? n_sent : 0u;
    __syncthreads();
    uint32_t lo = 0u, hi = 0u;
    if (tid < 64u) b2_quad_parent(msg, q, lo, hi, t_draw);
    if (tid < 4u) {
      wbuf[q] = lo;
      wbuf[4u + q] = hi;
    }
    n_sent += 1u;
    __syncthreads();
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      f[k] = wbuf[k];
      ok = ok && (f[k] < 2u * P31);
    }
    __syncthreads();  // everyone has read wbuf before the next draw overwrites it
    if (ok) break;    // block-uniform
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = f[k] >= P31 ? f[k] - P31 : f[k];
}
LMN_D void qchan_store(DevChannel* ch, const uint32_t* msg, uint32_t n_sent, uint32_t variant) {
  if (threadIdx.x < 8u) ch->digest[threadIdx.x] = msg[threadIdx.x];
  if (threadIdx.x == 0u) {
    ch->n_sent = n_sent;
    ch->variant = variant;
  }
}

// kind 1: the channel starts at step.start; mix_root(root 1); one draw_felts(2) per relation element set
LMN_D void chan_step_root_elems(uint32_t* scr, DevChannel* ch, uint32_t root_word, const ChanStep& st) {
  uint32_t *msg = scr, *wbuf = scr + 16;
  const uint32_t tid = threadIdx.x;
  DevReport* rep = st.rep;
  __syncthreads();
  if (tid < 8u) {
    msg[tid] = st.start.digest[tid];
    msg[8u + tid] = root_word;
    rep->roots[0][tid] = root_word;
  }
  if (tid == 0u) rep->bad = *st.bad_word;
  // trace reuse: the comparing transposes' marks travel with the verdict (they lie behind its two words)
  for (uint32_t k = tid; k < st.changed_words; k += blockDim.x) rep->changed[k] = st.bad_word[2u + k];
  qchan_mix(msg, 8u);
  uint32_t n_sent = 0u;
  const uint32_t t_draw = st.start.variant == 0u ? 64u : 37u;
  for (int i = 0; i < st.sets.n; ++i) {
    uint32_t f[8];
    qchan_draw_felts8(msg, wbuf, n_sent, t_draw, f);
    const int e = st.sets.set[i];
    if (tid == 0u && e >= 0) {
      rep->elems.z[e] = QM31{f[0], f[1], f[2], f[3]};
      rep->elems.alpha[e] = QM31{f[4], f[5], f[6], f[7]};
    }
  }
  __syncthreads();
  qchan_store(ch, msg, n_sent, st.start.variant);
}

// kind 2: mix_felts([claimed_i]) per component, mix_root(root 2), draw_felt() = the composition randomness; then the
// signed coefficient of every kernel constraint slot.  dg: lanes 0..7 hold the channel's digest (loaded by the caller)
LMN_D void chan_step_claims_root_alpha(uint32_t* scr, DevChannel* ch, uint32_t dg, uint32_t variant, uint32_t root_word,
                                       const ChanStep& st) {
  uint32_t *msg = scr, *wbuf = scr + 16, *cl = scr + 32;
  const uint32_t tid = threadIdx.x;
  const ChanCoeffPlan& plan = st.coeff;
  DevReport* rep = st.rep;
  __syncthreads();
  if (tid < (uint32_t)plan.n_inst * 4u) {   // every claimed sum in one round trip to memory
    const uint32_t w = reinterpret_cast<const uint32_t*>(plan.claimed[tid >> 2])[tid & 3u];
    cl[tid] = w;
    reinterpret_cast<uint32_t*>(&rep->claimed[tid >> 2])[tid & 3u] = w;
  }
  if (tid < 8u) msg[tid] = dg;
  for (int i = 0; i < plan.n_inst; ++i) {
    __syncthreads();
    if (tid >= 8u && tid < 16u) msg[tid] = tid < 12u ? cl[4 * i + (int)tid - 8] : 0u;
    qchan_mix(msg, 4u);
  }
  if (tid < 8u) {
    msg[8u + tid] = root_word;
    rep->roots[1][tid] = root_word;
  }
  qchan_mix(msg, 8u);
  uint32_t n_sent = 0u, f[8];
  qchan_draw_felts8(msg, wbuf, n_sent, variant == 0u ? 64u : 37u, f);
  const QM31 alpha{f[0], f[1], f[2], f[3]};
  if (tid == 0u) rep->comp_alpha = alpha;
  qchan_store(ch, msg, n_sent, variant);
  // one lane per (component, kernel slot): alpha^e by square-and-multiply
  for (int idx = (int)tid; idx < plan.n_inst * 16; idx += (int)blockDim.x) {
    const int i = idx >> 4, k = idx & 15;
    QM31 c = q_zero();
    if (k < plan.n_kernel[i] && plan.proto_index[i][k] >= 0) {
      uint32_t e = (uint32_t)(plan.n_total - 1 - ((int)plan.k0[i] + (int)plan.proto_index[i][k]));
      QM31 b = alpha;
      c = q_one();
      while (e) {
        if (e & 1u) c = q_mul(c, b);
        b = q_mul(b, b);
        e >>= 1;
      }
      if ((plan.neg[i] >> k) & 1u) c = q_neg(c);
    }
    st.coeff_out[idx] = c;
  }
}

// kind 3: mix_root(root 3), t = draw_felt(), the OODS point, the sample points and their mappings; the finished report
// goes to the host's page-locked copy
LMN_D void chan_step_root_oods(uint32_t* scr, DevChannel* ch, uint32_t dg, uint32_t variant, uint32_t root_word,
                               const ChanStep& st) {
  uint32_t *msg = scr, *wbuf = scr + 16, *sh_pt = scr + 24;
  const uint32_t tid = threadIdx.x;
  const ChanOodsPlan& plan = st.oods;
  DevReport* rep = st.rep;
  // the job table's words are fetched now (one round trip over the link, behind the hashing below) and stored at the end
  const uint32_t copy_words = st.copy_words;
  const uint32_t* copy_src = st.copy_src;
  uint32_t* copy_dst = st.copy_dst;
  const uint32_t copy_word = tid < copy_words ? copy_src[tid] : 0u;
  __syncthreads();
  if (tid < 8u) {
    msg[tid] = dg;
    msg[8u + tid] = root_word;
    rep->roots[2][tid] = root_word;
  }
  qchan_mix(msg, 8u);
  uint32_t n_sent = 0u, f[8];
  qchan_draw_felts8(msg, wbuf, n_sent, variant == 0u ? 64u : 37u, f);
  qchan_store(ch, msg, n_sent, variant);
  if (tid == 0u) {
    const QM31 tt{f[0], f[1], f[2], f[3]};
    rep->t = tt;
    const QM31 t2 = q_sqr(tt);
    const QM31 tinv = q_inv(q_add_m(t2, 1u));
    const QM31 x = q_mul(q_sub(q_one(), t2), tinv), y = q_mul(q_add(tt, tt), tinv);
    sh_pt[0] = x.a; sh_pt[1] = x.b; sh_pt[2] = x.c; sh_pt[3] = x.d;
    sh_pt[4] = y.a; sh_pt[5] = y.b; sh_pt[6] = y.c; sh_pt[7] = y.d;
  }
  __syncthreads();
  const QM31 ox{sh_pt[0], sh_pt[1], sh_pt[2], sh_pt[3]}, oy{sh_pt[4], sh_pt[5], sh_pt[6], sh_pt[7]};
  for (int p = (int)tid; p < plan.n_points; p += (int)blockDim.x) {
    QM31 px = ox, py = oy;
    if (p > 0) {   // secure point + base point (host.h qpt_add_m)
      const uint32_t bx = plan.step_x[p], by = plan.step_y[p];
      px = q_sub(q_mul_m(ox, bx), q_mul_m(oy, by));
      py = q_add(q_mul_m(ox, by), q_mul_m(oy, bx));
    }
    QM31* mp = st.maps_out + (size_t)p * plan.n_maps;
    mp[0] = py;
    mp[1] = px;
    QM31 cur = px;
    for (int k = 2; k < plan.n_maps; ++k) {
      cur = q_sub_m(q_add(q_sqr(cur), q_sqr(cur)), 1u);
      mp[k] = cur;
    }
  }
  // the report is complete: the last of the device-resident steps writes the host's copy itself (page-locked memory;
  // this launch's own words of it are visible to the block since the barrier above)
  const uint32_t* rw = reinterpret_cast<const uint32_t*>(rep);
  for (uint32_t k = tid; k < (uint32_t)(sizeof(DevReport) / 4); k += blockDim.x) st.rep_host[k] = rw[k];
  if (tid < copy_words) copy_dst[tid] = copy_word;
  for (uint32_t k = tid + blockDim.x; k < copy_words; k += blockDim.x) copy_dst[k] = copy_src[k];
}

// Blake2s over the `total_words` words at W (LDS, zero-padded to whole 64-byte blocks) -> msg[0..8): the hash of a
// message longer than one block (Channel::mix_felts: W = digest || values), on the first quad.  Called by all threads
// behind a barrier that made W visible; no barrier at the end.
LMN_D void qchan_hash_blocks(const uint32_t* W, uint32_t total_words, uint32_t* msg) {
  const uint32_t tid = threadIdx.x;
  const uint32_t n_blocks = (total_words + 15u) / 16u;
#ifdef LMN_EMU
  if (tid == 0u) {
    uint32_t h[8];
    b2_init(h);
    for (uint32_t b = 0; b < n_blocks; ++b) {
      const bool last = b + 1u == n_blocks;
      b2_compress(h, W + 16u * b, last ? 4u * total_words : 64u * (b + 1u), last ? 0xffffffffu : 0u);
    }
    for (int k = 0; k < 8; ++k) msg[k] = h[k];
  }
#else
  if (tid < 64u) {
    const uint32_t q = tid & 3u;
    uint32_t hl = q == 0 ? (0x6A09E667u ^ 0x01010020u) : q == 1 ? 0xBB67AE85u : q == 2 ? 0x3C6EF372u : 0xA54FF53Au;
    uint32_t hh = q == 0 ? 0x510E527Fu : q == 1 ? 0x9B05688Cu : q == 2 ? 0x1F83D9ABu : 0x5BE0CD19u;
    for (uint32_t b = 0; b < n_blocks; ++b) {
      const bool last = b + 1u == n_blocks;
      b2_quad_compress(W + 16u * b, q, hl, hh, last ? 4u * total_words : 64u * (b + 1u), last ? 0xffffffffu : 0u);
    }
    if (tid < 4u) {
      msg[q] = hl;
      msg[4u + q] = hh;
    }
  }
#endif
}

// =============================================================================================
// The step in front of the FRI quotient kernels (kernels.h QuotPrepPlan): mix_felts(sampled values), alpha = draw_felt(),
// the quotient tables of every LDE size.  One workgroup; block-uniform control flow.
// =============================================================================================
constexpr int QUOT_PREP_PLAN_WORDS = (int)(sizeof(QuotPrepPlan) / 4);
static_assert(sizeof(QuotPrepPlan) % 8 == 0, "the plan is fetched word by word");
LMN_KERNEL k_quot_prepare(DevChannel* ch, const QuotPrepPlan* __restrict__ plan_g) {
  LMN_SHARED alignas(16) uint32_t sh_plan[QUOT_PREP_PLAN_WORDS];
  LMN_SHARED uint32_t W[8 + 4 * QUOT_PREP_MAX_SAMPLES + 16];   // digest || values, zero-padded to whole blocks
  LMN_SHARED uint32_t scr[32];                                   // msg 16 | drawn words 8 | alpha 4
  LMN_SHARED QM31 sa[QUOT_MAX_ENTRIES], sb[QUOT_MAX_ENTRIES];
  const uint32_t tid = threadIdx.x;
  for (uint32_t k = tid; k < (uint32_t)QUOT_PREP_PLAN_WORDS; k += blockDim.x) sh_plan[k] = reinterpret_cast<const uint32_t*>(plan_g)[k];
  const uint32_t dgw = tid < 8u ? ch->digest[tid] : 0u;
  const uint32_t variant = ch->variant;
  __syncthreads();
  const QuotPrepPlan& plan = *reinterpret_cast<const QuotPrepPlan*>(sh_plan);
  const uint32_t n_val_words = 4u * (uint32_t)plan.n_samples, total_words = 8u + n_val_words;
  const uint32_t n_blocks = (total_words + 15u) / 16u;
  if (tid < 8u) W[tid] = dgw;
  for (uint32_t k = tid; k < n_blocks * 16u - 8u; k += blockDim.x) {
    uint32_t w = 0u;
    if (k < n_val_words) {
      w = reinterpret_cast<const uint32_t*>(plan.vals)[k];
      reinterpret_cast<uint32_t*>(plan.vals_host)[k] = w;   // the host's copy of the sampled values (page-locked memory)
    }
    W[8u + k] = w;
  }
  __syncthreads();
  // ---- Channel::mix_felts: digest <- Blake2s(digest || values)
  uint32_t* msg = scr;
  qchan_hash_blocks(W, total_words, msg);
  __syncthreads();
  // ---- alpha = draw_felt(); the channel goes on into the FRI commit loop
  uint32_t n_sent = 0u, f[8];
  qchan_draw_felts8(msg, scr + 16, n_sent, variant == 0u ? 64u : 37u, f);
  const QM31 alpha{f[0], f[1], f[2], f[3]};
  qchan_store(ch, msg, n_sent, variant);
  if (tid == 0u) plan.vals_host[plan.n_samples] = alpha;
  // ---- one lane per (column, sample): alpha^(k+1) times the line through (p.y, v) and (conj p.y, conj v)
  for (uint32_t e = tid; e < (uint32_t)plan.n_entries; e += blockDim.x) {
    const QuotPrepEntry en = plan.entries[e];
    const QuotPrepSize& sz = plan.size[en.size];
    const uint32_t local = e - sz.first_entry;
    const uint32_t k = local - (uint32_t)sz.batch_start[en.batch];
    const QM31 power = q_pow(alpha, (uint64_t)k + 1u);
    const uint32_t* vw = W + 8u + 4u * en.sample;
    const QM31 val{vw[0], vw[1], vw[2], vw[3]};
    const QM31 py = plan.maps[(size_t)sz.point[en.batch] * (size_t)plan.n_maps];
    const QM31 la = q_sub(q_conj(val), val);
    const QM31 lc = q_sub(q_conj(py), py);
    const QM31 lbb = q_sub(q_mul(val, lc), q_mul(la, py));
    sz.entries_out[local] = QuotEntry{en.col, q_mul(power, lc)};
    sa[e] = q_mul(power, la);
    sb[e] = q_mul(power, lbb);
  }
  __syncthreads();
  // ---- one lane per (size, batch): the batch's sums, its power of alpha, its point
  if (tid < (uint32_t)plan.n_sizes * (uint32_t)QUOT_MAX_BATCH) {
    const QuotPrepSize& sz = plan.size[tid / QUOT_MAX_BATCH];
    const int b = (int)(tid % QUOT_MAX_BATCH);
    if (b < sz.n_batch) {
      QM31 A = q_zero(), B = q_zero();
      for (int i = sz.batch_start[b]; i < sz.batch_start[b + 1]; ++i) {
        A = q_add(A, sa[sz.first_entry + (uint32_t)i]);
        B = q_add(B, sb[sz.first_entry + (uint32_t)i]);
      }
      const QM31* mp = plan.maps + (size_t)sz.point[b] * (size_t)plan.n_maps;
      const QM31 py = mp[0], px = mp[1];
      QuotDev* d = sz.dev_out;
      d->A[b] = A;
      d->B[b] = B;
      d->batch_coeff[b] = q_pow(alpha, (uint64_t)(sz.batch_start[b + 1] - sz.batch_start[b]));
      d->prx[b] = CM31{px.a, px.b};
      d->pix[b] = CM31{px.c, px.d};
      d->pry[b] = CM31{py.a, py.b};
      d->piy[b] = CM31{py.c, py.d};
    }
  }
  for (uint32_t k = tid; k < plan.copy_words; k += blockDim.x) plan.copy_dst[k] = plan.copy_src[k];
}
void launch_quot_prepare(DevChannel* ch, const QuotPrepPlan* plan, lmn_stream_t s) {
  if (!ch || !plan) throw LmnError(-100, "quot_prepare: no channel / plan");
  LMN_LAUNCH(k_quot_prepare, dim3(1), dim3(TPB), 0, s, ch, plan);
}

// root_word: lanes 0..7 hold the root's words; dg / variant: the channel as the caller fetched it at its start (kind 1
// starts from step.start instead)
LMN_D void chan_step_run(uint32_t* scr, DevChannel* ch, uint32_t dg, uint32_t variant, uint32_t root_word, const ChanStep& st) {
  if (st.kind == 1)
    chan_step_root_elems(scr, ch, root_word, st);
  else if (st.kind == 2)
    chan_step_claims_root_alpha(scr, ch, dg, variant, root_word, st);
  else if (st.kind == 3)
    chan_step_root_oods(scr, ch, dg, variant, root_word, st);
}

// a step as a launch of its own (trees whose root is not produced by k_merkle_small)
LMN_KERNEL k_chan_step(DevChannel* ch, const ChanStep* __restrict__ step, int step_kind, const uint32_t* __restrict__ root) {
  LMN_SHARED uint32_t scr[CHAN_STEP_SCRATCH];
  LMN_SHARED alignas(16) uint32_t sh_step[CHAN_STEP_WORDS];
  for (uint32_t k = threadIdx.x; k < (uint32_t)CHAN_STEP_WORDS; k += blockDim.x) sh_step[k] = reinterpret_cast<const uint32_t*>(step)[k];
  uint32_t dg = 0u, variant = 0u, root_word = 0u;
  if (threadIdx.x < 8u) root_word = root[threadIdx.x];
  if (step_kind != 1) {
    if (threadIdx.x < 8u) dg = ch->digest[threadIdx.x];
    variant = ch->variant;
  }
  __syncthreads();
  chan_step_run(scr, ch, dg, variant, root_word, *reinterpret_cast<const ChanStep*>(sh_step));
}
void check_chan_step(const ChanStep& st) {
  if (st.kind < 1 || st.kind > 3) throw LmnError(-100, "chan_step: bad kind");
  if (st.kind == 1 && (st.sets.n < 1 || st.sets.n > CHAN_N_ELEMS)) throw LmnError(-100, "chan_step: bad draw count");
  if (st.changed_words > (uint32_t)CHANGED_WORDS) throw LmnError(-100, "chan_step: more changed words than the report holds");
  if (st.kind == 2 && (st.coeff.n_inst < 1 || st.coeff.n_inst > CHAN_MAX_INST)) throw LmnError(-100, "chan_step: bad component count");
  if (st.kind == 3 && (st.oods.n_points < 1 || st.oods.n_points > CHAN_MAX_POINTS || st.oods.n_maps < 2))
    throw LmnError(-100, "chan_step: bad sample plan");
}
// `step`: device-visible (page-locked host memory is: read once)
void launch_chan_step(DevChannel* ch, const ChanStep* step, int step_kind, const uint32_t* root, lmn_stream_t s) {
  if (!step || step_kind < 1 || step_kind > 3) throw LmnError(-100, "chan_step: bad kind");
  LMN_LAUNCH(k_chan_step, dim3(1), dim3(TPB), 0, s, ch, step, step_kind, root);
}

// =============================================================================================
// FRI tail: all layers of size <= 1024 in ONE single-block launch: per layer Merkle-commit the
// line evaluation (LDS tree), mix the root into the device-resident channel, draw the folding
// alpha, fold.  Every layer's evaluations and tree levels still go to HBM for decommitment.
// =============================================================================================
LMN_KERNEL k_fri_tail(DevChannel* ch, const FriTailLayer* __restrict__ layers, int n_layers, int first_log,
                      QM31* alphas_out, uint32_t* roots_out, FriTailIo pre) {
  LMN_SHARED uint32_t sh[MERKLE_SMALL_BLOCK * 8];
  LMN_SHARED uint32_t shv[MERKLE_SMALL_BLOCK * 4];   // the layer's values, coordinate-major: the fold reads its pair here
  const uint32_t i = threadIdx.x;
  // the channel is read once and the layers' values once: a lane keeps value i of the current layer (its fold output is
  // the next layer's value i), so that no step of the chain waits for memory
  uint32_t dg = i < 8u ? ch->digest[i] : 0u;
  const uint32_t variant = ch->variant;
  QM31 mine = q_zero();
  {
    const uint32_t size0 = 1u << first_log;
    if (pre.src) {   // the first layer is the fold of the layer before it (same arithmetic as k_fold / MerkleFold)
      if (i < size0) {
        const uint64_t L = 2ull * size0;
        const uint32_t* __restrict__ sp = pre.src + 2ull * i;
        const QM31 a{sp[0], sp[L], sp[2 * L], sp[3 * L]};
        const QM31 b{sp[1], sp[L + 1], sp[2 * L + 1], sp[3 * L + 1]};
        mine = q_add(q_add(a, b), q_mul(*pre.alpha, q_mul_m(q_sub(a, b), pre.itw[i])));
        uint32_t* v0 = const_cast<uint32_t*>(layers[0].vals);
        v0[i] = mine.a;
        v0[size0 + i] = mine.b;
        v0[2 * size0 + i] = mine.c;
        v0[3 * size0 + i] = mine.d;
      }
    } else {
      const uint32_t* v0 = layers[0].vals;
      if (i < size0) mine = QM31{v0[i], v0[size0 + i], v0[2 * size0 + i], v0[3 * size0 + i]};
    }
  }
  for (int li = 0; li < n_layers; ++li) {
    const FriTailLayer& ly = layers[li];   // (read through the scalar cache where needed: a copy would be indexed in scratch memory)
    const int L = first_log - li;
    const uint32_t size = 1u << L;
    uint32_t cur[8];
    if (i < size) {
      uint32_t m[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) m[k] = 0u;
      m[0] = mine.a;
      m[1] = mine.b;
      m[2] = mine.c;
      m[3] = mine.d;
      shv[i] = mine.a;
      shv[MERKLE_SMALL_BLOCK + i] = mine.b;
      shv[2 * MERKLE_SMALL_BLOCK + i] = mine.c;
      shv[3 * MERKLE_SMALL_BLOCK + i] = mine.d;
      b2_compress_fresh_nz<4>(cur, m, 16u);
      store_hash(ly.merkle[L] + (uint64_t)i * 8, cur);
#pragma unroll
      for (int k = 0; k < 8; ++k) sh[k * MERKLE_SMALL_BLOCK + i] = cur[k];   // word-major (merkle_lds_level)
    }
    for (int l = L - 1; l >= 0; --l) merkle_lds_level<MERKLE_SMALL_BLOCK>(sh, ly.merkle[l], 0u, 1u << l);
    const QM31 alpha = chan_mix_root_draw_block(ch, dg, variant, sh, MERKLE_SMALL_BLOCK, sh + 16, &alphas_out[li],
                                                roots_out + li * 8);
    const uint32_t n = size >> 1;
    if (i < n) {
      const QM31 a{shv[2 * i], shv[MERKLE_SMALL_BLOCK + 2 * i], shv[2 * MERKLE_SMALL_BLOCK + 2 * i],
                   shv[3 * MERKLE_SMALL_BLOCK + 2 * i]};
      const QM31 b{shv[2 * i + 1], shv[MERKLE_SMALL_BLOCK + 2 * i + 1], shv[2 * MERKLE_SMALL_BLOCK + 2 * i + 1],
                   shv[3 * MERKLE_SMALL_BLOCK + 2 * i + 1]};
      QM31 f0 = q_add(a, b);
      QM31 f1 = q_mul_m(q_sub(a, b), ly.itw[i]);
      QM31 r = q_add(f0, q_mul(alpha, f1));
      ly.next[i] = r.a;
      ly.next[n + i] = r.b;
      ly.next[2 * n + i] = r.c;
      ly.next[3 * n + i] = r.d;
      mine = r;
    }
    __syncthreads();
  }
  if (pre.out_mirror)   // (this launch's own words of the block are visible to the block since the barrier above)
    for (uint32_t k = i; k < pre.out_words; k += blockDim.x) pre.out_mirror[k] = pre.out_block[k];
}

void launch_fri_tail(DevChannel* ch, const FriTailLayer* layers, int n_layers, int first_log, QM31* alphas_out,
                     uint32_t* roots_out, lmn_stream_t s, const FriTailIo* pre) {
  if (first_log > 10 || n_layers < 1 || n_layers > first_log) throw LmnError(-100, "fri_tail: bad arguments");
  const FriTailIo p = pre ? *pre : FriTailIo{nullptr, nullptr, nullptr, nullptr, nullptr, 0u};
  LMN_LAUNCH(k_fri_tail, dim3(1), dim3(MERKLE_SMALL_BLOCK), 0, s, ch, layers, n_layers, first_log, alphas_out,
             roots_out, p);
}

// =============================================================================================
// gather
// =============================================================================================
// A tree node its fused launch kept in registers only, recomputed from the launch's start level: lane q of a quad hashes
// start node (node << depth) + q, the quad reduces the 2^depth hashes pairwise; h of every lane of the quad = the node's
// hash.  Every lane of the workgroup calls it together (every quad does the same: block-uniform control flow).
LMN_D void merkle_recompute_node(const MerkleRecompute& j, uint32_t node, int depth, uint32_t (&h)[8]) {
  const uint32_t q = threadIdx.x & 3u;
  const uint32_t i0 = (node << depth) + (q & ((1u << depth) - 1u));
  if (j.below) {
    uint32_t mb[16];
    merkle_load_below(j.below, j.below_ncols, j.size, i0, mb);
    merkle_hash_below(j.sg, j.ncols, j.size, j.below_ncols, i0, mb, h);
  } else {
    merkle_hash_start(j.prev, j.sg, j.ncols, j.size, i0, h);
  }
  for (int s = 0; s < depth; ++s) {
    const bool hi = ((q >> s) & 1u) != 0u;
    uint32_t m[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t other = lmn_shfl_xor(h[k], 1 << s);
      m[k] = hi ? other : h[k];
      m[8 + k] = hi ? h[k] : other;
    }
    b2_compress_fresh(h, m, 64u);
  }
}

LMN_KERNEL k_gather(const uint32_t* __restrict__ arena, const uint32_t* __restrict__ shared,
                    const GatherEntry* __restrict__ entries, uint32_t n, const MerkleRecompute* __restrict__ jobs,
                    uint32_t n_jobs, uint32_t* __restrict__ out) {
  uint32_t e = blockIdx.x;
  if (e < n) {
    GatherEntry g = entries[e];
    // (block-uniform: one entry per workgroup)
    const uint32_t* src = (g.src_off & GATHER_SHARED) ? shared + (g.src_off & ~GATHER_SHARED) : arena + g.src_off;
    for (uint32_t k = threadIdx.x; k < g.len; k += blockDim.x) out[g.dst_off + k] = src[k];
    return;
  }
  e -= n;
  if (e >= n_jobs) return;
  const MerkleRecompute j = jobs[e];
  uint32_t h[8];
  merkle_recompute_node(j, j.node, j.depth, h);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) out[j.dst_off + k] = h[k];
  }
}

void launch_gather(const uint32_t* arena, const uint32_t* shared, const GatherEntry* entries, uint32_t n_entries,
                   const MerkleRecompute* jobs, uint32_t n_jobs, uint32_t* out, lmn_stream_t s) {
  if (n_entries + n_jobs == 0) return;
  LMN_LAUNCH(k_gather, dim3(n_entries + n_jobs), dim3(64), 0, s, arena, shared, entries, n_entries, jobs, n_jobs, out);
}

// =============================================================================================
// Decommitment on device handles (kernels.h launch_tree_decommit, launch_col_gather): one lane per plan entry.  A hash is
// two 16-byte loads and stores by one lane; a column word is read at base[column] + node.  The reads are a few kilobytes
// scattered over gigabytes, so there is nothing to coalesce: what counts is that the whole plan is ONE launch.
// =============================================================================================
constexpr uint32_t DECOMMIT_TPB = 256;

LMN_KERNEL k_tree_decommit(const uint32_t* const* __restrict__ src, const DecommitEntry* __restrict__ plan,
                           uint32_t n_hashes, uint32_t n_words, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_hashes + n_words) return;
  const DecommitEntry e = plan[t];
  const uint32_t* p = src[e.src];
  if (t < n_hashes) {
    const uint4* h = reinterpret_cast<const uint4*>(p) + (uint64_t)e.idx * 2;
    uint4* o = reinterpret_cast<uint4*>(out) + (uint64_t)t * 2;
    const uint4 a = h[0], b = h[1];
    o[0] = a;
    o[1] = b;
  } else {
    out[(uint64_t)n_hashes * 8 + (t - n_hashes)] = p[e.idx];
  }
}

void launch_tree_decommit(const uint32_t* const* src, const DecommitEntry* plan, uint32_t n_hashes, uint32_t n_words,
                          uint32_t* out, lmn_stream_t s) {
  const uint32_t n = n_hashes + n_words;
  if (n == 0) return;
  LMN_LAUNCH(k_tree_decommit, dim3((n + DECOMMIT_TPB - 1) / DECOMMIT_TPB), dim3(DECOMMIT_TPB), 0, s, src, plan, n_hashes,
             n_words, out);
}

LMN_KERNEL k_col_gather(const uint32_t* __restrict__ cols, uint32_t log_size, uint32_t ncols,
                        const uint32_t* __restrict__ positions, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t pos = positions[i];
  for (uint32_t j = 0; j < ncols; ++j) out[(uint64_t)j * n + i] = cols[((uint64_t)j << log_size) + pos];
}

void launch_col_gather(const uint32_t* cols, uint32_t log_size, uint32_t ncols, const uint32_t* positions, uint32_t n,
                       uint32_t* out, lmn_stream_t s) {
  if (n == 0) return;
  LMN_LAUNCH(k_col_gather, dim3((n + DECOMMIT_TPB - 1) / DECOMMIT_TPB), dim3(DECOMMIT_TPB), 0, s, cols, log_size, ncols,
             positions, n, out);
}

// =============================================================================================
// Openings planned on the device (kernels.h launch_open_plan / launch_open_offsets / launch_open_fetch).
//
// k_open_plan restates the host's opening rules (openings.h: walk_openings, for_each_pair_member) for one item per
// workgroup.  Every set it handles - the positions, a size's group, a layer's node set - is a sorted array of
// distinct values in LDS, so the sequential merge becomes counting: an element's place in a merged or compacted array is
// the number of elements in front of it, found by a block-wide exclusive scan over flags (open_scan) or a binary search
// (open_lb).  Per layer, from the leaves up:
//   A    = the parents of the previous node set, each with the mask of its children that were in it
//   G    = the layer's group: the positions folded to this size, pair-expanded under OPEN_FRI_PAIRS (then each pair member
//          that is no position gives 4 FRI witness entries)
//   cur  = A merged with G; a node of G is queried, a child outside the mask is a hash to fetch
// and a scan over cur's (hashes, queried) counts gives every entry its place in its list.  An entry carries its
// destination, so the order of the plan table itself is free and lanes write it without atomics.
// Nothing here trusts the positions: they are masked to the domain, every LDS index is checked against OPEN_MAX_NODES,
// every table index against the item's region, and k_open_fetch checks an entry's destination against the list it names.
// Control flow around every barrier depends on counts the whole workgroup holds alike.
// =============================================================================================
constexpr uint32_t OPEN_TPB = 256;
constexpr uint32_t OPEN_EPT = OPEN_MAX_NODES / OPEN_TPB;   // elements a lane owns: [tid * OPEN_EPT, (tid + 1) * OPEN_EPT)
constexpr uint32_t OPEN_GROUPS = 16;                       // the scan's second level: groups of OPEN_TPB / OPEN_GROUPS lane totals
static_assert(OPEN_EPT * OPEN_TPB == OPEN_MAX_NODES && OPEN_TPB % OPEN_GROUPS == 0, "a lane owns whole elements");

// exclusive scan of v[0 .. n) in place (n <= OPEN_MAX_NODES), returns the total; every lane of the block calls it
LMN_D uint32_t open_scan(uint32_t* v, uint32_t n, uint32_t* tot, uint32_t* grp) {
  const uint32_t tid = threadIdx.x, i0 = tid * OPEN_EPT;
  constexpr uint32_t PER = OPEN_TPB / OPEN_GROUPS;
  __syncthreads();
  uint32_t sum = 0u;
  for (uint32_t i = i0; i < i0 + OPEN_EPT && i < n; ++i) {
    const uint32_t t = v[i];
    v[i] = sum;
    sum += t;
  }
  tot[tid] = sum;
  __syncthreads();
  if (tid < OPEN_GROUPS) {
    uint32_t acc = 0u;
    for (uint32_t k = tid * PER; k < (tid + 1u) * PER; ++k) {
      const uint32_t t = tot[k];
      tot[k] = acc;
      acc += t;
    }
    grp[tid] = acc;
  }
  __syncthreads();
  uint32_t off = tot[tid], total = 0u;
  for (uint32_t g = 0; g < OPEN_GROUPS; ++g) {
    const uint32_t x = grp[g];
    off += g < tid / PER ? x : 0u;
    total += x;
  }
  for (uint32_t i = i0; i < i0 + OPEN_EPT && i < n; ++i) v[i] += off;
  __syncthreads();
  return total;
}
// number of elements of the ascending a[0 .. n) below x (ends for any content)
LMN_D uint32_t open_lb(const uint32_t* a, uint32_t n, uint32_t x) {
  uint32_t lo = 0u, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < x)
      lo = mid + 1u;
    else
      hi = mid;
  }
  return lo;
}

LMN_KERNEL k_open_plan(const uint32_t* __restrict__ count, const uint32_t* __restrict__ positions,
                       const uint32_t* __restrict__ found, uint32_t log_domain, const OpenItemDesc* __restrict__ items,
                       OpenItemHeader* __restrict__ headers, OpenEntry* __restrict__ entries, OpenEntry* __restrict__ jobs) {
  LMN_SHARED uint32_t s_pos[OPEN_MAX_POSITIONS];
  LMN_SHARED uint32_t s_set[2][OPEN_MAX_NODES];   // the previous and the current node set, swapped per layer
  LMN_SHARED uint32_t s_a[OPEN_MAX_NODES], s_g[OPEN_MAX_NODES], s_scan[OPEN_MAX_NODES];
  LMN_SHARED uint8_t s_amask[OPEN_MAX_NODES];     // A: bit b = child 2 * node + b was in the previous set
  LMN_SHARED uint8_t s_gin[OPEN_MAX_NODES];       // pair-expanded G: the member is a position itself
  LMN_SHARED uint8_t s_cflag[OPEN_MAX_NODES];     // cur: the child mask | 4 = queried
  LMN_SHARED uint32_t s_tot[OPEN_TPB], s_grp[OPEN_GROUPS];
  const uint32_t tid = threadIdx.x, i0 = tid * OPEN_EPT;
  const OpenItemDesc* it = items + blockIdx.x;
  const uint32_t max_log = it->max_log, layer_src0 = it->layer_src0, col_src0 = it->col_src0, cap = it->ent_cap;
  const bool pairs = (it->flags & OPEN_FRI_PAIRS) != 0u;
  OpenEntry* ent = entries + it->ent_off;
  OpenEntry* job = jobs + it->job_off;
  const uint32_t job_cap = it->job_cap;
  // (block-uniform: no positions without a nonce, and none for an item without a tree)
  const bool idle = (found && *found != 1u) || (it->flags & OPEN_EMPTY) != 0u;
  const uint32_t n = idle ? 0u : *count < OPEN_MAX_POSITIONS ? *count : OPEN_MAX_POSITIONS;
  bool overflow = !idle && (log_domain > OPEN_MAX_LOG || max_log > log_domain);
  const uint32_t dmask = overflow ? 0u : (uint32_t)((1ull << log_domain) - 1u);
  for (uint32_t i = tid; i < n; i += OPEN_TPB) s_pos[i] = positions[i] & dmask;
  __syncthreads();   // (the only barrier a lane's own elements do not cover: s_pos is loaded strided)
  uint32_t cnt[4] = {0u, 0u, 0u, 0u};
  uint32_t ne = 0u, nj = 0u, first_col = 0u, np = 0u;
  uint32_t* prev = s_set[0];
  uint32_t* cur = s_set[1];
  for (int log = idle ? -1 : (int)max_log; log >= 0 && !overflow; --log) {
    const uint32_t nc = it->ncols[log], shift = log_domain - (uint32_t)log;
    const uint32_t lmask = (uint32_t)((1ull << log) - 1u), cmask = (uint32_t)((2ull << log) - 1u);
    const bool have_prev = log < (int)max_log;
    // ---- A: the parents of the previous set
    uint32_t na = 0u;
    if (np) {
      for (uint32_t i = i0; i < i0 + OPEN_EPT && i < np; ++i) s_scan[i] = i == 0u || (prev[i] >> 1) != (prev[i - 1u] >> 1) ? 1u : 0u;
      na = open_scan(s_scan, np, s_tot, s_grp);
      for (uint32_t i = i0; i < i0 + OPEN_EPT && i < np; ++i) {
        const uint32_t v = prev[i];
        if (i != 0u && (v >> 1) == (prev[i - 1u] >> 1)) continue;
        uint32_t m = 1u << (v & 1u);
        if (i + 1u < np && (prev[i + 1u] >> 1) == (v >> 1)) m |= 1u << (prev[i + 1u] & 1u);
        s_a[s_scan[i]] = v >> 1;   // (its rank among at most np first-of-pair elements)
        s_amask[s_scan[i]] = (uint8_t)m;
      }
    }
    // ---- G: the positions folded to this size; F (the plain fold) is kept in `cur` while the pairs are made
    uint32_t ng = 0u;
    if (nc && n) {
      if (pairs && nc != 4u) {
        overflow = true;
        break;
      }
      for (uint32_t i = i0; i < i0 + OPEN_EPT && i < n; ++i)
        s_scan[i] = i == 0u || (s_pos[i] >> shift) != (s_pos[i - 1u] >> shift) ? 1u : 0u;
      const uint32_t nf = open_scan(s_scan, n, s_tot, s_grp);
      uint32_t* F = pairs ? cur : s_g;
      for (uint32_t i = i0; i < i0 + OPEN_EPT && i < n; ++i)
        if (i == 0u || (s_pos[i] >> shift) != (s_pos[i - 1u] >> shift)) F[s_scan[i]] = s_pos[i] >> shift;
      ng = nf;
      if (pairs) {
        __syncthreads();
        for (uint32_t i = i0; i < i0 + OPEN_EPT && i < nf; ++i) s_scan[i] = i == 0u || (F[i] >> 1) != (F[i - 1u] >> 1) ? 1u : 0u;
        const uint32_t n_pairs = open_scan(s_scan, nf, s_tot, s_grp);
        for (uint32_t i = i0; i < i0 + OPEN_EPT && i < nf; ++i) {
          const uint32_t v = F[i];
          if (i != 0u && (v >> 1) == (F[i - 1u] >> 1)) continue;
          const uint32_t k = 2u * s_scan[i];   // n_pairs <= nf <= 1024: k + 1 < OPEN_MAX_NODES
          const bool both = i + 1u < nf && (F[i + 1u] >> 1) == (v >> 1);
          s_g[k] = v & ~1u;
          s_g[k + 1u] = v | 1u;
          s_gin[k] = (v & 1u) == 0u ? 1u : 0u;
          s_gin[k + 1u] = (v & 1u) != 0u || both ? 1u : 0u;
        }
        ng = 2u * n_pairs;
        // the FRI witness of this size: 4 coordinate words per member that is no position, members ascending
        const uint32_t n_fri = ng >= nf ? ng - nf : 0u;
        if (ne + 4u * n_fri > cap) {
          overflow = true;
          break;
        }
        __syncthreads();
        for (uint32_t e = i0; e < i0 + OPEN_EPT && e < ng; ++e) {
          if (s_gin[e]) continue;
          const uint32_t at = e - open_lb(F, nf, s_g[e]);   // members in front of it that are no positions either
          if (at >= n_fri) continue;
          for (uint32_t k = 0; k < 4u; ++k)
            ent[ne + 4u * at + k] = OpenEntry{col_src0 + first_col + k, s_g[e] & lmask, cnt[OPEN_LIST_FRI] + 4u * at + k, OPEN_LIST_FRI};
        }
        cnt[OPEN_LIST_FRI] += 4u * n_fri;
        ne += 4u * n_fri;
      }
    }
    // ---- cur = A merged with G
    __syncthreads();
    uint32_t ncur;
    if (ng == 0u || na == 0u) {
      ncur = ng ? ng : na;
      for (uint32_t i = i0; i < i0 + OPEN_EPT && i < ncur; ++i) {
        cur[i] = ng ? s_g[i] : s_a[i];
        s_cflag[i] = ng ? (uint8_t)4u : s_amask[i];
      }
    } else {
      for (uint32_t i = i0; i < i0 + OPEN_EPT && i < na; ++i) {
        const uint32_t lb = open_lb(s_g, ng, s_a[i]);
        s_scan[i] = lb < ng && s_g[lb] == s_a[i] ? 1u : 0u;
      }
      const uint32_t n_both = open_scan(s_scan, na, s_tot, s_grp);   // s_scan[i]: nodes of A below A[i] that are in G as well
      ncur = na + ng - n_both;
      if (ncur > OPEN_MAX_NODES) {
        overflow = true;
        break;
      }
      for (uint32_t i = i0; i < i0 + OPEN_EPT && i < na; ++i) {
        const uint32_t a = s_a[i], lb = open_lb(s_g, ng, a);
        const bool in_g = lb < ng && s_g[lb] == a;
        const uint32_t r = i + lb - s_scan[i];
        if (r < ncur) {
          cur[r] = a;
          s_cflag[r] = (uint8_t)(s_amask[i] | (in_g ? 4u : 0u));
        }
      }
      for (uint32_t j = i0; j < i0 + OPEN_EPT && j < ng; ++j) {
        const uint32_t g = s_g[j], lb = open_lb(s_a, na, g);
        if (lb < na && s_a[lb] == g) continue;
        const uint32_t r = j + lb - (lb < na ? s_scan[lb] : n_both);
        if (r < ncur) {
          cur[r] = g;
          s_cflag[r] = (uint8_t)4u;
        }
      }
    }
    // ---- the layer's entries: per node the hashes of its children outside the mask, then its column values
    __syncthreads();
    for (uint32_t i = i0; i < i0 + OPEN_EPT && i < ncur; ++i) {
      const uint32_t f = s_cflag[i];
      const uint32_t hc = have_prev ? 2u - (f & 1u) - ((f >> 1) & 1u) : 0u;
      s_scan[i] = hc | ((f >> 2) & 1u) << 16;
    }
    const uint32_t both_tot = open_scan(s_scan, ncur, s_tot, s_grp);
    const uint32_t nh = both_tot & 0xffffu, nq = both_tot >> 16, nw = ncur - nq;
    // the children's layer was kept in registers by its launch: their hashes are recompute jobs
    const uint32_t cut = have_prev ? it->cut_of_layer[log + 1] : OPEN_STORED;
    const uint32_t nh_ent = cut == OPEN_STORED ? nh : 0u, nh_job = nh - nh_ent;
    if (ne + nh_ent + ncur * nc > cap || nj + nh_job > job_cap) {
      overflow = true;
      break;
    }
    for (uint32_t i = i0; i < i0 + OPEN_EPT && i < ncur; ++i) {
      const uint32_t f = s_cflag[i], node = cur[i] & lmask;
      const uint32_t qp = s_scan[i] >> 16, wp = i - qp;
      uint32_t hp = s_scan[i] & 0xffffu, slot = ne + (cut == OPEN_STORED ? hp : 0u) + i * nc;
      if (have_prev) {
        for (uint32_t b = 0; b < 2u; ++b)
          if (!((f >> b) & 1u)) {
            const uint32_t child = (2u * node + b) & cmask, dst = (cnt[OPEN_LIST_HASH] + hp) * 8u;
            if (cut == OPEN_STORED)
              ent[slot++] = OpenEntry{layer_src0 + (uint32_t)log + 1u, child, dst, OPEN_LIST_HASH};
            else
              job[nj + hp] = OpenEntry{cut, child, dst, OPEN_LIST_HASH | ((uint32_t)log + 1u) << 8};   // (| the children's layer)
            ++hp;
          }
      }
      const bool q = (f & 4u) != 0u;
      const uint32_t dst0 = q ? cnt[OPEN_LIST_QUERIED] + qp * nc : cnt[OPEN_LIST_WITNESS] + wp * nc;
      for (uint32_t c = 0; c < nc; ++c)
        ent[slot++] = OpenEntry{col_src0 + first_col + c, node, dst0 + c, q ? (uint32_t)OPEN_LIST_QUERIED : (uint32_t)OPEN_LIST_WITNESS};
    }
    cnt[OPEN_LIST_HASH] += nh;
    cnt[OPEN_LIST_QUERIED] += nq * nc;
    cnt[OPEN_LIST_WITNESS] += nw * nc;
    ne += nh_ent + ncur * nc;
    nj += nh_job;
    first_col += nc;
    uint32_t* t = prev;
    prev = cur;
    cur = t;
    np = ncur;
  }
  if (tid == 0u) {
    OpenItemHeader* h = headers + blockIdx.x;
    for (int k = 0; k < 4; ++k) h->count[k] = overflow ? 0u : cnt[k];
    h->n_entries = overflow ? 0u : ne;
    h->n_jobs = overflow ? 0u : nj;
    h->overflow = overflow ? 1u : 0u;
  }
}

// (one lane: at most 64 items x 4 lists, a few hundred cycles behind the planner - not worth a scan)
LMN_KERNEL k_open_offsets(const uint32_t* __restrict__ count, OpenHeader* header, OpenItemHeader* headers, uint32_t n_items,
                          uint32_t out_cap_words) {
  if (threadIdx.x != 0u) return;
  uint64_t at = 0u;
  uint32_t overflow = 0u;
  for (uint32_t k = 0; k < n_items; ++k) {
    OpenItemHeader* h = headers + k;
    overflow |= h->overflow;
    for (int l = 0; l < 4; ++l) {
      h->base[l] = (uint32_t)(at < out_cap_words ? at : out_cap_words);
      at += (uint64_t)h->count[l] * (l == OPEN_LIST_HASH ? 8u : 1u);
    }
  }
  if (at > out_cap_words) overflow = 1u;
  header->overflow = overflow;
  header->total_words = overflow ? 0u : (uint32_t)at;
  header->n_positions = *count < OPEN_MAX_POSITIONS ? *count : OPEN_MAX_POSITIONS;
}

// (an entry that fails a check below can only come from a defect of the planner: it raises the header's overflow word - a
// plain vector store of 1, whoever else stores it - and the host refuses the whole opening instead of reading stale words)
LMN_KERNEL k_open_fetch(const uint32_t* const* __restrict__ src, uint32_t n_src, const OpenItemDesc* __restrict__ items,
                        OpenHeader* header, const OpenItemHeader* __restrict__ headers,
                        const OpenEntry* __restrict__ entries, uint32_t* __restrict__ out) {
  const uint32_t item = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (header->overflow) return;
  const OpenItemHeader* h = headers + item;
  if (t >= h->n_entries || t >= items[item].ent_cap) return;   // the launch covers the host's upper bound
  const OpenEntry e = entries[items[item].ent_off + t];
  if (e.list > 3u || e.src >= n_src) {
    header->overflow = 1u;
    return;
  }
  const bool hash = e.list == OPEN_LIST_HASH;
  if ((uint64_t)e.dst + (hash ? 8u : 1u) > (uint64_t)h->count[e.list] * (hash ? 8u : 1u)) {
    header->overflow = 1u;
    return;
  }
  const uint32_t* p = src[e.src];
  uint32_t* o = out + h->base[e.list] + e.dst;   // (word-aligned only: the lists are compact)
  if (hash) {
    const uint4* hp = reinterpret_cast<const uint4*>(p) + (uint64_t)e.idx * 2;
    const uint4 a = hp[0], b = hp[1];
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w;
    o[4] = b.x, o[5] = b.y, o[6] = b.z, o[7] = b.w;
  } else {
    *o = p[e.idx];
  }
}

// A hash of a layer its fused launch never stored (k_gather's second form): one workgroup per job over the host's upper
// bound; lane q of a quad hashes start node (node << depth) + q, the quad reduces pairwise, every quad does the same.
LMN_KERNEL k_open_recompute(const MerkleRecompute* __restrict__ cuts, uint32_t n_cuts, const OpenItemDesc* __restrict__ items,
                            OpenHeader* header, const OpenItemHeader* __restrict__ headers,
                            const OpenEntry* __restrict__ jobs, uint32_t* __restrict__ out) {
  const uint32_t item = blockIdx.y, t = blockIdx.x;
  if (header->overflow) return;   // (block-uniform, as every return below)
  const OpenItemHeader* h = headers + item;
  if (t >= h->n_jobs || t >= items[item].job_cap) return;
  const OpenEntry e = jobs[items[item].job_off + t];
  if (e.src >= n_cuts || (uint64_t)e.dst + 8u > (uint64_t)h->count[OPEN_LIST_HASH] * 8u) {
    if (threadIdx.x == 0u) header->overflow = 1u;
    return;
  }
  const MerkleRecompute j = cuts[e.src];
  int start_log = 0;
  while ((1u << start_log) < j.size && start_log < 31) ++start_log;
  const int depth = start_log - (int)(e.list >> 8);
  if (depth < 0 || depth > 2) {
    if (threadIdx.x == 0u) header->overflow = 1u;
    return;
  }
  const uint32_t node = e.idx & ((1u << (start_log - depth)) - 1u);
  uint32_t hh[8];
  merkle_recompute_node(j, node, depth, hh);
  if (threadIdx.x == 0) {
    uint32_t* o = out + h->base[OPEN_LIST_HASH] + e.dst;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = hh[k];
  }
}

void launch_open_plan(const uint32_t* count, const uint32_t* positions, const uint32_t* found, uint32_t log_domain,
                      const OpenItemDesc* items, uint32_t n_items, OpenItemHeader* headers, OpenEntry* entries, OpenEntry* jobs,
                      lmn_stream_t s, uint64_t* n_launched) {
  if (!count || !positions || !items || !headers || !entries || !jobs || n_items == 0 || n_items > OPEN_MAX_ITEMS ||
      log_domain > OPEN_MAX_LOG)
    throw LmnError(-100, "open_plan: bad arguments");
  LMN_LAUNCH(k_open_plan, dim3(n_items), dim3(OPEN_TPB), 0, s, count, positions, found, log_domain, items, headers, entries, jobs);
  if (n_launched) ++*n_launched;
}
void launch_open_offsets(const uint32_t* count, OpenHeader* header, OpenItemHeader* headers, uint32_t n_items,
                         uint32_t out_cap_words, lmn_stream_t s) {
  LMN_LAUNCH(k_open_offsets, dim3(1), dim3(1), 0, s, count, header, headers, n_items, out_cap_words);
}
void launch_open_recompute(const MerkleRecompute* cuts, uint32_t n_cuts, const OpenItemDesc* items, uint32_t n_items,
                           uint32_t max_job_cap, OpenHeader* header, const OpenItemHeader* headers, const OpenEntry* jobs,
                           uint32_t* out, lmn_stream_t s) {
  if (max_job_cap == 0 || n_items == 0) return;
  LMN_LAUNCH(k_open_recompute, dim3(max_job_cap, n_items), dim3(64), 0, s, cuts, n_cuts, items, header, headers, jobs, out);
}
void launch_open_fetch(const uint32_t* const* src, uint32_t n_src, const OpenItemDesc* items, uint32_t n_items,
                       uint32_t max_cap, OpenHeader* header, const OpenItemHeader* headers, const OpenEntry* entries,
                       uint32_t* out, lmn_stream_t s, uint64_t* n_launched) {
  if (max_cap == 0 || n_items == 0) return;
  if (n_launched) ++*n_launched;
  LMN_LAUNCH(k_open_fetch, dim3((max_cap + OPEN_TPB - 1) / OPEN_TPB, n_items), dim3(OPEN_TPB), 0, s, src, n_src, items,
             header, headers, entries, out);
}

// =============================================================================================
// Proof-of-work grind (kernels.h launch_pow_grind): one compression per nonce, the smallest passing nonce of the
// window by a 64-bit atomicMin.  Block b examines [lo, lo + POW_TPB * POW_NPT) with lo = base + b * POW_TPB * POW_NPT,
// lane t the nonces lo + k * POW_TPB + t in ascending k, and stops at its first hit: the minimum of the window is exact
// (a block skips only when a smaller nonce has already been found, and a lane's first hit is its smallest).
// =============================================================================================
LMN_D unsigned long long pow_best_now(const unsigned long long* best) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(LMN_EMU)
  return __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // past the (non-coherent) vector L1
#else
  return *best;
#endif
}

// one nonce: the compression of its form with the zero message words folded out (blake2s.h b2_half_z)
template <bool KAT>
LMN_D bool pow_nonce_passes(const PowWords& pw, uint64_t nonce, uint64_t mask) {
  uint32_t m[16], h[8];
  if constexpr (KAT) {
    for (int i = 0; i < 8; ++i) h[i] = pw.w[i];
    m[0] = (uint32_t)nonce;
    m[1] = (uint32_t)(nonce >> 32);
    for (int i = 2; i < 16; ++i) m[i] = 0u;
    b2_compress_cv_nz<2>(h, m, 0u, 0u);
  } else {
    for (int i = 0; i < 8; ++i) m[i] = pw.w[i];
    m[8] = (uint32_t)nonce;
    m[9] = (uint32_t)(nonce >> 32);
    for (int i = 10; i < 16; ++i) m[i] = 0u;
    b2_compress_fresh_nz<10>(h, m, 40u);
  }
  // trailing zeros of words 0..3 (little-endian) >= pow_bits <=> the low pow_bits bits of words 0..1 are zero (pow_bits <= 40)
  return (((uint64_t)h[1] << 32 | h[0]) & mask) == 0u;
}

template <bool KAT>
LMN_KERNEL k_pow_grind(PowWords pw, uint64_t base, uint64_t mask, unsigned long long* best) {
  const uint64_t lo = base + (uint64_t)blockIdx.x * (POW_TPB * POW_NPT);
  if (pow_best_now(best) < lo) return;
  uint64_t found = ~0ull;
  for (uint32_t k = 0; k < POW_NPT; ++k) {
    const uint64_t nonce = lo + k * POW_TPB + threadIdx.x;
    if (pow_nonce_passes<KAT>(pw, nonce, mask)) {
      found = nonce;
      break;
    }
  }
  if (found != ~0ull) atomicMin(best, (unsigned long long)found);
}

// The same examination for MANY digests in one launch (kernels.h launch_grind_many): blockIdx.y selects an entry of the
// pending table, the entry a digest of `digests` and its word of `best`; blockIdx.x is k_pow_grind's block.  The entry
// and the eight digest words are the same for the whole workgroup: they are read through the scalar cache (constant
// address space, as k_quotients reads its entry table - nothing writes either table during the launch).
template <bool KAT>
LMN_KERNEL k_grind_many(const PowWords* __restrict__ digests, const uint32_t* __restrict__ pending, uint64_t base,
                        uint64_t mask, unsigned long long* best_of) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(LMN_EMU)
  typedef const uint32_t __attribute__((address_space(4))) * ConstWords;
  const uint32_t idx = ((ConstWords)(uintptr_t)pending)[blockIdx.y];
  const ConstWords dw = (ConstWords)(uintptr_t)(digests + idx);
#else
  const uint32_t idx = pending[blockIdx.y];
  const uint32_t* dw = digests[idx].w;
#endif
  unsigned long long* best = best_of + idx;
  const uint64_t lo = base + (uint64_t)blockIdx.x * (POW_TPB * POW_NPT);
  if (pow_best_now(best) < lo) return;
  PowWords pw;
  for (int i = 0; i < 8; ++i) pw.w[i] = dw[i];
  uint64_t found = ~0ull;
  for (uint32_t k = 0; k < POW_NPT; ++k) {
    const uint64_t nonce = lo + k * POW_TPB + threadIdx.x;
    if (pow_nonce_passes<KAT>(pw, nonce, mask)) {
      found = nonce;
      break;
    }
  }
  if (found != ~0ull) atomicMin(best, (unsigned long long)found);
}
#ifdef LMN_BATCH
// the batch build's kernels are device functions behind the trampoline; the leader of a grind collective launches this
// one itself (batch.cpp k_batch_copy is the precedent), so it gets an entry of its own
template <bool KAT>
__global__ void k_grind_many_entry(const PowWords* __restrict__ digests, const uint32_t* __restrict__ pending, uint64_t base,
                                   uint64_t mask, unsigned long long* best_of) {
  k_grind_many<KAT>(digests, pending, base, mask, best_of);
}
#endif

void launch_pow_grind(const PowWords& w, bool kat, uint64_t base, int window_log, uint32_t pow_bits,
                      unsigned long long* best, lmn_stream_t s) {
  static_assert(POW_TPB * POW_NPT == 1u << POW_MIN_WINDOW_LOG, "one block = the smallest window");
  if (window_log < POW_MIN_WINDOW_LOG || window_log > 32 || pow_bits > 40) throw LmnError(-100, "pow_grind: bad window");
  const uint64_t mask = (1ull << pow_bits) - 1u;
  const dim3 grid(1u << (window_log - POW_MIN_WINDOW_LOG));
  if (kat) {
    LMN_LAUNCH(k_pow_grind<true>, grid, dim3(POW_TPB), 0, s, w, base, mask, best);
  } else {
    LMN_LAUNCH(k_pow_grind<false>, grid, dim3(POW_TPB), 0, s, w, base, mask, best);
  }
}

void launch_grind_many(const PowWords* digests, const uint32_t* pending, uint32_t n_pending, bool kat, uint64_t base,
                       int window_log, uint32_t pow_bits, unsigned long long* best, lmn_stream_t s) {
  if (window_log < POW_MIN_WINDOW_LOG || window_log > 32 || pow_bits > 40 || n_pending == 0 || n_pending > 65535u)
    throw LmnError(-100, "grind_many: bad window");
  const uint64_t mask = (1ull << pow_bits) - 1u;
  const dim3 grid(1u << (window_log - POW_MIN_WINDOW_LOG), n_pending);
#ifdef LMN_BATCH
  // issued by the one member that runs the collective, not by every member: past the trampoline
  if (kat)
    hipLaunchKernelGGL(k_grind_many_entry<true>, grid, dim3(POW_TPB), 0, s, digests, pending, base, mask, best);
  else
    hipLaunchKernelGGL(k_grind_many_entry<false>, grid, dim3(POW_TPB), 0, s, digests, pending, base, mask, best);
  batch_check_hip(hipGetLastError(), "grind_many launch");
#else
  if (kat) {
    LMN_LAUNCH(k_grind_many<true>, grid, dim3(POW_TPB), 0, s, digests, pending, base, mask, best);
  } else {
    LMN_LAUNCH(k_grind_many<false>, grid, dim3(POW_TPB), 0, s, digests, pending, base, mask, best);
  }
#endif
}

// =============================================================================================
// The close of the FRI transcript (kernels.h launch_fri_close / launch_fri_queries): one workgroup each, block-uniform
// control flow, nothing whose length depends on the data - the host decides on first_bad and on a grind without a hit.
// =============================================================================================
constexpr uint32_t FRI_CLOSE_TPB = 1024;
constexpr uint32_t FRI_CLOSE_PAIRS = (1u << (FRI_CLOSE_MAX_LOG - 1)) / FRI_CLOSE_TPB;   // butterflies per lane and pass
static_assert(FRI_CLOSE_PAIRS * FRI_CLOSE_TPB * 2u == 1u << FRI_CLOSE_MAX_LOG, "a pass is held in registers across its barrier");

// Line interpolation as run_fri_commit's host loop does it: a pass over chunks of 2^d values turns the neighbours
// (2i, 2i+1) of every chunk into f0 = a + b (first half of the chunk) and f1 = (a - b) / x_i (second half); after log_n
// passes value bit_reverse(j) is coefficient j times n.  A pass reads its pairs into registers, waits, and writes: in place.
LMN_KERNEL k_fri_close(DevChannel* ch, const uint32_t* __restrict__ last, int log_n, int log_bound, FriCloseItw itw,
                       uint32_t n_inv, uint32_t* scratch, uint32_t* __restrict__ coeffs, int pow_prefixed, uint32_t pow_bits,
                       FriCloseState* st) {
  LMN_SHARED uint32_t sh[4u << FRI_CLOSE_LDS_LOG];                        // the passes of a layer of up to 2^FRI_CLOSE_LDS_LOG values
  LMN_SHARED uint32_t W[8 + (4 << FRI_CLOSE_MAX_BOUND_LOG) + 16];         // digest || coefficients, zero-padded to whole blocks
  LMN_SHARED uint32_t scr[32];                                            // digest 8 (+ 8 unused) | the prefixed form's message 16
  LMN_SHARED int sh_bad;
  const uint32_t tid = threadIdx.x, q = tid & 3u;
  const uint32_t n = 1u << log_n, bound = 1u << log_bound;
  const uint32_t dgw = tid < 8u ? ch->digest[tid] : 0u;
  uint32_t* buf = log_n <= FRI_CLOSE_LDS_LOG ? sh : scratch;               // coordinate k of value i at buf[k * n + i]
  for (uint32_t k = tid; k < 4u * n; k += blockDim.x) buf[k] = last[k];
  if (tid == 0u) sh_bad = 0x7fffffff;
  __syncthreads();
  for (int d = log_n; d >= 1; --d) {
    const uint32_t half = 1u << (d - 1);
    const uint32_t* __restrict__ tw = itw.p[d];
    QM31 f0[FRI_CLOSE_PAIRS], f1[FRI_CLOSE_PAIRS];
#pragma unroll
    for (uint32_t k = 0; k < FRI_CLOSE_PAIRS; ++k) {
      const uint32_t p = tid + k * FRI_CLOSE_TPB;   // pair i of chunk c: values c * 2^d + 2i, + 1
      if (p < n / 2u) {
        const uint32_t i = p & (half - 1u), at = 2u * p;
        const QM31 a{buf[at], buf[n + at], buf[2u * n + at], buf[3u * n + at]};
        const QM31 b{buf[at + 1u], buf[n + at + 1u], buf[2u * n + at + 1u], buf[3u * n + at + 1u]};
        f0[k] = q_add(a, b);
        f1[k] = q_mul_m(q_sub(a, b), tw[i]);
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < FRI_CLOSE_PAIRS; ++k) {
      const uint32_t p = tid + k * FRI_CLOSE_TPB;
      if (p < n / 2u) {
        const uint32_t i = p & (half - 1u), at = ((p >> (d - 1)) << d) + i;
        buf[at] = f0[k].a;
        buf[n + at] = f0[k].b;
        buf[2u * n + at] = f0[k].c;
        buf[3u * n + at] = f0[k].d;
        buf[at + half] = f1[k].a;
        buf[n + at + half] = f1[k].b;
        buf[2u * n + at + half] = f1[k].c;
        buf[3u * n + at + half] = f1[k].d;
      }
    }
    __syncthreads();
  }
  // ---- coefficient j = value bit_reverse(j) / n; the degree check; W = digest || the first `bound` coefficients
  const uint32_t total_words = 8u + 4u * bound, padded_words = (total_words + 15u) / 16u * 16u;
  if (tid < 8u) W[tid] = dgw;
  for (uint32_t k = total_words + tid; k < padded_words; k += blockDim.x) W[k] = 0u;
  int bad = 0x7fffffff;
  for (uint32_t j = tid; j < n; j += blockDim.x) {
    const uint32_t at = log_n ? __brev(j) >> (32 - log_n) : 0u;
    const QM31 c = q_mul_m(QM31{buf[at], buf[n + at], buf[2u * n + at], buf[3u * n + at]}, n_inv);
    coeffs[4u * j] = c.a;
    coeffs[4u * j + 1u] = c.b;
    coeffs[4u * j + 2u] = c.c;
    coeffs[4u * j + 3u] = c.d;
    if (j < bound) {
      W[8u + 4u * j] = c.a;
      W[9u + 4u * j] = c.b;
      W[10u + 4u * j] = c.c;
      W[11u + 4u * j] = c.d;
    } else if (!q_is_zero(c) && bad == 0x7fffffff) {
      bad = (int)j;   // (a lane meets its indices in ascending order)
    }
  }
  if (bad != 0x7fffffff) atomicMin(&sh_bad, bad);
  __syncthreads();
  // ---- Channel::mix_felts
  uint32_t* msg = scr;
  qchan_hash_blocks(W, total_words, msg);
  __syncthreads();
  if (tid < 8u) {
    ch->digest[tid] = msg[tid];
    st->digest_after_coeffs[tid] = msg[tid];
  }
  // ---- the words the grind hashes: the digest, or blake2s(0x12345678 || 12 zero bytes || digest || pow_bits) (52 bytes)
  uint32_t* pre = scr + 16;
  if (tid < 16u) pre[tid] = tid == 0u ? 0x12345678u : tid >= 4u && tid < 12u ? msg[tid - 4u] : tid == 12u ? pow_bits : 0u;
  __syncthreads();
  uint32_t lo = 0u, hi = 0u;
  if (tid < 64u) b2_quad_parent(pre, q, lo, hi, 52u);
  if (tid < 4u) {
    st->pow.w[q] = pow_prefixed ? lo : msg[q];
    st->pow.w[4u + q] = pow_prefixed ? hi : msg[4u + q];
  }
  if (tid == 0u) {
    ch->n_sent = 0u;
    st->best = ~0ull;
    st->pending = 0u;
    st->first_bad = sh_bad == 0x7fffffff ? 0xffffffffu : (uint32_t)sh_bad;
  }
}

void launch_fri_close(DevChannel* ch, const uint32_t* last, int log_n, int log_bound, const FriCloseItw& itw, uint32_t n_inv,
                      uint32_t* scratch, uint32_t* coeffs, bool pow_prefixed, uint32_t pow_bits, FriCloseState* st,
                      lmn_stream_t s) {
  if (!ch || !last || !coeffs || !st || log_n < 0 || log_n > FRI_CLOSE_MAX_LOG || log_bound < 0 || log_bound > log_n ||
      log_bound > FRI_CLOSE_MAX_BOUND_LOG || (log_n > FRI_CLOSE_LDS_LOG && !scratch))
    throw LmnError(-100, "fri_close: bad arguments");
  for (int d = 1; d <= log_n; ++d)
    if (!itw.p[d]) throw LmnError(-100, "fri_close: a twiddle table is missing");
  LMN_LAUNCH(k_fri_close, dim3(1), dim3(FRI_CLOSE_TPB), 0, s, ch, last, log_n, log_bound, itw, n_inv, scratch, coeffs,
             pow_prefixed ? 1 : 0, pow_bits, st);
}

// Every draw hashes digest || its own counter: draw k is the business of quad k alone, all of them at once.  Positions are
// made distinct and ranked by counting (at most 1024 of them: two passes over LDS per lane).
LMN_KERNEL k_fri_queries(DevChannel* ch, const FriCloseState* __restrict__ st, const uint32_t* __restrict__ coeffs,
                         uint32_t n_coeff_words, int hashed, uint32_t n_queries, uint32_t pos_mask, uint32_t* __restrict__ out) {
  static_assert(FRI_CLOSE_TPB == FRI_CLOSE_MAX_QUERIES, "one lane per position");
  LMN_SHARED uint32_t msgs[FRI_CLOSE_MAX_QUERIES / 8u * 16u];   // one message per draw; afterwards the sorted positions
  LMN_SHARED uint32_t pos[FRI_CLOSE_MAX_QUERIES], first[FRI_CLOSE_MAX_QUERIES];
  LMN_SHARED uint32_t scr[32];                                   // digest || nonce | the digest behind the coefficients
  const uint32_t tid = threadIdx.x, q = tid & 3u;
  FriCloseHeader* hdr = reinterpret_cast<FriCloseHeader*>(out);
  const unsigned long long nonce = st->best;
  if (nonce == ~0ull) {   // block-uniform
    if (tid == 0u) hdr->found = 0u;
    return;
  }
  const uint32_t variant = ch->variant;
  uint32_t* msg = scr;
  if (tid < 8u) {
    msg[tid] = ch->digest[tid];
    scr[16u + tid] = msg[tid];
  } else if (tid < 16u) {
    msg[tid] = tid == 8u ? (uint32_t)nonce : tid == 9u ? (uint32_t)(nonce >> 32) : 0u;
  }
  // ---- Channel::mix_u64: blake2s(digest || nonce LE), or the KAT form's bare compression (h = digest, m = nonce, t = 0, no final flag)
  if (hashed) {
    qchan_mix(msg, 2u);
  } else {
    __syncthreads();
    if (tid == 0u) {
      uint32_t h[8], m[16];
      for (int k = 0; k < 8; ++k) h[k] = msg[k];
      for (int k = 0; k < 16; ++k) m[k] = k < 2 ? msg[8 + k] : 0u;
      b2_compress(h, m, 0u, 0u);
      for (int k = 0; k < 8; ++k) msg[k] = h[k];
    }
  }
  __syncthreads();
  // ---- draw_random_words, ceil(n_queries / 8) times
  const uint32_t n_draws = (n_queries + 7u) / 8u;
  for (uint32_t k = tid; k < n_draws * 16u; k += blockDim.x) msgs[k] = (k & 15u) < 8u ? msg[k & 15u] : (k & 15u) == 8u ? k >> 4 : 0u;
  __syncthreads();
  const uint32_t g = tid >> 2;
  if (g < n_draws) {   // whole quads
    uint32_t lo = 0u, hi = 0u;
    b2_quad_parent(msgs + 16u * g, q, lo, hi, variant == 0u ? 64u : 37u);
    if (8u * g + q < n_queries) pos[8u * g + q] = lo & pos_mask;
    if (8u * g + 4u + q < n_queries) pos[8u * g + 4u + q] = hi & pos_mask;
  }
  __syncthreads();
  // ---- ascending and distinct: a position counts at its first occurrence, its rank is the number of smaller ones that count
  const uint32_t v = tid < n_queries ? pos[tid] : 0u;
  uint32_t is_first = tid < n_queries ? 1u : 0u;
  for (uint32_t j = 0; j < tid && j < n_queries; ++j) is_first &= pos[j] != v ? 1u : 0u;
  first[tid] = is_first;
  __syncthreads();
  uint32_t rank = 0u, n_positions = 0u;
  for (uint32_t j = 0; j < n_queries; ++j) {
    n_positions += first[j];
    rank += first[j] & (pos[j] < v ? 1u : 0u);
  }
  uint32_t* sorted = msgs;
  if (is_first) sorted[rank] = v;
  __syncthreads();
  // ---- the result block
  uint32_t* out_pos = out + sizeof(FriCloseHeader) / 4u;
  uint32_t* out_coeffs = out_pos + n_queries;
  if (tid < n_positions) out_pos[tid] = sorted[tid];
  for (uint32_t k = tid; k < n_coeff_words; k += blockDim.x) out_coeffs[k] = coeffs[k];
  if (tid < 8u) {
    hdr->digest_after_coeffs[tid] = scr[16u + tid];
    hdr->digest_after_nonce[tid] = msg[tid];
    hdr->digest_end[tid] = msg[tid];   // (draws leave the digest alone)
    ch->digest[tid] = msg[tid];
  }
  if (tid == 0u) {
    ch->n_sent = n_draws;
    hdr->found = 1u;
    hdr->first_bad = st->first_bad;
    hdr->n_positions = n_positions;
    hdr->n_sent_end = n_draws;
    hdr->nonce_lo = (uint32_t)nonce;
    hdr->nonce_hi = (uint32_t)(nonce >> 32);
  }
}

void launch_fri_queries(DevChannel* ch, const FriCloseState* st, const uint32_t* coeffs, uint32_t n_coeff_words,
                        bool hashed, uint32_t n_queries, uint32_t pos_mask, uint32_t* out, lmn_stream_t s) {
  if (!ch || !st || !coeffs || !out || n_queries < 1u || n_queries > FRI_CLOSE_MAX_QUERIES)
    throw LmnError(-100, "fri_queries: bad arguments");
  LMN_LAUNCH(k_fri_queries, dim3(1), dim3(FRI_CLOSE_TPB), 0, s, ch, st, coeffs, n_coeff_words, hashed ? 1 : 0, n_queries,
             pos_mask, out);
}

#include "kernels_verify.h"   // lmn_verify_many: k_verify_values, k_verify_trees

}  // namespace lmn
