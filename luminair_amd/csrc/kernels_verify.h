// Kernels of lmn_verify_many (kernels.h "proofs verified in batches"); included by kernels_merkle.hip inside namespace lmn.
//
// The verifier's back half (verifier.cpp verify_back, a visitor of openings.h's walk) restated for a device: what the host
// walks is, for a proof that passed the front, a function of the sorted distinct query positions alone -
//   the positions of a size        = the distinct values of position >> (top - log)
//   a FRI layer's decommitment set = those, pair-expanded: 2k and 2k + 1 for every distinct k = position >> (top - log + 1)
//   a tree level's node set        = the parents of the level below merged with the level's own queries
//                                  = the positions of that size (pair-expanded at a FRI tree's column levels),
// because every query list of one proof is a fold of the same positions.  A sequential merge therefore becomes a fold
// (vm_fold_positions) and an element's place in a witness list the number of flagged lanes in front of it (vm_rank).  It
// follows that every node of a level that has columns is queried: a valid decommitment has no column witness at all,
// and one that has is rejected by its length.
// Nothing here trusts proof content: positions are masked to the domain, every witness, queried-value and leaf index is
// compared with the descriptor's length before it is used - a list that runs out, or has elements left over, is a
// recorded rejection, never an access - and every LDS index is bounded by VM_MAX_POS / VM_MAX_NODES.
// Control flow around every barrier depends on values the whole workgroup holds alike.
#pragma once

constexpr uint32_t VM_WAVE = 64;
constexpr uint32_t VM_MAX_TPB = 256;

struct VmPt {
  uint32_t x, y;
};
LMN_D VmPt vm_pt_of_index(uint32_t k) {   // host.h pt_of_index
  k &= 0x7fffffffu;
  VmPt res{1u, 0u}, cur{2u, 1268011823u};
  while (k) {
    if (k & 1u) res = VmPt{m_sub(m_mul(res.x, cur.x), m_mul(res.y, cur.y)), m_add(m_mul(res.x, cur.y), m_mul(res.y, cur.x))};
    cur = VmPt{m_sub(m_dbl(m_sqr(cur.x)), 1u), m_dbl(m_mul(cur.x, cur.y))};
    k >>= 1;
  }
  return res;
}
LMN_D uint32_t vm_bit_reverse(uint32_t i, uint32_t bits) { return bits ? __brev(i) >> (32u - bits) : 0u; }
// host.h domain_point / line_domain_x (1 <= log <= 29: the layout's sizes)
LMN_D VmPt vm_domain_point(uint32_t log, uint32_t s) {
  const uint32_t idx = vm_bit_reverse(s, log), half = 1u << (log - 1u);
  const uint32_t init = 1u << (30u - log), step = log >= 2u ? 1u << (32u - log) : 0u;
  if (idx < half) return vm_pt_of_index(init + idx * step);
  const VmPt p = vm_pt_of_index(init + (idx - half) * step);
  return VmPt{p.x, m_neg(p.y)};
}
LMN_D uint32_t vm_line_domain_x(uint32_t log, uint32_t i) {
  const uint32_t init = 1u << (29u - log), step = log >= 1u ? 1u << (31u - log) : 0u;
  return vm_pt_of_index(init + vm_bit_reverse(i, log) * step).x;
}
LMN_D QM31 vm_ldq(const uint32_t* p) { return QM31{p[0], p[1], p[2], p[3]}; }

// The number of lanes of the workgroup in front of this one whose flag is set, and the number of set flags in *total;
// every lane of the workgroup calls it (blockDim.x: a multiple of 64, at most VM_MAX_TPB).
LMN_D uint32_t vm_rank(bool flag, uint32_t* s_w, uint32_t* total) {
  const unsigned long long b = lmn_ballot(flag);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t below = (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull));
  if (blockDim.x == VM_WAVE) {   // one wave: the ballot is the whole answer
    *total = (uint32_t)__builtin_popcountll(b);
    return below;
  }
  __syncthreads();   // (the previous call's readers of s_w)
  if (lane == 0u) s_w[wave] = (uint32_t)__builtin_popcountll(b);
  __syncthreads();
  uint32_t off = 0u, tot = 0u;
  for (uint32_t w = 0; w < blockDim.x / VM_WAVE; ++w) {
    const uint32_t x = s_w[w];
    off += w < wave ? x : 0u;
    tot += x;
  }
  *total = tot;
  return off + below;
}
// fp[0 .. return) = the distinct values of pos[i] >> sh, ascending (pos: n <= VM_MAX_POS ascending values); every lane calls it
LMN_D uint32_t vm_fold_positions(const uint32_t* pos, uint32_t n, uint32_t sh, uint32_t* fp, uint32_t* s_w) {
  uint32_t np = 0u;
  __syncthreads();   // (fp's readers)
  for (uint32_t i0 = 0; i0 < n; i0 += blockDim.x) {
    const uint32_t i = i0 + threadIdx.x;
    const bool first = i < n && (i == 0u || (pos[i] >> sh) != (pos[i - 1u] >> sh));
    uint32_t tot;
    const uint32_t r = vm_rank(first, s_w, &tot);
    if (first) fp[np + r] = pos[i] >> sh;   // (its rank among at most n firsts)
    np += tot;
  }
  __syncthreads();
  return np;
}
// the OR of every lane's word; every lane calls it, lane 0's result counts
LMN_D uint32_t vm_or(uint32_t v, uint32_t* s_bad) {
  s_bad[threadIdx.x] = v;
  __syncthreads();
  uint32_t r = 0u;
  if (threadIdx.x == 0u)
    for (uint32_t k = 0; k < blockDim.x; ++k) r |= s_bad[k];
  return r;
}

// One FRI layer at its queried positions fp[0 .. np) (openings.h for_each_pair_member + the fold): the sibling pairs from the
// known values and the witness, both members' coordinate words to the layer's leaf list, the pairs' folds to out[0 ..
// return).  wi / leaf_at: the places reached in the witness (QM31s) and the leaf list (words), advanced.
LMN_D uint32_t vm_layer_pairs(const uint32_t* fp, uint32_t np, const QM31* known, const uint32_t* wit, uint32_t wit_len,
                              uint32_t& wi, uint32_t* leaves, uint32_t leaves_len, uint32_t& leaf_at, bool circle,
                              uint32_t log, QM31 alpha, QM31* out, uint32_t* s_w, uint32_t& bad) {
  uint32_t npairs = 0u, nmiss = 0u;
  for (uint32_t i0 = 0; i0 < np; i0 += VM_WAVE) {
    const uint32_t i = i0 + threadIdx.x;
    const bool first = i < np && (i == 0u || (fp[i] >> 1) != (fp[i - 1u] >> 1));
    const bool both = first && i + 1u < np && (fp[i + 1u] >> 1) == (fp[i] >> 1);
    uint32_t totp, totm;
    const uint32_t rp = vm_rank(first, s_w, &totp), rm = vm_rank(first && !both, s_w, &totm);
    if (first) {
      const uint32_t p = npairs + rp;   // < np <= VM_MAX_POS
      const QM31 own = known[i];
      QM31 other = q_zero();
      if (both) {
        other = known[i + 1u];
      } else {
        const uint32_t w = wi + nmiss + rm;
        if (w < wit_len)
          other = vm_ldq(wit + 4u * w);
        else
          bad |= VM_FAIL_WITNESS_SHORT;
      }
      const bool odd = (fp[i] & 1u) != 0u;
      const QM31 a = odd ? other : own, b = odd ? own : other;
      const uint32_t at = leaf_at + 8u * p;
      if (at + 8u <= leaves_len) {
        uint32_t* o = leaves + at;
        o[0] = a.a, o[1] = a.b, o[2] = a.c, o[3] = a.d;
        o[4] = b.a, o[5] = b.b, o[6] = b.c, o[7] = b.d;
      } else {
        bad |= VM_FAIL_POSITIONS;
      }
      const uint32_t even = fp[i] & ~1u;
      const uint32_t t = circle ? vm_domain_point(log, even).y : vm_line_domain_x(log, even);
      out[p] = q_add(q_add(a, b), q_mul(alpha, q_mul_m(q_sub(a, b), m_inv(t))));
    }
    npairs += totp;
    nmiss += totm;
  }
  wi += nmiss;
  leaf_at += 8u * npairs;
  __syncthreads();
  return npairs;
}

// One wave per proof: verifier.cpp's quotient loop, the first layer, the inner layers and the last layer.
LMN_KERNEL k_verify_values(uint32_t* blk, uint32_t layout_off, uint32_t proofs_off, uint32_t n_proofs) {
  LMN_SHARED uint32_t s_pos[VM_MAX_POS], s_fp[VM_MAX_POS];
  LMN_SHARED QM31 s_q[VM_MAX_POS];                    // a size's quotient values at its positions
  LMN_SHARED QM31 s_fold[VM_MAX_SIZES][VM_MAX_POS];   // a size's pairs folded circle to line
  LMN_SHARED QM31 s_line[2][VM_MAX_POS];              // the line layers' values, alternating
  LMN_SHARED uint32_t s_npairs[VM_MAX_SIZES];
  LMN_SHARED uint32_t s_w[VM_MAX_TPB / VM_WAVE], s_bad[VM_WAVE];
  if (blockIdx.x >= n_proofs || blockDim.x != VM_WAVE) return;
  const uint32_t lane = threadIdx.x;
  const VmLayout* L = reinterpret_cast<const VmLayout*>(blk + layout_off);
  const VmBatch* batches = reinterpret_cast<const VmBatch*>(L + 1);
  const VmProof& d = reinterpret_cast<const VmProof*>(blk + proofs_off)[blockIdx.x];
  const uint32_t n_sizes = L->n_sizes < VM_MAX_SIZES ? L->n_sizes : VM_MAX_SIZES;
  const uint32_t n_inner = L->n_inner < VM_MAX_TREES - 5u ? L->n_inner : VM_MAX_TREES - 5u;
  const VmBatchCol* bcols = reinterpret_cast<const VmBatchCol*>(batches + L->n_batches);
  const uint32_t top = L->top;
  const uint32_t n = d.pos.len < VM_MAX_POS ? d.pos.len : VM_MAX_POS;
  const uint32_t dmask = (uint32_t)((1ull << top) - 1ull);
  for (uint32_t i = lane; i < n; i += VM_WAVE) s_pos[i] = blk[d.pos.off + i] & dmask;
  const QM31 quot_alpha = vm_ldq(blk + d.alphas);
  const uint32_t* alphas = blk + d.alphas + 4u;   // the fold alphas: 1 + n_inner
  uint32_t bad = 0u;

  // ---- per size: the quotient values at the size's positions, then its pairs in the first layer
  uint32_t wi = 0u, leaf_at = 0u;
  for (uint32_t s = 0; s < n_sizes; ++s) {
    const uint32_t log = L->size_log[s];
    const uint32_t np = vm_fold_positions(s_pos, n, top - log, s_fp, s_w);
    for (uint32_t qi = lane; qi < np; qi += VM_WAVE) {
      const VmPt dp = vm_domain_point(log, s_fp[qi]);
      QM31 acc = q_zero();
      for (uint32_t b = L->size_batch0[s]; b < L->size_batch0[s + 1u]; ++b) {
        const VmBatch B = batches[b];
        const uint32_t* pw = blk + d.points + 8u * (B.point < d.n_points ? B.point : 0u);
        const QM31 px = vm_ldq(pw), py = vm_ldq(pw + 4);
        const QM31 lc = q_sub(q_conj(py), py);
        QM31 alpha = q_one(), num = q_zero();
        for (uint32_t k = B.col0; k < B.col1; ++k) {
          const VmBatchCol c = bcols[k];
          alpha = q_mul(alpha, quot_alpha);
          const VmSpan qv = d.queried[c.tree & 3u];
          const uint32_t idx = d.qbase[c.tree & 3u][c.size & (VM_MAX_SIZES - 1u)] + qi * c.ncol + c.j;
          uint32_t f = 0u;
          if (idx < qv.len)
            f = blk[qv.off + idx];
          else
            bad |= VM_FAIL_QUERIED_SHAPE;
          const QM31 val = vm_ldq(blk + d.samples + 4u * k);
          const QM31 la = q_sub(q_conj(val), val);
          const QM31 lb = q_sub(q_mul(val, lc), q_mul(la, py));
          num = q_add(num, q_mul(alpha, q_sub(q_mul_m(lc, f), q_add(q_mul_m(la, dp.y), lb))));
        }
        const CM31 dx{m_sub(px.a, dp.x), px.b}, dy{m_sub(py.a, dp.y), py.b};
        const CM31 den = c_sub(c_mul(dx, CM31{py.c, py.d}), c_mul(dy, CM31{px.c, px.d}));
        if (c_norm(den) == 0u) bad |= VM_FAIL_DENOMINATOR;
        acc = q_add(q_mul(acc, alpha), q_mul_c(num, c_inv(den)));   // (alpha: quot_alpha to the batch's column count)
      }
      s_q[qi] = acc;
    }
    __syncthreads();
    const uint32_t ai = top - log;   // the layer behind whose fold the size joins: its circle fold takes that layer's alpha
    QM31 alpha = q_zero();
    if (ai <= n_inner)
      alpha = vm_ldq(alphas + 4u * ai);
    else
      bad |= VM_FAIL_POSITIONS;
    const uint32_t npairs = vm_layer_pairs(s_fp, np, s_q, blk + d.fri_wit[0].off, d.fri_wit[0].len, wi, blk + d.leaves[0].off,
                                           d.leaves[0].len, leaf_at, true, log, alpha, s_fold[s], s_w, bad);
    if (lane == 0u) s_npairs[s] = npairs;
  }
  if (wi != d.fri_wit[0].len) bad |= VM_FAIL_WITNESS_LONG;
  if (leaf_at != d.leaves[0].len) bad |= VM_FAIL_POSITIONS;
  __syncthreads();

  // ---- the line layers
  const QM31* known = s_fold[0];
  uint32_t ncur = n_sizes ? s_npairs[0] : 0u;
  bool stop = n_sizes == 0u;
  for (uint32_t li = 0; li < n_inner && !stop; ++li) {
    const uint32_t layer_log = top - 1u - li;
    const uint32_t np = vm_fold_positions(s_pos, n, 1u + li, s_fp, s_w);
    if (np != ncur) {
      bad |= VM_FAIL_POSITIONS;
      stop = true;
      break;
    }
    QM31* out = s_line[li & 1u];
    const VmSpan w = d.fri_wit[1u + li], lv = d.leaves[1u + li];
    const QM31 alpha = vm_ldq(alphas + 4u * (li + 1u));
    uint32_t lwi = 0u, lat = 0u;
    const uint32_t npairs = vm_layer_pairs(s_fp, np, known, blk + w.off, w.len, lwi, blk + lv.off, lv.len, lat, false,
                                           layer_log, alpha, out, s_w, bad);
    if (lwi != w.len) bad |= VM_FAIL_WITNESS_LONG;
    if (lat != lv.len) bad |= VM_FAIL_POSITIONS;
    const uint32_t js = L->join_of_layer[li];
    if (js != VM_NONE) {
      if (js >= n_sizes || s_npairs[js] != npairs) {
        bad |= VM_FAIL_POSITIONS;
      } else {
        const QM31 a2 = q_mul(alpha, alpha);
        for (uint32_t p = lane; p < npairs; p += VM_WAVE) out[p] = q_add(q_mul(out[p], a2), s_fold[js][p]);
      }
      __syncthreads();
    }
    known = out;
    ncur = npairs;
  }

  // ---- the last layer: its polynomial at the remaining positions
  if (!stop) {
    const uint32_t layer_log = top - 1u - n_inner;
    const uint32_t np = vm_fold_positions(s_pos, n, 1u + n_inner, s_fp, s_w);
    if (np != ncur) bad |= VM_FAIL_POSITIONS;
    for (uint32_t i = lane; i < np && np == ncur; i += VM_WAVE) {
      const uint32_t x = vm_line_domain_x(layer_log, s_fp[i]);
      QM31 val = q_zero();
      for (uint32_t j = 0; j < d.last.len; ++j) {
        QM31 term = vm_ldq(blk + d.last.off + 4u * j);
        uint32_t xx = x;
        for (uint32_t jj = j; jj; jj >>= 1) {
          if (jj & 1u) term = q_mul_m(term, xx);
          xx = m_sub(m_dbl(m_sqr(xx)), 1u);
        }
        val = q_add(val, term);
      }
      if (!q_eq(val, known[i])) bad |= VM_FAIL_FOLDS;
    }
  }
  const uint32_t all = vm_or(bad, s_bad);
  if (lane == 0u) blk[d.verdict] = VM_DONE | all;
}

// One workgroup per (proof, tree): openings.h walk_openings, as verifier.cpp replays it, from the deepest level to the root.
LMN_KERNEL k_verify_trees(uint32_t* blk, uint32_t layout_off, uint32_t proofs_off, uint32_t n_proofs, uint32_t n_trees) {
  LMN_SHARED uint32_t s_pos[VM_MAX_POS], s_fp[VM_MAX_POS];
  LMN_SHARED uint32_t s_set[2][VM_MAX_NODES];        // the previous and the current level's nodes, ascending
  LMN_SHARED uint32_t s_hash[2][VM_MAX_NODES * 8];   // and their hashes
  LMN_SHARED uint32_t s_w[VM_MAX_TPB / VM_WAVE], s_bad[VM_MAX_TPB];
  const uint32_t t = blockIdx.x, tid = threadIdx.x, tpb = blockDim.x;
  if (blockIdx.y >= n_proofs || t >= n_trees || t >= VM_MAX_TREES || tpb > VM_MAX_TPB || tpb % VM_WAVE) return;
  const VmLayout* L = reinterpret_cast<const VmLayout*>(blk + layout_off);
  const VmProof& d = reinterpret_cast<const VmProof*>(blk + proofs_off)[blockIdx.y];
  const bool fri = t >= 4u;
  const VmSpan q = fri ? d.leaves[t - 4u] : d.queried[t];
  const VmSpan hw = d.hash_wit[t], cw = d.col_wit[t];
  const uint32_t* root = blk + d.roots + 8u * t;
  uint32_t* verdict = blk + d.verdict + 1u + t;
  const uint32_t max_log = L->tree_max_log[t], top = L->top;
  if (max_log == VM_NONE) {   // a tree without columns: the hash of the empty message, and three empty lists
    if (tid == 0u) {
      uint32_t h[8], m[16];
      b2_init(h);
#pragma unroll
      for (int k = 0; k < 16; ++k) m[k] = 0u;
      b2_compress(h, m, 0u, 0xffffffffu);
      bool ok = q.len == 0u && hw.len == 0u && cw.len == 0u;
#pragma unroll
      for (int k = 0; k < 8; ++k) ok = ok && h[k] == root[k];
      *verdict = VM_DONE | (ok ? 0u : VM_FAIL_TREE);
    }
    return;
  }
  const uint32_t n = d.pos.len < VM_MAX_POS ? d.pos.len : VM_MAX_POS;
  const uint32_t dmask = (uint32_t)((1ull << top) - 1ull);
  for (uint32_t i = tid; i < n; i += tpb) s_pos[i] = blk[d.pos.off + i] & dmask;
  uint32_t bad = max_log > 31u || max_log > top ? VM_FAIL_TREE : 0u;
  uint32_t hi = 0u, qi = 0u, nprev = 0u, cur = 0u;
  for (int log = bad ? -1 : (int)max_log; log >= 0; --log) {
    const uint32_t nc = L->tree_ncols[t][log];
    const bool expand = fri && nc != 0u;   // a FRI layer is opened in sibling pairs
    if (expand && log == 0) {
      bad |= VM_FAIL_TREE;
      break;
    }
    const uint32_t nk = vm_fold_positions(s_pos, n, top - (uint32_t)log + (expand ? 1u : 0u), s_fp, s_w);
    const uint32_t ncur = expand ? 2u * nk : nk;   // <= VM_MAX_NODES
    uint32_t* set = s_set[cur];
    const uint32_t* prev = s_set[cur ^ 1u];
    uint32_t* hcur = s_hash[cur];
    const uint32_t* hprev = s_hash[cur ^ 1u];
    for (uint32_t i = tid; i < ncur; i += tpb) set[i] = expand ? 2u * s_fp[i >> 1] + (i & 1u) : s_fp[i];
    __syncthreads();
    const bool have = log < (int)max_log;   // the level has children
    const uint32_t npre = have ? 16u : 0u, nw = npre + nc, nblk = nw ? (nw + 15u) / 16u : 1u;
    uint32_t miss = 0u;
    for (uint32_t i0 = 0; i0 < ncur; i0 += tpb) {
      const uint32_t i = i0 + tid;
      const bool active = i < ncur;
      uint32_t li = VM_NONE, ri = VM_NONE;   // the children's places in the previous set
      bool lm = false, rm = false;           // or their absence: the hash comes from the witness
      if (active && have) {
        const uint32_t v = set[i];
        uint32_t lb = open_lb(prev, nprev, 2u * v);
        if (lb < nprev && prev[lb] == 2u * v)
          li = lb++;
        else
          lm = true;
        if (lb < nprev && prev[lb] == 2u * v + 1u)
          ri = lb;
        else
          rm = true;
      }
      uint32_t tl, tr;
      const uint32_t rl = vm_rank(lm, s_w, &tl), rr = vm_rank(rm, s_w, &tr);
      if (active) {
        const uint32_t hl = hi + miss + rl + rr, hr = hl + (lm ? 1u : 0u);   // witness hashes: node by node, left then right
        uint32_t pre[16];   // the children's hashes: from the previous level, or from the witness
#pragma unroll
        for (int k = 0; k < 16; ++k) pre[k] = 0u;
        if (have) {
          if (li != VM_NONE) {
#pragma unroll
            for (int k = 0; k < 8; ++k) pre[k] = hprev[li * 8u + k];
          } else if (hl < hw.len) {
#pragma unroll
            for (int k = 0; k < 8; ++k) pre[k] = blk[hw.off + hl * 8u + k];
          } else {
            bad |= VM_FAIL_TREE;
          }
          if (ri != VM_NONE) {
#pragma unroll
            for (int k = 0; k < 8; ++k) pre[8 + k] = hprev[ri * 8u + k];
          } else if (hr < hw.len) {
#pragma unroll
            for (int k = 0; k < 8; ++k) pre[8 + k] = blk[hw.off + hr * 8u + k];
          } else {
            bad |= VM_FAIL_TREE;
          }
        }
        const uint32_t q0 = qi + i * nc;   // every node of a level with columns is queried: its words follow each other
        uint32_t h[8];
        b2_init(h);
        for (uint32_t b = 0; b < nblk; ++b) {
          uint32_t m[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const uint32_t w = 16u * b + (uint32_t)k;
            uint32_t v = b == 0u ? pre[k] : 0u;
            if (w >= npre && w < nw) {
              const uint32_t qx = q0 + (w - npre);
              if (qx < q.len)
                v = blk[q.off + qx];
              else
                bad |= VM_FAIL_TREE;
            }
            m[k] = v;
          }
          const bool last = b + 1u == nblk;
          b2_compress(h, m, last ? 4u * nw : 64u * (b + 1u), last ? 0xffffffffu : 0u);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) hcur[i * 8u + k] = h[k];
      }
      miss += tl + tr;
    }
    hi += miss;
    qi += ncur * nc;
    nprev = ncur;
    cur ^= 1u;
    __syncthreads();
  }
  if (nprev != 1u || hi != hw.len || qi != q.len || cw.len != 0u) bad |= VM_FAIL_TREE;
  if (tid == 0u && !bad) {
    const uint32_t* h = s_hash[cur ^ 1u];
    for (int k = 0; k < 8; ++k)
      if (h[k] != root[k]) bad |= VM_FAIL_TREE;
  }
  const uint32_t all = vm_or(bad, s_bad);
  if (tid == 0u) *verdict = VM_DONE | all;
}

void launch_verify_values(uint32_t* blk, uint32_t layout_off, uint32_t proofs_off, uint32_t n_proofs, lmn_stream_t s,
                          uint64_t* n_launched) {
  if (!blk || n_proofs == 0) throw LmnError(-100, "verify_values: bad arguments");
  LMN_LAUNCH(k_verify_values, dim3(n_proofs), dim3(VM_WAVE), 0, s, blk, layout_off, proofs_off, n_proofs);
  if (n_launched) ++*n_launched;
}
void launch_verify_trees(uint32_t* blk, uint32_t layout_off, uint32_t proofs_off, uint32_t n_proofs, uint32_t n_trees,
                         uint32_t tpb, lmn_stream_t s, uint64_t* n_launched) {
  if (!blk || n_proofs == 0 || n_proofs > 65535u || n_trees == 0 || n_trees > VM_MAX_TREES ||
      (tpb != 64u && tpb != 128u && tpb != 256u))
    throw LmnError(-100, "verify_trees: bad arguments");
  LMN_LAUNCH(k_verify_trees, dim3(n_trees, n_proofs), dim3(tpb), 0, s, blk, layout_off, proofs_off, n_proofs, n_trees);
  if (n_launched) ++*n_launched;
}
