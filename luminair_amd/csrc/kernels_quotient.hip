// gfx950 kernels, part 5: constraint quotients of all 17 components, point evaluation, FRI quotients and folds
// (SURVEY.md section 8a rows a7, a9).
#include "kernels_common.h"
#include "constraints.h"

namespace lmn {

// =============================================================================================
// a7  Constraint quotients (composition polynomial) on the eval domain
// =============================================================================================
// storage index of the point p_s - 2^(eval_log - log_size) coset steps (mask offset -1)
LMN_D uint32_t prev_row_storage(uint32_t s, int eval_log, int log_size) {
  const int hb = eval_log - 1;
  const uint32_t low = s & 1u;
  uint32_t t = s >> 1;
  if (hb == 0) return s;
  const uint32_t mask = (1u << hb) - 1u;
  const uint32_t d = 1u << (eval_log - log_size - 1);
  uint32_t j = __brev(t) >> (32 - hb);
  j = (low ? j + d : j - d) & mask;
  t = __brev(j) >> (32 - hb);
  return (t << 1) | low;
}

// sum_k coeff[k] * constraint_k, accumulated lazily (QAcc: one v_mad_u64_u32 per coordinate for the
// M31-valued local constraints, folded every third term; k is compile-time after unrolling)
struct ConsAcc {
  QAcc acc;
  const QM31* coeff;
  int k;
  LMN_HD void bump() {
    ++k;
    if (k % 3 == 0) qacc_fold(acc);
  }
  LMN_HD void add_m(uint32_t c) {
    qacc_mad(acc, coeff[k], c);
    bump();
  }
  LMN_HD void add_q(QM31 c) {
    const QM31 t = q_mul(coeff[k], c);
    acc.a += t.a;
    acc.b += t.b;
    acc.c += t.c;
    acc.d += t.d;
    bump();
  }
};

// logup constraints for NREL relations; values are passed by value (no indexed private arrays:
// those get promoted to LDS and cost occupancy).  rc[j]: 0 = NodeElements (z, alpha); 1 = width-1
// LUT relation val - z2 (range check); 2 = width-2 LUT relation val + alpha2*id - z2 (sin/exp2/log2).
// neg: numerator is -mult.
struct CompElems {
  QM31 z, alpha, z2, alpha2;
};
template <int NREL>
LMN_D void logup_constraints(ConsAcc& ca, const CompositionArgs& a, const CompElems& ce, const uint32_t (&mult)[NREL],
                             const uint32_t (&val)[NREL], const uint32_t (&id)[NREL], const int (&rc)[NREL], bool neg,
                             uint32_t s, uint32_t t, uint64_t E) {
  QM31 prev = q_zero();
#pragma unroll
  for (int j = 0; j < NREL; ++j) {
    QM31 cur = load_secure_ub(a.inter + (uint64_t)(4 * j) * a.stride, a.stride, t);
    QM31 den = rc[j] == 1   ? q_sub(q_from_m(val[j]), ce.z2)
               : rc[j] == 2 ? q_sub(q_add_m(q_mul_m(ce.alpha2, id[j]), val[j]), ce.z2)
                            : q_sub(q_add_m(q_mul_m(ce.alpha, id[j]), val[j]), ce.z);
    QM31 diff;
    if (j < NREL - 1) {
      diff = q_sub(cur, prev);
    } else {
      uint32_t ps = prev_row_storage(s, a.eval_log, a.log_size);
      QM31 pr = load_secure_ub(a.prev_last, E, ps);
      diff = q_add(q_sub(q_sub(cur, pr), prev), a.claimed_shift[1]);
    }
    ca.add_q(q_sub_m(q_mul(diff, den), neg ? m_neg(mult[j]) : mult[j]));
    prev = cur;
  }
}

template <int KIND>
LMN_KERNEL k_composition(CompositionArgs a) {
  const uint64_t E = 1ull << a.eval_log;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;  // row inside the block handled by this launch
  if (t >= a.n_rows) return;
  const uint32_t s = a.row0 + t;                             // storage index on the whole eval domain
  // coefficients and relation elements: kernel arguments, or what the device-resident channel left in memory
  ConsAcc ca{qacc_zero(), a.d_coeff ? a.d_coeff : a.coeff, 0};
  const CompElems ce = a.d_elems ? CompElems{a.d_elems->z[0], a.d_elems->alpha[0], a.d_elems->z[a.es2], a.d_elems->alpha[a.es2]}
                                 : CompElems{a.z, a.alpha, a.z2, a.alpha2};
  const uint32_t* __restrict__ mn = a.main;   // wave-uniform column bases, the row as a 32-bit lane offset (ld_ub)
  const uint64_t cstride = a.stride;
  // the row in registers (compile-time indices only), its local constraints (constraints.h), then the relations as the
  // component's table entry wires them: main columns, or the preprocessed LUT columns of a lookup component
  constexpr ComponentSpec sp = kSpecs[KIND];
  constexpr int NC = sp.n_cols, NR = sp.n_rel;
  uint32_t c[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) c[k] = ld_col(mn, k, cstride, t);
  local_constraints<KIND>(c, [&](uint32_t v) { ca.add_m(v); });
  uint32_t rm[NR], rv[NR], ri[NR];
  int rc[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    rm[j] = c[sp.rel_mult[j]];
    if (sp.rel_pre[j]) {
      rv[j] = ld_ub(sp.rel_val[j] ? a.pre2 : a.pre, t);
      ri[j] = sp.rel_id[j] < 0 ? 0u : ld_ub(sp.rel_id[j] ? a.pre2 : a.pre, t);
    } else {
      rv[j] = c[sp.rel_val[j]];
      ri[j] = sp.rel_id[j] < 0 ? 0u : c[sp.rel_id[j]];
    }
    rc[j] = sp.rel_elems[j] == ELEMS_NODE ? 0 : sp.rel_id[j] < 0 ? 1 : 2;   // NodeElements / width-1 LUT / width-2 LUT
  }
  logup_constraints<NR>(ca, a, ce, rm, rv, ri, rc, sp.rel_neg[0] != 0, s, t, E);
  QM31 r = q_mul_m(qacc_reduce(ca.acc), a.zinv[(s >> a.log_size) & 1u]);
  if (a.accumulate) {
    r.a = m_add(r.a, ld_ub(a.out, s));
    r.b = m_add(r.b, ld_ub(a.out + E, s));
    r.c = m_add(r.c, ld_ub(a.out + 2 * E, s));
    r.d = m_add(r.d, ld_ub(a.out + 3 * E, s));
  }
  st_ub(a.out, s, r.a);
  st_ub(a.out + E, s, r.b);
  st_ub(a.out + 2 * E, s, r.c);
  st_ub(a.out + 3 * E, s, r.d);
}

void launch_composition(const CompositionArgs& a, lmn_stream_t s) {
  if (a.eval_log != a.log_size + 1) throw LmnError(-100, "composition: eval domain must be log_size+1");
  if (a.n_rows == 0 || (uint64_t)a.row0 + a.n_rows > (1ull << a.eval_log) || a.stride < a.n_rows || !a.prev_last)
    throw LmnError(-100, "composition: bad row block");
  dim3 g(cdiv(a.n_rows, TPB)), b(TPB);
#define LMN_COMP_CASE(K) case K: LMN_LAUNCH(k_composition<K>, g, b, 0, s, a); break;
  switch (composition_shape(a.kind)) {   // one instantiation per shape: Exp2 / Log2 run Sin's, their lookups SinLookup's
    LMN_COMP_CASE(0) LMN_COMP_CASE(1) LMN_COMP_CASE(2) LMN_COMP_CASE(3) LMN_COMP_CASE(4) LMN_COMP_CASE(5) LMN_COMP_CASE(6)
    LMN_COMP_CASE(7) LMN_COMP_CASE(8) LMN_COMP_CASE(13) LMN_COMP_CASE(14) LMN_COMP_CASE(15) LMN_COMP_CASE(16)
    default: throw LmnError(-100, "composition: unsupported component kind");
  }
#undef LMN_COMP_CASE
}

LMN_KERNEL k_secure_add(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = m_add(out[i], in[i]);
}
void launch_secure_add(uint32_t* out, const uint32_t* in, uint64_t n_words, lmn_stream_t s) {
  LMN_LAUNCH(k_secure_add, dim3(cdiv(n_words, TPB)), dim3(TPB), 0, s, out, in, n_words);
}

LMN_KERNEL k_add_cols(uint32_t* __restrict__ out, uint64_t out_stride, const uint32_t* __restrict__ in, uint64_t in_stride,
                      uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t* o = out + (uint64_t)blockIdx.y * out_stride + i;
  *o = m_add(*o, in[(uint64_t)blockIdx.y * in_stride + i]);
}
void launch_add_cols(uint32_t* out, uint64_t out_stride, const uint32_t* in, uint64_t in_stride, uint64_t n, int ncols,
                     lmn_stream_t s) {
  LMN_LAUNCH(k_add_cols, dim3(cdiv(n, TPB), (unsigned)ncols), dim3(TPB), 0, s, out, out_stride, in, in_stride, n);
}

// ---- the composition polynomial from half of its evaluation domain (kernels.h CompHalfFix)
// prod_k m[k0 + k]^(bit k of v), k < nbits
LMN_D uint32_t probe_basis(const ProbeMaps& pm, uint32_t v, int k0, int nbits) {
  uint32_t acc = 1u;
  for (int k = 0; k < nbits; ++k)
    if ((v >> k) & 1u) acc = m_mul(acc, pm.m[k0 + k]);
  return acc;
}
// sum of the block's values (every lane calls; valid in every lane)
LMN_D uint32_t probe_block_sum(uint32_t* red, uint32_t v) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int st = TPB / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] = m_add(red[threadIdx.x], red[threadIdx.x + st]);
    __syncthreads();
  }
  const uint32_t r = red[0];
  __syncthreads();
  return r;
}
// An M31 point's basis value of coefficient j factors over the bits of j: lane bits [0, 8) once per lane, bits [8, 12) per
// coefficient of the lane, bits [12, log_n) once per block.
LMN_KERNEL k_probe_dot(const uint32_t* __restrict__ coeffs, uint64_t stride, int log_n, ProbeMaps pm,
                       uint32_t* __restrict__ partial, uint32_t* __restrict__ tail_out) {
  LMN_SHARED uint32_t red[TPB];
  const uint32_t* __restrict__ col = coeffs + (uint64_t)blockIdx.y * stride;
  const uint64_t n = 1ull << log_n;
  const uint64_t j0 = (uint64_t)blockIdx.x << PROBE_CHUNK_LOG;
  const int lane_bits = log_n < 8 ? log_n : 8;
  const int mid_bits = log_n < PROBE_CHUNK_LOG ? (log_n > 8 ? log_n - 8 : 0) : PROBE_CHUNK_LOG - 8;
  uint32_t acc = 0u;
  for (uint32_t i = 0; i < (1u << mid_bits); ++i) {
    const uint64_t j = j0 + ((uint64_t)i << 8) + threadIdx.x;
    if (threadIdx.x < (1u << lane_bits) && j < n) acc = m_add(acc, m_mul(col[j], probe_basis(pm, i, 8, mid_bits)));
  }
  acc = m_mul(acc, probe_basis(pm, threadIdx.x, 0, lane_bits));
  if (log_n > PROBE_CHUNK_LOG) acc = m_mul(acc, probe_basis(pm, blockIdx.x, PROBE_CHUNK_LOG, log_n - PROBE_CHUNK_LOG));
  const uint32_t sum = probe_block_sum(red, acc);
  if (threadIdx.x == 0) {
    partial[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
    if (tail_out && blockIdx.x == 0) tail_out[blockIdx.y] = col[n];
  }
}
void launch_probe_dot(const uint32_t* coeffs, uint64_t stride, int log_n, const ProbeMaps& pm, uint32_t* partial,
                      uint32_t* tail_out, lmn_stream_t s) {
  if (log_n < 0 || log_n >= MAX_LOG) throw LmnError(-100, "probe_dot: bad size");
  LMN_LAUNCH(k_probe_dot, dim3(probe_dot_blocks(log_n), 4), dim3(TPB), 0, s, coeffs, stride, log_n, pm, partial, tail_out);
}

LMN_KERNEL k_comp_half_fix(CompHalfFix f) {
  LMN_SHARED uint32_t red[TPB];
  const uint32_t c4 = blockIdx.y;
  uint32_t acc = 0u;
  for (uint32_t k = threadIdx.x; k < f.n_g; k += blockDim.x) acc = m_add(acc, f.part_g[(uint64_t)c4 * f.n_g + k]);
  for (uint32_t k = threadIdx.x; k < f.n_f; k += blockDim.x) acc = m_sub(acc, f.part_f[(uint64_t)c4 * f.n_f + k]);
  // g(probe) - p(probe), p = this size's quotients + the folded polynomial: every lane gets the sum
  const uint32_t diff = m_sub(probe_block_sum(red, acc), f.probe[c4]);
  const uint32_t w = f.w_top[0];
  const uint32_t c = m_mul(diff, m_inv(m_add(w, w)));
  const uint64_t N = 1ull << f.log_half;
  uint32_t* __restrict__ col = f.coeffs + (uint64_t)c4 * f.coeff_stride;
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, gstep = (uint64_t)gridDim.x * blockDim.x;
  if (gid == 0) col[0] = m_sub(col[0], m_mul(w, c));
  for (uint64_t i = gid; i < N; i += gstep) col[N + i] = i == 0 ? c : 0u;
  if (f.lde) {
    uint32_t* __restrict__ l = f.lde + (uint64_t)c4 * f.lde_stride;
    const uint64_t per = N >> 12;   // words of a quarter that element 0 has spread to
    for (uint64_t i = gid; i < 4 * per; i += gstep) {
      const uint32_t h = (uint32_t)(i / per);
      const uint32_t we = f.w_ext[h >> 1];
      const uint32_t kappa = m_sub((h & 1u) ? m_neg(we) : we, w);
      uint32_t* p = l + (uint64_t)h * N + ((i % per) << 12);
      *p = m_add(*p, m_mul(c, kappa));
    }
  }
}
void launch_comp_half_fix(const CompHalfFix& f, lmn_stream_t s) {
  if (f.log_half < 0 || (f.lde && f.log_half < 12)) throw LmnError(-100, "comp_half_fix: bad size");
  const uint64_t N = 1ull << f.log_half;
  const unsigned gx = (unsigned)std::min<uint64_t>(std::max<uint64_t>(N / (4 * TPB), 1), 256);
  LMN_LAUNCH(k_comp_half_fix, dim3(gx, 4), dim3(TPB), 0, s, f);
}

// =============================================================================================
// a9  eval_at_point: sum_j coeff_j * basis_j(point), basis factored as lo-table x hi-table
// =============================================================================================
constexpr int EVAL_HI_PER_CHUNK = 8;
LMN_HD int eval_num_chunks_hd(int log_n) {
  if (log_n <= EVAL_LB) return 1;
  int total_hi = 1 << (log_n - EVAL_LB);
  int hpc = total_hi < EVAL_HI_PER_CHUNK ? total_hi : EVAL_HI_PER_CHUNK;
  return total_hi / hpc;
}
int eval_num_chunks(int log_n) { return eval_num_chunks_hd(log_n); }

// shard_world > 1 (single-proof sharding): the chunks of every job are dealt to the ranks in contiguous runs (a job
// with fewer chunks than ranks gives one chunk to each of the first ranks); a rank writes zero for chunks it does
// not own, so that the per-job reduction is this rank's PARTIAL sum - the ranks' partials are all-gathered (16 B per
// job and rank) and added on the host.
LMN_KERNEL k_eval_at_point(const EvalJob* __restrict__ jobs, const QM31* __restrict__ lo_tab,
                           const QM31* __restrict__ hi_tab, uint32_t hi_stride, QM31* __restrict__ partial_out,
                           int max_chunks, uint32_t shard_rank, uint32_t shard_world) {
  LMN_SHARED QM31 red[TPB];
  const EvalJob job = jobs[blockIdx.y];
  const int chunk = blockIdx.x;
  const int nchunks = eval_num_chunks_hd(job.log_n);
  if (chunk >= nchunks) return;
  if (shard_world > 1) {
    // job.owner >= 0: the coefficients exist on that rank only, which evaluates every chunk
    const uint32_t owner = job.owner >= 0 ? (uint32_t)job.owner
                           : (uint32_t)nchunks >= shard_world ? (uint32_t)chunk / ((uint32_t)nchunks / shard_world) : (uint32_t)chunk;
    if (owner != shard_rank) {
      if (threadIdx.x == 0) partial_out[(uint64_t)blockIdx.y * max_chunks + chunk] = q_zero();
      return;
    }
  }
  const int lb = job.log_n < EVAL_LB ? job.log_n : EVAL_LB;
  const uint32_t lo_n = 1u << lb;
  const uint32_t total_hi = 1u << (job.log_n - lb);
  const uint32_t hpc = total_hi / (uint32_t)nchunks;
  const QM31* L = lo_tab + ((uint64_t)job.point << EVAL_LB);
  const QM31* Hh = hi_tab + (uint64_t)job.point * hi_stride;
  // each lane owns at most 4 lo positions (tid + 256k): keep their basis values in registers
  QM31 Lr[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t lo = threadIdx.x + (uint32_t)k * TPB;
    Lr[k] = lo < lo_n ? L[lo] : q_zero();
  }
  // sum_hi H[hi] * (sum_lo L[lo] * c[hi, lo]) regrouped as sum_lo L[lo] * (sum_hi H[hi] * c[hi, lo]): the
  // inner sums are QM31 (wave-uniform H) x M31 products, accumulated lazily in 64-bit lanes; one full
  // QM31 product per owned lo position closes the chunk.
  QAcc in0 = qacc_zero(), in1 = qacc_zero(), in2 = qacc_zero(), in3 = qacc_zero();
  uint32_t pending = 0;
  // a chunk is at most EVAL_HI_PER_CHUNK runs of coefficients: all their loads are issued before the first product
  uint32_t cv[EVAL_HI_PER_CHUNK][4];
  QM31 Hv[EVAL_HI_PER_CHUNK];
#pragma unroll
  for (uint32_t hh = 0; hh < (uint32_t)EVAL_HI_PER_CHUNK; ++hh) {
    const uint32_t hi = chunk * hpc + hh;
    const uint32_t* __restrict__ cp = job.coeffs + ((uint64_t)hi << lb);
    Hv[hh] = hh < hpc ? Hh[hi] : q_zero();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t lo = threadIdx.x + (uint32_t)k * TPB;
      cv[hh][k] = (hh < hpc && lo < lo_n) ? ld_ub(cp, lo) : 0u;   // (block-uniform run of coefficients: kernels_common.h)
    }
  }
#pragma unroll
  for (uint32_t hh = 0; hh < (uint32_t)EVAL_HI_PER_CHUNK; ++hh) {
    if (hh >= hpc) break;
    qacc_mad(in0, Hv[hh], cv[hh][0]);
    qacc_mad(in1, Hv[hh], cv[hh][1]);
    qacc_mad(in2, Hv[hh], cv[hh][2]);
    qacc_mad(in3, Hv[hh], cv[hh][3]);
    if (++pending == 3) {
      pending = 0;
      qacc_fold(in0);
      qacc_fold(in1);
      qacc_fold(in2);
      qacc_fold(in3);
    }
  }
  QM31 acc = q_mul(Lr[0], qacc_reduce(in0));
  acc = q_add(acc, q_mul(Lr[1], qacc_reduce(in1)));
  acc = q_add(acc, q_mul(Lr[2], qacc_reduce(in2)));
  acc = q_add(acc, q_mul(Lr[3], qacc_reduce(in3)));
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int st = TPB / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] = q_add(red[threadIdx.x], red[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial_out[(uint64_t)blockIdx.y * max_chunks + chunk] = red[0];
}

void launch_eval_at_point(const EvalJob* jobs, int njobs, const QM31* lo_tab, const QM31* hi_tab, uint32_t hi_stride,
                          int max_log, QM31* partial_out, int max_chunks, lmn_stream_t s, uint32_t shard_rank,
                          uint32_t shard_world) {
  (void)max_log;
  LMN_LAUNCH(k_eval_at_point, dim3(max_chunks, njobs), dim3(TPB), 0, s, jobs, lo_tab, hi_tab, hi_stride, partial_out,
             max_chunks, shard_rank, shard_world);
}

// basis tables on the device: lo[p][j] = prod_{k<EVAL_LB} maps[p][k]^(bit k of j); hi[p][j] likewise
// with maps[p][EVAL_LB + k].  maps = [y, x, pi(x), pi^2(x), ...] per sample point.
LMN_KERNEL k_eval_tables(const QM31* __restrict__ maps, int maps_stride, QM31* __restrict__ lo_tab,
                         QM31* __restrict__ hi_tab, uint32_t hi_n, int hi_bits) {
  const int p = blockIdx.y;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const QM31* mp = maps + (uint64_t)p * maps_stride;
  const uint32_t lo_n = 1u << EVAL_LB;
  if (j < lo_n) {
    QM31 acc = q_one();
    for (int k = 0; k < EVAL_LB; ++k)
      if ((j >> k) & 1u) acc = q_mul(acc, mp[k]);
    lo_tab[(uint64_t)p * lo_n + j] = acc;
  }
  if (j < hi_n) {
    QM31 acc = q_one();
    for (int k = 0; k < hi_bits; ++k)
      if ((j >> k) & 1u) acc = q_mul(acc, mp[EVAL_LB + k]);
    hi_tab[(uint64_t)p * hi_n + j] = acc;
  }
}

void launch_eval_tables(const QM31* maps, int maps_stride, int npoints, QM31* lo_tab, QM31* hi_tab, uint32_t hi_n,
                        int hi_bits, lmn_stream_t s) {
  uint32_t n = hi_n > (1u << EVAL_LB) ? hi_n : (1u << EVAL_LB);
  LMN_LAUNCH(k_eval_tables, dim3(cdiv(n, TPB), npoints), dim3(TPB), 0, s, maps, maps_stride, lo_tab, hi_tab, hi_n,
             hi_bits);
}

// out[job] = sum over that job's chunks of partial[job][chunk]
LMN_KERNEL k_eval_reduce(const EvalJob* __restrict__ jobs, const QM31* __restrict__ partial, int max_chunks,
                         QM31* __restrict__ out) {
  LMN_SHARED QM31 red[TPB];
  const int job = blockIdx.x;
  const int nc = eval_num_chunks_hd(jobs[job].log_n);
  QM31 acc = q_zero();
  for (int c = threadIdx.x; c < nc; c += blockDim.x) acc = q_add(acc, partial[(uint64_t)job * max_chunks + c]);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int st = TPB / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] = q_add(red[threadIdx.x], red[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[job] = red[0];
}

void launch_eval_reduce(const EvalJob* jobs, int njobs, const QM31* partial, int max_chunks, QM31* out,
                        lmn_stream_t s) {
  LMN_LAUNCH(k_eval_reduce, dim3(njobs), dim3(TPB), 0, s, jobs, partial, max_chunks, out);
}

// =============================================================================================
// a9  FRI quotients: row = sum_batches [ row*alpha^|batch| + (sum_cols c*f(q) - (A*q.y + B)) / den ]
// =============================================================================================
LMN_HD uint32_t domain_x(const uint32_t* tw_x, uint32_t s) {
  uint32_t x = tw_x[s >> 2];
  return (s & 2u) ? m_neg(x) : x;
}
LMN_HD uint32_t domain_y(const uint32_t* tw_y, uint32_t s) {
  uint32_t y = tw_y[s >> 1];
  return (s & 1u) ? m_neg(y) : y;
}

// NB = number of sample-point batches (compile-time: exact loops, no dummy products); every lane owns
// QUOT_ROWS rows a quarter of the domain apart and inverts all their denominator norms with ONE field
// inversion (Montgomery batching: 3 products per element instead of a 37-product exponentiation per row).
// Rows per lane: 4 for one batch, 2 for two batches (the headline shape) - with the register budget of 8 waves per SIMD
// (64 VGPRs, no spills) those two launches fill the chip in whole rounds (16 waves per SIMD in two rounds of 8; at 87
// VGPRs the 8 waves per SIMD of the two-batch launch ran as 5 + 3): 0.167 -> 0.150 ms per proof, + 2 % proofs/s.
// Three and four batches keep 4 rows at the compiler's own budget (they would spill at 64).
template <int NB>
constexpr int quot_rows() { return NB == 2 ? 2 : 4; }   // rows per lane
template <int NB>
LMN_D void quotients_body(const QuotientArgs& a);
template <int NB>
LMN_KERNEL k_quotients(QuotientArgs a) { quotients_body<NB>(a); }
#if !defined(LMN_EMU) && !defined(LMN_BATCH)
template <int NB>
__attribute__((amdgpu_waves_per_eu(8, 8))) LMN_KERNEL k_quotients_occ(QuotientArgs a) { quotients_body<NB>(a); }
#else
template <int NB>
LMN_KERNEL k_quotients_occ(QuotientArgs a) { quotients_body<NB>(a); }
#endif
template <int NB>
LMN_D void quotients_body(const QuotientArgs& a) {
  constexpr int QUOT_ROWS = quot_rows<NB>();
#if defined(LMN_EMU) || !defined(__HIP_DEVICE_COMPILE__)
  // (column pointer, alpha^k * c) table staged once per block in LDS: the per-column loop then
  // reads wave-uniform LDS words instead of chasing pointers through global memory
  LMN_SHARED QuotEntry tab[QUOT_MAX_ENTRIES];
  const int nent = a.batch_start[NB];
  for (int e = threadIdx.x; e < nent; e += blockDim.x) tab[e] = a.entries[e];
  __syncthreads();
#define LMN_QCOL(e, row) tab[e].col[row]
#else
#define LMN_QCOL(e, row) ld_ub(tab[e].col, row)
  // The (column pointer, alpha^k * c) table is read through the SCALAR cache (constant address space: nothing writes it
  // during the launch): a column's base address and its coefficient arrive in SGPRs, so the column load takes an SGPR
  // base + the row as a 32-bit lane offset (no 64-bit vector address per load, one v_lshl_add_u64 of ~10 instructions per
  // column and row before) and the multiply-accumulates take the coefficient as their scalar operand; the LDS copy of
  // the table (a ds_read_b64 + ds_read_b128 per column and row group) is gone.
  typedef const QuotEntry __attribute__((address_space(4))) * ConstTab;
  const ConstTab tab = (ConstTab)(uintptr_t)a.entries;
#endif
#if defined(LMN_EMU) || !defined(__HIP_DEVICE_COMPILE__)
  const QuotDev& qd = *a.dev;
#else
  // (the same for the batches' sums and points: written before this launch, never during it)
  const QuotDev __attribute__((address_space(4)))& qd = *(const QuotDev __attribute__((address_space(4)))*)(uintptr_t)a.dev;
#endif
  const uint32_t Q = (1u << a.log_rows) / QUOT_ROWS;
  const uint32_t s0 = blockIdx.x * blockDim.x + threadIdx.x;  // row inside the block handled by this launch
  if (s0 >= Q) return;
  constexpr int NE = QUOT_ROWS * NB;
  CM31 den[NE];
  uint32_t nrm[NE], pre[NE], ys[QUOT_ROWS];
#pragma unroll
  for (int k = 0; k < QUOT_ROWS; ++k) {
    const uint32_t s = a.row0 + s0 + (uint32_t)k * Q;  // storage index on the whole domain
    const uint32_t x = a.log_size >= 2 ? domain_x(a.tw_x, s) : 0u;
    const uint32_t y = domain_y(a.tw_y, s);
    ys[k] = y;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int e = k * NB + b;
      CM31 dx{m_sub(qd.prx[b].a, x), qd.prx[b].b};
      CM31 dy{m_sub(qd.pry[b].a, y), qd.pry[b].b};
      den[e] = c_sub(c_mul(dx, CM31{qd.piy[b].a, qd.piy[b].b}), c_mul(dy, CM31{qd.pix[b].a, qd.pix[b].b}));
      nrm[e] = c_norm(den[e]);
      pre[e] = e == 0 ? nrm[e] : m_mul(pre[e - 1], nrm[e]);
    }
  }
  uint32_t inv = m_inv(pre[NE - 1]);
  CM31 dinv[NE];
#pragma unroll
  for (int e = NE - 1; e >= 0; --e) {
    const uint32_t ni = e == 0 ? inv : m_mul(inv, pre[e - 1]);
    inv = m_mul(inv, nrm[e]);
    dinv[e] = CM31{m_mul(den[e].a, ni), m_mul(m_neg(den[e].b), ni)};
  }
#pragma unroll
  for (int k = 0; k < QUOT_ROWS; ++k) {
    const uint32_t s = s0 + (uint32_t)k * Q;
    QM31 row = q_zero();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      // sum_k c_k * f_k(s) accumulated lazily in 64-bit lanes (three products per fold)
      QAcc acc = qacc_zero();
      const int k1 = a.batch_start[b + 1];
      int kk = a.batch_start[b];
      for (; kk + 6 <= k1; kk += 6) {
        uint32_t f0 = LMN_QCOL(kk, s), f1 = LMN_QCOL(kk + 1, s), f2 = LMN_QCOL(kk + 2, s);
        uint32_t f3 = LMN_QCOL(kk + 3, s), f4 = LMN_QCOL(kk + 4, s), f5 = LMN_QCOL(kk + 5, s);
        qacc_mad(acc, tab[kk].c, f0);
        qacc_mad(acc, tab[kk + 1].c, f1);
        qacc_mad(acc, tab[kk + 2].c, f2);
        qacc_fold(acc);
        qacc_mad(acc, tab[kk + 3].c, f3);
        qacc_mad(acc, tab[kk + 4].c, f4);
        qacc_mad(acc, tab[kk + 5].c, f5);
        qacc_fold(acc);
      }
      for (; kk < k1; ++kk) {
        qacc_mad(acc, tab[kk].c, LMN_QCOL(kk, s));
        qacc_fold(acc);
      }
      QM31 num = qacc_reduce(acc);
      num = q_sub(num, q_add(q_mul_m(QM31{qd.A[b].a, qd.A[b].b, qd.A[b].c, qd.A[b].d}, ys[k]),
                             QM31{qd.B[b].a, qd.B[b].b, qd.B[b].c, qd.B[b].d}));
      const QM31 term = q_mul_c(num, dinv[k * NB + b]);
      row = b == 0 ? term   // no 0 * coeff product for the first batch
                   : q_add(q_mul(row, QM31{qd.batch_coeff[b].a, qd.batch_coeff[b].b, qd.batch_coeff[b].c, qd.batch_coeff[b].d}), term);
    }
    uint32_t* o = a.out + s;
    o[0] = row.a;
    o[a.out_stride] = row.b;
    o[2ull * a.out_stride] = row.c;
    o[3ull * a.out_stride] = row.d;
  }
#undef LMN_QCOL
}

void launch_quotients(const QuotientArgs& a, lmn_stream_t s) {
  if (a.nbatch < 1 || a.nbatch > QUOT_MAX_BATCH) throw LmnError(-100, "quotients: bad batch count");
  if (a.batch_start[a.nbatch] > QUOT_MAX_ENTRIES) throw LmnError(-100, "quotients: too many column samples");
  if (!a.dev || !a.entries) throw LmnError(-100, "quotients: no batch table");
  if (a.log_size < 2 || a.log_rows < 2 || a.log_rows > a.log_size || (a.row0 & ((1u << a.log_rows) - 1u)) ||
      a.out_stride < (1ull << a.log_rows))
    throw LmnError(-100, "quotients: bad row block");
  if (a.nbatch == 1 && (1u << a.log_rows) < (unsigned)quot_rows<1>()) throw LmnError(-100, "quotients: row block too small");
  dim3 g(cdiv((1ull << a.log_rows) / 4, TPB)), g1(cdiv((1ull << a.log_rows) / quot_rows<1>(), TPB)),
      g2(cdiv((1ull << a.log_rows) / quot_rows<2>(), TPB)), b(TPB);
  switch (a.nbatch) {
    case 1: LMN_LAUNCH(k_quotients_occ<1>, g1, b, 0, s, a); break;
    case 2: LMN_LAUNCH(k_quotients_occ<2>, g2, b, 0, s, a); break;
    case 3: LMN_LAUNCH(k_quotients<3>, g, b, 0, s, a); break;
    default: LMN_LAUNCH(k_quotients<4>, g, b, 0, s, a); break;
  }
}

// =============================================================================================
// a9  FRI folds
// =============================================================================================
LMN_KERNEL k_fold(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t src_len,
                  const uint32_t* __restrict__ itw, const QM31* __restrict__ alpha_ptr, int accumulate,
                  uint64_t dst_stride) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (src_len >> 1)) return;
  const uint64_t n = dst_stride;
  const QM31 alpha = *alpha_ptr;
  const uint64_t L = src_len;
  QM31 a{src[2 * i], src[L + 2 * i], src[2 * L + 2 * i], src[3 * L + 2 * i]};
  QM31 b{src[2 * i + 1], src[L + 2 * i + 1], src[2 * L + 2 * i + 1], src[3 * L + 2 * i + 1]};
  QM31 f0 = q_add(a, b);
  QM31 f1 = q_mul_m(q_sub(a, b), itw[i]);
  QM31 r = q_add(f0, q_mul(alpha, f1));
  if (accumulate) {
    QM31 d{dst[i], dst[n + i], dst[2ull * n + i], dst[3ull * n + i]};
    r = q_add(q_mul(d, q_mul(alpha, alpha)), r);
  }
  dst[i] = r.a;
  dst[n + i] = r.b;
  dst[2ull * n + i] = r.c;
  dst[3ull * n + i] = r.d;
}

void launch_fold_circle_into_line(uint32_t* dst, const uint32_t* src, uint32_t src_len, const uint32_t* itw_y,
                                  const QM31* alpha, int accumulate, lmn_stream_t s, uint64_t dst_stride) {
  LMN_LAUNCH(k_fold, dim3(cdiv(src_len / 2, TPB)), dim3(TPB), 0, s, dst, src, src_len, itw_y, alpha, accumulate,
             dst_stride ? dst_stride : (uint64_t)(src_len / 2));
}
void launch_fold_line(uint32_t* dst, const uint32_t* src, uint32_t src_len, const uint32_t* itw_x, const QM31* alpha,
                      lmn_stream_t s, uint64_t dst_stride) {
  LMN_LAUNCH(k_fold, dim3(cdiv(src_len / 2, TPB)), dim3(TPB), 0, s, dst, src, src_len, itw_x, alpha, 0,
             dst_stride ? dst_stride : (uint64_t)(src_len / 2));
}

}  // namespace lmn
