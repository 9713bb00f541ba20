// The 17 AIR components on the host (their shapes and local constraints are constraints.h): the constraint slots under the
// protocol's constraint-form bits, the relation-element draws
// (components/mod.rs:227-235, lookups/mod.rs:44-51) and the host-side evaluation of the composition polynomial at the OODS
// point from sampled mask values (shared by the prover's self-check and the verifier).
#include "prover_internal.h"

namespace lmn {

// ------------------------------------------------------------------------------------ components
const ComponentSpec* component_spec(int kind) { return kind >= 0 && kind < N_KINDS ? &kSpecs[kind] : nullptr; }

ConstraintLayout constraint_layout(const ComponentSpec& sp, uint32_t flags) {
  ConstraintLayout L;
  L.n_kernel = sp.n_local + sp.n_rel;
  // kernel slot 1 is the eval_fixed_* constraint of Mul / Recip / Sqrt / Rem; Mul's kernel slot 2 is its zero slot
  bool drop_slot2 = false, extra_after1 = false, neg1 = false;
  switch (sp.kind) {
    case LMN_KIND_MUL: drop_slot2 = (flags & LMN_PV_MUL_ONE_SLOT) != 0; break;
    case LMN_KIND_RECIP: extra_after1 = (flags & LMN_PV_RECIP_TWO_SLOTS) != 0; neg1 = (flags & LMN_PV_RECIP_NEG) != 0; break;
    case LMN_KIND_SQRT: extra_after1 = (flags & LMN_PV_SQRT_TWO_SLOTS) != 0; neg1 = (flags & LMN_PV_SQRT_NEG) != 0; break;
    case LMN_KIND_REM: extra_after1 = (flags & LMN_PV_REM_TWO_SLOTS) != 0; neg1 = (flags & LMN_PV_REM_NEG) != 0; break;
    default: break;
  }
  int p = 0;
  for (int k = 0; k < L.n_kernel; ++k) {
    L.neg[k] = k == 1 && neg1;
    if (k == 2 && drop_slot2) {
      L.proto_index[k] = -1;
      continue;
    }
    L.proto_index[k] = p++;
    if (k == 1 && extra_after1) ++p;   // the helper's second (zero) slot
  }
  L.n_protocol = p;
  return L;
}

int relation_draw_sets(uint32_t protocol_flags, int sets_out[5]) {
  int n = 0;
  sets_out[n++] = ELEMS_NODE;
  sets_out[n++] = ELEMS_SIN;  // the KAT era drew a single LUT relation; HEAD: sin, exp2, log2, range_check
  if (protocol_flags & LMN_PV_LUT_DRAWS4) {
    sets_out[n++] = ELEMS_EXP2;
    sets_out[n++] = ELEMS_LOG2;
    sets_out[n++] = ELEMS_RANGE_CHECK;
  }
  return n;
}

RelElems draw_relation_elements(Channel& channel, uint32_t protocol_flags) {
  RelElems e;
  int sets[5];
  const int n = relation_draw_sets(protocol_flags, sets);
  for (int i = 0; i < n; ++i) {
    std::vector<QM31> d = channel.draw_felts(2);
    e.z[sets[i]] = d[0];
    e.alpha[sets[i]] = d[1];
    e.drawn[sets[i]] = true;
  }
  return e;
}

std::vector<int> assign_preprocessed(std::vector<Instance>& inst) {
  int log_of[N_PRE_IDS];
  for (int& l : log_of) l = -1;
  for (auto& ci : inst)
    for (int k = 0; k < ci.spec->n_pre; ++k) log_of[ci.spec->pre_id[k]] = ci.log_size;
  std::vector<int> order;
  for (int id = 0; id < N_PRE_IDS; ++id)
    if (log_of[id] >= 0) order.push_back(id);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return log_of[a] > log_of[b]; });
  int pos[N_PRE_IDS];
  std::vector<int> logs;
  for (size_t i = 0; i < order.size(); ++i) {
    pos[order[i]] = (int)i;
    logs.push_back(log_of[order[i]]);
  }
  for (auto& ci : inst)
    for (int k = 0; k < ci.spec->n_pre; ++k) ci.pre_idx[k] = pos[ci.spec->pre_id[k]];
  return logs;
}

// ------------------------------------------------------------------------------------ host-side AIR at a point
// local constraints at a point: constraints.h local_constraints<kind> on QM31 values
static std::vector<QM31> local_constraints_at(int kind, const std::vector<QM31>& c) {
  std::vector<QM31> out;
  auto emit = [&](QM31 v) { out.push_back(v); };
#define LMN_LC_CASE(K) case K: local_constraints<K>(c.data(), emit); break;
  switch (kind) {
    LMN_LC_CASE(0) LMN_LC_CASE(1) LMN_LC_CASE(2) LMN_LC_CASE(3) LMN_LC_CASE(4) LMN_LC_CASE(5) LMN_LC_CASE(6) LMN_LC_CASE(7)
    LMN_LC_CASE(8) LMN_LC_CASE(9) LMN_LC_CASE(10) LMN_LC_CASE(11) LMN_LC_CASE(12) LMN_LC_CASE(13) LMN_LC_CASE(14)
    LMN_LC_CASE(15) LMN_LC_CASE(16)
  }
#undef LMN_LC_CASE
  return out;
}

QM31 eval_composition_at_point(const std::vector<Instance>& inst,
                               const std::vector<std::vector<std::vector<QM31>>>& sv, QPt oods, const RelElems& elems,
                               QM31 comp_alpha, uint32_t protocol_flags) {
  QM31 acc = q_zero();
  for (auto& ci : inst) {
    const ComponentSpec* sp = ci.spec;
    std::vector<QM31> main(sp->n_cols);
    for (int c = 0; c < sp->n_cols; ++c) main[c] = sv[1][ci.main_start + c][0];
    std::vector<QM31> cons = local_constraints_at(sp->kind, main);
    QM31 prev = q_zero();
    QM31 shift = q_mul_m(ci.claimed, m_inv((uint32_t)((1ull << ci.log_size) % P31)));
    for (int j = 0; j < sp->n_rel; ++j) {
      const auto* cols = &sv[2][ci.inter_start + 4 * j];
      auto cell = [&](int idx) { return sp->rel_pre[j] ? sv[0][ci.pre_idx[idx]][0] : main[idx]; };
      const int es = sp->rel_elems[j];
      QM31 den = q_sub(cell(sp->rel_val[j]), elems.z[es]);
      if (sp->rel_id[j] >= 0) den = q_add(den, q_mul(elems.alpha[es], cell(sp->rel_id[j])));
      QM31 num = sp->rel_neg[j] ? q_neg(main[sp->rel_mult[j]]) : main[sp->rel_mult[j]];
      QM31 cur, diff;
      if (j < sp->n_rel - 1) {
        cur = q_from_partial_evals(cols[0][0], cols[1][0], cols[2][0], cols[3][0]);
        diff = q_sub(cur, prev);
      } else {
        QM31 prev_row = q_from_partial_evals(cols[0][0], cols[1][0], cols[2][0], cols[3][0]);
        cur = q_from_partial_evals(cols[0][1], cols[1][1], cols[2][1], cols[3][1]);
        diff = q_add(q_sub(q_sub(cur, prev_row), prev), shift);
      }
      cons.push_back(q_sub(q_mul(diff, den), num));
      prev = cur;
    }
    QM31 x = oods.x;
    for (int k = 0; k < ci.log_size - 1; ++k) x = q_sub_m(q_add(q_sqr(x), q_sqr(x)), 1u);
    QM31 zinv = q_inv(x);
    // kernel-slot values -> the protocol's constraint list (constraint-form bits: slots added / dropped, signs)
    const ConstraintLayout L = constraint_layout(*sp, protocol_flags);
    std::vector<QM31> proto(L.n_protocol, q_zero());
    for (int k = 0; k < L.n_kernel; ++k)
      if (L.proto_index[k] >= 0) proto[L.proto_index[k]] = L.neg[k] ? q_neg(cons[k]) : cons[k];
    for (auto& c : proto) acc = q_add(q_mul(acc, comp_alpha), q_mul(c, zinv));
  }
  return acc;
}

}  // namespace lmn
