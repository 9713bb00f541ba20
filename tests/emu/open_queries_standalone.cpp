// Stand-alone host program for the sanitizers (tests/emu/run_open_queries_standalone.sh): openings planned on the device
// through the C ABI of the emulation build compiled with -fsanitize=address,undefined - lmn_positions_*, lmn_open_queries
// on two trees in one call (one of them with LMN_OPEN_FRI_PAIRS), every refusal, lmn_col_fri_close_keep - compared with
// lmn_tree_decommit on the folded (and, for the pairs, expanded) groups and with the host columns; then one 64-row Add proof
// under LMN_DEVICE_FRI_CLOSE=1 LMN_DEVICE_DECOMMIT=1 (the openings planned and fetched behind k_fri_queries), compared with
// the default path's bytes and verified.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/luminair_hip.h"

static const uint32_t P = (1u << 31) - 1u;

#define CHECK(call)                                                                                   \
  do {                                                                                                \
    const int rc_ = (call);                                                                           \
    if (rc_ != LMN_OK) {                                                                              \
      fprintf(stderr, "%s -> %d (%s / %s)\n", #call, rc_, lmn_last_error(ctx), lmn_last_error(NULL)); \
      return 1;                                                                                       \
    }                                                                                                 \
  } while (0)
#define REQUIRE(cond)                                       \
  do {                                                      \
    if (!(cond)) {                                          \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);    \
      return 2;                                             \
    }                                                       \
  } while (0)

static std::vector<uint32_t> fold(const std::vector<uint32_t>& p, int n) {
  std::vector<uint32_t> out;
  for (uint32_t v : p)
    if (out.empty() || out.back() != (v >> n)) out.push_back(v >> n);
  return out;
}

struct Reference {
  std::vector<uint32_t> values, witness;
  std::vector<uint8_t> hashes;
};
// lmn_tree_decommit with one group per log size
static int reference(lmn_ctx* ctx, const lmn_tree* tree, const std::vector<const lmn_col*>& cols, const std::vector<uint32_t>& logs,
                     const std::vector<std::vector<uint32_t>>& groups, Reference& out) {
  std::vector<uint32_t> counts, flat;
  for (auto& g : groups) {
    counts.push_back((uint32_t)g.size());
    flat.insert(flat.end(), g.begin(), g.end());
  }
  uint32_t *v = NULL, *w = NULL;
  uint8_t* h = NULL;
  size_t nv = 0, nh = 0, nw = 0;
  CHECK(lmn_tree_decommit(ctx, tree, cols.data(), (uint32_t)cols.size(), logs.data(), counts.data(), (uint32_t)logs.size(),
                          flat.data(), &v, &nv, &h, &nh, &w, &nw));
  out.values.assign(v, v + nv);
  out.witness.assign(w, w + nw);
  out.hashes.assign(h, h + 32 * nh);
  lmn_free(v);
  lmn_free(h);
  lmn_free(w);
  return 0;
}
static bool same(const lmn_opening& o, const Reference& r) {
  return o.n_values == r.values.size() && o.n_column_words == r.witness.size() && o.n_hashes * 32 == r.hashes.size() &&
         (r.values.empty() || memcmp(o.queried_values, r.values.data(), r.values.size() * 4) == 0) &&
         (r.witness.empty() || memcmp(o.column_witness, r.witness.data(), r.witness.size() * 4) == 0) &&
         (r.hashes.empty() || memcmp(o.hash_witness, r.hashes.data(), r.hashes.size()) == 0);
}
static void release(lmn_opening& o) {
  lmn_free(o.queried_values);
  lmn_free(o.hash_witness);
  lmn_free(o.column_witness);
  lmn_free(o.fri_witness);
  o = lmn_opening{};
}
static bool zeroed(const lmn_opening& o) {
  return !o.queried_values && !o.hash_witness && !o.column_witness && !o.fri_witness && !o.n_values && !o.n_hashes &&
         !o.n_column_words && !o.n_fri_words;
}

int main() {
  lmn_config cfg;
  lmn_default_config(&cfg);
  cfg.pow_bits = 12;
  cfg.n_queries = 70;
  lmn_ctx* ctx = NULL;
  CHECK(lmn_ctx_create(0, &cfg, &ctx));
  // tree A: 3 columns of 2^7 rows and 2 of 2^5; tree B: secure columns (4 coordinate columns) of 2^8 and 2^6 rows
  uint32_t seed = 12345u;
  auto words = [&](size_t n) {
    std::vector<uint32_t> v(n);
    for (auto& x : v) x = (seed = seed * 1664525u + 1013904223u) % P;
    return v;
  };
  const std::vector<uint32_t> a7 = words(3 << 7), a5 = words(2 << 5), b8 = words(4 << 8), b6 = words(4 << 6);
  lmn_col *ca7 = NULL, *ca5 = NULL, *cb8 = NULL, *cb6 = NULL;
  CHECK(lmn_col_from_cpu(ctx, a7.data(), 3, 7, &ca7));
  CHECK(lmn_col_from_cpu(ctx, a5.data(), 2, 5, &ca5));
  CHECK(lmn_col_from_cpu(ctx, b8.data(), 4, 8, &cb8));
  CHECK(lmn_col_from_cpu(ctx, b6.data(), 4, 6, &cb6));
  const std::vector<const lmn_col*> cols_a{ca5, ca7}, cols_b{cb8, cb6};
  lmn_tree *ta = NULL, *tb = NULL;
  CHECK(lmn_col_commit(ctx, cols_a.data(), 2, &ta));
  CHECK(lmn_col_commit(ctx, cols_b.data(), 2, &tb));

  // ---- positions: round trip, then both trees in one call
  const uint32_t D = 10;
  const std::vector<uint32_t> pos{0, 5, 6, 7, 300, 301, 640, 1023};
  lmn_positions* dp = NULL;
  CHECK(lmn_positions_from_cpu(ctx, pos.data(), (uint32_t)pos.size(), D, &dp));
  REQUIRE(lmn_positions_log_domain(dp) == D);
  uint32_t back[1024], n_back = 0;
  CHECK(lmn_positions_to_cpu(ctx, dp, back, &n_back));
  REQUIRE(n_back == pos.size() && memcmp(back, pos.data(), pos.size() * 4) == 0);
  lmn_open_item items[2] = {{ta, cols_a.data(), 2, 0u}, {tb, cols_b.data(), 2, LMN_OPEN_FRI_PAIRS}};
  lmn_opening out[2];
  memset(out, 0xff, sizeof out);
  CHECK(lmn_open_queries(ctx, dp, items, 2, out));
  Reference ra, rb;
  if (reference(ctx, ta, cols_a, {7, 5}, {fold(pos, 3), fold(pos, 5)}, ra)) return 1;
  REQUIRE(same(out[0], ra) && out[0].n_fri_words == 0 && !out[0].fri_witness);
  // the pairs: every folded position with its sibling; 4 words per sibling that is no position, sizes descending
  std::vector<std::vector<uint32_t>> expanded;
  std::vector<uint32_t> fri;
  const uint32_t* secure[2] = {b8.data(), b6.data()};
  const int logs_b[2] = {8, 6};
  for (int s = 0; s < 2; ++s) {
    const std::vector<uint32_t> f = fold(pos, (int)D - logs_b[s]);
    std::vector<uint32_t> e;
    for (uint32_t p : f)
      if (e.empty() || e.back() != (p | 1u)) {
        e.push_back(p & ~1u);
        e.push_back(p | 1u);
      }
    for (uint32_t p : e) {
      bool is_pos = false;
      for (uint32_t q : f) is_pos |= q == p;
      if (!is_pos)
        for (int k = 0; k < 4; ++k) fri.push_back(secure[s][((size_t)k << logs_b[s]) + p]);
    }
    expanded.push_back(e);
  }
  if (reference(ctx, tb, cols_b, {8, 6}, expanded, rb)) return 1;
  REQUIRE(same(out[1], rb));
  REQUIRE(out[1].n_fri_words == fri.size() && !fri.empty() && memcmp(out[1].fri_witness, fri.data(), fri.size() * 4) == 0);
  release(out[0]);
  release(out[1]);

  // ---- every refusal: LMN_ERR_INVALID_ARGUMENT, a text naming the argument, the outputs zeroed
  struct Refusal {
    const char* name;
    const lmn_positions* p;
    std::vector<lmn_open_item> items;
    uint32_t n_items;
    bool null_items, null_out;
    const char* word;
  };
  lmn_positions *small = NULL, *many = NULL;
  const uint32_t two[2] = {1, 2};
  CHECK(lmn_positions_from_cpu(ctx, two, 2, 6, &small));
  std::vector<uint32_t> thousand(1024);
  for (uint32_t i = 0; i < 1024; ++i) thousand[i] = 2 * i;
  CHECK(lmn_positions_from_cpu(ctx, thousand.data(), 1024, 27, &many));
  const std::vector<uint32_t> wide_words(4096u << 10, 0u);
  lmn_col* wide = NULL;
  CHECK(lmn_col_from_cpu(ctx, wide_words.data(), 4096, 10, &wide));
  lmn_tree* tw = NULL;
  const lmn_col* cols_w[1] = {wide};
  CHECK(lmn_col_commit(ctx, cols_w, 1, &tw));
  const lmn_col* short_a[1] = {ca7};
  const lmn_col* null_in[2] = {ca5, NULL};
  const lmn_col* swapped[2] = {ca7, cb6};
  const std::vector<Refusal> refusals = {
      {"null positions", NULL, {{ta, cols_a.data(), 2, 0u}}, 1, false, false, "positions is null"},
      {"null items", dp, {{ta, cols_a.data(), 2, 0u}}, 1, true, false, "items is null"},
      {"null out", dp, {{ta, cols_a.data(), 2, 0u}}, 1, false, true, "out is null"},
      {"null tree", dp, {{NULL, cols_a.data(), 2, 0u}}, 1, false, false, "items[0].tree is null"},
      {"null cols", dp, {{ta, NULL, 2, 0u}}, 1, false, false, "items[0].cols is null"},
      {"null handle", dp, {{ta, null_in, 2, 0u}}, 1, false, false, "items[0].cols[1] is null"},
      {"65 items", dp, std::vector<lmn_open_item>(65, lmn_open_item{ta, cols_a.data(), 2, 0u}), 65, false, false, "n_items is 65"},
      {"tree above the domain", small, {{ta, cols_a.data(), 2, 0u}}, 1, false, false, "log_domain 6"},
      {"a column too few", dp, {{ta, short_a, 1, 0u}}, 1, false, false, "committed from 2"},
      {"other columns", dp, {{ta, swapped, 2, 0u}}, 1, false, false, "items[0].cols holds"},
      {"pairs on 3 + 2 columns", dp, {{ta, cols_a.data(), 2, LMN_OPEN_FRI_PAIRS}}, 1, false, false, "LMN_OPEN_FRI_PAIRS"},
      {"unknown flag", dp, {{ta, cols_a.data(), 2, 4u}}, 1, false, false, "unknown flag"},
      {"above 12 MiB", many, {{tw, cols_w, 1, 0u}}, 1, false, false, "upper bound"},
  };
  for (const Refusal& r : refusals) {
    std::vector<lmn_opening> o(r.n_items);
    memset(o.data(), 0xff, o.size() * sizeof(lmn_opening));
    const int rc = lmn_open_queries(ctx, r.p, r.null_items ? NULL : r.items.data(), r.n_items, r.null_out ? NULL : o.data());
    if (rc != LMN_ERR_INVALID_ARGUMENT || !strstr(lmn_last_error(ctx), r.word) || !strstr(lmn_last_error(ctx), "open_queries")) {
      fprintf(stderr, "refusal '%s': rc %d, text '%s'\n", r.name, rc, lmn_last_error(ctx));
      return 3;
    }
    if (!r.null_out)
      for (auto& x : o) REQUIRE(zeroed(x));
    // the context and the handles go on working
    lmn_opening again[1];
    CHECK(lmn_open_queries(ctx, dp, items, 1, again));
    REQUIRE(same(again[0], ra));
    release(again[0]);
  }
  REQUIRE(lmn_open_queries(NULL, dp, items, 1, out) == LMN_ERR_INVALID_ARGUMENT);
  // positions_from_cpu
  struct BadPositions {
    std::vector<uint32_t> p;
    uint32_t log_domain;
    const char* word;
  };
  std::vector<uint32_t> too_many(1025);
  for (uint32_t i = 0; i < 1025; ++i) too_many[i] = i;
  for (const BadPositions& b : std::vector<BadPositions>{{too_many, 12, "n is 1025"}, {{5, 40, 7}, 9, "ascending"}, {{5, 5}, 9, "ascending"},
                                                         {{5, 512}, 9, "out of range"}, {{5}, 32, "log_domain is 32"}}) {
    lmn_positions* bad = (lmn_positions*)(uintptr_t)1;
    REQUIRE(lmn_positions_from_cpu(ctx, b.p.data(), (uint32_t)b.p.size(), b.log_domain, &bad) == LMN_ERR_INVALID_ARGUMENT);
    REQUIRE(bad == NULL && strstr(lmn_last_error(ctx), b.word) && strstr(lmn_last_error(ctx), "positions_from_cpu"));
  }
  lmn_positions* bad = (lmn_positions*)(uintptr_t)1;
  REQUIRE(lmn_positions_from_cpu(ctx, NULL, 3, 9, &bad) == LMN_ERR_INVALID_ARGUMENT && bad == NULL);
  REQUIRE(lmn_positions_to_cpu(ctx, NULL, back, &n_back) == LMN_ERR_INVALID_ARGUMENT && n_back == 0);
  // zero positions, zero items
  lmn_positions* none = NULL;
  CHECK(lmn_positions_from_cpu(ctx, NULL, 0, D, &none));
  memset(out, 0xff, sizeof out);
  CHECK(lmn_open_queries(ctx, none, items, 2, out));
  REQUIRE(zeroed(out[0]) && zeroed(out[1]));
  CHECK(lmn_open_queries(ctx, dp, NULL, 0, NULL));
  lmn_positions_free(ctx, none);
  lmn_positions_free(ctx, NULL);

  // ---- lmn_col_fri_close_keep: the result of lmn_col_fri_close, and a handle that holds its positions
  const uint32_t last_log = cfg.log_last_layer + cfg.log_blowup;
  const std::vector<uint32_t> last_words = words((size_t)4 << last_log);
  lmn_col* last = NULL;
  CHECK(lmn_col_from_cpu(ctx, last_words.data(), 4, last_log, &last));
  uint8_t digest[32];
  for (int i = 0; i < 32; ++i) digest[i] = (uint8_t)(7 * i + 1);
  lmn_fri_close_result plain, kept;
  lmn_positions* kp = NULL;
  CHECK(lmn_col_fri_close(ctx, last, digest, 7, &plain));
  CHECK(lmn_col_fri_close_keep(ctx, last, digest, 7, &kept, &kp));
  REQUIRE(kept.nonce == plain.nonce && kept.n_positions == plain.n_positions && kept.first_bad == plain.first_bad &&
          memcmp(kept.positions, plain.positions, 4 * plain.n_positions) == 0 &&
          memcmp(kept.digest_end, plain.digest_end, 32) == 0 && memcmp(kept.coeffs, plain.coeffs, 16 * plain.n_coeffs) == 0);
  CHECK(lmn_positions_to_cpu(ctx, kp, back, &n_back));
  REQUIRE(lmn_positions_log_domain(kp) == 7 && n_back == plain.n_positions && memcmp(back, plain.positions, 4 * n_back) == 0);
  REQUIRE(plain.n_positions < 70);   // 70 draws into 128 positions: duplicates were removed
  const std::vector<uint32_t> drawn(plain.positions, plain.positions + plain.n_positions);
  CHECK(lmn_open_queries(ctx, kp, items, 1, out));
  Reference rk;
  if (reference(ctx, ta, cols_a, {7, 5}, {drawn, fold(drawn, 2)}, rk)) return 1;
  REQUIRE(same(out[0], rk));
  release(out[0]);
  lmn_fri_close_result z;
  lmn_positions* zp = (lmn_positions*)(uintptr_t)1;
  REQUIRE(lmn_col_fri_close_keep(ctx, last, digest, 32, &z, &zp) == LMN_ERR_INVALID_ARGUMENT && zp == NULL && z.positions == NULL);
  for (lmn_fri_close_result* r : {&plain, &kept}) {
    lmn_free(r->coeffs);
    lmn_free(r->positions);
  }
  lmn_positions_free(ctx, kp);
  lmn_col_free(ctx, last);

  lmn_positions_free(ctx, dp);
  lmn_positions_free(ctx, small);
  lmn_positions_free(ctx, many);
  lmn_tree_free(ctx, ta);
  lmn_tree_free(ctx, tb);
  lmn_tree_free(ctx, tw);
  for (lmn_col* c : {ca7, ca5, cb8, cb6, wide}) lmn_col_free(ctx, c);
  lmn_ctx_destroy(ctx);

  // ---- a 64-row Add proof (pow_bits 12, 70 queries) with default switches, then under both device switches
  std::vector<uint32_t> add_rows;
  for (uint32_t j = 0; j < 64; ++j) {
    // node 2 = node 0 + node 1, every multiplicity 0: the row satisfies lhs + rhs - out = 0 and adds nothing to the logup sums
    const uint32_t a = (7 * j + 3) % P, b = (11 * j + 5) % P, last = j == 63 ? 1u : 0u;
    const uint32_t row[15] = {2u, 0u, 1u, j, last, 2u, 0u, 1u, j + 1u, a, b, (a + b) % P, 0u, 0u, 0u};
    add_rows.insert(add_rows.end(), row, row + 15);
  }
  lmn_table table;
  memset(&table, 0, sizeof table);
  table.kind = 0;   // Add
  table.n_rows = 64;
  table.rows = add_rows.data();
  REQUIRE(lmn_kind_columns(0) == 15);
  uint8_t* proofs[2] = {NULL, NULL};
  size_t lens[2] = {0, 0};
  for (int dev = 0; dev < 2; ++dev) {
    if (dev) {
      setenv("LMN_DEVICE_FRI_CLOSE", "1", 1);
      setenv("LMN_DEVICE_DECOMMIT", "1", 1);
    }
    ctx = NULL;
    CHECK(lmn_ctx_create(0, &cfg, &ctx));
    CHECK(lmn_prove(ctx, &table, 1, NULL, &proofs[dev], &lens[dev]));
    REQUIRE(lmn_ctx_counter(ctx, 11) == (uint64_t)dev && lmn_ctx_counter(ctx, 9) == (uint64_t)dev);
    REQUIRE(lmn_ctx_counter(ctx, 12) == lmn_ctx_counter(ctx, 10));
    lmn_ctx_destroy(ctx);
  }
  ctx = NULL;
  REQUIRE(lens[0] == lens[1] && memcmp(proofs[0], proofs[1], lens[0]) == 0);
  CHECK(lmn_verify_with_config(proofs[1], lens[1], NULL, &cfg));
  lmn_free(proofs[0]);
  lmn_free(proofs[1]);
  printf("a 64-row proof under both device switches: the default path's %zu bytes, accepted\n", lens[0]);
  printf("open_queries: positions, two trees in one call (one with pairs), %zu refusals, fri_close_keep: ok\n", refusals.size());
  return 0;
}
