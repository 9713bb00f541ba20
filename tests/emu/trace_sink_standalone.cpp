// Stand-alone host program for the sanitizers (tests/emu/run_trace_sink_standalone.sh): the host logic of the device appends
// to row sinks (lmn_rows_append_*) through the C ABI of the emulation build, compiled once with -fsanitize=address,undefined
// and once with -fsanitize=thread.  First alone: two nodes and a host chunk in one sink, column for column; a refused element,
// the refused finish, reset, a clean table.  Then three threads: two drive two contexts, each appending to both sinks (the
// context's lock, then the sink's), while a third pushes host chunks and finishes and resets the two sinks in turn.  Under
// that race a call may find its sink finished or full - LMN_ERR_INVALID_ARGUMENT is a right answer there, anything else is
// not - and afterwards both sinks must still take and give back a table exactly.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/luminair_hip.h"

static const uint32_t P = (1u << 31) - 1u;
static const int NC = 15;   // columns of an Add row

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

static uint32_t m31(int64_t v) { return (uint32_t)(((v % (int64_t)P) + (int64_t)P) % (int64_t)P); }

// the rows of one Add node (add/table.rs) on in-contract operands: what lmn_trace_elementwise writes
static std::vector<uint32_t> add_rows(const std::vector<int32_t>& a, const std::vector<int32_t>& b, const lmn_node_info& info) {
  std::vector<uint32_t> rows;
  const size_t n = a.size();
  for (size_t i = 0; i < n; ++i) {
    const uint32_t row[NC] = {info.node_id, info.input_ids[0], info.input_ids[1], (uint32_t)i, i + 1 == n ? 1u : 0u,
                              info.node_id, info.input_ids[0], info.input_ids[1], (uint32_t)i + 1u,
                              m31(a[i]), m31(b[i]), m31((int64_t)a[i] + b[i]),
                              m31(info.input_mults[0]), m31(info.input_mults[1]), info.is_final_output ? 0u : m31(info.num_consumers)};
    rows.insert(rows.end(), row, row + NC);
  }
  return rows;
}

// a finished sink's columns == the rows transposed, then the padding row
static int same_columns(lmn_ctx* ctx, const lmn_table& t, const std::vector<uint32_t>& rows) {
  const size_t n = rows.size() / NC;
  REQUIRE(t.kind == LMN_KIND_ADD && t.flags == LMN_TABLE_COLS_ON_DEVICE && t.n_rows == n);
  size_t size = 16;
  while (size < n) size <<= 1;
  uint32_t pad[32];
  CHECK(lmn_kind_padding_row(LMN_KIND_ADD, pad));
  std::vector<uint32_t> got(NC * size);
  CHECK(lmn_download(ctx, t.rows, got.data(), got.size() * 4));
  for (int c = 0; c < NC; ++c)
    for (size_t r = 0; r < size; ++r) REQUIRE(got[c * size + r] == (r < n ? rows[r * NC + c] : pad[c]));
  return 0;
}

struct Operands {
  std::vector<int32_t> a, b;
  int32_t *da = nullptr, *db = nullptr, *out = nullptr;
  uint32_t* refused = nullptr;
};
static int make_operands(lmn_ctx* ctx, size_t n, uint32_t seed, Operands& o) {
  o.a.resize(n);
  o.b.resize(n);
  for (size_t i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    o.a[i] = (int32_t)(seed >> 12) - (1 << 19);
    seed = seed * 1664525u + 1013904223u;
    o.b[i] = (int32_t)(seed >> 12) - (1 << 19);
  }
  const uint32_t zero = 0;
  CHECK(lmn_upload(ctx, o.a.data(), n * 4, (void**)&o.da));
  CHECK(lmn_upload(ctx, o.b.data(), n * 4, (void**)&o.db));
  CHECK(lmn_upload(ctx, &zero, 4, (void**)&o.refused));
  CHECK(lmn_device_alloc(ctx, n * 4, (void**)&o.out));
  return 0;
}
static void free_operands(lmn_ctx* ctx, Operands& o) {
  for (void* p : {(void*)o.da, (void*)o.db, (void*)o.out, (void*)o.refused}) lmn_device_free(ctx, p);
}
static int append(lmn_ctx* ctx, lmn_rows* sink, const Operands& o, uint64_t n, const lmn_node_info& info) {
  return lmn_rows_append_elementwise_v(ctx, sink, LMN_KIND_ADD, o.da, NULL, o.db, NULL, n, &info, NULL, o.out, o.refused);
}

static int alone(lmn_ctx* ctx) {
  const lmn_node_info i1{3, {1, 2}, 1, 0, {-1, -1}}, ih{4, {1, 2}, 2, 0, {-1, -1}}, i2{5, {3, 2}, 0, 1, {-1, 0}};
  Operands o;
  if (int rc = make_operands(ctx, 300, 7u, o)) return rc;
  const std::vector<int32_t> a1(o.a.begin(), o.a.begin() + 257), b1(o.b.begin(), o.b.begin() + 257);
  const std::vector<int32_t> ah(o.a.begin(), o.a.begin() + 5), bh(o.b.begin(), o.b.begin() + 5);
  lmn_rows* sink = NULL;
  CHECK(lmn_rows_open(ctx, LMN_KIND_ADD, 257 + 5 + 300, &sink));
  // two nodes and a host chunk
  std::vector<uint32_t> want = add_rows(a1, b1, i1);
  const std::vector<uint32_t> host = add_rows(ah, bh, ih), last = add_rows(o.a, o.b, i2);
  CHECK(append(ctx, sink, o, 257, i1));
  CHECK(lmn_rows_push(sink, host.data(), 5));
  CHECK(append(ctx, sink, o, 300, i2));
  REQUIRE(lmn_rows_count(sink) == 562);
  REQUIRE(append(ctx, sink, o, 1, i1) == LMN_ERR_INVALID_ARGUMENT && strstr(lmn_last_error(ctx), "capacity"));
  want.insert(want.end(), host.begin(), host.end());
  want.insert(want.end(), last.begin(), last.end());
  lmn_table t{};
  CHECK(lmn_rows_finish(sink, &t));
  if (int rc = same_columns(ctx, t, want)) return rc;
  REQUIRE(append(ctx, sink, o, 1, i1) == LMN_ERR_INVALID_ARGUMENT && strstr(lmn_last_error(ctx), "lmn_rows_reset"));
  // a refused element (the sum leaves the value range): counted, the finish refused; a reset, then a clean table
  const int32_t big = (1 << 30) - 1;
  CHECK(lmn_upload_to(ctx, &big, 4, o.da + 9));
  CHECK(lmn_upload_to(ctx, &big, 4, o.db + 9));
  CHECK(lmn_rows_reset(sink));
  CHECK(append(ctx, sink, o, 20, i1));
  uint32_t n_refused = 0;
  int32_t out9 = -1;
  CHECK(lmn_download(ctx, o.refused, &n_refused, 4));
  CHECK(lmn_download(ctx, o.out + 9, &out9, 4));
  REQUIRE(n_refused == 1 && out9 == 0);
  REQUIRE(lmn_rows_finish(sink, &t) == LMN_ERR_INVALID_ARGUMENT && strstr(lmn_last_error(NULL), "refused"));
  REQUIRE(append(ctx, sink, o, 1, i1) == LMN_ERR_INVALID_ARGUMENT);
  CHECK(lmn_upload_to(ctx, &o.a[9], 4, o.da + 9));
  CHECK(lmn_upload_to(ctx, &o.b[9], 4, o.db + 9));
  CHECK(lmn_rows_reset(sink));
  CHECK(append(ctx, sink, o, 257, i1));
  CHECK(lmn_rows_finish(sink, &t));
  if (int rc = same_columns(ctx, t, add_rows(a1, b1, i1))) return rc;
  // refused before any launch: a null sink, another kind, n == 0
  REQUIRE(append(ctx, NULL, o, 1, i1) == LMN_ERR_INVALID_ARGUMENT && strstr(lmn_last_error(ctx), "rows"));
  REQUIRE(lmn_rows_append_reduce(ctx, sink, 0, o.da, 1, 5, 1, &i1, o.out, NULL) == LMN_ERR_INVALID_ARGUMENT);
  CHECK(lmn_rows_reset(sink));
  REQUIRE(append(ctx, sink, o, 0, i1) == LMN_ERR_EMPTY_TRACE && lmn_rows_count(sink) == 0);
  lmn_rows_close(sink);
  free_operands(ctx, o);
  return 0;
}

static const uint64_t NODE_ROWS = 70, CHUNK_ROWS_HOST = 9, CAPACITY = 600;
static std::atomic<int> failures{0};
static void expect(bool ok, const char* what, int rc) {
  if (!ok) {
    fprintf(stderr, "concurrent phase: %s -> %d\n", what, rc);
    failures.fetch_add(1);
  }
}

// one producer thread: its own context, appends to both sinks in turn
static void producer(lmn_ctx* ctx, lmn_rows* const sinks[2], uint32_t seed, int rounds) {
  Operands o;
  if (make_operands(ctx, NODE_ROWS, seed, o)) {
    failures.fetch_add(1);
    return;
  }
  const lmn_node_info info{seed, {1, 2}, 1, 0, {-1, -1}};
  for (int i = 0; i < rounds; ++i) {
    lmn_rows* s = sinks[(i + seed) & 1];
    const int rc = append(ctx, s, o, NODE_ROWS, info);
    expect(rc == LMN_OK || rc == LMN_ERR_INVALID_ARGUMENT, "lmn_rows_append_elementwise_v", rc);   // finished or full: refused
    expect(lmn_rows_count(s) <= CAPACITY, "lmn_rows_count", (int)lmn_rows_count(s));
    if ((i & 7) == 7) {
      uint32_t n_refused = 1;
      expect(lmn_download(ctx, o.refused, &n_refused, 4) == LMN_OK && n_refused == 0, "refused counter", (int)n_refused);
    }
  }
  free_operands(ctx, o);
}

// the third thread: host chunks into both sinks, and a finish and a reset of each in turn
static void pusher(lmn_rows* const sinks[2], int rounds) {
  std::vector<int32_t> a(CHUNK_ROWS_HOST, 5), b(CHUNK_ROWS_HOST, -7);
  const std::vector<uint32_t> chunk = add_rows(a, b, lmn_node_info{9, {1, 2}, 1, 0, {-1, -1}});
  for (int i = 0; i < rounds; ++i) {
    lmn_rows* s = sinks[i & 1];
    int rc = lmn_rows_push(s, chunk.data(), CHUNK_ROWS_HOST);
    expect(rc == LMN_OK || rc == LMN_ERR_INVALID_ARGUMENT, "lmn_rows_push", rc);
    if (i % 3 == 2) {
      lmn_table t{};
      rc = lmn_rows_finish(s, &t);
      expect(rc == LMN_OK || rc == LMN_ERR_INVALID_ARGUMENT || rc == LMN_ERR_EMPTY_TRACE, "lmn_rows_finish", rc);
      if (rc == LMN_OK) expect(t.n_rows == lmn_rows_count(s) && t.n_rows <= CAPACITY, "finished table", (int)t.n_rows);
      expect(lmn_rows_sync(s) == LMN_OK, "lmn_rows_sync", 0);
      expect(lmn_rows_reset(s) == LMN_OK, "lmn_rows_reset", 0);
    }
  }
}

int main() {
  lmn_ctx *ctx = NULL, *ctx_b = NULL;
  CHECK(lmn_ctx_create(0, NULL, &ctx));
  CHECK(lmn_ctx_create(0, NULL, &ctx_b));
  if (int rc = alone(ctx)) return rc;

  lmn_rows* sinks[2] = {NULL, NULL};
  CHECK(lmn_rows_open(ctx, LMN_KIND_ADD, CAPACITY, &sinks[0]));
  CHECK(lmn_rows_open(ctx_b, LMN_KIND_ADD, CAPACITY, &sinks[1]));
  const int rounds = 48;
  std::thread t1(producer, ctx, sinks, 1u, rounds), t2(producer, ctx_b, sinks, 2u, rounds), t3(pusher, sinks, rounds);
  t1.join();
  t2.join();
  t3.join();
  REQUIRE(failures.load() == 0);
  // both sinks still take a table and give it back exactly, from either context
  Operands o;
  if (int rc = make_operands(ctx_b, 257, 11u, o)) return rc;
  const lmn_node_info info{3, {1, 2}, 1, 0, {-1, -1}};
  for (lmn_rows* s : sinks) {
    lmn_ctx* ctx = ctx_b;   // (the macros' context)
    CHECK(lmn_rows_reset(s));
    CHECK(append(ctx, s, o, 257, info));
    lmn_table t{};
    CHECK(lmn_rows_finish(s, &t));
    if (int rc = same_columns(ctx, t, add_rows(o.a, o.b, info))) return rc;
    lmn_rows_close(s);
  }
  free_operands(ctx_b, o);
  lmn_ctx_destroy(ctx_b);
  lmn_ctx_destroy(ctx);
  printf("trace_sink_standalone ok\n");
  return 0;
}
