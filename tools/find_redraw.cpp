// Search for transcript inputs at which Channel::draw_base_felts (csrc/host.h; oracle/channel.py _draw_base_felts) takes its
// rare paths: a redraw (one of the eight words of a draw is >= 2P, P = 2^31 - 1: 0xFFFFFFFE or 0xFFFFFFFF, about 2^-28 per
// draw), the largest accepted word (0xFFFFFFFD -> P - 1) and a word equal to P (-> 0).  The hits are the records of
// tests/golden/transcript_redraw_seeds.json; tests/test_transcript_redraw_seeds.py checks every record with hashlib alone.
// Plain C++ with its own Blake2s (nothing of csrc/ is included: a fault there cannot hide in here), threads capped by an
// argument, no GPU.  Two consecutive redraws would cost about 2^56 trials and are out of reach.
//
// Build:
//   g++ -std=c++17 -O3 -march=native -pthread tools/find_redraw.cpp -o tools/bin/find_redraw
//
// Usage (every hit is one line of JSON on stdout, a record of the seeds file):
//   find_redraw chain <name> <64|37> <redraw|accept-edge|reduce-edge> <layers j,j,..> <word value hex|any> <idx lo> <idx hi>
//                     <threads> <seed> <root hex> [<root hex> ...]
//     hash-chain mode.  64 | 37: the draw encoding (37 = LMN_PV_DRAW_CTR_U32).  Finds, for every layer j of the list, a start
//     digest such that in the chain `mix_root(r_i); draw_felt()` over the given roots the event happens at layer j, in a word
//     whose index lies in [lo, hi] (and equals the given value, if one is given), and no other layer redraws or meets an
//     edge.  redraw: a word >= 2P at counter 0, none outside [lo, hi], and the draw at counter 1 is accepted.  A trial walks
//     the whole chain (2 compressions per layer) and counts for whichever listed layer it hits.
//   find_redraw trace <name> <set> <threads> <v lo> <v hi> <file> [<word value hex|any>]
//     main-trace mode.  <file> (tests/redraw_checks.py write_search_file; little-endian u32 words): magic 0x4c4d4e52,
//     encoding (64|37), number of draws, the channel's digest after the claims (8 words), log2 of the leaf count n, number of
//     leaf columns c, then c columns of n words (the base LDE, in leaf order) and c columns of n words (the LDE of the unit
//     change).  A trial is base + v * delta mod P, the Merkle root of oracle/merkle.py over these equal-size columns
//     (leaf = H(row), node = H(left || right)), mix_root, then the draws with a running counter.  Finds the v in [lo, hi)
//     for which draw number <set> (0-based) redraws once (on the given word value, if one is given) and no other draw of
//     the step does.  A word value below 2P (7FFFFFFF, FFFFFFFD) asks for an accepted draw that holds it instead, in draw
//     <set> or, with <set> = -1, in any: no draw of the step redraws.  (A kind-1 draw uses all eight words.)
//   find_redraw trace-root <file> <v>
//     the root of that trial alone, to compare with the oracle's before a search is started.
//
// The commands that made the committed records (8 threads, seed 1; what each took is in docs/HISTORY.md section 11).  Chain
// records: one command per entry of fri_checks.REDRAW_SEARCHES, which lists the event, the trees, the word value and the
// index range; `python tests/fri_checks.py commands` prints all twelve in full, with the roots of the reference:
//   find_redraw chain "<search name>" <64|37> <event> <trees> <value|any> <lo> <hi> 8 1 $(python tests/fri_checks.py roots "<search name>")
// Trace records (the input file first: `python tests/redraw_checks.py "<record name>" <file>`):
//   find_redraw trace "add8 inputs first set" 0 8 0 2147483647 a64.bin
//   find_redraw trace "add8 inputs first set u32" 0 8 0 2147483647 a37.bin
//   find_redraw trace "add8 inputs last set" 4 8 0 2147483647 a64.bin        (in two runs: [0, 250000000) without a hit, then from there)
//   find_redraw trace "add8 inputs last set u32" 4 8 0 2147483647 a37.bin
//   find_redraw trace "add8 inputs word P" -1 8 0 2147483647 a64.bin 7FFFFFFF
// (a64.bin: the input written for "add8 inputs first set", a37.bin: for "add8 inputs first set u32"; the records of one
// encoding share their input.)
// A trace record in the file also carries claims_digest (words 3 .. 10 of the input file), variant (redraw_checks.VARIANTS)
// and pie (the recipe: redraw_checks' constants), added when the line is put into the file; "trials" is the searcher's count.
#include <algorithm>
#include <array>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {
constexpr uint32_t P = 0x7fffffffu;
constexpr uint32_t IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
constexpr uint8_t SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// one unkeyed Blake2s-256 over a single block: m holds the message zero-padded to 64 bytes, len its length in bytes (<= 64)
inline void blake2s_block(uint32_t out[8], const uint32_t m[16], uint32_t len) {
  uint32_t v[16];
  for (int i = 0; i < 8; ++i) v[i] = IV[i];
  v[0] ^= 0x01010020u;
  uint32_t h[8];
  for (int i = 0; i < 8; ++i) h[i] = v[i];
  for (int i = 0; i < 8; ++i) v[8 + i] = IV[i];
  v[12] ^= len;
  v[14] ^= 0xffffffffu;
#define G(a, b, c, d, x, y)       \
  v[a] = v[a] + v[b] + (x);       \
  v[d] = rotr(v[d] ^ v[a], 16);   \
  v[c] = v[c] + v[d];             \
  v[b] = rotr(v[b] ^ v[c], 12);   \
  v[a] = v[a] + v[b] + (y);       \
  v[d] = rotr(v[d] ^ v[a], 8);    \
  v[c] = v[c] + v[d];             \
  v[b] = rotr(v[b] ^ v[c], 7);
#pragma GCC unroll 10
  for (int r = 0; r < 10; ++r) {
    const uint8_t* s = SIGMA[r];
    G(0, 4, 8, 12, m[s[0]], m[s[1]]);
    G(1, 5, 9, 13, m[s[2]], m[s[3]]);
    G(2, 6, 10, 14, m[s[4]], m[s[5]]);
    G(3, 7, 11, 15, m[s[6]], m[s[7]]);
    G(0, 5, 10, 15, m[s[8]], m[s[9]]);
    G(1, 6, 11, 12, m[s[10]], m[s[11]]);
    G(2, 7, 8, 13, m[s[12]], m[s[13]]);
    G(3, 4, 9, 14, m[s[14]], m[s[15]]);
  }
#undef G
  for (int i = 0; i < 8; ++i) out[i] = h[i] ^ v[i] ^ v[8 + i];
}

// digest <- H(digest || root)
inline void mix_root(uint32_t d[8], const uint32_t root[8]) {
  uint32_t m[16];
  memcpy(m, d, 32);
  memcpy(m + 8, root, 32);
  blake2s_block(d, m, 64u);
}
// the eight words of draw number ctr: H(digest || u64 counter padded to 32 bytes) or H(digest || u32 counter || 0x00)
inline void draw_words(uint32_t w[8], const uint32_t d[8], uint32_t ctr, uint32_t enc) {
  uint32_t m[16] = {0};
  memcpy(m, d, 32);
  m[8] = ctr;
  blake2s_block(w, m, enc);
}
inline bool all_accepted(const uint32_t w[8]) {
  bool ok = true;
  for (int k = 0; k < 8; ++k) ok = ok && w[k] < 0xFFFFFFFEu;
  return ok;
}
inline bool has_edge(const uint32_t w[8]) {   // an accepted draw that still meets an edge
  bool e = false;
  for (int k = 0; k < 8; ++k) e = e || w[k] == 0xFFFFFFFDu || (k < 4 && w[k] == P);
  return e;
}

std::string hex(const uint32_t* w, int n) {
  std::string s;
  char b[3];
  const uint8_t* p = reinterpret_cast<const uint8_t*>(w);
  for (int i = 0; i < 4 * n; ++i) {
    snprintf(b, sizeof b, "%02x", p[i]);
    s += b;
  }
  return s;
}
bool unhex(const char* s, uint32_t w[8]) {
  if (strlen(s) != 64) return false;
  uint8_t* p = reinterpret_cast<uint8_t*>(w);
  for (int i = 0; i < 32; ++i)
    if (sscanf(s + 2 * i, "%2hhx", &p[i]) != 1) return false;
  return true;
}

enum Event { REDRAW, ACCEPT_EDGE, REDUCE_EDGE };
const char* EVENT_NAMES[] = {"redraw", "accept-edge", "reduce-edge"};

int usage(const char* a0) {
  fprintf(stderr,
          "usage: %s chain <name> <64|37> <redraw|accept-edge|reduce-edge> <layers j,j,..> <word value hex|any> <idx lo> <idx hi> "
          "<threads> <seed> <root hex>...\n       %s trace <name> <set> <threads> <v lo> <v hi> <file> [<word value hex|any>]\n       %s trace-root <file> <v>\n",
          a0, a0, a0);
  return 2;
}

int run_chain(int argc, char** argv) {
  if (argc < 12) return usage(argv[0]);
  const std::string name = argv[2];
  const uint32_t enc = (uint32_t)atoi(argv[3]);
  int ev = -1;
  for (int e = 0; e < 3; ++e)
    if (!strcmp(argv[4], EVENT_NAMES[e])) ev = e;
  const bool any_value = !strcmp(argv[6], "any");
  const uint32_t value = any_value ? 0u : (uint32_t)strtoul(argv[6], nullptr, 16);
  const int lo = atoi(argv[7]), hi = atoi(argv[8]), nthreads = atoi(argv[9]);
  const uint64_t seed = strtoull(argv[10], nullptr, 0);
  std::vector<std::array<uint32_t, 8>> roots;
  for (int i = 11; i < argc; ++i) {
    std::array<uint32_t, 8> r;
    if (!unhex(argv[i], r.data())) return usage(argv[0]);
    roots.push_back(r);
  }
  const int L = (int)roots.size();
  std::vector<std::atomic<int>> wanted(L);
  for (auto& w : wanted) w = 0;
  int n_wanted = 0;
  for (char* t = strtok(argv[5], ","); t; t = strtok(nullptr, ",")) {
    const int j = atoi(t);
    if (j < 0 || j >= L) return usage(argv[0]);
    if (!wanted[j].exchange(1)) ++n_wanted;
  }
  if ((enc != 64 && enc != 37) || ev < 0 || lo < 0 || hi > 7 || lo > hi || nthreads < 1 || nthreads > 64 || !n_wanted ||
      (ev == REDUCE_EDGE && hi > 3))
    return usage(argv[0]);
  const uint32_t edge_value = ev == ACCEPT_EDGE ? 0xFFFFFFFDu : P;
  std::atomic<int> left{n_wanted};
  std::atomic<uint64_t> next{0};
  std::mutex out;
  constexpr uint64_t CHUNK = 1u << 16;
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; ++t)
    pool.emplace_back([&] {
      while (left.load() > 0) {
        const uint64_t c0 = next.fetch_add(CHUNK);
        for (uint64_t c = c0; c < c0 + CHUNK; ++c) {
          // the start digest: any 32 bytes will do, they are hashed with the first root at once
          uint32_t start[8] = {0x6e646572u, 0x20776172u, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)c, (uint32_t)(c >> 32), 0u, 0u};
          uint32_t d[8], w[8];
          memcpy(d, start, 32);
          int at = -1, idx = -1;
          uint32_t val = 0;
          bool good = true;
          for (int j = 0; j < L && good; ++j) {
            mix_root(d, roots[j].data());
            draw_words(w, d, 0u, enc);
            if (ev == REDRAW) {
              if (all_accepted(w)) {
                good = !has_edge(w);
                continue;
              }
              if (at >= 0 || !wanted[j].load(std::memory_order_relaxed)) {
                good = false;
                break;
              }
              int found = -1;
              for (int k = 0; k < 8; ++k)
                if (w[k] >= 0xFFFFFFFEu) {
                  if (k < lo || k > hi) good = false;
                  if (found < 0 && (any_value || w[k] == value)) found = k;
                }
              if (found < 0) good = false;
              if (!good) break;
              at = j, idx = found, val = w[found];
              draw_words(w, d, 1u, enc);
              good = all_accepted(w) && !has_edge(w);
            } else {
              if (!all_accepted(w)) {
                good = false;
                break;
              }
              if (!has_edge(w)) continue;
              if (at >= 0 || !wanted[j].load(std::memory_order_relaxed)) {
                good = false;
                break;
              }
              int found = -1, n_edges = 0;
              for (int k = 0; k < 8; ++k) {
                const bool e = w[k] == 0xFFFFFFFDu || (k < 4 && w[k] == P);
                n_edges += e;
                if (e && w[k] == edge_value && k >= lo && k <= hi) found = k;
              }
              if (found < 0 || n_edges != 1) {
                good = false;
                break;
              }
              at = j, idx = found, val = w[found];
            }
          }
          if (!good || at < 0) continue;
          if (!wanted[at].exchange(0)) continue;   // another thread was first
          {
            std::lock_guard<std::mutex> g(out);
            std::string rs;
            for (int j = 0; j < L; ++j) rs += std::string(j ? ", " : "") + "\"" + hex(roots[j].data(), 8) + "\"";
            printf("{\"name\": \"%s\", \"mode\": \"chain\", \"encoding\": %u, \"event\": \"%s\", \"roots\": [%s], \"digest\": \"%s\", "
                   "\"layer\": %d, \"word_index\": %d, \"word_value\": \"0x%08X\", \"counters\": [%s], \"trials\": %llu}\n",
                   name.c_str(), enc, EVENT_NAMES[ev], rs.c_str(), hex(start, 8).c_str(), at, idx, val,
                   ev == REDRAW ? "0, 1" : "0", (unsigned long long)c);
            fflush(stdout);
          }
          left.fetch_sub(1);
        }
      }
    });
  for (auto& th : pool) th.join();
  return 0;
}

// ---- main-trace mode
struct TraceFile {
  uint32_t enc = 0, n_draws = 0, digest[8] = {0}, log_n = 0, n_cols = 0;
  std::vector<uint32_t> base, delta;   // column-major: column c at [c * n, (c + 1) * n)
};

bool read_trace_file(const char* path, TraceFile& f) {
  FILE* fp = fopen(path, "rb");
  if (!fp) return false;
  uint32_t head[13];
  bool ok = fread(head, 4, 13, fp) == 13 && head[0] == 0x4c4d4e52u;
  if (ok) {
    f.enc = head[1];
    f.n_draws = head[2];
    memcpy(f.digest, head + 3, 32);
    f.log_n = head[11];
    f.n_cols = head[12];
    ok = (f.enc == 64 || f.enc == 37) && f.n_draws >= 1 && f.n_draws <= 16 && f.log_n <= 20 && f.n_cols >= 1 && f.n_cols <= 4096;
  }
  if (ok) {
    const size_t words = (size_t)f.n_cols << f.log_n;
    f.base.resize(words);
    f.delta.resize(words);
    ok = fread(f.base.data(), 4, words, fp) == words && fread(f.delta.data(), 4, words, fp) == words;
  }
  fclose(fp);
  return ok;
}

// general Blake2s-256 of n words (n >= 0)
void blake2s_words(uint32_t out[8], const uint32_t* w, size_t n) {
  if (n <= 16) {
    uint32_t m[16] = {0};
    memcpy(m, w, 4 * n);
    blake2s_block(out, m, (uint32_t)(4 * n));
    return;
  }
  // multi-block: restate the compression with a running state
  uint32_t h[8];
  for (int i = 0; i < 8; ++i) h[i] = IV[i];
  h[0] ^= 0x01010020u;
  const size_t blocks = (n + 15) / 16;
  for (size_t b = 0; b < blocks; ++b) {
    uint32_t m[16] = {0};
    const size_t k = std::min<size_t>(16, n - 16 * b);
    memcpy(m, w + 16 * b, 4 * k);
    const bool last = b + 1 == blocks;
    uint32_t v[16];
    for (int i = 0; i < 8; ++i) v[i] = h[i], v[8 + i] = IV[i];
    v[12] ^= (uint32_t)(last ? 4 * n : 64 * (b + 1));
    if (last) v[14] ^= 0xffffffffu;
    for (int r = 0; r < 10; ++r) {
      const uint8_t* s = SIGMA[r];
      auto G = [&](int a, int bb, int c, int d, uint32_t x, uint32_t y) {
        v[a] = v[a] + v[bb] + x;
        v[d] = rotr(v[d] ^ v[a], 16);
        v[c] = v[c] + v[d];
        v[bb] = rotr(v[bb] ^ v[c], 12);
        v[a] = v[a] + v[bb] + y;
        v[d] = rotr(v[d] ^ v[a], 8);
        v[c] = v[c] + v[d];
        v[bb] = rotr(v[bb] ^ v[c], 7);
      };
      G(0, 4, 8, 12, m[s[0]], m[s[1]]);
      G(1, 5, 9, 13, m[s[2]], m[s[3]]);
      G(2, 6, 10, 14, m[s[4]], m[s[5]]);
      G(3, 7, 11, 15, m[s[6]], m[s[7]]);
      G(0, 5, 10, 15, m[s[8]], m[s[9]]);
      G(1, 6, 11, 12, m[s[10]], m[s[11]]);
      G(2, 7, 8, 13, m[s[12]], m[s[13]]);
      G(3, 4, 9, 14, m[s[14]], m[s[15]]);
    }
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[8 + i];
  }
  memcpy(out, h, 32);
}

// the Merkle root of base + v * delta; lv, up: scratch of 8 n words each, rw of n_cols
const uint32_t* trace_root(const TraceFile& f, uint64_t v, uint32_t* lv, uint32_t* up, uint32_t* rw) {
  const size_t n = (size_t)1 << f.log_n, nc = f.n_cols;
  for (size_t r = 0; r < n; ++r) {
    for (size_t c = 0; c < nc; ++c) rw[c] = (uint32_t)((f.base[c * n + r] + v * f.delta[c * n + r]) % P);
    blake2s_words(&lv[8 * r], rw, nc);
  }
  const uint32_t* cur = lv;
  for (size_t sz = n >> 1; sz >= 1; sz >>= 1) {   // the level of sz nodes lies at up[8 sz .. 16 sz)
    for (size_t i = 0; i < sz; ++i) blake2s_block(&up[8 * (sz + i)], cur + 16 * i, 64u);
    cur = &up[8 * sz];
  }
  return cur;
}

int run_trace(int argc, char** argv) {
  TraceFile f;
  if (argc == 4 && !strcmp(argv[1], "trace-root")) {   // the root alone, to compare with the oracle's before a search
    if (!read_trace_file(argv[2], f)) return usage(argv[0]);
    const size_t n = (size_t)1 << f.log_n;
    std::vector<uint32_t> lv(8 * n), up(16 * n), rw(f.n_cols);
    printf("%s\n", hex(trace_root(f, strtoull(argv[3], nullptr, 0), lv.data(), up.data(), rw.data()), 8).c_str());
    return 0;
  }
  if (argc != 8 && argc != 9) return usage(argv[0]);
  const std::string name = argv[2];
  const int set = atoi(argv[3]), nthreads = atoi(argv[4]);
  const bool any_value = argc == 8 || !strcmp(argv[8], "any");
  const uint32_t value = any_value ? 0u : (uint32_t)strtoul(argv[8], nullptr, 16);
  const bool edge = !any_value && value < 0xFFFFFFFEu;
  const uint64_t vlo = strtoull(argv[5], nullptr, 0), vhi = strtoull(argv[6], nullptr, 0);
  if (!read_trace_file(argv[7], f) || (set < 0 && !edge) || set >= (int)f.n_draws || nthreads < 1 || nthreads > 64 || vhi > P || vlo >= vhi)
    return usage(argv[0]);
  const size_t n = (size_t)1 << f.log_n;
  std::atomic<uint64_t> next{vlo};
  std::atomic<bool> done{false};
  constexpr uint64_t CHUNK = 1u << 10;
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; ++t)
    pool.emplace_back([&] {
      std::vector<uint32_t> lv(8 * n), up(16 * n), rw(f.n_cols);
      while (!done.load()) {
        const uint64_t c0 = next.fetch_add(CHUNK);
        if (c0 >= vhi) return;
        for (uint64_t v = c0; v < std::min(c0 + CHUNK, vhi); ++v) {
          const uint32_t* root = trace_root(f, v, lv.data(), up.data(), rw.data());
          uint32_t d[8], w[8];
          memcpy(d, f.digest, 32);
          mix_root(d, root);
          uint32_t ctr = 0;
          int at = -1, idx = -1;
          uint32_t val = 0, c_at = 0;
          bool good = true;
          for (uint32_t s = 0; s < f.n_draws && good; ++s) {
            draw_words(w, d, ctr++, f.enc);
            if (edge) {   // an accepted word: no draw of the step redraws, the first draw (of `set`, if given) that holds it counts
              good = all_accepted(w);
              for (int k = 7; k >= 0 && good && at < 0; --k)
                if (w[k] == value && (set < 0 || (int)s == set)) idx = k, val = w[k];
              if (idx >= 0 && at < 0) at = (int)s, c_at = ctr - 1;
              continue;
            }
            if (all_accepted(w)) continue;
            if ((int)s != set) {
              good = false;
              break;
            }
            for (int k = 7; k >= 0; --k)
              if (w[k] >= 0xFFFFFFFEu && (any_value || w[k] == value)) idx = k, val = w[k];
            if (idx < 0) {
              good = false;
              break;
            }
            at = (int)s, c_at = ctr - 1;
            draw_words(w, d, ctr++, f.enc);
            good = all_accepted(w);
          }
          if (!good || at < 0 || done.exchange(true)) continue;
          printf("{\"name\": \"%s\", \"mode\": \"trace\", \"encoding\": %u, \"event\": \"%s\", \"value\": %llu, \"set\": %d, "
                 "\"n_draws\": %u, \"word_index\": %d, \"word_value\": \"0x%08X\", \"counters\": [%s], \"root\": \"%s\", "
                 "\"trials\": %llu}\n",
                 name.c_str(), f.enc, !edge ? "redraw" : value == P ? "reduce-edge" : "accept-edge", (unsigned long long)v, at, f.n_draws,
                 idx, val, (std::to_string(c_at) + (edge ? "" : ", " + std::to_string(c_at + 1))).c_str(), hex(root, 8).c_str(),
                 (unsigned long long)(v - vlo));
          fflush(stdout);
          return;
        }
      }
    });
  for (auto& th : pool) th.join();
  return done.load() ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "chain")) return run_chain(argc, argv);
  if (argc >= 2 && (!strcmp(argv[1], "trace") || !strcmp(argv[1], "trace-root"))) return run_trace(argc, argv);
  return usage(argv[0]);
}
