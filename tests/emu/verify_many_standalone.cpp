// Stand-alone host program for the sanitizers (tests/emu/run_verify_many_standalone.sh): lmn_verify_many through the C ABI of
// the emulation build compiled with -fsanitize=address,undefined.  The known-answer proof, its tamper matrix - per list
// that no transcript step mixes (queried values, every tree's hash and column witness, every FRI layer's witness): one
// word changed in the first, middle and last element, the last element dropped, one appended, two neighbours swapped - and
// the length edits: every length field of the proof raised and lowered by one and overwritten with large values, the bytes
// left as they are.  All cases go through ONE call; every verdict must equal lmn_verify_with_config's and nothing but the
// untouched proof may be accepted.  An index formed from proof content without a check would show here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/luminair_hip.h"

typedef std::vector<uint8_t> Bytes;

struct List {
  size_t len_off;    // where the u64 length field lies
  size_t elem;       // bytes per element
  uint64_t count;
  bool unmixed;      // no transcript step mixes the list: the device stage is what judges it
};

// walks the bincode layout of a proof with `n_slots` claim slots and records every length field
struct Walker {
  const Bytes& b;
  size_t o = 0;
  std::vector<List> lists;
  explicit Walker(const Bytes& bytes) : b(bytes) {}
  uint64_t u64() {
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) v |= (uint64_t)b.at(o + k) << (8 * k);
    o += 8;
    return v;
  }
  uint64_t list(size_t elem, bool unmixed, bool skip = true) {
    const size_t at = o;
    const uint64_t n = u64();
    lists.push_back({at, elem, n, unmixed});
    if (skip) o += (size_t)n * elem;
    return n;
  }
  void decommitment() {
    list(32, true);
    list(4, true);
  }
  void layer() {
    list(16, true);
    decommitment();
    o += 32;
  }
  void walk(int n_slots) {
    for (int i = 0; i < n_slots; ++i) o += b.at(o) ? 5 : 1;
    for (int i = 0; i < n_slots; ++i) o += b.at(o) ? 17 : 1;
    o += 3 * 4 + 8;
    list(32, false);
    const uint64_t nt = list(0, false, false);
    for (uint64_t t = 0; t < nt; ++t) {
      const uint64_t nc = list(0, false, false);
      for (uint64_t c = 0; c < nc; ++c) list(16, false);
    }
    const uint64_t nd = list(0, false, false);
    for (uint64_t t = 0; t < nd; ++t) decommitment();
    const uint64_t nq = list(0, false, false);
    for (uint64_t t = 0; t < nq; ++t) list(4, true);
    o += 8;
    layer();
    const uint64_t ni = list(0, false, false);
    for (uint64_t i = 0; i < ni; ++i) layer();
    list(16, false);
    o += 4;
  }
};

static void put_u64(Bytes& b, size_t at, uint64_t v) {
  for (int k = 0; k < 8; ++k) b[at + k] = (uint8_t)(v >> (8 * k));
}

int main(int argc, char** argv) {
  const char* path = argc > 1 ? argv[1] : "../golden/kat_simple/proof";
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 1;
  }
  Bytes kat;
  for (int c; (c = fgetc(f)) != EOF;) kat.push_back((uint8_t)c);
  fclose(f);
  Walker w(kat);
  w.walk(8);
  if (w.o != kat.size()) {
    fprintf(stderr, "the walker ends at %zu of %zu bytes\n", w.o, kat.size());
    return 1;
  }

  std::vector<Bytes> cases{kat};
  std::vector<std::string> names{"the untouched proof"};
  auto add = [&](const Bytes& b, const std::string& what) {
    cases.push_back(b);
    names.push_back(what);
  };
  for (size_t li = 0; li < w.lists.size(); ++li) {
    const List& l = w.lists[li];
    const std::string L = "list " + std::to_string(li) + " at " + std::to_string(l.len_off);
    const size_t data = l.len_off + 8;
    if (l.unmixed) {
      const size_t n = (size_t)l.count;
      for (size_t i : {(size_t)0, n / 2, n ? n - 1 : 0}) {
        if (!n) break;
        Bytes b = kat;
        b[data + i * l.elem] ^= 1u;
        add(b, L + ": element " + std::to_string(i) + " changed");
      }
      if (n) {
        Bytes b = kat;
        b.erase(b.begin() + (long)(data + (n - 1) * l.elem), b.begin() + (long)(data + n * l.elem));
        put_u64(b, l.len_off, n - 1);
        add(b, L + ": last element dropped");
      }
      {
        Bytes b = kat;
        b.insert(b.begin() + (long)(data + n * l.elem), l.elem, (uint8_t)0);
        b[data + n * l.elem] = 5u;
        put_u64(b, l.len_off, n + 1);
        add(b, L + ": one element appended");
      }
      for (size_t i = 0; i + 1 < n; ++i) {
        if (!memcmp(&kat[data + i * l.elem], &kat[data + (i + 1) * l.elem], l.elem)) continue;
        Bytes b = kat;
        for (size_t k = 0; k < l.elem; ++k) std::swap(b[data + i * l.elem + k], b[data + (i + 1) * l.elem + k]);
        add(b, L + ": elements " + std::to_string(i) + " and " + std::to_string(i + 1) + " swapped");
        break;
      }
    }
    // the length edits: the field alone
    for (uint64_t v : {l.count + 1, l.count - 1, (uint64_t)0, (uint64_t)0xffffffffu, (uint64_t)1 << 40, ~(uint64_t)0}) {
      if (v == l.count) continue;
      Bytes b = kat;
      put_u64(b, l.len_off, v);
      add(b, L + ": length " + std::to_string(l.count) + " overwritten with " + std::to_string(v));
    }
  }

  lmn_config cfg;
  lmn_default_config(&cfg);
  lmn_ctx* ctx = NULL;
  int rc = lmn_ctx_create(0, &cfg, &ctx);
  if (rc != LMN_OK) {
    fprintf(stderr, "lmn_ctx_create -> %d (%s)\n", rc, lmn_last_error(NULL));
    return 1;
  }
  const uint32_t n = (uint32_t)cases.size();
  std::vector<const uint8_t*> ptrs(n);
  std::vector<size_t> lens(n);
  for (uint32_t i = 0; i < n; ++i) {
    ptrs[i] = cases[i].data();
    lens[i] = cases[i].size();
  }
  std::vector<lmn_verify_result> res(n);
  rc = lmn_verify_many(ctx, ptrs.data(), lens.data(), n, NULL, &cfg, res.data());
  if (rc != LMN_OK) {
    fprintf(stderr, "lmn_verify_many -> %d (%s)\n", rc, lmn_last_error(ctx));
    return 1;
  }
  uint32_t device = 0, bad = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const int want = lmn_verify_with_config(ptrs[i], lens[i], NULL, &cfg);
    device += res[i].stage == 1u;
    if (res[i].rc != want || (i > 0 && res[i].rc == LMN_OK) || res[i].stage > 1u) {
      fprintf(stderr, "%s: lmn_verify_many says %d (stage %u, checks 0x%x), lmn_verify_with_config %d\n", names[i].c_str(),
              res[i].rc, res[i].stage, res[i].checks_failed, want);
      ++bad;
    }
  }
  if (res[0].rc != LMN_OK || res[0].stage != 1u) {
    fprintf(stderr, "the untouched proof: rc %d, stage %u\n", res[0].rc, res[0].stage);
    ++bad;
  }
  if (lmn_ctx_counter(ctx, 16) != device || lmn_ctx_counter(ctx, 17) != 0) {
    fprintf(stderr, "counters: %llu judged by the device stage, %llu at stage 2; results say %u\n",
            (unsigned long long)lmn_ctx_counter(ctx, 16), (unsigned long long)lmn_ctx_counter(ctx, 17), device);
    ++bad;
  }
  lmn_ctx_destroy(ctx);
  if (bad) return 2;
  printf("verify_many: %u cases in one call, %u of them judged by the device stage, every verdict equals lmn_verify_with_config's: ok\n",
         n, device);
  return 0;
}
