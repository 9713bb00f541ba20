// Exhaustive host search for the smallest proof-of-work nonce (Channel::grind of csrc/host.h) on many threads: finds the
// pinned vectors of tests/test_gpu_pow.py (a minimal nonce above 2^32) and proves their minimality, since every nonce
// below the answer is examined.  Build and run:
//   g++ -std=c++20 -O3 -DLMN_EMU -pthread -I luminair_amd/csrc tools/pow_exhaustive.cpp -o tools/bin/pow_exhaustive
//   tools/bin/pow_exhaustive <digest hex, 64 chars> <pow_bits> <protocol_variant> [threads=16]
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "host.h"

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <digest hex> <pow_bits> <protocol_variant> [threads]\n", argv[0]);
    return 2;
  }
  lmn::Hash32 d;
  uint8_t* b = reinterpret_cast<uint8_t*>(d.w);
  for (int i = 0; i < 32; ++i) sscanf(argv[1] + 2 * i, "%2hhx", &b[i]);
  const uint32_t pow_bits = (uint32_t)atoi(argv[2]);
  lmn::Channel ch((uint32_t)strtoul(argv[3], nullptr, 0));
  ch.set_digest(d);
  const int nthreads = argc > 4 ? atoi(argv[4]) : 16;
  constexpr uint64_t CHUNK = 1u << 20;
  std::atomic<uint64_t> next{0}, best{~0ull};
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; ++t)
    pool.emplace_back([&] {
      for (;;) {
        const uint64_t lo = next.fetch_add(CHUNK);
        if (lo >= best.load()) return;   // every chunk below the best has been claimed by some thread
        for (uint64_t n = lo; n < lo + CHUNK; ++n)
          if (ch.verify_pow_nonce(pow_bits, n)) {
            uint64_t cur = best.load();
            while (n < cur && !best.compare_exchange_weak(cur, n)) {
            }
            break;
          }
      }
    });
  for (auto& th : pool) th.join();
  printf("%llu\n", (unsigned long long)best.load());
  return 0;
}
