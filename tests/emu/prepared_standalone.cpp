// Stand-alone host program for the sanitizers (tests/emu/run_prepared_standalone.sh): settings prepared once through the C ABI
// of the emulation build compiled with -fsanitize=address,undefined - prepare, two proofs (the caller's LUT arrays
// overwritten in between), a submitted proof whose prepared handle is destroyed before the wait, destroy - and every proof
// compared with lmn_prove's bytes.  The pie is a Sin node over 20 inputs with a 32-row LUT, balanced by its SinLookup and
// Inputs tables; the LUT's second column is arbitrary data (the prover proves membership, not the function).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/luminair_hip.h"

static const uint32_t P = (1u << 31) - 1u;
static uint32_t m31(int64_t v) { return (uint32_t)(((v % (int64_t)P) + (int64_t)P) % (int64_t)P); }

#define CHECK(call)                                                                                   \
  do {                                                                                                \
    const int rc_ = (call);                                                                           \
    if (rc_ != LMN_OK) {                                                                              \
      fprintf(stderr, "%s -> %d (%s / %s)\n", #call, rc_, lmn_last_error(ctx), lmn_last_error(NULL)); \
      return 1;                                                                                       \
    }                                                                                                 \
  } while (0)

int main() {
  const int n = 20, lut_log = 5, lut_n = 1 << lut_log, lo = -16;
  std::vector<uint32_t> col0(lut_n), col1(lut_n), counts(lut_n, 0u);
  for (int i = 0; i < lut_n; ++i) {
    col0[i] = m31(lo + i);
    col1[i] = m31(3 * (int64_t)(lo + i) + 7);
  }
  std::vector<uint32_t> sin_rows, in_rows;
  for (int j = 0; j < n; ++j) {
    const int k = (j * 7) % lut_n;
    counts[k]++;
    const uint32_t last = j == n - 1 ? 1u : 0u;
    const uint32_t row[12] = {10u, 0u, (uint32_t)j, last, 10u, 0u, (uint32_t)j + 1u, col0[k], col1[k], P - 1u, 0u, 1u};
    sin_rows.insert(sin_rows.end(), row, row + 12);
    const uint32_t in[7] = {0u, (uint32_t)j, last, 0u, (uint32_t)j + 1u, col0[k], 1u};
    in_rows.insert(in_rows.end(), in, in + 7);
  }
  lmn_table tables[3];
  memset(tables, 0, sizeof tables);
  tables[0].kind = 3;    // Sin
  tables[0].n_rows = n;
  tables[0].rows = sin_rows.data();
  tables[1].kind = LMN_KIND_SIN_LOOKUP;
  tables[1].n_rows = lut_n;
  tables[1].rows = counts.data();
  tables[2].kind = 15;   // Inputs
  tables[2].n_rows = n;
  tables[2].rows = in_rows.data();
  lmn_lut lut;
  memset(&lut, 0, sizeof lut);
  lut.kind = LMN_LUT_SIN;
  lut.log_size = lut_log;
  lut.col0 = col0.data();
  lut.col1 = col1.data();
  lmn_settings settings;
  memset(&settings, 0, sizeof settings);
  settings.n_luts = 1;
  settings.luts = &lut;
  lmn_config cfg;
  lmn_default_config(&cfg);
  cfg.protocol_variant = 0x1f;   // LMN_VARIANT_PINNED: Sin has a claim slot

  lmn_ctx* ctx = NULL;
  CHECK(lmn_ctx_create(0, &cfg, &ctx));
  uint8_t *want = NULL, *got = NULL;
  size_t want_len = 0, got_len = 0;
  CHECK(lmn_prove(ctx, tables, 3, &settings, &want, &want_len));

  lmn_prepared* pp = NULL;
  CHECK(lmn_settings_prepare(0, &cfg, &settings, LMN_LOOKUP_SIN, &pp));
  if (lmn_prepared_lookups(pp) != LMN_LOOKUP_SIN) return 2;
  for (int round = 0; round < 2; ++round) {
    CHECK(lmn_prove_prepared(ctx, tables, 3, pp, &got, &got_len));
    if (got_len != want_len || memcmp(got, want, want_len) != 0) {
      fprintf(stderr, "prepared proof %d differs from lmn_prove's\n", round);
      return 3;
    }
    lmn_free(got);
    // the caller's LUT arrays are free once prepare has returned
    std::vector<uint32_t>(lut_n, 0xdeadbeefu).swap(col0);
    std::vector<uint32_t>(lut_n, 0xffffffffu).swap(col1);
  }
  uint8_t root[32];
  CHECK(lmn_prepared_root(pp, root));
  CHECK(lmn_prove_submit_prepared(ctx, tables, 3, pp));
  lmn_prepared_destroy(pp);   // the library holds its own reference until the wait
  CHECK(lmn_prove_wait(ctx, &got, &got_len));
  if (got_len != want_len || memcmp(got, want, want_len) != 0) {
    fprintf(stderr, "submitted prepared proof differs from lmn_prove's\n");
    return 4;
  }
  CHECK(lmn_verify_with_config(got, got_len, NULL, &cfg));
  bool root_in_proof = false;   // commitments[0] follows the claims, the config and the commitment count
  for (size_t o = 0; o + 32 <= got_len && !root_in_proof; ++o) root_in_proof = memcmp(got + o, root, 32) == 0;
  if (!root_in_proof) return 5;
  lmn_free(got);
  lmn_free(want);
  lmn_ctx_destroy(ctx);
  printf("prepared settings: prepare, two proofs, submit + destroy + wait, destroy: ok (%zu bytes each)\n", want_len);
  return 0;
}
