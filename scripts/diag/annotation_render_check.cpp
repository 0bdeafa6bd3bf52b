// annotation_render_check.cpp — the render side of csrc/annotation_fixed.h and the host entry
// point pas_gas_annotation_render in a program of their own, for a build under ASan + UBSan
// (tests/test_gas_annotation_render.py).  Seeded random binds are rendered into heap buffers of
// exactly the reported size, so a byte written past the annotation is a sanitizer report, and
// compared with a restated bindNode join (scheduler.go:317-335); the parser reads them back.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "pas.h"

static int fail(const char* what, int it) {
  std::fprintf(stderr, "FAIL %s at iteration %d\n", what, it);
  return 1;
}

int main() {
  std::mt19937_64 rng(317);
  const int kIterations = 20000;
  for (int it = 0; it < kIterations; ++it) {
    const int32_t k = 1 + (int32_t)(rng() % 9), nc = (int32_t)(rng() % 5);
    const int32_t n_cards = (int32_t)(rng() % (k + 2)) - 1;  // -1 .. k
    std::vector<std::string> names(k);
    std::vector<int64_t> off(k + 1, 0);
    std::string blob;
    for (int32_t c = 0; c < k; ++c) {
      const int len = (int)(rng() % 4) == 0 ? 0 : 1 + (int)(rng() % 7);
      for (int i = 0; i < len; ++i) {
        char ch = (char)(rng() % 256);
        names[c].push_back(ch == ',' || ch == '|' ? 'x' : ch);
      }
      blob += names[c];
      off[c + 1] = (int64_t)blob.size();
    }
    std::vector<int64_t> counts((size_t)nc * k, 0);
    const int64_t L = n_cards < 0 ? 0 : n_cards;
    bool bad = false;
    for (auto& v : counts)
      if (rng() % 3 == 0) v = (int64_t)(rng() % 4);
    if (rng() % 16 == 0 && !counts.empty())
      counts[rng() % counts.size()] = -1 - (int64_t)(rng() % 3);
    std::string want;
    for (int32_t c = 0; c < nc; ++c) {
      if (c) want += '|';
      bool first = true;
      for (int32_t j = 0; j < k; ++j) {
        const int64_t v = counts[(size_t)c * k + j];
        if (v < 0 || (v > 0 && j >= L)) bad = true;
        for (int64_t r = 0; r < v; ++r) {
          if (!first) want += ',';
          want += names[j];
          first = false;
        }
      }
    }
    int32_t status = -9;
    int64_t n = -9;
    int rc = pas_gas_annotation_render(nc, k, n_cards, counts.data(), off.data(), blob.data(),
                                       &status, nullptr, 0, &n);
    if (bad) {
      if (rc != PAS_OK || status != PAS_GAS_ERR_INPUT || n != 0) return fail("input status", it);
      continue;
    }
    if (status != PAS_GAS_OK || n != (int64_t)want.size()) return fail("length", it);
    if (rc != (n > 0 ? PAS_ECAPACITY : PAS_OK)) return fail("sizing call", it);
    std::vector<char> out((size_t)n);  // exactly the room: ASan sees one byte more
    rc = pas_gas_annotation_render(nc, k, n_cards, counts.data(), off.data(), blob.data(), &status,
                                   out.data(), n, &n);
    if (rc != PAS_OK || std::string(out.begin(), out.end()) != want) return fail("bytes", it);
    if (n > 0) {
      std::vector<char> small((size_t)n - 1);
      rc = pas_gas_annotation_render(nc, k, n_cards, counts.data(), off.data(), blob.data(),
                                     &status, small.data(), n - 1, &n);
      if (rc != PAS_ECAPACITY) return fail("short cap", it);
    }
    int64_t segs = 0, listed = 0, total = 0;
    for (int64_t v : counts) total += v;
    rc = pas_gas_annotation_parse(out.data(), n, 0, &segs, nullptr, &listed, nullptr, 0);
    if (rc != PAS_OK || segs != (nc > 0 ? nc : 1)) return fail("segments", it);
    // (a segment of one empty name reads back as no card: listed may only fall short by those)
    if (listed > total) return fail("listed", it);
  }
  // saturation: no buffer is touched
  int32_t status = -9;
  int64_t n = -9;
  const int64_t huge[2] = {INT64_MAX, INT64_MAX}, off2[3] = {0, 3, 3};
  int rc = pas_gas_annotation_render(1, 2, 2, huge, off2, "abc", &status, nullptr, 0, &n);
  if (rc != PAS_OK || status != PAS_GAS_ERR_OVERFLOW || n != 0) return fail("overflow", -1);
  std::printf("ok: %d random binds\n", kIterations);
  return 0;
}
