// Stand-alone check of csrc/annotation_fixed.h and its host entry point (csrc/gas_annotation.cpp)
// under ASan + UBSan: a program of its own, nothing preloaded, nothing loaded into Python.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Iplatform-aware-scheduling_amd/csrc scripts/diag/annotation_parse_check.cpp \
//       platform-aware-scheduling_amd/csrc/gas_annotation.cpp -o annotation_parse_check
//   annotation_parse_check [n_random = 100000]
// Every annotation is parsed out of a heap copy of exactly its length, and the output arrays
// have exactly max_containers / cap entries, so a read or write past either end is a sanitizer
// report.  The reference is strings.Split restated with std::string::find
// (node_resource_cache.go:241,253-256).  Exit status 0 and "ok" when everything agrees.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "annotation_fixed.h"
#include "pas.h"

namespace {

std::vector<std::string> go_split(const std::string& s, char sep) {
  std::vector<std::string> out;
  size_t at = 0;
  for (;;) {
    const size_t hit = s.find(sep, at);
    if (hit == std::string::npos) break;
    out.push_back(s.substr(at, hit - at));
    at = hit + 1;
  }
  out.push_back(s.substr(at));
  return out;
}

struct Collect {
  std::vector<int64_t> per_segment;
  std::vector<std::string> names;
  std::vector<int64_t> name_segment;
  const char* p;
  void name(int64_t j, int64_t c, int64_t beg, int64_t len) {
    if (j != (int64_t)names.size()) std::abort();
    names.emplace_back(p + beg, (size_t)len);
    name_segment.push_back(c);
  }
  void segment(int64_t c, int64_t n) {
    if (c != (int64_t)per_segment.size()) std::abort();
    per_segment.push_back(n);
  }
};

int64_t failures = 0;

void fail(const std::string& a, const char* what) {
  if (++failures <= 10) std::fprintf(stderr, "mismatch (%s) on %zu bytes\n", what, a.size());
}

void check(const std::string& a, int32_t max_containers, int64_t cap) {
  // the reference
  std::vector<int64_t> want_seg;
  std::vector<std::string> want_names;
  for (const std::string& seg : go_split(a, '|')) {
    const std::vector<std::string> names = seg.empty() ? std::vector<std::string>{}
                                                       : go_split(seg, ',');
    want_seg.push_back((int64_t)names.size());
    want_names.insert(want_names.end(), names.begin(), names.end());
  }
  // the walk, on a heap copy of exactly the annotation's bytes
  std::vector<char> heap(a.begin(), a.end());
  const char* p = heap.empty() ? nullptr : heap.data();
  Collect c{{}, {}, {}, p};
  const pas::AnnotationCounts r = pas::annotation_walk(p, (int64_t)heap.size(), c);
  if (r.n_segments != (int64_t)want_seg.size() || c.per_segment != want_seg) fail(a, "segments");
  if (r.n_listed != (int64_t)want_names.size() || c.names != want_names) fail(a, "names");
  const pas::AnnotationCounts r2 = pas::annotation_counts(p, (int64_t)heap.size());
  if (r2.n_segments != r.n_segments || r2.n_listed != r.n_listed) fail(a, "count pass");
  // the host entry point with exactly-sized outputs
  std::vector<int32_t> cpc((size_t)max_containers, -7);
  std::vector<int64_t> span((size_t)cap * 2, -7);
  int64_t n_seg = -1, n_listed = -1;
  const int rc = pas_gas_annotation_parse(p, (int64_t)heap.size(), max_containers, &n_seg,
                                          cpc.empty() ? nullptr : cpc.data(), &n_listed,
                                          span.empty() ? nullptr : span.data(), cap);
  if (rc != PAS_OK || n_seg != r.n_segments || n_listed != r.n_listed) fail(a, "entry point");
  for (int64_t s = 0; s < max_containers; ++s)
    if (cpc[s] != (s < n_seg ? (int32_t)want_seg[s] : -7)) fail(a, "cards_per_container");
  for (int64_t j = 0; j < cap; ++j) {
    if (j >= n_listed) {
      if (span[2 * j] != -7 || span[2 * j + 1] != -7) fail(a, "span past the names");
    } else if (span[2 * j] < 0 || span[2 * j + 1] < 0 ||
               span[2 * j] + span[2 * j + 1] > (int64_t)a.size() ||
               a.substr((size_t)span[2 * j], (size_t)span[2 * j + 1]) != want_names[j]) {
      fail(a, "name_span");
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  const int64_t n_random = argc > 1 ? std::atoll(argv[1]) : 100000;
  const std::string long_name(300, 'x');
  const std::vector<std::string> fixed = {
      "", "|", "||", ",", "a,", ",a", "a,,b", "a|", "|a", "card1,card10|card100", long_name,
      long_name + "," + long_name + "|" + long_name, std::string("a\0b,\0|\0", 7),
      "\xc3\xa9,\xff|\x80", "a|b|c|d|e|f|g|h", "a,b,c,d,e,f,g,h,i,j"};
  for (const std::string& a : fixed)
    for (int32_t mc : {0, 1, 2, 16})
      for (int64_t cap : {0, 1, 3, 400}) check(a, mc, cap);
  // seeded random strings over {a, b, 1, ',', '|', 0x00, 0xC3}
  const char alphabet[7] = {'a', 'b', '1', ',', '|', '\0', '\xc3'};
  uint64_t x = 0x9e3779b97f4a7c15ull;
  auto next = [&x]() {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;  // xorshift64
    return x;
  };
  for (int64_t i = 0; i < n_random; ++i) {
    std::string a((size_t)(next() % 24), 'a');
    for (char& ch : a) ch = alphabet[next() % 7];
    check(a, (int32_t)(next() % 5), (int64_t)(next() % 9));
  }
  if (failures) {
    std::fprintf(stderr, "%" PRId64 " mismatches\n", failures);
    return 1;
  }
  std::printf("ok: %zu fixed cases x 16 shapes, %" PRId64 " random strings\n", fixed.size(),
              n_random);
  return 0;
}
