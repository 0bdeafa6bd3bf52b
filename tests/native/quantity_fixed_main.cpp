// Stand-alone driver of csrc/quantity_fixed.h for tests/test_quantity_fixed.py: built with the
// host compiler under ASan + UBSan and run as a program of its own.
//   quantity_fixed_main <corpus>     corpus: records of int32 length + that many bytes
// prints "status whole nano decimals fit" per record.  Each literal is parsed out of a heap
// copy of exactly its length, so a read past either end of the span is a sanitizer report.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "quantity_fixed.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t len;
  while (std::fread(&len, sizeof(len), 1, f) == 1) {
    if (len < 0) return 2;
    std::vector<char> lit((size_t)len);
    if (len && std::fread(lit.data(), 1, (size_t)len, f) != (size_t)len) return 2;
    const pas::QuantityFixed r = pas::parse_quantity_fixed(lit.data(), len);
    std::printf("%d %" PRId64 " %u %d %d\n", r.status, r.whole, r.nano, r.decimals, r.fit);
  }
  std::fclose(f);
  return 0;
}
