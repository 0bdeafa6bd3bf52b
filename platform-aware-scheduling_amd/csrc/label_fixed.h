// label_fixed.h — the "gpu.intel.com/cards" label grammar in fixed-width state, for host and
// device code (plain C++ as well: no HIP header is needed to include this file).
//
// getNodeGPUList reads the label with one strings.Split on "."
// (gpu-aware-scheduling/pkg/gpuscheduler/scheduler.go:132-148), and Go's Split of the empty
// string gives one empty string, so
//   pieces (gpuCount)  = 1 + count('.')      duplicates and empty names included
//   cards              = the distinct pieces in sort.Strings order: bytewise, and a name sorts
//                        before any name it is a prefix of ("" < "card1" < "card10" < "card2")
// Names are opaque bytes: byte 0 and bytes >= 0x80 have no meaning here, only '.'.
//
// Nothing is stored per piece.  label_next finds the card that follows a given one in rank order
// with one pass over the label, so the cards are visited in rank order by calling it again and
// again: a label of B bytes costs O(B) per card, and a caller that stops at
// PAS_GAS_MAX_CARDS + 1 cards (label_count) pays at most 65 passes whatever the label holds.
#pragma once

#include <cstdint>

#include "pas.h"

#if defined(__HIP__)
#define PAS_LF_HD __host__ __device__
#else
#define PAS_LF_HD
#endif

namespace pas {

// a[0 .. an) against b[0 .. bn) as sort.Strings orders them: < 0, 0, > 0
PAS_LF_HD inline int label_name_cmp(const char* a, int64_t an, const char* b, int64_t bn) {
  const int64_t n = an < bn ? an : bn;
  for (int64_t i = 0; i < n; ++i) {
    const unsigned char x = (unsigned char)a[i], y = (unsigned char)b[i];
    if (x != y) return x < y ? -1 : 1;
  }
  return an < bn ? -1 : an > bn ? 1 : 0;
}

// 1 + count('.')
PAS_LF_HD inline int64_t label_pieces(const char* p, int64_t n) {
  int64_t pieces = 1;
  for (int64_t i = 0; i < n; ++i) pieces += p[i] == '.';
  return pieces;
}

// The least piece of the label p[0 .. n) above the name p[prev_beg .. prev_beg + prev_len)
// (has_prev false: the least piece of all) into *beg / *len; false when there is none.  Of
// equal pieces the first is reported.
PAS_LF_HD inline bool label_next(const char* p, int64_t n, bool has_prev, int64_t prev_beg,
                                 int64_t prev_len, int64_t* beg, int64_t* len) {
  bool found = false;
  int64_t bb = 0, bl = 0, pb = 0;
  for (int64_t i = 0; i <= n; ++i) {
    if (i < n && p[i] != '.') continue;
    const int64_t pl = i - pb;
    if ((!has_prev || label_name_cmp(p + pb, pl, p + prev_beg, prev_len) > 0) &&
        (!found || label_name_cmp(p + pb, pl, p + bb, bl) < 0)) {
      found = true;
      bb = pb;
      bl = pl;
    }
    pb = i + 1;
  }
  *beg = bb;
  *len = bl;
  return found;
}

// The distinct pieces of the label, counted up to `stop` (the count is min(distinct, stop))
PAS_LF_HD inline int32_t label_count(const char* p, int64_t n, int32_t stop) {
  int32_t cards = 0;
  int64_t b = 0, l = 0;
  while (cards < stop && label_next(p, n, cards > 0, b, l, &b, &l)) ++cards;
  return cards;
}

// Whether a piece of the label equals q[0 .. qn)
PAS_LF_HD inline bool label_lists(const char* p, int64_t n, const char* q, int64_t qn) {
  int64_t pb = 0;
  for (int64_t i = 0; i <= n; ++i) {
    if (i < n && p[i] != '.') continue;
    if (i - pb == qn) {
      int64_t j = 0;
      while (j < qn && p[pb + j] == q[j]) ++j;
      if (j == qn) return true;
    }
    pb = i + 1;
  }
  return false;
}

}  // namespace pas
