// quantity_fixed.h — resource.ParseQuantity of a byte span in fixed-width state, for host and
// device code (plain C++ as well: no HIP header is needed to include this file).
//
// The semantics are those of quantity.cpp (parse_quantity and its converters; apimachinery
// v0.22.2 restated in that file's header comment).  quantity.cpp holds the digits in strings and
// the inf.Dec value in a growing big integer; here one pass finds the literal's parts and a
// second pass folds the digits into a state whose size does not depend on the literal:
//
//   The result is wanted in units of 1e-9 ("nano units"), and everything past the cap of
//   +-(2^63 - 1) saturates, so a digit d of decimal weight 10^e nano units
//     e > 27        saturates the value when d != 0 (10^28 nano units are past every limit),
//     0 <= e <= 27  is folded into a 128-bit accumulator (below 10^28 < 2^94),
//     e < 0         is dropped into a sticky "non-zero digits dropped" flag: inf.RoundUp at
//                   Nano rounds away from zero whenever anything non-zero was dropped.
//   A binary suffix multiplies by 2^b (b = 10 .. 60) after the decimal point is placed, so up
//   to 2^60 nano units can come out of the dropped digits.  Those literals keep the first 63
//   dropped digits in seven base-1e9 limbs and multiply them by 2^b with carry; the carry out is
//   the integer part they contribute.  63 >= b digits make the result exact: the kept value x is
//   a multiple of 1 / (5^63 * 2^(63-b)) and the digits past the limbs add less than that, so
//   they never carry into the integer part and only feed the sticky flag.
//
// An int64Amount (the fast path of ParseQuantity) and an inf.Dec differ only in what happens
// out of range: the int64Amount keeps value * 10^scale, which the converters report as
// PAS_ENOTEXACT when its floor is outside int64; the inf.Dec is rounded and capped.  Which of
// the two a literal becomes is decided from the digit counts, the suffix and the scale exactly
// as ParseQuantity decides it.  The exponent arithmetic is done in 64 bits: an e/E exponent is
// ParseInt's int64 truncated to int32, and every sum formed from it here is exact (quantity.cpp
// forms some of them in int32).
#pragma once

#include <cstdint>

#include "pas.h"

#if defined(__HIP__)
#define PAS_QF_HD __host__ __device__
#else
#define PAS_QF_HD
#endif

namespace pas {

struct QuantityFixed {
  int32_t status;    // PAS_OK, PAS_EINVAL or PAS_ENOTEXACT
  int64_t whole;     // pas_quantity_to_wide's pair (0, 0 unless PAS_OK)
  uint32_t nano;
  int32_t decimals;  // pas_quantity_decimals (0 for PAS_EINVAL)
  int32_t fit;       // the largest s in 0..9 at which pas_quantity_to_scaled succeeds, or -1
  int64_t as_int64;  // pas_quantity_as_int64: 0 for an inf.Dec, a negative scale or an overflow
};

namespace qf {

typedef unsigned __int128 u128;

PAS_QF_HD inline bool is_digit(char c) { return c >= '0' && c <= '9'; }

PAS_QF_HD inline bool is_suffix_char(char c) {  // "eEinumkKMGTP"
  return c == 'e' || c == 'E' || c == 'i' || c == 'n' || c == 'u' || c == 'm' || c == 'k' ||
         c == 'K' || c == 'M' || c == 'G' || c == 'T' || c == 'P';
}

// One-letter decimal SI suffix -> exponent; false for a letter that is none.
PAS_QF_HD inline bool si_exponent(char c, int32_t* e) {
  switch (c) {
    case 'n': *e = -9; return true;
    case 'u': *e = -6; return true;
    case 'm': *e = -3; return true;
    case 'k': *e = 3; return true;
    case 'M': *e = 6; return true;
    case 'G': *e = 9; return true;
    case 'T': *e = 12; return true;
    case 'P': *e = 15; return true;
    case 'E': *e = 18; return true;
    default: return false;
  }
}

// First letter of a binary suffix "<c>i" -> the power of two; false for a letter that is none.
PAS_QF_HD inline bool binary_exponent(char c, int32_t* e) {
  switch (c) {
    case 'K': *e = 10; return true;
    case 'M': *e = 20; return true;
    case 'G': *e = 30; return true;
    case 'T': *e = 40; return true;
    case 'P': *e = 50; return true;
    case 'E': *e = 60; return true;
    default: return false;
  }
}

constexpr uint32_t kBillion = 1000000000u;
constexpr int kFracLimbs = 7;  // 63 dropped digits kept under a binary suffix

// The digit fold (see the file comment).
struct Fold {
  u128 acc = 0;       // the digits of weight 10^0 .. 10^27 nano units
  bool sat = false;   // a non-zero digit of weight above 10^27
  bool sticky = false;  // a non-zero digit dropped
  bool keep_frac = false;  // binary suffix: keep the first 63 dropped digits
  uint32_t fr[kFracLimbs] = {0, 0, 0, 0, 0, 0, 0};  // most significant limb first
  int32_t n_fr = 0;   // dropped digits kept so far

  PAS_QF_HD void digit(uint32_t d, int64_t e) {
    if (e > 27) {
      sat |= d != 0;
    } else if (e >= 0) {
      acc = acc * 10 + d;
    } else if (keep_frac && n_fr < 9 * kFracLimbs) {
      const int32_t g = n_fr / 9;
      for (int32_t q = 0; q < kFracLimbs; ++q)  // (no indexed store: the limbs stay registers)
        if (q == g) fr[q] = fr[q] * 10 + d;
      ++n_fr;
    } else {
      sticky |= d != 0;
    }
  }
};

}  // namespace qf

// resource.ParseQuantity of bytes [p, p + len) and what the converters of quantity.cpp make of
// the result.
PAS_QF_HD inline QuantityFixed parse_quantity_fixed(const char* p, int64_t len) {
  using qf::u128;
  QuantityFixed r;
  r.status = PAS_EINVAL;
  r.whole = 0;
  r.nano = 0;
  r.decimals = 0;
  r.fit = -1;
  r.as_int64 = 0;
  if (!p || len <= 0) return r;

  // ---- parseQuantityString: sign, integer digits (leading zeros stripped), fraction, suffix
  bool positive = true;
  int64_t pos = 0;
  if (p[0] == '-' || p[0] == '+') {
    positive = p[0] != '-';
    pos = 1;
  }
  while (pos < len && p[pos] == '0') ++pos;
  int64_t nb = pos, ne = pos, db = pos, de = pos, sb = len;
  if (pos < len) {  // (else: all zeros or only a sign, the value 0 with no suffix)
    while (ne < len && qf::is_digit(p[ne])) ++ne;
    pos = ne;
    db = de = pos;
    if (pos < len && p[pos] == '.') {
      db = de = pos + 1;
      while (de < len && qf::is_digit(p[de])) ++de;
      pos = de;
    }
    sb = pos;
    while (pos < len && qf::is_suffix_char(p[pos])) ++pos;
    if (pos < len && (p[pos] == '-' || p[pos] == '+')) ++pos;
    while (pos < len && qf::is_digit(p[pos])) ++pos;
    if (pos < len) return r;  // ErrFormatWrong (a byte 0 ends up here too)
  }
  const int64_t nlen = ne - nb, dlen = de - db, slen = len - sb;

  // ---- quantitySuffixer.interpret
  bool binary = false;
  int32_t exponent = 0;
  if (slen == 0) {
  } else if (slen == 1 && qf::si_exponent(p[sb], &exponent)) {
  } else if (slen == 2 && p[sb + 1] == 'i' && qf::binary_exponent(p[sb], &exponent)) {
    binary = true;
  } else if (slen > 1 && (p[sb] == 'e' || p[sb] == 'E')) {
    // strconv.ParseInt(suffix[1:], 10, 64), then int32(parsed)
    int64_t i = sb + 1;
    bool neg = false;
    if (p[i] == '+' || p[i] == '-') neg = p[i++] == '-';
    if (i >= len) return r;
    uint64_t v = 0;
    for (; i < len; ++i) {
      if (!qf::is_digit(p[i])) return r;
      if (v > 922337203685477580ull) return r;  // v * 10 would pass 2^63: range error
      v = v * 10 + (uint64_t)(p[i] - '0');
      if (v > (1ull << 63)) return r;
    }
    if (!neg && v > (uint64_t)INT64_MAX) return r;
    exponent = (int32_t)(uint32_t)(neg ? 0 - v : v);  // int32(parsed) truncates
  } else {
    return r;
  }

  // ---- int64Amount or inf.Dec.  The int64Amount's multiply by the binary mantissa cannot
  // overflow: its digits are at most 14 - 3 b / 10, so the product is below 10^14 * 1.1^6.
  const int64_t nlen_p = nlen > 0 ? nlen : 1;  // an empty integer part is "0"
  bool fast;
  if (!binary) {
    fast = nlen_p + dlen <= 18 && (int64_t)exponent - dlen >= -9;
  } else {
    fast = dlen == 0 && 14 - nlen_p - 3 * (exponent / 10) >= 0;
  }

  // ---- the digits, in nano units: the integer part's last digit has weight 10^unit
  const int64_t unit = 9 + (binary ? 0 : (int64_t)exponent);
  qf::Fold f;
  f.keep_frac = binary;
  int64_t e = unit + nlen - 1;
  for (int64_t i = nb; i < ne; ++i, --e) f.digit((uint32_t)(p[i] - '0'), e);
  e = unit - 1;
  for (int64_t i = db; i < de; ++i, --e) f.digit((uint32_t)(p[i] - '0'), e);
  // the last digit's weight, when above 10^0: trailing zeros (at most 27 when acc != 0)
  if (f.acc != 0) {
    int64_t z = unit - dlen;
    for (; z >= 9; z -= 9) f.acc *= qf::kBillion;
    uint32_t m = 1;
    for (; z > 0; --z) m *= 10;
    f.acc *= m;
  }
  // past both limits: floor(-x) >= -2^63 <=> x <= 2^63 * 1e9 nano units
  const u128 kLimNeg = ((u128)1 << 63) * qf::kBillion;
  const u128 kLimPos = kLimNeg - 1;                           // floor(x) <= 2^63 - 1
  const u128 kCap = (u128)INT64_MAX * qf::kBillion;           // maxAllowed, in nano units
  bool inexact = f.sticky;
  if (binary) {
    const int32_t b = exponent;
    if (f.acc > (kLimNeg >> b))
      f.sat = true;
    else
      f.acc <<= b;
    // the kept dropped digits times 2^b, in two steps of at most 30 bits (64-bit products)
    int32_t pad = f.n_fr % 9;
    if (pad != 0) {
      uint32_t m = 1;
      for (; pad < 9; ++pad) m *= 10;
      const int32_t g = f.n_fr / 9;
      for (int32_t q = 0; q < qf::kFracLimbs; ++q)
        if (q == g) f.fr[q] *= m;
    }
    uint64_t carry_total = 0;
    for (int32_t left = b; left > 0;) {
      const int32_t sh = left > 30 ? 30 : left;
      left -= sh;
      uint64_t c = 0;
      for (int32_t q = qf::kFracLimbs - 1; q >= 0; --q) {
        const uint64_t prod = ((uint64_t)f.fr[q] << sh) + c;
        f.fr[q] = (uint32_t)(prod % qf::kBillion);
        c = prod / qf::kBillion;
      }
      carry_total = (carry_total << sh) + c;
    }
    if (!f.sat) f.acc += carry_total;  // below 2^60: still far inside 128 bits
    for (int32_t q = 0; q < qf::kFracLimbs; ++q) inexact |= f.fr[q] != 0;
  }

  u128 mag = f.acc;  // |value| in nano units
  if (fast) {        // exact by construction: nothing was dropped
    if (f.sat || mag > (positive ? kLimPos : kLimNeg)) {
      r.status = PAS_ENOTEXACT;  // scale >= 0 here: an integer, decimals 0
      return r;
    }
  } else if (f.sat || mag > kCap) {
    mag = kCap;
  } else if (inexact) {
    mag += 1;  // inf.RoundUp: away from zero (the magnitude is rounded before the sign)
    if (mag > kCap) mag = kCap;
  }

  // ---- mag = q * 1e9 + rem (mag < 2^94: three 32-bit limbs, 64-bit divisions by a constant)
  const uint64_t hi = (uint64_t)(mag >> 64), lo = (uint64_t)mag;
  uint64_t cur = (hi << 32) | (lo >> 32);
  const uint64_t q1 = cur / qf::kBillion;
  cur = ((cur % qf::kBillion) << 32) | (lo & 0xffffffffull);
  const uint64_t q = (q1 << 32) | (cur / qf::kBillion);
  const uint32_t rem = (uint32_t)(cur % qf::kBillion);
  if (positive || mag == 0) {
    r.whole = (int64_t)q;
    r.nano = rem;
  } else if (rem == 0) {
    r.whole = (int64_t)(0 - q);
    r.nano = 0;
  } else {  // floor: -0.5 is (-1, 500000000)
    r.whole = (int64_t)(0 - q - 1);
    r.nano = qf::kBillion - rem;
  }
  // decimals: 9 minus the trailing zero digits of the nano value
  int32_t k = 0;
  uint32_t x = rem, pw = 1;  // x = rem / 10^(9 - k), pw = 10^k
  if (rem != 0) {
    k = 9;
    pw = qf::kBillion;
    while (x % 10 == 0) {
      x /= 10;
      pw /= 10;
      --k;
    }
  }
  r.decimals = k;
  // fit: value * 10^s = q * 10^s + rem / 10^(9 - s) inside int64, for s from k upwards
  const u128 lim = positive ? (u128)INT64_MAX : (u128)1 << 63;
  u128 m = (u128)q * pw + x;
  if (m <= lim) {
    int32_t s = k;
    while (s < 9 && m * 10 <= lim) {
      m *= 10;
      ++s;
    }
    r.fit = s;
  }
  // AsInt64: an int64Amount of scale >= 0 is the integer q (rem is 0), inside int64 or 0; the
  // scale is exponent - dlen, and 0 under a binary suffix (dlen is 0 on its fast path)
  if (fast && (binary || (int64_t)exponent - dlen >= 0) && q <= (uint64_t)INT64_MAX)
    r.as_int64 = positive ? (int64_t)q : -(int64_t)q;
  r.status = PAS_OK;
  return r;
}

}  // namespace pas
