// card_rows.h — the card-name table's rows as the string kernels read them (gas_annotations.hip,
// gas_node_strings.hip): one lane per event or update, a row's spans read from memory per
// compare, and the few device helpers both files' kernels share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pas_internal.h"

namespace pas {

__device__ __forceinline__ int32_t sat32(int64_t v) {
  return v > INT32_MAX ? INT32_MAX : (int32_t)v;
}

// the wave's largest v into *dst (one lane issues the atomic)
__device__ __forceinline__ void wave_max(int32_t v, int32_t* dst) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  if ((threadIdx.x & 63) == 0 && v > *(volatile int32_t*)dst) atomicMax(dst, v);
}

// Row s of the table is entries s * k .. s * k + k of the spans (GasCardNames, pas_internal.h)
struct CardView {
  int32_t k;
  const int64_t* beg;
  const int64_t* len;
  const char* pool;
};

inline CardView view_of(const GasCardNames& t) {
  return CardView{t.k, t.sp.beg, t.sp.len, t.sp.pool};
}

// The lowest position among the first L names of the row whose spans start at entry `row` that
// holds the name p[0 .. n) (the length first, then the bytes), else -1.
__device__ __forceinline__ int32_t row_find(const CardView& t, int64_t row, int32_t L,
                                            const char* __restrict__ p, int64_t n) {
  for (int32_t r = 0; r < L; ++r) {
    if (t.len[row + r] != n) continue;
    const char* q = t.pool + t.beg[row + r];
    int64_t i = 0;  // (not bytes_equal: its early return compiles to another annotation_ranks)
    while (i < n && q[i] == p[i]) ++i;
    if (i == n) return r;
  }
  return -1;
}

}  // namespace pas
