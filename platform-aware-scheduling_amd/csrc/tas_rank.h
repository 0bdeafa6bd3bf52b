// tas_rank.h — a value's rank in a column's sorted row: what the request-order prioritize
// paths (tas_request.hip: one request; tas_request_batch.hip: a batch) build their keys from,
// and where a resumed top-k list finds its cursor's tie run (tas_gas_topk.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pas_internal.h"

namespace pas {

// Number of entries of the ascending row[0, cnt) that are < v (lower) or <= v (upper).
// kWide: the same over a wide column's row (floors in row, nanos in nrow, exact pair order)
// for the pair (v, f); the narrow form reads neither nrow nor f.
template <bool kWide>
__device__ __forceinline__ int32_t bound(const int64_t* __restrict__ row,
                                         const uint32_t* __restrict__ nrow, int32_t cnt,
                                         int64_t v, uint32_t f, bool upper) {
  int32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const int32_t mid = (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1);
    const int64_t x = row[mid];
    bool before;
    if constexpr (kWide) {
      const uint32_t xf = nrow[mid];
      before = upper ? pair_not_above(x, xf, v, f) : pair_below(x, xf, v, f);
    } else {
      before = x < v || (upper && x == v);
    }
    if (before) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace pas
