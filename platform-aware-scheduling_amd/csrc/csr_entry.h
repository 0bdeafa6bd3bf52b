// csr_entry.h — one entry of a CSR batch of byte strings on the device (name_table.hip,
// gas_annotations.hip): offsets of the _device forms cannot be validated, so they are read
// clamped, as parse_literals (tas_ingest.hip) reads its literals.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pas {

__device__ __forceinline__ int64_t clamp_off(int64_t v, int64_t n) {
  return v < 0 ? 0 : v > n ? n : v;
}

// Entry i of a batch: bytes[*b .. *b + return), both ends clamped into [0, n_bytes] and the
// end not before the begin.
__device__ __forceinline__ int64_t entry_span(const int64_t* __restrict__ off, int64_t n_bytes,
                                              int64_t i, int64_t* b) {
  *b = clamp_off(off[i], n_bytes);
  const int64_t e = clamp_off(off[i + 1], n_bytes);
  return e < *b ? 0 : e - *b;
}

__device__ __forceinline__ bool bytes_equal(const char* __restrict__ a,
                                            const char* __restrict__ b, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

}  // namespace pas
