// csr_entry.h — a batch of byte strings (ByteSpans) and one entry of it on the device
// (tas_ingest.hip, name_table.hip, gas_annotations.hip, gas_node_strings.hip): offsets of the
// _device forms cannot be validated, so they are read clamped.
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

// A batch of byte strings, the one record from a C entry point to its kernels: entry i is
// bytes[off[i] .. off[i + 1]), off has one entry more than the batch, n_bytes is the byte total
// (off[n] of a host form, the caller's count of a _device form).
struct ByteSpans {
  int64_t n_bytes;
  const int64_t* off;
  const char* bytes;
  __device__ __forceinline__ int64_t span(int64_t i, int64_t* b) const {
    return entry_span(off, n_bytes, i, b);
  }
};

__device__ __forceinline__ bool bytes_equal(const char* __restrict__ a,
                                            const char* __restrict__ b, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

}  // namespace pas
