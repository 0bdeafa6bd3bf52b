// span_pool.h — what the two resident name tables share (name_table.hip: node names,
// gas_cards.hip: card names): spans (beg, len) into one byte pool that only grows, the CSR
// check of their host forms and the scans that pack a pool.
#pragma once

#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <string>

#include "pas_internal.h"

namespace pas {

// Temporary storage of an exclusive scan of n values (at least 16 bytes, so that a buffer of
// that size is never the null pointer that asks rocprim for the size), and the scan.
template <typename T>
inline int scan_size(pas_ctx* ctx, size_t n, size_t* bytes) {
  *bytes = 0;
  PAS_HIP(ctx, rocprim::exclusive_scan(nullptr, *bytes, (const T*)nullptr, (T*)nullptr, T(0), n,
                                       rocprim::plus<T>(), (hipStream_t) nullptr));
  *bytes = std::max<size_t>(*bytes, 16);
  return PAS_OK;
}

template <typename T>
inline int scan_run(pas_ctx* ctx, void* tmp, size_t bytes, const T* in, T* out, size_t n,
                    hipStream_t s) {
  PAS_HIP(ctx, rocprim::exclusive_scan(tmp, bytes, in, out, T(0), n, rocprim::plus<T>(), s));
  return PAS_OK;
}

inline void free_dev(void* p) {
  if (p) (void)hipFree(p);
}

// Span arrays of `cap` entries (+ 1: the scans' last element), all zero.  `what` names the
// table in the error.
inline int alloc_spans(pas_ctx* ctx, int64_t cap, int64_t** beg, int64_t** len, hipStream_t s,
                       const char* what) {
  *beg = *len = nullptr;
  const size_t bytes = sizeof(int64_t) * ((size_t)cap + 1);
  hipError_t e = hipMalloc(beg, bytes);
  if (e == hipSuccess) e = hipMalloc(len, bytes);
  if (e == hipSuccess) e = hipMemsetAsync(*len, 0, bytes, s);
  if (e == hipSuccess) e = hipMemsetAsync(*beg, 0, bytes, s);
  if (e != hipSuccess) {
    free_dev(*beg);
    free_dev(*len);
    *beg = *len = nullptr;
    return check_hip(ctx, e, what);
  }
  return PAS_OK;
}

// offsets [n + 1] of a host form: from 0 and non-decreasing
inline int check_csr(pas_ctx* ctx, int64_t n, const int64_t* off, const char* bytes,
                     const std::string& fn) {
  if (!off || off[0] != 0) return set_error(ctx, PAS_EINVAL, fn + ": offsets must start at 0");
  for (int64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return set_error(ctx, PAS_EINVAL, fn + ": offsets decrease");
  if (off[n] > 0 && !bytes) return set_error(ctx, PAS_EINVAL, fn + ": null input");
  return PAS_OK;
}

// Room for t.pool_used + more bytes in t.pool (NameTable, GasCardNames); synchronous on s when
// the pool moves.
template <class Table>
inline int grow_pool(pas_ctx* ctx, Table& t, int64_t more, hipStream_t s, const char* what) {
  const int64_t need = t.pool_used + more;
  if (need <= t.pool_cap) return PAS_OK;
  const int64_t cap = std::max(need, 2 * t.pool_cap);
  char* np = nullptr;
  PAS_HIP(ctx, hipMalloc(&np, (size_t)cap));
  hipError_t e = hipSuccess;
  if (t.pool_used > 0)
    e = hipMemcpyAsync(np, t.pool, (size_t)t.pool_used, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    free_dev(np);
    return check_hip(ctx, e, what);
  }
  free_dev(t.pool);
  t.pool = np;
  t.pool_cap = cap;
  return PAS_OK;
}

}  // namespace pas
