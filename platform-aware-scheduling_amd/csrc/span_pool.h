// span_pool.h — the layer under the two resident name tables (name_table.hip: node names,
// gas_cards.hip: card names): a SpanPool (pas_internal.h) is spans (beg, len) into one byte
// pool that only grows.  Here: the scans, the two checks of a call's byte spans (ByteSpans,
// csr_entry.h: every string verb's, not only the tables'), and what span_pool.hip builds on the
// scans.  `table` names the table in an error ("name table"), `fn` the
// entry point.
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

int no_table(pas_ctx* ctx, const std::string& fn, const char* table);

// The n byte spans of a host form: offsets [n + 1] from 0 and non-decreasing, bytes when the
// total is above 0.  `what` names the entry point, and the argument when it has several.
// has_bytes = false: offsets that count something other than bytes (the col_off of a quantity
// refresh counts entries), so no byte array goes with them and `bytes` is not looked at.
int check_host_spans(pas_ctx* ctx, int64_t n, const int64_t* off, const char* bytes,
                     const std::string& what, bool has_bytes = true);
// The n byte spans of a _device form, of which the host sees the count and the pointers only:
// n_bytes >= 0 whatever n is, and with n > 0 offsets, and bytes when n_bytes > 0.
int check_device_spans(pas_ctx* ctx, int64_t n, const ByteSpans& sp, const std::string& what);

// A compact map of n_new rows over n_old: every entry is -1 or a row above the entries before
// it.
int check_compact_map(pas_ctx* ctx, int32_t n_new, const int32_t* src, int32_t n_old,
                      const std::string& fn);

// Span arrays of `cap` entries (+ 1: the scans' last element), all zero.
int alloc_spans(pas_ctx* ctx, int64_t cap, int64_t** beg, int64_t** len, hipStream_t s,
                const char* what);

// Room for sp.pool_used + more bytes in sp.pool; synchronous on s when the pool moves.
int grow_pool(pas_ctx* ctx, SpanPool& sp, int64_t more, hipStream_t s, const char* what);

// A set from its host form: sp = spans of n entries from d_off (the uploaded name_off) over a
// pool that is a copy of bytes, enqueued on s.  d_named (may be null): a zeroed counter, + the
// entries that are not empty.  sp is empty on entry; a failure leaves it to the caller's
// free_pool.
int pool_set(pas_ctx* ctx, SpanPool& sp, int64_t n, const int64_t* name_off, const int64_t* d_off,
             const char* bytes, int32_t* d_named, hipStream_t s, const char* table);

// out = n_rows_new rows of k entries, row j the row d_map[j] of src (-1: an empty row; d_map
// null: the rows as they are), in storage of its own with the pool packed in entry order.
// d_scan: scan_size<int64_t>(n_rows_new * k + 1) bytes.  d_named (may be null): a zeroed
// counter, + the entries that are not empty, read back into *named.  Synchronizes s once (the
// byte total decides the pool's size) and leaves the gather enqueued.  src is untouched; a
// failure frees what was allocated.
int pool_gathered(pas_ctx* ctx, const SpanPool& src, int64_t n_rows_new, int32_t k,
                  const int32_t* d_map, void* d_scan, size_t scan_bytes, int32_t* d_named,
                  int32_t* named, SpanPool* out, hipStream_t s, const char* table);

// The entries of sp in entry order: offsets [n + 1] and the live bytes; PAS_ECAPACITY with the
// offsets delivered and the bytes withheld when cap is short.  On ctx->stream, after the change
// `after` stands for (null: the table only changes synchronously), synchronous.
int pool_get(pas_ctx* ctx, const SpanPool& sp, int64_t n, int64_t* off_out, char* bytes_out,
             int64_t cap, const DerivedSync* after, const std::string& fn);

// The rows row_slot[0 .. n_rows) (host array, every entry a row of sp) of k entries each, in call
// order: offsets [n_rows * k + 1] and their bytes, `total` of them (the caller's count); the
// capacity rule, stream and synchronization of pool_get.
int pool_get_rows(pas_ctx* ctx, const SpanPool& sp, int64_t n_rows, int32_t k,
                  const int32_t* row_slot, int64_t total, int64_t* off_out, char* bytes_out,
                  int64_t cap, const std::string& fn);

// New span arrays of n_rows_new x k_new entries holding the n_rows_old x k_old ones (the rest
// empty), swapped in; the pool as it is.  Synchronous on s.
int pool_repitch(pas_ctx* ctx, SpanPool& sp, int64_t n_rows_old, int32_t k_old,
                 int64_t n_rows_new, int32_t k_new, hipStream_t s, const char* table,
                 const std::string& fn);

}  // namespace pas
