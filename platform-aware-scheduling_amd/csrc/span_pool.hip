// span_pool.hip — the kernels and host routines under the two resident name tables
// (span_pool.h): spans from CSR offsets, the scan-and-gather that packs a pool (for a remap,
// a read-back or the card table's dead bytes), and the re-pitch of the spans for a new shape.
// One lane per entry in 256-lane blocks; a row of k entries is k adjacent spans, and the node
// table is the case k == 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "host_staging.h"
#include "pas_internal.h"
#include "span_pool.h"

namespace pas {
namespace {

constexpr int kTpb = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTpb - 1) / kTpb); }

// *ctr += the lanes of the block with `named` set, one atomic per wave; ctr may be null
__device__ __forceinline__ void count_named(bool named, int32_t* ctr) {
  if (!ctr) return;  // (uniform)
  const unsigned long long m = __ballot(named);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(ctr, (int32_t)__popcll(m));
}

// beg / len of n entries from their CSR offsets, the bytes standing at `base` of the pool
__global__ void spans_from_csr(int64_t n, const int64_t* __restrict__ off, int64_t base,
                               int64_t* __restrict__ beg, int64_t* __restrict__ len,
                               int32_t* ctr) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  bool named = false;
  if (i < n) {
    beg[i] = base + off[i];
    len[i] = off[i + 1] - off[i];
    named = off[i + 1] > off[i];
  }
  count_named(named, ctr);
}

// The old entry of new entry i: row src[i / k] (null: the same row), -1 for an empty row
__device__ __forceinline__ int64_t old_entry(const int32_t* __restrict__ src, int32_t k,
                                             int64_t i) {
  if (!src) return i;
  const int32_t s = src[i / k];
  return s < 0 ? -1 : (int64_t)s * k + i % k;
}

// The lengths of a remapped table
__global__ void spans_remap_lens(int64_t n, int32_t k, const int32_t* __restrict__ src,
                                 const int64_t* __restrict__ len_old,
                                 int64_t* __restrict__ len_new, int32_t* ctr) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  bool named = false;
  if (i < n) {
    const int64_t o = old_entry(src, k, i);
    const int64_t len = o < 0 ? 0 : len_old[o];
    len_new[i] = len;
    named = len > 0;
  }
  count_named(named, ctr);
}

// Entry i copied to its scanned place dst + beg_new[i]; nothing is written at or past dst_cap
// (the host sized dst from its own count of the live bytes)
__global__ void spans_gather(int64_t n, int32_t k, const int32_t* __restrict__ src,
                             const int64_t* __restrict__ beg_old,
                             const int64_t* __restrict__ len_old,
                             const char* __restrict__ pool_old,
                             const int64_t* __restrict__ beg_new, char* __restrict__ dst,
                             int64_t dst_cap) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n) return;
  const int64_t o = old_entry(src, k, i);
  if (o < 0) return;
  const int64_t len = len_old[o];
  if (beg_new[i] + len > dst_cap) return;
  const char* p = pool_old + beg_old[o];
  char* q = dst + beg_new[i];
  for (int64_t j = 0; j < len; ++j) q[j] = p[j];
}

// The spans of n entries in rows of k_old into rows of k_new (the new arrays are zero)
__global__ void spans_repitch(int64_t n, int32_t k_old, int32_t k_new,
                              const int64_t* __restrict__ beg_old,
                              const int64_t* __restrict__ len_old, int64_t* __restrict__ beg_new,
                              int64_t* __restrict__ len_new) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n) return;
  const int64_t at = i / k_old * k_new + i % k_old;
  beg_new[at] = beg_old[i];
  len_new[at] = len_old[i];
}

std::string of(const char* table, const char* what) { return std::string(table) + ": " + what; }

}  // namespace

void free_pool(SpanPool& sp) {
  free_dev(sp.beg);
  free_dev(sp.len);
  free_dev(sp.pool);
  sp = SpanPool{};
}

int no_table(pas_ctx* ctx, const std::string& fn, const char* table) {
  return set_error(ctx, PAS_ENOSNAP, fn + ": no " + table);
}

int check_host_spans(pas_ctx* ctx, int64_t n, const int64_t* off, const char* bytes,
                     const std::string& what, bool has_bytes) {
  if (!off || off[0] != 0) return set_error(ctx, PAS_EINVAL, what + ": offsets must start at 0");
  for (int64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return set_error(ctx, PAS_EINVAL, what + ": offsets decrease");
  if (has_bytes && off[n] > 0 && !bytes) return set_error(ctx, PAS_EINVAL, what + ": null bytes");
  return PAS_OK;
}

int check_device_spans(pas_ctx* ctx, int64_t n, const ByteSpans& sp, const std::string& what) {
  if (sp.n_bytes < 0) return set_error(ctx, PAS_EINVAL, what + ": a byte count < 0");
  if (n > 0 && (!sp.off || (sp.n_bytes > 0 && !sp.bytes)))
    return set_error(ctx, PAS_EINVAL, what + ": null offsets or bytes");
  return PAS_OK;
}

int check_compact_map(pas_ctx* ctx, int32_t n_new, const int32_t* src, int32_t n_old,
                      const std::string& fn) {
  if (n_new < 0 || (n_new > 0 && !src))
    return set_error(ctx, PAS_EINVAL, fn + ": bad slot count or null map");
  int32_t last = -1;
  for (int32_t j = 0; j < n_new; ++j) {
    const int32_t v = src[j];
    if (v == -1) continue;
    if (v < 0 || v >= n_old || v <= last)
      return set_error(ctx, PAS_EINVAL, fn + ": entry " + std::to_string(j) + " is neither -1 " +
                                            "nor a slot above the entries before it");
    last = v;
  }
  return PAS_OK;
}

int alloc_spans(pas_ctx* ctx, int64_t cap, int64_t** beg, int64_t** len, hipStream_t s,
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

int grow_pool(pas_ctx* ctx, SpanPool& sp, int64_t more, hipStream_t s, const char* what) {
  const int64_t need = sp.pool_used + more;
  if (need <= sp.pool_cap) return PAS_OK;
  const int64_t cap = std::max(need, 2 * sp.pool_cap);
  char* np = nullptr;
  PAS_HIP(ctx, hipMalloc(&np, (size_t)cap));
  hipError_t e = hipSuccess;
  if (sp.pool_used > 0)
    e = hipMemcpyAsync(np, sp.pool, (size_t)sp.pool_used, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    free_dev(np);
    return check_hip(ctx, e, what);
  }
  free_dev(sp.pool);
  sp.pool = np;
  sp.pool_cap = cap;
  return PAS_OK;
}

int pool_set(pas_ctx* ctx, SpanPool& sp, int64_t n, const int64_t* name_off, const int64_t* d_off,
             const char* bytes, int32_t* d_named, hipStream_t s, const char* table) {
  const int64_t total = name_off[n];
  sp.span_cap = std::max<int64_t>(n, 1);
  sp.pool_cap = std::max<int64_t>(total, 1);
  sp.pool_used = sp.live_bytes = total;
  int rc = alloc_spans(ctx, sp.span_cap, &sp.beg, &sp.len, s, of(table, "span arrays").c_str());
  if (rc) return rc;
  PAS_HIP(ctx, hipMalloc(&sp.pool, (size_t)sp.pool_cap));
  if (total > 0)
    PAS_HIP(ctx, hipMemcpyAsync(sp.pool, bytes, (size_t)total, hipMemcpyHostToDevice, s));
  if (n > 0) {
    spans_from_csr<<<blocks_for(n), kTpb, 0, s>>>(n, d_off, 0, sp.beg, sp.len, d_named);
    PAS_HIP(ctx, hipGetLastError());
  }
  return PAS_OK;
}

int pool_gathered(pas_ctx* ctx, const SpanPool& src, int64_t n_rows_new, int32_t k,
                  const int32_t* d_map, void* d_scan, size_t scan_bytes, int32_t* d_named,
                  int32_t* named, SpanPool* out, hipStream_t s, const char* table) {
  SpanPool nt;
  const int64_t n = n_rows_new * k;
  nt.span_cap = std::max<int64_t>(n, 1);
  auto build = [&]() -> int {
    int r = alloc_spans(ctx, nt.span_cap, &nt.beg, &nt.len, s, of(table, "span arrays").c_str());
    if (r) return r;
    if (n > 0) {
      spans_remap_lens<<<blocks_for(n), kTpb, 0, s>>>(n, k, d_map, src.len, nt.len, d_named);
      PAS_HIP(ctx, hipGetLastError());
    }
    if ((r = scan_run<int64_t>(ctx, d_scan, scan_bytes, nt.len, nt.beg, (size_t)n + 1, s)))
      return r;
    int64_t total = 0;
    PAS_HIP(ctx, hipMemcpyAsync(&total, nt.beg + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (d_named)
      PAS_HIP(ctx, hipMemcpyAsync(named, d_named, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PAS_HIP(ctx, hipStreamSynchronize(s));
    nt.pool_cap = std::max<int64_t>(total, 1);
    nt.pool_used = nt.live_bytes = total;
    PAS_HIP(ctx, hipMalloc(&nt.pool, (size_t)nt.pool_cap));
    if (n > 0) {
      spans_gather<<<blocks_for(n), kTpb, 0, s>>>(n, k, d_map, src.beg, src.len, src.pool, nt.beg,
                                                  nt.pool, nt.pool_cap);
      PAS_HIP(ctx, hipGetLastError());
    }
    return PAS_OK;
  };
  const int rc = build();
  if (rc) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s);
    free_pool(nt);
    return rc;
  }
  *out = nt;
  return PAS_OK;
}

int pool_get(pas_ctx* ctx, const SpanPool& sp, int64_t n, int64_t* off_out, char* bytes_out,
             int64_t cap, const DerivedSync* after, const std::string& fn) {
  if (!off_out || cap < 0 || (cap > 0 && !bytes_out))
    return set_error(ctx, PAS_EINVAL, fn + ": null output or cap < 0");
  int rc = activate(ctx);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const bool fits = cap >= sp.live_bytes;
  size_t scan_bytes = 0;
  if ((rc = scan_size<int64_t>(ctx, (size_t)n + 1, &scan_bytes))) return rc;
  Staging st(ctx);
  int64_t* d_off;
  char *d_bytes, *d_scan;
  st.out(d_off, off_out, (size_t)n + 1);
  st.out(d_bytes, bytes_out, fits ? (size_t)sp.live_bytes : 0);
  st.work(d_scan, scan_bytes);
  if ((rc = st.upload())) return rc;
  if (after && (rc = derived_wait(ctx, *after, s))) return rc;
  if ((rc = scan_run<int64_t>(ctx, d_scan, scan_bytes, sp.len, d_off, (size_t)n + 1, s)))
    return rc;
  if (fits && n > 0) {
    spans_gather<<<blocks_for(n), kTpb, 0, s>>>(n, 1, nullptr, sp.beg, sp.len, sp.pool, d_off,
                                                d_bytes, sp.live_bytes);
    PAS_HIP(ctx, hipGetLastError());
  }
  PAS_HIP(ctx, st.fetch());
  if (!fits)
    return set_error(ctx, PAS_ECAPACITY, fn + ": " + std::to_string(sp.live_bytes) +
                                             " bytes of names, cap " + std::to_string(cap));
  return PAS_OK;
}

int pool_get_rows(pas_ctx* ctx, const SpanPool& sp, int64_t n_rows, int32_t k,
                  const int32_t* row_slot, int64_t total, int64_t* off_out, char* bytes_out,
                  int64_t cap, const std::string& fn) {
  if (!off_out || cap < 0 || (cap > 0 && !bytes_out))
    return set_error(ctx, PAS_EINVAL, fn + ": null output or cap < 0");
  int rc = activate(ctx);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const int64_t n = n_rows * k;
  const bool fits = cap >= total;
  size_t scan_bytes = 0;
  if ((rc = scan_size<int64_t>(ctx, (size_t)n + 1, &scan_bytes))) return rc;
  Staging st(ctx);
  int32_t* d_rows;
  int64_t *d_off, *d_len;
  char *d_bytes, *d_scan;
  st.in(d_rows, row_slot, (size_t)n_rows);
  st.out(d_off, off_out, (size_t)n + 1);
  st.out(d_bytes, bytes_out, fits ? (size_t)total : 0);
  st.work(d_len, (size_t)n + 1);
  st.work(d_scan, scan_bytes);
  if ((rc = st.upload())) return rc;
  PAS_HIP(ctx, hipMemsetAsync(d_len + n, 0, sizeof(int64_t), s));
  if (n > 0) {
    spans_remap_lens<<<blocks_for(n), kTpb, 0, s>>>(n, k, d_rows, sp.len, d_len, nullptr);
    PAS_HIP(ctx, hipGetLastError());
  }
  if ((rc = scan_run<int64_t>(ctx, d_scan, scan_bytes, d_len, d_off, (size_t)n + 1, s))) return rc;
  if (fits && n > 0) {
    spans_gather<<<blocks_for(n), kTpb, 0, s>>>(n, k, d_rows, sp.beg, sp.len, sp.pool, d_off,
                                                d_bytes, total);
    PAS_HIP(ctx, hipGetLastError());
  }
  PAS_HIP(ctx, st.fetch());
  if (!fits)
    return set_error(ctx, PAS_ECAPACITY, fn + ": " + std::to_string(total) +
                                             " bytes of names, cap " + std::to_string(cap));
  return PAS_OK;
}

int pool_repitch(pas_ctx* ctx, SpanPool& sp, int64_t n_rows_old, int32_t k_old,
                 int64_t n_rows_new, int32_t k_new, hipStream_t s, const char* table,
                 const std::string& fn) {
  int64_t *beg, *len;
  const int64_t cap = std::max<int64_t>(n_rows_new * k_new, 1);
  int rc = alloc_spans(ctx, cap, &beg, &len, s, of(table, "span arrays").c_str());
  if (rc) return rc;
  const int64_t old = n_rows_old * k_old;
  hipError_t e = hipSuccess;
  if (old > 0) {
    spans_repitch<<<blocks_for(old), kTpb, 0, s>>>(old, k_old, k_new, sp.beg, sp.len, beg, len);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    free_dev(beg);
    free_dev(len);
    return check_hip(ctx, e, (fn + ": span copy").c_str());
  }
  free_dev(sp.beg);
  free_dev(sp.len);
  sp.beg = beg;
  sp.len = len;
  sp.span_cap = cap;
  return PAS_OK;
}

}  // namespace pas
