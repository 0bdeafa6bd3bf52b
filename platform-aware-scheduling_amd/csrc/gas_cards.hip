// gas_cards.hip — the resident card-name table: which card name stands in which card slot.
//
// The reference keeps a node's usage by card name (nodeStatuses map[string]nodeResources,
// gpu-aware-scheduling/pkg/gpuscheduler/node_resource_cache.go:64,259-272) and reads a pod's
// cards as names out of its annotation (:241,253-256); card slots (ranks into used[n][.])
// exist only here.  The table (GasCardNames, pas_internal.h) names the slots of every node row,
// so that the annotations of a pod-event batch are resolved on the device
// (gas_annotations.hip).  It changes only through the calls below, all of them synchronous:
//   set      spans from the caller's CSR, the blob is the pool
//   update   whole rows rewritten: the new bytes are appended to the pool, the rows' spans
//            point there, the old bytes are dead; when the dead bytes pass the live ones the
//            pool is gathered (scan of the lengths + one gather, as names_remap does)
//   resize   the spans re-pitched into n_slots_new x k_new, the pool as it is
//   remap    the rows renumbered by the compact map and the pool gathered
// A lookup compares a listed name with the first n_cards[node] spans of the node's row: a row
// holds at most PAS_GAS_MAX_CARDS names, so there is no hash.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_staging.h"
#include "pas_internal.h"
#include "span_pool.h"

namespace pas {
namespace {

constexpr int kTpb = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTpb - 1) / kTpb); }

// beg / len of a set from its CSR offsets
__global__ void cards_spans(int64_t n, const int64_t* __restrict__ off, int64_t* __restrict__ beg,
                            int64_t* __restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n) return;
  beg[i] = off[i];
  len[i] = off[i + 1] - off[i];
}

// Row r of an update (entries off[r * k .. r * k + k] of the bytes appended at `base`) into
// slot row_slot[r], unless a later row of the call names the same slot (keep[r] == 0).
__global__ void cards_write_rows(int64_t n, int32_t k, const int32_t* __restrict__ row_slot,
                                 const uint8_t* __restrict__ keep,
                                 const int64_t* __restrict__ off, int64_t base,
                                 int64_t* __restrict__ beg, int64_t* __restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n) return;
  const int64_t r = i / k;
  if (!keep[r]) return;
  const int64_t at = (int64_t)row_slot[r] * k + i % k;
  beg[at] = base + off[i];
  len[at] = off[i + 1] - off[i];
}

// The spans of n_old rows of k_old entries into rows of k_new (the new arrays are zero)
__global__ void cards_repitch(int64_t n, int32_t k_old, int32_t k_new,
                              const int64_t* __restrict__ beg_old,
                              const int64_t* __restrict__ len_old, int64_t* __restrict__ beg_new,
                              int64_t* __restrict__ len_new) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n) return;
  const int64_t at = i / k_old * k_new + i % k_old;
  beg_new[at] = beg_old[i];
  len_new[at] = len_old[i];
}

// The old entry of new entry i: row src[i / k] (null: the same row), -1 for an empty row
__device__ __forceinline__ int64_t old_entry(const int32_t* __restrict__ src, int32_t k,
                                             int64_t i) {
  if (!src) return i;
  const int32_t s = src[i / k];
  return s < 0 ? -1 : (int64_t)s * k + i % k;
}

__global__ void cards_gather_lens(int64_t n, int32_t k, const int32_t* __restrict__ src,
                                  const int64_t* __restrict__ len_old,
                                  int64_t* __restrict__ len_new) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n) return;
  const int64_t o = old_entry(src, k, i);
  len_new[i] = o < 0 ? 0 : len_old[o];
}

// Entry i copied to its scanned place dst + beg_new[i]; nothing is written at or past dst_cap
// (the host sized dst from its own count of the live bytes)
__global__ void cards_gather(int64_t n, int32_t k, const int32_t* __restrict__ src,
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

int no_table(pas_ctx* ctx, const char* fn) {
  return set_error(ctx, PAS_ENOSNAP, std::string(fn) + ": no card-name table");
}

// out = n_slots_new rows of t.k entries, row j the row d_src[j] of t (-1: empty; d_src null:
// the rows as they are), in storage of its own with the pool gathered in entry order;
// out.row_bytes is the caller's.  Synchronous on s.  A failure frees what it allocated.
int gathered(pas_ctx* ctx, const GasCardNames& t, int32_t n_slots_new, const int32_t* d_src,
             GasCardNames* out, hipStream_t s) {
  GasCardNames nt;
  nt.n_slots = n_slots_new;
  nt.k = t.k;
  const int64_t entries = (int64_t)n_slots_new * t.k;
  void* d_scan = nullptr;
  auto build = [&]() -> int {
    size_t scan_bytes = 0;
    int r = scan_size<int64_t>(ctx, (size_t)entries + 1, &scan_bytes);
    if (r) return r;
    if ((r = alloc_spans(ctx, entries, &nt.beg, &nt.len, s, "card-name table: span arrays")))
      return r;
    PAS_HIP(ctx, hipMalloc(&d_scan, scan_bytes));
    if (entries > 0) {
      cards_gather_lens<<<blocks_for(entries), kTpb, 0, s>>>(entries, t.k, d_src, t.len, nt.len);
      PAS_HIP(ctx, hipGetLastError());
    }
    if ((r = scan_run<int64_t>(ctx, d_scan, scan_bytes, nt.len, nt.beg, (size_t)entries + 1, s)))
      return r;
    int64_t total = 0;
    PAS_HIP(ctx, hipMemcpyAsync(&total, nt.beg + entries, sizeof(int64_t), hipMemcpyDeviceToHost,
                                s));
    PAS_HIP(ctx, hipStreamSynchronize(s));
    nt.pool_cap = std::max<int64_t>(total, 1);
    nt.pool_used = nt.live_bytes = total;
    PAS_HIP(ctx, hipMalloc(&nt.pool, (size_t)nt.pool_cap));
    if (entries > 0) {
      cards_gather<<<blocks_for(entries), kTpb, 0, s>>>(entries, t.k, d_src, t.beg, t.len, t.pool,
                                                        nt.beg, nt.pool, nt.pool_cap);
      PAS_HIP(ctx, hipGetLastError());
    }
    PAS_HIP(ctx, hipStreamSynchronize(s));
    return PAS_OK;
  };
  const int rc = build();
  if (rc) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s);
  }
  free_dev(d_scan);
  if (rc) {
    free_gas_cards(nt);
    return rc;
  }
  *out = std::move(nt);
  return PAS_OK;
}

// t's device storage replaced by nt's (host bookkeeping is the caller's)
void swap_in(GasCardNames& t, GasCardNames& nt) {
  free_dev(t.beg);
  free_dev(t.len);
  free_dev(t.pool);
  t.beg = nt.beg, t.len = nt.len, t.pool = nt.pool;
  t.pool_used = nt.pool_used, t.pool_cap = nt.pool_cap, t.live_bytes = nt.live_bytes;
  nt.beg = nt.len = nullptr;
  nt.pool = nullptr;
}

}  // namespace

void free_gas_cards(GasCardNames& t) {
  free_dev(t.beg);
  free_dev(t.len);
  free_dev(t.pool);
  t = GasCardNames{};
}

}  // namespace pas

using namespace pas;

extern "C" {

int pas_gas_card_names_set(pas_ctx* ctx, int32_t n_slots, int32_t k, const int64_t* name_off,
                           const char* bytes) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_card_names_set";
  if (n_slots < 0 || k < 1 || k > PAS_GAS_MAX_CARDS)
    return set_error(ctx, PAS_EINVAL, fn + ": n_slots < 0 or k outside [1, PAS_GAS_MAX_CARDS]");
  const int64_t entries = (int64_t)n_slots * k;
  int rc = check_csr(ctx, entries, name_off, bytes, fn);
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = ctx->stream;
  const int64_t total = name_off[entries];
  GasCardNames nt;
  nt.n_slots = n_slots;
  nt.k = k;
  nt.pool_cap = std::max<int64_t>(total, 1);
  nt.pool_used = nt.live_bytes = total;
  nt.row_bytes.resize((size_t)n_slots);
  for (int64_t r = 0; r < n_slots; ++r) nt.row_bytes[r] = name_off[(r + 1) * k] - name_off[r * k];
  nt.stamp.assign((size_t)n_slots, 0);
  Staging st(ctx);
  int64_t* d_off;
  st.in(d_off, name_off, (size_t)entries + 1);
  auto build = [&]() -> int {
    int r = st.upload();
    if (r) return r;
    if ((r = alloc_spans(ctx, entries, &nt.beg, &nt.len, s, "card-name table: span arrays")))
      return r;
    PAS_HIP(ctx, hipMalloc(&nt.pool, (size_t)nt.pool_cap));
    if (total > 0)
      PAS_HIP(ctx, hipMemcpyAsync(nt.pool, bytes, (size_t)total, hipMemcpyHostToDevice, s));
    if (entries > 0) {
      cards_spans<<<blocks_for(entries), kTpb, 0, s>>>(entries, d_off, nt.beg, nt.len);
      PAS_HIP(ctx, hipGetLastError());
    }
    PAS_HIP(ctx, hipStreamSynchronize(s));
    return PAS_OK;
  };
  if ((rc = build())) {  // the previous table stays as it was
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s);
    free_gas_cards(nt);
    return rc;
  }
  nt.valid = true;
  free_gas_cards(ctx->gas_cards);
  ctx->gas_cards = std::move(nt);
  return PAS_OK;
}

int pas_gas_card_names_update(pas_ctx* ctx, int32_t n_rows, const int32_t* row_slot,
                              const int64_t* name_off, const char* bytes) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_card_names_update";
  GasCardNames& t = ctx->gas_cards;
  if (!t.valid) return no_table(ctx, fn.c_str());
  if (n_rows < 0) return set_error(ctx, PAS_EINVAL, fn + ": n_rows < 0");
  if (n_rows == 0) return PAS_OK;
  if (!row_slot) return set_error(ctx, PAS_EINVAL, fn + ": null input");
  const int64_t entries = (int64_t)n_rows * t.k;
  int rc = check_csr(ctx, entries, name_off, bytes, fn);
  if (rc) return rc;
  for (int32_t r = 0; r < n_rows; ++r)
    if (row_slot[r] < 0 || row_slot[r] >= t.n_slots)
      return set_error(ctx, PAS_EINVAL, fn + ": row " + std::to_string(r) + " names slot " +
                                            std::to_string(row_slot[r]) + ", the table has " +
                                            std::to_string(t.n_slots));
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = ctx->stream;
  const int64_t total = name_off[entries];
  // a slot given twice keeps the later row: walking backwards, the first row seen of a slot
  std::vector<uint8_t> keep((size_t)n_rows);
  if (++t.stamp_clock == 0) {  // (the clock wrapped: no stale stamp may equal a new one)
    std::fill(t.stamp.begin(), t.stamp.end(), 0u);
    t.stamp_clock = 1;
  }
  for (int32_t r = n_rows - 1; r >= 0; --r) {
    keep[r] = t.stamp[row_slot[r]] != t.stamp_clock;
    t.stamp[row_slot[r]] = t.stamp_clock;
  }
  Staging st(ctx);
  int64_t* d_off;
  int32_t* d_slot;
  uint8_t* d_keep;
  st.in(d_off, name_off, (size_t)entries + 1);
  st.in(d_slot, row_slot, (size_t)n_rows);
  st.in(d_keep, static_cast<const uint8_t*>(keep.data()), (size_t)n_rows);
  if ((rc = st.upload())) return rc;
  if ((rc = grow_pool(ctx, t, total, s, "card-name table: pool copy"))) return rc;
  // nothing has changed so far; from here the table does
  if (total > 0)
    PAS_HIP(ctx, hipMemcpyAsync(t.pool + t.pool_used, bytes, (size_t)total, hipMemcpyHostToDevice,
                                s));
  cards_write_rows<<<blocks_for(entries), kTpb, 0, s>>>(entries, t.k, d_slot, d_keep, d_off,
                                                        t.pool_used, t.beg, t.len);
  PAS_HIP(ctx, hipGetLastError());
  PAS_HIP(ctx, hipStreamSynchronize(s));
  t.pool_used += total;
  for (int32_t r = 0; r < n_rows; ++r) {
    if (!keep[r]) continue;
    const int64_t b = name_off[(int64_t)(r + 1) * t.k] - name_off[(int64_t)r * t.k];
    t.live_bytes += b - t.row_bytes[row_slot[r]];
    t.row_bytes[row_slot[r]] = b;
  }
  if (t.pool_used - t.live_bytes > t.live_bytes) {  // more dead bytes than live ones
    GasCardNames nt;
    if ((rc = gathered(ctx, t, t.n_slots, nullptr, &nt, s))) return rc;
    swap_in(t, nt);
  }
  return PAS_OK;
}

int pas_gas_card_names_resize(pas_ctx* ctx, int32_t n_slots_new, int32_t k_new,
                              void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_card_names_resize";
  GasCardNames& t = ctx->gas_cards;
  if (!t.valid) return no_table(ctx, fn.c_str());
  if (n_slots_new < t.n_slots || k_new < t.k || k_new > PAS_GAS_MAX_CARDS)
    return set_error(ctx, PAS_EINVAL,
                     fn + ": " + std::to_string(n_slots_new) + " x " + std::to_string(k_new) +
                         ", the table has " + std::to_string(t.n_slots) + " x " +
                         std::to_string(t.k) + " (sizes only grow, k <= PAS_GAS_MAX_CARDS)");
  if (n_slots_new == t.n_slots && k_new == t.k) return PAS_OK;
  int rc = activate(ctx);
  if (rc) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  int64_t *beg, *len;
  if ((rc = alloc_spans(ctx, (int64_t)n_slots_new * k_new, &beg, &len, s,
                        "card-name table: span arrays"))) return rc;
  const int64_t old = (int64_t)t.n_slots * t.k;
  hipError_t e = hipSuccess;
  if (old > 0) {
    cards_repitch<<<blocks_for(old), kTpb, 0, s>>>(old, t.k, k_new, t.beg, t.len, beg, len);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    free_dev(beg);
    free_dev(len);
    return check_hip(ctx, e, "pas_gas_card_names_resize: span copy");
  }
  free_dev(t.beg);
  free_dev(t.len);
  t.beg = beg;
  t.len = len;
  t.n_slots = n_slots_new;
  t.k = k_new;
  t.row_bytes.resize((size_t)n_slots_new, 0);
  t.stamp.resize((size_t)n_slots_new, 0);
  return PAS_OK;
}

int pas_gas_card_names_remap(pas_ctx* ctx, int32_t n_slots_new, const int32_t* src_slot,
                             void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_card_names_remap";
  GasCardNames& t = ctx->gas_cards;
  if (!t.valid) return no_table(ctx, fn.c_str());
  if (n_slots_new < 0 || (n_slots_new > 0 && !src_slot))
    return set_error(ctx, PAS_EINVAL, fn + ": bad slot count or null map");
  int32_t last = -1;
  for (int32_t j = 0; j < n_slots_new; ++j) {
    const int32_t v = src_slot[j];
    if (v == -1) continue;
    if (v < 0 || v >= t.n_slots || v <= last)
      return set_error(ctx, PAS_EINVAL, fn + ": entry " + std::to_string(j) + " is neither -1 " +
                                            "nor a slot above the entries before it");
    last = v;
  }
  int rc = activate(ctx);
  if (rc) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  int32_t* d_src = nullptr;
  const size_t n2 = (size_t)n_slots_new;
  PAS_HIP(ctx, hipMalloc(&d_src, sizeof(int32_t) * std::max<size_t>(n2, 1)));
  GasCardNames nt;
  hipError_t e = hipSuccess;
  if (n2) e = hipMemcpyAsync(d_src, src_slot, sizeof(int32_t) * n2, hipMemcpyHostToDevice, s);
  rc = e != hipSuccess ? check_hip(ctx, e, "pas_gas_card_names_remap: map upload")
                       : gathered(ctx, t, n_slots_new, d_src, &nt, s);
  (void)hipStreamSynchronize(s);
  free_dev(d_src);
  if (rc) return rc;  // the table stays as it was
  swap_in(t, nt);
  std::vector<int64_t> row_bytes(n2);
  for (size_t j = 0; j < n2; ++j) row_bytes[j] = src_slot[j] >= 0 ? t.row_bytes[src_slot[j]] : 0;
  t.row_bytes.swap(row_bytes);
  t.stamp.assign(n2, 0);
  t.stamp_clock = 0;
  t.n_slots = n_slots_new;
  return PAS_OK;
}

int pas_gas_card_names_info(const pas_ctx* ctx, int32_t* n_slots, int32_t* k, int64_t* n_bytes) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->gas_cards.valid) return PAS_ENOSNAP;
  if (n_slots) *n_slots = ctx->gas_cards.n_slots;
  if (k) *k = ctx->gas_cards.k;
  if (n_bytes) *n_bytes = ctx->gas_cards.pool_used;
  return PAS_OK;
}

int pas_gas_card_names_get(pas_ctx* ctx, int64_t* name_off_out, char* bytes_out, int64_t cap) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_card_names_get";
  GasCardNames& t = ctx->gas_cards;
  if (!t.valid) return no_table(ctx, fn.c_str());
  if (!name_off_out || cap < 0 || (cap > 0 && !bytes_out))
    return set_error(ctx, PAS_EINVAL, fn + ": null output or cap < 0");
  int rc = activate(ctx);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const size_t entries = (size_t)t.n_slots * (size_t)t.k;
  const bool fits = cap >= t.live_bytes;
  size_t scan_bytes = 0;
  if ((rc = scan_size<int64_t>(ctx, entries + 1, &scan_bytes))) return rc;
  Staging st(ctx);
  int64_t* d_off;
  char *d_bytes, *d_scan;
  st.out(d_off, name_off_out, entries + 1);
  st.out(d_bytes, bytes_out, fits ? (size_t)t.live_bytes : 0);
  st.work(d_scan, scan_bytes);
  if ((rc = st.upload())) return rc;
  if ((rc = scan_run<int64_t>(ctx, d_scan, scan_bytes, t.len, d_off, entries + 1, s))) return rc;
  if (fits && entries > 0) {
    cards_gather<<<blocks_for((int64_t)entries), kTpb, 0, s>>>((int64_t)entries, t.k, nullptr,
                                                               t.beg, t.len, t.pool, d_off,
                                                               d_bytes, t.live_bytes);
    PAS_HIP(ctx, hipGetLastError());
  }
  PAS_HIP(ctx, st.fetch());
  if (!fits)
    return set_error(ctx, PAS_ECAPACITY, fn + ": " + std::to_string(t.live_bytes) +
                                             " bytes of names, cap " + std::to_string(cap));
  return PAS_OK;
}

int pas_gas_card_names_drop(pas_ctx* ctx) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->gas_cards.valid) return no_table(ctx, "pas_gas_card_names_drop");
  ctx->gas_cards.valid = false;
  return PAS_OK;
}

}  // extern "C"
