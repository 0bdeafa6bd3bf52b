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
//            pool is gathered (pool_gathered, span_pool.hip: the storage is the node table's)
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

constexpr const char* kTable = "card-name table";

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTpb - 1) / kTpb); }

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

// t's pool gathered through the compact map src_slot (null: the rows as they are, the dead
// bytes dropped) into n_slots_new rows, and swapped in; host bookkeeping is the caller's.
// Synchronous on s.  On a failure the table stays as it was.
int gather_in(pas_ctx* ctx, GasCardNames& t, int32_t n_slots_new, const int32_t* src_slot,
              hipStream_t s, const std::string& fn) {
  const size_t n2 = (size_t)n_slots_new;
  size_t scan_bytes = 0;
  int rc = scan_size<int64_t>(ctx, n2 * (size_t)t.k + 1, &scan_bytes);
  if (rc) return rc;
  int32_t* d_src = nullptr;
  void* d_scan = nullptr;
  SpanPool nt;
  auto build = [&]() -> int {
    if (src_slot) {
      PAS_HIP(ctx, hipMalloc(&d_src, sizeof(int32_t) * std::max<size_t>(n2, 1)));
      if (n2) {
        const hipError_t e =
            hipMemcpyAsync(d_src, src_slot, sizeof(int32_t) * n2, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return check_hip(ctx, e, (fn + ": map upload").c_str());
      }
    }
    PAS_HIP(ctx, hipMalloc(&d_scan, scan_bytes));
    return pool_gathered(ctx, t.sp, n_slots_new, t.k, d_src, d_scan, scan_bytes, nullptr, nullptr,
                         &nt, s, kTable);
  };
  rc = build();
  (void)hipStreamSynchronize(s);
  free_dev(d_src);
  free_dev(d_scan);
  if (rc) return rc;
  free_pool(t.sp);
  t.sp = nt;
  return PAS_OK;
}

}  // namespace

int card_names_gather_dead(pas_ctx* ctx, hipStream_t s, const std::string& fn) {
  GasCardNames& t = ctx->gas_cards;
  if (t.sp.pool_used - t.sp.live_bytes > t.sp.live_bytes)  // more dead bytes than live ones
    return gather_in(ctx, t, t.n_slots, nullptr, s, fn);
  return PAS_OK;
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
  int rc = check_host_spans(ctx, entries, name_off, bytes, fn);
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = ctx->stream;
  GasCardNames nt;
  nt.n_slots = n_slots;
  nt.k = k;
  nt.row_bytes.resize((size_t)n_slots);
  for (int64_t r = 0; r < n_slots; ++r) nt.row_bytes[r] = name_off[(r + 1) * k] - name_off[r * k];
  nt.stamp.assign((size_t)n_slots, 0);
  Staging st(ctx);
  int64_t* d_off;
  st.in(d_off, name_off, (size_t)entries + 1);
  auto build = [&]() -> int {
    int r = st.upload();
    if (r) return r;
    if ((r = pool_set(ctx, nt.sp, entries, name_off, d_off, bytes, nullptr, s, kTable))) return r;
    PAS_HIP(ctx, hipStreamSynchronize(s));
    return PAS_OK;
  };
  if ((rc = build())) {  // the previous table stays as it was
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s);
    free_pool(nt.sp);
    return rc;
  }
  nt.valid = true;
  free_pool(ctx->gas_cards.sp);
  ctx->gas_cards = std::move(nt);
  return PAS_OK;
}

int pas_gas_card_names_update(pas_ctx* ctx, int32_t n_rows, const int32_t* row_slot,
                              const int64_t* name_off, const char* bytes) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_card_names_update";
  GasCardNames& t = ctx->gas_cards;
  if (!t.valid) return no_table(ctx, fn, kTable);
  if (n_rows < 0) return set_error(ctx, PAS_EINVAL, fn + ": n_rows < 0");
  if (n_rows == 0) return PAS_OK;
  if (!row_slot) return set_error(ctx, PAS_EINVAL, fn + ": null input");
  const int64_t entries = (int64_t)n_rows * t.k;
  int rc = check_host_spans(ctx, entries, name_off, bytes, fn);
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
  SpanPool& sp = t.sp;
  if ((rc = grow_pool(ctx, sp, total, s, "card-name table: pool copy"))) return rc;
  // nothing has changed so far; from here the table does
  if (total > 0)
    PAS_HIP(ctx, hipMemcpyAsync(sp.pool + sp.pool_used, bytes, (size_t)total,
                                hipMemcpyHostToDevice, s));
  cards_write_rows<<<blocks_for(entries), kTpb, 0, s>>>(entries, t.k, d_slot, d_keep, d_off,
                                                        sp.pool_used, sp.beg, sp.len);
  PAS_HIP(ctx, hipGetLastError());
  PAS_HIP(ctx, hipStreamSynchronize(s));
  sp.pool_used += total;
  for (int32_t r = 0; r < n_rows; ++r) {
    if (!keep[r]) continue;
    const int64_t b = name_off[(int64_t)(r + 1) * t.k] - name_off[(int64_t)r * t.k];
    sp.live_bytes += b - t.row_bytes[row_slot[r]];
    t.row_bytes[row_slot[r]] = b;
  }
  return card_names_gather_dead(ctx, s, fn);
}

int pas_gas_card_names_resize(pas_ctx* ctx, int32_t n_slots_new, int32_t k_new,
                              void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_card_names_resize";
  GasCardNames& t = ctx->gas_cards;
  if (!t.valid) return no_table(ctx, fn, kTable);
  if (n_slots_new < t.n_slots || k_new < t.k || k_new > PAS_GAS_MAX_CARDS)
    return set_error(ctx, PAS_EINVAL,
                     fn + ": " + std::to_string(n_slots_new) + " x " + std::to_string(k_new) +
                         ", the table has " + std::to_string(t.n_slots) + " x " +
                         std::to_string(t.k) + " (sizes only grow, k <= PAS_GAS_MAX_CARDS)");
  if (n_slots_new == t.n_slots && k_new == t.k) return PAS_OK;
  int rc = activate(ctx);
  if (rc) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  if ((rc = pool_repitch(ctx, t.sp, t.n_slots, t.k, n_slots_new, k_new, s, kTable, fn))) return rc;
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
  if (!t.valid) return no_table(ctx, fn, kTable);
  int rc = check_compact_map(ctx, n_slots_new, src_slot, t.n_slots, fn);
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  const size_t n2 = (size_t)n_slots_new;
  if ((rc = gather_in(ctx, t, n_slots_new, src_slot, pick_stream(ctx, hip_stream), fn)))
    return rc;  // the table stays as it was
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
  if (n_bytes) *n_bytes = ctx->gas_cards.sp.pool_used;
  return PAS_OK;
}

int pas_gas_card_names_get(pas_ctx* ctx, int64_t* name_off_out, char* bytes_out, int64_t cap) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_card_names_get";
  GasCardNames& t = ctx->gas_cards;
  if (!t.valid) return no_table(ctx, fn, kTable);
  return pool_get(ctx, t.sp, (int64_t)t.n_slots * t.k, name_off_out, bytes_out, cap, nullptr, fn);
}

int pas_gas_card_names_get_rows(pas_ctx* ctx, int32_t n_rows, const int32_t* row_slot,
                                int64_t* name_off_out, char* bytes_out, int64_t cap) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_card_names_get_rows";
  GasCardNames& t = ctx->gas_cards;
  if (!t.valid) return no_table(ctx, fn, kTable);
  if (n_rows < 0 || (n_rows > 0 && !row_slot)) return set_error(ctx, PAS_EINVAL, fn + ": bad rows");
  int64_t total = 0;
  for (int32_t r = 0; r < n_rows; ++r) {
    if (row_slot[r] < 0 || row_slot[r] >= t.n_slots)
      return set_error(ctx, PAS_EINVAL, fn + ": row " + std::to_string(r) + " names slot " +
                                            std::to_string(row_slot[r]) + ", the table has " +
                                            std::to_string(t.n_slots));
    total += t.row_bytes[row_slot[r]];
  }
  return pool_get_rows(ctx, t.sp, n_rows, t.k, row_slot, total, name_off_out, bytes_out, cap, fn);
}

int pas_gas_card_names_drop(pas_ctx* ctx) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->gas_cards.valid) return no_table(ctx, "pas_gas_card_names_drop", kTable);
  ctx->gas_cards.valid = false;
  return PAS_OK;
}

}  // extern "C"
