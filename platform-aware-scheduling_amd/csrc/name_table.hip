// name_table.hip — the resident node-name table: names resolved to slots on the device.
//
// The reference keys everything by node name (NodeMetricsInfo map[string]NodeMetric,
// telemetry-aware-scheduling/pkg/metrics/client.go:25-32; args.NodeNames,
// gpu-aware-scheduling/pkg/gpuscheduler/scheduler.go:455-470); slots exist only here.  The
// table (NameTable, pas_internal.h) maps one to the other beside the snapshots it indexes:
//   names_lookup    one lane per name: hash (name_hash.h), probe from the home bucket with
//                   wraparound, compare all bytes against the pool on a tag match
//   names_insert    one lane per slot: CAS claims an empty bucket, atomicMin keeps the lowest
//                   slot of a name (pas_names_set's duplicate check: a slot that does not find
//                   itself afterwards is a loser and flags itself)
//   assignment      (a) lookup, (b) the unknown entries deduped through a scratch table whose
//                   word carries the entry index (atomicMin: the first appearance, whatever the
//                   arrival order), (c) the firsts and the spare slots ranked by scans, the
//                   k-th first takes the k-th spare slot, (d) the new names appended to the
//                   pool at scanned offsets and inserted, (e) the repeats take their first's
//                   slot
// The names are adjacent in one blob, so neighbouring lanes read neighbouring bytes, as
// parse_literals does.  The table's layout may depend on arrival order; no output does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "csr_entry.h"
#include "host_staging.h"
#include "name_hash.h"
#include "pas_internal.h"
#include "span_pool.h"

namespace pas {
namespace {

constexpr int kTpb = 256;
constexpr unsigned long long kEmpty = ~0ull;
constexpr const char* kTable = "name table";

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTpb - 1) / kTpb); }

struct NameView {
  int64_t mask;  // buckets - 1
  unsigned long long* table;
  int64_t* beg;
  int64_t* len;
  char* pool;
};

inline NameView view_of(const NameTable& t) {
  return NameView{t.buckets - 1, t.table, t.sp.beg, t.sp.len, t.sp.pool};
}

inline int64_t buckets_for(int64_t n_slots) {
  int64_t b = 2;
  while (b < 2 * n_slots) b <<= 1;
  return b;
}

__device__ __forceinline__ unsigned long long make_word(uint64_t h, uint32_t low) {
  return ((unsigned long long)name_tag(h) << 32) | low;
}

// The slot of the name p[0 .. n) with hash h, or -1.  The table is at most half full, so a
// probe always ends at an empty bucket.
__device__ __forceinline__ int32_t table_find(const NameView& t, const char* __restrict__ p,
                                              int64_t n, uint64_t h) {
  if (n == 0) return -1;
  for (int64_t b = (int64_t)h & t.mask;; b = (b + 1) & t.mask) {
    const unsigned long long w = t.table[b];
    if (w == kEmpty) return -1;
    if ((uint32_t)(w >> 32) != name_tag(h)) continue;
    const int32_t s = (int32_t)(uint32_t)w;
    if (t.len[s] == n && bytes_equal(t.pool + t.beg[s], p, n)) return s;
  }
}

__global__ void names_lookup(int64_t n, int64_t n_bytes, const int64_t* __restrict__ off,
                             const char* __restrict__ bytes, NameView t,
                             int32_t* __restrict__ slot, uint64_t* __restrict__ hash,
                             uint32_t* unknown, int count_empty) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  bool miss = false;
  if (i < n) {
    int64_t b;
    const int64_t len = entry_span(off, n_bytes, i, &b);
    const uint64_t h = name_hash(bytes + b, len);
    const int32_t s = table_find(t, bytes + b, len, h);
    slot[i] = s;
    if (hash) hash[i] = h;
    miss = s < 0 && (len > 0 || count_empty);
  }
  if (!unknown) return;  // (uniform)
  const unsigned long long m = __ballot(miss);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(unknown, (uint32_t)__popcll(m));
}

// Slot list[i] (null: slot i) into the table.  A bucket belongs to the name that claimed it;
// slots of the same name only lower its word, so it keeps the lowest of them.
__global__ void names_insert(int64_t n, const int32_t* __restrict__ list, NameView t) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n) return;
  const int32_t s = list ? list[i] : (int32_t)i;
  const int64_t len = t.len[s];
  if (len == 0) return;
  const char* p = t.pool + t.beg[s];
  const uint64_t h = name_hash(p, len);
  const unsigned long long word = make_word(h, (uint32_t)s);
  for (int64_t b = (int64_t)h & t.mask;; b = (b + 1) & t.mask) {
    unsigned long long w = *(volatile unsigned long long*)&t.table[b];
    if (w == kEmpty) {
      w = atomicCAS(&t.table[b], kEmpty, word);
      if (w == kEmpty) return;
    }
    if ((uint32_t)(w >> 32) != name_tag(h)) continue;
    const int32_t s2 = (int32_t)(uint32_t)w;
    if (s2 == s) return;
    if (t.len[s2] == len && bytes_equal(t.pool + t.beg[s2], p, len)) {
      atomicMin(&t.table[b], word);
      return;
    }
  }
}

// ctr[0] = the lowest slot that does not find itself (its name stands in a lower slot)
__global__ void names_flag_losers(int64_t n_slots, NameView t, int32_t* ctr) {
  const int64_t s = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (s >= n_slots) return;
  const int64_t len = t.len[s];
  if (len == 0) return;
  const char* p = t.pool + t.beg[s];
  if (table_find(t, p, len, name_hash(p, len)) != (int32_t)s) atomicMin(&ctr[0], (int32_t)s);
}

// ---- assignment

// (b) every unknown entry into the scratch table (word = tag << 32 | entry index)
__global__ void assign_dedupe(int64_t n, int64_t n_bytes, const int64_t* __restrict__ off,
                              const char* __restrict__ bytes, const int32_t* __restrict__ slot,
                              const uint64_t* __restrict__ hash, int64_t mask,
                              unsigned long long* scratch) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n || slot[i] >= 0) return;
  int64_t b0;
  const int64_t len = entry_span(off, n_bytes, i, &b0);
  if (len == 0) return;
  const uint64_t h = hash[i];
  const unsigned long long word = make_word(h, (uint32_t)i);
  for (int64_t b = (int64_t)h & mask;; b = (b + 1) & mask) {
    unsigned long long w = *(volatile unsigned long long*)&scratch[b];
    if (w == kEmpty) {
      w = atomicCAS(&scratch[b], kEmpty, word);
      if (w == kEmpty) return;
    }
    if ((uint32_t)(w >> 32) != name_tag(h)) continue;
    const int64_t j = (int64_t)(uint32_t)w;
    if (j == i) return;
    int64_t bj;
    if (entry_span(off, n_bytes, j, &bj) == len && bytes_equal(bytes + bj, bytes + b0, len)) {
      atomicMin(&scratch[b], word);
      return;
    }
  }
}

// (c) first_of[i] = the first appearance of an unknown entry's name (-1: known or empty);
// flag / flen [n + 1] = 1 / the name's length at the firsts, 0 elsewhere (the scans' inputs)
__global__ void assign_firsts(int64_t n, int64_t n_bytes, const int64_t* __restrict__ off,
                              const char* __restrict__ bytes, const int32_t* __restrict__ slot,
                              const uint64_t* __restrict__ hash, int64_t mask,
                              const unsigned long long* __restrict__ scratch,
                              int32_t* __restrict__ first_of, uint32_t* __restrict__ flag,
                              int64_t* __restrict__ flen) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i > n) return;
  int32_t first = -1;
  int64_t len = 0, b0 = 0;
  if (i < n && slot[i] < 0) len = entry_span(off, n_bytes, i, &b0);
  if (len > 0) {
    const uint64_t h = hash[i];
    for (int64_t b = (int64_t)h & mask;; b = (b + 1) & mask) {
      const unsigned long long w = scratch[b];
      if (w == kEmpty) break;  // (every unknown entry was inserted: not reached)
      if ((uint32_t)(w >> 32) != name_tag(h)) continue;
      const int64_t j = (int64_t)(uint32_t)w;
      int64_t bj;
      if (j == i ||
          (entry_span(off, n_bytes, j, &bj) == len && bytes_equal(bytes + bj, bytes + b0, len))) {
        first = (int32_t)j;
        break;
      }
    }
  }
  const bool is_first = first == (int32_t)i && i < n;
  if (i < n) first_of[i] = first;
  flag[i] = is_first ? 1u : 0u;
  flen[i] = is_first ? len : 0;
}

__global__ void names_spare_flags(int64_t n_slots, const int64_t* __restrict__ len,
                                  uint32_t* __restrict__ flag) {
  const int64_t s = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (s <= n_slots) flag[s] = s < n_slots && len[s] == 0 ? 1u : 0u;
}

// the first n_new spare slots in ascending order
__global__ void assign_spares(int64_t n_slots, uint32_t n_new, const uint32_t* __restrict__ flag,
                              const uint32_t* __restrict__ rank, int32_t* __restrict__ spare) {
  const int64_t s = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (s < n_slots && flag[s] && rank[s] < n_new) spare[rank[s]] = (int32_t)s;
}

// (d) the k-th first takes the k-th spare slot; its name goes to the pool at its scanned offset
__global__ void assign_commit(int64_t n, int64_t n_bytes, const int64_t* __restrict__ off,
                              const char* __restrict__ bytes, const uint32_t* __restrict__ flag,
                              const uint32_t* __restrict__ rank, const int64_t* __restrict__ fpos,
                              const int32_t* __restrict__ spare, int64_t pool_used, NameView t,
                              int32_t* __restrict__ slot, int32_t* __restrict__ new_entry,
                              int32_t* __restrict__ new_slot) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const uint32_t k = rank[i];
  const int32_t s = spare[k];
  int64_t b;
  const int64_t len = entry_span(off, n_bytes, i, &b);
  const int64_t at = pool_used + fpos[i];
  for (int64_t j = 0; j < len; ++j) t.pool[at + j] = bytes[b + j];
  t.beg[s] = at;
  t.len[s] = len;
  slot[i] = s;
  new_entry[k] = (int32_t)i;
  new_slot[k] = s;
}

// (e) the repeats of a new name
__global__ void assign_repeats(int64_t n, const int32_t* __restrict__ first_of,
                               const uint32_t* __restrict__ flag, int32_t* slot) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n || flag[i] || first_of[i] < 0) return;
  slot[i] = slot[first_of[i]];  // (a first's entry: written by assign_commit, not here)
}

// A hash of `buckets` buckets over the named slots of t (its spans and pool in place),
// replacing t.table; synchronous on s when the bucket count changes (the old table is freed).
int rebuild_table(pas_ctx* ctx, NameTable& t, int64_t buckets, hipStream_t s) {
  if (buckets != t.buckets) {
    unsigned long long* nt = nullptr;
    PAS_HIP(ctx, hipMalloc(&nt, sizeof(unsigned long long) * (size_t)buckets));
    if (t.table) {
      const hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) {
        free_dev(nt);
        return check_hip(ctx, e, "name table: hipStreamSynchronize");
      }
      free_dev(t.table);
    }
    t.table = nt;
    t.buckets = buckets;
  }
  PAS_HIP(ctx, hipMemsetAsync(t.table, 0xff, sizeof(unsigned long long) * (size_t)t.buckets, s));
  if (t.n_slots > 0) {
    names_insert<<<blocks_for(t.n_slots), kTpb, 0, s>>>(t.n_slots, nullptr, view_of(t));
    PAS_HIP(ctx, hipGetLastError());
  }
  return PAS_OK;
}

// pas_names_assign[_device] on device arrays (d_slot may be null), synchronous on s.
int names_assign_launch(pas_ctx* ctx, int64_t n, ByteSpans names, int32_t* d_slot,
                        int64_t new_cap, int32_t* new_entry_out, int32_t* new_slot_out,
                        int64_t* n_new_out, hipStream_t s) {
  NameTable& t = ctx->names;
  const int64_t n_bytes = names.n_bytes;
  const int64_t* d_off = names.off;
  const char* d_bytes = names.bytes;
  if (n_new_out) *n_new_out = 0;
  if (n == 0) return PAS_OK;
  const size_t nn = (size_t)n, ns = (size_t)t.n_slots;
  int64_t sb = 2;  // scratch buckets: at most half full even when every entry is new
  while (sb < 2 * n) sb <<= 1;
  size_t scan_n = 0, scan_s = 0, scan64 = 0;
  int rc = scan_size<uint32_t>(ctx, nn + 1, &scan_n);
  if (!rc) rc = scan_size<uint32_t>(ctx, ns + 1, &scan_s);
  if (!rc) rc = scan_size<int64_t>(ctx, nn + 1, &scan64);
  if (rc) return rc;
  const size_t scan_bytes = std::max({scan_n, scan_s, scan64});
  SlotScope scope(ctx, s, 0, &rc);
  if (!scope.slot) return rc;
  const size_t total = carve_size(
      {sizeof(uint32_t) * 4, sizeof(int32_t) * nn, sizeof(uint64_t) * nn, sizeof(int32_t) * nn,
       sizeof(uint32_t) * (nn + 1), sizeof(uint32_t) * (nn + 1), sizeof(int64_t) * (nn + 1),
       sizeof(int64_t) * (nn + 1), sizeof(uint32_t) * (ns + 1), sizeof(uint32_t) * (ns + 1),
       sizeof(int32_t) * nn, sizeof(int32_t) * nn, sizeof(int32_t) * nn,
       sizeof(unsigned long long) * (size_t)sb, scan_bytes});
  char* base = static_cast<char*>(slot_buf(ctx, scope.slot, kBufNames, total, s, &rc));
  if (!base) return rc;
  Carve cv{base};
  uint32_t* d_ctr = cv.take<uint32_t>(4);
  int32_t* d_own_slot = cv.take<int32_t>(nn);
  uint64_t* d_hash = cv.take<uint64_t>(nn);
  int32_t* d_first_of = cv.take<int32_t>(nn);
  uint32_t* d_flag = cv.take<uint32_t>(nn + 1);
  uint32_t* d_rank = cv.take<uint32_t>(nn + 1);
  int64_t* d_flen = cv.take<int64_t>(nn + 1);
  int64_t* d_fpos = cv.take<int64_t>(nn + 1);
  uint32_t* d_sflag = cv.take<uint32_t>(ns + 1);
  uint32_t* d_srank = cv.take<uint32_t>(ns + 1);
  int32_t* d_spare = cv.take<int32_t>(nn);
  int32_t* d_new_entry = cv.take<int32_t>(nn);
  int32_t* d_new_slot = cv.take<int32_t>(nn);
  unsigned long long* d_scratch = cv.take<unsigned long long>((size_t)sb);
  void* d_scan = cv.take<char>(scan_bytes);
  if (!d_slot) d_slot = d_own_slot;

  // (a) the lookups; one word back: the entries that name a new node
  PAS_HIP(ctx, hipMemsetAsync(d_ctr, 0, sizeof(uint32_t) * 4, s));
  rc = names_resolve_launch(ctx, n, names, d_slot, d_hash, d_ctr, false, s);
  if (rc) return rc;
  uint32_t n_unknown = 0;
  PAS_HIP(ctx, hipMemcpyAsync(&n_unknown, d_ctr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PAS_HIP(ctx, hipStreamSynchronize(s));
  if (n_unknown == 0) return PAS_OK;

  // (b), (c): firsts and spare slots, ranked
  PAS_HIP(ctx, hipMemsetAsync(d_scratch, 0xff, sizeof(unsigned long long) * (size_t)sb, s));
  assign_dedupe<<<blocks_for(n), kTpb, 0, s>>>(n, n_bytes, d_off, d_bytes, d_slot, d_hash, sb - 1,
                                               d_scratch);
  PAS_HIP(ctx, hipGetLastError());
  assign_firsts<<<blocks_for(n + 1), kTpb, 0, s>>>(n, n_bytes, d_off, d_bytes, d_slot, d_hash,
                                                   sb - 1, d_scratch, d_first_of, d_flag, d_flen);
  PAS_HIP(ctx, hipGetLastError());
  names_spare_flags<<<blocks_for(t.n_slots + 1), kTpb, 0, s>>>(t.n_slots, t.sp.len, d_sflag);
  PAS_HIP(ctx, hipGetLastError());
  if ((rc = scan_run<uint32_t>(ctx, d_scan, scan_bytes, d_flag, d_rank, nn + 1, s))) return rc;
  if ((rc = scan_run<int64_t>(ctx, d_scan, scan_bytes, d_flen, d_fpos, nn + 1, s))) return rc;
  if ((rc = scan_run<uint32_t>(ctx, d_scan, scan_bytes, d_sflag, d_srank, ns + 1, s))) return rc;
  uint32_t n_new = 0, n_spare = 0;
  int64_t new_bytes = 0;
  PAS_HIP(ctx, hipMemcpyAsync(&n_new, d_rank + nn, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PAS_HIP(ctx, hipMemcpyAsync(&n_spare, d_srank + ns, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PAS_HIP(ctx, hipMemcpyAsync(&new_bytes, d_fpos + nn, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  PAS_HIP(ctx, hipStreamSynchronize(s));
  if (n_new_out) *n_new_out = n_new;
  if ((int64_t)n_new > std::min<int64_t>(n_spare, new_cap))
    return set_error(ctx, PAS_ECAPACITY,
                     "pas_names_assign: " + std::to_string(n_new) + " new names, " +
                         std::to_string(n_spare) + " spare slots, new_cap " +
                         std::to_string(new_cap));
  if (!new_entry_out || !new_slot_out)
    return set_error(ctx, PAS_EINVAL, "pas_names_assign: new names and null output arrays");

  // (d), (e): nothing has changed so far; from here the table does
  if ((rc = grow_pool(ctx, t.sp, new_bytes, s, "name table: pool copy"))) return rc;
  assign_spares<<<blocks_for(t.n_slots), kTpb, 0, s>>>(t.n_slots, n_new, d_sflag, d_srank,
                                                       d_spare);
  PAS_HIP(ctx, hipGetLastError());
  assign_commit<<<blocks_for(n), kTpb, 0, s>>>(n, n_bytes, d_off, d_bytes, d_flag, d_rank, d_fpos,
                                               d_spare, t.sp.pool_used, view_of(t), d_slot,
                                               d_new_entry, d_new_slot);
  PAS_HIP(ctx, hipGetLastError());
  names_insert<<<blocks_for(n_new), kTpb, 0, s>>>(n_new, d_new_slot, view_of(t));
  PAS_HIP(ctx, hipGetLastError());
  assign_repeats<<<blocks_for(n), kTpb, 0, s>>>(n, d_first_of, d_flag, d_slot);
  PAS_HIP(ctx, hipGetLastError());
  t.sp.pool_used = t.sp.live_bytes = t.sp.pool_used + new_bytes;
  t.n_named += (int32_t)n_new;
  PAS_HIP(ctx, hipMemcpyAsync(new_entry_out, d_new_entry, sizeof(int32_t) * n_new,
                              hipMemcpyDeviceToHost, s));
  PAS_HIP(ctx, hipMemcpyAsync(new_slot_out, d_new_slot, sizeof(int32_t) * n_new,
                              hipMemcpyDeviceToHost, s));
  if ((rc = derived_built(ctx, ctx->names_sync, s))) return rc;
  PAS_HIP(ctx, hipStreamSynchronize(s));
  return PAS_OK;
}

}  // namespace

void free_names(NameTable& t) {
  free_pool(t.sp);
  free_dev(t.table);
  t = NameTable{};
}

int names_resolve_launch(pas_ctx* ctx, int64_t n, ByteSpans names, int32_t* d_slot,
                         uint64_t* d_hash, uint32_t* d_unknown, bool count_empty, hipStream_t s) {
  if (n <= 0) return PAS_OK;
  int rc = derived_wait(ctx, ctx->names_sync, s);
  if (rc) return rc;
  names_lookup<<<blocks_for(n), kTpb, 0, s>>>(n, names.n_bytes, names.off, names.bytes,
                                              view_of(ctx->names), d_slot, d_hash, d_unknown,
                                              count_empty ? 1 : 0);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

}  // namespace pas

using namespace pas;

extern "C" {

uint64_t pas_name_hash(const char* bytes, int64_t len) {
  return bytes && len > 0 ? name_hash(bytes, len) : name_hash("", 0);
}

int pas_names_set(pas_ctx* ctx, int32_t n_slots, const int64_t* name_off, const char* bytes) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_names_set";
  if (n_slots < 0) return set_error(ctx, PAS_EINVAL, fn + ": n_slots < 0");
  int rc = check_host_spans(ctx, n_slots, name_off, bytes, fn);
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = ctx->stream;
  NameTable nt;
  nt.n_slots = n_slots;
  int32_t* d_ctr = nullptr;  // {lowest loser, named slots}
  const int32_t ctr0[2] = {INT32_MAX, 0};
  int32_t ctr[2] = {INT32_MAX, 0};
  Staging st(ctx);
  int64_t* d_off;
  st.in(d_off, name_off, (size_t)n_slots + 1);
  st.work(d_ctr, 2);
  auto build = [&]() -> int {
    int r = st.upload();
    if (r) return r;
    PAS_HIP(ctx, hipMemcpyAsync(d_ctr, ctr0, sizeof(ctr0), hipMemcpyHostToDevice, s));
    if ((r = pool_set(ctx, nt.sp, n_slots, name_off, d_off, bytes, d_ctr + 1, s, kTable)))
      return r;
    if ((r = rebuild_table(ctx, nt, buckets_for(n_slots), s))) return r;
    if (n_slots > 0) {
      names_flag_losers<<<blocks_for(n_slots), kTpb, 0, s>>>(n_slots, view_of(nt), d_ctr);
      PAS_HIP(ctx, hipGetLastError());
    }
    PAS_HIP(ctx, hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
    PAS_HIP(ctx, hipStreamSynchronize(s));
    return PAS_OK;
  };
  rc = build();
  if (!rc && ctr[0] != INT32_MAX)
    rc = set_error(ctx, PAS_EINVAL, fn + ": slot " + std::to_string(ctr[0]) +
                                        " holds a name that also stands in a lower slot");
  if (rc) {  // the previous table stays as it was
    (void)hipStreamSynchronize(s);
    free_names(nt);
    return rc;
  }
  nt.n_named = ctr[1];
  nt.valid = true;
  free_names(ctx->names);
  ctx->names = nt;
  return derived_built(ctx, ctx->names_sync, s);
}

int pas_names_info(const pas_ctx* ctx, int32_t* n_slots, int32_t* n_named, int64_t* n_bytes) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->names.valid) return PAS_ENOSNAP;
  if (n_slots) *n_slots = ctx->names.n_slots;
  if (n_named) *n_named = ctx->names.n_named;
  if (n_bytes) *n_bytes = ctx->names.sp.pool_used;
  return PAS_OK;
}

int pas_names_drop(pas_ctx* ctx) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->names.valid) return no_table(ctx, "pas_names_drop", kTable);
  ctx->names.valid = false;
  return PAS_OK;
}

int pas_names_get(pas_ctx* ctx, int64_t* name_off_out, char* bytes_out, int64_t cap) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_names_get";
  NameTable& t = ctx->names;
  if (!t.valid) return no_table(ctx, fn, kTable);
  return pool_get(ctx, t.sp, t.n_slots, name_off_out, bytes_out, cap, &ctx->names_sync, fn);
}

int pas_names_resolve_device(pas_ctx* ctx, int64_t n, int64_t n_bytes, const int64_t* d_name_off,
                             const char* d_bytes, int32_t* d_slot_out, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_names_resolve_device";
  if (!ctx->names.valid) return no_table(ctx, fn, kTable);
  const ByteSpans names{n_bytes, d_name_off, d_bytes};
  if (n < 0) return set_error(ctx, PAS_EINVAL, fn + ": n < 0");
  int rc = check_device_spans(ctx, n, names, fn);
  if (rc || n == 0) return rc;
  if (!d_slot_out) return set_error(ctx, PAS_EINVAL, fn + ": null output");
  if ((rc = activate(ctx))) return rc;
  return names_resolve_launch(ctx, n, names, d_slot_out, nullptr, nullptr, false,
                              pick_stream(ctx, hip_stream));
}

int pas_names_resolve(pas_ctx* ctx, int64_t n, const int64_t* name_off, const char* bytes,
                      int32_t* slot_out) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_names_resolve";
  if (!ctx->names.valid) return no_table(ctx, fn, kTable);
  if (n < 0) return set_error(ctx, PAS_EINVAL, fn + ": n < 0");
  if (n == 0) return PAS_OK;
  int rc = check_host_spans(ctx, n, name_off, bytes, fn);
  if (rc) return rc;
  if (!slot_out) return set_error(ctx, PAS_EINVAL, fn + ": null output");
  if ((rc = activate(ctx))) return rc;
  Staging st(ctx);
  ByteSpans names;
  int32_t* d_slot;
  st.in_spans(names, n, name_off, bytes);
  st.out(d_slot, slot_out, (size_t)n);
  if ((rc = st.upload())) return rc;
  rc = names_resolve_launch(ctx, n, names, d_slot, nullptr, nullptr, false, ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_names_assign_device(pas_ctx* ctx, int64_t n, int64_t n_bytes, const int64_t* d_name_off,
                            const char* d_bytes, int32_t* d_slot_out, int64_t new_cap,
                            int32_t* new_entry_out, int32_t* new_slot_out, int64_t* n_new_out,
                            void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_names_assign_device";
  if (n_new_out) *n_new_out = 0;
  if (!ctx->names.valid) return no_table(ctx, fn, kTable);
  const ByteSpans names{n_bytes, d_name_off, d_bytes};
  if (n < 0 || n > INT32_MAX || new_cap < 0)
    return set_error(ctx, PAS_EINVAL, fn + ": n or new_cap out of range");
  int rc = check_device_spans(ctx, n, names, fn);
  if (rc || n == 0) return rc;
  if ((rc = activate(ctx))) return rc;
  return names_assign_launch(ctx, n, names, d_slot_out, new_cap, new_entry_out, new_slot_out,
                             n_new_out, pick_stream(ctx, hip_stream));
}

int pas_names_assign(pas_ctx* ctx, int64_t n, const int64_t* name_off, const char* bytes,
                     int32_t* slot_out, int64_t new_cap, int32_t* new_entry_out,
                     int32_t* new_slot_out, int64_t* n_new_out) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_names_assign";
  if (n_new_out) *n_new_out = 0;
  if (!ctx->names.valid) return no_table(ctx, fn, kTable);
  if (n < 0 || n > INT32_MAX || new_cap < 0)
    return set_error(ctx, PAS_EINVAL, fn + ": n or new_cap out of range");
  if (n == 0) return PAS_OK;
  int rc = check_host_spans(ctx, n, name_off, bytes, fn);
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  Staging st(ctx);
  ByteSpans names;
  int32_t* d_slot;
  st.in_spans(names, n, name_off, bytes);
  st.out_opt(d_slot, slot_out, (size_t)n);
  if ((rc = st.upload())) return rc;
  rc = names_assign_launch(ctx, n, names, d_slot, new_cap, new_entry_out, new_slot_out,
                           n_new_out, ctx->stream);
  if (rc && rc != PAS_ECAPACITY) return rc;
  const std::string msg = ctx->err;  // (PAS_ECAPACITY: slot_out holds the plain lookups)
  PAS_HIP(ctx, st.fetch());
  if (rc) ctx->err = msg;
  return rc;
}

int pas_names_resize(pas_ctx* ctx, int32_t n_slots_new, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_names_resize";
  NameTable& t = ctx->names;
  if (!t.valid) return no_table(ctx, fn, kTable);
  if (n_slots_new < t.n_slots)
    return set_error(ctx, PAS_EINVAL, fn + ": " + std::to_string(n_slots_new) + " slots, the " +
                                          "table has " + std::to_string(t.n_slots));
  int rc = activate(ctx);
  if (rc) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  if (n_slots_new > t.sp.span_cap &&
      (rc = pool_repitch(ctx, t.sp, t.n_slots, 1, n_slots_new, 1, s, kTable, fn)))
    return rc;
  t.n_slots = n_slots_new;
  if (2 * (int64_t)n_slots_new > t.buckets)  // the load factor would pass 1/2
    if ((rc = rebuild_table(ctx, t, buckets_for(n_slots_new), s))) return rc;
  if ((rc = derived_built(ctx, ctx->names_sync, s))) return rc;
  PAS_HIP(ctx, hipStreamSynchronize(s));
  return PAS_OK;
}

int pas_names_remap(pas_ctx* ctx, int32_t n_slots_new, const int32_t* src_slot,
                    void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_names_remap";
  NameTable& t = ctx->names;
  if (!t.valid) return no_table(ctx, fn, kTable);
  int rc = check_compact_map(ctx, n_slots_new, src_slot, t.n_slots, fn);
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  const size_t n2 = (size_t)n_slots_new;
  size_t scan_bytes = 0;
  if ((rc = scan_size<int64_t>(ctx, n2 + 1, &scan_bytes))) return rc;
  SlotScope scope(ctx, s, 0, &rc);
  if (!scope.slot) return rc;
  const size_t total = carve_size({sizeof(int32_t), sizeof(int32_t) * n2, scan_bytes});
  char* base = static_cast<char*>(slot_buf(ctx, scope.slot, kBufNames, total, s, &rc));
  if (!base) return rc;
  Carve cv{base};
  int32_t* d_named = cv.take<int32_t>(1);
  int32_t* d_src = cv.take<int32_t>(n2);
  void* d_scan = cv.take<char>(scan_bytes);
  NameTable nt;
  nt.n_slots = n_slots_new;
  auto build = [&]() -> int {
    PAS_HIP(ctx, hipMemsetAsync(d_named, 0, sizeof(int32_t), s));
    if (n2)
      PAS_HIP(ctx, hipMemcpyAsync(d_src, src_slot, sizeof(int32_t) * n2, hipMemcpyHostToDevice, s));
    int r = pool_gathered(ctx, t.sp, n_slots_new, 1, d_src, d_scan, scan_bytes, d_named,
                          &nt.n_named, &nt.sp, s, kTable);
    if (r) return r;
    if ((r = rebuild_table(ctx, nt, buckets_for(n_slots_new), s))) return r;
    PAS_HIP(ctx, hipStreamSynchronize(s));
    return PAS_OK;
  };
  rc = build();
  if (rc) {  // the table stays as it was
    (void)hipStreamSynchronize(s);
    free_names(nt);
    return rc;
  }
  nt.valid = true;
  free_names(t);
  ctx->names = nt;
  return derived_built(ctx, ctx->names_sync, s);
}

}  // extern "C"
