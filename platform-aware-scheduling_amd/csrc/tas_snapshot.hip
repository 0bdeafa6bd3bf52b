// tas_snapshot.hip — device-side build of the resident TAS snapshot, whole or per column.
//
// The reference re-derives node order per request: core.OrderedList ranges over the
// metric's map and sort.Slice-s it with Quantity.Cmp on every prioritize call
// (telemetry-aware-scheduling/pkg/strategies/core/operator.go:30-42), and every
// dontschedule rule scans the whole metric map (dontschedule/strategy.go:33-41).
// Here the snapshot (one AutoUpdatingCache refresh, cache/autoupdating.go:37-59) is
// sorted once per metric into three orders — ascending, descending, node index.  A
// rule's violating set is then a contiguous range of the ascending order, and a pod's
// prioritize list is a compaction of one order by the pod's pass bits.
//
// The cache refreshes one metric at a time (updateAllMetrics -> updateMetric ->
// WriteMetric replaces the metric's whole node map, autoupdating.go:45-73), so a column is
// the unit of update: tas_snapshot_update rebuilds the orders of the given columns only.
//
// Build of C columns (all M for a full upload):
//   1. per-word popcounts of the columns' presence bitmaps and their exclusive scan;
//   2. compaction, one thread per order position j of a column: a present node j goes to
//      its rank among the column's present nodes (coalesced: consecutive present nodes,
//      consecutive positions), positions past cnt get a pad;
//   3. one device-wide stable radix sort of keys {value, column} with node ids as values
//      (C*R pairs: every column occupies exactly R sorted positions, pads last), then the
//      same with {~value, column} for the descending order.  The keyed device-wide sort
//      fills the GPU, where a segmented sort runs one workgroup per column;
//   4. placement into the snapshot rows, with the range-search fences.
// Ties: the sorts are stable and the compacted input is in node-index order, so equal
// values stay in ascending node index in both orders (the documented tie-break; the
// reference's is unspecified Go-map order).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <type_traits>

#include "pas_internal.h"

namespace pas {
namespace {

constexpr int kTpb = 256;

// Sort key: the column's value (or ~value for the descending order) below the column
// index; pads carry INT64_MAX and follow every value of their column (stable sort, pads
// after the column's present nodes in the input).
struct SortKey {
  int64_t v;
  uint32_t c;
  uint32_t pad;
};
struct SortKeyBits {
  __host__ __device__ rocprim::tuple<uint32_t&, int64_t&> operator()(SortKey& k) const {
    return rocprim::tuple<uint32_t&, int64_t&>(k.c, k.v);
  }
};
// Wide columns (value = v + pad * 1e-9, v the floor): pad carries the nanos below the floor,
// so the key order is the exact order of the pairs.  The second instantiation of the same
// sort: the narrow build keeps its 64 + column bits.  Pads carry {INT64_MAX, 0xffffffff}.
struct WideKeyBits {
  __host__ __device__ rocprim::tuple<uint32_t&, int64_t&, uint32_t&> operator()(SortKey& k) const {
    return rocprim::tuple<uint32_t&, int64_t&, uint32_t&>(k.c, k.v, k.pad);
  }
};
template <bool kWide>
using KeyBits = std::conditional_t<kWide, WideKeyBits, SortKeyBits>;
template <bool kWide>
constexpr unsigned kValueBits = kWide ? 96 : 64;  // key bits below the column index
constexpr uint32_t kNanoMax = 999999999u;

__device__ __forceinline__ int32_t row_of(const int32_t* rows, int32_t c) {
  return rows ? rows[c] : c;
}

// popc[c*W + w] = present nodes in word w of column c; the last entry (c*W == C*W) is 0 so
// the exclusive scan yields every column's end.
__global__ void popc_words(const uint64_t* __restrict__ present, int64_t total_words,
                           int32_t N, int64_t W, uint32_t* __restrict__ popc) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i > total_words) return;
  popc[i] = i < total_words ? (uint32_t)__popcll(word_mask(present[i], i % W, N)) : 0u;
}

// One thread per (column c, order position j < R).  kWide: nano [M][N] are the snapshot's
// rows (already clamped), read at the column's row.
template <bool kWide>
__global__ void compact_keys(const uint64_t* __restrict__ present,
                             const int64_t* __restrict__ vals,
                             const uint32_t* __restrict__ nano, const uint32_t* __restrict__ scan,
                             const int32_t* __restrict__ rows, int32_t C, int32_t N, int32_t R,
                             int64_t W, int32_t MR, SortKey* __restrict__ keys,
                             int32_t* __restrict__ ids, int32_t* __restrict__ perm_index) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= (int64_t)C * R) return;
  const int32_t c = (int32_t)(i / R), j = (int32_t)(i % R);
  const int64_t m = row_of(rows, c);
  const uint32_t base = scan[(int64_t)c * W];
  const int32_t cnt = (int32_t)(scan[(int64_t)(c + 1) * W] - base);
  const int32_t sentinel = (int32_t)(W * 64);
  const int64_t out = (int64_t)c * R;
  if (j < N) {
    const int64_t w = j >> 6;
    const uint64_t bits = word_mask(present[(int64_t)c * W + w], w, N);
    if ((bits >> (j & 63)) & 1ull) {
      const int32_t pos = (int32_t)(scan[(int64_t)c * W + w] - base) +
                          __popcll(bits & ((1ull << (j & 63)) - 1ull));
      keys[out + pos] =
          SortKey{vals[(int64_t)c * N + j], (uint32_t)c, kWide ? nano[m * N + j] : 0u};
      ids[out + pos] = j;
      perm_index[(int64_t)kOrderIndex * MR + m * R + pos] = j;
    }
  }
  if (j >= cnt) {
    keys[out + j] = SortKey{INT64_MAX, (uint32_t)c, kWide ? 0xffffffffu : 0u};
    ids[out + j] = sentinel;
    perm_index[(int64_t)kOrderIndex * MR + m * R + j] = sentinel;
  }
}

// Ascending result -> sorted / perm_asc rows and the fences (f32[m][b] = sorted[32 b],
// f1k[m][a] = sorted[1024 a], 0 past cnt); the input keys become the descending keys
// (v1 < v2 <=> ~v1 > ~v2, no overflow).  kWide: floors and nanos of the sorted pairs side by
// side, fences of both; the descending keys complement both fields.
template <bool kWide>
__global__ void place_asc(const SortKey* __restrict__ skeys, const int32_t* __restrict__ sids,
                          SortKey* __restrict__ keys, const uint32_t* __restrict__ scan,
                          const int32_t* __restrict__ rows, int32_t C, int32_t R, int64_t W,
                          int32_t MR, int64_t* __restrict__ sorted, int32_t* __restrict__ perm,
                          int32_t* __restrict__ cnt_out, int64_t* __restrict__ f1k,
                          int64_t* __restrict__ f32, uint32_t* __restrict__ sorted_nano,
                          uint32_t* __restrict__ f1k_nano, uint32_t* __restrict__ f32_nano) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= (int64_t)C * R) return;
  const int32_t c = (int32_t)(i / R), j = (int32_t)(i % R);
  const int64_t m = row_of(rows, c);
  const int32_t cnt = (int32_t)(scan[(int64_t)(c + 1) * W] - scan[(int64_t)c * W]);
  const SortKey k = skeys[i];
  sorted[m * R + j] = k.v;
  if constexpr (kWide) sorted_nano[m * R + j] = k.pad;
  perm[(int64_t)kOrderAsc * MR + m * R + j] = sids[i];
  if ((j & 31) == 0) {
    const int64_t f = j < cnt ? k.v : 0;
    const uint32_t fn = j < cnt ? k.pad : 0u;
    f32[m * (R >> 5) + (j >> 5)] = f;
    if constexpr (kWide) f32_nano[m * (R >> 5) + (j >> 5)] = fn;
    if ((j & 1023) == 0) {
      f1k[m * (R >> 10) + (j >> 10)] = f;
      if constexpr (kWide) f1k_nano[m * (R >> 10) + (j >> 10)] = fn;
    }
  }
  if (j == 0) cnt_out[m] = cnt;
  if (j < cnt) {
    keys[i].v = ~keys[i].v;
    if constexpr (kWide) keys[i].pad = ~keys[i].pad;
  }
}

// nano [C][N] of an update into the snapshot's rows, clamped below 1e9 (the device form
// cannot check it on the host).
__global__ void clamp_nano(const uint32_t* __restrict__ in, const int32_t* __restrict__ rows,
                           int32_t C, int32_t N, uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= (int64_t)C * N) return;
  const int32_t c = (int32_t)(i / N), j = (int32_t)(i % N);
  out[(int64_t)rows[c] * N + j] = min(in[i], kNanoMax);
}

__global__ void place_desc(const int32_t* __restrict__ sids, const int32_t* __restrict__ rows,
                           int32_t C, int32_t R, int32_t MR, int32_t* __restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= (int64_t)C * R) return;
  const int32_t c = (int32_t)(i / R), j = (int32_t)(i % R);
  perm[(int64_t)kOrderDesc * MR + (int64_t)row_of(rows, c) * R + j] = sids[i];
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTpb - 1) / kTpb); }

inline unsigned bits_for(int32_t c) {  // bits of the column index in the sort key
  unsigned b = 1;
  while (b < 31 && (int64_t(1) << b) < c) ++b;
  return b;
}

// Temp storage of the largest (whole-snapshot, M columns of row R) sort of either key width.
template <bool kWide>
int alloc_sort_tmp(pas_ctx* ctx, TasSnapshot& t, size_t mr, int32_t M, hipStream_t s) {
  size_t sort_bytes = 0;
  SortKey* ka = static_cast<SortKey*>(t.keys_a);
  SortKey* kb = static_cast<SortKey*>(t.keys_b);
  PAS_HIP(ctx, rocprim::radix_sort_pairs(nullptr, sort_bytes, ka, kb, t.ids_a, t.ids_b, mr,
                                         KeyBits<kWide>{}, 0u,
                                         kValueBits<kWide> + bits_for(std::max(M, 1)), s));
  size_t& bytes = kWide ? t.wide_sort_tmp_bytes : t.sort_tmp_bytes;
  bytes = std::max<size_t>(sort_bytes, 16);
  PAS_HIP(ctx, hipMalloc(kWide ? &t.wide_sort_tmp : &t.sort_tmp, bytes));
  return PAS_OK;
}

// Orders of C columns whose values / presence sit at vals [C][N] / present [C][W]
// (rows: snapshot row of each column, nullptr = identity).  kWide: vals are the floors, the
// nanos are already in t.nano's rows.
template <bool kWide>
int build_columns(pas_ctx* ctx, int32_t C, const int32_t* d_rows, const int64_t* vals,
                  const uint64_t* present, hipStream_t s) {
  TasSnapshot& t = ctx->tas;
  const int32_t N = t.n_nodes, R = t.row;
  const int64_t W = w64(N);
  const int32_t MR = t.n_metrics * R;
  const int64_t cw = (int64_t)C * W;
  const int64_t cr = (int64_t)C * R;
  popc_words<<<blocks_for(cw + 1), kTpb, 0, s>>>(present, cw, N, W, t.popc);
  PAS_HIP(ctx, hipGetLastError());
  size_t scan_bytes = t.scan_tmp_bytes;
  PAS_HIP(ctx, rocprim::exclusive_scan(t.scan_tmp, scan_bytes, t.popc, t.word_scan, 0u,
                                       (size_t)(cw + 1), rocprim::plus<uint32_t>(), s));
  SortKey* ka = static_cast<SortKey*>(t.keys_a);
  SortKey* kb = static_cast<SortKey*>(t.keys_b);
  compact_keys<kWide><<<blocks_for(cr), kTpb, 0, s>>>(present, vals, t.nano, t.word_scan, d_rows,
                                                     C, N, R, W, MR, ka, t.ids_a, t.perm);
  PAS_HIP(ctx, hipGetLastError());
  const unsigned end_bit = kValueBits<kWide> + bits_for(C);
  void* const sort_tmp = kWide ? t.wide_sort_tmp : t.sort_tmp;
  const size_t sort_tmp_bytes = kWide ? t.wide_sort_tmp_bytes : t.sort_tmp_bytes;
  size_t sort_bytes = sort_tmp_bytes;
  PAS_HIP(ctx, rocprim::radix_sort_pairs(sort_tmp, sort_bytes, ka, kb, t.ids_a, t.ids_b,
                                         (size_t)cr, KeyBits<kWide>{}, 0u, end_bit, s));
  place_asc<kWide><<<blocks_for(cr), kTpb, 0, s>>>(kb, t.ids_b, ka, t.word_scan, d_rows, C, R, W,
                                                  MR, t.sorted, t.perm, t.cnt, t.f1k, t.f32,
                                                  t.sorted_nano, t.f1k_nano, t.f32_nano);
  PAS_HIP(ctx, hipGetLastError());
  sort_bytes = sort_tmp_bytes;
  PAS_HIP(ctx, rocprim::radix_sort_pairs(sort_tmp, sort_bytes, ka, kb, t.ids_a, t.ids_b,
                                         (size_t)cr, KeyBits<kWide>{}, 0u, end_bit, s));
  place_desc<<<blocks_for(cr), kTpb, 0, s>>>(t.ids_b, d_rows, C, R, MR, t.perm);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

// Storage of the wide parts, on the first wide column of a snapshot shape.
int ensure_wide(pas_ctx* ctx, hipStream_t s) {
  return ctx->tas.wide_flag ? PAS_OK : tas_alloc_wide(ctx, ctx->tas, s);
}

// Columns cols[0 .. n_cols) become wide (1) or narrow (0): host marks, count, device flags.
// Nothing to do (and nothing touched) while the snapshot has never held a wide column.
int mark_wide(pas_ctx* ctx, int32_t n_cols, const int32_t* cols, uint8_t wide, hipStream_t s) {
  TasSnapshot& t = ctx->tas;
  if (!t.wide_flag) return PAS_OK;
  bool changed = false;
  for (int32_t c = 0; c < n_cols; ++c) {
    uint8_t& f = t.wide_host[(size_t)cols[c]];
    changed |= f != wide;
    t.n_wide += (int32_t)wide - (int32_t)f;
    f = wide;
  }
  if (changed)  // wide_host lives as long as the snapshot; callers synchronize s after this
    PAS_HIP(ctx, hipMemcpyAsync(t.wide_flag, t.wide_host.data(), (size_t)t.n_metrics,
                                hipMemcpyHostToDevice, s));
  return PAS_OK;
}

// The columns cols[0 .. n_cols) replaced by d_vals / d_present (kWide: floors d_vals, nanos
// d_nano; the columns become wide, else narrow) and their orders rebuilt.
template <bool kWide>
int update_columns(pas_ctx* ctx, uint64_t gen, int32_t n_cols, const int32_t* cols,
                   const int64_t* d_vals, const uint32_t* d_nano, const uint64_t* d_present,
                   hipStream_t s) {
  TasSnapshot& t = ctx->tas;
  const int32_t N = t.n_nodes;
  const int64_t W = w64(N);
  if (n_cols > 0) {
    if constexpr (kWide) {
      if (int rc = ensure_wide(ctx, s)) {
        t.valid = false;
        return rc;
      }
    }
    // the new columns into their snapshot rows, then their orders
    for (int32_t c = 0; c < n_cols && N > 0; ++c) {
      const int64_t m = cols[c];
      PAS_HIP(ctx, hipMemcpyAsync(t.vals + m * N, d_vals + (int64_t)c * N, sizeof(int64_t) * N,
                                  hipMemcpyDeviceToDevice, s));
      PAS_HIP(ctx, hipMemcpyAsync(t.present + m * W, d_present + (int64_t)c * W,
                                  sizeof(uint64_t) * W, hipMemcpyDeviceToDevice, s));
    }
    PAS_HIP(ctx, hipMemcpyAsync(t.rows, cols, sizeof(int32_t) * n_cols, hipMemcpyHostToDevice,
                                s));
    // (a wide column refreshed by a narrow update is narrow again, at its recorded scale)
    if (int rc = mark_wide(ctx, n_cols, cols, kWide ? 1 : 0, s)) return rc;
    // cols is a caller-owned host array: wait for its copy before returning
    PAS_HIP(ctx, hipStreamSynchronize(s));
    t.valid = false;
    if constexpr (kWide) {
      if (N > 0) {
        clamp_nano<<<blocks_for((int64_t)n_cols * N), kTpb, 0, s>>>(d_nano, t.rows, n_cols, N,
                                                                   t.nano);
        PAS_HIP(ctx, hipGetLastError());
      }
    }
    if (int rc = build_columns<kWide>(ctx, n_cols, t.rows, d_vals, d_present, s)) return rc;
  }
  t.gen = gen;
  t.valid = true;
  ++t.epoch;
  return PAS_OK;
}

}  // namespace

__global__ void scale_fill_kernel(int64_t* tab, int32_t M) {
  const int32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < M) {
    tab[2 * m] = 1000;
    tab[2 * m + 1] = INT64_MAX / 1000;
  }
}

// Storage of a snapshot shape (pas_internal.h): shared by the build and the reshape.
int tas_alloc(pas_ctx* ctx, TasSnapshot& t, int32_t N, int32_t M, hipStream_t s) {
  const int64_t W = w64(N);
  const int32_t R = (int32_t)order_row(N);
  // vals / present hold one column even with no metric: the deschedule sweep reads column 0
  // over all N nodes for a rule whose metric is out of range (and drops what it read)
  const size_t mn = (size_t)std::max<int64_t>((int64_t)std::max(M, 1) * N, 1);
  const size_t mr = (size_t)std::max<int64_t>((int64_t)M * R, 1);
  const size_t mw = (size_t)std::max<int64_t>((int64_t)std::max(M, 1) * W, 1);
  const size_t mm = (size_t)std::max(M, 1);
  PAS_HIP(ctx, hipMalloc(&t.vals, sizeof(int64_t) * mn));
  PAS_HIP(ctx, hipMalloc(&t.present, sizeof(uint64_t) * mw));
  PAS_HIP(ctx, hipMalloc(&t.cnt, sizeof(int32_t) * mm));
  PAS_HIP(ctx, hipMalloc(&t.sorted, sizeof(int64_t) * mr));
  PAS_HIP(ctx, hipMalloc(&t.perm, sizeof(int32_t) * mr * kNumOrders));
  PAS_HIP(ctx, hipMalloc(&t.f1k, sizeof(int64_t) * (mr / 1024 + 1)));
  PAS_HIP(ctx, hipMalloc(&t.f32, sizeof(int64_t) * (mr / 32 + 1)));
  PAS_HIP(ctx, hipMalloc(&t.keys_a, sizeof(SortKey) * mr));
  PAS_HIP(ctx, hipMalloc(&t.keys_b, sizeof(SortKey) * mr));
  PAS_HIP(ctx, hipMalloc(&t.ids_a, sizeof(int32_t) * mr));
  PAS_HIP(ctx, hipMalloc(&t.ids_b, sizeof(int32_t) * mr));
  PAS_HIP(ctx, hipMalloc(&t.popc, sizeof(uint32_t) * (mw + 1)));
  PAS_HIP(ctx, hipMalloc(&t.word_scan, sizeof(uint32_t) * (mw + 1)));
  PAS_HIP(ctx, hipMalloc(&t.rows, sizeof(int32_t) * mm));
  PAS_HIP(ctx, hipMalloc(&t.scale_tab, sizeof(int64_t) * 2 * mm));
  // temp storage for the largest (whole-snapshot) sort and scan
  if (int rc = alloc_sort_tmp<false>(ctx, t, mr, M, s)) return rc;
  size_t scan_bytes = 0;
  PAS_HIP(ctx, rocprim::exclusive_scan(nullptr, scan_bytes, t.popc, t.word_scan, 0u,
                                       (size_t)(mw + 1), rocprim::plus<uint32_t>(), s));
  t.scan_tmp_bytes = std::max<size_t>(scan_bytes, 16);
  PAS_HIP(ctx, hipMalloc(&t.scan_tmp, t.scan_tmp_bytes));
  t.n_nodes = N;
  t.n_metrics = M;
  t.row = R;
  return PAS_OK;
}

int tas_alloc_wide(pas_ctx* ctx, TasSnapshot& t, hipStream_t s) {
  const size_t mn = (size_t)std::max<int64_t>((int64_t)t.n_metrics * t.n_nodes, 1);
  const size_t mr = (size_t)std::max<int64_t>((int64_t)t.n_metrics * t.row, 1);
  const size_t mm = (size_t)std::max(t.n_metrics, 1);
  PAS_HIP(ctx, hipMalloc(&t.nano, sizeof(uint32_t) * mn));
  PAS_HIP(ctx, hipMalloc(&t.sorted_nano, sizeof(uint32_t) * mr));
  PAS_HIP(ctx, hipMalloc(&t.f1k_nano, sizeof(uint32_t) * (mr / 1024 + 1)));
  PAS_HIP(ctx, hipMalloc(&t.f32_nano, sizeof(uint32_t) * (mr / 32 + 1)));
  if (int rc = alloc_sort_tmp<true>(ctx, t, mr, t.n_metrics, s)) return rc;
  PAS_HIP(ctx, hipMalloc(&t.wide_flag, mm));
  PAS_HIP(ctx, hipMemsetAsync(t.wide_flag, 0, mm, s));
  return PAS_OK;
}

int tas_snapshot_build(pas_ctx* ctx, uint64_t gen, int32_t N, int32_t M,
                       const int64_t* d_vals, const uint64_t* d_present, hipStream_t s) {
  TasSnapshot& t = ctx->tas;
  t.valid = false;
  const int64_t W = w64(N);
  const int64_t MN = (int64_t)M * N;
  const int32_t R = (int32_t)order_row(N);
  const int64_t MR = (int64_t)M * R;
  if (MR * kNumOrders > 0x7fffffffLL)
    return set_error(ctx, PAS_ECAPACITY,
                     "TAS snapshot: 3 * n_metrics * padded n_nodes must be < 2^31");
  if (t.n_nodes != N || t.n_metrics != M || !t.cnt) {
    PAS_HIP(ctx, hipStreamSynchronize(s));
    free_tas(ctx);
    if (int rc = tas_alloc(ctx, t, N, M, s)) return rc;
  }
  t.scale_host.assign(2 * (size_t)M, 0);
  for (int32_t m = 0; m < M; ++m) {
    t.scale_host[2 * (size_t)m] = 1000;
    t.scale_host[2 * (size_t)m + 1] = INT64_MAX / 1000;
  }
  // every column narrow again
  t.wide_host.assign((size_t)M, 0);
  t.n_wide = 0;
  if (t.wide_flag) PAS_HIP(ctx, hipMemsetAsync(t.wide_flag, 0, (size_t)std::max(M, 1), s));
  if (M > 0) {
    // every column milli until pas_tas_snapshot_set_scale says otherwise
    scale_fill_kernel<<<(M + 255) / 256, 256, 0, s>>>(t.scale_tab, M);
    PAS_HIP(ctx, hipGetLastError());
    if (MN > 0 && d_vals != t.vals)
      PAS_HIP(ctx, hipMemcpyAsync(t.vals, d_vals, sizeof(int64_t) * MN,
                                  hipMemcpyDeviceToDevice, s));
    if (MN > 0 && d_present != t.present)
      PAS_HIP(ctx, hipMemcpyAsync(t.present, d_present, sizeof(uint64_t) * M * W,
                                  hipMemcpyDeviceToDevice, s));
    if (int rc = build_columns<false>(ctx, M, nullptr, t.vals, t.present, s)) return rc;
  }
  t.gen = gen;
  t.valid = true;
  ++t.epoch;
  return PAS_OK;
}

int tas_snapshot_update(pas_ctx* ctx, uint64_t gen, int32_t n_cols, const int32_t* cols,
                        const int64_t* d_vals, const uint64_t* d_present, hipStream_t s) {
  return update_columns<false>(ctx, gen, n_cols, cols, d_vals, nullptr, d_present, s);
}

int tas_snapshot_update_wide(pas_ctx* ctx, uint64_t gen, int32_t n_cols, const int32_t* cols,
                             const int64_t* d_whole, const uint32_t* d_nano,
                             const uint64_t* d_present, hipStream_t s) {
  return update_columns<true>(ctx, gen, n_cols, cols, d_whole, d_nano, d_present, s);
}

int tas_snapshot_update_mixed(pas_ctx* ctx, uint64_t gen, int32_t n_narrow,
                              const int32_t* cols_narrow, int32_t n_wide,
                              const int32_t* cols_wide, const int64_t* d_vals,
                              const uint32_t* d_nano, const uint64_t* d_present, hipStream_t s) {
  TasSnapshot& t = ctx->tas;
  const int64_t N = t.n_nodes, W = w64(N);
  if (int rc = update_columns<false>(ctx, gen, n_narrow, cols_narrow, d_vals, nullptr, d_present,
                                     s))
    return rc;
  if (n_wide == 0) return PAS_OK;
  t.valid = false;  // half of the columns: not a state anything may read
  return update_columns<true>(ctx, gen, n_wide, cols_wide, d_vals + n_narrow * N,
                              d_nano + n_narrow * N, d_present + n_narrow * W, s);
}

}  // namespace pas
