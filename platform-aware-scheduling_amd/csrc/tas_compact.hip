// tas_compact.hip — the resident TAS snapshot with its node slots renumbered: dead slots
// dropped, the survivors moved down, spare slots wherever the map says.
//
// Every refresh of the reference's cache replaces a metric's whole node map with the nodes the
// metrics API returned this time (autoupdating.go:62-72): a node that left the cluster is in no
// map after one sync period.  Here a node is a slot, and the reshape (tas_reshape.hip) only
// appends slots.  This is the other half: new slot j holds old slot src_node[j] (-1: nothing),
// the named slots in strictly increasing order, every slot no entry names gone.
//
// No sort runs.  A column's three order rows list node ids; taking ids out of a sorted list
// leaves it sorted, and renumbering the rest by a monotone map keeps every tie in ascending
// node index, which is the order place_asc / place_desc (tas_snapshot.hip) produce.  So the
// order rows go through a stable stream compaction and the value rows through a gather:
//   slot map   dst[old N] = new slot or -1 (filled with -1, then dst[src_node[j]] = j);
//   count      per (column, plane, 1024-position segment of the old row): entries j < cnt[m]
//              with dst[perm[j]] >= 0;
//   scan       one workgroup per (column, plane) row: exclusive scan of the row's counts in
//              place; the total is cnt'[m], taken from the ascending plane (the planes list the
//              same nodes), written with the column's scale and kind;
//   scatter    each segment re-read, its kept entries ranked by wave ballots and prefix
//              popcounts behind the segment's base and written as dst[node] to the new row;
//              the ascending plane carries sorted (and sorted_nano) along from the same
//              positions, and the entry landing on a multiple of 32 / 1024 writes the fences;
//   fill       per (column, 1024-position segment of the new row): the pads at and past cnt'
//              as place_asc leaves them (sorted INT64_MAX, sorted_nano 0xffffffff, the new
//              sentinel W64' * 64 in all three planes, fences 0), and, the positions being
//              node indices too (R' >= N' + 1024), the column's vals / nano gathered through
//              src_node and its presence words as 64-lane ballots of the gathered bits.
// No atomics: every output position is computed, so the result is reproducible.  A source slot
// is below the old n_nodes, so upload bits past it in the last presence word never become
// nodes.  All kernels: 256 threads, offsets in 64 bits, 16 bytes of LDS at most, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pas_internal.h"

namespace pas {
namespace {

constexpr int kTpb = 256;
constexpr int kWaves = kTpb / 64;

// The shape and the resident arrays of a snapshot as a kernel argument (as tas_reshape.hip's).
struct ShapePtrs {
  int32_t N, M, R;
  int64_t W;
  int64_t* vals;
  uint64_t* present;
  int32_t* cnt;
  int64_t* sorted;
  int32_t* perm;
  int64_t* f1k;
  int64_t* f32;
  int64_t* scale_tab;
  uint8_t* wide_flag;  // null: no wide storage (then every pointer below is null too)
  uint32_t* nano;
  uint32_t* sorted_nano;
  uint32_t* f1k_nano;
  uint32_t* f32_nano;
};

ShapePtrs shape_ptrs(const TasSnapshot& t) {
  return ShapePtrs{t.n_nodes, t.n_metrics, t.row, w64(t.n_nodes), t.vals, t.present, t.cnt,
                   t.sorted, t.perm, t.f1k, t.f32, t.scale_tab, t.wide_flag, t.nano,
                   t.sorted_nano, t.f1k_nano, t.f32_nano};
}

__global__ __launch_bounds__(kTpb) void slot_map_kernel(const int32_t* __restrict__ src,
                                                        int32_t n_new,
                                                        int32_t* __restrict__ dst) {
  const int64_t j = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (j >= n_new) return;
  const int32_t s = src[j];
  if (s >= 0) dst[s] = (int32_t)j;
}

// The new slots of positions j .. j + 3 of order row (m, plane) of the old snapshot, -1 for an
// entry whose slot is dropped or a position at or past cnt (j a multiple of 4, below the old
// row's end).
__device__ __forceinline__ int4 kept_slots(const ShapePtrs& o, const int32_t* __restrict__ dst,
                                           int64_t m, int32_t plane, int32_t j, int32_t cnt) {
  int4 d = make_int4(-1, -1, -1, -1);
  if (j < cnt) {
    const int4 p = *reinterpret_cast<const int4*>(o.perm + (int64_t)plane * o.M * o.R +
                                                  m * o.R + j);
    d.x = dst[p.x];
    if (j + 1 < cnt) d.y = dst[p.y];
    if (j + 2 < cnt) d.z = dst[p.z];
    if (j + 3 < cnt) d.w = dst[p.w];
  }
  return d;
}

// counts[(3 m + plane) * segs + seg], segs = the segments of an old row that can hold entries.
__global__ __launch_bounds__(kTpb) void count_kernel(const ShapePtrs o,
                                                     const int32_t* __restrict__ dst,
                                                     int32_t segs, int32_t* __restrict__ counts) {
  __shared__ int32_t wave_n[kWaves];
  const int32_t seg = blockIdx.x % segs, row = blockIdx.x / segs, t = threadIdx.x;
  const int64_t m = row / kNumOrders;
  const int4 d = kept_slots(o, dst, m, row % kNumOrders, seg * 1024 + 4 * t, o.cnt[m]);
  const int32_t n = __popcll(__ballot(d.x >= 0)) + __popcll(__ballot(d.y >= 0)) +
                    __popcll(__ballot(d.z >= 0)) + __popcll(__ballot(d.w >= 0));
  if ((t & 63) == 0) wave_n[t >> 6] = n;
  __syncthreads();
  if (t == 0) counts[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

// One workgroup per (column, plane): the row's counts become their exclusive scan.  The
// ascending plane's workgroup writes the column's state.
__global__ __launch_bounds__(kTpb) void scan_kernel(const ShapePtrs o, const ShapePtrs n,
                                                    int32_t segs, int32_t* __restrict__ counts) {
  __shared__ int32_t wave_sum[kWaves];
  const int32_t row = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  int32_t* c = counts + (int64_t)row * segs;
  int32_t carry = 0;
  for (int32_t at = 0; at < segs; at += kTpb) {
    const int32_t v = at + t < segs ? c[at + t] : 0;
    int32_t x = v;  // inclusive scan of the wave
#pragma unroll
    for (int32_t off = 1; off < 64; off <<= 1) {
      const int32_t y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    __syncthreads();  // (the previous chunk's sums have been read)
    if (lane == 63) wave_sum[w] = x;
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int32_t i = 0; i < kWaves; ++i) {
      before += i < w ? wave_sum[i] : 0;
      all += wave_sum[i];
    }
    if (at + t < segs) c[at + t] = carry + before + x - v;
    carry += all;
  }
  if (row % kNumOrders == kOrderAsc && t == 0) {
    const int64_t m = row / kNumOrders;
    n.cnt[m] = carry;
    n.scale_tab[2 * m] = o.scale_tab[2 * m];
    n.scale_tab[2 * m + 1] = o.scale_tab[2 * m + 1];
    // (a column is wide only when the old snapshot has wide storage, and then the new has)
    if (n.wide_flag) n.wide_flag[m] = o.wide_flag && o.wide_flag[m] ? 1 : 0;
  }
}

// base [(3 m + plane) * segs + seg]: the scanned counts.
__global__ __launch_bounds__(kTpb) void scatter_kernel(const ShapePtrs o, const ShapePtrs n,
                                                       const int32_t* __restrict__ dst,
                                                       int32_t segs,
                                                       const int32_t* __restrict__ base) {
  __shared__ int32_t wave_n[kWaves];
  const int32_t seg = blockIdx.x % segs, row = blockIdx.x / segs, t = threadIdx.x;
  const int32_t plane = row % kNumOrders, lane = t & 63, w = t >> 6;
  const int64_t m = row / kNumOrders;
  const int32_t cnt = o.cnt[m], j = seg * 1024 + 4 * t;
  const int4 d = kept_slots(o, dst, m, plane, j, cnt);
  const int32_t slot[4] = {d.x, d.y, d.z, d.w};
  // kept entries of the wave's lower lanes, and of the wave
  const uint64_t below = (1ull << lane) - 1ull;
  int32_t rank = 0, wave_total = 0;
#pragma unroll
  for (int32_t i = 0; i < 4; ++i) {
    const uint64_t b = __ballot(slot[i] >= 0);
    rank += __popcll(b & below);
    wave_total += __popcll(b);
  }
  if (lane == 0) wave_n[w] = wave_total;
  __syncthreads();
#pragma unroll
  for (int32_t i = 0; i < kWaves; ++i) rank += i < w ? wave_n[i] : 0;
  int32_t pos = base[blockIdx.x] + rank;

  const int64_t row_o = m * o.R, row_n = m * n.R;
  int32_t* out = n.perm + (int64_t)plane * n.M * n.R + row_n;
  if (plane != kOrderAsc) {
#pragma unroll
    for (int32_t i = 0; i < 4; ++i)
      if (slot[i] >= 0) out[pos++] = slot[i];
    return;
  }
  // the ascending plane moves the sorted values with the ids, and writes the fences
  const bool wide = o.wide_flag && o.wide_flag[m] != 0;
  int64_t v[4] = {0, 0, 0, 0};
  uint32_t f[4] = {0u, 0u, 0u, 0u};
  if (j < cnt) {  // (with its three neighbours inside the old row: cnt <= o.R - 1024)
    const longlong2 a = *reinterpret_cast<const longlong2*>(o.sorted + row_o + j);
    const longlong2 b = *reinterpret_cast<const longlong2*>(o.sorted + row_o + j + 2);
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    if (wide) {
      const uint4 g = *reinterpret_cast<const uint4*>(o.sorted_nano + row_o + j);
      f[0] = g.x, f[1] = g.y, f[2] = g.z, f[3] = g.w;
    }
  }
#pragma unroll
  for (int32_t i = 0; i < 4; ++i) {
    if (slot[i] < 0) continue;
    out[pos] = slot[i];
    n.sorted[row_n + pos] = v[i];
    if (wide) n.sorted_nano[row_n + pos] = f[i];
    if ((pos & 31) == 0) {
      n.f32[m * (n.R >> 5) + (pos >> 5)] = v[i];
      if (wide) n.f32_nano[m * (n.R >> 5) + (pos >> 5)] = f[i];
      if ((pos & 1023) == 0) {
        n.f1k[m * (n.R >> 10) + (pos >> 10)] = v[i];
        if (wide) n.f1k_nano[m * (n.R >> 10) + (pos >> 10)] = f[i];
      }
    }
    ++pos;
  }
}

// One workgroup per (column, 1024-position segment of the new row): the pads of the order
// rows, and the values and presence of nodes [1024 seg, 1024 seg + 1024).  n.cnt is the scan's.
__global__ __launch_bounds__(kTpb) void fill_kernel(const ShapePtrs o, const ShapePtrs n,
                                                    const int32_t* __restrict__ src) {
  const int32_t segs = n.R >> 10;
  const int64_t m = blockIdx.x / segs;
  const int32_t seg = blockIdx.x % segs, t = threadIdx.x;
  const int32_t cnt = n.cnt[m];
  const bool wide = o.wide_flag && o.wide_flag[m] != 0;
  const int64_t row_n = m * n.R, mr_n = (int64_t)n.M * n.R;
  const int32_t sentinel = (int32_t)(n.W * 64);

  // pads: positions j .. j + 3, whole 16-byte stores past the one that cnt' splits
  const int32_t j = seg * 1024 + 4 * t;
  if (j >= cnt) {
    const longlong2 top = make_longlong2(INT64_MAX, INT64_MAX);
    *reinterpret_cast<longlong2*>(n.sorted + row_n + j) = top;
    *reinterpret_cast<longlong2*>(n.sorted + row_n + j + 2) = top;
#pragma unroll
    for (int32_t k = 0; k < kNumOrders; ++k)
      *reinterpret_cast<int4*>(n.perm + k * mr_n + row_n + j) =
          make_int4(sentinel, sentinel, sentinel, sentinel);
    if (wide)
      *reinterpret_cast<uint4*>(n.sorted_nano + row_n + j) =
          make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
    if ((j & 31) == 0) {
      n.f32[m * (n.R >> 5) + (j >> 5)] = 0;
      if (wide) n.f32_nano[m * (n.R >> 5) + (j >> 5)] = 0u;
      if ((j & 1023) == 0) {
        n.f1k[m * (n.R >> 10) + (j >> 10)] = 0;
        if (wide) n.f1k_nano[m * (n.R >> 10) + (j >> 10)] = 0u;
      }
    }
  } else if (j + 4 > cnt) {  // (cnt' is no multiple of 4: positions cnt' .. j + 3, no fence)
    for (int32_t q = cnt; q < j + 4; ++q) {
      n.sorted[row_n + q] = INT64_MAX;
      for (int32_t k = 0; k < kNumOrders; ++k) n.perm[k * mr_n + row_n + q] = sentinel;
      if (wide) n.sorted_nano[row_n + q] = 0xffffffffu;
    }
  }

  // values and presence: a wave's 64 lanes hold the 64 nodes of one presence word
#pragma unroll
  for (int32_t i = 0; i < 4; ++i) {
    const int32_t node = seg * 1024 + i * kTpb + t;
    const int64_t s = node < n.N ? src[node] : -1;
    bool bit = false;
    if (node < n.N) {
      n.vals[m * n.N + node] = s >= 0 ? o.vals[m * o.N + s] : 0;
      if (wide) n.nano[m * n.N + node] = s >= 0 ? o.nano[m * o.N + s] : 0u;
      bit = s >= 0 && (o.present[m * o.W + (s >> 6)] >> (s & 63) & 1ull);
    }
    const uint64_t word = __ballot(bit);
    if ((t & 63) == 0 && (node >> 6) < n.W) n.present[m * n.W + (node >> 6)] = word;
  }
}

}  // namespace

int tas_snapshot_compact(pas_ctx* ctx, uint64_t gen, int32_t N, const int32_t* src_node,
                         hipStream_t s) {
  TasSnapshot& t = ctx->tas;
  const int32_t M = t.n_metrics, oN = t.n_nodes;
  const int32_t segs = (int32_t)((oN + 1023) / 1024);  // old segments that can hold entries
  // a result without a wide column has no wide storage, as after a fresh snapshot_set
  TasSnapshot nt;
  int rc = tas_alloc(ctx, nt, N, M, s);
  if (!rc && t.n_wide > 0) rc = tas_alloc_wide(ctx, nt, s);
  // the call's own scratch: the map, its inverse and the segment counts
  const size_t src_bytes = sizeof(int32_t) * (size_t)std::max(N, 1);
  const size_t dst_bytes = sizeof(int32_t) * (size_t)std::max(oN, 1);
  const size_t cnt_bytes = sizeof(int32_t) * (size_t)std::max(kNumOrders * M * segs, 1);
  void* tmp = nullptr;
  hipError_t e = hipSuccess;
  if (!rc) {
    e = hipMalloc(&tmp, carve_size({src_bytes, dst_bytes, cnt_bytes}));
    if (e != hipSuccess) rc = check_hip(ctx, e, "pas_tas_snapshot_compact");
  }
  if (rc) {  // the resident snapshot was not touched
    tas_free_storage(nt);
    return rc;
  }
  Carve cv{static_cast<char*>(tmp)};
  int32_t* d_src = cv.take<int32_t>((size_t)std::max(N, 1));
  int32_t* d_dst = cv.take<int32_t>((size_t)std::max(oN, 1));
  int32_t* d_cnt = cv.take<int32_t>((size_t)std::max(kNumOrders * M * segs, 1));
  if (M > 0) {
    const ShapePtrs o = shape_ptrs(t), n = shape_ptrs(nt);
    if (N > 0)
      e = hipMemcpyAsync(d_src, src_node, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && oN > 0) e = hipMemsetAsync(d_dst, 0xff, sizeof(int32_t) * (size_t)oN, s);
    if (e == hipSuccess && N > 0 && oN > 0) {
      slot_map_kernel<<<(unsigned)((N + kTpb - 1) / kTpb), kTpb, 0, s>>>(d_src, N, d_dst);
      e = hipGetLastError();
    }
    const unsigned rows = (unsigned)(kNumOrders * M);
    if (e == hipSuccess && segs > 0) {
      count_kernel<<<rows * (unsigned)segs, kTpb, 0, s>>>(o, d_dst, segs, d_cnt);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      scan_kernel<<<rows, kTpb, 0, s>>>(o, n, segs, d_cnt);
      e = hipGetLastError();
    }
    if (e == hipSuccess && segs > 0) {
      scatter_kernel<<<rows * (unsigned)segs, kTpb, 0, s>>>(o, n, d_dst, segs, d_cnt);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      fill_kernel<<<(unsigned)((int64_t)M * (nt.row >> 10)), kTpb, 0, s>>>(o, n, d_src);
      e = hipGetLastError();
    }
  }
  // src_node is the caller's, and the old storage is freed below: its readers (these kernels,
  // and earlier calls of the host forms on the context's stream) have finished by then
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess && s != ctx->stream) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(tmp);
  if (e != hipSuccess) {
    tas_free_storage(nt);
    t.valid = false;
    return check_hip(ctx, e, "pas_tas_snapshot_compact");
  }
  nt.scale_host = t.scale_host;
  nt.wide_host.assign((size_t)M, 0);
  if (t.n_wide > 0) {
    nt.wide_host = t.wide_host;
    nt.n_wide = t.n_wide;
  }
  // the node-major copies stay with the context: the next user finds their epoch behind and
  // rebuilds them (into new storage when either is too small for the new shape)
  nt.vals_t = t.vals_t;
  nt.pres_t = t.pres_t;
  nt.vals_t_bytes = t.vals_t_bytes;
  nt.pres_t_bytes = t.pres_t_bytes;
  nt.t_epoch = t.t_epoch;
  nt.t_sync = t.t_sync;
  nt.epoch = t.epoch + 1;
  nt.gen = gen;
  nt.valid = true;
  t.vals_t = nullptr;
  t.pres_t = nullptr;
  tas_free_storage(t);
  t = nt;
  return PAS_OK;
}

}  // namespace pas
