// tas_reshape.hip — the resident TAS snapshot gathered into storage of another shape.
//
// The reference's TAS cache changes shape all the time: a policy's rules register metric
// names (controller.go:83-87,142-146 -> WriteMetric(name, nil)), the last user's delete drops
// one (autoupdating.go:127-137), and every refresh replaces a metric's whole node map with
// the nodes the metrics API returned this time (:62-72), so a node that joined the cluster is
// a new key.  None of that changes the orders of the untouched columns: a column's ascending,
// descending and index orders list node ids that stay valid when node slots are appended,
// and a column that moves keeps its rows.  So a reshape is a copy: no sort runs, the order
// rows are gathered into the new pitch and their pads rewritten.
//
// What changes with the shape, and the kernel therefore rewrites (tas_snapshot.hip's
// compact_keys / place_asc / place_desc leave exactly this for the same content):
//   R = order_row(N)   the pitch of sorted / perm rows, of f32 (R / 32) and f1k (R / 1024), and
//                      with M the stride M * R between the three perm planes;
//   W64 * 64           the sentinel of the perm pads: after growth past a multiple of 64 the
//                      old sentinel is a real node id, so every position at and past cnt[m] of
//                      all three planes gets the new one (the extra segment included);
//   the last presence word of an old row, which may carry upload bits past the old n_nodes
//   that would now be live slots: masked with the old count; new words are zero.
// Pads of sorted are INT64_MAX (sorted_nano 0xffffffff), fences are 0 past cnt; an empty
// column is all pads.
//
// One workgroup of 256 threads per (new column, 1024-position segment of its order row).  The
// segment's positions are also node indices (R >= N + 1024), so the same workgroup copies the
// column's vals / nano of nodes [1024 c, 1024 c + 1024) and its 16 presence words.  Order rows
// are 16-byte aligned (R is a multiple of 1024): two sorted values or four perm entries per
// lane and access, consecutive lanes consecutive 16 bytes.  vals rows have pitch N and are
// not: 8 bytes per lane.  The fences come from the sorted values the lane holds anyway.
// Memory bound, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pas_internal.h"

namespace pas {
namespace {

constexpr int kTpb = 256;

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

// o: the old snapshot (read only), n: the new storage, src [n.M]: old column or -1.
__global__ __launch_bounds__(kTpb) void reshape_kernel(const ShapePtrs o, const ShapePtrs n,
                                                       const int32_t* __restrict__ src) {
  const int32_t segs = n.R >> 10;
  const int64_t m = blockIdx.x / segs;
  const int32_t seg = blockIdx.x % segs, t = threadIdx.x;
  const int64_t sc = src[m];
  const bool kept = sc >= 0;
  const int32_t cnt = kept ? o.cnt[sc] : 0;
  // (a kept column is wide only when the old snapshot has wide storage, and then the new has)
  const bool wide = kept && o.wide_flag && o.wide_flag[sc] != 0;

  if (seg == 0 && t == 0) {
    n.cnt[m] = cnt;
    n.scale_tab[2 * m] = kept ? o.scale_tab[2 * sc] : 1000;
    n.scale_tab[2 * m + 1] = kept ? o.scale_tab[2 * sc + 1] : INT64_MAX / 1000;
    if (n.wide_flag) n.wide_flag[m] = wide ? 1 : 0;
  }

  // presence words of nodes [1024 seg, 1024 seg + 1024)
  if (t < 16) {
    const int64_t w = (int64_t)seg * 16 + t;
    if (w < n.W)
      n.present[m * n.W + w] = kept && w < o.W ? word_mask(o.present[sc * o.W + w], w, o.N) : 0ull;
  }

  // values of the same nodes, 8 bytes per lane
#pragma unroll
  for (int32_t i = 0; i < 4; ++i) {
    const int32_t node = seg * 1024 + i * kTpb + t;
    if (node < n.N) {
      const bool old = kept && node < o.N;
      n.vals[m * n.N + node] = old ? o.vals[sc * o.N + node] : 0;
      if (wide) n.nano[m * n.N + node] = old ? o.nano[sc * o.N + node] : 0u;
    }
  }

  const int64_t row_n = m * n.R, row_o = sc * o.R;  // (row_o is used only for a kept column)

  // sorted: positions j, j + 1 per lane, twice; j < cnt <= o.N <= o.R - 1024 is inside the
  // old row with its neighbour.  The fences f32 / f1k are the values at j % 32 == 0 / j % 1024
  // == 0 (0 past cnt).
#pragma unroll
  for (int32_t i = 0; i < 2; ++i) {
    const int32_t j = seg * 1024 + i * 512 + 2 * t;
    longlong2 v = make_longlong2(INT64_MAX, INT64_MAX);
    if (j < cnt) {
      v = *reinterpret_cast<const longlong2*>(o.sorted + row_o + j);
      if (j + 1 >= cnt) v.y = INT64_MAX;
    }
    *reinterpret_cast<longlong2*>(n.sorted + row_n + j) = v;
    if ((j & 31) == 0) {
      const int64_t f = j < cnt ? v.x : 0;
      n.f32[m * (n.R >> 5) + (j >> 5)] = f;
      if ((j & 1023) == 0) n.f1k[m * (n.R >> 10) + (j >> 10)] = f;
    }
  }

  // perm planes (and a wide column's sorted_nano): positions j .. j + 3 per lane
  const int32_t j = seg * 1024 + 4 * t;
  const int32_t sentinel = (int32_t)(n.W * 64);
  const int64_t mr_n = (int64_t)n.M * n.R, mr_o = (int64_t)o.M * o.R;
#pragma unroll
  for (int32_t k = 0; k < kNumOrders; ++k) {
    int4 p = make_int4(sentinel, sentinel, sentinel, sentinel);
    if (j < cnt) {
      p = *reinterpret_cast<const int4*>(o.perm + k * mr_o + row_o + j);
      if (j + 1 >= cnt) p.y = sentinel;
      if (j + 2 >= cnt) p.z = sentinel;
      if (j + 3 >= cnt) p.w = sentinel;
    }
    *reinterpret_cast<int4*>(n.perm + k * mr_n + row_n + j) = p;
  }
  if (wide) {
    uint4 f = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
    if (j < cnt) {
      f = *reinterpret_cast<const uint4*>(o.sorted_nano + row_o + j);
      if (j + 1 >= cnt) f.y = 0xffffffffu;
      if (j + 2 >= cnt) f.z = 0xffffffffu;
      if (j + 3 >= cnt) f.w = 0xffffffffu;
    }
    *reinterpret_cast<uint4*>(n.sorted_nano + row_n + j) = f;
    if ((j & 31) == 0) {
      const uint32_t fn = j < cnt ? f.x : 0u;
      n.f32_nano[m * (n.R >> 5) + (j >> 5)] = fn;
      if ((j & 1023) == 0) n.f1k_nano[m * (n.R >> 10) + (j >> 10)] = fn;
    }
  }
}

}  // namespace

int tas_snapshot_reshape(pas_ctx* ctx, uint64_t gen, int32_t N, int32_t M, const int32_t* src_col,
                         hipStream_t s) {
  TasSnapshot& t = ctx->tas;
  bool carry_wide = false;
  for (int32_t m = 0; m < M; ++m)
    carry_wide |= src_col[m] >= 0 && t.n_wide > 0 && t.wide_host[(size_t)src_col[m]] != 0;
  // a result without a wide column has no wide storage, as after a fresh snapshot_set
  TasSnapshot nt;
  int rc = tas_alloc(ctx, nt, N, M, s);
  if (!rc && carry_wide) rc = tas_alloc_wide(ctx, nt, s);
  if (rc) {  // the resident snapshot was not touched
    tas_free_storage(nt);
    return rc;
  }
  hipError_t e = hipSuccess;
  if (M > 0) {
    // the column map into the new build scratch's row list (unset until the next update)
    e = hipMemcpyAsync(nt.rows, src_col, sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      reshape_kernel<<<(unsigned)((int64_t)M * (nt.row >> 10)), kTpb, 0, s>>>(
          shape_ptrs(t), shape_ptrs(nt), nt.rows);
      e = hipGetLastError();
    }
  }
  // src_col is the caller's, and the old storage is freed below: its readers (the gather, and
  // earlier calls of the host forms on the context's stream) have finished by then
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess && s != ctx->stream) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    tas_free_storage(nt);
    t.valid = false;
    return check_hip(ctx, e, "pas_tas_snapshot_reshape");
  }
  nt.scale_host.assign(2 * (size_t)M, 0);
  nt.wide_host.assign((size_t)M, 0);
  for (int32_t m = 0; m < M; ++m) {
    const int32_t sc = src_col[m];
    const size_t a = 2 * (size_t)m, b = 2 * (size_t)std::max(sc, 0);
    nt.scale_host[a] = sc >= 0 ? t.scale_host[b] : 1000;
    nt.scale_host[a + 1] = sc >= 0 ? t.scale_host[b + 1] : INT64_MAX / 1000;
    if (sc >= 0 && t.n_wide > 0 && t.wide_host[(size_t)sc]) {
      nt.wide_host[(size_t)m] = 1;
      ++nt.n_wide;
    }
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
