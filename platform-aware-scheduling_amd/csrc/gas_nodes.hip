// gas_nodes.hip — node events on the resident GAS snapshot, and its growth in place.
//
// The reference reads the node from the lister on every fit (runSchedulingLogic,
// gpu-aware-scheduling/pkg/gpuscheduler/scheduler.go:282-300), so a changed cards label or a
// changed allocatable is seen by the next request, and it keeps the usage beside the node
// objects in nodeStatuses[nodeName][cardName] (node_resource_cache.go:64,259-272,474-491), keyed
// by names and never deleted: a node that vanishes and returns keeps its usage, and a card that
// leaves the label is only skipped (scheduler.go:230-234).  Here a node is a row: n_cards[n],
// cap[n][Q] and used[n][K][Q] with the label cards in slots [0, n_cards[n]) in sort.Strings
// order and, behind them, parked slots that nothing reads (pas.h).  A node event rewrites the
// row: new counts, new capacities, and the usage moved to the slots the new label gives its
// cards (pas_gas_nodes_update[_device]).
//
// The grouping is the shared one (gas_group.h): NodeRuns gives a key per update (its node, or N
// for an update whose node or card count is out of range) and a stable radix sort of (key, u)
// over the bits N needs; run_owner elects one owner thread per node.  The owner folds its run's
// slot maps in call order into one map (a later update's upd_src indexes the row the earlier one
// left, so the maps compose), reads the old row once, and writes the row, n_cards[n] and
// cap[n][*] once: the whole old row is in the thread's registers (scratch for 64-card
// snapshots) before its first store, so any permutation is safe in place, and no other thread
// touches the row.  No atomics on the snapshot.  The row code is this kernel's own: fully
// unrolled and register-resident at the 8- and 16-slot tiers (no scratch), where the walker of
// gas_commit.hip indexes its row dynamically.
//
// pas_gas_snapshot_resize re-pitches [N][K][Q] -> [N'][K'][Q] into new storage with one
// bandwidth-bound kernel (zero fill, -1 for the new nodes' counts).  pas_gas_snapshot_compact
// renumbers the node slots the same way: new row j is old row src_node[j], whole (a slot is
// all a deleted node's usage is keyed by here, where the reference keys it by name), or a spare
// row for -1; the rows no entry names are gone.
#include <hip/hip_runtime.h>

#include "gas_group.h"
#include "pas_internal.h"

namespace pas {
namespace {

constexpr int kMaxRes = PAS_GAS_MAX_RES;
constexpr int kNodesTpb = 256;

// v[s] for a slot s the caller has checked, 0 <= s < K <= KMAX.  The 8- and 16-slot tiers
// select over a fully unrolled chain, so v stays in registers; 64 slots index scratch.
template <int KMAX, typename T>
__device__ __forceinline__ T pick(const T (&v)[KMAX], int32_t s) {
  if constexpr (KMAX <= 16) {
    T r = v[0];
#pragma unroll
    for (int i = 1; i < KMAX; ++i) r = s == i ? v[i] : r;
    return r;
  } else {
    return v[s];
  }
}

// One thread per sorted position reports its update's status; the owners run_owner elects
// rewrite one node each.  upd_src is read defensively: a value outside [0, K) is "zero usage".
template <int KMAX>
__global__ __launch_bounds__(kNodesTpb) void gas_nodes_kernel(
    int32_t n_upd, int32_t N, int32_t K, int32_t Q, const uint32_t* __restrict__ key,
    const int32_t* __restrict__ order, const int32_t* __restrict__ upd_n_cards,
    const int64_t* __restrict__ upd_cap, const int32_t* __restrict__ upd_src,
    int32_t* __restrict__ n_cards, int64_t* __restrict__ cap, int64_t* __restrict__ used,
    int32_t* __restrict__ status) {
  const int64_t pos = (int64_t)blockIdx.x * kNodesTpb + threadIdx.x;
  bool bad;
  const int32_t i = run_owner<kNodesTpb>(pos, n_upd, N, key, &bad);
  if (pos < n_upd) status[order[pos]] = bad ? PAS_GAS_ERR_INPUT : PAS_GAS_OK;
  if (i < 0) return;
  const uint32_t n = key[i];
  int64_t* un = used + (int64_t)n * K * Q;
  // the old row, whole, before any store
  int64_t u[KMAX][kMaxRes];
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int q = 0; q < kMaxRes; ++q) u[k][q] = (k < K && q < Q) ? un[k * Q + q] : 0;
  // m[k] = the old slot whose usage slot k holds after the run's updates so far (-1: zeros)
  int32_t m[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) m[k] = k;
  int32_t last = order[i];
  for (int32_t j = i; j < n_upd && key[j] == n; ++j) {
    last = order[j];
    const int32_t* src = upd_src + (int64_t)last * K;
    int32_t t[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int32_t s = k < K ? src[k] : -1;
      t[k] = (s >= 0 && s < K) ? pick<KMAX>(m, s) : -1;
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) m[k] = t[k];
  }
  // the run's last update decides the count and the capacities
  n_cards[n] = upd_n_cards[last];
  for (int q = 0; q < Q; ++q) cap[(int64_t)n * Q + q] = upd_cap[(int64_t)last * Q + q];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k >= K) continue;
    const int32_t s = m[k];
#pragma unroll
    for (int q = 0; q < kMaxRes; ++q) {
      if (q >= Q) continue;
      int64_t v;
      if constexpr (KMAX <= 16) {  // (pick, on column q)
        v = u[0][q];
#pragma unroll
        for (int c = 1; c < KMAX; ++c) v = s == c ? u[c][q] : v;
      } else {
        v = u[s < 0 ? 0 : s][q];
      }
      un[k * Q + q] = s >= 0 ? v : 0;
    }
  }
}

// [N][K][Q] -> [N2][K2][Q]: thread t writes element t of the new usage, and the new count and
// capacities of its index while t is inside those arrays (new nodes: -1, 0; new slots: 0).
__global__ __launch_bounds__(256) void gas_repitch_kernel(
    int32_t N, int32_t K, int32_t Q, int32_t N2, int32_t K2, const int32_t* __restrict__ n_cards,
    const int64_t* __restrict__ cap, const int64_t* __restrict__ used,
    int32_t* __restrict__ n_cards2, int64_t* __restrict__ cap2, int64_t* __restrict__ used2) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)N2 * K2 * Q) return;
  const int32_t q = (int32_t)(t % Q);
  const int32_t k = (int32_t)(t / Q % K2);
  const int32_t n = (int32_t)(t / Q / K2);
  used2[t] = (n < N && k < K) ? used[((int64_t)n * K + k) * Q + q] : 0;
  if (t < N2) n_cards2[t] = t < N ? n_cards[t] : -1;
  if (t < (int64_t)N2 * Q) cap2[t] = t < (int64_t)N * Q ? cap[t] : 0;
}

// [N][K][Q] -> [N2][K][Q] through src [N2] (an old row or -1): thread t writes element t of the
// new usage, and the new count and capacities of its index while t is inside those arrays
// (spare rows: -1, 0, 0).
__global__ __launch_bounds__(256) void gas_compact_kernel(
    int32_t K, int32_t Q, int32_t N2, const int32_t* __restrict__ src,
    const int32_t* __restrict__ n_cards, const int64_t* __restrict__ cap,
    const int64_t* __restrict__ used, int32_t* __restrict__ n_cards2, int64_t* __restrict__ cap2,
    int64_t* __restrict__ used2) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t kq = (int64_t)K * Q;
  if (t < N2 * kq) {
    const int64_t s = src[t / kq];
    used2[t] = s >= 0 ? used[s * kq + t % kq] : 0;
  }
  if (t < N2) {
    const int32_t s = src[t];
    n_cards2[t] = s >= 0 ? n_cards[s] : -1;
  }
  if (t < (int64_t)N2 * Q) {
    const int64_t s = src[t / Q];
    cap2[t] = s >= 0 ? cap[s * Q + t % Q] : 0;
  }
}

}  // namespace

int gas_nodes_update_launch(pas_ctx* ctx, int32_t n_updates, const int32_t* d_node,
                            const int32_t* d_n_cards, const int64_t* d_cap,
                            const int32_t* d_src, int32_t* d_status, hipStream_t s) {
  if (n_updates == 0) return PAS_OK;
  GasSnapshot& g = ctx->gas;
  const int32_t N = g.n_nodes, K = g.max_cards, Q = g.n_res;
  NodeRuns runs(ctx, n_updates, d_node, [=] __device__(int32_t u) {
    return d_n_cards[u] >= -1 && d_n_cards[u] <= K;
  }, s);
  if (runs.rc) return runs.rc;
  const unsigned blocks = (unsigned)(((size_t)n_updates + kNodesTpb - 1) / kNodesTpb);
  card_tier(K, [&](auto km) {
    gas_nodes_kernel<decltype(km)::value><<<blocks, kNodesTpb, 0, s>>>(
        n_updates, N, K, Q, runs.key, runs.order, d_n_cards, d_cap, d_src, g.n_cards, g.cap,
        g.used, d_status);
  });
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

int gas_repitch_launch(pas_ctx* ctx, int32_t n_nodes_new, int32_t max_cards_new,
                       int32_t* d_n_cards_new, int64_t* d_cap_new, int64_t* d_used_new,
                       hipStream_t s) {
  const GasSnapshot& g = ctx->gas;
  const int64_t total = (int64_t)n_nodes_new * max_cards_new * g.n_res;
  if (total == 0) return PAS_OK;
  gas_repitch_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(
      g.n_nodes, g.max_cards, g.n_res, n_nodes_new, max_cards_new, g.n_cards, g.cap, g.used,
      d_n_cards_new, d_cap_new, d_used_new);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

int gas_compact_launch(pas_ctx* ctx, int32_t n_nodes_new, const int32_t* d_src_node,
                       int32_t* d_n_cards_new, int64_t* d_cap_new, int64_t* d_used_new,
                       hipStream_t s) {
  const GasSnapshot& g = ctx->gas;
  const int64_t total = (int64_t)n_nodes_new * g.max_cards * g.n_res;  // (K, Q >= 1)
  if (total == 0) return PAS_OK;
  gas_compact_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(
      g.max_cards, g.n_res, n_nodes_new, d_src_node, g.n_cards, g.cap, g.used, d_n_cards_new,
      d_cap_new, d_used_new);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

}  // namespace pas
