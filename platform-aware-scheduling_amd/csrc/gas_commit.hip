// gas_commit.hip — bind-time commit of GAS card selections into the resident snapshot.
//
// GASExtender.bindNode (gpu-aware-scheduling/pkg/gpuscheduler/scheduler.go:385-445) runs
// runSchedulingLogic for the pod on the chosen node once more (:417-421), then
// Cache.adjustPodResources(add) (node_resource_cache.go:240-287) adds, per container, the
// request divided by the container's card count to each card of its annotation segment, all
// or nothing (checkPodResourceAdjustment on a copy first, :187-238).  A pod leaving the node
// runs adjustPodResources(remove): subtractRM per card (resource_map.go:55-73, 103-127: a
// negative amount or a key the card lacks is an input error; results clamp at zero).
//
// Here both patch the device-resident used[N][K][Q] in place, so the frozen snapshot stays
// consistent across binds without a re-upload.  The host sorts the operations by node
// (stable); one thread owns each node and applies that node's operations in call order, so
// operations on one node see each other exactly as the reference's serialised binds do.
// This is latency work (a few thousand operations per call at most), not a hot kernel.
//
// The event path (pas_gas_apply[_device]) is the third writer: Cache.handlePod's
// adjustPodResources(add / remove) straight from a pod's annotation (node_resource_cache.go:
// 493-538), one ordered batch of pod events.  Its grouping runs on the device: a key kernel
// gives event e the key node[e] (N for an event whose kind, node or pod is out of range), a
// stable radix sort of (key, e) over the bits N needs makes one run per node with the events
// in call order, and one thread per run walks it on the node's usage held by that thread.  Its
// large case is the cold-start rebuild: every running pod's annotation as one ADD batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>

#include "gas_bind.h"
#include "gas_runs.h"
#include "pas_internal.h"

namespace pas {
namespace {

constexpr int kTpb = 64;
constexpr int kMaxRes = kBindMaxRes;

// KMAX: the snapshot's max_cards rounded up to 8 / 16 / 64 (the per-thread copies live in
// registers for the common shapes, in scratch for 64-card snapshots).
template <int KMAX>
__global__ __launch_bounds__(kTpb) void gas_bind_kernel(int32_t n_seg, BindArgs a) {
  const int32_t sgi = blockIdx.x * kTpb + threadIdx.x;
  if (sgi >= n_seg) return;
  const int32_t K = a.K, Q = a.Q;
  const int32_t n = a.op_node[a.order[a.seg_off[sgi]]];
  const int32_t ncard = min(a.n_cards[n], K);
  int64_t* un = a.used + (int64_t)n * K * Q;
  int64_t u[KMAX][kMaxRes], cap[kMaxRes];
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) u[k][q] = un[k * Q + q];
  for (int q = 0; q < Q; ++q) cap[q] = a.cap[(int64_t)n * Q + q];
  for (int32_t i = a.seg_off[sgi]; i < a.seg_off[sgi + 1]; ++i) {
    const int32_t op = a.order[i];
    const int32_t p = a.op_pod[op];
    // the bind itself (gas_bind.h), on the register copy
    a.status[op] = bind_one<KMAX>(a, u, cap, ncard, p, a.ncont[p], op) ? PAS_GAS_OK
                                                                      : PAS_GAS_WONT_FIT;
  }
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) un[k * Q + q] = u[k][q];
}

template <int KMAX>
__global__ __launch_bounds__(kTpb) void gas_release_kernel(int32_t n_seg, BindArgs a) {
  const int32_t sgi = blockIdx.x * kTpb + threadIdx.x;
  if (sgi >= n_seg) return;
  const int32_t K = a.K, Q = a.Q;
  const int32_t n = a.op_node[a.order[a.seg_off[sgi]]];
  const int32_t ncard = max(0, min(a.n_cards[n], K));
  int64_t* un = a.used + (int64_t)n * K * Q;
  int64_t u[KMAX][kMaxRes];
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) u[k][q] = un[k * Q + q];
  for (int32_t i = a.seg_off[sgi]; i < a.seg_off[sgi + 1]; ++i) {
    const int32_t op = a.order[i];
    const int32_t p = a.op_pod[op];
    // the release itself (gas_bind.h), on the register copy
    a.status[op] = release_one<KMAX>(a, u, ncard, p, a.ncont[p], op) ? PAS_GAS_OK
                                                                      : PAS_GAS_ERR_INPUT;
  }
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) un[k * Q + q] = u[k][q];
}

// Event e's sort key: its node, or N (sorts last) when kind, node or pod is out of range.
__global__ __launch_bounds__(256) void gas_apply_key_kernel(
    int32_t n_ev, int32_t N, int32_t n_pods, const int32_t* __restrict__ kind,
    const int32_t* __restrict__ pod, const int32_t* __restrict__ node,
    uint32_t* __restrict__ key, int32_t* __restrict__ idx) {
  const int32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_ev) return;
  const int32_t k = kind[e], p = pod[e], n = node[e];
  const bool ok = (k == PAS_GAS_EV_ADD || k == PAS_GAS_EV_REMOVE) && n >= 0 && n < N && p >= 0 &&
                  p < n_pods;
  key[e] = ok ? (uint32_t)n : (uint32_t)N;
  idx[e] = e;
}

// One thread per sorted position finds the heads: a position whose key differs from the one
// before it starts a node's run (a position whose key is N reports its own event).  Runs
// average many events, so the heads are few and scattered: the workgroup compacts them (their
// order is free, every node has one owner) and its first threads walk one run each, applying
// its events in order, so the walking lanes share waves and the other waves leave at once
// (4 x the rebuild's speed against a walk from the head's own lane).  a.order =
// the sorted event indices, key = the sorted keys; a.op_pod / a.ncont / a.cpc / a.cards are
// read as the _device form's contract says (n_containers clamped, negative counts 0, a list
// past cards_ld errInput).
constexpr int kApplyTpb = 1024;
template <int KMAX>
__global__ __launch_bounds__(kApplyTpb) void gas_apply_kernel(int32_t n_ev, int32_t N,
                                                              const uint32_t* __restrict__ key,
                                                              const int32_t* __restrict__ kind,
                                                              BindArgs a) {
  __shared__ int32_t heads[kApplyTpb];
  __shared__ int32_t n_heads;
  if (threadIdx.x == 0) n_heads = 0;
  __syncthreads();
  const int64_t pos = (int64_t)blockIdx.x * kApplyTpb + threadIdx.x;
  if (pos < n_ev) {
    const uint32_t kp = key[pos];
    if (kp >= (uint32_t)N)  // an event out of range
      a.status[a.order[pos]] = PAS_GAS_ERR_INPUT;
    else if (pos == 0 || key[pos - 1] != kp)
      heads[atomicAdd(&n_heads, 1)] = (int32_t)pos;
  }
  __syncthreads();
  if ((int32_t)threadIdx.x >= n_heads) return;
  const int32_t i = heads[threadIdx.x];
  const uint32_t n = key[i];
  const int32_t K = a.K, Q = a.Q;
  const int32_t ncard = max(0, min(a.n_cards[n], K));
  int64_t* un = a.used + (int64_t)n * K * Q;
  int64_t u[KMAX][kMaxRes];
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) u[k][q] = un[k * Q + q];
  for (int32_t j = i; j < n_ev && key[j] == n; ++j) {
    const int32_t e = a.order[j];
    const int32_t p = a.op_pod[e];
    const int32_t ncont = max(0, min(a.ncont[p], a.C));
    if (kind[e] == PAS_GAS_EV_ADD)
      a.status[e] = adopt_one<KMAX>(a, u, ncard, p, ncont, e);
    else
      a.status[e] = release_one<KMAX>(a, u, ncard, p, ncont, e) ? PAS_GAS_OK
                                                                 : PAS_GAS_ERR_INPUT;
  }
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) un[k * Q + q] = u[k][q];
}

}  // namespace

int gas_apply_launch(pas_ctx* ctx, int32_t n_events, const int32_t* d_kind,
                     const int32_t* d_pod, const int32_t* d_node, int32_t n_pods,
                     int32_t max_containers, const int64_t* d_req, const uint32_t* d_mask,
                     const int32_t* d_ncont, const int32_t* d_cpc, const int32_t* d_cards,
                     int32_t cards_ld, int32_t* d_status, hipStream_t s) {
  if (n_events == 0) return PAS_OK;
  GasSnapshot& g = ctx->gas;
  const size_t E = (size_t)n_events;
  const int32_t N = g.n_nodes;
  unsigned end_bit = 1;  // the bits of the largest key, N
  while ((uint64_t(1) << end_bit) <= (uint64_t)N) ++end_bit;
  size_t sort_bytes = 0;
  PAS_HIP(ctx, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr,
                                         (uint32_t*)nullptr, (int32_t*)nullptr,
                                         (int32_t*)nullptr, E, 0u, end_bit, s));
  sort_bytes = std::max<size_t>(sort_bytes, 16);
  int rc = PAS_OK;
  SlotScope scope(ctx, s, 0, &rc);
  if (!scope.slot) return rc;
  const size_t bytes = carve_size({4 * E, 4 * E, 4 * E, 4 * E, sort_bytes});
  void* buf = slot_buf(ctx, scope.slot, kBufApply, bytes, s, &rc);
  if (!buf) return rc;
  Carve cv{static_cast<char*>(buf)};
  uint32_t* d_key = cv.take<uint32_t>(E);
  uint32_t* d_key_sorted = cv.take<uint32_t>(E);
  int32_t* d_idx = cv.take<int32_t>(E);
  int32_t* d_order = cv.take<int32_t>(E);
  void* d_sort_tmp = cv.take<char>(sort_bytes);
  gas_apply_key_kernel<<<(unsigned)((E + 255) / 256), 256, 0, s>>>(n_events, N, n_pods, d_kind,
                                                                  d_pod, d_node, d_key, d_idx);
  PAS_HIP(ctx, hipGetLastError());
  PAS_HIP(ctx, rocprim::radix_sort_pairs(d_sort_tmp, sort_bytes, d_key, d_key_sorted, d_idx,
                                         d_order, E, 0u, end_bit, s));
  BindArgs a{g.max_cards, g.n_res, max_containers, -1,      d_order, nullptr, d_pod,
             d_node,      g.n_cards, g.cap,        g.used,  d_req,   d_mask,  d_ncont,
             d_cpc,       d_cards, cards_ld,       nullptr, d_status, nullptr, nullptr,
             nullptr,     nullptr};
  const unsigned blocks = (unsigned)((E + kApplyTpb - 1) / kApplyTpb);
  if (g.max_cards <= 8)
    gas_apply_kernel<8><<<blocks, kApplyTpb, 0, s>>>(n_events, N, d_key_sorted, d_kind, a);
  else if (g.max_cards <= 16)
    gas_apply_kernel<16><<<blocks, kApplyTpb, 0, s>>>(n_events, N, d_key_sorted, d_kind, a);
  else
    gas_apply_kernel<PAS_GAS_MAX_CARDS><<<blocks, kApplyTpb, 0, s>>>(n_events, N, d_key_sorted,
                                                                     d_kind, a);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

int gas_commit_launch(pas_ctx* ctx, bool release, int32_t n_seg, int32_t max_containers,
                      int32_t i915_index, const int32_t* d_order, const int32_t* d_seg_off,
                      const int32_t* d_pod, const int32_t* d_node, const int64_t* d_req,
                      const uint32_t* d_mask, const int32_t* d_ncont, const int32_t* d_cpc,
                      const int32_t* d_cards, int32_t cards_stride, uint32_t* d_res,
                      int32_t* d_status, uint8_t* d_cards_out, int32_t* d_nsel_out,
                      int64_t* d_counts_out, const int64_t* d_counts, hipStream_t s) {
  if (n_seg == 0) return PAS_OK;
  GasSnapshot& g = ctx->gas;
  BindArgs a{g.max_cards, g.n_res,  max_containers, i915_index, d_order, d_seg_off,
             d_pod,       d_node,   g.n_cards,      g.cap,      g.used,  d_req,
             d_mask,      d_ncont,  d_cpc,          d_cards,    cards_stride,
             d_res,       d_status, d_cards_out,    d_nsel_out, d_counts_out, d_counts};
  const unsigned blocks = (unsigned)((n_seg + kTpb - 1) / kTpb);
#define PAS_COMMIT(KM)                                       \
  if (release)                                               \
    gas_release_kernel<KM><<<blocks, kTpb, 0, s>>>(n_seg, a); \
  else                                                       \
    gas_bind_kernel<KM><<<blocks, kTpb, 0, s>>>(n_seg, a);
  if (g.max_cards <= 8) {
    PAS_COMMIT(8)
  } else if (g.max_cards <= 16) {
    PAS_COMMIT(16)
  } else {
    PAS_COMMIT(PAS_GAS_MAX_CARDS)
  }
#undef PAS_COMMIT
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

}  // namespace pas
