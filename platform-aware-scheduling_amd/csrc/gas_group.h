// gas_group.h — runs per node: what the writers of the resident GAS usage share.
//
// Every writer (bind, release, pod events: gas_commit.hip; node events: gas_nodes.hip) groups
// its items by node, gives each node one owner thread, and has the owner apply the node's run in
// call order on a private copy of the row, stored once.  Here is that skeleton: the sort keys
// and the stable sort (NodeRuns), the owner election inside a workgroup (run_owner), the
// dispatch on the snapshot's card tier (card_tier) and the key widths (key_bits).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <type_traits>

#include "pas_internal.h"

namespace pas {

// Bits that hold 0 .. n - 1 (at least 1).  A sort whose largest key is the out-of-range key N
// spans key_bits(N + 1).
inline unsigned key_bits(int64_t n) {
  unsigned b = 1;
  while ((int64_t(1) << b) < n) ++b;
  return b;
}

// f(std::integral_constant<int, KMAX>) with the snapshot's max_cards rounded up to 8 / 16 / 64:
// the per-thread rows live in registers for the common shapes, in scratch for 64 cards.
template <class F>
inline void card_tier(int32_t max_cards, F&& f) {
  if (max_cards <= 8)
    f(std::integral_constant<int, 8>{});
  else if (max_cards <= 16)
    f(std::integral_constant<int, 16>{});
  else
    f(std::integral_constant<int, PAS_GAS_MAX_CARDS>{});
}

// Item i's sort key: its node, or N (sorts last) when the node is out of range or valid(i)
// does not hold.
template <class Valid>
__global__ __launch_bounds__(256) void node_key_kernel(int32_t n_items, int32_t N,
                                                       const int32_t* __restrict__ node,
                                                       Valid valid, uint32_t* __restrict__ key,
                                                       int32_t* __restrict__ idx) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_items) return;
  const int32_t n = node[i];
  key[i] = n >= 0 && n < N && valid(i) ? (uint32_t)n : (uint32_t)N;
  idx[i] = i;
}

// The items of a batch grouped on the device: a stable radix sort of (key, i) over the bits N
// needs makes one run per node with the items in call order (and the out-of-range items last).
// key = the sorted keys, order = the item indices in that order, both in the stream's slot
// (kBufRuns), which is released (its event recorded on s) when the object leaves scope: after
// the launch that reads them.  rc != PAS_OK: nothing usable (ctx->err set).
struct NodeRuns {
  int rc = PAS_OK;
  SlotScope scope;
  const uint32_t* key = nullptr;
  const int32_t* order = nullptr;

  template <class Valid>
  NodeRuns(pas_ctx* ctx, int32_t n_items, const int32_t* d_node, Valid valid, hipStream_t s)
      : scope(ctx, s, 0, &rc) {
    if (scope.slot) rc = sort(ctx, n_items, d_node, valid, s);
  }

 private:
  template <class Valid>
  int sort(pas_ctx* ctx, int32_t n_items, const int32_t* d_node, Valid valid, hipStream_t s) {
    const size_t n = (size_t)n_items;
    const int32_t N = ctx->gas.n_nodes;
    const unsigned end_bit = key_bits((int64_t)N + 1);
    size_t sort_bytes = 0;
    PAS_HIP(ctx, rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (int32_t*)nullptr,
                                           (int32_t*)nullptr, n, 0u, end_bit, s));
    sort_bytes = std::max<size_t>(sort_bytes, 16);
    const size_t bytes = carve_size({4 * n, 4 * n, 4 * n, 4 * n, sort_bytes});
    void* buf = slot_buf(ctx, scope.slot, kBufRuns, bytes, s, &rc);
    if (!buf) return rc;
    Carve cv{static_cast<char*>(buf)};
    uint32_t* d_key = cv.take<uint32_t>(n);
    uint32_t* d_key_sorted = cv.take<uint32_t>(n);
    int32_t* d_idx = cv.take<int32_t>(n);
    int32_t* d_order = cv.take<int32_t>(n);
    void* d_sort_tmp = cv.take<char>(sort_bytes);
    node_key_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n_items, N, d_node, valid, d_key,
                                                               d_idx);
    PAS_HIP(ctx, hipGetLastError());
    PAS_HIP(ctx, rocprim::radix_sort_pairs(d_sort_tmp, sort_bytes, d_key, d_key_sorted, d_idx,
                                           d_order, n, 0u, end_bit, s));
    key = d_key_sorted;
    order = d_order;
    return PAS_OK;
  }
};

// Owner election in a workgroup of TPB sorted positions (pos = this thread's).  A position whose
// key differs from the one before it starts a node's run.  Runs average many items, so the heads
// are few and scattered: the workgroup compacts them (their order is free, every node has one
// owner) and its first threads get one head each, so the walking lanes share waves and the
// other waves leave at once (4 x the rebuild's speed against a walk from the head's own lane,
// DESIGN.md).  Returns the head position this thread owns, or -1; *bad = pos holds an
// out-of-range item (key N), which starts no run.  Every thread of the workgroup calls it.
template <int TPB>
__device__ __forceinline__ int32_t run_owner(int64_t pos, int32_t n_items, int32_t N,
                                             const uint32_t* __restrict__ key, bool* bad) {
  __shared__ int32_t heads[TPB];
  __shared__ int32_t n_heads;
  if (threadIdx.x == 0) n_heads = 0;
  __syncthreads();
  *bad = false;
  if (pos < n_items) {
    const uint32_t kp = key[pos];
    *bad = kp >= (uint32_t)N;
    if (!*bad && (pos == 0 || key[pos - 1] != kp)) heads[atomicAdd(&n_heads, 1)] = (int32_t)pos;
  }
  __syncthreads();
  return (int32_t)threadIdx.x < n_heads ? heads[threadIdx.x] : -1;
}

}  // namespace pas
