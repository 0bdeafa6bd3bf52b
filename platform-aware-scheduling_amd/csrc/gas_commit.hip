// gas_commit.hip — bind, release and pod events committed into the resident GAS snapshot.
//
// GASExtender.bindNode (gpu-aware-scheduling/pkg/gpuscheduler/scheduler.go:385-445) runs
// runSchedulingLogic for the pod on the chosen node once more (:417-421), then
// Cache.adjustPodResources(add) (node_resource_cache.go:240-287) adds, per container, the
// request divided by the container's card count to each card of its annotation segment, all
// or nothing (checkPodResourceAdjustment on a copy first, :187-238).  A pod leaving the node
// runs adjustPodResources(remove): subtractRM per card (resource_map.go:55-73, 103-127: a
// negative amount or a key the card lacks is an input error; results clamp at zero).  The event
// path (pas_gas_apply[_device]) is Cache.handlePod's adjustPodResources(add / remove) straight
// from a pod's annotation (node_resource_cache.go:493-538), one ordered batch of pod events.
//
// All three patch the device-resident used[N][K][Q] in place, so the frozen snapshot stays
// consistent without a re-upload, and all three run one kernel, gas_walk_kernel: the
// operations arrive sorted by node (stable: one run per node, in call order), one thread owns
// each run (run_owner, gas_group.h) and applies it on the node's usage held by that thread, so
// operations on one node see each other exactly as the reference's serialised calls do.  What
// differs is who sorts.  Bind and release are latency work (a single pair per call is the
// common case): the host sorts and uploads the sorted keys, so no key kernel and no rocprim
// launch stands before the walker.  Events group on the device (NodeRuns, gas_group.h: an
// event whose kind, node or pod is out of range gets the key N); their large case is the
// cold-start rebuild, every running pod's annotation as one ADD batch.
#include <hip/hip_runtime.h>

#include "gas_bind.h"
#include "gas_group.h"
#include "pas_internal.h"

namespace pas {
namespace {

constexpr int kMaxRes = kBindMaxRes;

enum class Op { kBind, kRelease, kEvents };

// Sorted positions per workgroup.  Events: 1 024 (against 256 and against no compaction,
// DESIGN.md): their runs are long, so a workgroup has few owners.  Bind and release: 64, one
// wave.  Their batches are a few thousand operations over as many nodes, so nearly every
// position is a head, and workgroups of 1 024 would put the whole batch on four compute units
// (measured: the 4 096-bind call a quarter slower).
template <Op OP>
constexpr int kWalkTpb = OP == Op::kEvents ? 1024 : 64;

// The owner of a run loads the node's usage, applies the run's operations in order (gas_bind.h)
// and stores the usage once.  a.order = the sorted operation indices, key = the sorted keys,
// kind = the events' kinds (kEvents only).  a.op_pod / a.ncont / a.cpc / a.cards are read as
// the events' _device form's contract says (n_containers clamped, negative counts 0, a list
// past cards_stride errInput); the host forms have validated them.
template <int KMAX, Op OP>
__global__ __launch_bounds__(kWalkTpb<OP>) void gas_walk_kernel(int32_t n_ops, int32_t N,
                                                                const uint32_t* __restrict__ key,
                                                                const int32_t* __restrict__ kind,
                                                                BindArgs a) {
  constexpr int kTpb = kWalkTpb<OP>;
  const int64_t pos = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  bool bad;
  const int32_t i = run_owner<kTpb>(pos, n_ops, N, key, &bad);
  if (bad) a.status[a.order[pos]] = PAS_GAS_ERR_INPUT;  // an event out of range
  if (i < 0) return;
  const uint32_t n = key[i];
  const int32_t K = a.K, Q = a.Q;
  const int32_t ncard = max(0, min(a.n_cards[n], K));
  int64_t* un = a.used + (int64_t)n * K * Q;
  int64_t u[KMAX][kMaxRes];
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) u[k][q] = un[k * Q + q];
  [[maybe_unused]] int64_t cap[kMaxRes];
  if constexpr (OP == Op::kBind)
    for (int q = 0; q < Q; ++q) cap[q] = a.cap[(int64_t)n * Q + q];
  for (int32_t j = i; j < n_ops && key[j] == n; ++j) {
    const int32_t op = a.order[j];
    const int32_t p = a.op_pod[op];
    const int32_t ncont = max(0, min(a.ncont[p], a.C));
    if constexpr (OP == Op::kBind)
      a.status[op] = bind_one<KMAX>(a, u, cap, ncard, p, ncont, op) ? PAS_GAS_OK
                                                                    : PAS_GAS_WONT_FIT;
    else if (OP == Op::kEvents && kind[op] == PAS_GAS_EV_ADD)
      a.status[op] = adopt_one<KMAX>(a, u, ncard, p, ncont, op);
    else
      a.status[op] = release_one<KMAX>(a, u, ncard, p, ncont, op) ? PAS_GAS_OK
                                                                  : PAS_GAS_ERR_INPUT;
  }
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) un[k * Q + q] = u[k][q];
}

// The walker over n_ops sorted positions; `a` gets the snapshot's fields here.
template <Op OP>
int walk_launch(pas_ctx* ctx, int32_t n_ops, const uint32_t* d_key, const int32_t* d_kind,
                BindArgs a, hipStream_t s) {
  const GasSnapshot& g = ctx->gas;
  a.K = g.max_cards, a.Q = g.n_res;
  a.n_cards = g.n_cards, a.cap = g.cap, a.used = g.used;
  constexpr int kTpb = kWalkTpb<OP>;
  const unsigned blocks = (unsigned)(((size_t)n_ops + kTpb - 1) / kTpb);
  card_tier(g.max_cards, [&](auto km) {
    gas_walk_kernel<decltype(km)::value, OP><<<blocks, kTpb, 0, s>>>(n_ops, g.n_nodes, d_key,
                                                                     d_kind, a);
  });
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

}  // namespace

int gas_apply_launch(pas_ctx* ctx, int32_t n_events, const int32_t* d_kind,
                     const int32_t* d_pod, const int32_t* d_node, const PodBatch& pods,
                     const int32_t* d_cpc, const int32_t* d_cards, int32_t cards_ld,
                     int32_t* d_status, hipStream_t s) {
  if (n_events == 0) return PAS_OK;
  const int32_t n_pods = pods.n_pods;
  NodeRuns runs(ctx, n_events, d_node, [=] __device__(int32_t e) {
    const int32_t k = d_kind[e], p = d_pod[e];
    return (k == PAS_GAS_EV_ADD || k == PAS_GAS_EV_REMOVE) && p >= 0 && p < n_pods;
  }, s);
  if (runs.rc) return runs.rc;
  BindArgs a{};
  a.C = pods.max_containers, a.i915 = -1;
  a.order = runs.order, a.op_pod = d_pod;
  a.req = pods.req, a.mask = pods.mask, a.ncont = pods.n_containers;
  a.cpc = d_cpc, a.cards = d_cards, a.cards_stride = cards_ld;
  a.status = d_status;
  return walk_launch<Op::kEvents>(ctx, n_events, runs.key, d_kind, a, s);
}

int gas_commit_launch(pas_ctx* ctx, bool release, int32_t n_ops, int32_t i915_index,
                      const int32_t* d_order, const uint32_t* d_key, const int32_t* d_pod,
                      const PodBatch& pods, const int32_t* d_cpc, const int32_t* d_cards,
                      int32_t cards_stride, uint32_t* d_res, int32_t* d_status,
                      uint8_t* d_cards_out, int32_t* d_nsel_out, int64_t* d_counts_out,
                      const int64_t* d_counts, hipStream_t s) {
  if (n_ops == 0) return PAS_OK;
  BindArgs a{};
  a.C = pods.max_containers, a.i915 = i915_index;
  a.order = d_order, a.op_pod = d_pod;
  a.req = pods.req, a.mask = pods.mask, a.ncont = pods.n_containers;
  a.cpc = d_cpc, a.cards = d_cards, a.cards_stride = cards_stride;
  a.res_out = d_res, a.status = d_status, a.cards_out = d_cards_out, a.nsel_out = d_nsel_out;
  a.counts_out = d_counts_out, a.counts = d_counts;
  return release ? walk_launch<Op::kRelease>(ctx, n_ops, d_key, nullptr, a, s)
                 : walk_launch<Op::kBind>(ctx, n_ops, d_key, nullptr, a, s);
}

}  // namespace pas
