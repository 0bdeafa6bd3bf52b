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
#include <hip/hip_runtime.h>

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
  const int32_t K = a.K, Q = a.Q, C = a.C;
  const int32_t n = a.op_node[a.order[a.seg_off[sgi]]];
  const int32_t ncard = max(0, min(a.n_cards[n], K));
  int64_t* un = a.used + (int64_t)n * K * Q;
  int64_t u[KMAX][kMaxRes];
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) u[k][q] = un[k * Q + q];
  for (int32_t i = a.seg_off[sgi]; i < a.seg_off[sgi + 1]; ++i) {
    const int32_t op = a.order[i];
    const int32_t p = a.op_pod[op];
    int64_t w[KMAX][kMaxRes];  // checkPodResourceAdjustment's copy
    for (int k = 0; k < K; ++k)
      for (int q = 0; q < Q; ++q) w[k][q] = u[k][q];
    bool ok = true;
    int32_t off = 0;
    if (a.counts) {  // the annotation as counts per container and card (any length)
      const int64_t* cnt = a.counts + (int64_t)op * C * K;
      for (int32_t c = 0; ok && c < a.ncont[p]; ++c) {
        int64_t kc = 0;  // numCards (the host checked that the sum does not overflow)
        for (int k = 0; k < K; ++k) kc += cnt[(int64_t)c * K + k];
        if (kc <= 0) continue;  // empty annotation segment
        const int64_t b = (int64_t)p * C + c;
        const uint32_t m = a.mask[b];
        if (m & PAS_REQ_UNKNOWN_KIND) ok = false;
        int64_t r[kMaxRes];
        for (int q = 0; q < Q; ++q) r[q] = a.req[b * Q + q] / kc;  // divide(numCards)
        for (int k = 0; ok && k < K; ++k) {
          const int64_t t = cnt[(int64_t)c * K + k];
          if (t <= 0) continue;
          for (int q = 0; q < Q; ++q) {
            if (!((m >> q) & 1u)) continue;
            if (r[q] < 0 || k >= ncard) {  // negative amount / a card the label lacks
              ok = false;
              break;
            }
            w[k][q] = subtract_times(w[k][q], r[q], t);
          }
        }
      }
    }
    for (int32_t c = 0; !a.counts && ok && c < a.ncont[p]; ++c) {
      const int32_t kc = a.cpc[(int64_t)op * C + c];
      if (kc <= 0) continue;  // empty annotation segment
      const int64_t b = (int64_t)p * C + c;
      const uint32_t m = a.mask[b];
      int64_t r[kMaxRes];
      for (int q = 0; q < Q; ++q) r[q] = a.req[b * Q + q] / kc;  // divide(numCards)
      // subtractRM of a key no card map has (a kind outside the snapshot) -> errInput
      if (m & PAS_REQ_UNKNOWN_KIND) ok = false;
      for (int32_t j = 0; ok && j < kc; ++j) {
        const int32_t k = a.cards[(int64_t)op * a.cards_stride + off + j];
        const bool known = k >= 0 && k < ncard;
        for (int q = 0; q < Q; ++q) {
          if (!((m >> q) & 1u)) continue;
          // subtract: negative amount or a key the card lacks -> errInput
          if (r[q] < 0 || !known) {
            ok = false;
            break;
          }
          const int64_t v = (int64_t)((uint64_t)w[k][q] - (uint64_t)r[q]);  // Go wraps
          w[k][q] = v < 0 ? 0 : v;  // capped to zero
        }
      }
      off += kc;
    }
    if (!ok) {
      a.status[op] = PAS_GAS_ERR_INPUT;
      continue;
    }
    for (int k = 0; k < K; ++k)
      for (int q = 0; q < Q; ++q) u[k][q] = w[k][q];
    a.status[op] = PAS_GAS_OK;
  }
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) un[k * Q + q] = u[k][q];
}

}  // namespace

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
