// gas_fit_requests.hip — the GAS filter of a batch of extender requests in request terms.
//
// GASExtender.filterNodes (scheduler.go:449-482) asks, per name of the request's NodeNames,
// whether runSchedulingLogic finds cards for the pod on that node's current usage.  The
// all-node fit (gas_fit.hip) answers for every node of the snapshot; a request names a few
// hundred.  Here one lane takes one (request, position): it loads the named node's n_cards /
// cap / used row into a private copy and runs the bind's fit on it (bind_one, gas_bind.h:
// the same restatement every writer of the usage runs, so a verdict here is the verdict a
// bind on the same usage gives).  The advanced copy is discarded, the verdict kept: a wave
// packs its 64 verdicts with one ballot and stores the word once.  Rows start word-aligned,
// so a wave never shares a word with another request.  Nothing resident is written.
#include <hip/hip_runtime.h>

#include "gas_bind.h"
#include "gas_group.h"
#include "pas_internal.h"
#include "request_batch.h"

namespace pas {
namespace {

constexpr int kTpb = 256;

template <int KMAX>
__global__ __launch_bounds__(kTpb) void gas_fit_requests_kernel(
    int32_t N, const int32_t* __restrict__ req_off, const int32_t* __restrict__ req_node,
    BindArgs a, uint64_t* __restrict__ out, int64_t ld) {
  const int32_t p = blockIdx.x, tid = threadIdx.x;  // request r's pod is pod r
  const int32_t off = req_off[p], n = req_off[p + 1] - off;
  const int32_t K = a.K, Q = a.Q;
  const int32_t ncont = max(0, min(a.ncont[p], a.C));
  uint64_t* __restrict__ row = out + (int64_t)p * ld;
  const int32_t words = (int32_t)(((int64_t)n + 63) >> 6);
  for (int64_t base = (int64_t)blockIdx.y * kTpb; base < (int64_t)words * 64;
       base += (int64_t)gridDim.y * kTpb) {
    const int64_t j = base + tid;  // past n in the last word's tail, and past the words
    int32_t node = -1;
    if (j < n) node = req_node[off + j];
    bool fits = false;
    if (node >= 0 && node < N) {  // else: the FetchNode error of a node the cache lacks
      const int32_t ncard = max(0, min(a.n_cards[node], K));
      const int64_t* __restrict__ un = a.used + (int64_t)node * K * Q;
      int64_t u[KMAX][kBindMaxRes];
      for (int k = 0; k < K; ++k)
        for (int q = 0; q < Q; ++q) u[k][q] = un[k * Q + q];
      int64_t cap[kBindMaxRes];
      for (int q = 0; q < Q; ++q) cap[q] = a.cap[(int64_t)node * Q + q];
      uint32_t word;  // bind_one's result word: this lane's, not kept
      BindArgs b = a;
      b.res_out = &word;
      fits = bind_one<KMAX>(b, u, cap, ncard, p, ncont, 0);
    }
    const uint64_t bits = __ballot(fits);
    if ((tid & 63) == 0 && (j >> 6) < words) row[j >> 6] = bits;  // the request's words only
  }
}

}  // namespace

int gas_fit_requests_launch(pas_ctx* ctx, int32_t n_requests, const int32_t* req_off,
                            const int32_t* d_req_node, int32_t i915_index, const PodBatch& pods,
                            uint64_t* d_fit, int64_t ld_words, HostStage* stage, hipStream_t s) {
  const int32_t longest = request_longest(n_requests, req_off);
  if (longest == 0) return PAS_OK;  // no row has a word
  const GasSnapshot& g = ctx->gas;
  int rc = PAS_OK;
  const size_t b_off = sizeof(int32_t) * ((size_t)n_requests + 1);
  SlotScope sc(ctx, s, carve_size({b_off}), &rc);
  if (!sc.slot) return rc;
  int32_t* d_off = static_cast<int32_t*>(sc.slot->p);
  if ((rc = upload_host(ctx, d_off, req_off, b_off, !stage, s))) return rc;
  BindArgs a{};
  a.K = g.max_cards, a.Q = g.n_res, a.C = pods.max_containers, a.i915 = i915_index;
  a.n_cards = g.n_cards, a.cap = g.cap, a.used = g.used;
  a.req = pods.req, a.mask = pods.mask, a.ncont = pods.n_containers;
  const dim3 grid((unsigned)n_requests, request_chunks(longest, kTpb));
  card_tier(g.max_cards, [&](auto km) {
    gas_fit_requests_kernel<decltype(km)::value><<<grid, kTpb, 0, s>>>(g.n_nodes, d_off,
                                                                      d_req_node, a, d_fit,
                                                                      ld_words);
  });
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

}  // namespace pas
