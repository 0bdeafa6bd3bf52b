// gas_annotations.hip — pod events from annotation strings, parsed and resolved on the device.
//
// Cache.handlePod gets a kind, the pod, the node's name and the pod's "gas-container-cards"
// annotation (gpu-aware-scheduling/pkg/gpuscheduler/node_resource_cache.go:493-538);
// adjustPodResources (:190-287) checks the arguments (errBadArgs, :192-196), splits the
// annotation (:241,253-256) and looks every listed card up by name in the node's usage map.
// pas_gas_apply takes that event already parsed into card ranks; here the string is the input:
//   1. annotation_count   one lane per event: the rules that need no card name (a kind, pod or
//                         node out of range; a segment count that differs from the container
//                         count; a node the snapshot does not hold; no card listed), the listed
//                         count, and the largest listed count of the events still pending,
//                         reduced per wave (one lane issues the atomic);
//   2. the call's one read-back: that count is the row length of the rank rows;
//   3. annotation_ranks   the same walk again (annotation_fixed.h): each listed name against the
//                         first n_cards[node] names of the node's row of the card-name table
//                         (gas_cards.hip), the length first, then the bytes;
//   4. gas_apply_launch   the walker of the event path, exactly as pas_gas_apply runs it; the
//                         events settled in step 1 go to it with node N, which it answers with
//                         PAS_GAS_ERR_INPUT and no change;
//   5. annotation_verdicts   writes the settled events' own status over that.
// The annotations are adjacent in one blob, so neighbouring lanes read neighbouring bytes, as
// parse_literals and names_lookup do.  No kernel uses LDS or a per-lane array: the walk's state
// is a few counters and a row's spans are read from memory per compare.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "annotation_fixed.h"
#include "csr_entry.h"
#include "pas_internal.h"

namespace pas {
namespace {

constexpr int kTpb = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTpb - 1) / kTpb); }

__device__ __forceinline__ int32_t sat32(int64_t v) {
  return v > INT32_MAX ? INT32_MAX : (int32_t)v;
}

struct CardView {
  int32_t k;
  const int64_t* beg;
  const int64_t* len;
  const char* pool;
};

// Rules 1-4 of pas_gas_apply_annotations for event e, else PAS_GAS_ANN_PENDING.  kind null:
// the resolve form, which has no kinds.  name_off non-null: node[e] is the slot the name table
// gave the event's node name (-1 without one), and an empty name is bad args.
__global__ __launch_bounds__(kTpb) void annotation_count(
    int32_t E, int32_t N, const int32_t* __restrict__ kind, const int32_t* __restrict__ pod,
    const int32_t* __restrict__ node, int64_t n_name_bytes, const int64_t* __restrict__ name_off,
    int32_t n_pods, const int32_t* __restrict__ ncont, int32_t C, int64_t n_ann_bytes,
    const int64_t* __restrict__ ann_off, const char* __restrict__ ann,
    int32_t* __restrict__ verdict, int32_t* __restrict__ n_listed,
    int32_t* __restrict__ walker_node, int32_t* max_pending) {
  const int32_t e = blockIdx.x * kTpb + threadIdx.x;
  int32_t pending = 0;  // this lane's listed count if its event is pending
  if (e < E) {
    int64_t b;
    const int64_t len = entry_span(ann_off, n_ann_bytes, e, &b);
    const AnnotationCounts cnt = annotation_counts(ann + b, len);
    const int32_t p = pod[e], n = node[e];
    int32_t v = PAS_GAS_ANN_PENDING;
    if ((kind && kind[e] != PAS_GAS_EV_ADD && kind[e] != PAS_GAS_EV_REMOVE) || p < 0 ||
        p >= n_pods) {
      v = PAS_GAS_ERR_INPUT;
    } else {
      const int32_t nc = max(0, min(ncont[p], C));
      int64_t nb;
      const bool unnamed = name_off && entry_span(name_off, n_name_bytes, e, &nb) == 0;
      if (cnt.n_segments != nc || unnamed)
        v = PAS_GAS_ERR_BAD_ARGS;
      else if (n == -1)
        v = PAS_GAS_OK;  // a node the snapshot does not hold: no usage to adjust
      else if (n < 0 || n >= N)
        v = PAS_GAS_ERR_INPUT;
      else if (cnt.n_listed == 0)
        v = PAS_GAS_OK;
    }
    verdict[e] = v;
    n_listed[e] = sat32(cnt.n_listed);
    if (walker_node) walker_node[e] = v == PAS_GAS_ANN_PENDING ? n : N;
    if (v == PAS_GAS_ANN_PENDING) pending = sat32(cnt.n_listed);
  }
  if (!max_pending) return;  // (uniform)
  for (int off = 32; off > 0; off >>= 1) pending = max(pending, __shfl_xor(pending, off, 64));
  if ((threadIdx.x & 63) == 0 && pending > *(volatile int32_t*)max_pending)
    atomicMax(max_pending, pending);
}

// The rank of the name p[0 .. n) among the first L names of a row whose spans start at beg /
// len: the lowest rank whose name has the same length and bytes, else -1.
__device__ __forceinline__ int32_t card_rank(const CardView& t, int64_t row, int32_t L,
                                             const char* __restrict__ p, int64_t n) {
  for (int32_t r = 0; r < L; ++r) {
    if (t.len[row + r] != n) continue;
    const char* q = t.pool + t.beg[row + r];
    int64_t i = 0;  // (not bytes_equal: its early return compiles to another annotation_ranks)
    while (i < n && q[i] == p[i]) ++i;
    if (i == n) return r;
  }
  return -1;
}

struct RankVisitor {
  const CardView& t;
  const char* p;
  int64_t row;
  int32_t L, C, cards_ld;
  int32_t* cpc;
  int32_t* cards;
  __device__ void name(int64_t j, int64_t, int64_t beg, int64_t len) {
    if (j < cards_ld) cards[j] = card_rank(t, row, L, p + beg, len);
  }
  __device__ void segment(int64_t c, int64_t names) {
    if (c < C) cpc[c] = sat32(names);
  }
};

// cpc [E][C] and cards [E][cards_ld] of the events: every event (only_pending == 0: the
// resolve form; the containers past the annotation's segments list 0 cards, the row past the
// listed cards holds -1) or only the pending ones (the apply forms: the walker reads no row of
// a settled event).  A node outside [0, N) has no label card: every rank is -1.
__global__ __launch_bounds__(kTpb) void annotation_ranks(
    int32_t E, int32_t N, const int32_t* __restrict__ node, const int32_t* __restrict__ verdict,
    int only_pending, const int32_t* __restrict__ n_cards, CardView t, int32_t C,
    int64_t n_ann_bytes, const int64_t* __restrict__ ann_off, const char* __restrict__ ann,
    int32_t cards_ld, int32_t* __restrict__ cpc, int32_t* __restrict__ cards) {
  const int32_t e = blockIdx.x * kTpb + threadIdx.x;
  if (e >= E || (only_pending && verdict[e] != PAS_GAS_ANN_PENDING)) return;
  int64_t b;
  const int64_t len = entry_span(ann_off, n_ann_bytes, e, &b);
  const int32_t n = node[e];
  const bool held = n >= 0 && n < N;
  const int32_t L = held ? max(0, min(n_cards[n], t.k)) : 0;
  int32_t* cpc_e = cpc + (int64_t)e * C;
  int32_t* cards_e = cards + (int64_t)e * cards_ld;
  const AnnotationCounts cnt = annotation_walk(
      ann + b, len,
      RankVisitor{t, ann + b, held ? (int64_t)n * t.k : 0, L, C, cards_ld, cpc_e, cards_e});
  if (only_pending) return;
  for (int64_t c = cnt.n_segments; c < C; ++c) cpc_e[c] = 0;
  for (int64_t j = cnt.n_listed; j < cards_ld; ++j) cards_e[j] = -1;
}

// The settled events' statuses over what the walker wrote for node N
__global__ __launch_bounds__(kTpb) void annotation_verdicts(int32_t E,
                                                            const int32_t* __restrict__ verdict,
                                                            int32_t* __restrict__ status) {
  const int32_t e = blockIdx.x * kTpb + threadIdx.x;
  if (e < E && verdict[e] != PAS_GAS_ANN_PENDING) status[e] = verdict[e];
}

CardView view_of(const GasCardNames& t) { return CardView{t.k, t.sp.beg, t.sp.len, t.sp.pool}; }

}  // namespace

int annotations_resolve_launch(pas_ctx* ctx, int32_t n_events, const int32_t* d_kind,
                               const int32_t* d_pod, const int32_t* d_node, int64_t n_name_bytes,
                               const int64_t* d_name_off, int32_t n_pods, const int32_t* d_ncont,
                               int32_t max_containers, int64_t n_ann_bytes,
                               const int64_t* d_ann_off, const char* d_ann_bytes, int32_t cards_ld,
                               int32_t* d_verdict, int32_t* d_n_listed, int32_t* d_cpc,
                               int32_t* d_cards, hipStream_t s) {
  if (n_events == 0) return PAS_OK;
  const GasSnapshot& g = ctx->gas;
  annotation_count<<<blocks_for(n_events), kTpb, 0, s>>>(
      n_events, g.n_nodes, d_kind, d_pod, d_node, n_name_bytes, d_name_off, n_pods, d_ncont,
      max_containers, n_ann_bytes, d_ann_off, d_ann_bytes, d_verdict, d_n_listed, nullptr,
      nullptr);
  PAS_HIP(ctx, hipGetLastError());
  annotation_ranks<<<blocks_for(n_events), kTpb, 0, s>>>(
      n_events, g.n_nodes, d_node, d_verdict, 0, g.n_cards, view_of(ctx->gas_cards),
      max_containers, n_ann_bytes, d_ann_off, d_ann_bytes, cards_ld, d_cpc, d_cards);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

int gas_apply_annotations_launch(pas_ctx* ctx, int32_t n_events, const int32_t* d_kind,
                                 const int32_t* d_pod, const int32_t* d_node,
                                 int64_t n_name_bytes, const int64_t* d_name_off,
                                 const char* d_name_bytes, int32_t n_pods, int32_t max_containers,
                                 const int64_t* d_req, const uint32_t* d_mask,
                                 const int32_t* d_ncont, int64_t n_ann_bytes,
                                 const int64_t* d_ann_off, const char* d_ann_bytes,
                                 int32_t* d_status, hipStream_t s) {
  if (n_events == 0) return PAS_OK;
  const GasSnapshot& g = ctx->gas;
  const size_t E = (size_t)n_events, C = (size_t)max_containers;
  int rc = PAS_OK;
  SlotScope scope(ctx, s, 0, &rc);
  if (!scope.slot) return rc;
  const size_t ev_bytes = carve_size({sizeof(int32_t), 4 * E, 4 * E, 4 * E, 4 * E});
  char* base = static_cast<char*>(slot_buf(ctx, scope.slot, kBufAnnotEvents, ev_bytes, s, &rc));
  if (!base) return rc;
  Carve cv{base};
  int32_t* d_max = cv.take<int32_t>(1);
  int32_t* d_verdict = cv.take<int32_t>(E);
  int32_t* d_n_listed = cv.take<int32_t>(E);
  int32_t* d_walker_node = cv.take<int32_t>(E);
  int32_t* d_slot = cv.take<int32_t>(E);
  if (!d_node) {  // the nodes by name: lookup only, into the slot's buffer
    rc = names_resolve_launch(ctx, n_events, n_name_bytes, d_name_off, d_name_bytes, d_slot,
                              nullptr, nullptr, false, s);
    if (rc) return rc;
    d_node = d_slot;
  } else {
    d_name_off = nullptr;
  }
  PAS_HIP(ctx, hipMemsetAsync(d_max, 0, sizeof(int32_t), s));
  annotation_count<<<blocks_for(n_events), kTpb, 0, s>>>(
      n_events, g.n_nodes, d_kind, d_pod, d_node, n_name_bytes, d_name_off, n_pods, d_ncont,
      max_containers, n_ann_bytes, d_ann_off, d_ann_bytes, d_verdict, d_n_listed, d_walker_node,
      d_max);
  PAS_HIP(ctx, hipGetLastError());
  int32_t longest = 0;  // the call's one read-back
  PAS_HIP(ctx, hipMemcpyAsync(&longest, d_max, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  PAS_HIP(ctx, hipStreamSynchronize(s));
  const int32_t cards_ld = std::max(1, longest);
  const size_t ws_bytes = carve_size({4 * E * C, 4 * E * (size_t)cards_ld});
  char* ws = static_cast<char*>(slot_buf(ctx, scope.slot, kBufAnnot, ws_bytes, s, &rc));
  if (!ws) {
    (void)hipGetLastError();  // (a failed allocation: no later launch check may see it)
    return rc;
  }
  Carve cw{ws};
  int32_t* d_cpc = cw.take<int32_t>(E * C);
  int32_t* d_cards = cw.take<int32_t>(E * (size_t)cards_ld);
  annotation_ranks<<<blocks_for(n_events), kTpb, 0, s>>>(
      n_events, g.n_nodes, d_node, d_verdict, 1, g.n_cards, view_of(ctx->gas_cards),
      max_containers, n_ann_bytes, d_ann_off, d_ann_bytes, cards_ld, d_cpc, d_cards);
  PAS_HIP(ctx, hipGetLastError());
  // nothing has changed so far; the walker changes the usage
  rc = gas_apply_launch(ctx, n_events, d_kind, d_pod, d_walker_node, n_pods, max_containers,
                        d_req, d_mask, d_ncont, d_cpc, d_cards, cards_ld, d_status, s);
  if (rc) return rc;
  annotation_verdicts<<<blocks_for(n_events), kTpb, 0, s>>>(n_events, d_verdict, d_status);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

}  // namespace pas
