// gas_bind.h — one GASExtender.bindNode on a node's usage held by the calling thread.
//
// The single restatement of the bind (scheduler.go:385-445): runSchedulingLogic on the
// node's current usage, then adjustPodResources(add) with the resulting annotation.  Both
// the pair-list commit (gas_commit.hip) and the batch placement (gas_place.hip) call it, so
// an operation gives the same word, selections and usage whichever call carries it.
// release_one and adopt_one are the reference's adjustPodResources(remove / add) from an
// annotation, shared the same way by the walker kernel's release and event forms
// (gas_commit.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gas_runs.h"
#include "pas.h"

namespace pas {

constexpr int kBindMaxRes = PAS_GAS_MAX_RES;

// checkResourceCapacity (scheduler.go:341-383) for one requested kind.
__device__ __forceinline__ bool kind_fits(int64_t need, int64_t cap, int64_t used) {
  if (need < 0 || cap <= 0 || used < 0) return false;
  const int64_t sum = (int64_t)((uint64_t)used + (uint64_t)need);
  return sum >= 0 && cap >= sum;
}

struct BindArgs {
  int32_t K, Q, C, i915;
  const int32_t* order;    // operation indices sorted by node (stable)
  const int32_t* op_pod;
  const int32_t* n_cards;
  const int64_t* cap;
  int64_t* used;
  const int64_t* req;      // [n_pods][C][Q]
  const uint32_t* mask;    // [n_pods][C]
  const int32_t* ncont;    // [n_pods]
  const int32_t* cpc;      // release / apply: [n_ops][C] cards per container
  const int32_t* cards;    // release / apply: [n_ops][cards_stride]
  int32_t cards_stride;    // 8 (pas_gas_release), PAS_GAS_MAX_SELECTIONS (_ex), cards_ld (apply)
  uint32_t* res_out;       // bind: [n_ops]
  int32_t* status;         // [n_ops]
  uint8_t* cards_out;      // bind_ex: [n_ops][PAS_GAS_MAX_SELECTIONS] or null
  int32_t* nsel_out;       // bind_ex: [n_ops] or null
  int64_t* counts_out;     // bind_counts: [n_ops][C][K] or null
  const int64_t* counts;   // release_counts: [n_ops][C][K] (else cpc / cards)
};

// Pod p (ncont containers) onto the node whose usage is u (cap its per-GPU capacities, ncard
// its cards): true and u advanced when it fits, false and u untouched otherwise.  The word,
// selections and counts of the operation go to row `op` of res_out / cards_out / nsel_out /
// counts_out (zeros when it does not fit); the caller records the status.
// KMAX: the snapshot's max_cards rounded up to 8 / 16 / 64 (the per-thread copies live in
// registers for the common shapes, in scratch for 64-card snapshots).
template <int KMAX>
__device__ __forceinline__ bool bind_one(const BindArgs& a, int64_t (&u)[KMAX][kBindMaxRes],
                                         const int64_t* cap, int32_t ncard, int32_t p,
                                         int32_t ncont, int64_t op) {
  const int32_t K = a.K, Q = a.Q, C = a.C;
  // runSchedulingLogic on the node's current usage: a working copy (readNodeResources,
  // node_resource_cache.go:474-491), first fit per selection, takes accumulate (addRM)
  int64_t w[KMAX][kBindMaxRes];
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) w[k][q] = u[k][q];
  bool fits = ncard > 0;  // FetchNode error / no cards label (:282-298)
  uint32_t word = 0;
  int64_t nsel = 0;
  bool packable = true;
  uint8_t* sel_out = a.cards_out ? a.cards_out + op * PAS_GAS_MAX_SELECTIONS : nullptr;
  if (sel_out)
    for (int j = 0; j < PAS_GAS_MAX_SELECTIONS; ++j) sel_out[j] = 0;
  int64_t* cnt = a.counts_out ? a.counts_out + op * C * K : nullptr;
  if (cnt)
    for (int64_t j = 0; j < (int64_t)C * K; ++j) cnt[j] = 0;
  for (int32_t c = 0; fits && c < ncont; ++c) {
    const int64_t b = (int64_t)p * C + c;
    const uint32_t m = a.mask[b];
    if (m == 0u) continue;  // no GPU resources: no cards (:206-208)
    int64_t r[kBindMaxRes];
    for (int q = 0; q < Q; ++q) r[q] = a.req[b * Q + q];
    int64_t num = 0;  // getNumI915 (:192-198)
    if (a.i915 >= 0 && ((m >> a.i915) & 1u) && r[a.i915] > 0) num = r[a.i915];
    if (num > 1)
      for (int q = 0; q < Q; ++q) r[q] /= num;  // getPerGPUResourceRequest (:180-190)
    if (num > kRunsFrom) {  // more than PAS_GAS_MAX_SELECTIONS: card runs (gas_runs.h)
      fits = container_runs<KMAX>(Q, m, r, num, cap, w, ncard, [&](int k, int64_t t) {
        if (cnt) cnt[(int64_t)c * K + k] += t;
      });
      nsel += num;
      packable = false;
      continue;
    }
    for (int64_t g = 0; g < num; ++g) {
      int chosen = -1;
      for (int k = 0; k < ncard && chosen < 0; ++k) {
        bool ok = !(m & PAS_REQ_UNKNOWN_KIND);  // a key no capacity map has (:349-354)
        for (int q = 0; q < Q; ++q)
          if ((m >> q) & 1u) ok = ok && kind_fits(r[q], cap[q], w[k][q]);
        if (ok) chosen = k;
      }
      if (chosen < 0) {  // errWontFit (:249-253)
        fits = false;
        break;
      }
      for (int q = 0; q < Q; ++q)
        if ((m >> q) & 1u) w[chosen][q] += r[q];  // addRM after a passing check
      if (nsel < PAS_GAS_PACKED) word |= (uint32_t)chosen << (3 * nsel);
      packable = packable && chosen < PAS_GAS_PACKED;
      if (sel_out && nsel < PAS_GAS_MAX_SELECTIONS) sel_out[nsel] = (uint8_t)chosen;
      if (cnt) cnt[(int64_t)c * K + chosen] += 1;
      ++nsel;
    }
  }
  if (!fits) {
    a.res_out[op] = 0u;
    if (a.nsel_out) a.nsel_out[op] = 0;
    if (sel_out)  // the selections of a bind that did not fit are not reported
      for (int j = 0; j < PAS_GAS_MAX_SELECTIONS; ++j) sel_out[j] = 0;
    if (cnt)
      for (int64_t j = 0; j < (int64_t)C * K; ++j) cnt[j] = 0;
    return false;
  }
  // the pas_gas_fit word: selections that do not pack are PAS_GAS_SEL_EXTENDED, more than
  // PAS_GAS_MAX_SELECTIONS PAS_GAS_SEL_LIMIT (cards_out zero, n_sel -1: counts_out has them)
  const bool wide = nsel > PAS_GAS_MAX_SELECTIONS;
  a.res_out[op] = nsel <= PAS_GAS_PACKED && packable
                      ? 0x80000000u | ((uint32_t)nsel << 24) | word
                      : 0x80000000u | ((uint32_t)(wide ? PAS_GAS_SEL_LIMIT
                                                       : PAS_GAS_SEL_EXTENDED) << 24);
  if (a.nsel_out) a.nsel_out[op] = wide ? -1 : (int32_t)nsel;
  if (sel_out && wide)
    for (int j = 0; j < PAS_GAS_MAX_SELECTIONS; ++j) sel_out[j] = 0;
  // adjustPodResources(add) with that annotation adds request / numCards (= numI915) to
  // each selected card: exactly the working copy's takes, which cannot overflow after the
  // capacity checks
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) u[k][q] = w[k][q];
  return true;
}

// adjustPodResources(remove) (node_resource_cache.go:236-287, subtractRM resource_map.go:
// 55-73,103-127) of operation `op` (pod p, ncont containers) on the node's usage u: true and u
// advanced, false (errInput) and u untouched.  The annotation is a.counts (counts per
// container and card) or a.cpc / a.cards; a card list that would run past its row is errInput
// (the host entry points reject it before the launch).
template <int KMAX>
__device__ __forceinline__ bool release_one(const BindArgs& a, int64_t (&u)[KMAX][kBindMaxRes],
                                            int32_t ncard, int32_t p, int32_t ncont,
                                            int64_t op) {
  const int32_t K = a.K, Q = a.Q, C = a.C;
  int64_t w[KMAX][kBindMaxRes];  // checkPodResourceAdjustment's copy
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) w[k][q] = u[k][q];
  bool ok = true;
  int32_t off = 0;
  if (a.counts) {  // the annotation as counts per container and card (any length)
    const int64_t* cnt = a.counts + op * C * K;
    for (int32_t c = 0; ok && c < ncont; ++c) {
      int64_t kc = 0;  // numCards (the host checked that the sum does not overflow)
      for (int k = 0; k < K; ++k) kc += cnt[(int64_t)c * K + k];
      if (kc <= 0) continue;  // empty annotation segment
      const int64_t b = (int64_t)p * C + c;
      const uint32_t m = a.mask[b];
      if (m & PAS_REQ_UNKNOWN_KIND) ok = false;
      int64_t r[kBindMaxRes];
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
  for (int32_t c = 0; !a.counts && ok && c < ncont; ++c) {
    const int32_t kc = a.cpc[op * C + c];
    if (kc <= 0) continue;  // empty annotation segment
    if ((int64_t)off + kc > a.cards_stride) {  // the list would leave its row
      ok = false;
      break;
    }
    const int64_t b = (int64_t)p * C + c;
    const uint32_t m = a.mask[b];
    int64_t r[kBindMaxRes];
    for (int q = 0; q < Q; ++q) r[q] = a.req[b * Q + q] / kc;  // divide(numCards)
    // subtractRM of a key no card map has (a kind outside the snapshot) -> errInput
    if (m & PAS_REQ_UNKNOWN_KIND) ok = false;
    for (int32_t j = 0; ok && j < kc; ++j) {
      const int32_t k = a.cards[op * a.cards_stride + off + j];
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
  if (!ok) return false;
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) u[k][q] = w[k][q];
  return true;
}

// adjustPodResources(add) straight from an annotation (Cache.handlePod's podAdded /
// podUpdated, node_resource_cache.go:190-287,493-538): no fit and no capacity check, only
// addRM's checks (resource_map.go:38-53,77-98).  Container c lists a.cpc[op][c] cards, stored
// consecutively in a.cards[op][..] as ranks into the node's label cards; request / numCards
// (divide, :129-145) goes to each listed card, a card listed twice twice.  The status of the
// first failing (container, listed card) is returned and u is untouched: a negative amount is
// PAS_GAS_ERR_INPUT (reported before an overflow on the same card, where the reference follows
// Go-map order), a sum that wraps below zero PAS_GAS_ERR_OVERFLOW.  A rank outside the label
// (negative or >= ncard) counts towards numCards and is otherwise skipped: no fit reads such
// a card.  PAS_REQ_UNKNOWN_KIND is ignored (the key's amount is not in the batch).  A card
// list that would run past its row is PAS_GAS_ERR_INPUT.
template <int KMAX>
__device__ __forceinline__ int32_t adopt_one(const BindArgs& a, int64_t (&u)[KMAX][kBindMaxRes],
                                             int32_t ncard, int32_t p, int32_t ncont,
                                             int64_t op) {
  const int32_t K = a.K, Q = a.Q, C = a.C;
  int64_t w[KMAX][kBindMaxRes];  // checkPodResourceAdjustment's copy
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) w[k][q] = u[k][q];
  int32_t off = 0;
  for (int32_t c = 0; c < ncont; ++c) {
    const int32_t kc = a.cpc[op * C + c];
    if (kc <= 0) continue;  // empty annotation segment
    if ((int64_t)off + kc > a.cards_stride) return PAS_GAS_ERR_INPUT;
    const int64_t b = (int64_t)p * C + c;
    const uint32_t m = a.mask[b];
    int64_t r[kBindMaxRes];
    for (int q = 0; q < Q; ++q) {
      r[q] = a.req[b * Q + q] / kc;  // divide(numCards)
      if (((m >> q) & 1u) && r[q] < 0) return PAS_GAS_ERR_INPUT;  // add: value < 0
    }
    for (int32_t j = 0; j < kc; ++j) {
      const int32_t k = a.cards[op * a.cards_stride + off + j];
      if (k < 0 || k >= ncard) continue;  // a card the label does not list
      for (int q = 0; q < Q; ++q) {
        if (!((m >> q) & 1u)) continue;
        const int64_t v = (int64_t)((uint64_t)w[k][q] + (uint64_t)r[q]);  // Go wraps
        if (v < 0) return PAS_GAS_ERR_OVERFLOW;
        w[k][q] = v;
      }
    }
    off += kc;
  }
  for (int k = 0; k < K; ++k)
    for (int q = 0; q < Q; ++q) u[k][q] = w[k][q];
  return PAS_GAS_OK;
}

}  // namespace pas
