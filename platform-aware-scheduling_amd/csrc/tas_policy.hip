// tas_policy.hip — the TAS verbs by policy id over the resident policy table.
//
// The reference reads a pod's TASPolicy from its cache on every request (cache.ReadPolicy;
// controller.go:61-176 keeps the objects current), and dontschedule.Violated
// (dontschedule/strategy.go:25-44) depends only on the policy's rules and the metric cache:
// not on the pod, not on the request's node list.  So the violating set of a policy is
// computed once per snapshot change by the deschedule sweep (tas_violations_launch over the
// table's CSR, wide columns included) and kept: viol [n_policies][W64].  The verbs then are
//
//   policy_pass_kernel             pass[p] = cand[p] & ~viol[pod_policy[p]], the whole filter
//   prio_gather_kernel             the pods' prio rules out of the table (and the all-zero rule
//                                  offsets), for the unchanged tas_eval_launch, which compacts
//                                  the order rows by the pass rows given as its candidates
//   filter_requests_policy_kernel  one lane per request position tests one bit of the
//                                  request's policy row; a wave packs 64 verdicts by ballot
//
// An id outside [0, n_policies) is read as -1 (no dontschedule rules, no prio rule), and a node
// id outside [0, n_nodes) as a node the snapshot does not hold: no kernel reads outside its
// arrays, whatever the ids are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "pas_internal.h"
#include "request_batch.h"

namespace pas {
namespace {

constexpr int kPassTpb = 256;

struct PassArgs {
  int32_t N, n_pods, n_policies, W64;
  const int32_t* pod_policy;
  const uint64_t* cand;  // [n_pods][W64] or null = every node
  const uint64_t* viol;  // [n_policies][W64]
  uint64_t* pass;        // [n_pods][W64]
};

// grid (chunks of a row, pods).  kVec: cand and pass are 16-byte aligned, so word (p, w) is
// 16-byte aligned iff p * W64 + w is even: a row is an odd first word (when its start is odd),
// 16-byte pairs, and an odd last word.  The pairs of a row are contiguous across the lanes.
// The viol row's alignment differs from the pod row's in general (another row index), so it is
// read by words; the rows are shared by the pods of a policy and stay in L2.
template <bool kVec>
__global__ __launch_bounds__(kPassTpb) void policy_pass_kernel(PassArgs a) {
  const int32_t W64 = a.W64;
  for (int32_t p = blockIdx.y; p < a.n_pods; p += gridDim.y) {
    int32_t pol = a.pod_policy[p];
    if (pol < 0 || pol >= a.n_policies) pol = -1;
    const uint64_t* __restrict__ v = pol >= 0 ? a.viol + (int64_t)pol * W64 : nullptr;
    const int64_t row = (int64_t)p * W64;
    const uint64_t* __restrict__ c = a.cand ? a.cand + row : nullptr;
    uint64_t* __restrict__ out = a.pass + row;
    auto one = [&](int32_t w) {
      out[w] = word_mask(c ? c[w] : ~0ull, w, a.N) & ~(v ? v[w] : 0ull);
    };
    const int32_t t = blockIdx.x * kPassTpb + threadIdx.x, stride = gridDim.x * kPassTpb;
    if constexpr (kVec) {
      const int32_t peel = (int32_t)(row & 1);
      const int32_t n_pair = (W64 - peel) >> 1;
      for (int32_t i = t; i < n_pair; i += stride) {
        const int32_t w = peel + 2 * i;
        ulonglong2 x = c ? *reinterpret_cast<const ulonglong2*>(c + w)
                         : ulonglong2{~0ull, ~0ull};
        x.x = word_mask(x.x, w, a.N) & ~(v ? v[w] : 0ull);
        x.y = word_mask(x.y, w + 1, a.N) & ~(v ? v[w + 1] : 0ull);
        *reinterpret_cast<ulonglong2*>(out + w) = x;
      }
      if (t == 0 && peel) one(0);
      if (t == 1 && ((W64 - peel) & 1)) one(W64 - 1);
    } else {
      for (int32_t w = t; w < W64; w += stride) one(w);
    }
  }
}

// prio[p] = the table's prio of pod p's policy, {-1, 0, 0} (no rule) for id -1; off[0 .. P]
// = 0: every pod owns no rule of the evaluation that follows.
__global__ __launch_bounds__(256) void prio_gather_kernel(
    int32_t n_pods, int32_t n_policies, const int32_t* __restrict__ pod_policy,
    const pas_rule* __restrict__ table_prio, pas_rule* __restrict__ prio,
    int32_t* __restrict__ off) {
  const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n_pods) return;
  off[p] = 0;
  if (p == n_pods) return;
  const int32_t pol = pod_policy[p];
  int32_t metric = -1, op = 0;
  int64_t target = 0;
  if (pol >= 0 && pol < n_policies) {
    metric = table_prio[pol].metric;
    op = table_prio[pol].op;
    target = table_prio[pol].target;
  }
  prio[p].metric = metric;
  prio[p].op = op;
  prio[p].target = target;
}

constexpr int kFiltTpb = 256;

struct PolFiltArgs {
  int32_t N, n_policies;
  int64_t W;
  const int32_t* req_off;     // device copies of the host's
  const int32_t* req_policy;
  const int32_t* req;
  const uint64_t* viol;
  uint64_t* out;
  int64_t ld;
};

// grid (request, 256-position chunk), as filter_requests_kernel: rows start word-aligned, so
// a wave never shares a word with another request.
__global__ __launch_bounds__(kFiltTpb) void filter_requests_policy_kernel(PolFiltArgs a) {
  const int32_t r = blockIdx.x, tid = threadIdx.x;
  const int32_t off = a.req_off[r], n = a.req_off[r + 1] - off;
  int32_t pol = a.req_policy[r];
  if (pol < 0 || pol >= a.n_policies) pol = -1;
  const uint64_t* __restrict__ v = pol >= 0 ? a.viol + (int64_t)pol * a.W : nullptr;
  uint64_t* __restrict__ row = a.out + (int64_t)r * a.ld;
  const int32_t words = (int32_t)(((int64_t)n + 63) >> 6);
  for (int64_t base = (int64_t)blockIdx.y * kFiltTpb; base < (int64_t)words * 64;
       base += (int64_t)gridDim.y * kFiltTpb) {
    const int64_t j = base + tid;  // past n in the last word's tail, and past the words
    int32_t node = -1;
    if (j < n) node = a.req[off + j];
    bool viol = false;
    // an unknown node is in no violating set: it passes (dontschedule/strategy.go:25-44)
    if (v && node >= 0 && node < a.N) viol = (v[node >> 6] >> (node & 63)) & 1ull;
    const uint64_t bits = __ballot(j < n && !viol);
    if ((tid & 63) == 0 && (j >> 6) < words) row[j >> 6] = bits;  // the request's words only
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int policies_viol(pas_ctx* ctx, hipStream_t s, const uint64_t** d_viol) {
  TasPolicies& pt = ctx->policies;
  const TasSnapshot& t = ctx->tas;
  *d_viol = nullptr;
  if (pt.viol_built && pt.viol_epoch == t.epoch && pt.viol_gen == t.gen &&
      pt.viol_serial == pt.serial) {
    *d_viol = pt.viol;
    return derived_wait(ctx, pt.viol_sync, s);
  }
  pt.viol_built = false;
  const size_t need =
      sizeof(uint64_t) * std::max<size_t>((size_t)pt.n_policies * (size_t)w64(t.n_nodes), 1);
  if (need > pt.viol_bytes) {
    if (pt.viol) {  // (a snapshot or table change is ordered after its readers by the caller)
      PAS_HIP(ctx, hipDeviceSynchronize());
      PAS_HIP(ctx, hipFree(pt.viol));
      pt.viol = nullptr;
      pt.viol_bytes = 0;
    }
    PAS_HIP(ctx, hipMalloc(&pt.viol, need));
    pt.viol_bytes = need;
  }
  // the sweep skips rules on missing columns and unknown operators, and knows wide columns
  if (pt.n_policies > 0)
    if (int rc = tas_violations_launch(ctx, pt.n_policies, pt.n_rules, pt.d_rules,
                                       pt.d_rule_off, pt.viol, s))
      return rc;
  if (int rc = derived_built(ctx, pt.viol_sync, s)) return rc;
  pt.viol_built = true;
  pt.viol_epoch = t.epoch;
  pt.viol_gen = t.gen;
  pt.viol_serial = pt.serial;
  *d_viol = pt.viol;
  return PAS_OK;
}

int policy_prio_gather(pas_ctx* ctx, AuxSlot* slot, int32_t n_pods, const int32_t* d_pod_policy,
                       pas_rule** d_prio, int32_t** d_off, hipStream_t s) {
  const size_t b_prio = sizeof(pas_rule) * (size_t)n_pods;
  const size_t b_off = sizeof(int32_t) * ((size_t)n_pods + 1);
  int rc = PAS_OK;
  void* buf = slot_buf(ctx, slot, kBufPolicy, carve_size({b_prio, b_off}), s, &rc);
  if (!buf) return rc;
  Carve cv{static_cast<char*>(buf)};
  *d_prio = cv.take<pas_rule>((size_t)n_pods);
  int32_t* off = cv.take<int32_t>((size_t)n_pods + 1);
  if (d_off) *d_off = off;
  prio_gather_kernel<<<(unsigned)(n_pods / 256 + 1), 256, 0, s>>>(
      n_pods, ctx->policies.n_policies, d_pod_policy, ctx->policies.d_prio, *d_prio, off);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

int policy_eval_launch(pas_ctx* ctx, int32_t n_pods, const int32_t* d_pod_policy,
                       const uint64_t* d_cand, uint32_t flags, uint64_t* d_pass,
                       int32_t* d_order, int32_t* d_len, hipStream_t s) {
  if (n_pods == 0) return PAS_OK;
  const TasPolicies& pt = ctx->policies;
  const TasSnapshot& t = ctx->tas;
  const int32_t W64 = (int32_t)w64(t.n_nodes);
  const bool filter = flags & PAS_TAS_FILTER, order = flags & PAS_TAS_PRIORITIZE;
  int rc = PAS_OK;
  if (filter && W64 > 0) {
    const uint64_t* viol = nullptr;
    if ((rc = policies_viol(ctx, s, &viol))) return rc;
    PassArgs a{t.n_nodes, n_pods, pt.n_policies, W64, d_pod_policy, d_cand, viol, d_pass};
    const bool vec = aligned16(d_pass) && (!d_cand || aligned16(d_cand));
    // two words per lane (vector form): a row of up to 512 words is one workgroup's
    const int32_t per_block = kPassTpb * (vec ? 2 : 1);
    const dim3 grid((unsigned)std::min((W64 + per_block - 1) / per_block, 1024),
                    (unsigned)std::min(n_pods, 65535));
    if (vec) policy_pass_kernel<true><<<grid, kPassTpb, 0, s>>>(a);
    else policy_pass_kernel<false><<<grid, kPassTpb, 0, s>>>(a);
    PAS_HIP(ctx, hipGetLastError());
  }
  if (!order) return PAS_OK;
  // the pods' prio rules and P + 1 zero offsets in the stream's slot (tas_eval_launch takes
  // the same slot's aux after this scope; the buffer stays the slot's until its next user)
  pas_rule* d_prio = nullptr;
  int32_t* d_off = nullptr;
  {
    SlotScope sc(ctx, s, 0, &rc);
    if (!sc.slot) return rc;
    if ((rc = policy_prio_gather(ctx, sc.slot, n_pods, d_pod_policy, &d_prio, &d_off, s)))
      return rc;
  }
  // pas_tas_eval's candidate rule: the lists over pass when the filter ran, else over cand
  // (then the bitmaps are not consulted at all)
  return tas_eval_launch(ctx, n_pods, 0, nullptr, d_off, d_prio, filter ? d_pass : d_cand,
                         PAS_TAS_PRIORITIZE, nullptr, d_order, d_len, 0, s);
}

int filter_requests_policy_launch(pas_ctx* ctx, int32_t n_requests, const int32_t* req_off,
                                  const int32_t* req_policy, const int32_t* d_req,
                                  uint64_t* d_pass, int64_t ld_words, HostStage* stage,
                                  hipStream_t s) {
  const int32_t longest = request_longest(n_requests, req_off);
  if (longest == 0) return PAS_OK;  // no row has a word
  const TasSnapshot& t = ctx->tas;
  const uint64_t* viol = nullptr;
  int rc = policies_viol(ctx, s, &viol);
  if (rc) return rc;
  const size_t b_off = sizeof(int32_t) * ((size_t)n_requests + 1);
  const size_t b_pol = sizeof(int32_t) * (size_t)n_requests;
  SlotScope sc(ctx, s, 0, &rc);
  if (!sc.slot) return rc;
  void* buf = slot_buf(ctx, sc.slot, kBufPolicy, carve_size({b_off, b_pol}), s, &rc);
  if (!buf) return rc;
  Carve cv{static_cast<char*>(buf)};
  int32_t* d_off = cv.take<int32_t>((size_t)n_requests + 1);
  int32_t* d_pol = cv.take<int32_t>((size_t)n_requests);
  if ((rc = upload_host(ctx, d_off, req_off, b_off, false, s))) return rc;
  if ((rc = upload_host(ctx, d_pol, req_policy, b_pol, !stage, s))) return rc;
  PolFiltArgs a{t.n_nodes, ctx->policies.n_policies, w64(t.n_nodes), d_off, d_pol, d_req,
                viol,      d_pass,                   ld_words};
  filter_requests_policy_kernel<<<dim3((unsigned)n_requests, request_chunks(longest, kFiltTpb)),
                                  kFiltTpb, 0, s>>>(a);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

}  // namespace pas
