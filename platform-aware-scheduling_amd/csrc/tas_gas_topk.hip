// tas_gas_topk.hip — combined TAS + GAS per-pod top-k, evaluated along each pod's order.
//
// BASELINE configs[4]: per pending pod, the first k entries of the
// HostPriorityList over the nodes that pass the pod's dontschedule filter
// (dontschedule.Violated + filterNodes, telemetryscheduler.go:184-225) and fit its GPU
// request (GASExtender.filterNodes -> runSchedulingLogic, gpuscheduler/scheduler.go:280-338,
// 449-482), in prioritizeNodesForRule order (telemetryscheduler.go:128-149,
// operator.go:30-42), as merge records for the node-sharded top-k of tas_topk.hip.
//
// The composed path (pas_gas_fit_bitmap_device -> pas_tas_topk_device) evaluates every
// (pod, node): a fit bit for each of the shard's nodes and the pod's whole LDS pass bitmap,
// although only the first k passing nodes of the order are kept.  Here half a wave (32
// lanes) owns a pod and walks its order row (the snapshot's per-metric order,
// tas_snapshot.hip) 32 positions at a time: each lane evaluates its position's node directly
// — candidate bit, every dontschedule rule of the pod (EvaluateRule on the node's value),
// then the GAS first fit on the node's card usage (only for lanes still passing) — and the
// pod stops once k nodes are kept.  The result is the same list: the k first positions of
// the order whose node passes both filters.  With filter and fit rates near 1 (C5: ~0.93
// and ~0.97) a pod with k = 16 needs one round, 32 node evaluations instead of the shard's N.
//
// The node values come from node-major copies of the snapshot (vals_t [N][M], pres_t
// [N][M/64], built once per snapshot change): a lane's rules read its node's own row (the
// 16 metrics of a 128-byte line together) and one presence word, instead of one line per
// rule in the metric-major columns.  A pod's dontschedule rules are compiled once into LDS
// as value ranges (LazyRule) and read back per round as broadcast LDS reads.
//
// Records: key = order key of the node's value under the pod's operator (tas_topk.hip),
// node = global id (local + node_base); past len: key INT64_MAX, node INT32_MAX.  The kWide
// instantiations (pas_tas_gas_topk_wide_device) write the wide records (key, sub, node) of
// pas.h instead and evaluate rules and jumps on wide columns exactly.
//
// Resuming (pas_tas_gas_topk[_wide]_after_device): the pod's list continues strictly after a
// cursor record.  Ascending (key[, sub], node) is the order of the row, so the records not
// after the cursor are a prefix of the row whose length topk_start_kernel finds by binary
// search (the value's tie run, then the node id within the run); the kAfter instantiations of
// the walk begin at that position instead of 0 and are otherwise the same kernel.
//
// By policy id (pas_tas[_gas]_topk_policies*_device): the pod names a row of the resident
// policy table and the dontschedule verdict of a node is one bit of the policy's cached
// violating set (tas_policy.hip, policies_viol).  The kPolicy instantiations of the walk read
// that bit where the rules form evaluates the pod's rules: no rule LDS, no node-major copies.
// With kFit = false the same walk is the TAS-only top-k (no GAS snapshot).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gas_runs.h"
#include "pas_internal.h"
#include "tas_rank.h"

namespace pas {
namespace {

constexpr int kTpb = 256;
constexpr int kWaves = kTpb / 64;
constexpr int kRuleBatch = 8;  // rule gathers in flight per lane
constexpr int kMaxRes = PAS_GAS_MAX_RES;

struct LazyTopkParams {
  int32_t n_pods, N, M, R, W64, k, node_base;
  const pas_rule* rules;
  const int32_t* rule_off;
  int32_t n_rules;  // bounds rule_off: a pod's span is clamped into [0, n_rules]
  const pas_rule* prio;
  const uint64_t* cand;  // [P][W64] or null (every node a candidate)
  const int32_t* perm;   // [3][M][R] snapshot orders
  const int32_t* cnt;    // [M]
  const int64_t* vals;   // [M][N]
  const int64_t* vals_t;    // [N][M]
  const uint64_t* pres_t;   // [N][WM]
  int32_t WM;
  const int64_t* sorted;  // [M][R] ascending present values; fences f1k [M][R/1024], f32
  const int64_t* f1k;
  const int64_t* f32;
  const int64_t* scale_tab;  // [M][2] the columns' fixed point (target_scaled)
  // GAS snapshot (same nodes) and the pods' requests
  int32_t K, Q, C, i915;
  const int32_t* n_cards;
  const int64_t* cap;
  const int64_t* used;
  const int64_t* req;     // [P][C][Q]
  const uint32_t* mask;   // [P][C]
  const int32_t* ncont;   // [P]
  int64_t* key_out;       // [P][k]
  int32_t* node_out;      // [P][k]
  int32_t* len_out;       // [P]
  // the wide records (kWide instantiations only): sub_out [P][k]; the wide columns' nanos
  // [M][N] and flags [M], both null while the snapshot holds no wide column
  uint32_t* sub_out;
  const uint32_t* nano;
  const uint8_t* wide_flag;
  const uint32_t* sorted_nano;  // [M][R] and fences [M][R/1024], [M][R/32] (the jumps' search)
  const uint32_t* f1k_nano;
  const uint32_t* f32_nano;
  // the policy form (kPolicy instantiations only): rules / rule_off / prio are then the
  // resident table's, indexed by policy, not by pod; pod_policy [P], an id outside
  // [0, n_policies) read as -1; viol [n_policies][W64] the policies' violating sets
  const int32_t* pod_policy;
  int32_t n_policies;
  const uint64_t* viol;
};


__device__ __forceinline__ int64_t order_key(int32_t op, int64_t v) {
  return op == PAS_OP_GREATER_THAN ? ~v : op == PAS_OP_LESS_THAN ? v : 0;
}

// checkResourceCapacity for one kind (scheduler.go:341-383): need >= 0, capacity > 0,
// used >= 0, used + need without overflow and within capacity.
__device__ __forceinline__ bool kind_fits(int64_t need, int64_t cap, int64_t used) {
  if (need < 0 || cap <= 0 || used < 0) return false;
  const int64_t sum = (int64_t)((uint64_t)used + (uint64_t)need);
  return sum >= 0 && cap >= sum;
}

// runSchedulingLogic (scheduler.go:280-338) of pod p on node n, the fit verdict only: a
// working copy of the node's card usage (readNodeResources, node_resource_cache.go:474-491),
// per container getPerGPUResourceRequest (:180-190) and numI915 selections (:192-198), each
// the first card in lexicographic order passing checkResourceCapacity, whose usage then
// takes the request (addRM).  KMAX: the snapshot's cards per node fit in registers
// (fully unrolled) for KMAX <= 16; the wide case keeps the copy in scratch.  QW: the kinds
// the copy holds (the snapshot's Q for KMAX <= 8, so C5's three kinds take 8 x 3 values, not
// 8 x 4; PAS_GAS_MAX_RES otherwise).
template <int KMAX, int QW>
__device__ bool lane_fit(const LazyTopkParams& a, int32_t p, int32_t n) {
  // every load of the node at once (card count, capacities, the usage of all its card slots):
  // predicating the usage loads on the card count would wait for that load first
  const int32_t nc = a.n_cards[n];
  constexpr int kUnroll = KMAX <= 16 ? KMAX : 1;
  const int32_t Q = a.Q, K = a.K;
  int64_t cap[kMaxRes];
  int64_t w[KMAX][QW];
#pragma unroll
  for (int q = 0; q < kMaxRes; ++q) cap[q] = q < Q ? a.cap[(int64_t)n * Q + q] : 0;
  if (Q == QW && ((KMAX * QW) & 1) == 0 && ((K * Q) & 1) == 0 && K <= KMAX) {
    // the node's usage row as 16-byte loads (half the load instructions; the row starts on
    // 16 bytes: an even number of values per node)
    typedef int64_t v2i64 __attribute__((ext_vector_type(2)));
    const v2i64* row = reinterpret_cast<const v2i64*>(a.used + (int64_t)n * K * Q);
    int64_t f[KMAX * QW];
#pragma unroll
    for (int i = 0; i < KMAX * QW / 2; ++i) {
      const v2i64 x = 2 * i < K * Q ? row[i] : v2i64{0, 0};
      f[2 * i] = x.x;
      f[2 * i + 1] = x.y;
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
#pragma unroll
      for (int q = 0; q < QW; ++q) w[k][q] = f[k * QW + q];
  } else {
#pragma unroll kUnroll
    for (int k = 0; k < KMAX; ++k)
#pragma unroll
      for (int q = 0; q < QW; ++q)
        w[k][q] = (k < K && q < Q) ? a.used[((int64_t)n * K + k) * Q + q] : 0;
  }
  if (nc <= 0) return false;  // FetchNode error / no cards label (:282-298)
  const int32_t ncard = min(nc, min(K, KMAX));
#pragma unroll kUnroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int q = 0; q < QW; ++q) w[k][q] = k < ncard ? w[k][q] : 0;
  const int32_t nct = min(max(a.ncont[p], 0), a.C);  // (as gas_prep_kernel: within the rows)
  for (int32_t c = 0; c < nct; ++c) {
    const int64_t b = (int64_t)p * a.C + c;
    const uint32_t m = a.mask[b];
    if (m == 0u) continue;  // no GPU resources: no cards (:206-208)
    int64_t r[kMaxRes];
#pragma unroll
    for (int q = 0; q < kMaxRes; ++q) r[q] = q < Q ? a.req[b * Q + q] : 0;
    int64_t num = 0;  // getNumI915
    if (a.i915 >= 0 && ((m >> a.i915) & 1u) && r[a.i915] > 0) num = r[a.i915];
    if (num > 1)
#pragma unroll
      for (int q = 0; q < kMaxRes; ++q) r[q] /= num;
    if (num > kRunsFrom) {  // card runs (gas_runs.h)
      if (!container_runs<KMAX, QW>(Q, m, r, num, cap, w, ncard, [](int, int64_t) {}))
        return false;
      continue;
    }
    for (int64_t g = 0; g < num; ++g) {
      int chosen = -1;
#pragma unroll kUnroll
      for (int k = KMAX - 1; k >= 0; --k) {  // first fit = lowest k
        bool ok = k < ncard && !(m & PAS_REQ_UNKNOWN_KIND);  // (a key no capacity has)
#pragma unroll
        for (int q = 0; q < QW; ++q)
          if (q < Q && ((m >> q) & 1u)) ok = ok && kind_fits(r[q], cap[q], w[k][q]);
        chosen = ok ? k : chosen;
      }
      if (chosen < 0) return false;  // errWontFit (:249-253)
#pragma unroll kUnroll
      for (int k = 0; k < KMAX; ++k)
#pragma unroll
        for (int q = 0; q < QW; ++q)
          if (k == chosen && q < Q && ((m >> q) & 1u)) w[k][q] += r[q];
    }
  }
  return true;
}

// Positions [lb, ub) of value t (milli) in metric m's ascending column (c present values),
// found by the pod's 32 lanes in three rounds of loads, as the eval prep's range search does
// (tas_eval.hip ranges_group): the 1024-stride fences, the 32-stride fences of one block, the
// 32 values of one 32-block.  lb = values < t, ub = values <= t.  kWide with wcol (the column
// is wide): the floors come with their nanos (sorted_nano and its fences) and ub counts the
// pairs <= (t, 0), i.e. lb plus the nodes of whole == t with nano == 0; lb needs no nano.
template <bool kWide>
__device__ void half_bounds(const LazyTopkParams& a, int32_t m, int32_t c, int64_t t, int sub,
                            uint64_t half_mask, bool wcol, int32_t* lb, int32_t* ub) {
  const int64_t* sv = a.sorted + (int64_t)m * a.R;
  const int64_t* f1 = a.f1k + (int64_t)m * (a.R >> 10);
  const int64_t* f2 = a.f32 + (int64_t)m * (a.R >> 5);
  // value (v, nano f) <= t: the narrow compare when f is 0
  auto not_above = [&](int64_t v, uint32_t f) { return v < t || (v == t && f == 0u); };
  const int32_t na = (c + 1023) >> 10, nb = (c + 31) >> 5;
  int32_t cl = 0, cu = 0;
  for (int32_t i0 = 0; i0 < na; i0 += 8 * 32) {
    int64_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = f1[min(i0 + u * 32 + sub, max(na - 1, 0))];
    if constexpr (kWide) {
      uint32_t g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        g[u] = wcol ? a.f1k_nano[(int64_t)m * (a.R >> 10) + min(i0 + u * 32 + sub, max(na - 1, 0))]
                    : 0u;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool in = i0 + u * 32 + sub < na;
        cl += in && v[u] < t;
        cu += in && not_above(v[u], g[u]);
      }
      continue;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool in = i0 + u * 32 + sub < na;
      cl += in && v[u] < t;
      cu += in && v[u] <= t;
    }
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {  // (xor within the half)
    cl += __shfl_xor(cl, off, 64);
    cu += __shfl_xor(cu, off, 64);
  }
  const int32_t n1l = cl, n1u = cu;
  const int32_t b1l = max(n1l - 1, 0), b1u = max(n1u - 1, 0);
  const int32_t e2l = n1l ? min(32, nb - b1l * 32) : 0, e2u = n1u ? min(32, nb - b1u * 32) : 0;
  const int64_t x2l = f2[b1l * 32 + min(sub, max(e2l - 1, 0))];
  const int64_t x2u = f2[b1u * 32 + min(sub, max(e2u - 1, 0))];
  uint32_t g2u = 0;
  if constexpr (kWide)
    if (wcol) g2u = a.f32_nano[(int64_t)m * (a.R >> 5) + b1u * 32 + min(sub, max(e2u - 1, 0))];
  const int32_t n2l = __popcll(__ballot(sub < e2l && x2l < t) & half_mask);
  const int32_t n2u = __popcll(
      __ballot(sub < e2u && (kWide ? not_above(x2u, g2u) : x2u <= t)) & half_mask);
  const int32_t b2l = b1l * 32 + max(n2l - 1, 0), b2u = b1u * 32 + max(n2u - 1, 0);
  const int32_t e3l = n1l ? min(32, c - b2l * 32) : 0, e3u = n1u ? min(32, c - b2u * 32) : 0;
  const int64_t x3l = sv[b2l * 32 + min(sub, max(e3l - 1, 0))];
  const int64_t x3u = sv[b2u * 32 + min(sub, max(e3u - 1, 0))];
  uint32_t g3u = 0;
  if constexpr (kWide)
    if (wcol) g3u = a.sorted_nano[(int64_t)m * a.R + b2u * 32 + min(sub, max(e3u - 1, 0))];
  const int32_t n3l = __popcll(__ballot(sub < e3l && x3l < t) & half_mask);
  const int32_t n3u = __popcll(
      __ballot(sub < e3u && (kWide ? not_above(x3u, g3u) : x3u <= t)) & half_mask);
  *lb = n1l ? b2l * 32 + n3l : 0;
  *ub = n1u ? b2u * 32 + n3u : 0;
}

constexpr int kPodLanes = 32;                // lanes per pod (order positions per round)
constexpr int kPodsPerWave = 64 / kPodLanes;
constexpr int kPodsPerBlock = kWaves * kPodsPerWave;
constexpr int kStageRules = kPodLanes;       // rules of a pod compiled into LDS (one per lane)

// A dontschedule rule compiled once per pod: EvaluateRule (operator.go:13-26) on the node's
// value v (milli) as the range test  (uint64)(v - lo) <= span, with the saturating target
//  folded in: LessThan t -> [INT64_MIN, t*1000 - 1], GreaterThan t ->
// [t*1000 + 1, INT64_MAX], Equals t -> [t*1000, t*1000]; a target past the int64 milli range
// selects every value or none.  metric < 0: never evaluated (not cached, unknown operator, or
// a range that selects nothing).
struct alignas(16) LazyRule {
  int64_t lo;
  uint64_t span;
};

__device__ __forceinline__ void compile_rule(const pas_rule& ru, int32_t M,
                                             const int64_t* __restrict__ scale_tab,
                                             int32_t* metric, LazyRule* out) {
  int64_t tm = 0;
  const int sat = target_scaled(ru.target, scale_tab, (ru.metric >= 0 && ru.metric < M)
                                                          ? ru.metric : 0, &tm);
  int64_t lo = 0, hi = -1;  // empty
  if (ru.metric >= 0 && ru.metric < M) {
    if (ru.op == PAS_OP_LESS_THAN) {
      if (sat > 0) lo = INT64_MIN, hi = INT64_MAX;
      else if (sat == 0 && tm > INT64_MIN) lo = INT64_MIN, hi = tm - 1;
    } else if (ru.op == PAS_OP_GREATER_THAN) {
      if (sat < 0) lo = INT64_MIN, hi = INT64_MAX;
      else if (sat == 0 && tm < INT64_MAX) lo = tm + 1, hi = INT64_MAX;
    } else if (ru.op == PAS_OP_EQUALS) {
      if (sat == 0) lo = hi = tm;
    }
  }
  const bool live = lo <= hi;
  *metric = live ? ru.metric : -1;
  out->lo = lo;
  out->span = (uint64_t)hi - (uint64_t)lo;
}

// The same for the wide instantiations, where the rule's column may be wide (pas_internal.h
// wide_below / wide_equal / wide_above: the target as it is, no scale, no saturation).  The
// nano of a node matters only where whole == target, so the rule stays the range test on the
// floor plus a condition on the range's edge value whole == t: LessThan t -> [MIN, t - 1] (no
// edge); GreaterThan t -> [t, MAX], the edge hits only with nano != 0; Equals t -> [t, t], the
// edge hits only with nano == 0.  The nano is loaded only by a lane whose floor is the edge.
constexpr int32_t kEdgeNone = 0, kEdgeNanoNonZero = 1, kEdgeNanoZero = 2;
__device__ __forceinline__ void compile_rule_wide(const pas_rule& ru, int32_t M,
                                                  const int64_t* __restrict__ scale_tab,
                                                  const uint8_t* __restrict__ wide_flag,
                                                  int32_t* metric, LazyRule* out, int64_t* edge,
                                                  int32_t* mode) {
  *edge = 0;
  *mode = kEdgeNone;
  if (!(wide_flag && ru.metric >= 0 && ru.metric < M && wide_flag[ru.metric])) {
    compile_rule(ru, M, scale_tab, metric, out);
    return;
  }
  const int64_t t = ru.target;
  int64_t lo = 0, hi = -1;  // empty
  if (ru.op == PAS_OP_LESS_THAN) {
    if (t > INT64_MIN) lo = INT64_MIN, hi = t - 1;
  } else if (ru.op == PAS_OP_GREATER_THAN) {
    lo = t, hi = INT64_MAX;
    *mode = kEdgeNanoNonZero;
  } else if (ru.op == PAS_OP_EQUALS) {
    lo = hi = t;
    *mode = kEdgeNanoZero;
  }
  *edge = t;
  *metric = lo <= hi ? ru.metric : -1;
  out->lo = lo;
  out->span = (uint64_t)hi - (uint64_t)lo;
}

// (at least 4 waves per SIMD for the register-resident shapes: the gathers need waves in
// flight)
// The wide instantiations of those shapes need about 12 more registers at the fit's peak
// (the wide columns' pointers and the edge test stay live beside the card state) and spill
// 12 - 52 bytes per lane under the 128-register cap of 4 waves, so they ask for 3 waves (168
// registers, no scratch): the narrow instantiations keep 4.
template <int KMAX, int QW, bool kWide>
constexpr int topk_waves() { return KMAX <= 8 && QW <= 3 ? (kWide ? 3 : 4) : 1; }
// kWide: the wide records (key, sub, node) in the canonical unit (pas.h), rules and jumps on
// wide columns; the narrow instantiations (kWide = false) hold none of that code.
// kAfter: the walk begins at the pod's start position, which topk_start_kernel left in
// len_out[p] (the walk writes the list's length there at its end); nothing else differs.
// kPolicy (pas_tas[_gas]_topk_policies*_device): the pod names a row of the resident policy
// table (tas_policy.hip).  Its prio rule and rule span are the table's, and a node's
// dontschedule verdict is one bit of the policy's cached violating set, viol [n_policies][W64]:
// no rule is compiled into LDS or evaluated, vals_t / pres_t are not read.  The jumps still
// read the table's rules, through the same code.  The sweep that builds viol skips what the
// rule loops here skip (unknown operators, metrics outside the snapshot, absent values), so
// the lists are those of the rules form.
// kFit = false (kPolicy only): no GAS fit, the TAS-only top-k; KMAX / QW are then unused.
template <int KMAX, int QW, bool kWide, bool kAfter, bool kPolicy = false, bool kFit = true>
__global__ __launch_bounds__(kTpb)
__attribute__((amdgpu_waves_per_eu(topk_waves<KMAX, QW, kWide>())))
void tas_gas_topk_kernel(LazyTopkParams a) {
  static_assert(kFit || kPolicy, "the rules form always fits");
  // the pods' compiled rules, kStageRules per pod (pods of at most that many rules); none in
  // the kPolicy instantiations, which reference no LDS
  __shared__ LazyRule srule[kPolicy ? 1 : kPodsPerBlock][kPolicy ? 1 : kStageRules];
  __shared__ int32_t smetric[kPolicy ? 1 : kPodsPerBlock][kPolicy ? 1 : kStageRules];
  // (kWide) the rules' edge value and mode (compile_rule_wide)
  constexpr bool kEdgeLds = kWide && !kPolicy;
  __shared__ int64_t sedge[kEdgeLds ? kPodsPerBlock : 1][kEdgeLds ? kStageRules : 1];
  __shared__ int32_t smode[kEdgeLds ? kPodsPerBlock : 1][kEdgeLds ? kStageRules : 1];
  const int lane = threadIdx.x & 63;
  const int half = lane / kPodLanes, sub = lane % kPodLanes;
  // XCD-aware: blocks b and b + 8 share an XCD; each XCD takes a contiguous run of the
  // bucketed pod list (MI355X_MICROARCH.md)
  const int32_t nb = gridDim.x, b = blockIdx.x;
  const int32_t xcd = b & 7, per = nb >> 3, rem = nb & 7;
  const int32_t slot = xcd * per + min(xcd, rem) + (b >> 3);
  const int32_t pos = slot * kPodsPerBlock + (int32_t)(threadIdx.x >> 6) * kPodsPerWave + half;
  const uint64_t half_mask = half ? ~0ull << 32 : 0xFFFFFFFFull;
  const uint64_t below = half_mask & ((1ull << lane) - 1ull);
  const bool have = pos < a.n_pods;
  // the pod's descriptor (the eval prep's form): {pod, order row or -1, present count},
  // {first rule, end rule}; pods in index order (bucketing them by order row first, as the
  // eval prep does, was measured slower here: the one-block grouping of 64k pods costs more
  // than the L2 locality gains)
  int4 d0 = make_int4(0, -1, 0, 0), d1 = make_int4(0, 0, 0, 0);
  // (kPolicy) the pod's policy, -1 = none: no prio rule (the empty list) and no rules; at =
  // the pod's row of prio and rule_off, which is the policy's there
  int32_t pol = -1;
  if constexpr (kPolicy) {
    if (have) pol = a.pod_policy[pos];
    if (pol < 0 || pol >= a.n_policies) pol = -1;
    if (have) d0.x = pos;
  }
  const int32_t at = kPolicy ? pol : pos;
  if (kPolicy ? pol >= 0 : have) {
    const pas_rule q = a.prio[at];
    const int32_t cq = (q.metric >= 0 && q.metric < a.M) ? a.cnt[q.metric] : 0;
    const int oq = q.op == PAS_OP_GREATER_THAN ? kOrderDesc
                   : q.op == PAS_OP_LESS_THAN  ? kOrderAsc
                                               : kOrderIndex;
    d0 = make_int4(pos, cq > 0 ? oq * a.M + q.metric : -1, cq, 0);
    // (clamped into [0, n_rules] and non-decreasing: a device rule_off that is not a CSR
    // never indexes past the rules, as the eval prep's rule_span)
    const int32_t r0 = min(max(a.rule_off[at], 0), a.n_rules);
    d1 = make_int4(r0, min(max(a.rule_off[at + 1], r0), a.n_rules), 0, 0);
  }
  const int32_t p = d0.x;
  const int32_t k = a.k;
  const pas_rule pr = !kPolicy ? a.prio[p] : pol >= 0 ? a.prio[pol] : pas_rule{-1, 0, 0};
  // bucket -1: no scheduling rule / metric not cached / no node has it: empty list
  // (telemetryscheduler.go:92-96); d0.z = the metric's present count
  const int32_t c0 = (have && d0.y >= 0) ? d0.z : 0;
  const int32_t r0 = d1.x, r1 = d1.y;
  // Rules on the prioritize metric itself select one contiguous range of a sorted order row
  // (EvaluateRule over the ascending column, a3): a pod whose rule excludes the top of its
  // own order (e.g. GreaterThan on the metric it prioritizes by GreaterThan) would walk
  // thousands of violating positions.  Such ranges (asc positions from the prep's search,
  // mirrored for the descending row) are jumped over at the start of each round; the rule
  // check per node still runs, so the skip only saves rounds.
  constexpr int kSkip = 4;
  int32_t slo[kSkip], shi[kSkip], ns = 0;
#pragma unroll
  for (int i = 0; i < kSkip; ++i) slo[i] = shi[i] = 0;
  const int ord = d0.y >= 0 ? d0.y / a.M : kOrderIndex;
  const bool sorted_row = c0 > 0 && ord != kOrderIndex;
  // (kWide) the prioritize column is wide: the jumps below.  (The records read the flag and
  // the column's multiplier again where they are written: nothing more stays live across
  // the fit, whose card state fills the registers of the 4-waves shapes.)
  bool pwide = false;
  if constexpr (kWide) pwide = c0 > 0 && a.wide_flag && a.wide_flag[pr.metric];
  // The pod's rules are loaded one per lane (32 at a time, a single round trip) and only the
  // ones on the prioritize metric are walked, one per half at a time (a rule by rule scan
  // waited for a load per rule).
  for (int32_t rc = r0; __ballot(sorted_row && rc < r1); rc += kPodLanes) {
   const bool in_l = sorted_row && rc + sub < r1;
   const pas_rule ru_l = a.rules[in_l ? rc + sub : 0];
   const bool same_l = in_l && ru_l.metric == pr.metric && ru_l.op >= 0 && ru_l.op <= 2;
   const uint64_t sm = __ballot(same_l);
   uint32_t todo = (uint32_t)sm | (uint32_t)(sm >> 32);  // rule slots some half walks
   while (todo) {
    const int u = __builtin_ctz(todo);
    todo &= todo - 1;
    const int src = half * kPodLanes + u;  // this half's rule in slot u
    pas_rule ru;
    ru.metric = __shfl(ru_l.metric, src, 64);
    ru.op = __shfl(ru_l.op, src, 64);
    ru.target = __shfl(ru_l.target, src, 64);
    const bool same = (sm >> src) & 1ull;
    int64_t tm = 0;
    int sat = target_scaled(ru.target, a.scale_tab, same ? pr.metric : 0, &tm);
    // A wide prioritize column: the target as it is against the pairs, lb = #(whole < t),
    // ub = #(pair <= (t, 0)).  The ranges below are then exact for a wide column too: [0, lb)
    // violates LessThan t, [ub, c) GreaterThan t (the nodes of whole == t with nano != 0
    // included), [lb, ub) Equals t (whole == t with nano == 0).
    if constexpr (kWide)
      if (pwide) tm = ru.target, sat = 0;
    int32_t lb = 0, ub = 0;
    half_bounds<kWide>(a, same ? pr.metric : 0, same ? c0 : 0, tm, sub, half_mask, pwide, &lb,
                       &ub);
    if (sat != 0) lb = ub = sat > 0 ? c0 : 0;
    if (same) {
      // the rule's nodes in ascending positions, mirrored for the descending row
      const int32_t gx = ru.op == PAS_OP_LESS_THAN ? 0 : ru.op == PAS_OP_GREATER_THAN ? ub : lb;
      const int32_t gy = ru.op == PAS_OP_LESS_THAN ? lb : ru.op == PAS_OP_GREATER_THAN ? c0 : ub;
      const int32_t lo = ord == kOrderDesc ? c0 - gy : gx;
      const int32_t hi = ord == kOrderDesc ? c0 - gx : gy;
      if (hi > lo) {
#pragma unroll
        for (int i = 0; i < kSkip; ++i)
          if (i == ns) {
            slo[i] = lo;
            shi[i] = hi;
          }
        ns = min(ns + 1, kSkip);
      }
    }
   }
  }
  // Pods of at most kStageRules rules (every pod of the wave): each lane compiles one rule
  // of its pod into LDS, read back per round as broadcast LDS reads instead of a global load
  // per lane, rule and round.
  const int pslot = (int)(threadIdx.x >> 6) * kPodsPerWave + half;
  const bool staged = !__ballot(have && r1 - r0 > kStageRules);
  if constexpr (!kPolicy) {
    if (staged) {
      LazyRule cr{0, 0};
      int32_t cm = -1;
      if constexpr (kWide) {
        int64_t ce = 0;
        int32_t cmode = kEdgeNone;
        if (have && r0 + sub < r1)
          compile_rule_wide(a.rules[r0 + sub], a.M, a.scale_tab, a.wide_flag, &cm, &cr, &ce,
                            &cmode);
        sedge[pslot][sub] = ce;
        smode[pslot][sub] = cmode;
      } else {
        if (have && r0 + sub < r1) compile_rule(a.rules[r0 + sub], a.M, a.scale_tab, &cm, &cr);
      }
      srule[pslot][sub] = cr;
      smetric[pslot][sub] = cm;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    }
  }
  const int32_t nr = have ? r1 - r0 : 0;
  const int32_t* row = a.perm + (int64_t)(d0.y >= 0 ? d0.y : 0) * a.R;
  const int64_t* mcol = a.vals + (int64_t)(d0.y >= 0 ? pr.metric : 0) * a.N;
  int64_t* keys = a.key_out + (int64_t)p * k;
  int32_t* nodes = a.node_out + (int64_t)p * k;
  int32_t kept = 0;
  int32_t j0 = 0;
  if constexpr (kAfter) j0 = have ? min(max(a.len_out[p], 0), c0) : 0;
  for (;; j0 += kPodLanes) {
#pragma unroll
    for (int it = 0; it < kSkip; ++it)
#pragma unroll
      for (int i = 0; i < kSkip; ++i)
        if (i < ns && j0 >= slo[i] && j0 < shi[i]) j0 = shi[i];
    const bool active = j0 < c0 && kept < k;  // (uniform within the pod's half)
    if (!__ballot(active)) break;
    const int32_t j = j0 + sub;
    const bool valid = active && j < c0;
    const int32_t n = valid ? row[j] : 0;
    bool ok = valid;
    if (a.cand) ok = ok && ((a.cand[(int64_t)p * a.W64 + (n >> 6)] >> (n & 63)) & 1ull);
    // dontschedule.Violated (strategy.go:25-44) at this node: any rule whose metric the node
    // has and whose EvaluateRule holds; rules on metrics outside the cache or with an
    // unknown operator are skipped.  kRuleBatch rules' loads in flight at once.
    bool viol = false;
    if constexpr (kPolicy) {
      // the policy's cached verdict: one word of its violating set, by the lanes still
      // passing (n < N: an entry of the order row below the present count)
      if (ok && pol >= 0)
        viol = (a.viol[(int64_t)pol * a.W64 + (n >> 6)] >> (n & 63)) & 1ull;
    } else {
      const int64_t* vrow = a.vals_t + (int64_t)n * a.M;
      const uint64_t* prow = a.pres_t + (int64_t)n * a.WM;
      if (staged) {
        for (int32_t rb = 0; __ballot(ok && rb < nr); rb += kRuleBatch) {
          int32_t m[kRuleBatch];
          int64_t v[kRuleBatch];
          uint64_t pw[kRuleBatch];
#pragma unroll
          for (int u = 0; u < kRuleBatch; ++u) m[u] = smetric[pslot][min(rb + u, kStageRules - 1)];
          // (one presence word per node when the snapshot has at most 64 metrics)
          const uint64_t pw0 = a.WM == 1 ? prow[0] : 0;
#pragma unroll
          for (int u = 0; u < kRuleBatch; ++u) {
            const int32_t mm = m[u] >= 0 ? m[u] : 0;
            v[u] = vrow[mm];
            pw[u] = a.WM == 1 ? pw0 : prow[mm >> 6];
          }
#pragma unroll
          for (int u = 0; u < kRuleBatch; ++u) {
            const LazyRule cr = srule[pslot][min(rb + u, kStageRules - 1)];
            bool hit = rb + u < nr && m[u] >= 0 &&
                       (uint64_t)v[u] - (uint64_t)cr.lo <= cr.span &&
                       ((pw[u] >> (m[u] & 63)) & 1ull);
            if constexpr (kWide) {
              // the range's edge on a wide column: the node's nano decides (a rare gather of
              // the metric-major nano column, by the lanes on the edge only)
              const int32_t md = smode[pslot][min(rb + u, kStageRules - 1)];
              if (hit && md != kEdgeNone && v[u] == sedge[pslot][min(rb + u, kStageRules - 1)]) {
                const uint32_t f = a.nano[(int64_t)m[u] * a.N + n];
                hit = (f != 0u) == (md == kEdgeNanoNonZero);
              }
            }
            viol = viol || hit;
          }
        }
      }
      for (int32_t rb = r0; !staged && __ballot(ok && rb < r1); rb += kRuleBatch) {
        pas_rule ru[kRuleBatch];
        int64_t v[kRuleBatch];
        uint64_t pw[kRuleBatch];
#pragma unroll
        for (int u = 0; u < kRuleBatch; ++u) ru[u] = a.rules[max(min(rb + u, r1 - 1), 0)];
#pragma unroll
        for (int u = 0; u < kRuleBatch; ++u) {
          const int32_t m = (ru[u].metric >= 0 && ru[u].metric < a.M) ? ru[u].metric : 0;
          v[u] = vrow[m];
          pw[u] = prow[m >> 6];
        }
#pragma unroll
        for (int u = 0; u < kRuleBatch; ++u) {
          const pas_rule rule = ru[u];
          if (rb + u >= r1 || rule.metric < 0 || rule.metric >= a.M || rule.op < 0 || rule.op > 2)
            continue;
          if constexpr (kWide) {
            if (a.wide_flag && a.wide_flag[rule.metric]) {
              const int64_t t = rule.target;
              uint32_t f = 0;
              if (v[u] == t && rule.op != PAS_OP_LESS_THAN)
                f = a.nano[(int64_t)rule.metric * a.N + n];
              const bool wh = rule.op == PAS_OP_LESS_THAN      ? wide_below(v[u], f, t)
                              : rule.op == PAS_OP_GREATER_THAN ? wide_above(v[u], f, t)
                                                               : wide_equal(v[u], f, t);
              viol = viol || (wh && ((pw[u] >> (rule.metric & 63)) & 1ull));
              continue;
            }
          }
          int64_t tm = 0;
          const int sat = target_scaled(rule.target, a.scale_tab, rule.metric, &tm);
          bool hit;
          if (rule.op == PAS_OP_LESS_THAN) hit = sat > 0 || (sat == 0 && v[u] < tm);
          else if (rule.op == PAS_OP_GREATER_THAN) hit = sat < 0 || (sat == 0 && v[u] > tm);
          else hit = sat == 0 && v[u] == tm;
          viol = viol || (hit && ((pw[u] >> (rule.metric & 63)) & 1ull));
        }
      }
    }
    ok = ok && !viol;
    if constexpr (kFit) {
      if (ok) ok = lane_fit<KMAX, QW>(a, p, n);
    }
    const uint64_t keep = __ballot(ok) & half_mask;
    if (ok) {
      const int32_t rank = kept + __popcll(keep & below);
      if (rank < k) {
        nodes[rank] = n + a.node_base;
        if constexpr (kWide) {
          // the canonical pair of the node's value (one 64-bit division per kept record of a
          // narrow column, none per node walked)
          int64_t W = mcol[n];
          uint32_t F = 0;
          if (a.wide_flag && a.wide_flag[pr.metric]) F = a.nano[(int64_t)pr.metric * a.N + n];
          else canonical_pair(W, a.scale_tab[2 * pr.metric], &W, &F);
          wide_order_key(pr.op, W, F, &keys[rank], &a.sub_out[(int64_t)p * k + rank]);
        } else {
          keys[rank] = order_key(pr.op, mcol[n]);
        }
      }
    }
    kept += active ? __popcll(keep) : 0;
  }
  if (!have) return;
  const int32_t len = min(kept, k);
  for (int32_t i = len + sub; i < k; i += kPodLanes) {
    keys[i] = INT64_MAX;
    if constexpr (kWide) a.sub_out[(int64_t)p * k + i] = UINT32_MAX;
    nodes[i] = INT32_MAX;
  }
  if (sub == 0) a.len_out[p] = len;
}

// vals [M][N] -> vals_t [N][M] through 64 x 64 LDS tiles (coalesced both ways)
__global__ __launch_bounds__(kTpb) void transpose_vals_kernel(int32_t N, int32_t M,
                                                               const int64_t* __restrict__ vals,
                                                               int64_t* __restrict__ vals_t) {
  __shared__ int64_t tile[64][65];
  const int32_t n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += kWaves) {
    const int32_t m = m0 + r, n = n0 + tx;
    tile[r][tx] = (m < M && n < N) ? vals[(int64_t)m * N + n] : 0;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += kWaves) {
    const int32_t n = n0 + r, m = m0 + tx;
    if (n < N && m < M) vals_t[(int64_t)n * M + m] = tile[tx][r];
  }
}

// present [M][W64] -> pres_t [N][WM]: bit m of node n's word m / 64
__global__ __launch_bounds__(kTpb) void transpose_present_kernel(
    int32_t N, int32_t M, int32_t W64, int32_t WM, const uint64_t* __restrict__ present,
    uint64_t* __restrict__ pres_t) {
  const int32_t n = blockIdx.x * kTpb + threadIdx.x;
  if (n >= N) return;
  for (int32_t w = 0; w < WM; ++w) {
    uint64_t word = 0;
    for (int32_t j = 0; j < 64 && w * 64 + j < M; ++j) {
      const uint64_t bit = (present[(int64_t)(w * 64 + j) * W64 + (n >> 6)] >> (n & 63)) & 1ull;
      word |= bit << j;
    }
    pres_t[(int64_t)n * WM + w] = word;
  }
}

// The resumed walk's start positions (pas.h, "Resuming a top-k list").
struct TopkStartParams {
  int32_t n_pods, N, M, R, node_base;
  const pas_rule* prio;
  const int32_t* perm;          // [3][M][R]
  const int32_t* cnt;           // [M]
  const int64_t* sorted;        // [M][R]
  const uint32_t* sorted_nano;  // [M][R] (wide columns)
  const int64_t* scale_tab;
  const uint8_t* wide_flag;     // null while the snapshot holds no wide column
  const int64_t* after_key;     // [P] the cursors
  const uint32_t* after_sub;    // [P] (kWide)
  const int32_t* after_node;    // [P] global ids
  int32_t* start;               // [P]
};

// First position of [lo, hi) at which before(position) does not hold (hi if none); before
// must hold on a prefix of the range.
template <typename F>
__device__ __forceinline__ int32_t first_not(int32_t lo, int32_t hi, F before) {
  while (lo < hi) {
    const int32_t mid = (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1);
    if (before(mid)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// start[p] = the number of entries of pod p's order row whose record is <= the pod's cursor
// in ascending (key[, sub], node), a lane per pod.  Sorted rows: the cursor's key decodes to a
// value (v = key for LessThan, ~key for GreaterThan; kWide: the pair (W, F) from key and sub
// the same way); [lb, ub) is that value's tie run in the ascending column, mirrored to
// [c0 - ub, c0 - lb) in the descending row; everything before the run is before the cursor,
// and within the run (ascending node index in both rows) the nodes up to the cursor's.  Index
// rows: every record has key 0 (sub 0), so a cursor key below that starts at 0, one above it
// at c0, and key 0 at the number of nodes up to the cursor's.  kWide on a narrow column
// compares each probed stored value's canonical pair with (W, F): the cursor is never
// converted into the column's unit, which the sentinels would overflow.  Every bit pattern of
// a cursor has a start in [0, c0]; c0 = 0 (no rule, metric not cached) stays the empty list.
template <bool kWide>
__global__ __launch_bounds__(kTpb) void topk_start_kernel(TopkStartParams a) {
  const int32_t p = blockIdx.x * kTpb + threadIdx.x;
  if (p >= a.n_pods) return;
  const pas_rule q = a.prio[p];
  const int32_t m = q.metric;
  const int32_t c0 = (m >= 0 && m < a.M) ? a.cnt[m] : 0;
  int32_t start = 0;
  if (c0 > 0) {
    const int64_t ck = a.after_key[p];
    uint32_t cs = 0;
    if constexpr (kWide) cs = a.after_sub[p];
    // the cursor's node as a local id, clamped to [-1, N]: a node below the shard counts none
    // of a run, one at or past the shard's end all of it
    const int64_t loc = (int64_t)a.after_node[p] - (int64_t)a.node_base;
    const int32_t cn = (int32_t)(loc < -1 ? -1 : loc > a.N ? a.N : loc);
    const int ord = q.op == PAS_OP_GREATER_THAN ? kOrderDesc
                    : q.op == PAS_OP_LESS_THAN  ? kOrderAsc
                                                : kOrderIndex;
    const int32_t* row = a.perm + ((int64_t)ord * a.M + m) * a.R;
    auto node_not_above = [&](int32_t j) { return row[j] <= cn; };
    if (ord == kOrderIndex) {
      const bool above = ck > 0 || (kWide && ck == 0 && cs > 0u);
      start = ck < 0 ? 0 : above ? c0 : first_not(0, c0, node_not_above);
    } else {
      const bool desc = ord == kOrderDesc;
      const int64_t v = desc ? ~ck : ck;
      const int64_t* sv = a.sorted + (int64_t)m * a.R;
      int32_t lb, ub;
      if constexpr (kWide) {
        const uint32_t f = desc ? ~cs : cs;
        if (a.wide_flag && a.wide_flag[m]) {
          const uint32_t* sn = a.sorted_nano + (int64_t)m * a.R;
          lb = bound<true>(sv, sn, c0, v, f, false);
          ub = lb + bound<true>(sv + lb, sn + lb, c0 - lb, v, f, true);
        } else {
          const int64_t mult = a.scale_tab[2 * m];
          auto before = [&](int32_t j, bool upper) {
            int64_t W;
            uint32_t F;
            canonical_pair(sv[j], mult, &W, &F);
            return upper ? pair_not_above(W, F, v, f) : pair_below(W, F, v, f);
          };
          lb = first_not(0, c0, [&](int32_t j) { return before(j, false); });
          ub = first_not(lb, c0, [&](int32_t j) { return before(j, true); });
        }
      } else {
        lb = bound<false>(sv, nullptr, c0, v, 0u, false);
        ub = lb + bound<false>(sv + lb, nullptr, c0 - lb, v, 0u, true);
      }
      const int32_t t0 = desc ? c0 - ub : lb, t1 = desc ? c0 - lb : ub;
      start = first_not(t0, t1, node_not_above);
    }
  }
  a.start[p] = start;
}

template <bool kWide, bool kAfter>
void topk_dispatch(const LazyTopkParams& a, unsigned grid, hipStream_t s) {
  if (a.K <= 8) {
    switch (a.Q) {
      case 1: tas_gas_topk_kernel<8, 1, kWide, kAfter><<<grid, kTpb, 0, s>>>(a); break;
      case 2: tas_gas_topk_kernel<8, 2, kWide, kAfter><<<grid, kTpb, 0, s>>>(a); break;
      case 3: tas_gas_topk_kernel<8, 3, kWide, kAfter><<<grid, kTpb, 0, s>>>(a); break;
      default: tas_gas_topk_kernel<8, kMaxRes, kWide, kAfter><<<grid, kTpb, 0, s>>>(a); break;
    }
  } else if (a.K <= 16) {
    tas_gas_topk_kernel<16, kMaxRes, kWide, kAfter><<<grid, kTpb, 0, s>>>(a);
  } else {
    tas_gas_topk_kernel<PAS_GAS_MAX_CARDS, kMaxRes, kWide, kAfter><<<grid, kTpb, 0, s>>>(a);
  }
}

// The same tiers for the policy form (kPolicy, with the fit).
template <bool kWide, bool kAfter>
void topk_policy_dispatch(const LazyTopkParams& a, unsigned grid, hipStream_t s) {
  if (a.K <= 8) {
    switch (a.Q) {
      case 1: tas_gas_topk_kernel<8, 1, kWide, kAfter, true><<<grid, kTpb, 0, s>>>(a); break;
      case 2: tas_gas_topk_kernel<8, 2, kWide, kAfter, true><<<grid, kTpb, 0, s>>>(a); break;
      case 3: tas_gas_topk_kernel<8, 3, kWide, kAfter, true><<<grid, kTpb, 0, s>>>(a); break;
      default: tas_gas_topk_kernel<8, kMaxRes, kWide, kAfter, true><<<grid, kTpb, 0, s>>>(a); break;
    }
  } else if (a.K <= 16) {
    tas_gas_topk_kernel<16, kMaxRes, kWide, kAfter, true><<<grid, kTpb, 0, s>>>(a);
  } else {
    tas_gas_topk_kernel<PAS_GAS_MAX_CARDS, kMaxRes, kWide, kAfter, true><<<grid, kTpb, 0, s>>>(a);
  }
}

template <bool kWide, bool kAfter, bool kPolicy>
void topk_launch_walk(const LazyTopkParams& a, unsigned grid, hipStream_t s) {
  if constexpr (kPolicy) topk_policy_dispatch<kWide, kAfter>(a, grid, s);
  else topk_dispatch<kWide, kAfter>(a, grid, s);
}

// The walk's parameters that come from the TAS snapshot and the call's outputs (d_sub null =
// the 64-bit records); the rules, the GAS side and the policy fields are the caller's to set.
LazyTopkParams topk_params(const TasSnapshot& t, int32_t n_pods, const uint64_t* d_cand,
                           int32_t k, int32_t node_base, int64_t* d_key, uint32_t* d_sub,
                           int32_t* d_node, int32_t* d_len) {
  LazyTopkParams a{};
  a.n_pods = n_pods;
  a.N = t.n_nodes;
  a.M = t.n_metrics;
  a.R = t.row;
  a.W64 = (int32_t)w64(t.n_nodes);
  a.k = k;
  a.node_base = node_base;
  a.cand = d_cand;
  a.perm = t.perm;
  a.cnt = t.cnt;
  a.vals = t.vals;
  a.WM = (t.n_metrics + 63) / 64;
  a.sorted = t.sorted;
  a.f1k = t.f1k;
  a.f32 = t.f32;
  a.scale_tab = t.scale_tab;
  a.key_out = d_key;
  a.node_out = d_node;
  a.len_out = d_len;
  a.sub_out = d_sub;
  a.nano = t.n_wide > 0 ? t.nano : nullptr;
  a.wide_flag = t.n_wide > 0 ? t.wide_flag : nullptr;
  a.sorted_nano = t.sorted_nano;
  a.f1k_nano = t.f1k_nano;
  a.f32_nano = t.f32_nano;
  return a;
}

void topk_gas_params(LazyTopkParams& a, const GasSnapshot& g, int32_t i915_index,
                     const PodBatch& pods) {
  a.K = g.max_cards;
  a.Q = g.n_res;
  a.C = pods.max_containers;
  a.i915 = i915_index;
  a.n_cards = g.n_cards;
  a.cap = g.cap;
  a.used = g.used;
  a.req = pods.req;
  a.mask = pods.mask;
  a.ncont = pods.n_containers;
}

// The walk on s, timed as PAS_K_TAS_GAS_TOPK: from the lists' beginning, or (d_after_key)
// resumed after the cursors, whose start positions topk_start_kernel leaves in len_out where
// the walk reads them.  d_start_prio [P]: the pods' prio rules for the start kernel (the rules
// form's a.prio; the policy form's gathered out of the table).  fit = false: the kFit = false
// walk (kPolicy, not resumed).
template <bool kPolicy>
int topk_walk(pas_ctx* ctx, const LazyTopkParams& a, bool fit, const pas_rule* d_start_prio,
              const int64_t* d_after_key, const uint32_t* d_after_sub,
              const int32_t* d_after_node, hipStream_t s) {
  const TasSnapshot& t = ctx->tas;
  TimedLaunch tl;
  timing_begin(ctx, s, PAS_K_TAS_GAS_TOPK, &tl);
  const unsigned grid = (unsigned)((a.n_pods + kPodsPerBlock - 1) / kPodsPerBlock);
  if constexpr (kPolicy) {
    if (!fit) {
      if (a.sub_out) tas_gas_topk_kernel<8, 1, true, false, true, false><<<grid, kTpb, 0, s>>>(a);
      else tas_gas_topk_kernel<8, 1, false, false, true, false><<<grid, kTpb, 0, s>>>(a);
      timing_end(ctx, s, &tl);
      PAS_HIP(ctx, hipGetLastError());
      return PAS_OK;
    }
  }
  if (d_after_key) {
    TopkStartParams b;
    b.n_pods = a.n_pods;
    b.N = a.N;
    b.M = a.M;
    b.R = t.row;
    b.node_base = a.node_base;
    b.prio = d_start_prio;
    b.perm = t.perm;
    b.cnt = t.cnt;
    b.sorted = t.sorted;
    b.sorted_nano = t.sorted_nano;
    b.scale_tab = t.scale_tab;
    b.wide_flag = a.wide_flag;
    b.after_key = d_after_key;
    b.after_sub = d_after_sub;
    b.after_node = d_after_node;
    b.start = a.len_out;
    const unsigned sgrid = (unsigned)((a.n_pods + kTpb - 1) / kTpb);
    if (a.sub_out) {
      topk_start_kernel<true><<<sgrid, kTpb, 0, s>>>(b);
      topk_launch_walk<true, true, kPolicy>(a, grid, s);
    } else {
      topk_start_kernel<false><<<sgrid, kTpb, 0, s>>>(b);
      topk_launch_walk<false, true, kPolicy>(a, grid, s);
    }
  } else if (a.sub_out) {
    topk_launch_walk<true, false, kPolicy>(a, grid, s);
  } else {
    topk_launch_walk<false, false, kPolicy>(a, grid, s);
  }
  timing_end(ctx, s, &tl);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

}  // namespace

int tas_gas_topk_launch(pas_ctx* ctx, int32_t n_rules, const pas_rule* d_rules,
                        const int32_t* d_rule_off, const pas_rule* d_prio,
                        const uint64_t* d_cand, int32_t i915_index, const PodBatch& pods,
                        int32_t k, int32_t node_base, int64_t* d_key, uint32_t* d_sub,
                        int32_t* d_node, int32_t* d_len, const int64_t* d_after_key,
                        const uint32_t* d_after_sub, const int32_t* d_after_node, hipStream_t s) {
  const int32_t n_pods = pods.n_pods;
  if (n_pods == 0) return PAS_OK;
  TasSnapshot& t = ctx->tas;
  const int32_t N = t.n_nodes, M = t.n_metrics;
  const int32_t WM = (M + 63) / 64;
  // node-major copies, once per snapshot change
  if (t.t_epoch != t.epoch && N > 0 && M > 0) {
    const size_t bv = sizeof(int64_t) * (size_t)N * M, bp = sizeof(uint64_t) * (size_t)N * WM;
    // (two allocations, each with its own size: a reshape can keep their sum and grow one)
    if (t.vals_t_bytes < bv || t.pres_t_bytes < bp) {
      if (t.vals_t || t.pres_t) {
        PAS_HIP(ctx, hipStreamSynchronize(s));
        if (t.vals_t) PAS_HIP(ctx, hipFree(t.vals_t));
        if (t.pres_t) PAS_HIP(ctx, hipFree(t.pres_t));
        t.vals_t = nullptr;
        t.pres_t = nullptr;
      }
      t.vals_t_bytes = t.pres_t_bytes = 0;
      PAS_HIP(ctx, hipMalloc(&t.vals_t, bv));
      t.vals_t_bytes = bv;
      PAS_HIP(ctx, hipMalloc(&t.pres_t, bp));
      t.pres_t_bytes = bp;
    }
    transpose_vals_kernel<<<dim3((unsigned)((N + 63) / 64), (unsigned)((M + 63) / 64)), kTpb, 0,
                            s>>>(N, M, t.vals, t.vals_t);
    transpose_present_kernel<<<(unsigned)((N + kTpb - 1) / kTpb), kTpb, 0, s>>>(
        N, M, (int32_t)w64(N), WM, t.present, t.pres_t);
    PAS_HIP(ctx, hipGetLastError());
    t.t_epoch = t.epoch;
    if (int e = derived_built(ctx, t.t_sync, s)) return e;
  } else if (int e = derived_wait(ctx, t.t_sync, s)) {
    return e;  // built by a call on another stream, maybe still running
  }
  LazyTopkParams a = topk_params(t, n_pods, d_cand, k, node_base, d_key, d_sub, d_node, d_len);
  a.rules = d_rules;
  a.rule_off = d_rule_off;
  a.n_rules = std::max(n_rules, 0);
  a.prio = d_prio;
  a.vals_t = t.vals_t;
  a.pres_t = t.pres_t;
  topk_gas_params(a, ctx->gas, i915_index, pods);
  return topk_walk<false>(ctx, a, true, d_prio, d_after_key, d_after_sub, d_after_node, s);
}

// The policy form: the walk over the resident table and its cached violating sets.  Neither
// builds nor reads the node-major copies (vals_t / pres_t): a context that only ever calls
// this form never allocates them.
int tas_gas_topk_policies_launch(pas_ctx* ctx, const int32_t* d_pod_policy,
                                 const uint64_t* d_cand, bool fit, int32_t i915_index,
                                 const PodBatch& pods, int32_t k, int32_t node_base,
                                 int64_t* d_key, uint32_t* d_sub, int32_t* d_node, int32_t* d_len,
                                 const int64_t* d_after_key, const uint32_t* d_after_sub,
                                 const int32_t* d_after_node, hipStream_t s) {
  const int32_t n_pods = pods.n_pods;
  if (n_pods == 0) return PAS_OK;
  const TasPolicies& pt = ctx->policies;
  // built on s if the snapshot or the table changed, else s waits for the build's event
  const uint64_t* viol = nullptr;
  int rc = policies_viol(ctx, s, &viol);
  if (rc) return rc;
  LazyTopkParams a =
      topk_params(ctx->tas, n_pods, d_cand, k, node_base, d_key, d_sub, d_node, d_len);
  a.rules = pt.d_rules;
  a.rule_off = pt.d_rule_off;
  a.n_rules = pt.n_rules;
  a.prio = pt.d_prio;
  a.pod_policy = d_pod_policy;
  a.n_policies = pt.n_policies;
  a.viol = viol;
  if (!fit) return topk_walk<true>(ctx, a, false, nullptr, nullptr, nullptr, nullptr, s);
  topk_gas_params(a, ctx->gas, i915_index, pods);
  if (!d_after_key) return topk_walk<true>(ctx, a, true, nullptr, nullptr, nullptr, nullptr, s);
  // the start kernel takes per-pod prio rules: gathered out of the table into the stream's
  // slot, which stays this call's until the walk is enqueued
  SlotScope sc(ctx, s, 0, &rc);
  if (!sc.slot) return rc;
  pas_rule* d_prio = nullptr;
  if ((rc = policy_prio_gather(ctx, sc.slot, n_pods, d_pod_policy, &d_prio, nullptr, s)))
    return rc;
  return topk_walk<true>(ctx, a, true, d_prio, d_after_key, d_after_sub, d_after_node, s);
}

}  // namespace pas
