// gas_place.hip — batch placement: pods bound in order along their candidate rows.
//
// The definition is sequential (pas.h, pas_gas_place): pod after pod, each pod tries the
// nodes of its row in order and commits to the first one that takes it, and every bind sees
// the usage left by the binds before it (GASExtender.bindNode is called pod after pod,
// scheduler.go:385-445).  Binds on different nodes do not see each other, so the work is done
// in node-centric rounds, each a few launches on the call's stream:
//
//   mark    every unfinished pod q appends the key (node under its cursor, q) and marks each
//           LATER in-range entry of its row: blocker[n] = the lowest such q, kept as an
//           agent-scope 64-bit atomicMax of (round << 32) | ~q, so nothing is cleared
//           between rounds (a word of an earlier round is no blocker)
//   sort    the keys (rocprim radix sort): one run per node, pods ascending within it
//   commit  one wave per run holds the node's usage in LDS and takes its pods in order while
//           pod <= blocker[n]: a pod that fits is finished, one that does not moves its
//           cursor to the next in-range entry (finished unplaced at the row's end); the
//           usage is written back once and the pods finished are counted into one word,
//           once per workgroup
//
// The host reads that word after each round and stops when no pod is left.
//
// Exact: when p is processed at n, every lower unfinished pod that could still bind to n
// sits earlier in the same run or would be a blocker below p.  No higher pod can have
// committed to n before: p was unfinished then with n at or after its cursor, so p was ahead
// of that pod in the run or was its blocker.  `<=` because a row that repeats a node makes the
// pod its own blocker.  One node has one owner wave per round (no atomics on the usage);
// kernel boundaries order the rounds.  The lowest unfinished pod is never blocked, so every
// round moves a cursor: at most sum(row lengths) rounds, which the host loop enforces.
#include <hip/hip_runtime.h>

#include "gas_bind.h"
#include "gas_group.h"
#include "pas_internal.h"

namespace pas {
namespace {

constexpr int kTpb = 64;       // commit: one wave per workgroup, one workgroup per key
constexpr int kPodTpb = 256;   // init / mark: one thread per pod
constexpr int kMaxRes = kBindMaxRes;

struct PlaceCtr {
  uint32_t n_keys[2];    // keys of the round (by round parity; mark zeroes the other one)
  uint32_t finished[2];  // pods the round's commit finished (by round parity, likewise)
  uint32_t active;       // pods with an in-range entry at the start
  uint32_t placed;       // pods placed so far
  unsigned long long total_len;  // sum of the clamped row lengths: the round bound
};

struct PlaceArgs {
  int32_t n_pods, k, ld, n_nodes;
  int64_t node_base;
  int32_t pod_bits;        // key = node << pod_bits | pod
  const int32_t* cand;     // [n_pods][ld]
  const int32_t* cand_len; // [n_pods] or null
  int32_t* cursor;         // [n_pods] entry the pod tries next, -1 = finished
  unsigned long long* blocker;  // [n_nodes]
  unsigned long long* keys;     // [n_pods]
  PlaceCtr* ctr;
  int32_t* place_node;
  int32_t* place_rank;
};

__device__ __forceinline__ int32_t row_len(const PlaceArgs& a, int32_t p) {
  return a.cand_len ? max(0, min(a.cand_len[p], a.k)) : a.k;
}
// The shard's node of entry j of row p, -1 for padding and ids of other shards.
__device__ __forceinline__ int32_t row_node(const PlaceArgs& a, int32_t p, int32_t j) {
  const int64_t n = (int64_t)a.cand[(int64_t)p * a.ld + j] - a.node_base;
  return n >= 0 && n < a.n_nodes ? (int32_t)n : -1;
}
// The first in-range entry of row p at or after j, -1 past the row's end.
__device__ __forceinline__ int32_t next_entry(const PlaceArgs& a, int32_t p, int32_t j,
                                              int32_t len) {
  for (; j < len; ++j)
    if (row_node(a, p, j) >= 0) return j;
  return -1;
}
// Lane 0 of the wave gets the sum (every lane of the wave calls it).
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

__global__ __launch_bounds__(kPodTpb) void place_init_kernel(PlaceArgs a, uint32_t* res_out,
                                                             int32_t* nsel_out) {
  const int32_t p = blockIdx.x * kPodTpb + threadIdx.x;
  unsigned long long act = 0, len = 0;
  if (p < a.n_pods) {
    len = (unsigned long long)row_len(a, p);
    const int32_t c = next_entry(a, p, 0, (int32_t)len);
    a.cursor[p] = c;
    a.place_node[p] = -1;
    a.place_rank[p] = -1;
    res_out[p] = 0u;
    if (nsel_out) nsel_out[p] = 0;
    act = c >= 0;
  }
  act = wave_sum(act);
  len = wave_sum(len);
  if ((threadIdx.x & 63) == 0) {
    if (act) atomicAdd(&a.ctr->active, (uint32_t)act);
    if (len) atomicAdd(&a.ctr->total_len, len);
  }
}

__global__ __launch_bounds__(kPodTpb) void place_mark_kernel(PlaceArgs a, uint32_t round) {
  const int32_t p = blockIdx.x * kPodTpb + threadIdx.x;
  const uint32_t par = round & 1u;
  if (p == 0) {  // the next round's words (this round uses the other parity)
    a.ctr->n_keys[par ^ 1u] = 0u;
    a.ctr->finished[par ^ 1u] = 0u;
  }
  if (p >= a.n_pods) return;
  const int32_t c = a.cursor[p];
  if (c < 0) return;
  const int32_t len = row_len(a, p);
  const int32_t n = c < len ? row_node(a, p, c) : -1;
  if (n < 0) return;  // (a cursor rests on in-range entries only)
  const uint32_t slot = atomicAdd(&a.ctr->n_keys[par], 1u);
  if (slot < (uint32_t)a.n_pods)
    a.keys[slot] = ((unsigned long long)n << a.pod_bits) | (unsigned long long)p;
  const unsigned long long word = ((unsigned long long)round << 32) | (uint32_t)~(uint32_t)p;
  for (int32_t j = c + 1; j < len; ++j) {
    const int32_t m = row_node(a, p, j);
    if (m >= 0) atomicMax(&a.blocker[m], word);
  }
}

// One wave per key; the wave at a run's first key does the run.  The node's usage lives in LDS.
// The binds of a run are sequential, but a bind that does not fit changes nothing: the wave
// tries the run's next 64 pods at once, each lane on a private copy of the usage, and takes
// them up to and including the first that fits: the lanes before it failed on exactly the
// usage the sequential loop shows them, that lane commits its copy, and the lanes after it
// are tried again on the new usage (whatever they wrote to the result rows is written again).
template <int KMAX>
__global__ __launch_bounds__(kTpb) void place_commit_kernel(PlaceArgs a, BindArgs b,
                                                            uint32_t round, uint32_t n_keys) {
  __shared__ int64_t su[KMAX][kMaxRes];
  const uint32_t head = blockIdx.x;  // < n_keys (the grid)
  const uint32_t lane = threadIdx.x;
  const unsigned long long n = a.keys[head] >> a.pod_bits;
  if (head > 0 && (a.keys[head - 1] >> a.pod_bits) == n) return;  // not a run's first key
  if (n >= (unsigned long long)a.n_nodes) return;
  const int32_t K = b.K, Q = b.Q;
  const int32_t ncard = min(b.n_cards[n], K);
  int64_t* un = b.used + (int64_t)n * K * Q;
  for (int32_t e = lane; e < K * Q; e += kTpb) su[e / Q][e % Q] = un[e];
  int64_t cap[kMaxRes];
  for (int q = 0; q < Q; ++q) cap[q] = b.cap[(int64_t)n * Q + q];
  const unsigned long long blk = a.blocker[n];
  const uint32_t last = (uint32_t)(blk >> 32) == round ? ~(uint32_t)blk : 0xffffffffu;
  const unsigned long long pod_mask = (1ull << a.pod_bits) - 1ull;
  __syncthreads();
  uint32_t base = head, done = 0, placed = 0;  // (wave-uniform)
  for (;;) {
    // the run's pods at base .. base + 63 that are not blocked: a prefix of the lanes (the
    // keys ascend by node, then pod)
    const uint32_t t = base + lane;
    bool valid = false;
    int32_t p = 0;
    if (t < n_keys) {
      const unsigned long long key = a.keys[t];
      const uint32_t pu = (uint32_t)(key & pod_mask);
      valid = (key >> a.pod_bits) == n && pu <= last && pu < (uint32_t)a.n_pods;
      p = (int32_t)pu;
    }
    const int n_valid = __popcll(__ballot(valid));
    if (n_valid == 0) break;
    bool tried = false, fit = false;
    int32_t c = -1, len = 0;
    int64_t u[KMAX][kMaxRes];
    if (valid) {
      c = a.cursor[p];
      len = row_len(a, p);
      if (c >= 0 && c < len) {  // (a cursor rests on an entry of the row)
        tried = true;
        for (int k = 0; k < K; ++k)
          for (int q = 0; q < Q; ++q) u[k][q] = su[k][q];
        fit = bind_one<KMAX>(b, u, cap, ncard, p, max(0, min(b.ncont[p], b.C)), p);
      }
    }
    const unsigned long long fits = __ballot(fit);
    const uint32_t first = fits ? (uint32_t)__ffsll((long long)fits) - 1u : (uint32_t)kTpb;
    bool ended = false;  // finished unplaced
    if (tried && lane < first) {
      const int32_t c2 = next_entry(a, p, c + 1, len);
      a.cursor[p] = c2;
      ended = c2 < 0;
    } else if (tried && lane == first) {
      for (int k = 0; k < K; ++k)
        for (int q = 0; q < Q; ++q) su[k][q] = u[k][q];
      a.place_node[p] = a.cand[(int64_t)p * a.ld + c];
      a.place_rank[p] = c;
      a.cursor[p] = -1;
    }
    done += (uint32_t)__popcll(__ballot(ended)) + (first < (uint32_t)kTpb);
    placed += first < (uint32_t)kTpb;
    __syncthreads();  // the committed usage, before the next lanes copy it
    if (first < (uint32_t)kTpb) {
      base += first + 1u;
    } else {
      if (n_valid < kTpb) break;  // the run's end, or its first blocked pod
      base += kTpb;
    }
  }
  for (int32_t e = lane; e < K * Q; e += kTpb) un[e] = su[e / Q][e % Q];
  if (lane == 0) {
    if (done) atomicAdd(&a.ctr->finished[round & 1u], done);
    if (placed) atomicAdd(&a.ctr->placed, placed);
  }
}

}  // namespace

int gas_place_launch(pas_ctx* ctx, int32_t i915_index, const PodBatch& pods, int32_t k,
                     int32_t ld, int32_t node_base, const int32_t* d_cand,
                     const int32_t* d_cand_len, int32_t* d_place_node, int32_t* d_place_rank,
                     uint32_t* d_res, uint8_t* d_cards_out, int32_t* d_nsel_out,
                     int64_t* d_counts_out, int32_t* n_placed, int32_t* n_rounds,
                     bool* began, hipStream_t s) {
  *began = false;
  if (n_placed) *n_placed = 0;
  if (n_rounds) *n_rounds = 0;
  const int32_t n_pods = pods.n_pods;
  if (n_pods == 0) return PAS_OK;
  GasSnapshot& g = ctx->gas;
  const size_t P = (size_t)n_pods, N = (size_t)std::max(g.n_nodes, 1);
  const unsigned pod_bits = key_bits(n_pods), end_bit = pod_bits + key_bits(g.n_nodes);
  if (!ctx->place_host)  // the round loop's read-back (pinned)
    PAS_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->place_host), sizeof(PlaceCtr)));
  PlaceCtr* h = static_cast<PlaceCtr*>(ctx->place_host);
  size_t sort_bytes = 0;
  PAS_HIP(ctx, rocprim::radix_sort_keys(nullptr, sort_bytes, (unsigned long long*)nullptr,
                                        (unsigned long long*)nullptr, P, 0u, end_bit, s));
  sort_bytes = std::max<size_t>(sort_bytes, 16);
  int rc = PAS_OK;
  SlotScope scope(ctx, s, 0, &rc);
  if (!scope.slot) return rc;
  const size_t bytes = carve_size({sizeof(PlaceCtr), sizeof(int32_t) * P, 8 * P, 8 * P, 8 * N,
                                   sort_bytes});
  void* buf = slot_buf(ctx, scope.slot, kBufPlace, bytes, s, &rc);
  if (!buf) return rc;
  Carve cv{static_cast<char*>(buf)};
  PlaceCtr* d_ctr = cv.take<PlaceCtr>(1);
  int32_t* d_cursor = cv.take<int32_t>(P);
  unsigned long long* d_keys = cv.take<unsigned long long>(P);
  unsigned long long* d_sorted = cv.take<unsigned long long>(P);
  unsigned long long* d_blocker = cv.take<unsigned long long>(N);
  void* d_sort_tmp = cv.take<char>(sort_bytes);

  const int32_t K = g.max_cards, C = pods.max_containers;
  PAS_HIP(ctx, hipMemsetAsync(d_ctr, 0, sizeof(PlaceCtr), s));
  PAS_HIP(ctx, hipMemsetAsync(d_blocker, 0, 8 * N, s));
  if (d_cards_out) PAS_HIP(ctx, hipMemsetAsync(d_cards_out, 0, P * PAS_GAS_MAX_SELECTIONS, s));
  if (d_counts_out && C > 0)
    PAS_HIP(ctx, hipMemsetAsync(d_counts_out, 0, sizeof(int64_t) * P * (size_t)C * (size_t)K, s));
  if ((rc = derived_wait(ctx, g.derived_sync, s))) return rc;  // a fit's build reads `used`

  PlaceArgs a{n_pods, k, ld, g.n_nodes, node_base, (int32_t)pod_bits, d_cand, d_cand_len,
              d_cursor, d_blocker, d_keys, d_ctr, d_place_node, d_place_rank};
  BindArgs b{};
  b.K = K, b.Q = g.n_res, b.C = C, b.i915 = i915_index;
  b.n_cards = g.n_cards, b.cap = g.cap, b.used = g.used;
  b.req = pods.req, b.mask = pods.mask, b.ncont = pods.n_containers;
  b.res_out = d_res, b.cards_out = d_cards_out, b.nsel_out = d_nsel_out;
  b.counts_out = C > 0 ? d_counts_out : nullptr;
  const unsigned pod_blocks = (unsigned)((P + kPodTpb - 1) / kPodTpb);
  place_init_kernel<<<pod_blocks, kPodTpb, 0, s>>>(a, d_res, d_nsel_out);
  PAS_HIP(ctx, hipGetLastError());
  PAS_HIP(ctx, hipMemcpyAsync(h, d_ctr, sizeof(PlaceCtr), hipMemcpyDeviceToHost, s));
  PAS_HIP(ctx, hipStreamSynchronize(s));
  uint32_t active = h->active;
  // every round moves a cursor, and the cursors move sum(row lengths) times at most
  const uint64_t cap = std::min<uint64_t>((uint64_t)h->total_len + 1, 0xfffffffeull);
  uint64_t round = 0;
  a.keys = d_sorted;  // the commit reads the sorted keys; the mark writes d_keys
  while (active > 0) {
    if (round >= cap || active > (uint32_t)n_pods)
      return set_error(ctx, PAS_EDEVICE, "pas_gas_place: round bound exceeded");
    ++round;
    PlaceArgs am = a;
    am.keys = d_keys;
    place_mark_kernel<<<pod_blocks, kPodTpb, 0, s>>>(am, (uint32_t)round);
    PAS_HIP(ctx, hipGetLastError());
    size_t need = 0;
    PAS_HIP(ctx, rocprim::radix_sort_keys(nullptr, need, d_keys, d_sorted, (size_t)active, 0u,
                                          end_bit, s));
    if (need > sort_bytes)
      return set_error(ctx, PAS_EDEVICE, "pas_gas_place: sort storage grew with fewer keys");
    need = sort_bytes;
    PAS_HIP(ctx, rocprim::radix_sort_keys(d_sort_tmp, need, d_keys, d_sorted, (size_t)active,
                                          0u, end_bit, s));
    *began = true;
    card_tier(K, [&](auto km) {
      place_commit_kernel<decltype(km)::value><<<active, kTpb, 0, s>>>(a, b, (uint32_t)round,
                                                                       active);
    });
    PAS_HIP(ctx, hipGetLastError());
    PAS_HIP(ctx, hipMemcpyAsync(h, d_ctr, sizeof(PlaceCtr), hipMemcpyDeviceToHost, s));
    PAS_HIP(ctx, hipStreamSynchronize(s));
    const uint32_t fin = h->finished[round & 1];
    if (fin > active || h->n_keys[round & 1] != active)
      return set_error(ctx, PAS_EDEVICE, "pas_gas_place: inconsistent round counts");
    active -= fin;
  }
  if (n_placed) *n_placed = (int32_t)h->placed;
  if (n_rounds) *n_rounds = (int32_t)std::min<uint64_t>(round, INT32_MAX);
  return PAS_OK;
}

}  // namespace pas
