// tas_request_batch.hip — the TAS verbs for a batch of extender requests in request terms.
//
// pas_tas_prioritize_requests: request r's list is exactly pas_tas_prioritize_request's
// (tas_request.hip: first occurrences that have the metric, keyed rank << pb | position,
// sorted).  A request of up to kReqCap positions is one workgroup's work and never leaves
// LDS:
//
//   1. first occurrences: an open-addressing table of the request's nodes in LDS (2 * kReqCap
//      slots: CAS claims a slot for a node, atomicMin keeps the node's lowest position), so
//      a node listed twice keeps the lower position wherever the two lie, and two requests
//      of a batch that list the same node never see each other (no first[R][N] table)
//   2. key[j] = rank << 11 | j for first occurrences that have the metric (rank from the
//      column's sorted row, tas_rank.h), all ones for every other position and the padding
//   3. bitonic sort of the keys in LDS (workgroup barriers only around the steps that cross
//      a wave's 128 keys); positions, the -1 tail and the length are written
//
// Longer requests go through prio_request_launch on the same stream, one after the other,
// each writing at its CSR offset (the host knows the lengths: req_off is a host array).
//
// pas_tas_filter_requests: one lane per request position.  A workgroup resolves its
// request's dontschedule rules once into LDS (the value range a rule hits, as the deschedule
// sweep of tas_eval.hip does), every lane gathers its node's values from the metric-major
// columns, and a wave packs its 64 verdicts with one ballot and stores the word once.  Rows
// start word-aligned, so a wave never shares a word with another request.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "pas_internal.h"
#include "request_batch.h"
#include "tas_rank.h"

namespace pas {
namespace {

// ----------------------------------------------------------------------- prioritize

constexpr int kPrioTpb = 512;
constexpr int kPosBits = 11;
constexpr int kReqCap = 1 << kPosBits;  // S: positions of a request one workgroup sorts
constexpr int kSlots = 2 * kReqCap;     // node table slots (load factor <= 1/2)
static_assert(kReqCap == kRequestCap, "request_batch.h states the cap");

// Request r of the batch as the kernel reads it (built on the host from req_off / prio).
struct PrioDesc {
  int32_t off, n;      // CSR span
  int32_t metric, op;  // prio[r]
  int32_t wide;        // the metric's column is wide
  int32_t pad[3];
};

struct PrioArgs {
  int32_t N, row;
  const PrioDesc* desc;
  const int32_t* req;
  const int64_t* vals;
  const uint64_t* present;
  const int32_t* cnt;
  const int64_t* sorted;
  const uint32_t* nano;
  const uint32_t* sorted_nano;
  int32_t* pos;
  int32_t* len;
};

__global__ __launch_bounds__(kPrioTpb) void prio_requests_kernel(PrioArgs a) {
  __shared__ uint64_t keys[kReqCap];   // 16 KiB
  __shared__ int32_t t_node[kSlots];   // 16 KiB
  __shared__ int32_t t_first[kSlots];  // 16 KiB
  __shared__ int32_t kept;
  const int32_t r = blockIdx.x, tid = threadIdx.x;
  const PrioDesc d = a.desc[r];
  const int32_t n = d.n;
  if (n > kReqCap) return;  // the host runs it through the single-request path
  if (n <= 0) {
    if (tid == 0) a.len[r] = 0;
    return;
  }
  const int32_t* __restrict__ rq = a.req + d.off;
  int32_t* __restrict__ out = a.pos + d.off;
  if (d.metric < 0) {  // no scheduling rule / metric not cached: the empty list
    for (int32_t j = tid; j < n; j += kPrioTpb) out[j] = -1;
    if (tid == 0) a.len[r] = 0;
    return;
  }
  int32_t P = 1;  // the sort's size: n rounded up to a power of two
  while (P < n) P <<= 1;
  for (int32_t i = tid; i < kSlots; i += kPrioTpb) {
    t_node[i] = -1;
    t_first[i] = INT32_MAX;
  }
  if (tid == 0) kept = 0;
  __syncthreads();
  // 1. every known node claims a slot; the slot keeps the node's lowest position
  for (int32_t j = tid; j < n; j += kPrioTpb) {
    const int32_t node = rq[j];
    if (node < 0 || node >= a.N) continue;
    uint32_t h = ((uint32_t)node * 2654435761u) >> (32 - kPosBits - 1);
    for (;;) {
      const int32_t old = atomicCAS(&t_node[h], -1, node);
      if (old == -1 || old == node) break;
      h = (h + 1) & (kSlots - 1);
    }
    atomicMin(&t_first[h], j);
    keys[j] = h;  // this thread reads it back below
  }
  __syncthreads();
  // 2. keys
  const int64_t W = ((int64_t)a.N + 63) >> 6;
  const int64_t mrow = (int64_t)d.metric * a.row, mcol = (int64_t)d.metric * a.N;
  for (int32_t j = tid; j < P; j += kPrioTpb) {
    uint64_t key = ~0ull;
    bool keep = false;
    if (j < n) {
      const int32_t node = rq[j];
      if (node >= 0 && node < a.N && t_first[(uint32_t)keys[j]] == j) {
        const uint64_t word = a.present[(int64_t)d.metric * W + (node >> 6)];
        if ((word >> (node & 63)) & 1ull) {
          keep = true;
          uint64_t rank = 0;
          if (d.op == PAS_OP_LESS_THAN || d.op == PAS_OP_GREATER_THAN) {
            const int64_t v = a.vals[mcol + node];
            const int32_t c = a.cnt[d.metric];
            const int64_t* row = a.sorted + mrow;
            const bool up = d.op == PAS_OP_GREATER_THAN;
            int32_t b;
            if (d.wide) b = bound<true>(row, a.sorted_nano + mrow, c, v, a.nano[mcol + node], up);
            else b = bound<false>(row, nullptr, c, v, 0u, up);
            rank = (uint64_t)(up ? c - b : b);
          }
          key = rank << kPosBits | (uint64_t)j;
        }
      }
    }
    keys[j] = key;
    // one LDS atomic per wave (the active lanes are a prefix of the wave: lane 0 is in it)
    const uint64_t ballot = __ballot(keep);
    if ((tid & 63) == 0 && ballot) atomicAdd(&kept, (int32_t)__popcll(ballot));
  }
  __syncthreads();
  // 3. bitonic sort, ascending: the all-ones keys end up last
  for (int32_t k = 2; k <= P; k <<= 1) {
    for (int32_t j = k >> 1; j > 0; j >>= 1) {
      for (int32_t t = tid; t < (P >> 1); t += kPrioTpb) {
        const int32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t x = keys[i], y = keys[l];
        if ((x > y) == ((i & k) == 0)) {
          keys[i] = y;
          keys[l] = x;
        }
      }
      // A wave's 64 consecutive pairs of a step with j <= 64 lie in one aligned block of 128
      // keys, the same block in every such step: those steps exchange between the lanes of
      // one wave, in program order through the LDS, and need no workgroup barrier.  Only a
      // step with j >= 128 reads what other waves wrote (and writes what they read next).
      const int32_t nj = j > 1 ? j >> 1 : (k < P ? k : INT32_MAX);  // the next step's (or the end)
      if (j >= 128 || nj >= 128) __syncthreads();
      else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
  }
  const int32_t m = kept;
  for (int32_t i = tid; i < n; i += kPrioTpb)
    out[i] = i < m ? (int32_t)(keys[i] & (uint64_t)(kReqCap - 1)) : -1;
  if (tid == 0) a.len[r] = m;
}

// ----------------------------------------------------------------------- filter

constexpr int kFiltTpb = 256;
constexpr int kRuleTile = 64;  // rules resolved into LDS at a time

// A dontschedule rule as the lanes evaluate it.  kind 0: never evaluated (metric not cached,
// unknown operator); 1: narrow column, violates iff lo <= v <= hi; 2 + op: wide column,
// the pair against the integer target lo.
struct FiltRule {
  int32_t metric, kind;
  int64_t lo, hi;
};

struct FiltArgs {
  int32_t N, M, n_rules, has_wide;
  const int32_t* req_off;  // device copy of the host's
  const int32_t* req;
  const pas_rule* rules;
  const int32_t* rule_off;
  const int64_t* vals;
  const uint64_t* present;
  const uint32_t* nano;
  const uint8_t* wide_flag;
  const int64_t* scale_tab;
  uint64_t* out;
  int64_t ld;
};

__global__ __launch_bounds__(kFiltTpb) void filter_requests_kernel(FiltArgs a) {
  __shared__ FiltRule tile[kRuleTile];
  const int32_t r = blockIdx.x, tid = threadIdx.x;
  const int32_t off = a.req_off[r], n = a.req_off[r + 1] - off;
  // the rule span clamped into [0, n_rules] and non-decreasing, as tas_eval.hip's rule_span:
  // a device rule_off that is not a CSR never indexes past the rules
  const int32_t r0 = min(max(a.rule_off[r], 0), a.n_rules);
  const int32_t r1 = min(max(a.rule_off[r + 1], r0), a.n_rules);
  const int64_t W = ((int64_t)a.N + 63) >> 6;
  uint64_t* __restrict__ row = a.out + (int64_t)r * a.ld;
  const int32_t words = (int32_t)(((int64_t)n + 63) >> 6);
  for (int64_t base = (int64_t)blockIdx.y * kFiltTpb; base < (int64_t)words * 64;
       base += (int64_t)gridDim.y * kFiltTpb) {
    const int64_t j = base + tid;  // past n in the last word's tail, and past the words
    int32_t node = -1;
    if (j < n) node = a.req[off + j];
    const bool known = node >= 0 && node < a.N;
    bool viol = false;
    for (int32_t t0 = r0; t0 < r1; t0 += kRuleTile) {
      const int32_t nt = min(kRuleTile, r1 - t0);
      __syncthreads();  // the previous tile's readers
      if (tid < nt) {
        const pas_rule ru = a.rules[t0 + tid];
        FiltRule f{ru.metric, 0, 1, 0};
        if (ru.metric >= 0 && ru.metric < a.M && ru.op >= 0 && ru.op <= 2) {
          if (a.has_wide && a.wide_flag[ru.metric]) {
            f.kind = 2 + ru.op;
            f.lo = ru.target;
          } else {
            f.kind = 1;
            int64_t tm = 0;
            const int sat = target_scaled(ru.target, a.scale_tab, ru.metric, &tm);
            if (ru.op == PAS_OP_LESS_THAN) {  // v < t
              if (sat > 0) f.lo = INT64_MIN, f.hi = INT64_MAX;
              else if (sat == 0 && tm != INT64_MIN) f.lo = INT64_MIN, f.hi = tm - 1;
            } else if (ru.op == PAS_OP_GREATER_THAN) {  // v > t
              if (sat < 0) f.lo = INT64_MIN, f.hi = INT64_MAX;
              else if (sat == 0 && tm != INT64_MAX) f.lo = tm + 1, f.hi = INT64_MAX;
            } else if (sat == 0) {  // v == t
              f.lo = f.hi = tm;
            }
          }
        }
        tile[tid] = f;
      }
      __syncthreads();
      if (!known) continue;
      for (int32_t t = 0; t < nt; ++t) {
        const FiltRule f = tile[t];
        if (f.kind == 0) continue;
        const uint64_t word = a.present[(int64_t)f.metric * W + (node >> 6)];
        if (!((word >> (node & 63)) & 1ull)) continue;  // the node lacks the metric
        const int64_t v = a.vals[(int64_t)f.metric * a.N + node];
        if (f.kind == 1) {
          viol |= v >= f.lo && v <= f.hi;
        } else {
          const uint32_t fr = a.nano[(int64_t)f.metric * a.N + node];
          const int32_t op = f.kind - 2;
          viol |= op == PAS_OP_LESS_THAN      ? wide_below(v, fr, f.lo)
                  : op == PAS_OP_GREATER_THAN ? wide_above(v, fr, f.lo)
                                              : wide_equal(v, fr, f.lo);
        }
      }
    }
    // an unknown node is in no violating set: it passes (dontschedule/strategy.go:25-44)
    const uint64_t bits = __ballot(j < n && !(known && viol));
    if ((tid & 63) == 0 && (j >> 6) < words) row[j >> 6] = bits;  // the request's words only
  }
}

}  // namespace

int upload_host(pas_ctx* ctx, void* dst, const void* src, size_t bytes, bool wait,
                hipStream_t s) {
  PAS_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
  if (wait) PAS_HIP(ctx, hipStreamSynchronize(s));
  return PAS_OK;
}

int32_t request_longest(int32_t n_requests, const int32_t* req_off) {
  int32_t longest = 0;
  for (int32_t r = 0; r < n_requests; ++r) longest = std::max(longest, req_off[r + 1] - req_off[r]);
  return longest;
}

unsigned request_chunks(int32_t longest, int tpb) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>(((int64_t)longest + tpb - 1) / tpb, 1),
                                     65535);
}

int prio_requests_launch(pas_ctx* ctx, int32_t n_requests, const int32_t* req_off,
                         const pas_rule* prio, const int32_t* d_req, int32_t* d_pos,
                         int32_t* d_len, HostStage* stage, hipStream_t s) {
  const TasSnapshot& t = ctx->tas;
  // the descriptors' host copy: the caller's stage when it keeps one until it has synchronized
  HostStage local;
  std::vector<char>& bytes = (stage ? stage : &local)->bytes;
  bytes.resize(sizeof(PrioDesc) * (size_t)n_requests);
  PrioDesc* desc = reinterpret_cast<PrioDesc*>(bytes.data());
  size_t ws_long = 0;
  int32_t n_short = 0;
  for (int32_t r = 0; r < n_requests; ++r) {
    PrioDesc& d = desc[(size_t)r];
    d = PrioDesc{};
    d.off = req_off[r], d.n = req_off[r + 1] - req_off[r];
    d.metric = prio[r].metric, d.op = prio[r].op;
    d.wide = d.metric >= 0 && t.n_wide > 0 && t.wide_host[(size_t)d.metric];
    if (d.n > kReqCap) {
      size_t ws = 0;
      int rc = prio_request_workspace(ctx, d.n, &ws);
      if (rc) return rc;
      ws_long = std::max(ws_long, ws);
    } else {
      ++n_short;
    }
  }
  int rc = PAS_OK;
  const size_t b_desc = bytes.size();
  SlotScope sc(ctx, s, carve_size({b_desc, ws_long}), &rc);
  if (!sc.slot) return rc;
  Carve cv{static_cast<char*>(sc.slot->p)};
  PrioDesc* d_desc = cv.take<PrioDesc>((size_t)n_requests);
  void* d_ws = cv.take<char>(ws_long);
  if (n_short) {
    if ((rc = upload_host(ctx, d_desc, desc, b_desc, !stage, s))) return rc;
    PrioArgs a{t.n_nodes, t.row,  d_desc, d_req,         t.vals, t.present,
               t.cnt,     t.sorted, t.nano, t.sorted_nano, d_pos,  d_len};
    prio_requests_kernel<<<(unsigned)n_requests, kPrioTpb, 0, s>>>(a);
    PAS_HIP(ctx, hipGetLastError());
  }
  for (int32_t r = 0; r < n_requests; ++r) {
    const PrioDesc& d = desc[(size_t)r];
    if (d.n <= kReqCap) continue;
    if ((rc = prio_request_launch(ctx, prio[r], d.n, d_req + d.off, d_pos + d.off, d_len + r,
                                  d_ws, ws_long, s)))
      return rc;
  }
  return PAS_OK;
}

int filter_requests_launch(pas_ctx* ctx, int32_t n_requests, const int32_t* req_off,
                           int32_t n_rules, const pas_rule* d_rules, const int32_t* d_rule_off,
                           const int32_t* d_req, uint64_t* d_pass, int64_t ld_words,
                           HostStage* stage, hipStream_t s) {
  const int32_t longest = request_longest(n_requests, req_off);
  if (longest == 0) return PAS_OK;  // no row has a word
  const TasSnapshot& t = ctx->tas;
  int rc = PAS_OK;
  const size_t b_off = sizeof(int32_t) * ((size_t)n_requests + 1);
  SlotScope sc(ctx, s, carve_size({b_off}), &rc);
  if (!sc.slot) return rc;
  int32_t* d_off = static_cast<int32_t*>(sc.slot->p);
  if ((rc = upload_host(ctx, d_off, req_off, b_off, !stage, s))) return rc;
  FiltArgs a{t.n_nodes, t.n_metrics, n_rules, t.n_wide > 0, d_off, d_req, d_rules, d_rule_off,
             t.vals, t.present, t.nano, t.wide_flag, t.scale_tab, d_pass, ld_words};
  filter_requests_kernel<<<dim3((unsigned)n_requests, request_chunks(longest, kFiltTpb)),
                           kFiltTpb, 0, s>>>(a);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

}  // namespace pas
