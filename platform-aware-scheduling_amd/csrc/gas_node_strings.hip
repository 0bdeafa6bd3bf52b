// gas_node_strings.hip — node events from label and allocatable strings, parsed and resolved on
// the device: the node-side twin of gas_annotations.hip.
//
// A node event of the informer is the node, its "gpu.intel.com/cards" label and one allocatable
// literal per resource kind.  getNodeGPUList splits the label on "."
// (gpu-aware-scheduling/pkg/gpuscheduler/scheduler.go:132-148), getPerGPUResourceCapacity takes
// AsInt64 of every allocatable and divides it by the number of pieces (:150-178,
// resource_map.go:129-145), and the usage is kept by card name (node_resource_cache.go:64,
// 259-272).  pas_gas_nodes_update takes that event already worked out into a card count,
// capacities and a slot map; here the strings are the input:
//   1. node_strings_parse    one lane per update: the rules that need no card name (a state or a
//                            slot out of range, a literal ParseQuantity rejects), the pieces, the
//                            distinct count up to PAS_GAS_MAX_CARDS + 1 (label_fixed.h), the
//                            capacities (quantity_fixed.h), and the largest distinct count of the
//                            pending updates, reduced per wave (one lane issues the atomic);
//   2. NodeRuns + node_strings_rounds   the position of every pending update in its node's run
//                            (call order) and the longest run;
//   3. node_strings_resolve  for the updates at run position r: each label card, in rank order,
//                            against the K names of the node's row of the card-name table (the
//                            length first, then the bytes), the old slots the label does not
//                            list parked behind them, and the new row's byte total;
//   4. the call's read-back: the largest distinct count (PAS_ECAPACITY before anything changed),
//                            the longest run, and the rows' byte totals (the pool's room and the
//                            table's host accounting);
//   5. scan, node_strings_names, node_strings_commit   the new rows' names appended to the
//                            table's pool (label names from the call's blob, parked names from
//                            their old place) and the rows' spans pointed there;
//   6. gas_nodes_update_launch   the row walker, exactly as pas_gas_nodes_update runs it; the
//                            updates that are settled or wait for a later position go to it with
//                            node N, which it answers with PAS_GAS_ERR_INPUT and no change;
//   7. node_strings_status   the updates' own statuses.
// Steps 3-6 run once per run position, so several updates of one node see each other in call
// order; a batch without a repeated node is one round and one synchronize, and every further
// round reads its rows' byte totals back again.
//
// A lane per update, not a wave: a label's pieces are not bounded by 64 (10 000 copies of one
// name are one card), so a lane-per-piece layout would need a second path for long labels, and
// the cold start this is for has tens of thousands of updates, which fill the device with
// lanes.  The labels are adjacent in one blob, so neighbouring lanes read neighbouring bytes.
// No kernel uses LDS or a per-lane array: the state of a walk is two spans and a few counters,
// and a row's spans are read from memory per compare.  The atomics are on the workspace only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "card_rows.h"
#include "gas_group.h"
#include "host_staging.h"
#include "label_fixed.h"
#include "pas_internal.h"
#include "quantity_fixed.h"
#include "span_pool.h"

namespace pas {
namespace {

constexpr int kTpb = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTpb - 1) / kTpb); }

constexpr int32_t kPending = PAS_GAS_ANN_PENDING;  // (-1: no status has that value)

// Rules 1-4 of pas_gas_nodes_update_strings for update u.  names.off non-null: node[u] is the
// slot the name table gave the update's node name (-1 without one).
__global__ __launch_bounds__(kTpb) void node_strings_parse(
    int32_t U, int32_t N, int32_t Q, const int32_t* __restrict__ node, ByteSpans names,
    const int32_t* __restrict__ state, ByteSpans label, ByteSpans lit,
    int32_t* __restrict__ verdict, int32_t* __restrict__ n_cards, int32_t* __restrict__ gpu_count,
    int64_t* __restrict__ cap, int32_t* most) {
  const int32_t u = blockIdx.x * kTpb + threadIdx.x;
  int32_t pending = 0;  // this lane's distinct count if its update is pending
  if (u < U) {
    const int32_t st = state[u], n = node[u];
    const bool held = n >= 0 && n < N;
    int32_t v = kPending, nc = 0, gpus = 0;
    if (st != PAS_GAS_NODE_GONE && st != PAS_GAS_NODE_NO_LABEL && st != PAS_GAS_NODE_LABEL) {
      v = PAS_GAS_ERR_INPUT;
    } else if (names.off) {
      int64_t nb;
      if (names.span(u, &nb) == 0)
        v = PAS_GAS_ERR_INPUT;
      else if (!held)  // a node the snapshot never held leaves without a trace
        v = st == PAS_GAS_NODE_GONE ? PAS_GAS_OK : PAS_GAS_ERR_INPUT;
    } else if (!held) {
      v = PAS_GAS_ERR_INPUT;
    }
    int64_t* cap_u = cap + (int64_t)u * Q;
    for (int32_t q = 0; q < Q; ++q) cap_u[q] = 0;
    if (st == PAS_GAS_NODE_GONE && v != PAS_GAS_ERR_INPUT) nc = -1;
    if (v == kPending && st == PAS_GAS_NODE_LABEL) {
      int64_t b;
      const int64_t len = label.span(u, &b);
      const int64_t pieces = label_pieces(label.bytes + b, len);
      gpus = sat32(pieces);
      nc = label_count(label.bytes + b, len, PAS_GAS_MAX_CARDS + 1);
      for (int32_t q = 0; q < Q; ++q) {
        int64_t lb;
        const int64_t ll = lit.span((int64_t)u * Q + q, &lb);
        if (ll == 0) continue;  // a resource the node does not have
        const QuantityFixed r = parse_quantity_fixed(lit.bytes + lb, ll);
        if (r.status == PAS_EINVAL) v = PAS_GAS_ERR_INPUT;
        cap_u[q] = r.as_int64 / pieces;  // resourceMap.divide: truncates toward zero
      }
      if (v != kPending) {
        nc = 0;
        gpus = 0;
        for (int32_t q = 0; q < Q; ++q) cap_u[q] = 0;
      } else {
        pending = nc;
      }
    }
    verdict[u] = v;
    n_cards[u] = nc;
    gpu_count[u] = gpus;
  }
  if (!most) return;  // (uniform)
  wave_max(pending, most);
}

// round[u] = the position of update u in its node's run (-1: settled), *longest = the longest run
__global__ __launch_bounds__(kTpb) void node_strings_rounds(int32_t U, int32_t N,
                                                            const uint32_t* __restrict__ key,
                                                            const int32_t* __restrict__ order,
                                                            int32_t* __restrict__ round,
                                                            int32_t* longest) {
  const int32_t pos = blockIdx.x * kTpb + threadIdx.x;
  int32_t mine = 0;
  if (pos < U) {
    const uint32_t kp = key[pos];
    int32_t c = -1;
    if (kp < (uint32_t)N) {
      c = 0;
      while (pos - c - 1 >= 0 && key[pos - c - 1] == kp) ++c;
      mine = c + 1;
    }
    round[order[pos]] = c;
  }
  wave_max(mine, longest);
}

// Rule 5 for the pending updates at run position r (r < 0: every pending update, the resolve
// form): the slot map src [U][K], the parked cards lost, the new row's bytes (-1: the update
// writes no names: its row stays) and the node handed to the walker (N: not this round).
// n_cards_res is the resident count: the old label range.
__global__ __launch_bounds__(kTpb) void node_strings_resolve(
    int32_t U, int32_t N, int32_t r, const int32_t* __restrict__ node,
    const int32_t* __restrict__ verdict, const int32_t* __restrict__ round,
    const int32_t* __restrict__ n_cards, const int32_t* __restrict__ n_cards_res, CardView t,
    ByteSpans label, int32_t* __restrict__ src, int32_t* __restrict__ n_dropped,
    int64_t* __restrict__ row_bytes, int64_t* __restrict__ scan_in,
    int32_t* __restrict__ walker_node) {
  const int32_t u = blockIdx.x * kTpb + threadIdx.x;
  if (u > U) return;
  if (u == U) {
    if (scan_in) scan_in[U] = 0;  // the scan's last element: the total
    return;
  }
  const int32_t K = t.k;
  const bool pending = verdict[u] == kPending;
  const bool take = pending && (r < 0 || round[u] == r);
  if (walker_node) walker_node[u] = take ? node[u] : N;
  if (row_bytes) row_bytes[u] = -1;
  if (scan_in) scan_in[u] = 0;
  int32_t* src_u = src + (int64_t)u * K;
  if (!take) {
    if (r <= 0 && n_dropped) n_dropped[u] = 0;
    if (r < 0)  // the resolve form's settled updates: a defined row
      for (int32_t k = 0; k < K; ++k) src_u[k] = -1;
    return;
  }
  const int32_t nc = n_cards[u];
  if (n_dropped) n_dropped[u] = 0;
  if (nc <= 0) {  // gone or without a label: the row stays where it is
    for (int32_t k = 0; k < K; ++k) src_u[k] = k;
    return;
  }
  if (nc > K) {  // PAS_ECAPACITY: the host returns before anything is applied
    for (int32_t k = 0; k < K; ++k) src_u[k] = -1;
    return;
  }
  const int32_t n = node[u];
  const int64_t row = (int64_t)n * K;
  const int32_t l_old = max(0, min(n_cards_res[n], K));
  int64_t lb;
  const int64_t ll = label.span(u, &lb);
  const char* p = label.bytes + lb;
  int64_t bytes = 0, b = 0, l = 0;
  for (int32_t i = 0; i < nc; ++i) {  // the label cards in rank order
    label_next(p, ll, i > 0, b, l, &b, &l);
    src_u[i] = row_find(t, row, t.k, p + b, l);
    bytes += l;
  }
  int32_t at = nc, dropped = 0;
  for (int32_t j = 0; j < K; ++j) {  // the old slots the label does not list, in slot order
    const int64_t lj = t.len[row + j];
    if (lj == 0 && j >= l_old) continue;  // an unused slot
    if (label_lists(p, ll, t.pool + t.beg[row + j], lj)) continue;
    if (at < K) {
      src_u[at++] = j;
      bytes += lj;
    } else {
      ++dropped;
    }
  }
  for (int32_t k = at; k < K; ++k) src_u[k] = -1;
  if (n_dropped) n_dropped[u] = dropped;
  if (row_bytes) row_bytes[u] = bytes;
  if (scan_in) scan_in[u] = bytes;
}

// The new rows' names at pool[base + row_off[u] ..) and their spans into new_beg / new_len
// [U][K]; nothing is written at or past pool_cap (the host sized the pool from the read-back).
__global__ __launch_bounds__(kTpb) void node_strings_names(
    int32_t U, const int32_t* __restrict__ node, const int32_t* __restrict__ n_cards,
    const int64_t* __restrict__ row_bytes, const int64_t* __restrict__ row_off,
    const int32_t* __restrict__ src, CardView t, char* __restrict__ pool, int64_t base,
    int64_t pool_cap, ByteSpans label, int64_t* __restrict__ new_beg,
    int64_t* __restrict__ new_len) {
  const int32_t u = blockIdx.x * kTpb + threadIdx.x;
  if (u >= U || row_bytes[u] < 0) return;
  const int32_t K = t.k, nc = n_cards[u];
  const int64_t row = (int64_t)node[u] * K;
  int64_t lb;
  const int64_t ll = label.span(u, &lb);
  const char* p = label.bytes + lb;
  int64_t cur = base + row_off[u], b = 0, l = 0;
  int64_t* nb = new_beg + (int64_t)u * K;
  int64_t* nl = new_len + (int64_t)u * K;
  for (int32_t i = 0; i < nc; ++i) {
    label_next(p, ll, i > 0, b, l, &b, &l);
    nb[i] = cur;
    nl[i] = l;
    if (cur + l <= pool_cap)
      for (int64_t x = 0; x < l; ++x) pool[cur + x] = p[b + x];
    cur += l;
  }
  for (int32_t k = nc; k < K; ++k) {
    const int32_t j = src[(int64_t)u * K + k];
    const int64_t lj = j >= 0 ? t.len[row + j] : 0;
    nb[k] = cur;
    nl[k] = lj;
    if (lj > 0 && cur + lj <= pool_cap) {
      const char* q = t.pool + t.beg[row + j];
      for (int64_t x = 0; x < lj; ++x) pool[cur + x] = q[x];
    }
    cur += lj;
  }
}

// The rows' spans pointed at the new names (one lane per entry; a node is in a round once)
__global__ __launch_bounds__(kTpb) void node_strings_commit(
    int64_t n, int32_t K, const int32_t* __restrict__ node, const int64_t* __restrict__ row_bytes,
    const int64_t* __restrict__ new_beg, const int64_t* __restrict__ new_len,
    int64_t* __restrict__ beg, int64_t* __restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n) return;
  const int64_t u = i / K;
  if (row_bytes[u] < 0) return;
  const int64_t at = (int64_t)node[u] * K + i % K;
  beg[at] = new_beg[i];
  len[at] = new_len[i];
}

__global__ __launch_bounds__(kTpb) void node_strings_status(int32_t U,
                                                            const int32_t* __restrict__ verdict,
                                                            int32_t* __restrict__ status) {
  const int32_t u = blockIdx.x * kTpb + threadIdx.x;
  if (u < U) status[u] = verdict[u] == kPending ? PAS_GAS_OK : verdict[u];
}

// the call's arrays on the device
struct NodeStrings {
  int32_t U;
  const int32_t* node;  // null: the nodes by name
  ByteSpans names;
  const int32_t* state;
  ByteSpans label, lit;
  int32_t *status, *n_cards, *gpu_count;  // outputs: any but status may be null
  int64_t* cap;
  int32_t *src, *n_dropped;
};

int d2d(pas_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (dst && bytes) PAS_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
  return PAS_OK;
}

// What the two launches share: the workspace's per-update arrays and the parse pass.
struct Stage {
  int32_t *scal, *verdict, *slot, *n_cards, *gpu_count, *round, *n_dropped, *walker, *wstatus;
  int32_t* src;
  int64_t *cap, *row_bytes, *scan_in, *row_off, *new_beg, *new_len;
  void* scan_tmp;
  size_t scan_bytes;
};

int stage_parse(pas_ctx* ctx, AuxSlot* slot, const NodeStrings& a, bool update, Stage* w,
                const int32_t** d_node, hipStream_t s) {
  const GasSnapshot& g = ctx->gas;
  const size_t U = (size_t)a.U, K = (size_t)g.max_cards, Q = (size_t)g.n_res;
  int rc = PAS_OK;
  w->scan_bytes = 0;
  if (update && (rc = scan_size<int64_t>(ctx, U + 1, &w->scan_bytes))) return rc;
  const size_t uk = update ? U * K : 0, u1 = update ? U : 0;
  const size_t bytes = carve_size({16, 4 * U, 4 * U, 4 * U, 4 * U, 4 * u1, 4 * U, 4 * u1, 4 * u1,
                                   4 * U * K, 8 * U * Q, 8 * u1, 8 * (u1 + 1), 8 * (u1 + 1),
                                   8 * uk, 8 * uk, w->scan_bytes});
  char* base = static_cast<char*>(slot_buf(ctx, slot, kBufNodeStrings, bytes, s, &rc));
  if (!base) return rc;
  Carve cv{base};
  w->scal = cv.take<int32_t>(4);
  w->verdict = cv.take<int32_t>(U);
  w->slot = cv.take<int32_t>(U);
  w->n_cards = cv.take<int32_t>(U);
  w->gpu_count = cv.take<int32_t>(U);
  w->round = cv.take<int32_t>(u1);
  w->n_dropped = cv.take<int32_t>(U);
  w->walker = cv.take<int32_t>(u1);
  w->wstatus = cv.take<int32_t>(u1);
  w->src = cv.take<int32_t>(U * K);
  w->cap = cv.take<int64_t>(U * Q);
  w->row_bytes = cv.take<int64_t>(u1);
  w->scan_in = cv.take<int64_t>(u1 + 1);
  w->row_off = cv.take<int64_t>(u1 + 1);
  w->new_beg = cv.take<int64_t>(uk);
  w->new_len = cv.take<int64_t>(uk);
  w->scan_tmp = cv.take<char>(w->scan_bytes);
  ByteSpans names{};
  *d_node = a.node;
  if (!a.node) {  // the nodes by name: lookup only, into the slot's buffer
    rc = names_resolve_launch(ctx, a.U, a.names, w->slot, nullptr, nullptr, false, s);
    if (rc) return rc;
    *d_node = w->slot;
    names = a.names;
  }
  PAS_HIP(ctx, hipMemsetAsync(w->scal, 0, 16, s));
  node_strings_parse<<<blocks_for(a.U), kTpb, 0, s>>>(
      a.U, g.n_nodes, g.n_res, *d_node, names, a.state, a.label, a.lit, w->verdict, w->n_cards,
      w->gpu_count, w->cap, w->scal);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

int resolve_launch(pas_ctx* ctx, const NodeStrings& a, hipStream_t s) {
  if (a.U == 0) return PAS_OK;
  const GasSnapshot& g = ctx->gas;
  const size_t U = (size_t)a.U, Q = (size_t)g.n_res;
  int rc = PAS_OK;
  SlotScope scope(ctx, s, 0, &rc);
  if (!scope.slot) return rc;
  Stage w;
  const int32_t* d_node;
  if ((rc = stage_parse(ctx, scope.slot, a, false, &w, &d_node, s))) return rc;
  node_strings_resolve<<<blocks_for(a.U + 1), kTpb, 0, s>>>(
      a.U, g.n_nodes, -1, d_node, w.verdict, nullptr, w.n_cards, g.n_cards,
      view_of(ctx->gas_cards), a.label, a.src ? a.src : w.src, w.n_dropped, nullptr, nullptr,
      nullptr);
  PAS_HIP(ctx, hipGetLastError());
  node_strings_status<<<blocks_for(a.U), kTpb, 0, s>>>(a.U, w.verdict, a.status);
  PAS_HIP(ctx, hipGetLastError());
  if ((rc = d2d(ctx, a.n_cards, w.n_cards, 4 * U, s))) return rc;
  if ((rc = d2d(ctx, a.gpu_count, w.gpu_count, 4 * U, s))) return rc;
  if ((rc = d2d(ctx, a.cap, w.cap, 8 * U * Q, s))) return rc;
  return d2d(ctx, a.n_dropped, w.n_dropped, 4 * U, s);
}

// pas_gas_nodes_update_strings[_names][_device] on device arrays.  *began: the resident arrays
// have been written (an error past that point leaves them half written).
int update_launch(pas_ctx* ctx, const NodeStrings& a, int32_t* need_cards, bool* began,
                  hipStream_t s, const std::string& fn) {
  *began = false;
  if (need_cards) *need_cards = 0;
  if (a.U == 0) return PAS_OK;
  GasSnapshot& g = ctx->gas;
  GasCardNames& t = ctx->gas_cards;
  const int32_t N = g.n_nodes, K = g.max_cards;
  const size_t U = (size_t)a.U, Q = (size_t)g.n_res;
  int rc = PAS_OK;
  SlotScope scope(ctx, s, 0, &rc);
  if (!scope.slot) return rc;
  Stage w;
  const int32_t* d_node;
  if ((rc = stage_parse(ctx, scope.slot, a, true, &w, &d_node, s))) return rc;
  {
    const int32_t* verdict = w.verdict;
    NodeRuns runs(ctx, a.U, d_node, [=] __device__(int32_t u) { return verdict[u] == kPending; },
                  s);
    if (runs.rc) return runs.rc;
    node_strings_rounds<<<blocks_for(a.U), kTpb, 0, s>>>(a.U, N, runs.key, runs.order, w.round,
                                                         w.scal + 1);
    PAS_HIP(ctx, hipGetLastError());
  }
  std::vector<int32_t> h_node(U);
  std::vector<int64_t> h_bytes(U);
  int32_t scal[2] = {0, 0};  // the largest distinct count, the longest run
  for (int32_t r = 0; r == 0 || r < scal[1]; ++r) {
    node_strings_resolve<<<blocks_for(a.U + 1), kTpb, 0, s>>>(
        a.U, N, r, d_node, w.verdict, w.round, w.n_cards, g.n_cards, view_of(t), a.label, w.src,
        w.n_dropped, w.row_bytes, w.scan_in, w.walker);
    PAS_HIP(ctx, hipGetLastError());
    if ((rc = scan_run<int64_t>(ctx, w.scan_tmp, w.scan_bytes, w.scan_in, w.row_off, U + 1, s)))
      return rc;
    // the read-back (round 0: the call's one synchronize before anything resident is written)
    if (r == 0)
      PAS_HIP(ctx, hipMemcpyAsync(scal, w.scal, sizeof scal, hipMemcpyDeviceToHost, s));
    PAS_HIP(ctx, hipMemcpyAsync(h_node.data(), w.walker, 4 * U, hipMemcpyDeviceToHost, s));
    PAS_HIP(ctx, hipMemcpyAsync(h_bytes.data(), w.row_bytes, 8 * U, hipMemcpyDeviceToHost, s));
    PAS_HIP(ctx, hipStreamSynchronize(s));
    if (r == 0) {
      if (need_cards) *need_cards = scal[0];
      if (scal[0] > K)
        return set_error(ctx, PAS_ECAPACITY,
                         fn + ": a label lists " + (scal[0] > PAS_GAS_MAX_CARDS ? "more than " : "") +
                             std::to_string(std::min<int32_t>(scal[0], PAS_GAS_MAX_CARDS)) +
                             " cards, max_cards is " + std::to_string(K));
    }
    int64_t total = 0;
    for (size_t u = 0; u < U; ++u)
      if (h_bytes[u] > 0) total += h_bytes[u];
    if ((rc = grow_pool(ctx, t.sp, total, s, "card-name table: pool copy"))) return rc;
    // nothing has changed so far; from here the table and the snapshot do
    *began = true;
    node_strings_names<<<blocks_for(a.U), kTpb, 0, s>>>(
        a.U, d_node, w.n_cards, w.row_bytes, w.row_off, w.src, view_of(t), t.sp.pool,
        t.sp.pool_used, t.sp.pool_cap, a.label, w.new_beg, w.new_len);
    PAS_HIP(ctx, hipGetLastError());
    node_strings_commit<<<blocks_for((int64_t)U * K), kTpb, 0, s>>>(
        (int64_t)U * K, K, d_node, w.row_bytes, w.new_beg, w.new_len, t.sp.beg, t.sp.len);
    PAS_HIP(ctx, hipGetLastError());
    t.sp.pool_used += total;
    for (size_t u = 0; u < U; ++u) {
      if (h_bytes[u] < 0) continue;
      t.sp.live_bytes += h_bytes[u] - t.row_bytes[h_node[u]];
      t.row_bytes[h_node[u]] = h_bytes[u];
    }
    if ((rc = gas_nodes_update_launch(ctx, a.U, w.walker, w.n_cards, w.cap, w.src, w.wstatus, s)))
      return rc;
    if ((rc = d2d(ctx, a.n_dropped, w.n_dropped, 4 * U, s))) return rc;
  }
  node_strings_status<<<blocks_for(a.U), kTpb, 0, s>>>(a.U, w.verdict, a.status);
  PAS_HIP(ctx, hipGetLastError());
  if ((rc = d2d(ctx, a.n_cards, w.n_cards, 4 * U, s))) return rc;
  if ((rc = d2d(ctx, a.cap, w.cap, 8 * U * Q, s))) return rc;
  return card_names_gather_dead(ctx, s, fn);
}

const char* const kNoSnap = "no GAS snapshot uploaded";

// The snapshot, the tables and the scalars and pointers of either form (gen null: the resolve
// forms, which check no generation)
int strings_check(pas_ctx* ctx, bool by_name, const uint64_t* gen_from, int32_t n_updates,
                  const void* node, const void* name_off, const void* state, const void* label_off,
                  const void* cap_off, const void* status_out, const std::string& fn) {
  if (!ctx->gas.valid) return set_error(ctx, PAS_ENOSNAP, kNoSnap);
  if (gen_from && ctx->gas.gen != *gen_from)
    return set_error(ctx, PAS_ESTALE, "GAS snapshot generation mismatch");
  const GasCardNames& t = ctx->gas_cards;
  if (!t.valid) return set_error(ctx, PAS_ENOSNAP, fn + ": no card-name table");
  if (by_name && !ctx->names.valid) return set_error(ctx, PAS_ENOSNAP, fn + ": no name table");
  if (t.n_slots != ctx->gas.n_nodes || t.k != ctx->gas.max_cards)
    return set_error(ctx, PAS_EINVAL,
                     fn + ": the card-name table is " + std::to_string(t.n_slots) + " x " +
                         std::to_string(t.k) + ", the GAS snapshot " +
                         std::to_string(ctx->gas.n_nodes) + " x " +
                         std::to_string(ctx->gas.max_cards));
  if (n_updates < 0) return set_error(ctx, PAS_EINVAL, fn + ": bad shape");
  if (n_updates > 0 &&
      (!(by_name ? name_off : node) || !state || !label_off || !cap_off || !status_out))
    return set_error(ctx, PAS_EINVAL, fn + ": null input");
  return PAS_OK;
}

int update_device(pas_ctx* ctx, bool by_name, uint64_t gen_from, uint64_t gen_to, NodeStrings a,
                  int32_t* need_cards, void* hip_stream, const std::string& fn) {
  if (!ctx) return PAS_EINVAL;
  int rc = strings_check(ctx, by_name, &gen_from, a.U, a.node, a.names.off, a.state, a.label.off,
                         a.lit.off, a.status, fn);
  if (rc) return rc;
  if (a.U > 0 && ((rc = check_device_spans(ctx, a.U, a.label, fn + ": label_off")) ||
                  (rc = check_device_spans(ctx, a.U, a.lit, fn + ": cap_off")) ||
                  (by_name &&
                   (rc = check_device_spans(ctx, a.U, a.names, fn + ": node_name_off")))))
    return rc;
  if ((rc = activate(ctx))) return rc;
  bool began = false;
  rc = update_launch(ctx, a, need_cards, &began, pick_stream(ctx, hip_stream), fn);
  return gas_finish(ctx, rc, began, gen_to, true);
}

struct HostArgs {
  int32_t n_updates;
  const int32_t* node;
  const int64_t* name_off;
  const char* name_bytes;
  const int32_t* state;
  const int64_t* label_off;
  const char* label_bytes;
  const int64_t* cap_off;
  const char* cap_bytes;
  int32_t *status, *n_cards, *gpu_count;
  int64_t* cap;
  int32_t *src, *n_dropped;
};

// The host forms: validate, upload, run the _device forms' path, wait and copy the outputs back.
int strings_host(pas_ctx* ctx, bool by_name, bool update, uint64_t gen_from, uint64_t gen_to,
                 const HostArgs& h, int32_t* need_cards, const std::string& fn) {
  if (!ctx) return PAS_EINVAL;
  int rc = strings_check(ctx, by_name, update ? &gen_from : nullptr, h.n_updates, h.node,
                         h.name_off, h.state, h.label_off, h.cap_off, h.status, fn);
  if (rc) return rc;
  if (need_cards) *need_cards = 0;
  if (h.n_updates == 0) return update ? gas_finish(ctx, PAS_OK, false, gen_to, true) : PAS_OK;
  const GasSnapshot& g = ctx->gas;
  const size_t U = (size_t)h.n_updates, K = (size_t)g.max_cards, Q = (size_t)g.n_res;
  if ((rc = check_host_spans(ctx, h.n_updates, h.label_off, h.label_bytes, fn + ": label_off")) ||
      (rc = check_host_spans(ctx, (int64_t)(U * Q), h.cap_off, h.cap_bytes, fn + ": cap_off")) ||
      (by_name && (rc = check_host_spans(ctx, h.n_updates, h.name_off, h.name_bytes,
                                         fn + ": node_name_off"))))
    return rc;
  for (size_t u = 0; u < U; ++u) {
    if (!by_name && (h.node[u] < 0 || h.node[u] >= g.n_nodes))
      return set_error(ctx, PAS_EINVAL, fn + ": node index out of range");
    if (h.state[u] < PAS_GAS_NODE_GONE || h.state[u] > PAS_GAS_NODE_LABEL)
      return set_error(ctx, PAS_EINVAL, fn + ": state outside {-1, 0, 1}");
  }
  if ((rc = activate(ctx))) return rc;
  Staging st(ctx);
  NodeStrings a{};
  a.U = h.n_updates;
  if (by_name)
    st.in_spans(a.names, h.n_updates, h.name_off, h.name_bytes);
  else
    st.in(a.node, h.node, U);
  st.in(a.state, h.state, U);
  st.in_spans(a.label, h.n_updates, h.label_off, h.label_bytes);
  st.in_spans(a.lit, (int64_t)(U * Q), h.cap_off, h.cap_bytes);
  st.out(a.status, h.status, U);
  st.out_opt(a.n_cards, h.n_cards, U);
  st.out_opt(a.gpu_count, h.gpu_count, U);
  st.out_opt(a.cap, h.cap, U * Q);
  st.out_opt(a.src, h.src, U * K);
  st.out_opt(a.n_dropped, h.n_dropped, U);
  if ((rc = st.upload())) return rc;
  if (!update) {
    if ((rc = resolve_launch(ctx, a, ctx->stream))) return rc;
    PAS_HIP(ctx, st.fetch());
    return PAS_OK;
  }
  bool began = false;
  rc = update_launch(ctx, a, need_cards, &began, ctx->stream, fn);
  if (!rc && st.fetch() != hipSuccess) {
    began = true;
    rc = set_error(ctx, PAS_EDEVICE, fn + ": copy of the results");
  }
  return gas_finish(ctx, rc, began, gen_to, true);
}

}  // namespace
}  // namespace pas

using namespace pas;

extern "C" {

int pas_gas_nodes_update_strings(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                 int32_t n_updates, const int32_t* upd_node,
                                 const int32_t* upd_state, const int64_t* label_off,
                                 const char* label_bytes, const int64_t* cap_off,
                                 const char* cap_bytes, int32_t* status_out, int32_t* n_cards_out,
                                 int64_t* cap_out, int32_t* n_dropped_out, int32_t* need_cards) {
  const HostArgs h{n_updates, upd_node, nullptr, nullptr, upd_state, label_off, label_bytes,
                   cap_off, cap_bytes, status_out, n_cards_out, nullptr, cap_out, nullptr,
                   n_dropped_out};
  return strings_host(ctx, false, true, gen_from, gen_to, h, need_cards,
                      "pas_gas_nodes_update_strings");
}

int pas_gas_nodes_update_strings_names(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                       int32_t n_updates, const int64_t* node_name_off,
                                       const char* node_name_bytes, const int32_t* upd_state,
                                       const int64_t* label_off, const char* label_bytes,
                                       const int64_t* cap_off, const char* cap_bytes,
                                       int32_t* status_out, int32_t* n_cards_out,
                                       int64_t* cap_out, int32_t* n_dropped_out,
                                       int32_t* need_cards) {
  const HostArgs h{n_updates, nullptr, node_name_off, node_name_bytes, upd_state, label_off,
                   label_bytes, cap_off, cap_bytes, status_out, n_cards_out, nullptr, cap_out,
                   nullptr, n_dropped_out};
  return strings_host(ctx, true, true, gen_from, gen_to, h, need_cards,
                      "pas_gas_nodes_update_strings_names");
}

int pas_gas_nodes_resolve_strings(pas_ctx* ctx, int32_t n_updates, const int32_t* upd_node,
                                  const int32_t* upd_state, const int64_t* label_off,
                                  const char* label_bytes, const int64_t* cap_off,
                                  const char* cap_bytes, int32_t* status_out,
                                  int32_t* n_cards_out, int32_t* gpu_count_out, int64_t* cap_out,
                                  int32_t* src_out, int32_t* n_dropped_out) {
  const HostArgs h{n_updates, upd_node, nullptr, nullptr, upd_state, label_off, label_bytes,
                   cap_off, cap_bytes, status_out, n_cards_out, gpu_count_out, cap_out, src_out,
                   n_dropped_out};
  return strings_host(ctx, false, false, 0, 0, h, nullptr, "pas_gas_nodes_resolve_strings");
}

int pas_gas_nodes_update_strings_device(
    pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_updates,
    const int32_t* d_upd_node, const int32_t* d_upd_state, int64_t n_label_bytes,
    const int64_t* d_label_off, const char* d_label_bytes, int64_t n_cap_bytes,
    const int64_t* d_cap_off, const char* d_cap_bytes, int32_t* d_status_out,
    int32_t* d_n_cards_out, int64_t* d_cap_out, int32_t* d_n_dropped_out, int32_t* need_cards,
    void* hip_stream) {
  NodeStrings a{n_updates, d_upd_node, ByteSpans{}, d_upd_state,
                ByteSpans{n_label_bytes, d_label_off, d_label_bytes},
                ByteSpans{n_cap_bytes, d_cap_off, d_cap_bytes}, d_status_out, d_n_cards_out,
                nullptr, d_cap_out, nullptr, d_n_dropped_out};
  return update_device(ctx, false, gen_from, gen_to, a, need_cards, hip_stream,
                       "pas_gas_nodes_update_strings_device");
}

int pas_gas_nodes_update_strings_names_device(
    pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_updates, int64_t n_name_bytes,
    const int64_t* d_node_name_off, const char* d_node_name_bytes, const int32_t* d_upd_state,
    int64_t n_label_bytes, const int64_t* d_label_off, const char* d_label_bytes,
    int64_t n_cap_bytes, const int64_t* d_cap_off, const char* d_cap_bytes,
    int32_t* d_status_out, int32_t* d_n_cards_out, int64_t* d_cap_out, int32_t* d_n_dropped_out,
    int32_t* need_cards, void* hip_stream) {
  NodeStrings a{n_updates, nullptr, ByteSpans{n_name_bytes, d_node_name_off, d_node_name_bytes},
                d_upd_state, ByteSpans{n_label_bytes, d_label_off, d_label_bytes},
                ByteSpans{n_cap_bytes, d_cap_off, d_cap_bytes}, d_status_out, d_n_cards_out,
                nullptr, d_cap_out, nullptr, d_n_dropped_out};
  return update_device(ctx, true, gen_from, gen_to, a, need_cards, hip_stream,
                       "pas_gas_nodes_update_strings_names_device");
}

int pas_gas_nodes_resolve_strings_device(
    pas_ctx* ctx, int32_t n_updates, const int32_t* d_upd_node, const int32_t* d_upd_state,
    int64_t n_label_bytes, const int64_t* d_label_off, const char* d_label_bytes,
    int64_t n_cap_bytes, const int64_t* d_cap_off, const char* d_cap_bytes,
    int32_t* d_status_out, int32_t* d_n_cards_out, int32_t* d_gpu_count_out, int64_t* d_cap_out,
    int32_t* d_src_out, int32_t* d_n_dropped_out, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_nodes_resolve_strings_device";
  NodeStrings a{n_updates, d_upd_node, ByteSpans{}, d_upd_state,
                ByteSpans{n_label_bytes, d_label_off, d_label_bytes},
                ByteSpans{n_cap_bytes, d_cap_off, d_cap_bytes}, d_status_out, d_n_cards_out,
                d_gpu_count_out, d_cap_out, d_src_out, d_n_dropped_out};
  int rc = strings_check(ctx, false, nullptr, n_updates, d_upd_node, nullptr, d_upd_state,
                         d_label_off, d_cap_off, d_status_out, fn);
  if (rc) return rc;
  if (n_updates > 0 && ((rc = check_device_spans(ctx, n_updates, a.label, fn + ": label_off")) ||
                        (rc = check_device_spans(ctx, n_updates, a.lit, fn + ": cap_off"))))
    return rc;
  if ((rc = activate(ctx))) return rc;
  return resolve_launch(ctx, a, pick_stream(ctx, hip_stream));
}

}  // extern "C"
