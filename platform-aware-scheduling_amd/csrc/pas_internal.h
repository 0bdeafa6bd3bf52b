// pas_internal.h — context and snapshot state shared by the HIP translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "csr_entry.h"
#include "pas.h"

namespace pas {

constexpr int kOrderAsc = 0;   // LessThan   (operator.go:38-39)
constexpr int kOrderDesc = 1;  // GreaterThan (operator.go:36-37)
constexpr int kOrderIndex = 2; // any other operator: no sort
constexpr int kNumOrders = 3;

inline int64_t w64(int64_t n) { return (n + 63) / 64; }
inline int64_t w32(int64_t n) { return (n + 31) / 32; }

// Order rows are padded to whole 1024-position segments plus one more segment, filled with
// a sentinel node id (see TasSnapshot), so that a segment load never needs a bound check.
constexpr int kOrderPad = 1024;
inline int64_t order_row(int64_t n) { return (n + kOrderPad - 1) / kOrderPad * kOrderPad + kOrderPad; }

// Data a call derives from the resident snapshot on its own stream (once per snapshot
// change) and later calls read, possibly on other streams: an event recorded after the build
// orders those calls after it (derived_wait).
struct DerivedSync {
  hipEvent_t ev = nullptr;
  hipStream_t stream = nullptr;
  bool valid = false;
};

// Device-resident TAS snapshot.  Layout in HBM (M metrics, N nodes, R = order_row(N)):
//   vals     int64 [M][N]      raw v_milli (deschedule sweep reads it directly)
//   present  uint64 [M][W64]   (vals and present have room for one column when M = 0)
//   cnt      int32 [M]         nodes that have metric m
//   sorted   int64 [M][R]      ascending values of the present nodes (first cnt[m])
//   perm     int32 [3][M][R]   node ids in asc / desc / index order (first cnt[m]); the
//                              rest of each row holds the sentinel W64 * 64, a node id
//                              whose bit in the evaluator's LDS pass bitmap is always 0
//   f1k, f32 int64 [M][R/1024], [M][R/32]  every 1024th / 32nd sorted value (rule ranges
//                              are found in three coalesced rounds: tas_eval.hip)
struct TasSnapshot {
  bool valid = false;
  uint64_t gen = 0;
  int32_t n_nodes = 0;
  int32_t n_metrics = 0;
  int32_t row = 0;  // R
  int64_t* vals = nullptr;
  uint64_t* present = nullptr;
  int32_t* cnt = nullptr;
  int64_t* sorted = nullptr;
  int32_t* perm = nullptr;
  int64_t* f1k = nullptr;  // [M][R / 1024] sorted[m][1024 a]: fences of the range search
  int64_t* f32 = nullptr;  // [M][R / 32]   sorted[m][32 b]
  // column m holds value * 10^scale[m]: scale_tab[m] = {10^scale, INT64_MAX / 10^scale}
  // (pas_tas_snapshot_set_scale; milli after every snapshot_set)
  int64_t* scale_tab = nullptr;
  std::vector<int64_t> scale_host;  // the same table on the host (set_scale keeps wide columns')
  // Wide columns (pas_tas_snapshot_update_wide): the value of node n is vals[m][n] +
  // nano[m][n] * 1e-9 (vals holds the floor), sorted[m] / f1k / f32 hold the floors in the
  // exact pair order and sorted_nano / f1k_nano / f32_nano the nanos at the same positions.
  // Allocated by the first wide update (all null before); wide_flag [M] on the device and
  // wide_host mark the wide columns, n_wide counts them.  scale_tab keeps a wide column's
  // recorded scale (the wide compares do not read it).
  int32_t n_wide = 0;
  std::vector<uint8_t> wide_host;
  uint8_t* wide_flag = nullptr;
  uint32_t* nano = nullptr;         // [M][N]
  uint32_t* sorted_nano = nullptr;  // [M][R]
  uint32_t* f1k_nano = nullptr;     // [M][R / 1024]
  uint32_t* f32_nano = nullptr;     // [M][R / 32]
  void* wide_sort_tmp = nullptr;    // temp storage of the wide (128-bit key) sort
  size_t wide_sort_tmp_bytes = 0;
  // build scratch (kept for column updates): sort keys {value, row} and node ids, two
  // buffers each, [M][R]; per-word popcounts and their scan; the updated rows
  void* keys_a = nullptr;
  void* keys_b = nullptr;
  int32_t* ids_a = nullptr;
  int32_t* ids_b = nullptr;
  uint32_t* popc = nullptr;        // [M*W64 + 1]
  uint32_t* word_scan = nullptr;   // [M*W64 + 1]
  int32_t* rows = nullptr;         // [M]
  void* sort_tmp = nullptr;
  size_t sort_tmp_bytes = 0;
  void* scan_tmp = nullptr;
  size_t scan_tmp_bytes = 0;
  // node-major copies for per-node gathers (tas_gas_topk.hip), built by the first call that
  // needs them after a change: vals_t int64 [N][M], pres_t uint64 [N][ceil(M / 64)].
  // `epoch` counts snapshot changes, `t_epoch` is the epoch the copies were built at.
  uint64_t epoch = 1;
  uint64_t t_epoch = 0;
  int64_t* vals_t = nullptr;
  uint64_t* pres_t = nullptr;
  size_t vals_t_bytes = 0;  // the two allocations' sizes
  size_t pres_t_bytes = 0;
  DerivedSync t_sync;  // the copies' build
};

// Word w of a presence row of N nodes without the bits at and past N (an upload may carry
// them in the last word).
__host__ __device__ __forceinline__ uint64_t word_mask(uint64_t bits, int64_t w, int32_t N) {
  const int64_t lo = w * 64;
  return lo + 64 > N ? bits & ((N - lo) >= 64 ? ~0ull : ((1ull << (N - lo)) - 1)) : bits;
}

// Device-resident GAS snapshot (node-major):
//   n_cards int32 [N], cap int64 [N][Q], used int64 [N][K][Q]
// core.EvaluateRule's CmpInt64 (operator.go:16-22) against column m's fixed point: the
// integer target * 10^scale[m] in *tm (0), or the saturation when that is past int64: +1 above
// every value, -1 below every value.  A column at scale 0 never saturates:
// every int64 is a valid value there (-2^63 included), so the target is compared as it is,
// and a caller that forms tm - 1 or tm + 1 guards tm == INT64_MIN / INT64_MAX itself.
__device__ __forceinline__ int target_scaled(int64_t t, const int64_t* __restrict__ scale_tab,
                                             int32_t m, int64_t* tm) {
  const int64_t mult = scale_tab[2 * m], maxq = scale_tab[2 * m + 1];
  if (mult == 1) {
    *tm = t;
    return 0;
  }
  if (t > maxq) return 1;
  if (t < -maxq) return -1;
  *tm = t * mult;
  return 0;
}

// The same compares for a wide column's pair (value = whole + nano * 1e-9, whole the floor,
// nano < 1e9) against the integer target t, exact in 64-bit arithmetic.  "Above" is
// ceil(value) > t without forming ceil = whole + (nano != 0), which a pair (2^63 - 1,
// nano != 0) would overflow; the target is compared as it is (no scale, no saturation), so
// whole = -2^63 is ordinary too.
__device__ __forceinline__ bool wide_below(int64_t whole, uint32_t, int64_t t) {
  return whole < t;
}
__device__ __forceinline__ bool wide_equal(int64_t whole, uint32_t nano, int64_t t) {
  return whole == t && nano == 0u;
}
__device__ __forceinline__ bool wide_not_above(int64_t whole, uint32_t nano, int64_t t) {
  return whole < t || wide_equal(whole, nano, t);
}
__device__ __forceinline__ bool wide_above(int64_t whole, uint32_t nano, int64_t t) {
  return whole > t || (whole == t && nano != 0u);
}
// A pair against the pair (v, f), in the columns' order: whole signed, then nano unsigned.
__device__ __forceinline__ bool pair_below(int64_t whole, uint32_t nano, int64_t v, uint32_t f) {
  return whole < v || (whole == v && nano < f);
}
__device__ __forceinline__ bool pair_not_above(int64_t whole, uint32_t nano, int64_t v,
                                               uint32_t f) {
  return whole < v || (whole == v && nano <= f);
}

// The canonical pair (W, F) of a narrow column's value v held at multiplier mult = 10^s,
// s = 0..9 (scale_tab[2m]): v * 10^-s = W + F * 1e-9 with W the floor (toward -inf) and
// 0 <= F < 1e9, the unit of the wide merge records (pas.h).  Exact: the remainder is below
// 10^9 and 10^(9-s) scales it below 10^9.
__host__ __device__ __forceinline__ void canonical_pair(int64_t v, int64_t mult, int64_t* W,
                                                        uint32_t* F) {
  int64_t q = v / mult, r = v - q * mult;
  if (r < 0) {
    q -= 1;
    r += mult;
  }
  *W = q;
  *F = (uint32_t)r * (1000000000u / (uint32_t)mult);
}
// The wide merge record (key, sub) of the pair under the prioritize operator: ascending
// (key signed, sub unsigned) is the HostPriorityList order (~ reverses both fields).
__host__ __device__ __forceinline__ void wide_order_key(int32_t op, int64_t W, uint32_t F,
                                                        int64_t* key, uint32_t* sub) {
  *key = op == PAS_OP_GREATER_THAN ? ~W : op == PAS_OP_LESS_THAN ? W : 0;
  *sub = op == PAS_OP_GREATER_THAN ? ~F : op == PAS_OP_LESS_THAN ? F : 0u;
}

struct GasSnapshot {
  bool valid = false;
  uint64_t gen = 0;
  int32_t n_nodes = 0;
  int32_t max_cards = 0;
  int32_t n_res = 0;
  int32_t* n_cards = nullptr;
  int64_t* cap = nullptr;
  int64_t* used = nullptr;
  // per-snapshot values the fit derives (gas_fit.hip: flipped kind minima, nodes past the
  // fast kernels' card count), recomputed by the first fit after a change: `epoch` counts
  // changes of n_cards / cap / used, `derived_epoch` is the epoch they were computed at
  uint64_t epoch = 1;
  uint64_t derived_epoch = 0;
  void* derived = nullptr;  // gflip[4] u64 | n_big_nodes i32 (+pad) | big_nodes[N] i32
  // card-major free values of the first 8 cards, free_t[k][q][n] (gas_fit.hip), derived
  // with the above: the fit kernels' per-node loads are then coalesced
  void* free_t = nullptr;
  DerivedSync derived_sync;  // the derived values' build
};

// The resident TASPolicy table (pas_tas_policies_set, tas_policy.hip): the policies' rules as
// the reference's cache holds the TASPolicy objects (cache.ReadPolicy), on the host (the host
// forms' validation, pas_tas_policies_info) and on the device (one allocation: rules |
// rule_off | prio).  `col_epoch` is the context's column epoch at the set: a later change of
// the snapshot's column numbering makes the table stale.  `serial` counts the sets.
// Derived: viol [n_policies][W64], the policies' dontschedule violating sets
// (dontschedule/strategy.go:25-44 depends on the rules and the metric cache only), built by
// the first policy verb after the snapshot's content or the table changed, on that verb's
// stream; later verbs on other streams wait for viol_sync's event.  The table lives beside
// the snapshot struct, not in it: reshape and compact build a new struct and swap it in.
struct TasPolicies {
  bool valid = false;
  int32_t n_policies = 0;
  int32_t n_rules = 0;
  uint64_t serial = 0;
  uint64_t col_epoch = 0;
  std::vector<pas_rule> rules;     // [n_rules]
  std::vector<int32_t> rule_off;   // [n_policies + 1]
  std::vector<pas_rule> prio;      // [n_policies]
  void* dev = nullptr;
  size_t dev_bytes = 0;
  pas_rule* d_rules = nullptr;
  int32_t* d_rule_off = nullptr;
  pas_rule* d_prio = nullptr;
  uint64_t* viol = nullptr;
  size_t viol_bytes = 0;
  bool viol_built = false;  // viol holds the sets of (viol_epoch, viol_gen, viol_serial)
  uint64_t viol_epoch = 0;  // TasSnapshot::epoch
  uint64_t viol_gen = 0;
  uint64_t viol_serial = 0;
  DerivedSync viol_sync;
};

// Spans into one byte pool (span_pool.hip): the storage under the two resident name tables.
// Entry i is pool[beg[i] .. beg[i] + len[i]).  The span arrays hold span_cap + 1 entries (the
// scans' last element) and len is 0 from the table's entries on.  The pool only grows:
// pool_used counts every byte ever appended, live_bytes the bytes the spans still name (the
// sum of the lengths); a pool is packed by a scan of the lengths and one gather.
struct SpanPool {
  int64_t* beg = nullptr;
  int64_t* len = nullptr;
  int64_t span_cap = 0;
  char* pool = nullptr;
  int64_t pool_used = 0;
  int64_t pool_cap = 0;
  int64_t live_bytes = 0;
};

// The resident node-name table (name_table.hip): which name stands in which node slot, for
// every snapshot of the context (combined contexts share one slot numbering, so it belongs to
// neither).  Slot s is entry s of `sp`; len 0 marks a spare slot, so the empty name never has
// a slot.  The pool's order is the order of arrival, not of the slots, and no byte of it is
// ever dead (live_bytes = pool_used).  `table` is an open-addressing hash of the named slots,
// `buckets` a power of two >= 2 * n_slots: word = tag << 32 | slot (name_hash.h), all ones =
// empty, linear probing with wraparound; nothing is ever deleted in place (a remap rebuilds).
// Storage only grows.
struct NameTable {
  bool valid = false;
  int32_t n_slots = 0;
  int32_t n_named = 0;
  SpanPool sp;
  unsigned long long* table = nullptr;
  int64_t buckets = 0;
};

// The resident card-name table (gas_cards.hip): the names of the card slots of every node slot,
// beside the GAS snapshot struct and not in it (resize and compact replace that struct).  Row s
// holds k entries in the order of used[s][.]: the label cards in sort.Strings order, then what
// the caller keeps behind them (parked cards).  Entry (s, c) is entry s * k + c of `sp`; names
// are opaque bytes and the empty name is a name like any other.  A row rewrite appends the new
// bytes to the pool and leaves the old ones dead: sp.live_bytes is the sum of row_bytes, the
// rows' byte totals kept on the host.  When the dead bytes pass the live ones the pool is
// gathered.
struct GasCardNames {
  bool valid = false;
  int32_t n_slots = 0;
  int32_t k = 0;
  SpanPool sp;
  std::vector<int64_t> row_bytes;  // [n_slots]
  std::vector<uint32_t> stamp;     // [n_slots] the last update call that named the slot
  uint32_t stamp_clock = 0;
};

// slot_buf buffers
enum SlotBuf {
  kBufGpass = 0,  // pass bitmaps of clusters past the LDS bitmap (tas_eval)
  kBufMerge = 1,  // cut list and ping-pong rows of the full-list merge (tas_list_merge.hip)
  kBufLabel = 2,  // per-workgroup partial counts of the label plan (tas_labels.hip)
  kBufPlace = 3,  // cursors, keys, blockers and sort storage of a placement (gas_place.hip)
  // sort keys, item order and sort storage of a batch grouped by node (gas_group.h): one
  // buffer for pod events and node updates, since two calls on one slot are ordered (stream
  // order, or the slot's event), so a batch never finds the other's storage still in use
  kBufRuns = 4,
  // per-pod prio rules and the all-zero rule offsets of an evaluation by policy id, or the
  // request offsets and policy ids of a request filter by policy id (tas_policy.hip)
  kBufPolicy = 5,
  kBufPatch = 6,      // segment counts and violated pairs of a patch list (tas_patches.hip)
  kBufPatchViol = 7,  // the sweep's bitmaps of pas_tas_deschedule_patches without viol_out
  // parsed entries, per-column summary and plan, and the column buffers of a refresh from
  // Quantity literals (tas_ingest.hip)
  kBufIngest = 8,
  // resolved slots, hashes, the first-seen scratch table, scan inputs and outputs of a name
  // lookup or assignment (name_table.hip)
  kBufNames = 9,
  // the parsed annotations of a pod-event batch (gas_annotations.hip): cards per container
  // [E][max_containers] and card ranks [E][cards_ld], sized after the call's read-back
  kBufAnnot = 10,
  // the same batch's per-event words, sized before it: the largest pending list, verdicts,
  // listed counts, the nodes handed to the walker and the slots of the nodes given by name
  kBufAnnotEvents = 11,
  // the per-update words, slot maps, capacities, new spans and scan storage of a node-event batch
  // given as strings (gas_node_strings.hip)
  kBufNodeStrings = 12,
  // the per-span lengths and scan storage of a render (gas_render.hip), and the rendered bytes
  // of a host form, sized after the call's read-back
  kBufRender = 13,
  kBufRenderBytes = 14,
  kSlotBufs = 15
};

// Per-call device scratch of the _device entry points (TAS rule ranges and pod descriptors,
// GAS lists, rank rows and list counts), one set per stream in use.  A call takes the slot of
// its stream (stream order protects it), else a free slot, else the least recently used one
// after waiting (hipStreamWaitEvent) for that slot's last call: calls on different streams
// never share scratch while they may run, and calls on two alternating streams (a pipeline
// of batches) run without waiting for each other.
struct AuxSlot {
  void* p = nullptr;  // aux: TAS ranges | desc | keys, or the GAS fit's lists and rank rows
  size_t bytes = 0;
  hipStream_t stream = nullptr;
  bool used = false;      // stream / ev are valid
  hipEvent_t ev = nullptr;  // recorded on `stream` after the slot's last call
  uint64_t last = 0;      // use clock (LRU)
  // the GAS fit's list counts, two sets: a fit uses one (zero) and its prep kernel zeroes the
  // other for the next fit on this slot (no fill launch per fit)
  int32_t* gas_counts = nullptr;
  int gas_counts_set = 0;
  int64_t* gas_limit = nullptr;  // pods of the slot's last GAS fit past PAS_GAS_MAX_SELECTIONS
  // the GAS fit's side streams (one-selection + generic kernels; sequential kernel), forked
  // from and joined to the caller's stream per fit, and their events (events mode)
  hipStream_t side = nullptr, side2 = nullptr;
  hipEvent_t fork = nullptr, join = nullptr, join2 = nullptr;
  // device-side fork / join (gas_fit.hip): flags [prep done, side done, side2 done, abort,
  // prep started] each set to the fit's epoch (a per-slot count of fits); abort = the epoch of
  // a fit whose wait timed out (its fit kernels return at entry)
  uint32_t* gas_sync = nullptr;
  uint32_t gas_epoch = 0;
  // further per-stream buffers of the _device entry points (slot_buf), grown on demand
  void* buf[kSlotBufs] = {};
  size_t buf_bytes[kSlotBufs] = {};
};
constexpr int kAuxSlots = 4;

// Sub-buffers of one scratch allocation, each rounded up to 256 bytes: carve_size() of the
// sub-buffers' byte sizes is what take() of their element counts, in the same order, uses.
// For the _launch functions' AuxSlot and slot_buf storage (gas_fit.hip, gas_place.hip,
// gas_group.h, the *_requests launches); the host forms' arrays in ctx->scratch are stated
// once each to a Staging (host_staging.h), which sizes and lays them out itself.
struct Carve {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off += (count * sizeof(T) + 255) & ~size_t(255);
    return p;
  }
};
inline size_t carve_size(std::initializer_list<size_t> sizes) {
  size_t s = 0;
  for (size_t b : sizes) s += (b + 255) & ~size_t(255);
  return s;
}

struct TimedLaunch {
  hipEvent_t start;
  hipEvent_t stop;
  int32_t kernel;
};

}  // namespace pas

struct pas_ctx {
  int device = 0;
  int n_cu = 256;  // compute units of the device (persistent grids)
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  pas::TasSnapshot tas;
  pas::GasSnapshot gas;
  pas::TasPolicies policies;
  pas::NameTable names;
  pas::DerivedSync names_sync;  // the last change of `names`: lookups on other streams wait
  pas::GasCardNames gas_cards;  // (every change is synchronous: no event is needed)
  // counts the calls that can renumber or re-create the TAS snapshot's metric columns
  // (snapshot_set, reshape, drop): a policy table set at an older value is stale
  uint64_t tas_col_epoch = 1;
  // per-call scratch of the host-buffer entry points, which all run on ctx->stream and
  // synchronize it before they return (grown on demand; the _device entry points use the
  // per-stream AuxSlot buffers instead)
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  pas::AuxSlot aux_slot[pas::kAuxSlots];
  uint64_t aux_clock = 0;
  int gas_last_slot = -1;  // aux slot of the last GAS fit (pas_gas_limit_count)
  // the GAS fit's fork / join of its side streams: -1 unresolved, 0 events, 1 device flags
  // (gas_fit.hip gas_sync_mode), and the flags' sticky timeout report (host-pinned, written
  // by a wait kernel that gave up)
  int gas_sync_mode = -1;
  uint32_t* gas_sync_fault = nullptr;
  int gas_force_timeouts = 0;  // PAS_GAS_FORCE_TIMEOUT: the next n flag-mode fits time out
  void* place_host = nullptr;  // pas_gas_place: the round counts' read-back (host-pinned)
  // timing
  int timing = 0;  // 0 off, PAS_TIMING_SPAN, PAS_TIMING_KERNELS (pas_set_timing)
  std::vector<pas::TimedLaunch> pending;
  std::vector<hipEvent_t> event_pool;
  double total_ms[PAS_K_COUNT] = {};
  int64_t launches[PAS_K_COUNT] = {};
};

namespace pas {

int set_error(pas_ctx* ctx, int code, const std::string& msg);
int check_hip(pas_ctx* ctx, hipError_t e, const char* what);
#define PAS_HIP(ctx, expr)                                       \
  do {                                                           \
    hipError_t _e = (expr);                                      \
    if (_e != hipSuccess) return ::pas::check_hip(ctx, _e, #expr); \
  } while (0)

int ensure_scratch(pas_ctx* ctx, size_t bytes);
// After building snapshot-derived data on s / before reading it on s.
int derived_built(pas_ctx* ctx, DerivedSync& d, hipStream_t s);
int derived_wait(pas_ctx* ctx, const DerivedSync& d, hipStream_t s);
// The aux slot for a call on stream s with at least `bytes` of aux (ordered after the slot's
// previous user when that ran on another stream), and its release after the call's launches
// (records the slot's event on s).  nullptr on error (ctx->err set, *rc the status).
AuxSlot* aux_acquire(pas_ctx* ctx, hipStream_t s, size_t bytes, int* rc);
void aux_release(pas_ctx* ctx, AuxSlot* slot, hipStream_t s);
// Buffer `which` (SlotBuf) of an acquired slot, at least `bytes`: grown after the slot's
// earlier calls (ordered before s by aux_acquire) have finished.  nullptr on error (*rc).
void* slot_buf(pas_ctx* ctx, AuxSlot* slot, int which, size_t bytes, hipStream_t s, int* rc);
// aux_acquire + aux_release around a scope (every exit records the slot's event on s).
struct SlotScope {
  pas_ctx* ctx;
  AuxSlot* slot;
  hipStream_t s;
  SlotScope(pas_ctx* c, hipStream_t st, size_t bytes, int* rc)
      : ctx(c), slot(aux_acquire(c, st, bytes, rc)), s(st) {}
  ~SlotScope() {
    if (slot) aux_release(ctx, slot, s);
  }
  SlotScope(const SlotScope&) = delete;
  SlotScope& operator=(const SlotScope&) = delete;
};
int activate(pas_ctx* ctx);  // hipSetDevice(ctx->device)
hipStream_t pick_stream(pas_ctx* ctx, void* s);

// Checks of pas_api.hip that the entry points of other files share.  check_update: the TAS
// snapshot, its generation and the columns of a column update (distinct, below n_metrics).
// check_gas_gen: the GAS snapshot and its generation.  gas_pod_check: pod p of a host batch has
// n_containers[p] within [0, max_containers] and no mask bit at or above n_res.
int check_update(pas_ctx* ctx, uint64_t gen_from, int32_t n_cols, const int32_t* cols,
                 const void* vals, const void* present, const char* fn);
int check_gas_gen(pas_ctx* ctx, uint64_t gen);
int gas_pod_check(pas_ctx* ctx, int32_t p, int32_t max_containers, const uint32_t* req_mask,
                  const int32_t* n_containers, const char* fn);

// A GAS pod batch on the device: req [P][C][Q], mask [P][C], n_containers [P].  The host forms
// fill it through stage_pods (host_staging.h), the _device forms from their arguments; the
// pointers of a staged batch are valid at P == 0 or C == 0 too (nothing is copied then): the
// kernels read no request of a pod without containers.
struct PodBatch {
  int32_t n_pods;
  int32_t max_containers;
  const int64_t* req;
  const uint32_t* mask;
  const int32_t* n_containers;
};

// The end of a call that writes the resident GAS snapshot.  rc == PAS_OK: the generation steps
// to gen_to and the epoch advances.  Otherwise rc comes back as it is, and when the error came
// after the call's first resident write (`wrote`) the snapshot is of unknown content:
// ctx->gas.valid is cleared, and ctx->gas_cards.valid with it when the call writes that table
// too (`cards`).
int gas_finish(pas_ctx* ctx, int rc, bool wrote, uint64_t gen_to, bool cards = false);

// Bracket a launch with timing events when ctx->timing is on.
void timing_begin(pas_ctx* ctx, hipStream_t s, int kernel, TimedLaunch* tl);
void timing_end(pas_ctx* ctx, hipStream_t s, TimedLaunch* tl);

void free_tas(pas_ctx* ctx);
void free_gas(pas_ctx* ctx);
// The device storage of a TAS snapshot shape into t (tas_snapshot.hip): every array and the
// build scratch of n_nodes x n_metrics, content unset, t.n_nodes / n_metrics / row set; then
// the wide parts of that shape (wide_flag zeroed on s).  A failure leaves what it had
// allocated in t for tas_free_storage, which frees every array of t and nulls the pointers.
int tas_alloc(pas_ctx* ctx, TasSnapshot& t, int32_t n_nodes, int32_t n_metrics, hipStream_t s);
int tas_alloc_wide(pas_ctx* ctx, TasSnapshot& t, hipStream_t s);
void tas_free_storage(TasSnapshot& t);

// Per-translation-unit entry points used by the C-ABI layer.
int tas_snapshot_build(pas_ctx* ctx, uint64_t gen, int32_t n_nodes, int32_t n_metrics,
                       const int64_t* d_vals, const uint64_t* d_present, hipStream_t s);
// Replace metric columns cols[0..n_cols) (host array, distinct, < n_metrics) with
// d_vals [n_cols][N] / d_present [n_cols][W64] and rebuild their orders.
int tas_snapshot_update(pas_ctx* ctx, uint64_t gen, int32_t n_cols, const int32_t* cols,
                        const int64_t* d_vals, const uint64_t* d_present, hipStream_t s);
// The same with wide columns: d_whole [n_cols][N] (floors), d_nano [n_cols][N] (read clamped
// below 1e9), d_present [n_cols][W64]; the columns become wide.
int tas_snapshot_update_wide(pas_ctx* ctx, uint64_t gen, int32_t n_cols, const int32_t* cols,
                             const int64_t* d_whole, const uint32_t* d_nano,
                             const uint64_t* d_present, hipStream_t s);
// Both in one step: rows [0, n_narrow) of d_vals / d_present replace the columns cols_narrow
// as narrow columns, rows [n_narrow, n_narrow + n_wide) replace cols_wide as wide ones with
// the same rows of d_nano (the two column lists are host arrays, together distinct).  The
// snapshot is not valid between the two rebuilds; gen is published once, after both.
int tas_snapshot_update_mixed(pas_ctx* ctx, uint64_t gen, int32_t n_narrow,
                              const int32_t* cols_narrow, int32_t n_wide,
                              const int32_t* cols_wide, const int64_t* d_vals,
                              const uint32_t* d_nano, const uint64_t* d_present, hipStream_t s);
// free_pool (span_pool.hip): the span arrays and the pool of sp, which is empty afterwards.
void free_pool(SpanPool& sp);
// Name table (name_table.hip).  free_names: every array of the table (pas_destroy).
// names_resolve_launch: d_slot[i] = the slot of entry i of `names` (offsets read clamped into
// [0, n_bytes]) or -1, enqueued on s after the last table change; d_hash (the names' hashes) and
// d_unknown (a zeroed counter: + the entries without a slot, the empty ones only when
// count_empty) may be null.  The caller has checked ctx->names.valid.
void free_names(NameTable& t);
int names_resolve_launch(pas_ctx* ctx, int64_t n, ByteSpans names, int32_t* d_slot,
                         uint64_t* d_hash, uint32_t* d_unknown, bool count_empty, hipStream_t s);
// What the annotation forms share (pas_gas_annotations_resolve*, pas_gas_apply_annotations*,
// pas_gas_annotations_render*): the card-name table is there and has the resident snapshot's
// shape, and the name table is there when the nodes come by name.  The caller has checked the
// snapshot.
int gas_annotations_tables(pas_ctx* ctx, bool by_name, const std::string& fn);
// The card-name table's pool gathered on s when its dead bytes have passed the live ones
// (gas_cards.hip: the rule of pas_gas_card_names_update), for a caller that appended rows on the
// device and kept row_bytes / live_bytes / pool_used in step (gas_node_strings.hip).
int card_names_gather_dead(pas_ctx* ctx, hipStream_t s, const std::string& fn);
// The resident snapshot gathered into storage of n_nodes_new (>= the resident count) x
// n_metrics_new (tas_reshape.hip): new column m is old column src_col[m] or, for -1, empty
// (src_col: host [n_metrics_new], distinct old columns or -1; the caller has checked it and
// the new shape against the snapshot's size limit).  No sort runs.  Synchronous on s; the old storage is freed once s and the context's stream are
// idle.  An allocation failure leaves the resident snapshot as it was.
int tas_snapshot_reshape(pas_ctx* ctx, uint64_t gen, int32_t n_nodes_new, int32_t n_metrics_new,
                         const int32_t* src_col, hipStream_t s);
// The resident snapshot with its node slots renumbered into storage of n_nodes_new slots
// (tas_compact.hip): new slot j is old slot src_node[j] or, for -1, spare; an old slot no
// entry names is dropped from every column (src_node: host [n_nodes_new], its non-negative
// entries strictly increasing and below the resident count; the caller has checked it and the
// new shape against the size limit).  No sort runs.  Synchronous and failing as the reshape.
int tas_snapshot_compact(pas_ctx* ctx, uint64_t gen, int32_t n_nodes_new,
                         const int32_t* src_node, hipStream_t s);
int tas_eval_launch(pas_ctx* ctx, int32_t n_pods, int32_t n_rules, const pas_rule* d_rules,
                    const int32_t* d_rule_off, const pas_rule* d_prio, const uint64_t* d_cand,
                    uint32_t flags, uint64_t* d_pass, int32_t* d_order, int32_t* d_len,
                    int32_t topk, hipStream_t s);
// Single-request prioritize (tas_request.hip): workspace bytes for n_req positions, and the
// launch (rule is host-side; ws = that many device bytes).
int prio_request_workspace(pas_ctx* ctx, int32_t n_req, size_t* bytes);  // status
int prio_request_launch(pas_ctx* ctx, const pas_rule& rule, int32_t n_req, const int32_t* d_req,
                        int32_t* d_pos, int32_t* d_len, void* ws, size_t ws_bytes,
                        hipStream_t s);
// The verbs for a batch of requests in request terms (tas_request_batch.hip,
// gas_fit_requests.hip): req_off [R + 1] and prio [R] are host arrays (a valid CSR, the
// metrics below n_metrics), everything else is on the device; the workspace is the slot of s.
// Enqueued on s.  stage == nullptr (the _device forms): the launch waits for the copy of the
// host arrays, which are the caller's again on return.  Otherwise (the host forms, which
// synchronize s before they return) nothing waits: the caller keeps req_off and *stage, where
// the launch puts what it derives from the host arrays, until it has synchronized.
struct HostStage {
  std::vector<char> bytes;
};
int prio_requests_launch(pas_ctx* ctx, int32_t n_requests, const int32_t* req_off,
                         const pas_rule* prio, const int32_t* d_req, int32_t* d_pos,
                         int32_t* d_len, HostStage* stage, hipStream_t s);
int filter_requests_launch(pas_ctx* ctx, int32_t n_requests, const int32_t* req_off,
                           int32_t n_rules, const pas_rule* d_rules, const int32_t* d_rule_off,
                           const int32_t* d_req, uint64_t* d_pass, int64_t ld_words,
                           HostStage* stage, hipStream_t s);
int gas_fit_requests_launch(pas_ctx* ctx, int32_t n_requests, const int32_t* req_off,
                            const int32_t* d_req_node, int32_t i915_index, const PodBatch& pods,
                            uint64_t* d_fit, int64_t ld_words, HostStage* stage, hipStream_t s);
// (n_rules bounds the device rule_off: offsets are clamped into [0, n_rules], rule_span)
int tas_violations_launch(pas_ctx* ctx, int32_t n_strat, int32_t n_rules,
                          const pas_rule* d_rules, const int32_t* d_rule_off, uint64_t* d_viol,
                          hipStream_t s);
// The verbs by policy id (tas_policy.hip) over the resident table ctx->policies (valid and
// current: the caller has checked).  policies_viol: the table's violation bitmaps, built on s
// if the snapshot or the table changed since the last build, else s ordered after that build.
int policies_viol(pas_ctx* ctx, hipStream_t s, const uint64_t** d_viol);
// pas_tas_eval_policies on device arrays (d_pod_policy [n_pods], an id outside
// [0, n_policies) read as -1), enqueued on s.
int policy_eval_launch(pas_ctx* ctx, int32_t n_pods, const int32_t* d_pod_policy,
                       const uint64_t* d_cand, uint32_t flags, uint64_t* d_pass,
                       int32_t* d_order, int32_t* d_len, hipStream_t s);
// The pods' prio rules gathered out of the table ({-1, 0, 0} for id -1) and n_pods + 1 zero rule
// offsets, in buffer kBufPolicy of the acquired slot; enqueued on s.  d_off may be null.
int policy_prio_gather(pas_ctx* ctx, AuxSlot* slot, int32_t n_pods, const int32_t* d_pod_policy,
                       pas_rule** d_prio, int32_t** d_off, hipStream_t s);
// pas_tas_filter_requests_policies: req_off [R + 1] and req_policy [R] are host arrays, stage
// as for filter_requests_launch.
int filter_requests_policy_launch(pas_ctx* ctx, int32_t n_requests, const int32_t* req_off,
                                  const int32_t* req_policy, const int32_t* d_req,
                                  uint64_t* d_pass, int64_t ld_words, HostStage* stage,
                                  hipStream_t s);
// A GAS fit whose side-stream wait timed out (device flags) reports here: after the fit's
// stream was synchronized, PAS_EDEVICE (and the side streams drained) if a wait gave up since
// the last report, else PAS_OK.
int gas_fault_check(pas_ctx* ctx);
int gas_fit_launch(pas_ctx* ctx, int32_t i915_index, const PodBatch& pods, uint32_t* d_res,
                   int64_t ld_res, uint64_t* d_fit, pas_gas_selection* d_side, int64_t side_cap,
                   int64_t* d_side_count, hipStream_t s);
// (d_sub / d_subs of the top-k and merge launches: the wide records' third array, pas.h;
// null = the 64-bit records)
int tas_topk_launch(pas_ctx* ctx, int32_t n_pods, int32_t n_rules, const pas_rule* d_rules,
                    const int32_t* d_rule_off, const pas_rule* d_prio, const uint64_t* d_cand,
                    int32_t k, int32_t node_base, int64_t* d_key, uint32_t* d_sub,
                    int32_t* d_node, int32_t* d_len, hipStream_t s);
// d_after_key / d_after_sub (wide records) / d_after_node: the pods' cursors, the lists resume
// strictly after them (pas.h); null d_after_key = the lists from their beginning.
int tas_gas_topk_launch(pas_ctx* ctx, int32_t n_rules, const pas_rule* d_rules,
                        const int32_t* d_rule_off, const pas_rule* d_prio,
                        const uint64_t* d_cand, int32_t i915_index, const PodBatch& pods,
                        int32_t k, int32_t node_base, int64_t* d_key, uint32_t* d_sub,
                        int32_t* d_node, int32_t* d_len, const int64_t* d_after_key,
                        const uint32_t* d_after_sub, const int32_t* d_after_node, hipStream_t s);
// The same walk by policy id over the resident table (valid and current: the caller has
// checked) and its cached violating sets; fit = false: TAS only (no GAS snapshot; of pods only
// n_pods is read, and no cursor argument).  Neither builds nor reads the node-major copies.
int tas_gas_topk_policies_launch(pas_ctx* ctx, const int32_t* d_pod_policy,
                                 const uint64_t* d_cand, bool fit, int32_t i915_index,
                                 const PodBatch& pods, int32_t k, int32_t node_base,
                                 int64_t* d_key, uint32_t* d_sub, int32_t* d_node, int32_t* d_len,
                                 const int64_t* d_after_key, const uint32_t* d_after_sub,
                                 const int32_t* d_after_node, hipStream_t s);
int list_merge_launch(pas_ctx* ctx, int32_t n_pods, int32_t n_shards, int32_t width,
                      const int64_t* d_keys, const uint32_t* d_subs, const int32_t* d_nodes,
                      int32_t* d_out_node, int64_t out_ld, int32_t* d_out_len, hipStream_t s);
int topk_merge_launch(pas_ctx* ctx, int32_t n_pods, int32_t k, int32_t n_shards,
                      const int64_t* d_keys, const uint32_t* d_subs, const int32_t* d_nodes,
                      int32_t* d_out_node, int32_t* d_out_len, hipStream_t s);
// Bind (fit + commit, release = false) or release of n_ops operations the host grouped by
// node: order = the operation indices sorted by node (stable), key[i] = the node of operation
// order[i] (all in range).  The walker kernel of the event path applies them (gas_commit.hip).
int gas_commit_launch(pas_ctx* ctx, bool release, int32_t n_ops, int32_t i915_index,
                      const int32_t* d_order, const uint32_t* d_key, const int32_t* d_pod,
                      const PodBatch& pods, const int32_t* d_cpc, const int32_t* d_cards,
                      int32_t cards_stride, uint32_t* d_res, int32_t* d_status,
                      uint8_t* d_cards_out, int32_t* d_nsel_out, int64_t* d_counts_out,
                      const int64_t* d_counts, hipStream_t s);
// Pod events (pas_gas_apply[_device]) on device arrays: grouped by node on the device
// (NodeRuns, gas_group.h: storage from the stream's slot) and applied in call order by the
// walker kernel, all enqueued on s.  Nothing of the snapshot has changed when it returns an
// error.
int gas_apply_launch(pas_ctx* ctx, int32_t n_events, const int32_t* d_kind,
                     const int32_t* d_pod, const int32_t* d_node, const PodBatch& pods,
                     const int32_t* d_cpc, const int32_t* d_cards,
                     int32_t cards_ld, int32_t* d_status, hipStream_t s);
// Node updates (pas_gas_nodes_update[_device], gas_nodes.hip) on device arrays: grouped by node
// on the device (NodeRuns, gas_group.h) and applied in call order, all enqueued on s.  Nothing
// of the snapshot has changed when it returns an error.
int gas_nodes_update_launch(pas_ctx* ctx, int32_t n_updates, const int32_t* d_node,
                            const int32_t* d_n_cards, const int64_t* d_cap,
                            const int32_t* d_src, int32_t* d_status, hipStream_t s);
// The resident n_cards / cap / used copied into storage of n_nodes_new x max_cards_new (both
// >= the resident shape), new nodes -1 / 0 / 0 and new card slots 0; reads the snapshot only.
int gas_repitch_launch(pas_ctx* ctx, int32_t n_nodes_new, int32_t max_cards_new,
                       int32_t* d_n_cards_new, int64_t* d_cap_new, int64_t* d_used_new,
                       hipStream_t s);
// The resident rows gathered into storage of n_nodes_new x max_cards: new row j is old row
// d_src_node[j] (device [n_nodes_new], every entry -1 or below the resident count), or -1 / 0 /
// 0 for -1; reads the snapshot only.
int gas_compact_launch(pas_ctx* ctx, int32_t n_nodes_new, const int32_t* d_src_node,
                       int32_t* d_n_cards_new, int64_t* d_cap_new, int64_t* d_used_new,
                       hipStream_t s);
// Batch placement (gas_place.hip): the rounds of pas_gas_place_device on s, returning when the
// placement is complete.  *began: commits were launched (an error past that point leaves
// the resident usage half committed: the caller invalidates the snapshot).
int gas_place_launch(pas_ctx* ctx, int32_t i915_index, const PodBatch& pods, int32_t k,
                     int32_t ld, int32_t node_base, const int32_t* d_cand,
                     const int32_t* d_cand_len, int32_t* d_place_node, int32_t* d_place_rank,
                     uint32_t* d_res, uint8_t* d_cards_out, int32_t* d_nsel_out,
                     int64_t* d_counts_out, int32_t* n_placed, int32_t* n_rounds,
                     bool* began, hipStream_t s);
// Policy names of the deschedule strategies (updateNodeLabels keys its non-violated set by
// name, deschedule/enforce.go:89-134).  A name is represented by its first strategy k
// (canonical); bit k of canon marks those.  Names held by one strategy are the bits of single;
// each name held by two or more strategies is a group: its member strategies and its k.  A
// node's violated names: (add & single) | {key[g] : add & group[g] != 0}.
struct NamePlan {
  uint64_t canon = 0;
  uint64_t single = 0;
  int32_t n_groups = 0;
  uint8_t key[32] = {};
  uint64_t group[32] = {};
};
// The plan of name_id[0 .. n_strat) (NULL = all distinct); n_strat <= 64.
NamePlan make_name_plan(int32_t n_strat, const int32_t* name_id);
__device__ __forceinline__ uint64_t violated_names(const NamePlan& np, uint64_t add) {
  uint64_t vn = add & np.single;
  for (int32_t g = 0; g < np.n_groups; ++g)
    vn |= (add & np.group[g]) ? 1ull << np.key[g] : 0ull;
  return vn;
}
int label_plan_launch(pas_ctx* ctx, int32_t n_nodes, int32_t n_strat, const NamePlan& names,
                      const uint64_t* d_viol, const uint64_t* d_labels, uint64_t* d_add,
                      uint64_t* d_rem, int64_t* d_total, hipStream_t s);
// totalViolations from per-block counts of violated pairs: *d_total = pairs - sum(d_part).
int label_total_launch(pas_ctx* ctx, int32_t n_parts, int64_t pairs, const int64_t* d_part,
                       int64_t* d_total, hipStream_t s);
// The deschedule sweep with the label plan fused in (pas_tas_deschedule_device): viol as
// tas_violations_launch, add / rem / total as label_plan_launch on those bitmaps.
int tas_deschedule_launch(pas_ctx* ctx, int32_t n_strat, int32_t n_rules,
                          const pas_rule* d_rules, const int32_t* d_rule_off, uint64_t* d_viol,
                          const NamePlan& names,
                          const uint64_t* d_labels, uint64_t* d_add, uint64_t* d_rem,
                          int64_t* d_total, hipStream_t s);
// The plan as a patch list (tas_patches.hip): the nodes whose reduced masks (pas.h,
// pas_tas_label_patches) are not both zero, in ascending node index, as records d_node / d_add
// / d_rem [0 .. min(cap, n)), n to *d_n_patches, total as label_plan_launch.  d_labels,
// d_violating and d_null may be null; the record arrays too when cap is 0.
int label_patches_launch(pas_ctx* ctx, int32_t n_nodes, int32_t n_strat, const NamePlan& names,
                         const uint64_t* d_viol, const uint64_t* d_labels,
                         const uint64_t* d_violating, const uint64_t* d_null, int64_t cap,
                         int32_t* d_node, uint64_t* d_add, uint64_t* d_rem, int64_t* d_n_patches,
                         int64_t* d_total, hipStream_t s);
// tas_violations_launch into d_viol (null: the stream's slot), then label_patches_launch on
// those bitmaps for the snapshot's nodes.
int tas_deschedule_patches_launch(pas_ctx* ctx, int32_t n_strat, int32_t n_rules,
                                  const pas_rule* d_rules, const int32_t* d_rule_off,
                                  uint64_t* d_viol, const NamePlan& names,
                                  const uint64_t* d_labels, const uint64_t* d_violating,
                                  const uint64_t* d_null, int64_t cap, int32_t* d_node,
                                  uint64_t* d_add, uint64_t* d_rem, int64_t* d_n_patches,
                                  int64_t* d_total, hipStream_t s);

}  // namespace pas
