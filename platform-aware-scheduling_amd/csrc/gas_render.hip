// gas_render.hip — bind annotations and node names rendered from the resident name tables.
//
// bindNode hands the apiserver a "gas-container-cards" string per pod, card names joined by ","
// and containers by "|" (gpu-aware-scheduling/pkg/gpuscheduler/scheduler.go:317-335, 423-431),
// and the node's name for the Binding.  A placement answers in slots and card counts; the names
// stand in the two span pools (name_table.hip, gas_cards.hip).  A render is three steps over B
// spans (binds, or names):
//   1. render_lengths   a wavefront per span: annotation_render_len (annotation_fixed.h) over the
//                       bind's (container, card) items, 64 at a time with a saturating sum, reads
//                       sp.len of the node's row and gives the span's status and byte length;
//   2. scan_run         over the B + 1 lengths: the offsets, whose last one is the byte total.
//                       It is the call's one read-back: it sizes or checks the output;
//   3. render_write     a wavefront per span again: annotation_render_write, the items' starts
//                       from a prefix over the wave, the lanes striding over the bytes of each
//                       item, so neighbouring lanes store neighbouring bytes whatever the count
//                       or the name's length.  Stores are single bytes: a span starts on any
//                       byte residue and a wave's 64 byte stores already fall into one or two
//                       64-byte lines.
// A node name is the bind of one segment with one item, so pas_names_render is the same three
// steps.  A wavefront per span leaves a short bind's lanes idle in step 3; a flat byte-parallel
// grid that finds its span by a binary search of the offsets would not, at the price of the
// search and a second walk of the bind per 64 bytes.  The wavefront per span is what is built;
// the other mapping is unmeasured.  Nothing resident is written and no generation moves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "annotation_fixed.h"
#include "host_staging.h"
#include "pas_internal.h"
#include "span_pool.h"

namespace pas {
namespace {

constexpr int kTpb = 256;
constexpr int kWavesPerBlock = kTpb / 64;

// The 64 lanes of a wavefront as annotation_fixed.h's lane group; every lane is active.
struct Wave64 {
  static constexpr int kWidth = 64;
  __device__ int lane() const { return threadIdx.x & 63; }
  __device__ int64_t sum(int64_t v) const {
    for (int off = 32; off > 0; off >>= 1) v = render_sat_add(v, __shfl_xor(v, off, 64));
    return v;
  }
  __device__ bool any(bool p) const { return __ballot(p) != 0; }
  __device__ int64_t scan(int64_t v, int64_t* total) const {
    int64_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t y = __shfl_up(x, d, 64);
      if (lane() >= d) x += y;
    }
    *total = __shfl(x, 63, 64);
    return x - v;
  }
  __device__ uint64_t ballot(bool p) const { return __ballot(p); }
  __device__ int64_t from(int64_t v, int t) const { return __shfl(v, t, 64); }
  __device__ const char* from(const char* v, int t) const {
    return reinterpret_cast<const char*>(__shfl((unsigned long long)(uintptr_t)v, t, 64));
  }
};

// Row `row` of a span pool: name `rank` is entry row + rank
struct RowNames {
  const int64_t* beg_;
  const int64_t* len_;
  const char* pool_;
  int64_t row;
  __device__ int64_t len(int64_t rank) const { return len_[row + rank]; }
  __device__ const char* ptr(int64_t rank) const { return pool_ + beg_[row + rank]; }
};

// What a batch says of span b before its items are read: false for a span that is empty without
// a walk (*status says why), else the bind's segments, the row of its names and how many of
// them a bind may list.
struct Opened {
  int32_t nc;
  int64_t L, row;
};

struct CountsSrc {
  const int64_t* counts;  // the bind's [C][K]
  int32_t K;
  __device__ int64_t items(int32_t) const { return K; }
  __device__ void item(int64_t flat, int64_t i, int64_t* count, int64_t* rank) const {
    *count = counts[flat];
    *rank = i;
  }
};

struct RanksSrc {
  const int32_t* cpc;    // the bind's [C]
  const int32_t* cards;  // the bind's [cards_ld]
  int32_t cards_ld;
  // (one item past the row at most: that one is the error, and a wild count costs no long walk)
  __device__ int64_t items(int32_t c) const {
    return max(0, min(cpc[c], cards_ld == INT32_MAX ? cards_ld : cards_ld + 1));
  }
  __device__ void item(int64_t flat, int64_t, int64_t* count, int64_t* rank) const {
    const bool held = flat < cards_ld;
    *count = held ? 1 : -1;
    *rank = held ? cards[flat] : -1;
  }
};

// The binds of pas_gas_annotations_render*: node -1 is an unplaced pod, an empty span
struct BindBatch {
  int32_t N, K, C;
  const int32_t* node;
  const int32_t* ncont;
  const int32_t* n_cards;
  __device__ bool open(int64_t b, int32_t* status, Opened* o) const {
    const int32_t n = node[b];
    *status = n == -1 ? PAS_GAS_OK : PAS_GAS_ERR_INPUT;
    if (n < 0 || n >= N) return false;
    o->nc = max(0, min(ncont[b], C));
    o->L = max(0, min(n_cards[n], K));
    o->row = (int64_t)n * K;
    return true;
  }
};

struct CountsBatch : BindBatch {
  const int64_t* counts;
  __device__ CountsSrc src(int64_t b) const { return CountsSrc{counts + b * C * K, K}; }
};

struct RanksBatch : BindBatch {
  const int32_t* cpc;
  const int32_t* cards;
  int32_t cards_ld;
  __device__ RanksSrc src(int64_t b) const {
    return RanksSrc{cpc + b * C, cards + b * cards_ld, cards_ld};
  }
};

// The names of pas_names_render: one segment of one item, the slot's name
struct OneName {
  __device__ int64_t items(int32_t) const { return 1; }
  __device__ void item(int64_t, int64_t, int64_t* count, int64_t* rank) const {
    *count = 1;
    *rank = 0;
  }
};

struct SlotBatch {
  int32_t n_slots, slot_base;
  const int32_t* slot;
  __device__ bool open(int64_t b, int32_t* status, Opened* o) const {
    const int64_t s = (int64_t)slot[b] - slot_base;
    *status = PAS_GAS_OK;
    if (s < 0 || s >= n_slots) return false;
    *o = Opened{1, 1, s};
    return true;
  }
  __device__ OneName src(int64_t) const { return OneName{}; }
};

// len [B + 1] (the last one 0: the scan's total) and status [B] (may be null), a wavefront each
template <class Batch>
__global__ __launch_bounds__(kTpb) void render_lengths(int64_t B, Batch batch, RowNames t,
                                                       int32_t* __restrict__ status,
                                                       int64_t* __restrict__ len) {
  const int64_t b = ((int64_t)blockIdx.x * kTpb + threadIdx.x) >> 6;  // (uniform in the wave)
  if (b > B) return;
  const Wave64 w;
  int32_t st = PAS_GAS_OK;
  int64_t n = 0;
  Opened o;
  if (b < B && batch.open(b, &st, &o)) {
    t.row = o.row;
    st = annotation_render_len(w, o.nc, o.L, batch.src(b), t, &n);
  }
  if (w.lane() != 0) return;
  len[b] = n;
  if (b < B && status) status[b] = st;
}

// Span b into out[off[b] .. off[b + 1]); nothing for an empty span or one that ends past cap
template <class Batch>
__global__ __launch_bounds__(kTpb) void render_write(int64_t B, Batch batch, RowNames t,
                                                     const int64_t* __restrict__ off,
                                                     char* __restrict__ out, int64_t cap) {
  const int64_t b = ((int64_t)blockIdx.x * kTpb + threadIdx.x) >> 6;
  if (b >= B) return;
  const int64_t beg = off[b], end = off[b + 1];
  int32_t st;
  Opened o;
  if (end <= beg || beg < 0 || end > cap || !batch.open(b, &st, &o)) return;
  t.row = o.row;
  annotation_render_write(Wave64{}, o.nc, o.L, batch.src(b), t, out + beg, end - beg);
}

inline unsigned wave_blocks(int64_t waves) {
  return (unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
}

// The three steps for B spans of `batch` over the pool sp, on s: d_status [B] (may be null) and
// d_off [B + 1] always, *n_bytes_out (may be null) the byte total, and the bytes when cap holds
// them, into d_bytes, or (d_bytes null) into host_bytes through the slot's buffer; else
// PAS_ECAPACITY.  Synchronizes s once, before the write pass is enqueued.
template <class Batch>
int render_spans(pas_ctx* ctx, int64_t B, const Batch& batch, const SpanPool& sp,
                 int32_t* d_status, int64_t* d_off, char* d_bytes, char* host_bytes, int64_t cap,
                 int64_t* n_bytes_out, hipStream_t s, const std::string& fn) {
  int rc = PAS_OK;
  size_t scan_bytes = 0;
  if ((rc = scan_size<int64_t>(ctx, (size_t)B + 1, &scan_bytes))) return rc;
  SlotScope scope(ctx, s, 0, &rc);
  if (!scope.slot) return rc;
  const size_t ws = carve_size({sizeof(int64_t) * ((size_t)B + 1), scan_bytes});
  char* base = static_cast<char*>(slot_buf(ctx, scope.slot, kBufRender, ws, s, &rc));
  if (!base) return rc;
  Carve cv{base};
  int64_t* d_len = cv.take<int64_t>((size_t)B + 1);
  void* d_scan = cv.take<char>(scan_bytes);
  const RowNames t{sp.beg, sp.len, sp.pool, 0};
  render_lengths<<<wave_blocks(B + 1), kTpb, 0, s>>>(B, batch, t, d_status, d_len);
  PAS_HIP(ctx, hipGetLastError());
  if ((rc = scan_run<int64_t>(ctx, d_scan, scan_bytes, d_len, d_off, (size_t)B + 1, s))) return rc;
  int64_t total = 0;  // the call's one read-back
  PAS_HIP(ctx, hipMemcpyAsync(&total, d_off + B, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  PAS_HIP(ctx, hipStreamSynchronize(s));
  if (n_bytes_out) *n_bytes_out = total;
  if (cap < total)
    return set_error(ctx, PAS_ECAPACITY, fn + ": " + std::to_string(total) +
                                             " bytes to render, cap " + std::to_string(cap));
  if (total == 0) return PAS_OK;
  if (!d_bytes) {
    d_bytes = static_cast<char*>(
        slot_buf(ctx, scope.slot, kBufRenderBytes, (size_t)total, s, &rc));
    if (!d_bytes) {
      (void)hipGetLastError();  // (a failed allocation: no later launch check may see it)
      return rc;
    }
  } else {
    host_bytes = nullptr;
  }
  render_write<<<wave_blocks(B), kTpb, 0, s>>>(B, batch, t, d_off, d_bytes, total);
  PAS_HIP(ctx, hipGetLastError());
  if (host_bytes)
    PAS_HIP(ctx, hipMemcpyAsync(host_bytes, d_bytes, (size_t)total, hipMemcpyDeviceToHost, s));
  return PAS_OK;
}

// The snapshot, the card-name table and the shape arguments every bind form shares
int bind_forms_check(pas_ctx* ctx, int32_t n_binds, int32_t max_containers, const void* node,
                     const void* ncont, const void* items, const void* status_out,
                     const void* off_out, const void* bytes_out, int64_t cap,
                     const std::string& fn) {
  if (!ctx->gas.valid) return set_error(ctx, PAS_ENOSNAP, "no GAS snapshot uploaded");
  int rc = gas_annotations_tables(ctx, false, fn);
  if (rc) return rc;
  if (n_binds < 0 || max_containers < 0 || cap < 0)
    return set_error(ctx, PAS_EINVAL, fn + ": bad shape");
  if (!status_out || !off_out || (cap > 0 && !bytes_out))
    return set_error(ctx, PAS_EINVAL, fn + ": null output");
  if (n_binds > 0 && (!node || !ncont || (max_containers > 0 && !items)))
    return set_error(ctx, PAS_EINVAL, fn + ": null input");
  return activate(ctx);
}

BindBatch bind_batch(const pas_ctx* ctx, int32_t max_containers, const int32_t* d_node,
                     const int32_t* d_ncont) {
  const GasSnapshot& g = ctx->gas;
  return BindBatch{g.n_nodes, g.max_cards, max_containers, d_node, d_ncont, g.n_cards};
}

// A host form's binds: n_containers in [0, max_containers], nodes -1 or in the snapshot
int bind_host_check(pas_ctx* ctx, int32_t n_binds, const int32_t* node, const int32_t* ncont,
                    int32_t max_containers, const std::string& fn) {
  for (int32_t b = 0; b < n_binds; ++b) {
    if (node[b] < -1 || node[b] >= ctx->gas.n_nodes)
      return set_error(ctx, PAS_EINVAL, fn + ": bind " + std::to_string(b) + " names node " +
                                            std::to_string(node[b]));
    if (ncont[b] < 0 || ncont[b] > max_containers)
      return set_error(ctx, PAS_EINVAL, fn + ": bind " + std::to_string(b) + " has " +
                                            std::to_string(ncont[b]) + " containers");
  }
  return PAS_OK;
}

// The end of a host form: the outputs come back also when the bytes did not fit
int host_finish(pas_ctx* ctx, int rc, Staging& st) {
  if (rc && rc != PAS_ECAPACITY) return rc;
  PAS_HIP(ctx, st.fetch());
  return rc;
}

}  // namespace
}  // namespace pas

using namespace pas;

extern "C" {

int pas_gas_annotations_render_device(pas_ctx* ctx, int32_t n_binds, const int32_t* d_bind_node,
                                      const int32_t* d_n_containers, int32_t max_containers,
                                      const int64_t* d_counts, int32_t* d_status_out,
                                      int64_t* d_ann_off_out, char* d_ann_bytes_out, int64_t cap,
                                      int64_t* n_bytes_out, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_annotations_render_device";
  int rc = bind_forms_check(ctx, n_binds, max_containers, d_bind_node, d_n_containers, d_counts,
                            d_status_out, d_ann_off_out, d_ann_bytes_out, cap, fn);
  if (rc) return rc;
  CountsBatch batch{bind_batch(ctx, max_containers, d_bind_node, d_n_containers), d_counts};
  return render_spans(ctx, n_binds, batch, ctx->gas_cards.sp, d_status_out, d_ann_off_out,
                      d_ann_bytes_out, nullptr, cap, n_bytes_out, pick_stream(ctx, hip_stream),
                      fn);
}

int pas_gas_annotations_render(pas_ctx* ctx, int32_t n_binds, const int32_t* bind_node,
                               const int32_t* n_containers, int32_t max_containers,
                               const int64_t* counts, int32_t* status_out, int64_t* ann_off_out,
                               char* ann_bytes_out, int64_t cap, int64_t* n_bytes_out) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_annotations_render";
  int rc = bind_forms_check(ctx, n_binds, max_containers, bind_node, n_containers, counts,
                            status_out, ann_off_out, ann_bytes_out, cap, fn);
  if (rc) return rc;
  if ((rc = bind_host_check(ctx, n_binds, bind_node, n_containers, max_containers, fn)))
    return rc;
  const size_t B = (size_t)n_binds;
  Staging st(ctx);
  int32_t *d_node, *d_nc, *d_status;
  int64_t *d_counts, *d_off;
  st.in(d_node, bind_node, B);
  st.in(d_nc, n_containers, B);
  st.in(d_counts, counts, B * (size_t)max_containers * (size_t)ctx->gas.max_cards);
  st.out(d_status, status_out, B);
  st.out(d_off, ann_off_out, B + 1);
  if ((rc = st.upload())) return rc;
  CountsBatch batch{bind_batch(ctx, max_containers, d_node, d_nc), d_counts};
  rc = render_spans(ctx, n_binds, batch, ctx->gas_cards.sp, d_status, d_off, nullptr,
                    ann_bytes_out, cap, n_bytes_out, ctx->stream, fn);
  return host_finish(ctx, rc, st);
}

int pas_gas_annotations_render_ranks_device(
    pas_ctx* ctx, int32_t n_binds, const int32_t* d_bind_node, const int32_t* d_n_containers,
    int32_t max_containers, const int32_t* d_cards_per_container, const int32_t* d_cards,
    int32_t cards_ld, int32_t* d_status_out, int64_t* d_ann_off_out, char* d_ann_bytes_out,
    int64_t cap, int64_t* n_bytes_out, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_annotations_render_ranks_device";
  int rc = bind_forms_check(ctx, n_binds, max_containers, d_bind_node, d_n_containers,
                            d_cards_per_container, d_status_out, d_ann_off_out, d_ann_bytes_out,
                            cap, fn);
  if (rc) return rc;
  if (cards_ld < 0 || (n_binds > 0 && cards_ld > 0 && !d_cards))
    return set_error(ctx, PAS_EINVAL, fn + ": cards_ld < 0 or null cards");
  RanksBatch batch{bind_batch(ctx, max_containers, d_bind_node, d_n_containers),
                   d_cards_per_container, d_cards, cards_ld};
  return render_spans(ctx, n_binds, batch, ctx->gas_cards.sp, d_status_out, d_ann_off_out,
                      d_ann_bytes_out, nullptr, cap, n_bytes_out, pick_stream(ctx, hip_stream),
                      fn);
}

int pas_gas_annotations_render_ranks(pas_ctx* ctx, int32_t n_binds, const int32_t* bind_node,
                                     const int32_t* n_containers, int32_t max_containers,
                                     const int32_t* cards_per_container, const int32_t* cards,
                                     int32_t cards_ld, int32_t* status_out, int64_t* ann_off_out,
                                     char* ann_bytes_out, int64_t cap, int64_t* n_bytes_out) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_annotations_render_ranks";
  int rc = bind_forms_check(ctx, n_binds, max_containers, bind_node, n_containers,
                            cards_per_container, status_out, ann_off_out, ann_bytes_out, cap, fn);
  if (rc) return rc;
  if (cards_ld < 0 || (n_binds > 0 && cards_ld > 0 && !cards))
    return set_error(ctx, PAS_EINVAL, fn + ": cards_ld < 0 or null cards");
  if ((rc = bind_host_check(ctx, n_binds, bind_node, n_containers, max_containers, fn)))
    return rc;
  const size_t B = (size_t)n_binds;
  Staging st(ctx);
  int32_t *d_node, *d_nc, *d_cpc, *d_cards, *d_status;
  int64_t* d_off;
  st.in(d_node, bind_node, B);
  st.in(d_nc, n_containers, B);
  st.in(d_cpc, cards_per_container, B * (size_t)max_containers);
  st.in(d_cards, cards, B * (size_t)cards_ld);
  st.out(d_status, status_out, B);
  st.out(d_off, ann_off_out, B + 1);
  if ((rc = st.upload())) return rc;
  RanksBatch batch{bind_batch(ctx, max_containers, d_node, d_nc), d_cpc, d_cards, cards_ld};
  rc = render_spans(ctx, n_binds, batch, ctx->gas_cards.sp, d_status, d_off, nullptr,
                    ann_bytes_out, cap, n_bytes_out, ctx->stream, fn);
  return host_finish(ctx, rc, st);
}

static int names_render_check(pas_ctx* ctx, int64_t n, const void* slot, const void* off_out,
                              const void* bytes_out, int64_t cap, const std::string& fn) {
  if (!ctx->names.valid) return no_table(ctx, fn, "name table");
  if (n < 0 || n > INT32_MAX || cap < 0) return set_error(ctx, PAS_EINVAL, fn + ": bad shape");
  if (!off_out || (cap > 0 && !bytes_out) || (n > 0 && !slot))
    return set_error(ctx, PAS_EINVAL, fn + ": null input or output");
  return activate(ctx);
}

int pas_names_render_device(pas_ctx* ctx, int64_t n, const int32_t* d_slot, int32_t slot_base,
                            int64_t* d_off_out, char* d_bytes_out, int64_t cap,
                            int64_t* n_bytes_out, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_names_render_device";
  int rc = names_render_check(ctx, n, d_slot, d_off_out, d_bytes_out, cap, fn);
  if (rc) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  if ((rc = derived_wait(ctx, ctx->names_sync, s))) return rc;
  return render_spans(ctx, n, SlotBatch{ctx->names.n_slots, slot_base, d_slot}, ctx->names.sp,
                      nullptr, d_off_out, d_bytes_out, nullptr, cap, n_bytes_out, s, fn);
}

int pas_names_render(pas_ctx* ctx, int64_t n, const int32_t* slot, int32_t slot_base,
                     int64_t* off_out, char* bytes_out, int64_t cap, int64_t* n_bytes_out) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_names_render";
  int rc = names_render_check(ctx, n, slot, off_out, bytes_out, cap, fn);
  if (rc) return rc;
  Staging st(ctx);
  int32_t* d_slot;
  int64_t* d_off;
  st.in(d_slot, slot, (size_t)n);
  st.out(d_off, off_out, (size_t)n + 1);
  if ((rc = st.upload())) return rc;
  if ((rc = derived_wait(ctx, ctx->names_sync, ctx->stream))) return rc;
  rc = render_spans(ctx, n, SlotBatch{ctx->names.n_slots, slot_base, d_slot}, ctx->names.sp,
                    nullptr, d_off, nullptr, bytes_out, cap, n_bytes_out, ctx->stream, fn);
  return host_finish(ctx, rc, st);
}

}  // extern "C"
