// pas_api.hip — the C-ABI surface (include/pas.h): context, errors, timing and the
// host-pointer wrappers around the device launches.  The verbs that take strings keep their
// entry points next to their kernels (tas_ingest.hip, name_table.hip, gas_cards.hip,
// gas_annotations.hip, gas_node_strings.hip, gas_render.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "host_staging.h"
#include "pas.h"
#include "pas_internal.h"

namespace pas {

int set_error(pas_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

int check_hip(pas_ctx* ctx, hipError_t e, const char* what) {
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  return set_error(ctx, e == hipErrorOutOfMemory ? PAS_ENOMEM : PAS_EDEVICE, m);
}

int activate(pas_ctx* ctx) {
  PAS_HIP(ctx, hipSetDevice(ctx->device));
  return PAS_OK;
}

hipStream_t pick_stream(pas_ctx* ctx, void* s) {
  if (s == PAS_STREAM_NULL) return nullptr;  // the HIP null stream
  return s ? reinterpret_cast<hipStream_t>(s) : ctx->stream;
}

int ensure_scratch(pas_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->scratch_bytes) return PAS_OK;
  if (ctx->scratch) {
    PAS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PAS_HIP(ctx, hipFree(ctx->scratch));
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
  }
  size_t want = std::max(bytes, size_t(1) << 20);
  PAS_HIP(ctx, hipMalloc(&ctx->scratch, want));
  ctx->scratch_bytes = want;
  return PAS_OK;
}

// PAS_OK, or check_hip's status for a failed call
static int hip_status(pas_ctx* ctx, hipError_t e, const char* what) {
  return e == hipSuccess ? PAS_OK : check_hip(ctx, e, what);
}

AuxSlot* aux_acquire(pas_ctx* ctx, hipStream_t s, size_t bytes, int* rc) {
  AuxSlot* slot = nullptr;
  for (AuxSlot& a : ctx->aux_slot)
    if (a.used && a.stream == s) slot = &a;  // this stream's own slot: stream order
  if (!slot)
    for (AuxSlot& a : ctx->aux_slot)
      if (!a.used && !slot) slot = &a;
  if (!slot) {  // the least recently used slot, after its last call
    slot = &ctx->aux_slot[0];
    for (AuxSlot& a : ctx->aux_slot)
      if (a.last < slot->last) slot = &a;
    *rc = hip_status(ctx, hipStreamWaitEvent(s, slot->ev, 0), "aux_acquire: hipStreamWaitEvent");
    if (*rc) return nullptr;
  }
  if (!slot->ev) {
    *rc = hip_status(ctx, hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming),
                    "aux_acquire: hipEventCreateWithFlags");
    if (*rc) return nullptr;
  }
  if (bytes > slot->bytes) {
    if (slot->p) {  // the slot's earlier calls are ordered before s: let them finish
      *rc = hip_status(ctx, hipStreamSynchronize(s), "aux_acquire: hipStreamSynchronize");
      if (!*rc) *rc = hip_status(ctx, hipFree(slot->p), "aux_acquire: hipFree");
      if (*rc) return nullptr;
      slot->p = nullptr;
      slot->bytes = 0;
    }
    *rc = hip_status(ctx, hipMalloc(&slot->p, bytes), "aux_acquire: hipMalloc");
    if (*rc) return nullptr;
    slot->bytes = bytes;
  }
  *rc = PAS_OK;
  return slot;
}

void* slot_buf(pas_ctx* ctx, AuxSlot* slot, int which, size_t bytes, hipStream_t s, int* rc) {
  *rc = PAS_OK;
  if (bytes <= slot->buf_bytes[which]) return slot->buf[which];
  if (slot->buf[which]) {  // the slot's earlier calls are ordered before s: let them finish
    *rc = hip_status(ctx, hipStreamSynchronize(s), "slot_buf: hipStreamSynchronize");
    if (!*rc) *rc = hip_status(ctx, hipFree(slot->buf[which]), "slot_buf: hipFree");
    if (*rc) return nullptr;
    slot->buf[which] = nullptr;
    slot->buf_bytes[which] = 0;
  }
  *rc = hip_status(ctx, hipMalloc(&slot->buf[which], bytes), "slot_buf: hipMalloc");
  if (*rc) return nullptr;
  slot->buf_bytes[which] = bytes;
  return slot->buf[which];
}

int derived_built(pas_ctx* ctx, DerivedSync& d, hipStream_t s) {
  if (!d.ev) {
    int rc = hip_status(ctx, hipEventCreateWithFlags(&d.ev, hipEventDisableTiming),
                        "derived_built: hipEventCreateWithFlags");
    if (rc) return rc;
  }
  int rc = hip_status(ctx, hipEventRecord(d.ev, s), "derived_built: hipEventRecord");
  if (rc) return rc;
  d.stream = s;
  d.valid = true;
  return PAS_OK;
}

int derived_wait(pas_ctx* ctx, const DerivedSync& d, hipStream_t s) {
  if (!d.valid || d.stream == s) return PAS_OK;  // same stream: stream order
  return hip_status(ctx, hipStreamWaitEvent(s, d.ev, 0), "derived_wait: hipStreamWaitEvent");
}

void aux_release(pas_ctx* ctx, AuxSlot* slot, hipStream_t s) {
  (void)hipEventRecord(slot->ev, s);
  slot->stream = s;
  slot->used = true;
  slot->last = ++ctx->aux_clock;
}

static hipEvent_t take_event(pas_ctx* ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

void timing_begin(pas_ctx* ctx, hipStream_t s, int kernel, TimedLaunch* tl) {
  tl->kernel = -1;
  // span-level timing brackets whole paths only: events between the launches of a path
  // would add gaps to the span they measure
  if (!ctx->timing || (ctx->timing == PAS_TIMING_SPAN && kernel != PAS_K_TAS_SPAN &&
                       kernel != PAS_K_PRIO_REQUEST && kernel != PAS_K_GAS_FIT && kernel != PAS_K_TAS_VIOLATIONS &&
                       kernel != PAS_K_TAS_LABELS))
    return;
  tl->start = take_event(ctx);
  tl->stop = take_event(ctx);
  if (!tl->start || !tl->stop) return;
  tl->kernel = kernel;
  (void)hipEventRecord(tl->start, s);
}

void timing_end(pas_ctx* ctx, hipStream_t s, TimedLaunch* tl) {
  if (tl->kernel < 0) return;
  (void)hipEventRecord(tl->stop, s);
  ctx->pending.push_back(*tl);
}

static void resolve_timing(pas_ctx* ctx) {
  for (auto& tl : ctx->pending) {
    float ms = 0.f;
    if (hipEventSynchronize(tl.stop) == hipSuccess &&
        hipEventElapsedTime(&ms, tl.start, tl.stop) == hipSuccess) {
      ctx->total_ms[tl.kernel] += ms;
      ctx->launches[tl.kernel] += 1;
    }
    ctx->event_pool.push_back(tl.start);
    ctx->event_pool.push_back(tl.stop);
  }
  ctx->pending.clear();
}

static void free_ptr(void*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

void tas_free_storage(TasSnapshot& t) {
  free_ptr(reinterpret_cast<void*&>(t.vals));
  free_ptr(reinterpret_cast<void*&>(t.present));
  free_ptr(reinterpret_cast<void*&>(t.vals_t));
  free_ptr(reinterpret_cast<void*&>(t.pres_t));
  t.vals_t_bytes = 0;
  t.pres_t_bytes = 0;
  t.t_epoch = 0;
  free_ptr(reinterpret_cast<void*&>(t.cnt));
  free_ptr(reinterpret_cast<void*&>(t.sorted));
  free_ptr(reinterpret_cast<void*&>(t.perm));
  free_ptr(reinterpret_cast<void*&>(t.f1k));
  free_ptr(reinterpret_cast<void*&>(t.f32));
  free_ptr(reinterpret_cast<void*&>(t.scale_tab));
  free_ptr(reinterpret_cast<void*&>(t.wide_flag));
  free_ptr(reinterpret_cast<void*&>(t.nano));
  free_ptr(reinterpret_cast<void*&>(t.sorted_nano));
  free_ptr(reinterpret_cast<void*&>(t.f1k_nano));
  free_ptr(reinterpret_cast<void*&>(t.f32_nano));
  free_ptr(t.wide_sort_tmp);
  free_ptr(t.keys_a);
  free_ptr(t.keys_b);
  free_ptr(reinterpret_cast<void*&>(t.ids_a));
  free_ptr(reinterpret_cast<void*&>(t.ids_b));
  free_ptr(reinterpret_cast<void*&>(t.popc));
  free_ptr(reinterpret_cast<void*&>(t.word_scan));
  free_ptr(reinterpret_cast<void*&>(t.rows));
  free_ptr(t.sort_tmp);
  free_ptr(t.scan_tmp);
}

void free_tas(pas_ctx* ctx) {
  TasSnapshot& t = ctx->tas;
  tas_free_storage(t);
  const hipEvent_t ev = t.t_sync.ev;  // kept for the context's life (pas_destroy)
  t = TasSnapshot{};
  t.t_sync.ev = ev;
}

void free_gas(pas_ctx* ctx) {
  GasSnapshot& g = ctx->gas;
  free_ptr(reinterpret_cast<void*&>(g.n_cards));
  free_ptr(reinterpret_cast<void*&>(g.cap));
  free_ptr(reinterpret_cast<void*&>(g.used));
  free_ptr(g.derived);
  free_ptr(g.free_t);
  const hipEvent_t ev = g.derived_sync.ev;
  g = GasSnapshot{};
  g.derived_sync.ev = ev;
}

int gas_annotations_tables(pas_ctx* ctx, bool by_name, const std::string& fn) {
  const GasCardNames& t = ctx->gas_cards;
  if (!t.valid) return set_error(ctx, PAS_ENOSNAP, fn + ": no card-name table");
  if (by_name && !ctx->names.valid) return set_error(ctx, PAS_ENOSNAP, fn + ": no name table");
  if (t.n_slots != ctx->gas.n_nodes || t.k != ctx->gas.max_cards)
    return set_error(ctx, PAS_EINVAL,
                     fn + ": the card-name table is " + std::to_string(t.n_slots) + " x " +
                         std::to_string(t.k) + ", the GAS snapshot " +
                         std::to_string(ctx->gas.n_nodes) + " x " +
                         std::to_string(ctx->gas.max_cards));
  return PAS_OK;
}

int check_update(pas_ctx* ctx, uint64_t gen_from, int32_t n_cols, const int32_t* cols,
                 const void* vals, const void* present, const char* fn) {
  if (!ctx->tas.valid) return set_error(ctx, PAS_ENOSNAP, std::string(fn) + ": no TAS snapshot");
  if (ctx->tas.gen != gen_from)
    return set_error(ctx, PAS_ESTALE, std::string(fn) + ": resident generation " +
                                          std::to_string(ctx->tas.gen) + ", update from " +
                                          std::to_string(gen_from));
  const int32_t M = ctx->tas.n_metrics;
  if (n_cols < 0 || n_cols > M)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad column count");
  if (n_cols > 0 && (!cols || (ctx->tas.n_nodes > 0 && (!vals || !present))))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  std::vector<char> seen((size_t)M, 0);
  for (int32_t c = 0; c < n_cols; ++c) {
    if (cols[c] < 0 || cols[c] >= M || seen[(size_t)cols[c]]++)
      return set_error(ctx, PAS_EINVAL,
                       std::string(fn) + ": columns must be distinct metric indices < n_metrics");
  }
  return PAS_OK;
}

int check_gas_gen(pas_ctx* ctx, uint64_t gen) {
  if (!ctx->gas.valid) return set_error(ctx, PAS_ENOSNAP, "no GAS snapshot uploaded");
  if (ctx->gas.gen != gen) return set_error(ctx, PAS_ESTALE, "GAS snapshot generation mismatch");
  return PAS_OK;
}

int gas_pod_check(pas_ctx* ctx, int32_t p, int32_t max_containers,
                  const uint32_t* req_mask, const int32_t* n_containers,
                  const char* fn) {
  if (n_containers[p] < 0 || n_containers[p] > max_containers)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": n_containers out of range");
  for (int32_t c = 0; c < n_containers[p]; ++c)
    if ((req_mask[(int64_t)p * max_containers + c] & ~PAS_REQ_UNKNOWN_KIND) >> ctx->gas.n_res)
      return set_error(ctx, PAS_EINVAL, std::string(fn) + ": mask bit >= n_res");
  return PAS_OK;
}

int gas_finish(pas_ctx* ctx, int rc, bool wrote, uint64_t gen_to, bool cards) {
  if (rc) {
    if (wrote) {
      ctx->gas.valid = false;
      if (cards) ctx->gas_cards.valid = false;
    }
    return rc;
  }
  ctx->gas.gen = gen_to;
  ++ctx->gas.epoch;
  return PAS_OK;
}

}  // namespace pas

using namespace pas;

extern "C" {

int pas_abi_version(void) { return PAS_ABI_VERSION; }

int pas_create(const pas_config* cfg, pas_ctx** out) {
  if (!out) return PAS_EINVAL;
  *out = nullptr;
  pas_ctx* ctx = new (std::nothrow) pas_ctx();
  if (!ctx) return PAS_ENOMEM;
  int dev = cfg ? cfg->device : -1;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) {
      delete ctx;
      return PAS_EDEVICE;
    }
  }
  ctx->device = dev;
  if (hipSetDevice(dev) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return PAS_EDEVICE;
  }
  ctx->stream = ctx->own_stream;
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
      n_cu > 0)
    ctx->n_cu = n_cu;
  *out = ctx;
  return PAS_OK;
}

void pas_destroy(pas_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  resolve_timing(ctx);
  for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
  free_tas(ctx);
  free_gas(ctx);
  if (ctx->tas.t_sync.ev) (void)hipEventDestroy(ctx->tas.t_sync.ev);
  if (ctx->gas.derived_sync.ev) (void)hipEventDestroy(ctx->gas.derived_sync.ev);
  if (ctx->policies.dev) (void)hipFree(ctx->policies.dev);
  if (ctx->policies.viol) (void)hipFree(ctx->policies.viol);
  if (ctx->policies.viol_sync.ev) (void)hipEventDestroy(ctx->policies.viol_sync.ev);
  free_names(ctx->names);
  free_pool(ctx->gas_cards.sp);
  if (ctx->names_sync.ev) (void)hipEventDestroy(ctx->names_sync.ev);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->gas_sync_fault) (void)hipHostFree(ctx->gas_sync_fault);
  if (ctx->place_host) (void)hipHostFree(ctx->place_host);
  for (AuxSlot& a : ctx->aux_slot) {
    if (a.p) (void)hipFree(a.p);
    if (a.gas_counts) (void)hipFree(a.gas_counts);
    if (a.gas_limit) (void)hipFree(a.gas_limit);
    if (a.gas_sync) (void)hipFree(a.gas_sync);
    if (a.ev) (void)hipEventDestroy(a.ev);
    if (a.fork) (void)hipEventDestroy(a.fork);
    if (a.join) (void)hipEventDestroy(a.join);
    if (a.join2) (void)hipEventDestroy(a.join2);
    if (a.side) (void)hipStreamDestroy(a.side);
    if (a.side2) (void)hipStreamDestroy(a.side2);
    for (void* b : a.buf)
      if (b) (void)hipFree(b);
  }
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

const char* pas_last_error(const pas_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int pas_set_stream(pas_ctx* ctx, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  ctx->stream = hip_stream == PAS_STREAM_NULL ? nullptr
                : hip_stream                  ? reinterpret_cast<hipStream_t>(hip_stream)
                                              : ctx->own_stream;
  return PAS_OK;
}

int pas_synchronize(pas_ctx* ctx) {
  if (!ctx) return PAS_EINVAL;
  PAS_HIP(ctx, hipSetDevice(ctx->device));
  PAS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // every stream's calls: the slots' last users and the GAS fits' side streams
  for (AuxSlot& a : ctx->aux_slot) {
    if (a.used && a.ev) PAS_HIP(ctx, hipEventSynchronize(a.ev));
    if (a.side) PAS_HIP(ctx, hipStreamSynchronize(a.side));
    if (a.side2) PAS_HIP(ctx, hipStreamSynchronize(a.side2));
  }
  // a GAS fit whose side-stream wait gave up (device flags): its results are incomplete
  return gas_fault_check(ctx);
}

int pas_parse_operator(const char* op) {
  if (!op) return PAS_EINVAL;
  if (std::strcmp(op, "LessThan") == 0) return PAS_OP_LESS_THAN;
  if (std::strcmp(op, "GreaterThan") == 0) return PAS_OP_GREATER_THAN;
  if (std::strcmp(op, "Equals") == 0) return PAS_OP_EQUALS;
  return PAS_EINVAL;
}

// pas_quantity_to_milli / pas_quantity_as_int64: quantity.cpp (host only)

// --------------------------------------------------------------------------- TAS

int pas_tas_snapshot_set(pas_ctx* ctx, uint64_t gen, int32_t n_nodes, int32_t n_metrics,
                         const int64_t* v_milli, const uint64_t* present) {
  if (!ctx) return PAS_EINVAL;
  if (n_nodes < 0 || n_metrics < 0 || (n_nodes > 0 && n_metrics > 0 && (!v_milli || !present)))
    return set_error(ctx, PAS_EINVAL, "pas_tas_snapshot_set: bad shape or null input");
  int rc = activate(ctx);
  if (rc) return rc;
  Staging st(ctx);
  int64_t* d_v;
  uint64_t* d_p;
  st.in(d_v, v_milli, (size_t)n_nodes * (size_t)n_metrics);
  st.in(d_p, present, (size_t)w64(n_nodes) * (size_t)n_metrics);
  if ((rc = st.upload())) return rc;
  ++ctx->tas_col_epoch;
  rc = tas_snapshot_build(ctx, gen, n_nodes, n_metrics, d_v, d_p, ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_tas_snapshot_set_device(pas_ctx* ctx, uint64_t gen, int32_t n_nodes, int32_t n_metrics,
                                const int64_t* d_v_milli, const uint64_t* d_present,
                                void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  if (n_nodes < 0 || n_metrics < 0) return set_error(ctx, PAS_EINVAL, "bad snapshot shape");
  int rc = activate(ctx);
  if (rc) return rc;
  ++ctx->tas_col_epoch;
  return tas_snapshot_build(ctx, gen, n_nodes, n_metrics, d_v_milli, d_present,
                            pick_stream(ctx, hip_stream));
}

// The host forms' staging: the columns (nano with the wide form only) into the context's
// scratch, the update on the context's stream, and its end awaited.
static int stage_update(pas_ctx* ctx, uint64_t gen_to, int32_t n_cols, const int32_t* cols,
                        const int64_t* vals, const uint32_t* nano, const uint64_t* present,
                        bool wide) {
  int rc = activate(ctx);
  if (rc) return rc;
  const size_t N = (size_t)ctx->tas.n_nodes, n = (size_t)n_cols;
  Staging st(ctx);
  int64_t* d_v;
  uint32_t* d_n;
  uint64_t* d_p;
  st.in(d_v, vals, n * N);
  st.in(d_n, nano, wide ? n * N : 0);
  st.in(d_p, present, n * (size_t)w64(N));
  if ((rc = st.upload())) return rc;
  hipStream_t s = ctx->stream;
  rc = wide ? tas_snapshot_update_wide(ctx, gen_to, n_cols, cols, d_v, d_n, d_p, s)
            : tas_snapshot_update(ctx, gen_to, n_cols, cols, d_v, d_p, s);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_tas_snapshot_update(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_cols,
                            const int32_t* cols, const int64_t* v_milli,
                            const uint64_t* present) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_update(ctx, gen_from, n_cols, cols, v_milli, present, "pas_tas_snapshot_update");
  if (rc) return rc;
  return stage_update(ctx, gen_to, n_cols, cols, v_milli, nullptr, present, false);
}

int pas_tas_snapshot_update_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                   int32_t n_cols, const int32_t* cols, const int64_t* d_v_milli,
                                   const uint64_t* d_present, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_update(ctx, gen_from, n_cols, cols, d_v_milli, d_present,
                        "pas_tas_snapshot_update_device");
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  return tas_snapshot_update(ctx, gen_to, n_cols, cols, d_v_milli, d_present,
                             pick_stream(ctx, hip_stream));
}

int pas_tas_snapshot_update_wide(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                 int32_t n_cols, const int32_t* cols, const int64_t* whole,
                                 const uint32_t* nano, const uint64_t* present) {
  if (!ctx) return PAS_EINVAL;
  const char* fn = "pas_tas_snapshot_update_wide";
  int rc = check_update(ctx, gen_from, n_cols, cols, whole, present, fn);
  if (rc) return rc;
  const int32_t N = ctx->tas.n_nodes;
  if (n_cols > 0 && N > 0 && !nano) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  for (int64_t i = 0; i < (int64_t)n_cols * N; ++i)
    if (nano[i] > 999999999u)
      return set_error(ctx, PAS_EINVAL, std::string(fn) + ": nano of column " +
                                            std::to_string(cols[i / N]) + ", node " +
                                            std::to_string(i % N) + " is not below 10^9");
  return stage_update(ctx, gen_to, n_cols, cols, whole, nano, present, true);
}

int pas_tas_snapshot_update_wide_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                        int32_t n_cols, const int32_t* cols,
                                        const int64_t* d_whole, const uint32_t* d_nano,
                                        const uint64_t* d_present, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const char* fn = "pas_tas_snapshot_update_wide_device";
  int rc = check_update(ctx, gen_from, n_cols, cols, d_whole, d_present, fn);
  if (rc) return rc;
  if (n_cols > 0 && ctx->tas.n_nodes > 0 && !d_nano)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  if ((rc = activate(ctx))) return rc;
  return tas_snapshot_update_wide(ctx, gen_to, n_cols, cols, d_whole, d_nano, d_present,
                                  pick_stream(ctx, hip_stream));
}

int pas_tas_snapshot_drop(pas_ctx* ctx) {
  if (!ctx) return PAS_EINVAL;
  ctx->tas.valid = false;
  ++ctx->tas_col_epoch;
  return PAS_OK;
}

int pas_tas_snapshot_wide_count(const pas_ctx* ctx, int32_t* n_wide) {
  if (!ctx || !n_wide) return PAS_EINVAL;
  if (!ctx->tas.valid) return PAS_ENOSNAP;
  *n_wide = ctx->tas.n_wide;
  return PAS_OK;
}

// The top-k records carry one 64-bit merge key per node: no exact key for a wide column yet.
static int check_no_wide(pas_ctx* ctx, const char* fn) {
  if (ctx->tas.n_wide == 0) return PAS_OK;
  size_t m = 0;
  while (m < ctx->tas.wide_host.size() && !ctx->tas.wide_host[m]) ++m;
  return set_error(ctx, PAS_ENOTEXACT, std::string(fn) + ": metric column " + std::to_string(m) +
                                           " is wide (64-bit top-k merge keys cannot order it)");
}

int pas_tas_snapshot_info(const pas_ctx* ctx, uint64_t* gen, int32_t* n_nodes,
                          int32_t* n_metrics) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->tas.valid) return PAS_ENOSNAP;
  if (gen) *gen = ctx->tas.gen;
  if (n_nodes) *n_nodes = ctx->tas.n_nodes;
  if (n_metrics) *n_metrics = ctx->tas.n_metrics;
  return PAS_OK;
}

static int check_tas_gen(pas_ctx* ctx, uint64_t gen) {
  if (!ctx->tas.valid) return set_error(ctx, PAS_ENOSNAP, "no TAS snapshot uploaded");
  if (ctx->tas.gen != gen)
    return set_error(ctx, PAS_ESTALE, "TAS snapshot generation mismatch: resident " +
                                          std::to_string(ctx->tas.gen) + ", requested " +
                                          std::to_string(gen));
  return PAS_OK;
}

int pas_tas_snapshot_set_scale(pas_ctx* ctx, uint64_t gen, int32_t n_metrics,
                               const int32_t* col_scale, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  const int32_t M = ctx->tas.n_metrics;
  if (n_metrics != M || (M > 0 && !col_scale))
    return set_error(ctx, PAS_EINVAL, "pas_tas_snapshot_set_scale: n_metrics != the snapshot's");
  std::vector<int64_t> tab(2 * (size_t)M);
  for (int32_t m = 0; m < M; ++m) {
    if (col_scale[m] < 0 || col_scale[m] > 9)
      return set_error(ctx, PAS_EINVAL, "pas_tas_snapshot_set_scale: scale outside 0..9");
    int64_t mult = 1;
    for (int32_t i = 0; i < col_scale[m]; ++i) mult *= 10;
    tab[2 * (size_t)m] = mult;
    tab[2 * (size_t)m + 1] = INT64_MAX / mult;
  }
  if (M == 0) return PAS_OK;
  if (ctx->tas.n_wide > 0)  // a wide column keeps its recorded scale
    for (int32_t m = 0; m < M; ++m)
      if (ctx->tas.wide_host[(size_t)m]) {
        tab[2 * (size_t)m] = ctx->tas.scale_host[2 * (size_t)m];
        tab[2 * (size_t)m + 1] = ctx->tas.scale_host[2 * (size_t)m + 1];
      }
  ctx->tas.scale_host = tab;
  ctx->policies.viol_built = false;  // the generation stays: the policy bitmaps go by hand
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  // (into the resident table, not scratch: no Staging)
  PAS_HIP(ctx, hipMemcpyAsync(ctx->tas.scale_tab, tab.data(), sizeof(int64_t) * tab.size(),
                              hipMemcpyHostToDevice, s));
  PAS_HIP(ctx, hipStreamSynchronize(s));  // tab is this call's
  return PAS_OK;
}

int pas_tas_snapshot_reshape(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                             int32_t n_nodes_new, int32_t n_metrics_new, const int32_t* src_col,
                             void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_tas_snapshot_reshape";
  int rc = check_tas_gen(ctx, gen_from);
  if (rc) return rc;
  TasSnapshot& t = ctx->tas;
  const int32_t M = t.n_metrics;
  if (n_nodes_new < t.n_nodes)
    return set_error(ctx, PAS_EINVAL, fn + ": the node count only grows");
  if (n_metrics_new < 0 || (!src_col && n_metrics_new < M))
    return set_error(ctx, PAS_EINVAL, fn + ": fewer metric columns need a src_col");
  // pas_tas_snapshot_set's limit, before anything of that size is allocated, here or there
  if ((int64_t)n_metrics_new * order_row(n_nodes_new) * kNumOrders > 0x7fffffffLL)
    return set_error(ctx, PAS_ECAPACITY,
                     "TAS snapshot: 3 * n_metrics * padded n_nodes must be < 2^31");
  // the column map, checked: an old column at most once, or -1
  std::vector<int32_t> src((size_t)n_metrics_new);
  std::vector<char> seen((size_t)M, 0);
  bool identity = n_metrics_new == M;
  for (int32_t m = 0; m < n_metrics_new; ++m) {
    const int32_t c = src_col ? src_col[m] : m < M ? m : -1;
    if (c < -1 || c >= M || (c >= 0 && seen[(size_t)c]++))
      return set_error(ctx, PAS_EINVAL,
                       fn + ": src_col entries must be distinct columns < n_metrics, or -1");
    src[(size_t)m] = c;
    identity &= c == m;
  }
  if (identity && n_nodes_new == t.n_nodes) {  // the same shape and columns
    t.gen = gen_to;
    return PAS_OK;
  }
  if ((rc = activate(ctx))) return rc;
  ++ctx->tas_col_epoch;
  return tas_snapshot_reshape(ctx, gen_to, n_nodes_new, n_metrics_new, src.data(),
                              pick_stream(ctx, hip_stream));
}

// The node map of the compactions: n_new >= 0 entries (a host array), each -1 or an old slot
// below n_old, the old slots strictly increasing.  *identity: n_new == n_old and entry j is j.
static int check_node_map(pas_ctx* ctx, int32_t n_old, int32_t n_new, const int32_t* src_node,
                          const std::string& fn, bool* identity) {
  if (n_new < 0 || (n_new > 0 && !src_node))
    return set_error(ctx, PAS_EINVAL, fn + ": n_nodes_new < 0, or no src_node");
  int32_t last = -1;
  *identity = n_new == n_old;
  for (int32_t j = 0; j < n_new; ++j) {
    const int32_t s = src_node[j];
    *identity &= s == j;
    if (s == -1) continue;
    if (s < -1 || s >= n_old || s <= last)
      return set_error(ctx, PAS_EINVAL,
                       fn + ": src_node entries must be -1 or strictly increasing slots < n_nodes");
    last = s;
  }
  return PAS_OK;
}

int pas_tas_snapshot_compact(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                             int32_t n_nodes_new, const int32_t* src_node, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen_from);
  if (rc) return rc;
  TasSnapshot& t = ctx->tas;
  bool identity;
  if ((rc = check_node_map(ctx, t.n_nodes, n_nodes_new, src_node, "pas_tas_snapshot_compact",
                           &identity)))
    return rc;
  // pas_tas_snapshot_set's limit, before anything of that size is allocated, here or there
  if ((int64_t)t.n_metrics * order_row(n_nodes_new) * kNumOrders > 0x7fffffffLL)
    return set_error(ctx, PAS_ECAPACITY,
                     "TAS snapshot: 3 * n_metrics * padded n_nodes must be < 2^31");
  if (identity) {  // every slot in place
    t.gen = gen_to;
    return PAS_OK;
  }
  if ((rc = activate(ctx))) return rc;
  return tas_snapshot_compact(ctx, gen_to, n_nodes_new, src_node, pick_stream(ctx, hip_stream));
}

int pas_tas_snapshot_get(pas_ctx* ctx, uint64_t* gen, int64_t* vals_out, uint64_t* present_out,
                         int32_t* scale_out, uint8_t* wide_out, uint32_t* nano_out) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->tas.valid) return set_error(ctx, PAS_ENOSNAP, "no TAS snapshot uploaded");
  const TasSnapshot& t = ctx->tas;
  const size_t M = (size_t)t.n_metrics, N = (size_t)t.n_nodes, W = (size_t)w64(t.n_nodes);
  int rc = activate(ctx);
  if (rc) return rc;
  // (out of the resident arrays, not scratch: no Staging)
  hipStream_t s = ctx->stream;
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  if (vals_out && M * N)
    PAS_HIP(ctx, hipMemcpyAsync(vals_out, t.vals, sizeof(int64_t) * M * N, d2h, s));
  if (present_out && M * W)
    PAS_HIP(ctx, hipMemcpyAsync(present_out, t.present, sizeof(uint64_t) * M * W, d2h, s));
  if (nano_out && M * N && t.nano)
    PAS_HIP(ctx, hipMemcpyAsync(nano_out, t.nano, sizeof(uint32_t) * M * N, d2h, s));
  PAS_HIP(ctx, hipStreamSynchronize(s));
  for (size_t m = 0; m < M; ++m) {
    // the resident last word keeps what its upload carried past n_nodes
    if (present_out && W) {
      uint64_t& last = present_out[m * W + W - 1];
      last = word_mask(last, (int64_t)W - 1, t.n_nodes);
    }
    const bool wide = t.n_wide > 0 && t.wide_host[m];
    if (nano_out && !wide) std::memset(nano_out + m * N, 0, sizeof(uint32_t) * N);  // unset rows
    if (wide_out) wide_out[m] = wide ? 1 : 0;
    if (scale_out) {
      int32_t sc = 0;
      for (int64_t mult = t.scale_host[2 * m]; mult > 1; mult /= 10) ++sc;
      scale_out[m] = sc;
    }
  }
  if (gen) *gen = t.gen;
  return PAS_OK;
}

// Host-side rule validation: an unknown operator string panics in core.EvaluateRule
// (operator.go:25) only when the rule is evaluated, i.e. when its metric is cached
// (dontschedule/strategy.go:28-32 skips missing metrics first).  Here: PAS_EINVAL.
// An unknown operator panics in the reference only when EvaluateRule runs, i.e. when the
// rule's metric map has at least one node (dontschedule/strategy.go:33-41, operator.go:25);
// otherwise the rule is never evaluated.  The column count is read back only in that
// (rare) case.  The *_device entry points do not validate: their callers parse operators
// with pas_parse_operator when the policy is built, and the kernels skip unknown ones.
static int validate_rules(pas_ctx* ctx, int32_t n, const pas_rule* rules) {
  for (int32_t i = 0; i < n; ++i) {
    const pas_rule& r = rules[i];
    if (r.op >= 0 && r.op <= 2) continue;
    if (r.metric < 0 || r.metric >= ctx->tas.n_metrics) continue;  // never evaluated
    int32_t c = 0;
    PAS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PAS_HIP(ctx, hipMemcpy(&c, ctx->tas.cnt + r.metric, sizeof(c), hipMemcpyDeviceToHost));
    if (c == 0) continue;  // empty metric map: no EvaluateRule call
    return set_error(ctx, PAS_EINVAL, "rule " + std::to_string(i) + ": unknown operator " +
                                          std::to_string(r.op) +
                                          " (the reference panics in EvaluateRule)");
  }
  return PAS_OK;
}

static int validate_csr(pas_ctx* ctx, int32_t n, const int32_t* off, const char* what) {
  if (off[0] != 0) return set_error(ctx, PAS_EINVAL, std::string(what) + ": offsets[0] != 0");
  for (int32_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i])
      return set_error(ctx, PAS_EINVAL, std::string(what) + ": offsets not monotone");
  return PAS_OK;
}

int pas_tas_eval(pas_ctx* ctx, uint64_t gen, int32_t n_pods, const pas_rule* rules,
                 const int32_t* rule_off, const pas_rule* prio, const uint64_t* cand,
                 uint32_t flags, uint64_t* pass_out, int32_t* order_out, int32_t* order_len) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  if (n_pods < 0 || (n_pods > 0 && (!rule_off || !prio)))
    return set_error(ctx, PAS_EINVAL, "pas_tas_eval: null rule_off/prio");
  if ((flags & PAS_TAS_FILTER) && n_pods > 0 && !pass_out)
    return set_error(ctx, PAS_EINVAL, "pas_tas_eval: FILTER without pass_out");
  if ((flags & PAS_TAS_PRIORITIZE) && n_pods > 0 && (!order_out || !order_len))
    return set_error(ctx, PAS_EINVAL, "pas_tas_eval: PRIORITIZE without order outputs");
  if (n_pods == 0) return PAS_OK;
  if ((rc = validate_csr(ctx, n_pods, rule_off, "rule_off"))) return rc;
  const int32_t n_rules = rule_off[n_pods];
  if (n_rules > 0 && !rules) return set_error(ctx, PAS_EINVAL, "pas_tas_eval: null rules");
  if ((rc = validate_rules(ctx, n_rules, rules))) return rc;
  if ((rc = activate(ctx))) return rc;
  const size_t P = (size_t)n_pods, N = (size_t)ctx->tas.n_nodes, W = (size_t)w64(N);
  const bool filter = flags & PAS_TAS_FILTER, order = flags & PAS_TAS_PRIORITIZE;
  Staging st(ctx);
  pas_rule *d_rules, *d_prio;
  int32_t *d_off, *d_order, *d_len;
  uint64_t *d_cand, *d_pass;
  st.in(d_rules, rules, (size_t)n_rules);
  st.in(d_off, rule_off, P + 1);
  st.in(d_prio, prio, P);
  st.in_opt(d_cand, cand, W * P);
  st.out_opt(d_pass, filter ? pass_out : nullptr, W * P);
  st.out(d_len, order ? order_len : nullptr, P);
  st.out_opt(d_order, order ? order_out : nullptr, N * P);
  if ((rc = st.upload())) return rc;
  rc = tas_eval_launch(ctx, n_pods, n_rules, d_rules, d_off, d_prio, d_cand, flags, d_pass,
                       d_order, d_len, 0, ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_tas_eval_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t n_rules,
                        const pas_rule* d_rules, const int32_t* d_rule_off,
                        const pas_rule* d_prio, const uint64_t* d_cand, uint32_t flags,
                        uint64_t* d_pass_out, int32_t* d_order_out, int32_t* d_order_len,
                        void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  if (n_pods < 0 || n_rules < 0) return set_error(ctx, PAS_EINVAL, "negative count");
  if (n_pods == 0) return PAS_OK;
  if (!d_rule_off || !d_prio || (n_rules > 0 && !d_rules))
    return set_error(ctx, PAS_EINVAL, "pas_tas_eval_device: null input");
  if ((flags & PAS_TAS_FILTER) && !d_pass_out)
    return set_error(ctx, PAS_EINVAL, "pas_tas_eval_device: FILTER without pass_out");
  if ((flags & PAS_TAS_PRIORITIZE) && (!d_order_out || !d_order_len))
    return set_error(ctx, PAS_EINVAL, "pas_tas_eval_device: PRIORITIZE without outputs");
  if ((rc = activate(ctx))) return rc;
  return tas_eval_launch(ctx, n_pods, n_rules, d_rules, d_rule_off, d_prio, d_cand, flags,
                         d_pass_out, d_order_out, d_order_len, 0, pick_stream(ctx, hip_stream));
}

static int check_prio_request(pas_ctx* ctx, const pas_rule* prio, int32_t n_req,
                              const void* req, const void* pos, const void* len) {
  if (!prio || n_req < 0 || !len || (n_req > 0 && (!req || !pos)))
    return set_error(ctx, PAS_EINVAL, "pas_tas_prioritize_request: bad argument");
  if (prio->metric >= ctx->tas.n_metrics)
    return set_error(ctx, PAS_EINVAL, "pas_tas_prioritize_request: metric out of range");
  return PAS_OK;
}

int pas_tas_prioritize_request(pas_ctx* ctx, uint64_t gen, const pas_rule* prio, int32_t n_req,
                               const int32_t* req_node, int32_t* pos_out, int32_t* len_out) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  if ((rc = check_prio_request(ctx, prio, n_req, req_node, pos_out, len_out))) return rc;
  if ((rc = activate(ctx))) return rc;
  size_t ws = 0;
  if ((rc = prio_request_workspace(ctx, n_req, &ws))) return rc;
  Staging st(ctx);
  int32_t *d_req, *d_pos, *d_len;
  char* d_ws;
  st.in(d_req, req_node, (size_t)n_req);
  st.out(d_len, len_out, 1);
  st.out(d_pos, pos_out, (size_t)n_req);
  st.work(d_ws, ws);
  if ((rc = st.upload())) return rc;
  if ((rc = prio_request_launch(ctx, *prio, n_req, d_req, d_pos, d_len, d_ws, ws, ctx->stream)))
    return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_tas_prioritize_request_device(pas_ctx* ctx, uint64_t gen, const pas_rule* prio,
                                      int32_t n_req, const int32_t* d_req_node,
                                      int32_t* d_pos_out, int32_t* d_len_out,
                                      void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  if ((rc = check_prio_request(ctx, prio, n_req, d_req_node, d_pos_out, d_len_out))) return rc;
  if ((rc = activate(ctx))) return rc;
  size_t ws = 0;
  if ((rc = prio_request_workspace(ctx, n_req, &ws))) return rc;
  // the workspace is the stream's aux slot (calls on other streams may run beside this one)
  hipStream_t s = pick_stream(ctx, hip_stream);
  SlotScope sc(ctx, s, ws, &rc);
  if (!sc.slot) return rc;
  return prio_request_launch(ctx, *prio, n_req, d_req_node, d_pos_out, d_len_out, sc.slot->p, ws,
                             s);
}

// ------------------------------------------------------- batches of requests in request terms

// The requests of a *_requests call: R >= 0, req_off [R + 1] a CSR from 0 (its total is an
// int32, so at most INT32_MAX), req_node given when any request names a node.  *longest = the
// longest request.
static int check_requests(pas_ctx* ctx, int32_t n_requests, const int32_t* req_off,
                          const void* req_node, const char* fn, int32_t* longest) {
  *longest = 0;
  if (n_requests < 0) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": negative count");
  if (n_requests == 0) return PAS_OK;
  if (!req_off) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null req_off");
  int rc = validate_csr(ctx, n_requests, req_off, "req_off");
  if (rc) return rc;
  if (req_off[n_requests] > 0 && !req_node)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null req_node");
  for (int32_t r = 0; r < n_requests; ++r)
    *longest = std::max(*longest, req_off[r + 1] - req_off[r]);
  return PAS_OK;
}

// A bitmap output of a *_requests call: rows of ld_words >= W64(longest request).
static int check_request_rows(pas_ctx* ctx, int32_t longest, const void* out, int64_t ld_words,
                              const char* fn) {
  if (ld_words < w64(longest))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": ld_words < W64(longest request)");
  if (longest > 0 && !out) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null output");
  return PAS_OK;
}

// The rows a *_requests kernel wrote at pitch ld_dev, copied into the caller's rows of pitch
// ld_words: the W64(n_r) words of request r, nothing past them.  `rows` [n_requests][ld_dev]
// is the output the caller stated to st.
static int fetch_request_rows(pas_ctx* ctx, Staging& st, int32_t n_requests,
                              const int32_t* req_off, const std::vector<uint64_t>& rows,
                              int64_t ld_dev, uint64_t* out, int64_t ld_words) {
  PAS_HIP(ctx, st.fetch());
  for (int32_t r = 0; r < n_requests; ++r)
    std::copy_n(rows.data() + r * ld_dev, w64(req_off[r + 1] - req_off[r]), out + r * ld_words);
  return PAS_OK;
}

static int check_prio_requests(pas_ctx* ctx, int32_t n_requests, const pas_rule* prio,
                               int32_t total, const void* pos, const void* len) {
  if (n_requests == 0) return PAS_OK;
  if (!prio || !len || (total > 0 && !pos))
    return set_error(ctx, PAS_EINVAL, "pas_tas_prioritize_requests: null argument");
  for (int32_t r = 0; r < n_requests; ++r)
    if (prio[r].metric >= ctx->tas.n_metrics)
      return set_error(ctx, PAS_EINVAL, "pas_tas_prioritize_requests: request " +
                                            std::to_string(r) + ": metric out of range");
  return PAS_OK;
}

int pas_tas_prioritize_requests(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                const int32_t* req_off, const pas_rule* prio,
                                const int32_t* req_node, int32_t* pos_out, int32_t* len_out) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  int32_t longest = 0;
  if ((rc = check_requests(ctx, n_requests, req_off, req_node, "pas_tas_prioritize_requests",
                           &longest)))
    return rc;
  if (n_requests == 0) return PAS_OK;
  const int32_t T = req_off[n_requests];
  if ((rc = check_prio_requests(ctx, n_requests, prio, T, pos_out, len_out))) return rc;
  if ((rc = activate(ctx))) return rc;
  Staging st(ctx);
  int32_t *d_req, *d_pos, *d_len;
  st.in(d_req, req_node, (size_t)T);
  // (the few lengths before the positions: fetched in the other order, a call of 16 requests
  // x 1 000 nodes measured 7 us longer, 0.088 against 0.081 ms)
  st.out(d_len, len_out, (size_t)n_requests);
  st.out(d_pos, pos_out, (size_t)T);
  if ((rc = st.upload())) return rc;
  hipStream_t s = ctx->stream;
  HostStage stage;  // until the synchronize of the fetch
  if ((rc = prio_requests_launch(ctx, n_requests, req_off, prio, d_req, d_pos, d_len, &stage,
                                 s))) {
    (void)hipStreamSynchronize(s);  // a copy from the stage may be in flight
    return rc;
  }
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_tas_prioritize_requests_device(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                       const int32_t* req_off, const pas_rule* prio,
                                       const int32_t* d_req_node, int32_t* d_pos_out,
                                       int32_t* d_len_out, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  int32_t longest = 0;
  if ((rc = check_requests(ctx, n_requests, req_off, d_req_node,
                           "pas_tas_prioritize_requests_device", &longest)))
    return rc;
  if (n_requests == 0) return PAS_OK;
  if ((rc = check_prio_requests(ctx, n_requests, prio, req_off[n_requests], d_pos_out,
                                d_len_out)))
    return rc;
  if ((rc = activate(ctx))) return rc;
  return prio_requests_launch(ctx, n_requests, req_off, prio, d_req_node, d_pos_out, d_len_out,
                              nullptr, pick_stream(ctx, hip_stream));
}

int pas_tas_filter_requests(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                            const int32_t* req_off, const pas_rule* rules,
                            const int32_t* rule_off, const int32_t* req_node,
                            uint64_t* pass_out, int64_t ld_words) {
  const char* fn = "pas_tas_filter_requests";
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  int32_t longest = 0;
  if ((rc = check_requests(ctx, n_requests, req_off, req_node, fn, &longest))) return rc;
  if (n_requests == 0) return PAS_OK;
  if ((rc = check_request_rows(ctx, longest, pass_out, ld_words, fn))) return rc;
  if (!rule_off) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null rule_off");
  if ((rc = validate_csr(ctx, n_requests, rule_off, "rule_off"))) return rc;
  const int32_t n_rules = rule_off[n_requests];
  if (n_rules > 0 && !rules) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null rules");
  // (before the empty-list return: Violated runs before filterNodes looks at the node list)
  if ((rc = validate_rules(ctx, n_rules, rules))) return rc;
  if (longest == 0) return PAS_OK;
  if ((rc = activate(ctx))) return rc;
  const int32_t T = req_off[n_requests];
  const int64_t ld_dev = w64(longest);
  std::vector<uint64_t> rows((size_t)(n_requests * ld_dev));
  Staging st(ctx);
  int32_t *d_req, *d_off;
  pas_rule* d_rules;
  uint64_t* d_rows;
  st.in(d_req, req_node, (size_t)T);
  st.in(d_rules, rules, (size_t)n_rules);
  st.in(d_off, rule_off, (size_t)n_requests + 1);
  st.out(d_rows, rows.data(), rows.size());
  if ((rc = st.upload())) return rc;
  hipStream_t s = ctx->stream;
  HostStage stage;  // (req_off is the caller's until fetch_request_rows has synchronized)
  if ((rc = filter_requests_launch(ctx, n_requests, req_off, n_rules, d_rules, d_off, d_req,
                                   d_rows, ld_dev, &stage, s))) {
    (void)hipStreamSynchronize(s);  // the copy of req_off may be in flight
    return rc;
  }
  return fetch_request_rows(ctx, st, n_requests, req_off, rows, ld_dev, pass_out, ld_words);
}

int pas_tas_filter_requests_device(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                   const int32_t* req_off, int32_t n_rules,
                                   const pas_rule* d_rules, const int32_t* d_rule_off,
                                   const int32_t* d_req_node, uint64_t* d_pass_out,
                                   int64_t ld_words, void* hip_stream) {
  const char* fn = "pas_tas_filter_requests_device";
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  int32_t longest = 0;
  if ((rc = check_requests(ctx, n_requests, req_off, d_req_node, fn, &longest))) return rc;
  if (n_requests == 0) return PAS_OK;
  if ((rc = check_request_rows(ctx, longest, d_pass_out, ld_words, fn))) return rc;
  if (n_rules < 0 || !d_rule_off || (n_rules > 0 && !d_rules))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad rules");
  if ((rc = activate(ctx))) return rc;
  return filter_requests_launch(ctx, n_requests, req_off, n_rules, d_rules, d_rule_off,
                                d_req_node, d_pass_out, ld_words, nullptr,
                                pick_stream(ctx, hip_stream));
}

int pas_tas_violations(pas_ctx* ctx, uint64_t gen, int32_t n_strategies, const pas_rule* rules,
                       const int32_t* rule_off, uint64_t* viol_out) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  if (n_strategies < 0) return set_error(ctx, PAS_EINVAL, "negative strategy count");
  if (n_strategies == 0) return PAS_OK;
  if (!rule_off || !viol_out) return set_error(ctx, PAS_EINVAL, "null rule_off/viol_out");
  if ((rc = validate_csr(ctx, n_strategies, rule_off, "rule_off"))) return rc;
  const int32_t n_rules = rule_off[n_strategies];
  if (n_rules > 0 && !rules) return set_error(ctx, PAS_EINVAL, "null rules");
  if ((rc = validate_rules(ctx, n_rules, rules))) return rc;
  if ((rc = activate(ctx))) return rc;
  Staging st(ctx);
  pas_rule* d_rules;
  int32_t* d_off;
  uint64_t* d_viol;
  st.in(d_rules, rules, (size_t)n_rules);
  st.in(d_off, rule_off, (size_t)n_strategies + 1);
  st.out(d_viol, viol_out, (size_t)w64(ctx->tas.n_nodes) * (size_t)n_strategies);
  if ((rc = st.upload())) return rc;
  rc = tas_violations_launch(ctx, n_strategies, n_rules, d_rules, d_off, d_viol, ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_tas_violations_device(pas_ctx* ctx, uint64_t gen, int32_t n_strategies,
                              int32_t n_rules, const pas_rule* d_rules,
                              const int32_t* d_rule_off, uint64_t* d_viol_out,
                              void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  if (n_strategies < 0 || n_rules < 0) return set_error(ctx, PAS_EINVAL, "negative count");
  if (n_strategies == 0) return PAS_OK;
  if (!d_rule_off || !d_viol_out || (n_rules > 0 && !d_rules))
    return set_error(ctx, PAS_EINVAL, "pas_tas_violations_device: null input");
  if ((rc = activate(ctx))) return rc;
  return tas_violations_launch(ctx, n_strategies, n_rules, d_rules, d_rule_off, d_viol_out,
                               pick_stream(ctx, hip_stream));
}

// ------------------------------------------------------------ the resident policy table

int pas_tas_policies_set(pas_ctx* ctx, int32_t n_policies, const pas_rule* rules,
                         const int32_t* rule_off, const pas_rule* prio) {
  const std::string fn = "pas_tas_policies_set";
  if (!ctx) return PAS_EINVAL;
  if (!ctx->tas.valid)  // the metric indices are the resident snapshot's columns
    return set_error(ctx, PAS_ENOSNAP, fn + ": no TAS snapshot");
  if (n_policies < 0 || (n_policies > 0 && (!rule_off || !prio)))
    return set_error(ctx, PAS_EINVAL, fn + ": negative count or null rule_off/prio");
  static const int32_t no_off[1] = {0};
  if (n_policies == 0) rule_off = no_off;
  int rc = validate_csr(ctx, n_policies, rule_off, "rule_off");
  if (rc) return rc;
  const int32_t n_rules = rule_off[n_policies];
  if (n_rules > 0 && !rules) return set_error(ctx, PAS_EINVAL, fn + ": null rules");
  if ((rc = activate(ctx))) return rc;
  TasPolicies& pt = ctx->policies;
  const size_t P = (size_t)n_policies, R = (size_t)n_rules;
  const size_t b_rules = sizeof(pas_rule) * R, b_off = sizeof(int32_t) * (P + 1),
               b_prio = sizeof(pas_rule) * P;
  const size_t need = carve_size({b_rules, b_off, b_prio});
  pt.valid = false;
  // (the caller orders a table change after the verbs that read the table on other streams,
  // as a snapshot change)
  PAS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (need > pt.dev_bytes) {
    if (pt.dev) {
      PAS_HIP(ctx, hipDeviceSynchronize());
      PAS_HIP(ctx, hipFree(pt.dev));
      pt.dev = nullptr;
      pt.dev_bytes = 0;
    }
    PAS_HIP(ctx, hipMalloc(&pt.dev, need));
    pt.dev_bytes = need;
  }
  pt.rules.assign(rules, rules + R);
  pt.rule_off.assign(rule_off, rule_off + P + 1);
  pt.prio.assign(prio, prio + P);
  Carve cv{static_cast<char*>(pt.dev)};
  pt.d_rules = cv.take<pas_rule>(R);
  pt.d_rule_off = cv.take<int32_t>(P + 1);
  pt.d_prio = cv.take<pas_rule>(P);
  hipStream_t s = ctx->stream;
  if (b_rules)
    PAS_HIP(ctx, hipMemcpyAsync(pt.d_rules, pt.rules.data(), b_rules, hipMemcpyHostToDevice, s));
  PAS_HIP(ctx, hipMemcpyAsync(pt.d_rule_off, pt.rule_off.data(), b_off, hipMemcpyHostToDevice, s));
  if (b_prio)
    PAS_HIP(ctx, hipMemcpyAsync(pt.d_prio, pt.prio.data(), b_prio, hipMemcpyHostToDevice, s));
  PAS_HIP(ctx, hipStreamSynchronize(s));  // verbs on any stream may read the table from here on
  pt.n_policies = n_policies;
  pt.n_rules = n_rules;
  pt.col_epoch = ctx->tas_col_epoch;
  ++pt.serial;
  pt.valid = true;
  return PAS_OK;
}

int pas_tas_policies_info(const pas_ctx* ctx, int32_t* n_policies, int32_t* n_rules) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->policies.valid) return PAS_EINVAL;
  if (n_policies) *n_policies = ctx->policies.n_policies;
  if (n_rules) *n_rules = ctx->policies.n_rules;
  return PAS_OK;
}

int pas_tas_policies_drop(pas_ctx* ctx) {
  if (!ctx) return PAS_EINVAL;
  ctx->policies.valid = false;  // (the storage is kept for the next table)
  ctx->policies.viol_built = false;
  return PAS_OK;
}

// A policy verb's preconditions: the snapshot at gen, a table, and the table not older than
// the snapshot's column numbering.
static int check_policies(pas_ctx* ctx, uint64_t gen, const char* fn) {
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  if (!ctx->policies.valid)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": no policy table (pas_tas_policies_set)");
  if (ctx->policies.col_epoch != ctx->tas_col_epoch)
    return set_error(ctx, PAS_ESTALE,
                     std::string(fn) + ": the policy table predates a column change of the TAS "
                                       "snapshot (set, reshape or drop): set the table again");
  return PAS_OK;
}

// ids [n] within [-1, n_policies); seen (when given): the policies the ids reference.
static int check_policy_ids(pas_ctx* ctx, int32_t n, const int32_t* ids, const char* fn,
                            std::vector<char>* seen) {
  const int32_t np = ctx->policies.n_policies;
  if (seen) seen->assign((size_t)np, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (ids[i] < -1 || ids[i] >= np)
      return set_error(ctx, PAS_EINVAL, std::string(fn) + ": policy id " +
                                            std::to_string(ids[i]) + " at " + std::to_string(i) +
                                            " outside [-1, n_policies)");
    if (seen && ids[i] >= 0) (*seen)[(size_t)ids[i]] = 1;
  }
  return PAS_OK;
}

// validate_rules' test (the reference panics where EvaluateRule meets an unknown operator) on
// the rules of the referenced policies only: a policy no pod names is never read.
static int validate_policies(pas_ctx* ctx, const std::vector<char>& seen) {
  const TasPolicies& pt = ctx->policies;
  for (int32_t i = 0; i < pt.n_policies; ++i) {
    if (!seen[(size_t)i]) continue;
    const int32_t a = pt.rule_off[(size_t)i], b = pt.rule_off[(size_t)i + 1];
    if (int rc = validate_rules(ctx, b - a, pt.rules.data() + a)) {
      ctx->err = "policy " + std::to_string(i) + ", " + ctx->err;
      return rc;
    }
  }
  return PAS_OK;
}

int pas_tas_policies_violated(pas_ctx* ctx, uint64_t gen, uint64_t* viol_out) {
  const char* fn = "pas_tas_policies_violated";
  if (!ctx) return PAS_EINVAL;
  int rc = check_policies(ctx, gen, fn);
  if (rc) return rc;
  const size_t words = (size_t)ctx->policies.n_policies * (size_t)w64(ctx->tas.n_nodes);
  if (words == 0) return PAS_OK;
  if (!viol_out) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null viol_out");
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = ctx->stream;
  const uint64_t* viol = nullptr;
  if ((rc = policies_viol(ctx, s, &viol))) return rc;
  // (out of the resident bitmaps, not scratch: no Staging)
  PAS_HIP(ctx, hipMemcpyAsync(viol_out, viol, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, s));
  PAS_HIP(ctx, hipStreamSynchronize(s));
  return PAS_OK;
}

int pas_tas_policies_violated_device(pas_ctx* ctx, uint64_t gen, uint64_t* d_viol_out,
                                     void* hip_stream) {
  const char* fn = "pas_tas_policies_violated_device";
  if (!ctx) return PAS_EINVAL;
  int rc = check_policies(ctx, gen, fn);
  if (rc) return rc;
  const size_t words = (size_t)ctx->policies.n_policies * (size_t)w64(ctx->tas.n_nodes);
  if (words == 0) return PAS_OK;
  if (!d_viol_out) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null viol_out");
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  const uint64_t* viol = nullptr;
  if ((rc = policies_viol(ctx, s, &viol))) return rc;
  PAS_HIP(ctx, hipMemcpyAsync(d_viol_out, viol, sizeof(uint64_t) * words,
                              hipMemcpyDeviceToDevice, s));
  return PAS_OK;
}

int pas_tas_eval_policies(pas_ctx* ctx, uint64_t gen, int32_t n_pods, const int32_t* pod_policy,
                          const uint64_t* cand, uint32_t flags, uint64_t* pass_out,
                          int32_t* order_out, int32_t* order_len) {
  const std::string fn = "pas_tas_eval_policies";
  if (!ctx) return PAS_EINVAL;
  int rc = check_policies(ctx, gen, fn.c_str());
  if (rc) return rc;
  if (n_pods < 0 || (n_pods > 0 && !pod_policy))
    return set_error(ctx, PAS_EINVAL, fn + ": negative count or null pod_policy");
  if ((flags & PAS_TAS_FILTER) && n_pods > 0 && !pass_out)
    return set_error(ctx, PAS_EINVAL, fn + ": FILTER without pass_out");
  if ((flags & PAS_TAS_PRIORITIZE) && n_pods > 0 && (!order_out || !order_len))
    return set_error(ctx, PAS_EINVAL, fn + ": PRIORITIZE without order outputs");
  if (n_pods == 0) return PAS_OK;
  std::vector<char> seen;
  if ((rc = check_policy_ids(ctx, n_pods, pod_policy, fn.c_str(), &seen))) return rc;
  if ((rc = validate_policies(ctx, seen))) return rc;
  if ((rc = activate(ctx))) return rc;
  const size_t P = (size_t)n_pods, N = (size_t)ctx->tas.n_nodes, W = (size_t)w64(N);
  const bool filter = flags & PAS_TAS_FILTER, order = flags & PAS_TAS_PRIORITIZE;
  Staging st(ctx);
  int32_t *d_pol, *d_order, *d_len;
  uint64_t *d_cand, *d_pass;
  st.in(d_pol, pod_policy, P);
  st.in_opt(d_cand, cand, W * P);
  st.out_opt(d_pass, filter ? pass_out : nullptr, W * P);
  st.out(d_len, order ? order_len : nullptr, P);
  st.out_opt(d_order, order ? order_out : nullptr, N * P);
  if ((rc = st.upload())) return rc;
  rc = policy_eval_launch(ctx, n_pods, d_pol, d_cand, flags, d_pass, d_order, d_len,
                          ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_tas_eval_policies_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods,
                                 const int32_t* d_pod_policy, const uint64_t* d_cand,
                                 uint32_t flags, uint64_t* d_pass_out, int32_t* d_order_out,
                                 int32_t* d_order_len, void* hip_stream) {
  const std::string fn = "pas_tas_eval_policies_device";
  if (!ctx) return PAS_EINVAL;
  int rc = check_policies(ctx, gen, fn.c_str());
  if (rc) return rc;
  if (n_pods < 0) return set_error(ctx, PAS_EINVAL, fn + ": negative count");
  if (n_pods == 0) return PAS_OK;
  if (!d_pod_policy) return set_error(ctx, PAS_EINVAL, fn + ": null pod_policy");
  if ((flags & PAS_TAS_FILTER) && !d_pass_out)
    return set_error(ctx, PAS_EINVAL, fn + ": FILTER without pass_out");
  if ((flags & PAS_TAS_PRIORITIZE) && (!d_order_out || !d_order_len))
    return set_error(ctx, PAS_EINVAL, fn + ": PRIORITIZE without outputs");
  if ((rc = activate(ctx))) return rc;
  return policy_eval_launch(ctx, n_pods, d_pod_policy, d_cand, flags, d_pass_out, d_order_out,
                            d_order_len, pick_stream(ctx, hip_stream));
}

int pas_tas_filter_requests_policies(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                     const int32_t* req_off, const int32_t* req_policy,
                                     const int32_t* req_node, uint64_t* pass_out,
                                     int64_t ld_words) {
  const char* fn = "pas_tas_filter_requests_policies";
  if (!ctx) return PAS_EINVAL;
  int rc = check_policies(ctx, gen, fn);
  if (rc) return rc;
  int32_t longest = 0;
  if ((rc = check_requests(ctx, n_requests, req_off, req_node, fn, &longest))) return rc;
  if (n_requests == 0) return PAS_OK;
  if ((rc = check_request_rows(ctx, longest, pass_out, ld_words, fn))) return rc;
  if (!req_policy) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null req_policy");
  std::vector<char> seen;
  if ((rc = check_policy_ids(ctx, n_requests, req_policy, fn, &seen))) return rc;
  // (before the empty-list return: Violated runs before filterNodes looks at the node list)
  if ((rc = validate_policies(ctx, seen))) return rc;
  if (longest == 0) return PAS_OK;
  if ((rc = activate(ctx))) return rc;
  const int32_t T = req_off[n_requests];
  const int64_t ld_dev = w64(longest);
  std::vector<uint64_t> rows((size_t)(n_requests * ld_dev));
  Staging st(ctx);
  int32_t* d_req;
  uint64_t* d_rows;
  st.in(d_req, req_node, (size_t)T);
  st.out(d_rows, rows.data(), rows.size());
  if ((rc = st.upload())) return rc;
  hipStream_t s = ctx->stream;
  HostStage stage;  // (req_off / req_policy are the caller's until the fetch has synchronized)
  if ((rc = filter_requests_policy_launch(ctx, n_requests, req_off, req_policy, d_req, d_rows,
                                          ld_dev, &stage, s))) {
    (void)hipStreamSynchronize(s);  // the copies of the host arrays may be in flight
    return rc;
  }
  return fetch_request_rows(ctx, st, n_requests, req_off, rows, ld_dev, pass_out, ld_words);
}

int pas_tas_filter_requests_policies_device(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                            const int32_t* req_off, const int32_t* req_policy,
                                            const int32_t* d_req_node, uint64_t* d_pass_out,
                                            int64_t ld_words, void* hip_stream) {
  const char* fn = "pas_tas_filter_requests_policies_device";
  if (!ctx) return PAS_EINVAL;
  int rc = check_policies(ctx, gen, fn);
  if (rc) return rc;
  int32_t longest = 0;
  if ((rc = check_requests(ctx, n_requests, req_off, d_req_node, fn, &longest))) return rc;
  if (n_requests == 0) return PAS_OK;
  if ((rc = check_request_rows(ctx, longest, d_pass_out, ld_words, fn))) return rc;
  if (!req_policy) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null req_policy");
  if ((rc = activate(ctx))) return rc;
  return filter_requests_policy_launch(ctx, n_requests, req_off, req_policy, d_req_node,
                                       d_pass_out, ld_words, nullptr,
                                       pick_stream(ctx, hip_stream));
}

// --------------------------------------------------------------------------- GAS

static int gas_alloc(pas_ctx* ctx, int32_t n_nodes, int32_t max_cards, int32_t n_res) {
  GasSnapshot& g = ctx->gas;
  if (g.n_nodes != n_nodes || g.max_cards != max_cards || g.n_res != n_res || !g.n_cards) {
    PAS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    free_gas(ctx);
    const size_t nn = (size_t)std::max(n_nodes, 1);
    PAS_HIP(ctx, hipMalloc(&g.n_cards, sizeof(int32_t) * nn));
    PAS_HIP(ctx, hipMalloc(&g.cap, sizeof(int64_t) * nn * (size_t)std::max(n_res, 1)));
    PAS_HIP(ctx, hipMalloc(&g.used, sizeof(int64_t) * nn * (size_t)std::max(max_cards, 1) *
                                        (size_t)std::max(n_res, 1)));
    PAS_HIP(ctx, hipMalloc(&g.derived, 64 + sizeof(int32_t) * nn));
    PAS_HIP(ctx, hipMalloc(&g.free_t, sizeof(int64_t) * PAS_GAS_PACKED *
                                          (size_t)std::max(n_res, 1) * nn));
    g.n_nodes = n_nodes;
    g.max_cards = max_cards;
    g.n_res = n_res;
  }
  return PAS_OK;
}

static int gas_shape_ok(pas_ctx* ctx, int32_t n_nodes, int32_t max_cards, int32_t n_res) {
  if (n_nodes < 0 || max_cards < 1 || n_res < 1)
    return set_error(ctx, PAS_EINVAL, "pas_gas_snapshot_set: bad shape");
  if (max_cards > PAS_GAS_MAX_CARDS || n_res > PAS_GAS_MAX_RES)
    return set_error(ctx, PAS_ECAPACITY,
                     "pas_gas_snapshot_set: max_cards <= 64 and n_res <= 4 supported");
  return PAS_OK;
}

int pas_gas_snapshot_set(pas_ctx* ctx, uint64_t gen, int32_t n_nodes, int32_t max_cards,
                         int32_t n_res, const int32_t* n_cards, const int64_t* cap_per_gpu,
                         const int64_t* used) {
  if (!ctx) return PAS_EINVAL;
  int rc = gas_shape_ok(ctx, n_nodes, max_cards, n_res);
  if (rc) return rc;
  if (n_nodes > 0 && (!n_cards || !cap_per_gpu || !used))
    return set_error(ctx, PAS_EINVAL, "pas_gas_snapshot_set: null input");
  for (int32_t n = 0; n < n_nodes; ++n)
    if (n_cards[n] > max_cards)
      return set_error(ctx, PAS_EINVAL, "pas_gas_snapshot_set: n_cards > max_cards");
  if ((rc = activate(ctx))) return rc;
  if ((rc = gas_alloc(ctx, n_nodes, max_cards, n_res))) return rc;
  GasSnapshot& g = ctx->gas;
  hipStream_t s = ctx->stream;
  if (n_nodes > 0) {  // straight into the resident arrays, not scratch: no Staging
    PAS_HIP(ctx, hipMemcpyAsync(g.n_cards, n_cards, sizeof(int32_t) * n_nodes,
                                hipMemcpyHostToDevice, s));
    PAS_HIP(ctx, hipMemcpyAsync(g.cap, cap_per_gpu, sizeof(int64_t) * n_nodes * n_res,
                                hipMemcpyHostToDevice, s));
    PAS_HIP(ctx, hipMemcpyAsync(g.used, used,
                                sizeof(int64_t) * (size_t)n_nodes * max_cards * n_res,
                                hipMemcpyHostToDevice, s));
  }
  PAS_HIP(ctx, hipStreamSynchronize(s));
  g.gen = gen;
  ++g.epoch;
  g.valid = true;
  return PAS_OK;
}

// The device snapshot's card counts, which the host cannot check: a count past max_cards is
// read as max_cards (pas_gas_snapshot_set rejects it), so every node has its result written
// by the fit kernels that cover its cards.
__global__ void clamp_cards_kernel(int32_t* __restrict__ n_cards, int32_t n, int32_t max_cards) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) n_cards[i] = min(n_cards[i], max_cards);
}

int pas_gas_snapshot_set_device(pas_ctx* ctx, uint64_t gen, int32_t n_nodes, int32_t max_cards,
                                int32_t n_res, const int32_t* d_n_cards,
                                const int64_t* d_cap_per_gpu, const int64_t* d_used,
                                void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = gas_shape_ok(ctx, n_nodes, max_cards, n_res);
  if (rc) return rc;
  if (n_nodes > 0 && (!d_n_cards || !d_cap_per_gpu || !d_used))
    return set_error(ctx, PAS_EINVAL, "pas_gas_snapshot_set_device: null input");
  if ((rc = activate(ctx))) return rc;
  if ((rc = gas_alloc(ctx, n_nodes, max_cards, n_res))) return rc;
  GasSnapshot& g = ctx->gas;
  hipStream_t s = pick_stream(ctx, hip_stream);
  if (n_nodes > 0) {  // device to device, into the resident arrays
    PAS_HIP(ctx, hipMemcpyAsync(g.n_cards, d_n_cards, sizeof(int32_t) * n_nodes,
                                hipMemcpyDeviceToDevice, s));
    PAS_HIP(ctx, hipMemcpyAsync(g.cap, d_cap_per_gpu, sizeof(int64_t) * n_nodes * n_res,
                                hipMemcpyDeviceToDevice, s));
    PAS_HIP(ctx, hipMemcpyAsync(g.used, d_used,
                                sizeof(int64_t) * (size_t)n_nodes * max_cards * n_res,
                                hipMemcpyDeviceToDevice, s));
    clamp_cards_kernel<<<(unsigned)((n_nodes + 255) / 256), 256, 0, s>>>(g.n_cards, n_nodes,
                                                                         max_cards);
    PAS_HIP(ctx, hipGetLastError());
  }
  g.gen = gen;
  ++g.epoch;
  g.valid = true;
  return PAS_OK;
}

// Shared host path of pas_gas_bind / pas_gas_release: validates, groups the operations by
// node (stable), uploads everything in one scratch carve and runs the walker kernel.
static int gas_commit(pas_ctx* ctx, bool release, uint64_t gen_from, uint64_t gen_to,
                      int32_t n_ops, const int32_t* op_pod, const int32_t* op_node,
                      int32_t n_pods, int32_t max_containers, int32_t i915_index,
                      const int64_t* req, const uint32_t* req_mask, const int32_t* n_containers,
                      const int32_t* cpc, const int32_t* cards, int32_t cards_stride,
                      uint32_t* res_out, int32_t* status_out, uint8_t* cards_out,
                      int32_t* nsel_out, int64_t* counts_out, const int64_t* counts,
                      const char* fn) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_gas_gen(ctx, gen_from);
  if (rc) return rc;
  const GasSnapshot& g = ctx->gas;
  const int32_t Q = g.n_res, N = g.n_nodes;
  if (n_ops < 0 || n_pods < 0 || max_containers < 0 || i915_index >= Q || i915_index < -1)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if (n_ops > 0 && (!op_pod || !op_node || !status_out || !n_containers ||
                    (max_containers > 0 && (!req || !req_mask)) ||
                    (release ? (!counts && (!cpc || !cards)) : !res_out)))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  const int32_t K = g.max_cards;
  std::vector<int32_t> order((size_t)n_ops);
  for (int32_t i = 0; i < n_ops; ++i) {
    order[(size_t)i] = i;
    if (op_node[i] < 0 || op_node[i] >= N || op_pod[i] < 0 || op_pod[i] >= n_pods)
      return set_error(ctx, PAS_EINVAL, std::string(fn) + ": node or pod index out of range");
    const int32_t p = op_pod[i];
    if ((rc = gas_pod_check(ctx, p, max_containers, req_mask, n_containers, fn))) return rc;
    // annotation cards of a release: within the card list (cards[i][cards_stride]), or per
    // container a count sum that fits int64 (counts form).  Binds have no selection limit.
    const int64_t limit = cards_stride;
    int64_t sel = 0;
    for (int32_t c = 0; release && c < n_containers[p]; ++c) {
      if (counts) {
        int64_t kc = 0;
        for (int32_t k = 0; k < K; ++k) {
          const int64_t t = counts[((int64_t)i * max_containers + c) * K + k];
          if (t < 0 || kc > INT64_MAX - t)
            return set_error(ctx, PAS_EINVAL, std::string(fn) + ": card counts negative or "
                                                               "past int64");
          kc += t;
        }
        continue;
      }
      const int64_t v = cpc[(int64_t)i * max_containers + c];
      if (v < 0) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": negative card count");
      sel = std::min(sel + std::min(v, limit + 1), limit + 1);
    }
    if (release && !counts && sel > limit)
      return set_error(ctx, PAS_EINVAL, std::string(fn) + ": more than " +
                                            std::to_string(limit) + " cards for one pod");
  }
  std::stable_sort(order.begin(), order.end(),
                   [&](int32_t a, int32_t b) { return op_node[a] < op_node[b]; });
  std::vector<uint32_t> key((size_t)n_ops);  // the sorted keys: one run per node
  for (int32_t i = 0; i < n_ops; ++i) key[(size_t)i] = (uint32_t)op_node[order[(size_t)i]];
  if ((rc = activate(ctx))) return rc;
  // (cpc and cards are a release's in its card-list form, counts a release's in its counts
  // form, res a bind's; the selections and the counts out are a bind's options)
  const size_t ops = (size_t)n_ops, C = (size_t)max_containers;
  Staging st(ctx);
  PodBatch d;
  int32_t *d_pod, *d_order, *d_cpc, *d_cards, *d_status, *d_nsel;
  uint32_t *d_key, *d_res;
  uint8_t* d_sel;
  int64_t *d_cnt_in, *d_cnt_out;
  stage_pods(st, d, n_pods, max_containers, req, req_mask, n_containers);
  st.in(d_pod, op_pod, ops);
  st.in(d_order, order.data(), ops);
  st.in(d_key, key.data(), ops);
  st.in(d_cpc, cpc, ops * C);
  st.in(d_cards, cards, ops * (size_t)cards_stride);
  st.in_opt(d_cnt_in, counts, ops * C * (size_t)K);
  st.out(d_res, release ? nullptr : res_out, ops);
  st.out_opt(d_cnt_out, counts_out, ops * C * (size_t)K);
  st.out_opt(d_sel, cards_out, ops * PAS_GAS_MAX_SELECTIONS);
  st.out_opt(d_nsel, cards_out ? nsel_out : nullptr, ops);
  st.out(d_status, status_out, ops);
  if (n_ops > 0) {
    if ((rc = st.upload())) return rc;
    if ((rc = gas_commit_launch(ctx, release, n_ops, i915_index, d_order, d_key, d_pod, d, d_cpc,
                                d_cards, cards_stride, d_res, d_status, d_sel, d_nsel, d_cnt_out,
                                d_cnt_in, ctx->stream)))
      return rc;
  }
  rc = n_ops > 0 ? st.fetch_results(fn) : PAS_OK;
  return gas_finish(ctx, rc, rc != PAS_OK, gen_to);
}

int pas_gas_bind(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_binds,
                 const int32_t* bind_pod, const int32_t* bind_node, int32_t n_pods,
                 int32_t max_containers, int32_t i915_index, const int64_t* req,
                 const uint32_t* req_mask, const int32_t* n_containers, uint32_t* res_out,
                 int32_t* status_out) {
  return gas_commit(ctx, false, gen_from, gen_to, n_binds, bind_pod, bind_node, n_pods,
                    max_containers, i915_index, req, req_mask, n_containers, nullptr, nullptr,
                    PAS_GAS_PACKED, res_out, status_out, nullptr, nullptr, nullptr, nullptr,
                    "pas_gas_bind");
}

int pas_gas_bind_ex(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_binds,
                    const int32_t* bind_pod, const int32_t* bind_node, int32_t n_pods,
                    int32_t max_containers, int32_t i915_index, const int64_t* req,
                    const uint32_t* req_mask, const int32_t* n_containers, uint32_t* res_out,
                    int32_t* status_out, uint8_t* cards_out, int32_t* n_sel_out) {
  if (!ctx) return PAS_EINVAL;
  if (n_binds > 0 && (!cards_out || !n_sel_out))
    return set_error(ctx, PAS_EINVAL, "pas_gas_bind_ex: null input");
  return gas_commit(ctx, false, gen_from, gen_to, n_binds, bind_pod, bind_node, n_pods,
                    max_containers, i915_index, req, req_mask, n_containers, nullptr, nullptr,
                    PAS_GAS_PACKED, res_out, status_out, n_binds > 0 ? cards_out : nullptr,
                    n_sel_out, nullptr, nullptr, "pas_gas_bind_ex");
}

int pas_gas_bind_counts(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_binds,
                        const int32_t* bind_pod, const int32_t* bind_node, int32_t n_pods,
                        int32_t max_containers, int32_t i915_index, const int64_t* req,
                        const uint32_t* req_mask, const int32_t* n_containers,
                        uint32_t* res_out, int32_t* status_out, int64_t* counts_out) {
  if (!ctx) return PAS_EINVAL;
  if (n_binds > 0 && max_containers > 0 && !counts_out)
    return set_error(ctx, PAS_EINVAL, "pas_gas_bind_counts: null input");
  return gas_commit(ctx, false, gen_from, gen_to, n_binds, bind_pod, bind_node, n_pods,
                    max_containers, i915_index, req, req_mask, n_containers, nullptr, nullptr,
                    PAS_GAS_PACKED, res_out, status_out, nullptr, nullptr,
                    n_binds > 0 && max_containers > 0 ? counts_out : nullptr, nullptr,
                    "pas_gas_bind_counts");
}

int pas_gas_release(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_releases,
                    const int32_t* rel_pod, const int32_t* rel_node, int32_t n_pods,
                    int32_t max_containers, const int64_t* req, const uint32_t* req_mask,
                    const int32_t* n_containers, const int32_t* cards_per_container,
                    const int32_t* cards, int32_t* status_out) {
  return gas_commit(ctx, true, gen_from, gen_to, n_releases, rel_pod, rel_node, n_pods,
                    max_containers, -1, req, req_mask, n_containers, cards_per_container, cards,
                    PAS_GAS_PACKED, nullptr, status_out, nullptr, nullptr, nullptr, nullptr,
                    "pas_gas_release");
}

int pas_gas_release_ex(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_releases,
                       const int32_t* rel_pod, const int32_t* rel_node, int32_t n_pods,
                       int32_t max_containers, const int64_t* req, const uint32_t* req_mask,
                       const int32_t* n_containers, const int32_t* cards_per_container,
                       const int32_t* cards, int32_t* status_out) {
  return gas_commit(ctx, true, gen_from, gen_to, n_releases, rel_pod, rel_node, n_pods,
                    max_containers, -1, req, req_mask, n_containers, cards_per_container, cards,
                    PAS_GAS_MAX_SELECTIONS, nullptr, status_out, nullptr, nullptr, nullptr,
                    nullptr, "pas_gas_release_ex");
}

int pas_gas_release_counts(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                           int32_t n_releases, const int32_t* rel_pod, const int32_t* rel_node,
                           int32_t n_pods, int32_t max_containers, const int64_t* req,
                           const uint32_t* req_mask, const int32_t* n_containers,
                           const int64_t* counts, int32_t* status_out) {
  if (!ctx) return PAS_EINVAL;
  if (n_releases > 0 && max_containers > 0 && !counts)
    return set_error(ctx, PAS_EINVAL, "pas_gas_release_counts: null input");
  static const int64_t kNone = 0;  // no containers: nothing to read
  return gas_commit(ctx, true, gen_from, gen_to, n_releases, rel_pod, rel_node, n_pods,
                    max_containers, -1, req, req_mask, n_containers, nullptr, nullptr, 1,
                    nullptr, status_out, nullptr, nullptr, nullptr, counts ? counts : &kNone,
                    "pas_gas_release_counts");
}

// What pas_gas_apply and pas_gas_apply_device share: the checks a host can make on either
// form's scalars and pointers.
static int gas_apply_check(pas_ctx* ctx, uint64_t gen_from, int32_t n_events, const void* ev_kind,
                           const void* ev_pod, const void* ev_node, int32_t n_pods,
                           int32_t max_containers, const void* req, const void* req_mask,
                           const void* n_containers, const void* cpc, const void* cards,
                           int32_t cards_ld, const void* status_out, const char* fn) {
  int rc = check_gas_gen(ctx, gen_from);
  if (rc) return rc;
  if (n_events < 0 || n_pods < 0 || max_containers < 0 || cards_ld < 1)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if (n_events > 0 && (!ev_kind || !ev_pod || !ev_node || !status_out || !cards ||
                       (n_pods > 0 && !n_containers) ||
                       (max_containers > 0 && (!cpc || (n_pods > 0 && (!req || !req_mask))))))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  return PAS_OK;
}

int pas_gas_apply_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_events,
                         const int32_t* d_ev_kind, const int32_t* d_ev_pod,
                         const int32_t* d_ev_node, int32_t n_pods, int32_t max_containers,
                         const int64_t* d_req, const uint32_t* d_req_mask,
                         const int32_t* d_n_containers, const int32_t* d_cards_per_container,
                         const int32_t* d_cards, int32_t cards_ld, int32_t* d_status_out,
                         void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = gas_apply_check(ctx, gen_from, n_events, d_ev_kind, d_ev_pod, d_ev_node, n_pods,
                           max_containers, d_req, d_req_mask, d_n_containers,
                           d_cards_per_container, d_cards, cards_ld, d_status_out,
                           "pas_gas_apply_device");
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  const PodBatch pods{n_pods, max_containers, d_req, d_req_mask, d_n_containers};
  rc = gas_apply_launch(ctx, n_events, d_ev_kind, d_ev_pod, d_ev_node, pods,
                        d_cards_per_container, d_cards, cards_ld, d_status_out,
                        pick_stream(ctx, hip_stream));
  return gas_finish(ctx, rc, false, gen_to);
}

int pas_gas_apply(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_events,
                  const int32_t* ev_kind, const int32_t* ev_pod, const int32_t* ev_node,
                  int32_t n_pods, int32_t max_containers, const int64_t* req,
                  const uint32_t* req_mask, const int32_t* n_containers,
                  const int32_t* cards_per_container, const int32_t* cards, int32_t cards_ld,
                  int32_t* status_out) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_apply";
  int rc = gas_apply_check(ctx, gen_from, n_events, ev_kind, ev_pod, ev_node, n_pods,
                           max_containers, req, req_mask, n_containers, cards_per_container,
                           cards, cards_ld, status_out, fn.c_str());
  if (rc) return rc;
  const int32_t N = ctx->gas.n_nodes;
  for (int32_t e = 0; e < n_events; ++e) {
    if (ev_kind[e] != PAS_GAS_EV_ADD && ev_kind[e] != PAS_GAS_EV_REMOVE)
      return set_error(ctx, PAS_EINVAL, fn + ": event kind out of range");
    if (ev_node[e] < 0 || ev_node[e] >= N || ev_pod[e] < 0 || ev_pod[e] >= n_pods)
      return set_error(ctx, PAS_EINVAL, fn + ": node or pod index out of range");
    const int32_t p = ev_pod[e];
    if ((rc = gas_pod_check(ctx, p, max_containers, req_mask, n_containers, fn.c_str())))
      return rc;
    int64_t sel = 0;
    for (int32_t c = 0; c < n_containers[p]; ++c) {
      const int64_t v = cards_per_container[(int64_t)e * max_containers + c];
      if (v < 0) return set_error(ctx, PAS_EINVAL, fn + ": negative card count");
      sel += v;  // at most max_containers * INT32_MAX
    }
    if (sel > cards_ld)
      return set_error(ctx, PAS_EINVAL, fn + ": more than cards_ld cards for one pod");
  }
  if ((rc = activate(ctx))) return rc;
  const size_t E = (size_t)n_events;
  Staging st(ctx);
  PodBatch d;
  int32_t *d_kind, *d_pod, *d_node, *d_cpc, *d_cards, *d_status;
  stage_pods(st, d, n_pods, max_containers, req, req_mask, n_containers);
  st.in(d_kind, ev_kind, E);
  st.in(d_pod, ev_pod, E);
  st.in(d_node, ev_node, E);
  st.in(d_cpc, cards_per_container, E * (size_t)max_containers);
  st.in(d_cards, cards, E * (size_t)cards_ld);
  st.out(d_status, status_out, E);
  if (n_events > 0) {
    if ((rc = st.upload())) return rc;
    // the _device form's path: grouping and commit on the device
    if ((rc = gas_apply_launch(ctx, n_events, d_kind, d_pod, d_node, d, d_cpc, d_cards, cards_ld,
                               d_status, ctx->stream)))
      return rc;
  }
  rc = n_events > 0 ? st.fetch_results(fn) : PAS_OK;
  return gas_finish(ctx, rc, rc != PAS_OK, gen_to);
}

// What pas_gas_place and pas_gas_place_device share: the checks a host can make on either
// form's scalars and pointers.
static int gas_place_check(pas_ctx* ctx, uint64_t gen_from, int32_t n_pods,
                           int32_t max_containers, int32_t i915_index, const void* req,
                           const void* req_mask, const void* n_containers, int32_t k, int32_t ld,
                           const void* cand_node, const void* place_node, const void* place_rank,
                           const void* res_out, const void* cards_out, const void* n_sel_out,
                           const char* fn) {
  int rc = check_gas_gen(ctx, gen_from);
  if (rc) return rc;
  if (n_pods < 0 || max_containers < 0 || i915_index >= ctx->gas.n_res || i915_index < -1 ||
      k < 1 || ld < k)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if ((cards_out == nullptr) != (n_sel_out == nullptr))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": cards_out and n_sel_out go together");
  if (n_pods > 0 && (!n_containers || !cand_node || !place_node || !place_rank || !res_out ||
                     (max_containers > 0 && (!req || !req_mask))))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  return PAS_OK;
}

int pas_gas_place_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_pods,
                         int32_t max_containers, int32_t i915_index, const int64_t* d_req,
                         const uint32_t* d_req_mask, const int32_t* d_n_containers, int32_t k,
                         int32_t ld, int32_t node_base, const int32_t* d_cand_node,
                         const int32_t* d_cand_len, int32_t* d_place_node,
                         int32_t* d_place_rank, uint32_t* d_res_out, uint8_t* d_cards_out,
                         int32_t* d_n_sel_out, int64_t* d_counts_out, int32_t* n_placed,
                         int32_t* n_rounds, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = gas_place_check(ctx, gen_from, n_pods, max_containers, i915_index, d_req, d_req_mask,
                           d_n_containers, k, ld, d_cand_node, d_place_node, d_place_rank,
                           d_res_out, d_cards_out, d_n_sel_out, "pas_gas_place_device");
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  bool began = false;
  const PodBatch pods{n_pods, max_containers, d_req, d_req_mask, d_n_containers};
  rc = gas_place_launch(ctx, i915_index, pods, k, ld, node_base, d_cand_node, d_cand_len,
                        d_place_node, d_place_rank, d_res_out, d_cards_out, d_n_sel_out,
                        d_counts_out, n_placed, n_rounds, &began, pick_stream(ctx, hip_stream));
  // (a failure after commits began leaves no valid snapshot behind: a device error)
  if (rc && began && rc != PAS_EDEVICE) rc = set_error(ctx, PAS_EDEVICE, ctx->err);
  return gas_finish(ctx, rc, began, gen_to);
}

int pas_gas_place(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_pods,
                  int32_t max_containers, int32_t i915_index, const int64_t* req,
                  const uint32_t* req_mask, const int32_t* n_containers, int32_t k, int32_t ld,
                  int32_t node_base, const int32_t* cand_node, const int32_t* cand_len,
                  int32_t* place_node, int32_t* place_rank, uint32_t* res_out,
                  uint8_t* cards_out, int32_t* n_sel_out, int64_t* counts_out,
                  int32_t* n_placed, int32_t* n_rounds) {
  if (!ctx) return PAS_EINVAL;
  const char* fn = "pas_gas_place";
  int rc = gas_place_check(ctx, gen_from, n_pods, max_containers, i915_index, req, req_mask,
                           n_containers, k, ld, cand_node, place_node, place_rank, res_out,
                           cards_out, n_sel_out, fn);
  if (rc) return rc;
  for (int32_t p = 0; p < n_pods; ++p)
    if ((rc = gas_pod_check(ctx, p, max_containers, req_mask, n_containers, fn))) return rc;
  if ((rc = activate(ctx))) return rc;
  const size_t P = (size_t)n_pods, C = (size_t)max_containers;
  Staging st(ctx);
  PodBatch d;
  int32_t *d_cand, *d_len, *d_node, *d_rank, *d_nsel;
  uint32_t* d_res;
  uint8_t* d_sel;
  int64_t* d_cnt;
  stage_pods(st, d, n_pods, max_containers, req, req_mask, n_containers);
  st.in(d_cand, cand_node, P * (size_t)ld);
  st.in_opt(d_len, cand_len, P);
  st.out(d_node, place_node, P);
  st.out(d_rank, place_rank, P);
  st.out(d_res, res_out, P);
  st.out_opt(d_sel, cards_out, P * PAS_GAS_MAX_SELECTIONS);
  st.out_opt(d_nsel, n_sel_out, P);
  st.out_opt(d_cnt, C > 0 ? counts_out : nullptr, P * C * (size_t)ctx->gas.max_cards);
  if ((rc = st.upload())) return rc;
  bool began = false;
  rc = gas_place_launch(ctx, i915_index, d, k, ld, node_base, d_cand, d_len, d_node, d_rank,
                        d_res, d_sel, d_nsel, d_cnt, n_placed, n_rounds, &began, ctx->stream);
  if (!rc && n_pods > 0) rc = st.fetch_results(fn);
  if (rc && began && rc != PAS_EDEVICE) rc = set_error(ctx, PAS_EDEVICE, ctx->err);
  return gas_finish(ctx, rc, began, gen_to);
}

int pas_gas_snapshot_get(pas_ctx* ctx, uint64_t* gen, int64_t* used_out) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->gas.valid) return set_error(ctx, PAS_ENOSNAP, "no GAS snapshot uploaded");
  const GasSnapshot& g = ctx->gas;
  const size_t b = sizeof(int64_t) * (size_t)g.n_nodes * g.max_cards * g.n_res;
  if (b && !used_out) return set_error(ctx, PAS_EINVAL, "pas_gas_snapshot_get: null output");
  int rc = activate(ctx);
  if (rc) return rc;
  // (out of the resident array, not scratch: no Staging)
  if (b) PAS_HIP(ctx, hipMemcpyAsync(used_out, g.used, b, hipMemcpyDeviceToHost, ctx->stream));
  PAS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (gen) *gen = g.gen;
  return PAS_OK;
}

int pas_gas_snapshot_info(const pas_ctx* ctx, uint64_t* gen, int32_t* n_nodes, int32_t* max_cards,
                          int32_t* n_res) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->gas.valid) return PAS_ENOSNAP;
  if (gen) *gen = ctx->gas.gen;
  if (n_nodes) *n_nodes = ctx->gas.n_nodes;
  if (max_cards) *max_cards = ctx->gas.max_cards;
  if (n_res) *n_res = ctx->gas.n_res;
  return PAS_OK;
}

int pas_gas_snapshot_get_nodes(pas_ctx* ctx, uint64_t* gen, int32_t* n_cards_out,
                               int64_t* cap_out) {
  if (!ctx) return PAS_EINVAL;
  if (!ctx->gas.valid) return set_error(ctx, PAS_ENOSNAP, "no GAS snapshot uploaded");
  const GasSnapshot& g = ctx->gas;
  const size_t N = (size_t)g.n_nodes;
  if (N && (!n_cards_out || !cap_out))
    return set_error(ctx, PAS_EINVAL, "pas_gas_snapshot_get_nodes: null output");
  int rc = activate(ctx);
  if (rc) return rc;
  if (N) {  // out of the resident arrays, not scratch: no Staging
    PAS_HIP(ctx, hipMemcpyAsync(n_cards_out, g.n_cards, sizeof(int32_t) * N,
                                hipMemcpyDeviceToHost, ctx->stream));
    PAS_HIP(ctx, hipMemcpyAsync(cap_out, g.cap, sizeof(int64_t) * N * g.n_res,
                                hipMemcpyDeviceToHost, ctx->stream));
  }
  PAS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (gen) *gen = g.gen;
  return PAS_OK;
}

// What pas_gas_nodes_update and pas_gas_nodes_update_device share: the checks a host can make
// on either form's scalars and pointers.
static int gas_nodes_check(pas_ctx* ctx, uint64_t gen_from, int32_t n_updates,
                           const void* upd_node, const void* upd_n_cards, const void* upd_cap,
                           const void* upd_src, const void* status_out, const char* fn) {
  int rc = check_gas_gen(ctx, gen_from);
  if (rc) return rc;
  if (n_updates < 0) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if (n_updates > 0 && (!upd_node || !upd_n_cards || !upd_cap || !upd_src || !status_out))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  return PAS_OK;
}

int pas_gas_nodes_update_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                int32_t n_updates, const int32_t* d_upd_node,
                                const int32_t* d_upd_n_cards, const int64_t* d_upd_cap,
                                const int32_t* d_upd_src, int32_t* d_status_out,
                                void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = gas_nodes_check(ctx, gen_from, n_updates, d_upd_node, d_upd_n_cards, d_upd_cap,
                           d_upd_src, d_status_out, "pas_gas_nodes_update_device");
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  rc = gas_nodes_update_launch(ctx, n_updates, d_upd_node, d_upd_n_cards, d_upd_cap, d_upd_src,
                               d_status_out, pick_stream(ctx, hip_stream));
  return gas_finish(ctx, rc, false, gen_to);
}

int pas_gas_nodes_update(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_updates,
                         const int32_t* upd_node, const int32_t* upd_n_cards,
                         const int64_t* upd_cap, const int32_t* upd_src, int32_t* status_out) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_gas_nodes_update";
  int rc = gas_nodes_check(ctx, gen_from, n_updates, upd_node, upd_n_cards, upd_cap, upd_src,
                           status_out, fn.c_str());
  if (rc) return rc;
  const int32_t N = ctx->gas.n_nodes, K = ctx->gas.max_cards, Q = ctx->gas.n_res;
  for (int32_t u = 0; u < n_updates; ++u) {
    if (upd_node[u] < 0 || upd_node[u] >= N)
      return set_error(ctx, PAS_EINVAL, fn + ": node index out of range");
    if (upd_n_cards[u] < -1 || upd_n_cards[u] > K)
      return set_error(ctx, PAS_EINVAL, fn + ": n_cards outside [-1, max_cards]");
    uint64_t seen = 0;  // K <= 64 source slots
    for (int32_t k = 0; k < K; ++k) {
      const int32_t s = upd_src[(int64_t)u * K + k];
      if (s < 0) continue;
      if (s >= K) return set_error(ctx, PAS_EINVAL, fn + ": src >= max_cards");
      if (seen >> s & 1) return set_error(ctx, PAS_EINVAL, fn + ": a src slot repeats in a row");
      seen |= uint64_t(1) << s;
    }
  }
  if ((rc = activate(ctx))) return rc;
  const size_t U = (size_t)n_updates;
  Staging st(ctx);
  int32_t *d_node, *d_nc, *d_src, *d_status;
  int64_t* d_cap;
  st.in(d_node, upd_node, U);
  st.in(d_nc, upd_n_cards, U);
  st.in(d_cap, upd_cap, U * (size_t)Q);
  st.in(d_src, upd_src, U * (size_t)K);
  st.out(d_status, status_out, U);
  if (n_updates > 0) {
    if ((rc = st.upload())) return rc;
    // the _device form's path: grouping and the rows' rewrite on the device
    if ((rc = gas_nodes_update_launch(ctx, n_updates, d_node, d_nc, d_cap, d_src, d_status,
                                      ctx->stream)))
      return rc;
  }
  rc = n_updates > 0 ? st.fetch_results(fn) : PAS_OK;
  return gas_finish(ctx, rc, rc != PAS_OK, gen_to);
}

// The resident snapshot moved into new storage of n_nodes_new x max_cards_new, for the calls
// that change its shape: fill(n_cards, cap, used, derived) launches the copy on s (derived: the
// new storage for the fit's derived values, unset until the next fit, free as staging).  The
// old storage is freed after s and the context's stream are idle.
using GasFill = std::function<int(int32_t*, int64_t*, int64_t*, void*)>;
static int gas_restore(pas_ctx* ctx, uint64_t gen_to, int32_t n_nodes_new, int32_t max_cards_new,
                       hipStream_t s, const char* fn, const GasFill& fill) {
  GasSnapshot& g = ctx->gas;
  const size_t nn = (size_t)std::max(n_nodes_new, 1), Q = (size_t)g.n_res;
  int32_t* n_cards = nullptr;
  int64_t *cap = nullptr, *used = nullptr;
  void *derived = nullptr, *free_t = nullptr;
  int rc = PAS_OK;
  hipError_t e = hipMalloc(&n_cards, sizeof(int32_t) * nn);
  if (e == hipSuccess) e = hipMalloc(&cap, sizeof(int64_t) * nn * Q);
  if (e == hipSuccess) e = hipMalloc(&used, sizeof(int64_t) * nn * (size_t)max_cards_new * Q);
  if (e == hipSuccess) e = hipMalloc(&derived, 64 + sizeof(int32_t) * nn);
  if (e == hipSuccess) e = hipMalloc(&free_t, sizeof(int64_t) * PAS_GAS_PACKED * Q * nn);
  if (e == hipSuccess) {
    rc = fill(n_cards, cap, used, derived);
    // the old storage is freed below: its readers (the copy, and earlier calls of the host
    // forms on the context's stream) have finished by then
    if (!rc) e = hipStreamSynchronize(s);
    if (!rc && e == hipSuccess && s != ctx->stream) e = hipStreamSynchronize(ctx->stream);
  }
  if (rc || e != hipSuccess) {  // the resident snapshot was only read: it stays as it is
    for (void* p : {(void*)n_cards, (void*)cap, (void*)used, derived, free_t})
      if (p) (void)hipFree(p);
    return rc ? rc : check_hip(ctx, e, fn);
  }
  free_ptr(reinterpret_cast<void*&>(g.n_cards));
  free_ptr(reinterpret_cast<void*&>(g.cap));
  free_ptr(reinterpret_cast<void*&>(g.used));
  free_ptr(g.derived);
  free_ptr(g.free_t);
  g.n_cards = n_cards;
  g.cap = cap;
  g.used = used;
  g.derived = derived;
  g.free_t = free_t;
  g.n_nodes = n_nodes_new;
  g.max_cards = max_cards_new;
  g.gen = gen_to;
  ++g.epoch;  // the next fit derives its values again, into the new storage
  return PAS_OK;
}

int pas_gas_snapshot_resize(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                            int32_t n_nodes_new, int32_t max_cards_new, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_gas_gen(ctx, gen_from);
  if (rc) return rc;
  GasSnapshot& g = ctx->gas;
  if (n_nodes_new < g.n_nodes || max_cards_new < g.max_cards)
    return set_error(ctx, PAS_EINVAL, "pas_gas_snapshot_resize: the snapshot only grows");
  if (max_cards_new > PAS_GAS_MAX_CARDS)
    return set_error(ctx, PAS_ECAPACITY, "pas_gas_snapshot_resize: max_cards <= 64 supported");
  if (n_nodes_new == g.n_nodes && max_cards_new == g.max_cards) {
    g.gen = gen_to;
    return PAS_OK;
  }
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  return gas_restore(ctx, gen_to, n_nodes_new, max_cards_new, s, "pas_gas_snapshot_resize",
                     [&](int32_t* n_cards, int64_t* cap, int64_t* used, void*) {
                       return gas_repitch_launch(ctx, n_nodes_new, max_cards_new, n_cards, cap,
                                                 used, s);
                     });
}

int pas_gas_snapshot_compact(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                             int32_t n_nodes_new, const int32_t* src_node, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const char* fn = "pas_gas_snapshot_compact";
  int rc = check_gas_gen(ctx, gen_from);
  if (rc) return rc;
  GasSnapshot& g = ctx->gas;
  bool identity;
  if ((rc = check_node_map(ctx, g.n_nodes, n_nodes_new, src_node, fn, &identity))) return rc;
  if (identity) {  // every row in place
    g.gen = gen_to;
    return PAS_OK;
  }
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  return gas_restore(ctx, gen_to, n_nodes_new, g.max_cards, s, fn,
                     [&](int32_t* n_cards, int64_t* cap, int64_t* used, void* derived) {
                       if (n_nodes_new == 0) return (int)PAS_OK;
                       // the map rides in the new derived storage; src_node is the caller's
                       // again once s has been synchronized
                       int32_t* d_src = static_cast<int32_t*>(derived);
                       PAS_HIP(ctx, hipMemcpyAsync(d_src, src_node,
                                                   sizeof(int32_t) * (size_t)n_nodes_new,
                                                   hipMemcpyHostToDevice, s));
                       return gas_compact_launch(ctx, n_nodes_new, d_src, n_cards, cap, used, s);
                     });
}

// Host path of pas_gas_fit / pas_gas_fit_ex: validates, uploads the batch, runs the fit and
// copies the words (and side records) back.
static int gas_fit_host(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                        int32_t i915_index, const int64_t* req, const uint32_t* req_mask,
                        const int32_t* n_containers, uint32_t* res_out,
                        pas_gas_selection* side, int64_t side_cap, int64_t* side_count,
                        const char* fn) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_gas_gen(ctx, gen);
  if (rc) return rc;
  const int32_t Q = ctx->gas.n_res;
  if (n_pods < 0 || max_containers < 0 || i915_index >= Q || i915_index < -1 || side_cap < 0)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if (side_count) *side_count = 0;
  if (n_pods == 0) return PAS_OK;
  if (!n_containers || !res_out || (max_containers > 0 && (!req || !req_mask)) ||
      (side_cap > 0 && !side))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  // Validate the batch (no limit on card selections: see PAS_GAS_SEL_LIMIT)
  for (int32_t p = 0; p < n_pods; ++p)
    if ((rc = gas_pod_check(ctx, p, max_containers, req_mask, n_containers, fn))) return rc;
  if ((rc = activate(ctx))) return rc;
  const int64_t N = ctx->gas.n_nodes;
  int64_t count = 0;
  Staging st(ctx);
  PodBatch d;
  uint32_t* d_res;
  pas_gas_selection* d_side;
  int64_t* d_count;
  stage_pods(st, d, n_pods, max_containers, req, req_mask, n_containers);
  st.out(d_res, res_out, (size_t)n_pods * (size_t)N);
  st.work(d_side, (size_t)side_cap);  // (fetched below, once the count is known)
  st.out_opt(d_count, side_count ? &count : nullptr, 1);
  if ((rc = st.upload())) return rc;
  rc = gas_fit_launch(ctx, i915_index, d, d_res, N, nullptr, side_cap > 0 ? d_side : nullptr,
                      side_cap, d_count, ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  // a side-stream wait of this fit that gave up: its words are incomplete
  if ((rc = gas_fault_check(ctx))) return rc;
  if (side_count) {
    *side_count = count;
    // the records the fit produced, not the capacity: a blocking copy outside st
    const int64_t got = std::min(count, side_cap);
    if (got > 0)
      PAS_HIP(ctx, hipMemcpy(side, d_side, sizeof(pas_gas_selection) * (size_t)got,
                             hipMemcpyDeviceToHost));
  }
  return PAS_OK;
}

int pas_gas_fit(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                int32_t i915_index, const int64_t* req, const uint32_t* req_mask,
                const int32_t* n_containers, uint32_t* res_out) {
  return gas_fit_host(ctx, gen, n_pods, max_containers, i915_index, req, req_mask, n_containers,
                      res_out, nullptr, 0, nullptr, "pas_gas_fit");
}

int pas_gas_fit_ex(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                   int32_t i915_index, const int64_t* req, const uint32_t* req_mask,
                   const int32_t* n_containers, uint32_t* res_out, pas_gas_selection* side,
                   int64_t side_cap, int64_t* side_count) {
  if (!ctx) return PAS_EINVAL;
  if (!side_count) return set_error(ctx, PAS_EINVAL, "pas_gas_fit_ex: null side_count");
  return gas_fit_host(ctx, gen, n_pods, max_containers, i915_index, req, req_mask, n_containers,
                      res_out, side, side_cap, side_count, "pas_gas_fit_ex");
}

static int gas_fit_device_common(pas_ctx* ctx, uint64_t gen, int32_t n_pods,
                                 int32_t max_containers, int32_t i915_index,
                                 const int64_t* d_req, const uint32_t* d_req_mask,
                                 const int32_t* d_n_containers, uint32_t* d_res_out,
                                 int64_t ld_res, uint64_t* d_fit_out, pas_gas_selection* d_side,
                                 int64_t side_cap, int64_t* d_side_count, void* hip_stream,
                                 const char* fn) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_gas_gen(ctx, gen);
  if (rc) return rc;
  if (ld_res < 0) ld_res = ctx->gas.n_nodes;  // dense rows
  if (n_pods < 0 || max_containers < 0 || i915_index >= ctx->gas.n_res || i915_index < -1 ||
      side_cap < 0 || ld_res < ctx->gas.n_nodes)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if (n_pods > 0 && (!d_n_containers || (!d_res_out && !d_fit_out) ||
                     (max_containers > 0 && (!d_req || !d_req_mask)) || (side_cap > 0 && !d_side)))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  if ((rc = activate(ctx))) return rc;
  const PodBatch pods{n_pods, max_containers, d_req, d_req_mask, d_n_containers};
  return gas_fit_launch(ctx, i915_index, pods, d_res_out, ld_res, d_fit_out,
                        side_cap > 0 ? d_side : nullptr, side_cap, d_side_count,
                        pick_stream(ctx, hip_stream));
}

int pas_gas_fit_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                       int32_t i915_index, const int64_t* d_req, const uint32_t* d_req_mask,
                       const int32_t* d_n_containers, uint32_t* d_res_out, void* hip_stream) {
  if (ctx && !d_res_out && n_pods > 0)
    return set_error(ctx, PAS_EINVAL, "pas_gas_fit_device: null input");
  return gas_fit_device_common(ctx, gen, n_pods, max_containers, i915_index, d_req, d_req_mask,
                               d_n_containers, d_res_out, -1, nullptr, nullptr, 0, nullptr,
                               hip_stream, "pas_gas_fit_device");
}

int pas_gas_fit_ex_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                          int32_t i915_index, const int64_t* d_req, const uint32_t* d_req_mask,
                          const int32_t* d_n_containers, uint32_t* d_res_out,
                          pas_gas_selection* d_side, int64_t side_cap, int64_t* d_side_count,
                          void* hip_stream) {
  if (ctx && ((!d_res_out && n_pods > 0) || !d_side_count))
    return set_error(ctx, PAS_EINVAL, "pas_gas_fit_ex_device: null input");
  return gas_fit_device_common(ctx, gen, n_pods, max_containers, i915_index, d_req, d_req_mask,
                               d_n_containers, d_res_out, -1, nullptr, d_side, side_cap,
                               d_side_count, hip_stream, "pas_gas_fit_ex_device");
}

int pas_gas_fit_ld_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                          int32_t i915_index, const int64_t* d_req, const uint32_t* d_req_mask,
                          const int32_t* d_n_containers, uint32_t* d_res_out, int64_t ld_res,
                          pas_gas_selection* d_side, int64_t side_cap, int64_t* d_side_count,
                          void* hip_stream) {
  if (ctx && !d_res_out && n_pods > 0)
    return set_error(ctx, PAS_EINVAL, "pas_gas_fit_ld_device: null input");
  if (ctx && ld_res < 0) return set_error(ctx, PAS_EINVAL, "pas_gas_fit_ld_device: ld_res < 0");
  return gas_fit_device_common(ctx, gen, n_pods, max_containers, i915_index, d_req, d_req_mask,
                               d_n_containers, d_res_out, ld_res, nullptr, d_side, side_cap,
                               d_side_count, hip_stream, "pas_gas_fit_ld_device");
}

int pas_gas_limit_count(pas_ctx* ctx, int64_t* n_pods_out) {
  if (!ctx) return PAS_EINVAL;
  if (!n_pods_out) return set_error(ctx, PAS_EINVAL, "pas_gas_limit_count: null output");
  *n_pods_out = 0;
  if (ctx->gas_last_slot < 0) return PAS_OK;  // no fit on this context yet
  const AuxSlot& a = ctx->aux_slot[ctx->gas_last_slot];
  int rc = activate(ctx);
  if (rc) return rc;
  PAS_HIP(ctx, hipEventSynchronize(a.ev));
  PAS_HIP(ctx, hipMemcpy(n_pods_out, a.gas_limit, sizeof(int64_t), hipMemcpyDeviceToHost));
  return PAS_OK;
}

int pas_gas_fit_bitmap_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                              int32_t i915_index, const int64_t* d_req,
                              const uint32_t* d_req_mask, const int32_t* d_n_containers,
                              uint64_t* d_fit_out, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_gas_gen(ctx, gen);
  if (rc) return rc;
  if (n_pods < 0 || max_containers < 0 || i915_index >= ctx->gas.n_res || i915_index < -1)
    return set_error(ctx, PAS_EINVAL, "pas_gas_fit_bitmap_device: bad shape");
  if (n_pods > 0 && !d_fit_out)
    return set_error(ctx, PAS_EINVAL, "pas_gas_fit_bitmap_device: null input");
  return gas_fit_device_common(ctx, gen, n_pods, max_containers, i915_index, d_req, d_req_mask,
                               d_n_containers, nullptr, -1, d_fit_out, nullptr, 0, nullptr,
                               hip_stream, "pas_gas_fit_bitmap_device");
}

// What the two forms of pas_gas_fit_requests check alike; *longest = the longest request.
static int check_gas_requests(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                              const int32_t* req_off, const void* req_node,
                              int32_t max_containers, int32_t i915_index, const void* req,
                              const void* req_mask, const void* n_containers, const void* fit,
                              int64_t ld_words, const char* fn, int32_t* longest) {
  int rc = check_gas_gen(ctx, gen);
  if (rc) return rc;
  if (max_containers < 0 || i915_index >= ctx->gas.n_res || i915_index < -1)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if ((rc = check_requests(ctx, n_requests, req_off, req_node, fn, longest))) return rc;
  if (n_requests == 0) return PAS_OK;
  if ((rc = check_request_rows(ctx, *longest, fit, ld_words, fn))) return rc;
  if (!n_containers || (max_containers > 0 && (!req || !req_mask)))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  return PAS_OK;
}

int pas_gas_fit_requests(pas_ctx* ctx, uint64_t gen, int32_t n_requests, const int32_t* req_off,
                         const int32_t* req_node, int32_t max_containers, int32_t i915_index,
                         const int64_t* req, const uint32_t* req_mask,
                         const int32_t* n_containers, uint64_t* fit_out, int64_t ld_words) {
  const char* fn = "pas_gas_fit_requests";
  if (!ctx) return PAS_EINVAL;
  int32_t longest = 0;
  int rc = check_gas_requests(ctx, gen, n_requests, req_off, req_node, max_containers,
                              i915_index, req, req_mask, n_containers, fit_out, ld_words, fn,
                              &longest);
  if (rc || n_requests == 0) return rc;
  for (int32_t p = 0; p < n_requests; ++p)
    if ((rc = gas_pod_check(ctx, p, max_containers, req_mask, n_containers, fn))) return rc;
  if (longest == 0) return PAS_OK;
  if ((rc = activate(ctx))) return rc;
  const int64_t ld_dev = w64(longest);
  std::vector<uint64_t> rows((size_t)(n_requests * ld_dev));
  Staging st(ctx);
  PodBatch d;
  int32_t* d_node;
  uint64_t* d_rows;
  st.in(d_node, req_node, (size_t)req_off[n_requests]);
  stage_pods(st, d, n_requests, max_containers, req, req_mask, n_containers);
  st.out(d_rows, rows.data(), rows.size());
  if ((rc = st.upload())) return rc;
  hipStream_t s = ctx->stream;
  HostStage stage;  // (req_off is the caller's until fetch_request_rows has synchronized)
  if ((rc = gas_fit_requests_launch(ctx, n_requests, req_off, d_node, i915_index, d, d_rows,
                                    ld_dev, &stage, s))) {
    (void)hipStreamSynchronize(s);  // the copy of req_off may be in flight
    return rc;
  }
  return fetch_request_rows(ctx, st, n_requests, req_off, rows, ld_dev, fit_out, ld_words);
}

int pas_gas_fit_requests_device(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                const int32_t* req_off, const int32_t* d_req_node,
                                int32_t max_containers, int32_t i915_index, const int64_t* d_req,
                                const uint32_t* d_req_mask, const int32_t* d_n_containers,
                                uint64_t* d_fit_out, int64_t ld_words, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int32_t longest = 0;
  int rc = check_gas_requests(ctx, gen, n_requests, req_off, d_req_node, max_containers,
                              i915_index, d_req, d_req_mask, d_n_containers, d_fit_out, ld_words,
                              "pas_gas_fit_requests_device", &longest);
  if (rc || n_requests == 0) return rc;
  if ((rc = activate(ctx))) return rc;
  const PodBatch pods{n_requests, max_containers, d_req, d_req_mask, d_n_containers};
  return gas_fit_requests_launch(ctx, n_requests, req_off, d_req_node, i915_index, pods,
                                 d_fit_out, ld_words, nullptr, pick_stream(ctx, hip_stream));
}

// --------------------------------------------------------------------------- deschedule labels

static int check_label_plan(pas_ctx* ctx, int32_t n_nodes, int32_t n_strat, const void* viol,
                            const void* add, const void* rem, const void* total,
                            const char* fn) {
  if (n_nodes < 0 || n_strat < 0 || n_strat > 64)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape (0 <= n_strat <= 64)");
  if (!total || (n_nodes > 0 && (!add || !rem || (n_strat > 0 && !viol))))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null argument");
  return PAS_OK;
}

int pas_tas_label_plan(pas_ctx* ctx, int32_t n_nodes, int32_t n_strat, const uint64_t* viol,
                       const int32_t* name_id, const uint64_t* labels, uint64_t* add_out,
                       uint64_t* remove_out, int64_t* total_out) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_label_plan(ctx, n_nodes, n_strat, viol, add_out, remove_out, total_out,
                            "pas_tas_label_plan");
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  const size_t bits = (size_t)n_strat * (size_t)w64(n_nodes);
  Staging st(ctx);
  uint64_t *d_viol, *d_labels, *d_add, *d_rem;
  int64_t* d_total;
  st.in(d_viol, viol, bits);
  st.in_opt(d_labels, labels, bits);
  st.out(d_add, add_out, (size_t)n_nodes);
  st.out(d_rem, remove_out, (size_t)n_nodes);
  st.out(d_total, total_out, 1);
  if ((rc = st.upload())) return rc;
  rc = label_plan_launch(ctx, n_nodes, n_strat, make_name_plan(n_strat, name_id), d_viol,
                         d_labels, d_add, d_rem, d_total, ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_tas_label_plan_device(pas_ctx* ctx, int32_t n_nodes, int32_t n_strat,
                              const uint64_t* d_viol, const int32_t* name_id,
                              const uint64_t* d_labels, uint64_t* d_add_out,
                              uint64_t* d_remove_out, int64_t* d_total_out, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_label_plan(ctx, n_nodes, n_strat, d_viol, d_add_out, d_remove_out,
                            d_total_out, "pas_tas_label_plan_device");
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  return label_plan_launch(ctx, n_nodes, n_strat, make_name_plan(n_strat, name_id), d_viol,
                           d_labels, d_add_out, d_remove_out, d_total_out,
                           pick_stream(ctx, hip_stream));
}

int pas_tas_deschedule_device(pas_ctx* ctx, uint64_t gen, int32_t n_strategies,
                              int32_t n_rules, const pas_rule* d_rules,
                              const int32_t* d_rule_off, uint64_t* d_viol_out,
                              const int32_t* name_id, const uint64_t* d_labels,
                              uint64_t* d_add_out, uint64_t* d_remove_out, int64_t* d_total_out,
                              void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  if (n_rules < 0) return set_error(ctx, PAS_EINVAL, "negative count");
  if ((rc = check_label_plan(ctx, ctx->tas.n_nodes, n_strategies, d_viol_out, d_add_out,
                             d_remove_out, d_total_out, "pas_tas_deschedule_device")))
    return rc;
  if (n_strategies > 0 && (!d_rule_off || (n_rules > 0 && !d_rules)))
    return set_error(ctx, PAS_EINVAL, "pas_tas_deschedule_device: null input");
  if ((rc = activate(ctx))) return rc;
  return tas_deschedule_launch(ctx, n_strategies, n_rules, d_rules, d_rule_off, d_viol_out,
                               make_name_plan(n_strategies, name_id), d_labels, d_add_out,
                               d_remove_out, d_total_out, pick_stream(ctx, hip_stream));
}

// What the patch-list entry points check alike (the shape as check_label_plan).
static int check_label_patches(pas_ctx* ctx, int32_t n_nodes, int32_t n_strat, const void* viol,
                               int64_t cap, const void* node, const void* add, const void* rem,
                               const void* n_patches, const void* total, const char* fn) {
  if (n_nodes < 0 || n_strat < 0 || n_strat > 64)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape (0 <= n_strat <= 64)");
  if (cap < 0) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": cap < 0");
  if (!total || !n_patches || (cap > 0 && (!node || !add || !rem)) ||
      (n_nodes > 0 && n_strat > 0 && !viol))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null argument");
  return PAS_OK;
}

// The host forms' records: device arrays of min(cap, n_nodes) records (a list is never longer),
// of which the first min(cap, n_patches) are copied back once the count is known.
struct PatchRecords {
  int32_t* d_node;
  uint64_t *d_add, *d_rem;
  int64_t* d_n;
  int64_t room;
  void state(Staging& st, int32_t n_nodes, int64_t cap, int64_t* n_patches) {
    room = std::min<int64_t>(cap, n_nodes);
    st.work(d_node, (size_t)room);
    st.work(d_add, (size_t)room);
    st.work(d_rem, (size_t)room);
    st.out(d_n, n_patches, 1);
  }
  // after st.fetch(): *n_patches is the list's length
  int fetch(pas_ctx* ctx, int64_t n_patches, int32_t* node, uint64_t* add, uint64_t* rem) {
    const size_t n = (size_t)std::min(room, n_patches);
    if (n == 0) return PAS_OK;
    PAS_HIP(ctx, hipMemcpyAsync(node, d_node, sizeof(int32_t) * n, hipMemcpyDeviceToHost,
                                ctx->stream));
    PAS_HIP(ctx, hipMemcpyAsync(add, d_add, sizeof(uint64_t) * n, hipMemcpyDeviceToHost,
                                ctx->stream));
    PAS_HIP(ctx, hipMemcpyAsync(rem, d_rem, sizeof(uint64_t) * n, hipMemcpyDeviceToHost,
                                ctx->stream));
    PAS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PAS_OK;
  }
};

int pas_tas_label_patches(pas_ctx* ctx, int32_t n_nodes, int32_t n_strat, const uint64_t* viol,
                          const int32_t* name_id, const uint64_t* labels,
                          const uint64_t* violating, const uint64_t* null_, int64_t cap,
                          int32_t* patch_node, uint64_t* patch_add, uint64_t* patch_rem,
                          int64_t* n_patches, int64_t* total_out) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_label_patches(ctx, n_nodes, n_strat, viol, cap, patch_node, patch_add,
                               patch_rem, n_patches, total_out, "pas_tas_label_patches");
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  const size_t bits = (size_t)n_strat * (size_t)w64(n_nodes);
  Staging st(ctx);
  uint64_t *d_viol, *d_labels, *d_violating, *d_null;
  int64_t* d_total;
  PatchRecords rec;
  st.in(d_viol, viol, bits);
  st.in_opt(d_labels, labels, bits);
  st.in_opt(d_violating, labels ? violating : nullptr, bits);
  st.in_opt(d_null, labels ? null_ : nullptr, bits);
  rec.state(st, n_nodes, cap, n_patches);
  st.out(d_total, total_out, 1);
  if ((rc = st.upload())) return rc;
  rc = label_patches_launch(ctx, n_nodes, n_strat, make_name_plan(n_strat, name_id), d_viol,
                            d_labels, d_violating, d_null, rec.room, rec.d_node, rec.d_add,
                            rec.d_rem, rec.d_n, d_total, ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return rec.fetch(ctx, *n_patches, patch_node, patch_add, patch_rem);
}

int pas_tas_label_patches_device(pas_ctx* ctx, int32_t n_nodes, int32_t n_strat,
                                 const uint64_t* d_viol, const int32_t* name_id,
                                 const uint64_t* d_labels, const uint64_t* d_violating,
                                 const uint64_t* d_null, int64_t cap, int32_t* d_patch_node,
                                 uint64_t* d_patch_add, uint64_t* d_patch_rem,
                                 int64_t* d_n_patches, int64_t* d_total_out, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_label_patches(ctx, n_nodes, n_strat, d_viol, cap, d_patch_node, d_patch_add,
                               d_patch_rem, d_n_patches, d_total_out,
                               "pas_tas_label_patches_device");
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  return label_patches_launch(ctx, n_nodes, n_strat, make_name_plan(n_strat, name_id), d_viol,
                              d_labels, d_violating, d_null, cap, d_patch_node, d_patch_add,
                              d_patch_rem, d_n_patches, d_total_out,
                              pick_stream(ctx, hip_stream));
}

int pas_tas_deschedule_patches(pas_ctx* ctx, uint64_t gen, int32_t n_strat,
                               const pas_rule* rules, const int32_t* rule_off,
                               const int32_t* name_id, const uint64_t* labels,
                               const uint64_t* violating, const uint64_t* null_,
                               uint64_t* viol_out, int64_t cap, int32_t* patch_node,
                               uint64_t* patch_add, uint64_t* patch_rem, int64_t* n_patches,
                               int64_t* total_out) {
  const char* fn = "pas_tas_deschedule_patches";
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  const int32_t N = ctx->tas.n_nodes;
  // (the sweep's bitmaps are the call's own when viol_out is null)
  if ((rc = check_label_patches(ctx, N, n_strat, ctx, cap, patch_node, patch_add, patch_rem,
                                n_patches, total_out, fn)))
    return rc;
  int32_t n_rules = 0;
  if (n_strat > 0) {
    if (!rule_off) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null rule_off");
    if ((rc = validate_csr(ctx, n_strat, rule_off, "rule_off"))) return rc;
    n_rules = rule_off[n_strat];
    if (n_rules > 0 && !rules) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null rules");
    if ((rc = validate_rules(ctx, n_rules, rules))) return rc;
  }
  if ((rc = activate(ctx))) return rc;
  const size_t bits = (size_t)n_strat * (size_t)w64(N);
  Staging st(ctx);
  pas_rule* d_rules;
  int32_t* d_off;
  uint64_t *d_viol, *d_labels, *d_violating, *d_null;
  int64_t* d_total;
  PatchRecords rec;
  st.in(d_rules, rules, (size_t)n_rules);
  st.in(d_off, rule_off, n_strat > 0 ? (size_t)n_strat + 1 : 0);
  st.in_opt(d_labels, labels, bits);
  st.in_opt(d_violating, labels ? violating : nullptr, bits);
  st.in_opt(d_null, labels ? null_ : nullptr, bits);
  st.out_opt(d_viol, viol_out, bits);
  rec.state(st, N, cap, n_patches);
  st.out(d_total, total_out, 1);
  if ((rc = st.upload())) return rc;
  rc = tas_deschedule_patches_launch(ctx, n_strat, n_rules, d_rules, d_off, d_viol,
                                     make_name_plan(n_strat, name_id), d_labels, d_violating,
                                     d_null, rec.room, rec.d_node, rec.d_add, rec.d_rem, rec.d_n,
                                     d_total, ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return rec.fetch(ctx, *n_patches, patch_node, patch_add, patch_rem);
}

int pas_tas_deschedule_patches_device(pas_ctx* ctx, uint64_t gen, int32_t n_strat,
                                      int32_t n_rules, const pas_rule* d_rules,
                                      const int32_t* d_rule_off, const int32_t* name_id,
                                      const uint64_t* d_labels, const uint64_t* d_violating,
                                      const uint64_t* d_null, uint64_t* d_viol_out, int64_t cap,
                                      int32_t* d_patch_node, uint64_t* d_patch_add,
                                      uint64_t* d_patch_rem, int64_t* d_n_patches,
                                      int64_t* d_total_out, void* hip_stream) {
  const char* fn = "pas_tas_deschedule_patches_device";
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  if (n_rules < 0) return set_error(ctx, PAS_EINVAL, "negative count");
  if ((rc = check_label_patches(ctx, ctx->tas.n_nodes, n_strat, ctx, cap, d_patch_node,
                                d_patch_add, d_patch_rem, d_n_patches, d_total_out, fn)))
    return rc;
  if (n_strat > 0 && (!d_rule_off || (n_rules > 0 && !d_rules)))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null input");
  if ((rc = activate(ctx))) return rc;
  return tas_deschedule_patches_launch(ctx, n_strat, n_rules, d_rules, d_rule_off, d_viol_out,
                                       make_name_plan(n_strat, name_id), d_labels, d_violating,
                                       d_null, cap, d_patch_node, d_patch_add, d_patch_rem,
                                       d_n_patches, d_total_out, pick_stream(ctx, hip_stream));
}

// --------------------------------------------------------------------------- node shards

// (d_top_sub: the wide entry points' third record array; fn names the entry point)
static int tas_topk_api(pas_ctx* ctx, const char* fn, bool wide, uint64_t gen, int32_t n_pods,
                        int32_t n_rules, const pas_rule* d_rules, const int32_t* d_rule_off,
                        const pas_rule* d_prio, const uint64_t* d_cand, int32_t k,
                        int32_t node_base, int64_t* d_top_key, uint32_t* d_top_sub,
                        int32_t* d_top_node, int32_t* d_top_len, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, gen);
  if (rc) return rc;
  if (n_pods < 0 || n_rules < 0 || k < 1 || node_base < 0)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if (!wide && (rc = check_no_wide(ctx, fn))) return rc;
  if ((int64_t)node_base + ctx->tas.n_nodes > INT32_MAX)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": node ids past int32");
  if (n_pods == 0) return PAS_OK;
  if (!d_rule_off || !d_prio || (n_rules > 0 && !d_rules) || !d_top_key || !d_top_node ||
      !d_top_len || (wide && !d_top_sub))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null argument");
  if ((rc = activate(ctx))) return rc;
  return tas_topk_launch(ctx, n_pods, n_rules, d_rules, d_rule_off, d_prio, d_cand, k,
                         node_base, d_top_key, wide ? d_top_sub : nullptr, d_top_node,
                         d_top_len, pick_stream(ctx, hip_stream));
}

int pas_tas_topk_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t n_rules,
                        const pas_rule* d_rules, const int32_t* d_rule_off,
                        const pas_rule* d_prio, const uint64_t* d_cand, int32_t k,
                        int32_t node_base, int64_t* d_top_key, int32_t* d_top_node,
                        int32_t* d_top_len, void* hip_stream) {
  return tas_topk_api(ctx, "pas_tas_topk_device", false, gen, n_pods, n_rules, d_rules,
                      d_rule_off, d_prio, d_cand, k, node_base, d_top_key, nullptr, d_top_node,
                      d_top_len, hip_stream);
}

int pas_tas_topk_wide_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t n_rules,
                             const pas_rule* d_rules, const int32_t* d_rule_off,
                             const pas_rule* d_prio, const uint64_t* d_cand, int32_t k,
                             int32_t node_base, int64_t* d_top_key, uint32_t* d_top_sub,
                             int32_t* d_top_node, int32_t* d_top_len, void* hip_stream) {
  return tas_topk_api(ctx, "pas_tas_topk_wide_device", true, gen, n_pods, n_rules, d_rules,
                      d_rule_off, d_prio, d_cand, k, node_base, d_top_key, d_top_sub,
                      d_top_node, d_top_len, hip_stream);
}

static int tas_gas_topk_api(pas_ctx* ctx, const char* fn, bool wide, uint64_t tas_gen,
                            uint64_t gas_gen, int32_t n_pods, int32_t n_rules,
                            const pas_rule* d_rules, const int32_t* d_rule_off,
                            const pas_rule* d_prio, const uint64_t* d_cand,
                            int32_t max_containers, int32_t i915_index, const int64_t* d_req,
                            const uint32_t* d_req_mask, const int32_t* d_n_containers,
                            int32_t k, int32_t node_base, int64_t* d_top_key,
                            uint32_t* d_top_sub, int32_t* d_top_node, int32_t* d_top_len,
                            bool after, const int64_t* d_after_key,
                            const uint32_t* d_after_sub, const int32_t* d_after_node,
                            void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_tas_gen(ctx, tas_gen);
  if (rc) return rc;
  if ((rc = check_gas_gen(ctx, gas_gen))) return rc;
  if (ctx->gas.n_nodes != ctx->tas.n_nodes)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": TAS and GAS snapshots differ in node count");
  if (n_pods < 0 || n_rules < 0 || k < 1 || node_base < 0 || max_containers < 0 ||
      i915_index >= ctx->gas.n_res || i915_index < -1)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if (!wide && (rc = check_no_wide(ctx, fn))) return rc;
  if ((int64_t)node_base + ctx->tas.n_nodes > INT32_MAX)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": node ids past int32");
  if (n_pods == 0) return PAS_OK;
  if (!d_rule_off || !d_prio || (n_rules > 0 && !d_rules) || !d_top_key || !d_top_node ||
      !d_top_len || !d_n_containers || (max_containers > 0 && (!d_req || !d_req_mask)) ||
      (wide && !d_top_sub) ||
      (after && (!d_after_key || !d_after_node || (wide && !d_after_sub))))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null argument");
  if ((rc = activate(ctx))) return rc;
  const PodBatch pods{n_pods, max_containers, d_req, d_req_mask, d_n_containers};
  return tas_gas_topk_launch(ctx, n_rules, d_rules, d_rule_off, d_prio, d_cand, i915_index, pods,
                             k, node_base, d_top_key, wide ? d_top_sub : nullptr, d_top_node,
                             d_top_len, after ? d_after_key : nullptr,
                             wide ? d_after_sub : nullptr, d_after_node,
                             pick_stream(ctx, hip_stream));
}

int pas_tas_gas_topk_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen, int32_t n_pods,
                            int32_t n_rules, const pas_rule* d_rules, const int32_t* d_rule_off,
                            const pas_rule* d_prio, const uint64_t* d_cand,
                            int32_t max_containers, int32_t i915_index, const int64_t* d_req,
                            const uint32_t* d_req_mask, const int32_t* d_n_containers,
                            int32_t k, int32_t node_base, int64_t* d_top_key,
                            int32_t* d_top_node, int32_t* d_top_len, void* hip_stream) {
  return tas_gas_topk_api(ctx, "pas_tas_gas_topk_device", false, tas_gen, gas_gen, n_pods,
                          n_rules, d_rules, d_rule_off, d_prio, d_cand, max_containers,
                          i915_index, d_req, d_req_mask, d_n_containers, k, node_base,
                          d_top_key, nullptr, d_top_node, d_top_len, false, nullptr, nullptr,
                          nullptr, hip_stream);
}

int pas_tas_gas_topk_wide_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                 int32_t n_pods, int32_t n_rules, const pas_rule* d_rules,
                                 const int32_t* d_rule_off, const pas_rule* d_prio,
                                 const uint64_t* d_cand, int32_t max_containers,
                                 int32_t i915_index, const int64_t* d_req,
                                 const uint32_t* d_req_mask, const int32_t* d_n_containers,
                                 int32_t k, int32_t node_base, int64_t* d_top_key,
                                 uint32_t* d_top_sub, int32_t* d_top_node, int32_t* d_top_len,
                                 void* hip_stream) {
  return tas_gas_topk_api(ctx, "pas_tas_gas_topk_wide_device", true, tas_gen, gas_gen, n_pods,
                          n_rules, d_rules, d_rule_off, d_prio, d_cand, max_containers,
                          i915_index, d_req, d_req_mask, d_n_containers, k, node_base,
                          d_top_key, d_top_sub, d_top_node, d_top_len, false, nullptr, nullptr,
                          nullptr, hip_stream);
}

int pas_tas_gas_topk_after_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                  int32_t n_pods, int32_t n_rules, const pas_rule* d_rules,
                                  const int32_t* d_rule_off, const pas_rule* d_prio,
                                  const uint64_t* d_cand, int32_t max_containers,
                                  int32_t i915_index, const int64_t* d_req,
                                  const uint32_t* d_req_mask, const int32_t* d_n_containers,
                                  int32_t k, int32_t node_base, const int64_t* d_after_key,
                                  const int32_t* d_after_node, int64_t* d_top_key,
                                  int32_t* d_top_node, int32_t* d_top_len, void* hip_stream) {
  return tas_gas_topk_api(ctx, "pas_tas_gas_topk_after_device", false, tas_gen, gas_gen, n_pods,
                          n_rules, d_rules, d_rule_off, d_prio, d_cand, max_containers,
                          i915_index, d_req, d_req_mask, d_n_containers, k, node_base,
                          d_top_key, nullptr, d_top_node, d_top_len, true, d_after_key, nullptr,
                          d_after_node, hip_stream);
}

int pas_tas_gas_topk_wide_after_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                       int32_t n_pods, int32_t n_rules, const pas_rule* d_rules,
                                       const int32_t* d_rule_off, const pas_rule* d_prio,
                                       const uint64_t* d_cand, int32_t max_containers,
                                       int32_t i915_index, const int64_t* d_req,
                                       const uint32_t* d_req_mask,
                                       const int32_t* d_n_containers, int32_t k,
                                       int32_t node_base, const int64_t* d_after_key,
                                       const uint32_t* d_after_sub, const int32_t* d_after_node,
                                       int64_t* d_top_key, uint32_t* d_top_sub,
                                       int32_t* d_top_node, int32_t* d_top_len,
                                       void* hip_stream) {
  return tas_gas_topk_api(ctx, "pas_tas_gas_topk_wide_after_device", true, tas_gen, gas_gen,
                          n_pods, n_rules, d_rules, d_rule_off, d_prio, d_cand, max_containers,
                          i915_index, d_req, d_req_mask, d_n_containers, k, node_base,
                          d_top_key, d_top_sub, d_top_node, d_top_len, true, d_after_key,
                          d_after_sub, d_after_node, hip_stream);
}

// The top-k entry points by policy id: the checks of tas_topk_api / tas_gas_topk_api (gas:
// with the GAS snapshot) and those of the policy verbs.
static int topk_policies_api(pas_ctx* ctx, const char* fn, bool gas, bool wide, uint64_t tas_gen,
                             uint64_t gas_gen, int32_t n_pods, const int32_t* d_pod_policy,
                             const uint64_t* d_cand, int32_t max_containers, int32_t i915_index,
                             const int64_t* d_req, const uint32_t* d_req_mask,
                             const int32_t* d_n_containers, int32_t k, int32_t node_base,
                             int64_t* d_top_key, uint32_t* d_top_sub, int32_t* d_top_node,
                             int32_t* d_top_len, bool after, const int64_t* d_after_key,
                             const uint32_t* d_after_sub, const int32_t* d_after_node,
                             void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  int rc = check_policies(ctx, tas_gen, fn);
  if (rc) return rc;
  if (gas) {
    if ((rc = check_gas_gen(ctx, gas_gen))) return rc;
    if (ctx->gas.n_nodes != ctx->tas.n_nodes)
      return set_error(ctx, PAS_EINVAL,
                       std::string(fn) + ": TAS and GAS snapshots differ in node count");
    if (max_containers < 0 || i915_index >= ctx->gas.n_res || i915_index < -1)
      return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  }
  if (n_pods < 0 || k < 1 || node_base < 0)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if (!wide && (rc = check_no_wide(ctx, fn))) return rc;
  if ((int64_t)node_base + ctx->tas.n_nodes > INT32_MAX)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": node ids past int32");
  if (n_pods == 0) return PAS_OK;
  if (!d_pod_policy || !d_top_key || !d_top_node || !d_top_len || (wide && !d_top_sub) ||
      (gas && (!d_n_containers || (max_containers > 0 && (!d_req || !d_req_mask)))) ||
      (after && (!d_after_key || !d_after_node || (wide && !d_after_sub))))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null argument");
  if ((rc = activate(ctx))) return rc;
  const PodBatch pods{n_pods, max_containers, d_req, d_req_mask, d_n_containers};
  return tas_gas_topk_policies_launch(ctx, d_pod_policy, d_cand, gas, i915_index, pods, k,
                                      node_base, d_top_key, wide ? d_top_sub : nullptr,
                                      d_top_node, d_top_len, after ? d_after_key : nullptr,
                                      wide ? d_after_sub : nullptr, d_after_node,
                                      pick_stream(ctx, hip_stream));
}

int pas_tas_topk_policies_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods,
                                 const int32_t* d_pod_policy, const uint64_t* d_cand, int32_t k,
                                 int32_t node_base, int64_t* d_top_key, int32_t* d_top_node,
                                 int32_t* d_top_len, void* hip_stream) {
  return topk_policies_api(ctx, "pas_tas_topk_policies_device", false, false, gen, 0, n_pods,
                           d_pod_policy, d_cand, 0, -1, nullptr, nullptr, nullptr, k, node_base,
                           d_top_key, nullptr, d_top_node, d_top_len, false, nullptr, nullptr,
                           nullptr, hip_stream);
}

int pas_tas_topk_policies_wide_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods,
                                      const int32_t* d_pod_policy, const uint64_t* d_cand,
                                      int32_t k, int32_t node_base, int64_t* d_top_key,
                                      uint32_t* d_top_sub, int32_t* d_top_node,
                                      int32_t* d_top_len, void* hip_stream) {
  return topk_policies_api(ctx, "pas_tas_topk_policies_wide_device", false, true, gen, 0, n_pods,
                           d_pod_policy, d_cand, 0, -1, nullptr, nullptr, nullptr, k, node_base,
                           d_top_key, d_top_sub, d_top_node, d_top_len, false, nullptr, nullptr,
                           nullptr, hip_stream);
}

int pas_tas_gas_topk_policies_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                     int32_t n_pods, const int32_t* d_pod_policy,
                                     const uint64_t* d_cand, int32_t max_containers,
                                     int32_t i915_index, const int64_t* d_req,
                                     const uint32_t* d_req_mask, const int32_t* d_n_containers,
                                     int32_t k, int32_t node_base, int64_t* d_top_key,
                                     int32_t* d_top_node, int32_t* d_top_len, void* hip_stream) {
  return topk_policies_api(ctx, "pas_tas_gas_topk_policies_device", true, false, tas_gen,
                           gas_gen, n_pods, d_pod_policy, d_cand, max_containers, i915_index,
                           d_req, d_req_mask, d_n_containers, k, node_base, d_top_key, nullptr,
                           d_top_node, d_top_len, false, nullptr, nullptr, nullptr, hip_stream);
}

int pas_tas_gas_topk_policies_wide_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                          int32_t n_pods, const int32_t* d_pod_policy,
                                          const uint64_t* d_cand, int32_t max_containers,
                                          int32_t i915_index, const int64_t* d_req,
                                          const uint32_t* d_req_mask,
                                          const int32_t* d_n_containers, int32_t k,
                                          int32_t node_base, int64_t* d_top_key,
                                          uint32_t* d_top_sub, int32_t* d_top_node,
                                          int32_t* d_top_len, void* hip_stream) {
  return topk_policies_api(ctx, "pas_tas_gas_topk_policies_wide_device", true, true, tas_gen,
                           gas_gen, n_pods, d_pod_policy, d_cand, max_containers, i915_index,
                           d_req, d_req_mask, d_n_containers, k, node_base, d_top_key, d_top_sub,
                           d_top_node, d_top_len, false, nullptr, nullptr, nullptr, hip_stream);
}

int pas_tas_gas_topk_policies_after_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                           int32_t n_pods, const int32_t* d_pod_policy,
                                           const uint64_t* d_cand, int32_t max_containers,
                                           int32_t i915_index, const int64_t* d_req,
                                           const uint32_t* d_req_mask,
                                           const int32_t* d_n_containers, int32_t k,
                                           int32_t node_base, const int64_t* d_after_key,
                                           const int32_t* d_after_node, int64_t* d_top_key,
                                           int32_t* d_top_node, int32_t* d_top_len,
                                           void* hip_stream) {
  return topk_policies_api(ctx, "pas_tas_gas_topk_policies_after_device", true, false, tas_gen,
                           gas_gen, n_pods, d_pod_policy, d_cand, max_containers, i915_index,
                           d_req, d_req_mask, d_n_containers, k, node_base, d_top_key, nullptr,
                           d_top_node, d_top_len, true, d_after_key, nullptr, d_after_node,
                           hip_stream);
}

int pas_tas_gas_topk_policies_wide_after_device(
    pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen, int32_t n_pods,
    const int32_t* d_pod_policy, const uint64_t* d_cand, int32_t max_containers,
    int32_t i915_index, const int64_t* d_req, const uint32_t* d_req_mask,
    const int32_t* d_n_containers, int32_t k, int32_t node_base, const int64_t* d_after_key,
    const uint32_t* d_after_sub, const int32_t* d_after_node, int64_t* d_top_key,
    uint32_t* d_top_sub, int32_t* d_top_node, int32_t* d_top_len, void* hip_stream) {
  return topk_policies_api(ctx, "pas_tas_gas_topk_policies_wide_after_device", true, true,
                           tas_gen, gas_gen, n_pods, d_pod_policy, d_cand, max_containers,
                           i915_index, d_req, d_req_mask, d_n_containers, k, node_base,
                           d_top_key, d_top_sub, d_top_node, d_top_len, true, d_after_key,
                           d_after_sub, d_after_node, hip_stream);
}

static int topk_merge_api(pas_ctx* ctx, const char* fn, bool wide, int32_t n_pods, int32_t k,
                          int32_t n_shards, const int64_t* d_keys, const uint32_t* d_subs,
                          const int32_t* d_nodes, int32_t* d_out_node, int32_t* d_out_len,
                          void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  if (n_pods < 0 || k < 1 || n_shards < 1) return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if (n_pods == 0) return PAS_OK;
  if (!d_keys || !d_nodes || !d_out_node || !d_out_len || (wide && !d_subs))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null argument");
  int rc = activate(ctx);
  if (rc) return rc;
  return topk_merge_launch(ctx, n_pods, k, n_shards, d_keys, wide ? d_subs : nullptr, d_nodes,
                           d_out_node, d_out_len, pick_stream(ctx, hip_stream));
}

int pas_topk_merge_device(pas_ctx* ctx, int32_t n_pods, int32_t k, int32_t n_shards,
                          const int64_t* d_keys, const int32_t* d_nodes, int32_t* d_out_node,
                          int32_t* d_out_len, void* hip_stream) {
  return topk_merge_api(ctx, "pas_topk_merge_device", false, n_pods, k, n_shards, d_keys,
                        nullptr, d_nodes, d_out_node, d_out_len, hip_stream);
}

int pas_topk_merge_wide_device(pas_ctx* ctx, int32_t n_pods, int32_t k, int32_t n_shards,
                               const int64_t* d_keys, const uint32_t* d_subs,
                               const int32_t* d_nodes, int32_t* d_out_node, int32_t* d_out_len,
                               void* hip_stream) {
  return topk_merge_api(ctx, "pas_topk_merge_wide_device", true, n_pods, k, n_shards, d_keys,
                        d_subs, d_nodes, d_out_node, d_out_len, hip_stream);
}

static int list_merge_api(pas_ctx* ctx, const char* fn, bool wide, int32_t n_pods,
                          int32_t n_shards, int32_t width, const int64_t* d_keys,
                          const uint32_t* d_subs, const int32_t* d_nodes, int32_t* d_out_node,
                          int64_t out_ld, int32_t* d_out_len, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  if (n_pods < 0 || n_shards < 1 || n_shards > 4096 || width < 1 ||
      out_ld < (int64_t)n_shards * width || (int64_t)n_shards * width > INT32_MAX)
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": bad shape");
  if (n_pods == 0) return PAS_OK;
  if (!d_keys || !d_nodes || !d_out_node || !d_out_len || (wide && !d_subs))
    return set_error(ctx, PAS_EINVAL, std::string(fn) + ": null argument");
  int rc = activate(ctx);
  if (rc) return rc;
  return list_merge_launch(ctx, n_pods, n_shards, width, d_keys, wide ? d_subs : nullptr,
                           d_nodes, d_out_node, out_ld, d_out_len,
                           pick_stream(ctx, hip_stream));
}

int pas_list_merge_device(pas_ctx* ctx, int32_t n_pods, int32_t n_shards, int32_t width,
                          const int64_t* d_keys, const int32_t* d_nodes, int32_t* d_out_node,
                          int64_t out_ld, int32_t* d_out_len, void* hip_stream) {
  return list_merge_api(ctx, "pas_list_merge_device", false, n_pods, n_shards, width, d_keys,
                        nullptr, d_nodes, d_out_node, out_ld, d_out_len, hip_stream);
}

int pas_list_merge_wide_device(pas_ctx* ctx, int32_t n_pods, int32_t n_shards, int32_t width,
                               const int64_t* d_keys, const uint32_t* d_subs,
                               const int32_t* d_nodes, int32_t* d_out_node, int64_t out_ld,
                               int32_t* d_out_len, void* hip_stream) {
  return list_merge_api(ctx, "pas_list_merge_wide_device", true, n_pods, n_shards, width,
                        d_keys, d_subs, d_nodes, d_out_node, out_ld, d_out_len, hip_stream);
}

// --------------------------------------------------------------------------- timing

int pas_set_timing(pas_ctx* ctx, int enable) {
  if (!ctx) return PAS_EINVAL;
  if (enable < 0 || enable > PAS_TIMING_KERNELS)
    return set_error(ctx, PAS_EINVAL, "pas_set_timing: level must be 0, 1 or 2");
  ctx->timing = enable;
  return PAS_OK;
}

int pas_kernel_time(pas_ctx* ctx, int32_t kernel_id, double* total_ms, int64_t* launches) {
  if (!ctx || kernel_id < 0 || kernel_id >= PAS_K_COUNT) return PAS_EINVAL;
  resolve_timing(ctx);
  if (total_ms) *total_ms = ctx->total_ms[kernel_id];
  if (launches) *launches = ctx->launches[kernel_id];
  return PAS_OK;
}

int pas_reset_timing(pas_ctx* ctx) {
  if (!ctx) return PAS_EINVAL;
  resolve_timing(ctx);
  for (int i = 0; i < PAS_K_COUNT; ++i) {
    ctx->total_ms[i] = 0;
    ctx->launches[i] = 0;
  }
  return PAS_OK;
}

}  // extern "C"
