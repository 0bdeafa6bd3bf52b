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
#include "card_rows.h"
#include "host_staging.h"
#include "pas_internal.h"
#include "span_pool.h"

namespace pas {
namespace {

constexpr int kTpb = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTpb - 1) / kTpb); }

// Rules 1-4 of pas_gas_apply_annotations for event e, else PAS_GAS_ANN_PENDING.  kind null:
// the resolve form, which has no kinds.  name_off non-null: node[e] is the slot the name table
// gave the event's node name (-1 without one), and an empty name is bad args; of the names only
// the offsets are read (which is why they come as two arguments: as a ByteSpans member the
// offsets lose their __restrict__, and the kernel's SGPR count changes with it).
__global__ __launch_bounds__(kTpb) void annotation_count(
    int32_t E, int32_t N, const int32_t* __restrict__ kind, const int32_t* __restrict__ pod,
    const int32_t* __restrict__ node, int64_t n_name_bytes, const int64_t* __restrict__ name_off,
    int32_t n_pods, const int32_t* __restrict__ ncont, int32_t C, ByteSpans ann,
    int32_t* __restrict__ verdict,
    int32_t* __restrict__ n_listed, int32_t* __restrict__ walker_node, int32_t* max_pending) {
  const int32_t e = blockIdx.x * kTpb + threadIdx.x;
  int32_t pending = 0;  // this lane's listed count if its event is pending
  if (e < E) {
    int64_t b;
    const int64_t len = ann.span(e, &b);
    const AnnotationCounts cnt = annotation_counts(ann.bytes + b, len);
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
  wave_max(pending, max_pending);
}

struct RankVisitor {
  const CardView& t;
  const char* p;
  int64_t row;
  int32_t L, C, cards_ld;
  int32_t* cpc;
  int32_t* cards;
  __device__ void name(int64_t j, int64_t, int64_t beg, int64_t len) {
    if (j < cards_ld) cards[j] = row_find(t, row, L, p + beg, len);
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
    int only_pending, const int32_t* __restrict__ n_cards, CardView t, int32_t C, ByteSpans ann,
    int32_t cards_ld, int32_t* __restrict__ cpc, int32_t* __restrict__ cards) {
  const int32_t e = blockIdx.x * kTpb + threadIdx.x;
  if (e >= E || (only_pending && verdict[e] != PAS_GAS_ANN_PENDING)) return;
  int64_t b;
  const int64_t len = ann.span(e, &b);
  const int32_t n = node[e];
  const bool held = n >= 0 && n < N;
  const int32_t L = held ? max(0, min(n_cards[n], t.k)) : 0;
  int32_t* cpc_e = cpc + (int64_t)e * C;
  int32_t* cards_e = cards + (int64_t)e * cards_ld;
  const AnnotationCounts cnt = annotation_walk(
      ann.bytes + b, len,
      RankVisitor{t, ann.bytes + b, held ? (int64_t)n * t.k : 0, L, C, cards_ld, cpc_e, cards_e});
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

// The event batch of one call: an entry point fills it from its arguments (a host form with
// host pointers, which resolve_host / apply_host replace with the staged ones), so that the
// plain and _names forms, and the host and _device forms, differ by what they fill in.
struct AnnEvents {
  int32_t n_events;
  const int32_t* kind;  // null: the resolve forms, which have no kinds
  const int32_t* pod;
  const int32_t* node;  // null: the nodes by name
  ByteSpans names;      // the node names (a host form: n_bytes is set once they are checked)
  ByteSpans ann;
  int32_t* status;      // the apply forms' output
  int32_t cards_ld;     // the resolve forms' outputs: [E], [E], [E][C], [E][cards_ld]
  int32_t *verdict, *n_listed, *cpc, *cards;
};

// The parse-alone form on device arrays, enqueued on s: per event the verdict of the rules of
// pas_gas_apply_annotations, the listed count, the cards per container and the ranks of the first
// cards_ld listed cards.  Of pods only n_pods, max_containers and n_containers are read.  The
// caller has checked the snapshot and the card-name table.
int annotations_resolve_launch(pas_ctx* ctx, const AnnEvents& a, const PodBatch& pods,
                               hipStream_t s) {
  if (a.n_events == 0) return PAS_OK;
  const GasSnapshot& g = ctx->gas;
  annotation_count<<<blocks_for(a.n_events), kTpb, 0, s>>>(
      a.n_events, g.n_nodes, a.kind, a.pod, a.node, 0, nullptr, pods.n_pods, pods.n_containers,
      pods.max_containers, a.ann, a.verdict, a.n_listed, nullptr, nullptr);
  PAS_HIP(ctx, hipGetLastError());
  annotation_ranks<<<blocks_for(a.n_events), kTpb, 0, s>>>(
      a.n_events, g.n_nodes, a.node, a.verdict, 0, g.n_cards, view_of(ctx->gas_cards),
      pods.max_containers, a.ann, a.cards_ld, a.cpc, a.cards);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

// pas_gas_apply_annotations[_names][_device] on device arrays: the count pass, the call's one
// read-back (s is synchronized), the rank pass into the slot's workspace, gas_apply_launch and
// the status fix-up.  a.node null: the nodes by name, resolved through the name table, which the
// caller has checked like the snapshot and the card-name table.  Nothing of the snapshot has
// changed when it returns an error.
int gas_apply_annotations_launch(pas_ctx* ctx, const AnnEvents& a, const PodBatch& pods,
                                 hipStream_t s) {
  const int32_t n_events = a.n_events;
  if (n_events == 0) return PAS_OK;
  const GasSnapshot& g = ctx->gas;
  const size_t E = (size_t)n_events, C = (size_t)pods.max_containers;
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
  const int32_t* d_node = a.node;
  ByteSpans names{};
  if (!d_node) {  // the nodes by name: lookup only, into the slot's buffer
    rc = names_resolve_launch(ctx, n_events, a.names, d_slot, nullptr, nullptr, false, s);
    if (rc) return rc;
    d_node = d_slot;
    names = a.names;
  }
  PAS_HIP(ctx, hipMemsetAsync(d_max, 0, sizeof(int32_t), s));
  annotation_count<<<blocks_for(n_events), kTpb, 0, s>>>(
      n_events, g.n_nodes, a.kind, a.pod, d_node, names.n_bytes, names.off, pods.n_pods,
      pods.n_containers, pods.max_containers, a.ann, d_verdict, d_n_listed, d_walker_node, d_max);
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
      pods.max_containers, a.ann, cards_ld, d_cpc, d_cards);
  PAS_HIP(ctx, hipGetLastError());
  // nothing has changed so far; the walker changes the usage
  rc = gas_apply_launch(ctx, n_events, a.kind, a.pod, d_walker_node, pods, d_cpc, d_cards,
                        cards_ld, a.status, s);
  if (rc) return rc;
  annotation_verdicts<<<blocks_for(n_events), kTpb, 0, s>>>(n_events, d_verdict, a.status);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

// What every form checks first: the snapshot (gen_from null: the resolve forms, which check no
// generation), the tables, then the scalars and pointers a host can check on either form
// (by_name: the nodes by name).  The pods are the call's, host or device.
int events_check(pas_ctx* ctx, bool by_name, const uint64_t* gen_from, const AnnEvents& a,
                 const PodBatch& pods, const std::string& fn) {
  int rc = PAS_OK;
  if (gen_from) {
    if ((rc = check_gas_gen(ctx, *gen_from))) return rc;
  } else if (!ctx->gas.valid) {
    return set_error(ctx, PAS_ENOSNAP, "no GAS snapshot uploaded");
  }
  if ((rc = gas_annotations_tables(ctx, by_name, fn))) return rc;
  const bool apply = gen_from != nullptr;
  if (a.n_events < 0 || pods.n_pods < 0 || pods.max_containers < 0 || (!apply && a.cards_ld < 1))
    return set_error(ctx, PAS_EINVAL, fn + ": bad shape");
  if (a.n_events == 0) return PAS_OK;
  const bool pods_null = (pods.n_pods > 0 && !pods.n_containers) ||
                         (apply && pods.max_containers > 0 && pods.n_pods > 0 &&
                          (!pods.req || !pods.mask));
  const bool outs_null = apply ? !a.kind || !a.status
                               : !a.verdict || !a.n_listed || !a.cards ||
                                     (pods.max_containers > 0 && !a.cpc);
  if (!a.pod || !(by_name ? (const void*)a.names.off : a.node) || !a.ann.off || pods_null ||
      outs_null)
    return set_error(ctx, PAS_EINVAL, fn + ": null input");
  return PAS_OK;
}

// The _device forms: gen_to steps only with an apply form (gen_from non-null)
int events_device(pas_ctx* ctx, bool by_name, const uint64_t* gen_from, uint64_t gen_to,
                  const AnnEvents& a, const PodBatch& pods, void* hip_stream,
                  const std::string& fn) {
  if (!ctx) return PAS_EINVAL;
  int rc = events_check(ctx, by_name, gen_from, a, pods, fn);
  if (rc) return rc;
  if ((rc = check_device_spans(ctx, a.n_events, a.ann, fn + ": ann_off")) ||
      (rc = check_device_spans(ctx, by_name ? a.n_events : 0, a.names, fn + ": node_name_off")))
    return rc;
  if ((rc = activate(ctx))) return rc;
  hipStream_t s = pick_stream(ctx, hip_stream);
  if (!gen_from) return annotations_resolve_launch(ctx, a, pods, s);
  return gas_finish(ctx, gas_apply_annotations_launch(ctx, a, pods, s), false, gen_to);
}

// What the host forms share past events_check: the spans, then the staging of the events (pod,
// the nodes or their names, the annotations) into a, in the order the arguments come.  h holds
// the caller's host pointers.
int events_host_spans(pas_ctx* ctx, bool by_name, const AnnEvents& h, const std::string& fn) {
  int rc = check_host_spans(ctx, h.n_events, h.ann.off, h.ann.bytes, fn + ": ann_off");
  if (!rc && by_name)
    rc = check_host_spans(ctx, h.n_events, h.names.off, h.names.bytes, fn + ": node_name_off");
  return rc;
}

void stage_nodes(Staging& st, bool by_name, const AnnEvents& h, AnnEvents& a) {
  if (by_name)
    st.in_spans(a.names, h.n_events, h.names.off, h.names.bytes);
  else
    st.in(a.node, h.node, (size_t)h.n_events);
}

// pas_gas_annotations_resolve: validate, upload, run the _device form's path, wait and copy the
// outputs back.
int resolve_host(pas_ctx* ctx, const AnnEvents& h, const PodBatch& hp, const std::string& fn) {
  if (!ctx) return PAS_EINVAL;
  int rc = events_check(ctx, false, nullptr, h, hp, fn);
  if (rc || h.n_events == 0) return rc;
  if ((rc = events_host_spans(ctx, false, h, fn))) return rc;
  if ((rc = activate(ctx))) return rc;
  const size_t E = (size_t)h.n_events;
  Staging st(ctx);
  PodBatch pods{hp.n_pods, hp.max_containers, nullptr, nullptr, nullptr};
  AnnEvents a{};
  a.n_events = h.n_events;
  a.cards_ld = h.cards_ld;
  st.in(a.pod, h.pod, E);
  stage_nodes(st, false, h, a);
  st.in(pods.n_containers, hp.n_containers, (size_t)hp.n_pods);
  st.in_spans(a.ann, h.n_events, h.ann.off, h.ann.bytes);
  st.out(a.verdict, h.verdict, E);
  st.out(a.n_listed, h.n_listed, E);
  st.out(a.cpc, h.cpc, E * (size_t)hp.max_containers);
  st.out(a.cards, h.cards, E * (size_t)h.cards_ld);
  if ((rc = st.upload())) return rc;
  if ((rc = annotations_resolve_launch(ctx, a, pods, ctx->stream))) return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

// pas_gas_apply_annotations[_names]: validate (rules 1 and 3 are PAS_EINVAL for the call),
// upload, run the _device forms' path, wait and copy status_out back.
int apply_host(pas_ctx* ctx, bool by_name, uint64_t gen_from, uint64_t gen_to, const AnnEvents& h,
               const PodBatch& hp, const std::string& fn) {
  if (!ctx) return PAS_EINVAL;
  int rc = events_check(ctx, by_name, &gen_from, h, hp, fn);
  if (rc) return rc;
  const int32_t n_events = h.n_events, N = ctx->gas.n_nodes;
  if (n_events == 0) return gas_finish(ctx, activate(ctx), false, gen_to);
  if ((rc = events_host_spans(ctx, by_name, h, fn))) return rc;
  for (int32_t e = 0; e < n_events; ++e) {
    if (h.kind[e] != PAS_GAS_EV_ADD && h.kind[e] != PAS_GAS_EV_REMOVE)
      return set_error(ctx, PAS_EINVAL, fn + ": event kind out of range");
    if (h.pod[e] < 0 || h.pod[e] >= hp.n_pods)
      return set_error(ctx, PAS_EINVAL, fn + ": pod index out of range");
    if (!by_name && h.node[e] != -1 && (h.node[e] < 0 || h.node[e] >= N))
      return set_error(ctx, PAS_EINVAL, fn + ": node neither -1 nor a slot of the snapshot");
    if ((rc = gas_pod_check(ctx, h.pod[e], hp.max_containers, hp.mask, hp.n_containers,
                            fn.c_str())))
      return rc;
  }
  if ((rc = activate(ctx))) return rc;
  const size_t E = (size_t)n_events;
  Staging st(ctx);
  PodBatch pods;
  AnnEvents a{};
  a.n_events = n_events;
  stage_pods(st, pods, hp.n_pods, hp.max_containers, hp.req, hp.mask, hp.n_containers);
  st.in(a.kind, h.kind, E);
  st.in(a.pod, h.pod, E);
  stage_nodes(st, by_name, h, a);
  st.in_spans(a.ann, n_events, h.ann.off, h.ann.bytes);
  st.out(a.status, h.status, E);
  if ((rc = st.upload())) return rc;
  if ((rc = gas_apply_annotations_launch(ctx, a, pods, ctx->stream))) return rc;
  rc = st.fetch_results(fn);
  return gas_finish(ctx, rc, rc != PAS_OK, gen_to);
}

}  // namespace
}  // namespace pas

using namespace pas;

extern "C" {

int pas_gas_annotations_resolve_device(pas_ctx* ctx, int32_t n_events, const int32_t* d_ev_pod,
                                       const int32_t* d_ev_node, int32_t n_pods,
                                       const int32_t* d_n_containers, int32_t max_containers,
                                       int64_t n_ann_bytes, const int64_t* d_ann_off,
                                       const char* d_ann_bytes, int32_t cards_ld,
                                       int32_t* d_verdict_out, int32_t* d_n_listed_out,
                                       int32_t* d_cards_per_container_out, int32_t* d_cards_out,
                                       void* hip_stream) {
  const AnnEvents a{n_events, nullptr, d_ev_pod, d_ev_node, ByteSpans{},
                    ByteSpans{n_ann_bytes, d_ann_off, d_ann_bytes}, nullptr, cards_ld,
                    d_verdict_out, d_n_listed_out, d_cards_per_container_out, d_cards_out};
  return events_device(ctx, false, nullptr, 0, a,
                       PodBatch{n_pods, max_containers, nullptr, nullptr, d_n_containers},
                       hip_stream, "pas_gas_annotations_resolve_device");
}

int pas_gas_annotations_resolve(pas_ctx* ctx, int32_t n_events, const int32_t* ev_pod,
                                const int32_t* ev_node, int32_t n_pods,
                                const int32_t* n_containers, int32_t max_containers,
                                const int64_t* ann_off, const char* ann_bytes, int32_t cards_ld,
                                int32_t* verdict_out, int32_t* n_listed_out,
                                int32_t* cards_per_container_out, int32_t* cards_out) {
  const AnnEvents h{n_events, nullptr, ev_pod, ev_node, ByteSpans{},
                    ByteSpans{0, ann_off, ann_bytes}, nullptr, cards_ld, verdict_out,
                    n_listed_out, cards_per_container_out, cards_out};
  return resolve_host(ctx, h, PodBatch{n_pods, max_containers, nullptr, nullptr, n_containers},
                      "pas_gas_annotations_resolve");
}

int pas_gas_apply_annotations_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                     int32_t n_events, const int32_t* d_ev_kind,
                                     const int32_t* d_ev_pod, const int32_t* d_ev_node,
                                     int32_t n_pods, int32_t max_containers, const int64_t* d_req,
                                     const uint32_t* d_req_mask, const int32_t* d_n_containers,
                                     int64_t n_ann_bytes, const int64_t* d_ann_off,
                                     const char* d_ann_bytes, int32_t* d_status_out,
                                     void* hip_stream) {
  AnnEvents a{n_events, d_ev_kind, d_ev_pod, d_ev_node, ByteSpans{},
              ByteSpans{n_ann_bytes, d_ann_off, d_ann_bytes}, d_status_out};
  return events_device(ctx, false, &gen_from, gen_to, a,
                       PodBatch{n_pods, max_containers, d_req, d_req_mask, d_n_containers},
                       hip_stream, "pas_gas_apply_annotations_device");
}

int pas_gas_apply_annotations_names_device(
    pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_events, const int32_t* d_ev_kind,
    const int32_t* d_ev_pod, int64_t n_name_bytes, const int64_t* d_node_name_off,
    const char* d_node_name_bytes, int32_t n_pods, int32_t max_containers, const int64_t* d_req,
    const uint32_t* d_req_mask, const int32_t* d_n_containers, int64_t n_ann_bytes,
    const int64_t* d_ann_off, const char* d_ann_bytes, int32_t* d_status_out, void* hip_stream) {
  AnnEvents a{n_events, d_ev_kind, d_ev_pod, nullptr,
              ByteSpans{n_name_bytes, d_node_name_off, d_node_name_bytes},
              ByteSpans{n_ann_bytes, d_ann_off, d_ann_bytes}, d_status_out};
  return events_device(ctx, true, &gen_from, gen_to, a,
                       PodBatch{n_pods, max_containers, d_req, d_req_mask, d_n_containers},
                       hip_stream, "pas_gas_apply_annotations_names_device");
}

int pas_gas_apply_annotations(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_events,
                              const int32_t* ev_kind, const int32_t* ev_pod,
                              const int32_t* ev_node, int32_t n_pods, int32_t max_containers,
                              const int64_t* req, const uint32_t* req_mask,
                              const int32_t* n_containers, const int64_t* ann_off,
                              const char* ann_bytes, int32_t* status_out) {
  AnnEvents h{n_events, ev_kind, ev_pod, ev_node, ByteSpans{}, ByteSpans{0, ann_off, ann_bytes},
              status_out};
  return apply_host(ctx, false, gen_from, gen_to, h,
                    PodBatch{n_pods, max_containers, req, req_mask, n_containers},
                    "pas_gas_apply_annotations");
}

int pas_gas_apply_annotations_names(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                    int32_t n_events, const int32_t* ev_kind,
                                    const int32_t* ev_pod, const int64_t* node_name_off,
                                    const char* node_name_bytes, int32_t n_pods,
                                    int32_t max_containers, const int64_t* req,
                                    const uint32_t* req_mask, const int32_t* n_containers,
                                    const int64_t* ann_off, const char* ann_bytes,
                                    int32_t* status_out) {
  AnnEvents h{n_events, ev_kind, ev_pod, nullptr, ByteSpans{0, node_name_off, node_name_bytes},
              ByteSpans{0, ann_off, ann_bytes}, status_out};
  return apply_host(ctx, true, gen_from, gen_to, h,
                    PodBatch{n_pods, max_containers, req, req_mask, n_containers},
                    "pas_gas_apply_annotations_names");
}

}  // extern "C"
