/*
 * pas.h — C-ABI of the MI355X-native Platform Aware Scheduling evaluator.
 *
 * This is the drop-in boundary beneath the reference's extender.Scheduler
 * HTTP verbs (extender/types.go:11-15; registered at extender/scheduler.go:86-91).
 * The Go handlers keep decoding extender.Args and encoding FilterResult /
 * HostPriorityList; the compute they do per request is replaced by the batched
 * entry points below (cgo binding shown in INTEGRATION.md).
 *
 * Conventions
 *   - Plain C types only; no exceptions or aborts cross this boundary.
 *   - Every function returns a pas_status (0 = OK, negative = error) and leaves a
 *     message retrievable with pas_last_error(ctx).
 *   - Host-pointer entry points copy their inputs in and results out and return
 *     when the results are in host memory.  *_device entry points take device
 *     pointers and a hipStream_t (as void*) and return once the work is enqueued.
 *   - A pas_ctx is NOT thread safe: callers serialise calls per context (the GAS
 *     extender already holds GASExtender.rwmutex around filter/bind,
 *     gpu-aware-scheduling/pkg/gpuscheduler/scheduler.go:463-465).
 *   - Bitmaps are little-endian uint64 words, node n at bit (n & 63) of word n >> 6;
 *     W64(n) = (n + 63) / 64 words per row, bits >= n_nodes are zero.
 *   - Metric values are int64 fixed-point columns: column m holds value * 10^scale[m] of
 *     the reference's resource.Quantity (telemetry-aware-scheduling/pkg/metrics/
 *     client.go:25-29), scale 3 ("milli") unless pas_tas_snapshot_set_scale says otherwise.
 *     ParseQuantity keeps at most 9 fractional digits (it rounds to 1e-9), so a column with
 *     scale = the most decimal places of its values (pas_quantity_decimals, 0..9) is exact;
 *     pas_quantity_to_scaled() converts a Quantity string and reports PAS_ENOTEXACT only
 *     when value * 10^scale is outside int64.
 */
#ifndef PAS_H_
#define PAS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAS_ABI_VERSION 3

typedef enum pas_status {
  PAS_OK = 0,
  PAS_EINVAL = -1,     /* bad argument (shape, operator, null pointer) */
  PAS_ESTALE = -2,     /* generation mismatch between call and resident snapshot */
  PAS_ENOTEXACT = -3,  /* a value is not representable as exact int64 milli (or: integer part
                          outside int64, pas_quantity_to_wide; top-k over a wide column) */
  PAS_EDEVICE = -4,    /* HIP runtime error */
  PAS_ENOMEM = -5,     /* device or host allocation failed */
  PAS_ENOSNAP = -6,    /* no snapshot uploaded yet */
  PAS_ECAPACITY = -7,  /* shape exceeds a documented kernel limit / an output buffer */
  PAS_EDECODE = -8     /* request body that json.Decoder.Decode(&args) rejects */
} pas_status;

/* TASPolicyRule.Operator (telemetrypolicy/api/v1alpha1/types.go:31-35), evaluated as
 * in core.EvaluateRule (strategies/core/operator.go:13-26).  Any other string panics
 * in the reference (operator.go:25: nil map entry); here it is PAS_EINVAL. */
typedef enum pas_op {
  PAS_OP_LESS_THAN = 0,
  PAS_OP_GREATER_THAN = 1,
  PAS_OP_EQUALS = 2
} pas_op;

/* One TASPolicyRule with the metric name resolved to a snapshot column.
 * metric < 0 or >= n_metrics means "metric not in the cache": the rule is skipped,
 * as dontschedule.Violated does on a ReadMetric error (dontschedule/strategy.go:28-32). */
typedef struct pas_rule {
  int32_t metric;
  int32_t op;      /* pas_op */
  int64_t target;  /* TASPolicyRule.Target, integer units (NOT milli) */
} pas_rule;

typedef struct pas_config {
  int32_t device;    /* HIP device ordinal; -1 = current device */
  int32_t reserved;  /* must be 0 */
} pas_config;

typedef struct pas_ctx pas_ctx;

int pas_abi_version(void);

/* Context: owns one HIP stream (replaceable with pas_set_stream), the resident
 * snapshots and scratch. */
int pas_create(const pas_config* cfg, pas_ctx** out);
void pas_destroy(pas_ctx* ctx);
const char* pas_last_error(const pas_ctx* ctx);
int pas_set_stream(pas_ctx* ctx, void* hip_stream); /* NULL = the context's own stream */
/* A hip_stream argument (here and in every _device entry point) of NULL names the context's
 * current stream; PAS_STREAM_NULL names the HIP null stream (e.g. torch's default stream).
 * Evaluation calls may be issued on several streams without host synchronisation: the
 * context keeps per-stream scratch (calls on two or more streams in turn overlap), orders a
 * call after the last user of the scratch it takes over, and orders readers of data it
 * derives from a snapshot after that data's build.  A call that CHANGES a resident snapshot
 * (snapshot_set, snapshot_update, gas_bind, gas_release) must be ordered by the caller after
 * the calls on other streams that still read it. */
#define PAS_STREAM_NULL ((void*)1)
/* Waits for the context's stream and for the last calls on every other stream the context
 * ran on (and the GAS fits' internal side streams).  Returns PAS_EDEVICE when a GAS fit
 * enqueued since the last report could not complete: one of its internal stream waits gave
 * up (pas_gas_fit_device: its outputs are not to be used); the report is cleared, so the
 * next call starts clean.  The host-pointer GAS forms report this themselves. */
int pas_synchronize(pas_ctx* ctx);

/* Operator string -> pas_op ("LessThan", "GreaterThan", "Equals"), else PAS_EINVAL.
 * Replaces the map lookup in core.EvaluateRule (operator.go:14-25). */
int pas_parse_operator(const char* op);

/* resource.Quantity string -> the parsed quantity's value * 1000, exactly.  Parsing is
 * resource.ParseQuantity of k8s.io/apimachinery v0.22.2 (sign, digits, optional fraction,
 * suffix n u m k M G T P E Ki Mi Gi Ti Pi Ei or e/E exponent), including its inf.Dec
 * path: values it cannot hold as int64Amount are rounded away from zero to 1e-9 and
 * capped at +-(2^63 - 1) — the value core.EvaluateRule compares (operator.go:16-22).
 * PAS_ENOTEXACT if that value has sub-milli precision or is outside int64 milli range;
 * PAS_EINVAL if ParseQuantity would fail. */
int pas_quantity_to_milli(const char* quantity, int64_t* milli_out);
/* The same at any decimal scale: value * 10^places exactly, 0 <= places <= 9 (EINVAL
 * otherwise); PAS_ENOTEXACT if that is not an integer or is outside int64.
 * pas_quantity_to_milli is places = 3. */
int pas_quantity_to_scaled(const char* quantity, int32_t places, int64_t* out);
/* The fewest decimal places (0..9) that hold the parsed value exactly: "1500u" -> 4,
 * "0.0005" -> 4, "1e-7" -> 7, "2k" -> 0, "1.5" -> 1. */
int pas_quantity_decimals(const char* quantity, int32_t* places);
/* The parsed value as the wide pair (whole, nano): value = whole + nano * 10^-9 with
 * 0 <= nano < 10^9, whole = floor(value) ("-0.5" -> (-1, 500000000)).  ParseQuantity keeps at
 * most 9 fractional digits, so every parsed quantity whose floor fits int64 converts exactly,
 * at any precision and with no column-wide scale.  PAS_EINVAL if ParseQuantity would fail;
 * PAS_ENOTEXACT only when the integer part is outside int64 (the int64Amount "1e19"). */
int pas_quantity_to_wide(const char* quantity, int64_t* whole, uint32_t* nano);

/* resource.ParseQuantity(quantity).AsInt64() with `ok` ignored, as the reference uses it
 * (gpuscheduler/utils.go:23, scheduler.go:155).  That is 0 — even for integral values —
 * for an inf.Dec-backed quantity (19 or more significant digits, a fraction with a
 * binary suffix, a binary suffix past the int64Amount precision estimate such as "1Pi",
 * scale below nano) and for an int64Amount with negative scale ("1000m", "10.0");
 * value * 10^scale (0 on overflow) otherwise.  Pass the string the informer decoded: the
 * apiserver stores quantities in canonical form ("1000m" arrives as "1").
 * PAS_EINVAL if ParseQuantity would fail. */
int pas_quantity_as_int64(const char* quantity, int64_t* out);

/* One literal given as a byte span (no terminator; a byte 0 inside is PAS_EINVAL, as is an empty
 * span), parsed by the fixed-width ParseQuantity the device runs per literal
 * (csrc/quantity_fixed.h).  Host only.  Returns the status: PAS_OK, PAS_EINVAL or PAS_ENOTEXACT,
 * those of pas_quantity_to_wide.  Outputs (each may be NULL):
 *   whole, nano   pas_quantity_to_wide's pair (0, 0 unless PAS_OK)
 *   decimals      pas_quantity_decimals, defined unless PAS_EINVAL ("1e19": 0)
 *   fit           the largest places in 0..9 at which pas_quantity_to_scaled succeeds, or -1 if
 *                 none does; never below decimals otherwise
 * An e/E exponent is ParseInt's int64 truncated to int32, as in ParseQuantity, and every sum
 * formed from it is exact: "1e2147483647" is PAS_ENOTEXACT, "1e-2147483647" is (0, 1). */
int pas_quantity_parse_fixed(const char* bytes, int64_t len, int64_t* whole, uint32_t* nano,
                             int32_t* decimals, int32_t* fit);

/* Quantity.AsInt64 of one literal given as a byte span, from the same routine: *out is what
 * pas_quantity_as_int64 answers (0 for an inf.Dec-backed literal, for an int64Amount with a
 * negative scale and on overflow; value * 10^scale otherwise, scale = exponent - fraction digits).
 * Host only.  Returns the status of pas_quantity_parse_fixed ("1e19": PAS_ENOTEXACT and 0); out
 * may be NULL. */
int pas_quantity_as_int64_fixed(const char* bytes, int64_t len, int64_t* out);

/* A batch of literals parsed on the device, one lane per literal: literal i is
 * bytes[lit_off[i] .. lit_off[i + 1]).  Per literal the outputs of pas_quantity_parse_fixed
 * (whole, nano 0 unless its status is PAS_OK; an output array may be NULL).  The call returns
 * PAS_OK whatever the literals' statuses are; n = 0 is valid.
 * The host form stages its arrays and returns PAS_EINVAL unless lit_off starts at 0 and never
 * decreases.  The _device form checks nothing of d_lit_off: both ends of every span are read
 * clamped into [0, n_bytes] and the end not before the begin, so no offset takes the kernel
 * outside d_bytes; a span that clamps to empty is PAS_EINVAL in its status.  It is asynchronous
 * on hip_stream. */
int pas_quantities_to_wide(pas_ctx* ctx, int64_t n, const int64_t* lit_off, const char* bytes,
                           int64_t* whole, uint32_t* nano, int32_t* decimals, int32_t* status);
int pas_quantities_to_wide_device(pas_ctx* ctx, int64_t n, int64_t n_bytes,
                                  const int64_t* d_lit_off, const char* d_bytes,
                                  int64_t* d_whole, uint32_t* d_nano, int32_t* d_decimals,
                                  int32_t* d_status, void* hip_stream);

/* ------------------------------------------------------------------------- */
/* Telemetry Aware Scheduling                                                */
/* ------------------------------------------------------------------------- */

/* Upload a node-metric snapshot: the content of AutoUpdatingCache's
 * "metrics/<name>" entries (cache/autoupdating.go:76-85) as SoA columns.
 *   v_milli [n_metrics][n_nodes]      value * 1000 (ignored where not present), or
 *                                     value * 10^scale[m] with pas_tas_snapshot_set_scale
 *   present [n_metrics][W64(n_nodes)] node has this metric (NodeMetricsInfo key set)
 * The device builds per-metric sorted orders once here, so that per-request
 * evaluation never sorts (core.OrderedList, operator.go:30-42, sorts per request).
 * gen is an opaque generation id checked by the eval calls (PAS_ESTALE). */
int pas_tas_snapshot_set(pas_ctx* ctx, uint64_t gen, int32_t n_nodes, int32_t n_metrics,
                         const int64_t* v_milli, const uint64_t* present);
int pas_tas_snapshot_set_device(pas_ctx* ctx, uint64_t gen, int32_t n_nodes, int32_t n_metrics,
                                const int64_t* d_v_milli, const uint64_t* d_present,
                                void* hip_stream);
int pas_tas_snapshot_info(const pas_ctx* ctx, uint64_t* gen, int32_t* n_nodes,
                          int32_t* n_metrics);

/* Decimal scale of each column of the resident snapshot generation gen: column m holds
 * value * 10^col_scale[m] (0 <= col_scale[m] <= 9, host array of n_metrics = the snapshot's
 * metric count).  Every column is 3 (milli) after pas_tas_snapshot_set[_device]; a column
 * refresh keeps the column's scale.  Rule targets are integers (TASPolicyRule.Target,
 * telemetrypolicy/api/v1alpha1/types.go:31-35), so core.EvaluateRule's CmpInt64
 * (operator.go:16-22) is exact against target * 10^scale (saturated past int64), and
 * OrderedList's Cmp (:37,39) is the integer order of one column: sub-milli metric values
 * evaluate on the device exactly.  Every int64 value is valid in a narrow
 * column at any scale, -2^63 and 2^63 - 1 included, and every int64 target is compared
 * exactly against it (at scale 0 nothing saturates: the target is compared as it is).
 * Order this call after evaluations on
 * other streams that still read the snapshot, as a snapshot change; it is synchronous on
 * hip_stream (NULL: the context's stream). */
int pas_tas_snapshot_set_scale(pas_ctx* ctx, uint64_t gen, int32_t n_metrics,
                               const int32_t* col_scale, void* hip_stream);

/* Column refresh: AutoUpdatingCache.updateMetric replaces one metric's whole node map
 * (cache/autoupdating.go:45-73, WriteMetric :100-112).  Replaces the resident snapshot's
 * columns cols[0 .. n_cols) (distinct metric indices, host array) with
 * v_milli[n_cols][n_nodes] / present[n_cols][W64] and rebuilds only their orders; the
 * snapshot moves from generation gen_from (PAS_ESTALE otherwise) to gen_to.  Node count and
 * metric count are unchanged (pas_tas_snapshot_reshape adds node slots and adds, drops or
 * moves metric columns on the device).
 * The _device form is asynchronous on hip_stream except for the copy of cols. */
int pas_tas_snapshot_update(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_cols,
                            const int32_t* cols, const int64_t* v_milli,
                            const uint64_t* present);
int pas_tas_snapshot_update_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                   int32_t n_cols, const int32_t* cols, const int64_t* d_v_milli,
                                   const uint64_t* d_present, void* hip_stream);

/* Wide columns: columns whose values do not all fit int64 at one decimal scale (a byte
 * counter past 9.22e15, 1e-7 next to 1e12, more than 18 significant digits).  Replaces
 * columns cols[0 .. n_cols) of the resident snapshot with wide columns
 *   whole [n_cols][n_nodes] int64, nano [n_cols][n_nodes] uint32, present [n_cols][W64]
 * (pas_quantity_to_wide; ignored where not present).  The order of a wide column is the
 * exact order of the pairs (whole signed, then nano unsigned; ties in ascending node index),
 * and every rule compare against an integer target is exact:  v < t <=> whole < t,
 * v == t <=> whole == t and nano == 0,  v > t <=> whole > t or (whole == t and nano != 0).
 * Filter, prioritize, the deschedule sweep (both forms) and the request prioritize evaluate
 * wide columns; so do the top-k entry points with wide merge records
 * (pas_tas_topk_wide_device, pas_tas_gas_topk_wide_device and their merges).  The 64-bit
 * record forms (pas_tas_topk_device, pas_tas_gas_topk_device) return PAS_ENOTEXACT while the
 * resident snapshot holds a wide column: use the wide entry points there.
 * The contract is pas_tas_snapshot_update[_device]'s: gen_from is checked (PAS_ESTALE), the
 * generation moves to gen_to in the same call, only these columns' orders are rebuilt; the
 * _device form is asynchronous on hip_stream except for the copy of cols.  The host form
 * rejects a nano >= 10^9 (PAS_EINVAL); the device form reads nano clamped to 999999999.
 * pas_tas_snapshot_set[_device] makes every column narrow again; pas_tas_snapshot_update
 * [_device] on a wide column makes it narrow at the column's recorded scale;
 * pas_tas_snapshot_set_scale ignores its entries for wide columns.  The wide parts' storage is
 * allocated when a first wide column arrives. */
int pas_tas_snapshot_update_wide(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                 int32_t n_cols, const int32_t* cols, const int64_t* whole,
                                 const uint32_t* nano, const uint64_t* present);
int pas_tas_snapshot_update_wide_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                        int32_t n_cols, const int32_t* cols,
                                        const int64_t* d_whole, const uint32_t* d_nano,
                                        const uint64_t* d_present, void* hip_stream);

/* Column refresh from the Quantity literals themselves: a metric refresh as it arrives
 * (NodeMetricsInfo, {node: resource.Quantity}, metrics/client.go:25-32) installs its columns in
 * one call, parsed, scaled and encoded on the device.  The result is exactly what
 * snapshot.tas_snapshot_from_metrics_wide + pas_tas_snapshot_update + pas_tas_snapshot_update_wide
 * + pas_tas_snapshot_set_scale install.
 *   cols, col_off  host arrays in both forms: column cols[c] (distinct, inside the snapshot, else
 *                  PAS_EINVAL) is replaced by the entries [col_off[c], col_off[c + 1]), as
 *                  updateMetric replaces a metric's whole node map; col_off starts at 0, never
 *                  decreases, T = col_off[n_cols] <= INT32_MAX
 *   entry_node [T] the node slot of each entry
 *   lit_off [T+1], bytes   entry i's literal is bytes[lit_off[i] .. lit_off[i + 1])
 *   kind_out [n_cols]      0 narrow, 1 wide (may be NULL)
 *   scale_out [n_cols]     the column's recorded scale after the call (may be NULL)
 *   bad_entry              see 1 (may be NULL)
 * 1. Every entry of every column is parsed (pas_quantity_parse_fixed), whatever its node.  If
 *    any status is not PAS_OK the call returns the status of the lowest such entry, writes that
 *    entry's index to bad_entry and changes nothing: the snapshot stays valid at gen_from.
 *    Otherwise bad_entry is -1.
 * 2. The entries with 0 <= entry_node < n_nodes are in range; the others take no further part.
 * 3. k = the most decimals among the column's in-range entries (0 if none), s = max(k, 3).
 * 4. The column is narrow at scale s iff every in-range entry has fit >= s: it then holds
 *    value * 10^s and its recorded scale becomes s.  Otherwise it is wide, holds the (whole,
 *    nano) pairs, and its recorded scale stays what it was.
 * 5. Presence is exactly the in-range nodes; a column with no in-range entry becomes empty,
 *    narrow, milli.  A node listed twice in one column is PAS_EINVAL in the host form.  In the
 *    _device form the entry with the highest index gives the value, while 3 and 4 count every
 *    in-range entry.
 * 6. The orders of these columns, and only these, are rebuilt; the narrow ones' scale table
 *    entries are written on the same stream before; the generation is published once, as
 *    gen_to, and no state between gen_from and gen_to is ever valid.  n_cols = 0 moves the
 *    generation only.  PAS_ESTALE and PAS_ENOSNAP as pas_tas_snapshot_update.
 * The narrow / wide marks and the scales are host state, decided from a per-column summary the
 * call reads back: both forms are synchronous on hip_stream (the host form on the context's
 * stream), like pas_tas_snapshot_set_scale and pas_tas_snapshot_reshape.  The _device form
 * reads d_lit_off clamped as pas_quantities_to_wide_device does.  Workspace comes from the
 * stream's slot and only grows. */
int pas_tas_snapshot_update_quantities(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                       int32_t n_cols, const int32_t* cols,
                                       const int64_t* col_off, const int32_t* entry_node,
                                       const int64_t* lit_off, const char* bytes,
                                       int32_t* kind_out, int32_t* scale_out,
                                       int64_t* bad_entry);
int pas_tas_snapshot_update_quantities_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                              int32_t n_cols, const int32_t* cols,
                                              const int64_t* col_off, int64_t n_bytes,
                                              const int32_t* d_entry_node,
                                              const int64_t* d_lit_off, const char* d_bytes,
                                              int32_t* kind_out, int32_t* scale_out,
                                              int64_t* bad_entry, void* hip_stream);
/* Change the shape of the resident snapshot on the device: node slots are appended and metric
 * columns added, dropped or moved, without a host copy and without a sort (the orders of a
 * kept column do not change; its rows are gathered into the new pitch and their pads
 * rewritten).  The reference's cache does this all the time: WriteMetric(name, nil) for the
 * rules of a new policy (controller.go:83-87,142-146), DeleteMetric with the last user
 * (autoupdating.go:127-137), and a refresh whose node map lists a node first seen (:62-72).
 *   n_nodes_new    >= the resident n_nodes (PAS_EINVAL otherwise: nodes only grow, as in
 *                  pas_gas_snapshot_resize); slots [n_nodes, n_nodes_new) carry no present
 *                  bit in any column
 *   n_metrics_new  >= 0
 *   src_col        host [n_metrics_new]: new column m is old column src_col[m] with its
 *                  values, presence, recorded scale and narrow / wide kind, or, for -1, an
 *                  empty column (no node present, scale milli, narrow).  Any other value and
 *                  an old column named twice are PAS_EINVAL.  NULL: old column m for m <
 *                  n_metrics, -1 from there on (PAS_EINVAL when n_metrics_new < n_metrics).
 * gen_from is checked (PAS_ESTALE, PAS_ENOSNAP without a snapshot; nothing changed) and the
 * snapshot moves to gen_to.  The limits are pas_tas_snapshot_set's (PAS_ECAPACITY: 3 *
 * n_metrics_new * padded n_nodes_new < 2^31; checked before anything is allocated).  The same
 * shape with every column in place moves the generation only.  Synchronous on hip_stream (NULL:
 * the context's stream): new storage is allocated and filled by one gather kernel, hip_stream
 * and the context's stream are synchronized, then the old storage is freed; the caller orders
 * the call after readers on other streams, as for every snapshot change.  When the new
 * storage cannot be allocated the old snapshot stays valid and untouched (PAS_ENOMEM); a HIP
 * failure after that leaves the context without a TAS snapshot (PAS_ENOSNAP until the next
 * pas_tas_snapshot_set).  Afterwards every evaluation answers what it would on a snapshot
 * built from the same content by pas_tas_snapshot_set + pas_tas_snapshot_set_scale +
 * pas_tas_snapshot_update_wide.  The wide parts' storage is carried over when a kept column is
 * wide and otherwise allocated again by the next wide update. */
int pas_tas_snapshot_reshape(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                             int32_t n_nodes_new, int32_t n_metrics_new,
                             const int32_t* src_col /* host [n_metrics_new], or NULL */,
                             void* hip_stream);
/* Renumber the node slots of the resident snapshot on the device: dead slots are dropped, the
 * others move down, without a host copy and without a sort.  Every refresh of the reference's
 * cache replaces a metric's whole node map (autoupdating.go:62-72), so a node that left the
 * cluster is in no map after one sync period; here its slot stays until a compaction drops it.
 *   n_nodes_new    >= 0; smaller than, equal to or larger than the resident n_nodes
 *   src_node       host [n_nodes_new]: new slot j holds old slot src_node[j] with its value,
 *                  nano and presence in every column, or, for -1, nothing (a spare slot: no
 *                  present bit in any column).  The entries >= 0 are strictly increasing and <
 *                  n_nodes, -1 may stand anywhere; anything else is PAS_EINVAL.  An old slot that
 *                  no entry names is dropped from every column and from its three orders.
 * Removing ids from a sorted list leaves it sorted and the monotone map keeps ties in ascending
 * node index, so the orders are compacted in place of being sorted again: a stable stream
 * compaction of the order rows (counts per 1024-position segment, their scan, a ranked
 * scatter; no atomics, so the result is reproducible) and a gather of the value rows.  Metric
 * columns, recorded scales and the narrow / wide kinds stay as they are.  Generation, errors,
 * limits and storage are pas_tas_snapshot_reshape's: gen_from is checked (PAS_ESTALE,
 * PAS_ENOSNAP; nothing changed), PAS_ECAPACITY before anything is allocated, PAS_ENOMEM leaves
 * the old snapshot valid, synchronous on hip_stream with the old storage freed after both
 * streams are synchronized, a HIP failure after the launch leaves PAS_ENOSNAP; the identity map
 * moves the generation only.  Afterwards every evaluation answers what it would on a snapshot
 * built from the same content by pas_tas_snapshot_set + pas_tas_snapshot_set_scale +
 * pas_tas_snapshot_update_wide. */
int pas_tas_snapshot_compact(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                             int32_t n_nodes_new, const int32_t* src_node /* host [n_nodes_new] */,
                             void* hip_stream);
/* Read back the resident snapshot and its generation; any output may be NULL.  present_out
 * has the bits at and past n_nodes cleared; values and nanos are meaningful only where the
 * bit is set.  scale_out is each column's recorded decimal scale, wide_out 1 for a wide
 * column; nano_out is zero for every narrow column. */
int pas_tas_snapshot_get(pas_ctx* ctx, uint64_t* gen, int64_t* vals_out /*[M][N]*/,
                         uint64_t* present_out /*[M][W64]*/, int32_t* scale_out /*[M]*/,
                         uint8_t* wide_out /*[M]*/, uint32_t* nano_out /*[M][N]*/);
/* Forget the resident TAS snapshot (its storage is kept): every call that checks a
 * generation answers PAS_ENOSNAP until the next pas_tas_snapshot_set[_device].  For a
 * binding that installs a snapshot in two steps (set, then the wide columns) and must not
 * leave the first step's state behind when the second fails. */
int pas_tas_snapshot_drop(pas_ctx* ctx);
/* Number of wide columns of the resident snapshot (PAS_ENOSNAP without one). */
int pas_tas_snapshot_wide_count(const pas_ctx* ctx, int32_t* n_wide);

#define PAS_TAS_FILTER 1u      /* produce pass_out (MetricsExtender.filterNodes) */
#define PAS_TAS_PRIORITIZE 2u  /* produce order_out/order_len (prioritizeNodesForRule) */

/* Batched TAS filter + prioritize for n_pods pending pods against the resident
 * snapshot.  Replaces, per pod:
 *   filter:     dontschedule.Strategy.Violated (dontschedule/strategy.go:25-44) and the
 *               candidate loop of MetricsExtender.filterNodes (telemetryscheduler.go:204-211)
 *   prioritize: prioritizeNodesForRule (telemetryscheduler.go:128-149) with
 *               core.OrderedList (operator.go:30-42).
 * Inputs
 *   rules, rule_off  CSR of each pod's dontschedule rules: pod p owns
 *                    rules[rule_off[p] .. rule_off[p+1])
 *   prio             [n_pods] scheduleonmetric Rules[0] (getSchedulingRule,
 *                    telemetryscheduler.go:115-124); metric < 0 = no rule / missing metric
 *   cand             [n_pods][W64] candidate bitmaps (args.Nodes), or NULL = every node
 * Outputs
 *   pass_out   [n_pods][W64]  cand AND NOT violated            (flag PAS_TAS_FILTER)
 *   order_out  [n_pods][n_nodes], order_len [n_pods]           (flag PAS_TAS_PRIORITIZE)
 *              node indices of prioritize candidates that have the metric, best first;
 *              HostPriority.Score of entry i is 10 - i (telemetryscheduler.go:145).
 *              Candidates are pass_out when PAS_TAS_FILTER is also set (kube-scheduler
 *              prioritizes the filter-feasible nodes), else cand.
 * Order (the reference's is Go-map order + unstable sort.Slice, i.e. unspecified for
 * ties and for operators other than LessThan/GreaterThan): GreaterThan = value
 * descending, LessThan = value ascending, ties by ascending node index; any other
 * operator = ascending node index.  The oracle uses the same rule.
 * The _device form cannot check d_rule_off on the host: each pod's span is read clamped,
 * [a, b) with a = clamp(rule_off[p], 0, n_rules), b = clamp(rule_off[p+1], a, n_rules), so an
 * offset array that is not a CSR never takes a kernel outside the rules. */
int pas_tas_eval(pas_ctx* ctx, uint64_t gen, int32_t n_pods, const pas_rule* rules,
                 const int32_t* rule_off, const pas_rule* prio, const uint64_t* cand,
                 uint32_t flags, uint64_t* pass_out, int32_t* order_out, int32_t* order_len);
int pas_tas_eval_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t n_rules,
                        const pas_rule* d_rules, const int32_t* d_rule_off,
                        const pas_rule* d_prio, const uint64_t* d_cand, uint32_t flags,
                        uint64_t* d_pass_out, int32_t* d_order_out, int32_t* d_order_len,
                        void* hip_stream);

/* Prioritize of ONE extender request in the request's own terms.  Replaces
 * prioritizeNodesForRule (telemetryscheduler.go:128-149) + core.OrderedList
 * (operator.go:30-42) for args.Nodes.Items given as
 *   req_node [n_req]  snapshot node index of Items[j] (pas_decode_args' req_node; -1 or any
 *                     index outside [0, n_nodes) = a node the snapshot does not hold)
 *   prio              the pod's scheduleonmetric Rules[0] (host struct); metric < 0 = no
 *                     rule / metric not cached -> empty list
 * Outputs
 *   pos_out  [n_req]  request positions j of the listed nodes, best first (-1 past len);
 *                     HostPriority i is {Items[pos_out[i]].Name, 10 - i}
 *   len_out           entries: the distinct request nodes that have the metric
 * Order: GreaterThan value descending, LessThan ascending, ties by ascending position of
 * the node's first occurrence in the request; any other operator: first occurrences in
 * request order.  (pas_tas_eval breaks ties by snapshot node index instead; the two agree
 * when the request lists nodes in snapshot order.)  A repeated name is listed once
 * (filteredNodeData is a map, :135-139).  The _device form takes device req_node /
 * pos_out / len_out and is asynchronous on hip_stream. */
int pas_tas_prioritize_request(pas_ctx* ctx, uint64_t gen, const pas_rule* prio, int32_t n_req,
                               const int32_t* req_node, int32_t* pos_out, int32_t* len_out);
int pas_tas_prioritize_request_device(pas_ctx* ctx, uint64_t gen, const pas_rule* prio,
                                      int32_t n_req, const int32_t* d_req_node,
                                      int32_t* d_pos_out, int32_t* d_len_out,
                                      void* hip_stream);

/* The extender verbs for a BATCH of R requests, each with its own node list, in request
 * terms (micro-batched concurrent requests).  Shared by the three
 * families below (pas_tas_prioritize_requests, pas_tas_filter_requests,
 * pas_gas_fit_requests):
 *   req_off  [R + 1]  HOST array in both forms: request r lists req_off[r + 1] - req_off[r]
 *                     nodes.  req_off[0] = 0, non-decreasing, T = req_off[R] <= INT32_MAX
 *                     (else PAS_EINVAL).  R = 0 and empty requests are valid.
 *   req_node [T]      the requests' snapshot node ids back to back, as pas_decode_args
 *                     writes them; a value outside [0, n_nodes) = a node the snapshot does
 *                     not hold.  No kernel reads outside its arrays, whatever it holds.
 * Bitmap outputs have a row pitch: request r's row is out[r * ld_words ..), ld_words >=
 * W64(longest request).  Bit j belongs to request position j; bits at and past the request's
 * length are written 0 up to W64(n_req_r) words, words past that are left untouched.  A row
 * is what pas_encode_tas_filter_result / pas_encode_gas_filter_result take with req_node =
 * 0 .. n - 1.  The _device forms take device req_node / outputs, draw their workspace from
 * the stream's slot and are asynchronous on hip_stream (apart from the copy of their host
 * arrays).  Nothing resident is written and no generation moves.
 *
 * pas_tas_prioritize_requests: request r gets exactly the output of
 * pas_tas_prioritize_request(gen, &prio[r], n_r, req_node + req_off[r], ..): request-local
 * positions at pos_out[req_off[r] + i], -1 past len_out[r].  prio [R] is a host array in
 * both forms; prio[r].metric < 0 = empty list, >= n_metrics PAS_EINVAL.  Two requests of one
 * batch that list the same node do not see each other. */
int pas_tas_prioritize_requests(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                const int32_t* req_off, const pas_rule* prio,
                                const int32_t* req_node, int32_t* pos_out, int32_t* len_out);
int pas_tas_prioritize_requests_device(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                       const int32_t* req_off, const pas_rule* prio,
                                       const int32_t* d_req_node, int32_t* d_pos_out,
                                       int32_t* d_len_out, void* hip_stream);

/* pas_tas_filter_requests: MetricsExtender.filterNodes per request.  Bit j of request r's
 * row is set iff the node at position j is unknown to the snapshot or violates none of the
 * request's dontschedule rules rules[rule_off[r] .. rule_off[r + 1]) (pas_tas_eval's rule
 * semantics: a metric that is not cached or that the node lacks skips the rule).  A repeated
 * node keeps its verdict at every position.  The host form validates the CSR and the
 * operators as pas_tas_eval does; the _device form reads d_rule_off clamped into
 * [0, n_rules] and skips unknown operators, as pas_tas_eval_device. */
int pas_tas_filter_requests(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                            const int32_t* req_off, const pas_rule* rules,
                            const int32_t* rule_off, const int32_t* req_node,
                            uint64_t* pass_out, int64_t ld_words);
int pas_tas_filter_requests_device(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                   const int32_t* req_off, int32_t n_rules,
                                   const pas_rule* d_rules, const int32_t* d_rule_off,
                                   const int32_t* d_req_node, uint64_t* d_pass_out,
                                   int64_t ld_words, void* hip_stream);

/* Deschedule sweep: for each registered deschedule strategy s (rules
 * rules[rule_off[s] .. rule_off[s+1])), the node set of deschedule.Strategy.Violated
 * (deschedule/strategy.go:31-50), as the bitmap viol_out[s][W64].  The per-node
 * policy lists of nodeStatusForStrategy (deschedule/enforce.go:154-164) are the
 * columns of this matrix.  The _device forms (and pas_tas_deschedule_device) read d_rule_off
 * clamped into [0, n_rules] and non-decreasing, in strategy order, so an offset array that is
 * not a CSR never takes the sweep outside the rules or the strategies. */
int pas_tas_violations(pas_ctx* ctx, uint64_t gen, int32_t n_strategies, const pas_rule* rules,
                       const int32_t* rule_off, uint64_t* viol_out);
int pas_tas_violations_device(pas_ctx* ctx, uint64_t gen, int32_t n_strategies,
                              int32_t n_rules, const pas_rule* d_rules,
                              const int32_t* d_rule_off, uint64_t* d_viol_out,
                              void* hip_stream);

/* The resident policy table: the TASPolicy objects the reference keeps in its cache
 * (WritePolicy / ReadPolicy / DeletePolicy, cache/types.go:11-22) and keeps current through
 * the controller's onAdd / onUpdate / onDelete (controller/controller.go:61-176).  Its verbs
 * read a pod's policy on every request (getPolicyFromPod, telemetryscheduler.go:103-112); here
 * a pod or a request names a row of the table, its policy id.
 *   rules, rule_off   CSR of the policies' dontschedule rules: policy i owns
 *                     rules[rule_off[i] .. rule_off[i + 1])
 *   prio              [n_policies] scheduleonmetric Rules[0]; metric < 0 = none, as in
 *                     pas_tas_eval
 * All host arrays (the table is a few KB).  The call replaces any earlier table; n_policies = 0
 * is a valid table.  Metric indices are columns of the resident TAS snapshot: PAS_ENOSNAP
 * without one.  An unknown operator is accepted here: the reference panics only where the rule
 * is evaluated (operator.go:25), and so do the verbs below.  Synchronous on the context's
 * stream; order it after policy verbs that still run on other streams, as a snapshot change.
 *
 * The table against the snapshot.  Column numbering: pas_tas_snapshot_set[_device],
 * pas_tas_snapshot_reshape (unless it moves the generation only) and pas_tas_snapshot_drop can
 * renumber or re-create columns; a policy verb called with a table set before such a call
 * returns PAS_ESTALE (its message names the policy table; a generation mismatch names the
 * generation): resolve the metric names again and set the table again.  Values:
 * pas_tas_snapshot_update[_wide][_device], pas_tas_snapshot_set_scale and
 * pas_tas_snapshot_compact keep the table valid.
 *
 * Derived: the policies' violating sets, viol [n_policies][W64] (dontschedule.Violated,
 * dontschedule/strategy.go:25-44, depends only on the rules and the metric cache).  The first
 * policy verb after the snapshot's content or the table changed builds them with the
 * deschedule sweep on its own stream; later verbs read them, verbs on other streams ordered
 * after the build by an event, never by the host.  pas_tas_policies_info: PAS_EINVAL without a
 * table.  pas_tas_policies_drop forgets the table (its storage is kept): the policy verbs
 * answer PAS_EINVAL until the next set. */
int pas_tas_policies_set(pas_ctx* ctx, int32_t n_policies, const pas_rule* rules,
                         const int32_t* rule_off, const pas_rule* prio);
int pas_tas_policies_info(const pas_ctx* ctx, int32_t* n_policies, int32_t* n_rules);
int pas_tas_policies_drop(pas_ctx* ctx);

/* The cached violating sets viol_out [n_policies][W64] (built if needed): what
 * pas_tas_violations answers for the table's rules.  A binding can answer single filter
 * requests from them in host memory between two refreshes.  The operators are not validated
 * (an unknown one is skipped, as in pas_tas_violations_device). */
int pas_tas_policies_violated(pas_ctx* ctx, uint64_t gen, uint64_t* viol_out);
int pas_tas_policies_violated_device(pas_ctx* ctx, uint64_t gen, uint64_t* d_viol_out,
                                     void* hip_stream);

/* pas_tas_eval[_device] by policy id: exactly its outputs (pass_out, order_out, order_len; the
 * flags, cand and the candidate rule as there) with pod p's rules and prio being table row
 * pod_policy[p].  -1 = no dontschedule rules and no prio rule: pass = cand, empty list.  With
 * PAS_TAS_FILTER alone the call is one pass over the bitmaps (pass = cand AND NOT viol[id]);
 * with PAS_TAS_PRIORITIZE alone the bitmaps are not consulted.  The host form returns
 * PAS_EINVAL for an id outside [-1, n_policies) and, as pas_tas_eval, for an unknown operator
 * on a cached non-empty column in a policy the batch references (a policy no pod names does not
 * fail the call); the device form reads an id outside the range as -1 and skips unknown
 * operators. */
int pas_tas_eval_policies(pas_ctx* ctx, uint64_t gen, int32_t n_pods, const int32_t* pod_policy,
                          const uint64_t* cand, uint32_t flags, uint64_t* pass_out,
                          int32_t* order_out, int32_t* order_len);
int pas_tas_eval_policies_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods,
                                 const int32_t* d_pod_policy, const uint64_t* d_cand,
                                 uint32_t flags, uint64_t* d_pass_out, int32_t* d_order_out,
                                 int32_t* d_order_len, void* hip_stream);

/* pas_tas_filter_requests[_device] by policy id: its contract (row pitch, tail bits, unknown
 * nodes pass, a repeated node keeps its verdict) with request r's rules being table row
 * req_policy[r].  req_policy [R] is a host array in both forms, as req_off; ids are handled as
 * in pas_tas_eval_policies (host form PAS_EINVAL, device form -1).  Prioritize in request terms
 * needs no verb of its own: pas_tas_prioritize_requests takes a host prio [R]. */
int pas_tas_filter_requests_policies(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                     const int32_t* req_off, const int32_t* req_policy,
                                     const int32_t* req_node, uint64_t* pass_out,
                                     int64_t ld_words);
int pas_tas_filter_requests_policies_device(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                            const int32_t* req_off, const int32_t* req_policy,
                                            const int32_t* d_req_node, uint64_t* d_pass_out,
                                            int64_t ld_words, void* hip_stream);

/* Deschedule label plan (Deschedule.updateNodeLabels, deschedule/enforce.go:99-151) for
 * n_strategies <= 64 strategies from a sweep's viol[s][W64(n_nodes)] and the nodes' labels.
 * The reference keys its non-violated set by policy NAME (allPolicies, :89-95), and two
 * registered strategies may share a name (SetPolicyName drops the namespace,
 * controller/controller.go:80; AddStrategy drops only Equals duplicates,
 * core/enforcer.go:84-103):
 *   name_id      [s] host array: strategies s and t share a policy name iff
 *                name_id[s] == name_id[t] (any int32 values); NULL = all names distinct.
 *                A name is represented by its first strategy k (lowest index).
 *   labels       [s][W64] bit set = the node carries label <policy name of s> (any value);
 *                only the rows of each name's first strategy are read; NULL = no node
 *                carries any
 *   add_out      [n_nodes] bit s = strategy s violated at the node: add "<name>":
 *                "violating", one entry per violating strategy (:108-117)
 *   remove_out   [n_nodes] bit k = name k (its first strategy) violated by none of its
 *                strategies and carried: remove it, then add it as "null" (:118-132)
 *   total_out    the function's int result: the count of NON-violated (node, name) pairs
 *                (totalViolations++ sits in the non-violated loop, :133)
 * More than 64 strategies: call per group of <= 64 that keeps every name's strategies
 * together, OR the masks' strategy offsets back in and sum the totals (DescheduleEnforcer).
 * pas_label_patch_json renders one node's masks as the PATCH body.  The _device forms take
 * device viol / labels / outputs and a host name_id, and are asynchronous on hip_stream. */
int pas_tas_label_plan(pas_ctx* ctx, int32_t n_nodes, int32_t n_strategies,
                       const uint64_t* viol, const int32_t* name_id, const uint64_t* labels,
                       uint64_t* add_out, uint64_t* remove_out, int64_t* total_out);
int pas_tas_label_plan_device(pas_ctx* ctx, int32_t n_nodes, int32_t n_strategies,
                              const uint64_t* d_viol, const int32_t* name_id,
                              const uint64_t* d_labels, uint64_t* d_add_out,
                              uint64_t* d_remove_out, int64_t* d_total_out, void* hip_stream);

/* The deschedule sweep and its label plan in one pass (Deschedule.Cleanup's violation lists,
 * deschedule/strategy.go:31-50, then updateNodeLabels, enforce.go:99-151): outputs as
 * pas_tas_violations_device (viol_out) followed by pas_tas_label_plan_device on those
 * bitmaps for the snapshot's n_nodes (name_id / labels / add_out / remove_out / total_out),
 * without re-reading the bitmaps.  n_strategies <= 64. */
int pas_tas_deschedule_device(pas_ctx* ctx, uint64_t gen, int32_t n_strategies,
                              int32_t n_rules, const pas_rule* d_rules,
                              const int32_t* d_rule_off, uint64_t* d_viol_out,
                              const int32_t* name_id, const uint64_t* d_labels,
                              uint64_t* d_add_out, uint64_t* d_remove_out, int64_t* d_total_out,
                              void* hip_stream);

/* json.Marshal of the node's []patchValue (enforce.go:21-25, 74-86) for the masks of
 * pas_tas_label_plan: adds in strategy order, then a remove + add "null" pair per removed
 * label in the order of the names' first strategies (the reference emits these in Go-map
 * order).  names[s] = policy name of strategy s.  Writes at most cap bytes (no terminator); *len = full length;
 * PAS_ECAPACITY if it exceeds cap.  Host-only. */
int pas_label_patch_json(int32_t n_strategies, const char* const* names, uint64_t add_mask,
                         uint64_t remove_mask, char* buf, int64_t cap, int64_t* len);

/* The label plan as a patch list: one record per node whose PATCH body is not "[]", in
 * ascending node index, compacted on the device, so that an enforcer reads and patches only
 * the nodes that change.  viol, name_id, labels and total_out are those of pas_tas_label_plan,
 * and add[node] / rem[node] below are its masks.  Two optional bitmaps describe the VALUES of
 * the carried labels, in the shape and row convention of labels ([s][W64], only the rows of
 * each name's first strategy k read, and only where the labels bit is set; both ignored when
 * labels is NULL):
 *   violating    bit (k, node): the node's label <name k> has the value "violating"
 *   null_        bit (k, node): it has the value "null"
 * The reduced masks drop what would write a value the label already holds:
 *   add'[node]   add[node] without the bits of EVERY strategy of name k where
 *                labels & violating has bit (k, node) (two violating strategies of one name
 *                write the same label)
 *   rem'[node]   rem[node] & ~(labels & null_)[k]
 * Applying the reduced patch gives the node the labels the full patch gives it.  A bit set in
 * both value bitmaps is contradictory input; each bitmap is applied as stated, so the result is
 * defined.  With both NULL the list is exactly the nodes of a non-empty reference body.
 *   patch_node   [cap] int32 node index, ascending
 *   patch_add    [cap] add' of that node
 *   patch_rem    [cap] rem' of that node
 *   n_patches    the nodes with add' | rem' != 0, also when that exceeds cap
 *   total_out    as pas_tas_label_plan (it does not depend on the values)
 * Records [0, min(cap, n_patches)) are written and are the first in node order; nothing at or
 * past that is touched: call again with larger arrays, as with the side buffer of
 * pas_gas_fit_ex.  cap = 0 with NULL record arrays only counts.  n_nodes = 0 or
 * n_strategies = 0: n_patches = 0, total 0.  Shape limits and errors as pas_tas_label_plan.
 * The order comes from a segmented count, a scan and a ranked scatter: no atomics, so a list is
 * reproducible.  The host form copies back only min(cap, n_patches) records.  The _device form
 * takes device bitmaps and outputs (d_n_patches and d_total_out: device int64, valid after the
 * stream) and a host name_id, and is asynchronous on hip_stream. */
int pas_tas_label_patches(pas_ctx* ctx, int32_t n_nodes, int32_t n_strategies,
                          const uint64_t* viol, const int32_t* name_id, const uint64_t* labels,
                          const uint64_t* violating, const uint64_t* null_, int64_t cap,
                          int32_t* patch_node, uint64_t* patch_add, uint64_t* patch_rem,
                          int64_t* n_patches, int64_t* total_out);
int pas_tas_label_patches_device(pas_ctx* ctx, int32_t n_nodes, int32_t n_strategies,
                                 const uint64_t* d_viol, const int32_t* name_id,
                                 const uint64_t* d_labels, const uint64_t* d_violating,
                                 const uint64_t* d_null, int64_t cap, int32_t* d_patch_node,
                                 uint64_t* d_patch_add, uint64_t* d_patch_rem,
                                 int64_t* d_n_patches, int64_t* d_total_out, void* hip_stream);

/* The deschedule sweep and its patch list in one call, as pas_tas_deschedule_device is to
 * pas_tas_violations_device + pas_tas_label_plan_device: the sweep of pas_tas_violations over
 * the resident snapshot, then pas_tas_label_patches on its bitmaps for the snapshot's n_nodes.
 * viol_out [s][W64] is optional: NULL keeps the bitmaps in the call's own workspace (the
 * stream's, in the _device form).  Generation, rule and offset checks as pas_tas_violations
 * (host form) and pas_tas_deschedule_device (_device form, d_rule_off read clamped);
 * n_strategies <= 64. */
int pas_tas_deschedule_patches(pas_ctx* ctx, uint64_t gen, int32_t n_strategies,
                               const pas_rule* rules, const int32_t* rule_off,
                               const int32_t* name_id, const uint64_t* labels,
                               const uint64_t* violating, const uint64_t* null_,
                               uint64_t* viol_out, int64_t cap, int32_t* patch_node,
                               uint64_t* patch_add, uint64_t* patch_rem, int64_t* n_patches,
                               int64_t* total_out);
int pas_tas_deschedule_patches_device(pas_ctx* ctx, uint64_t gen, int32_t n_strategies,
                                      int32_t n_rules, const pas_rule* d_rules,
                                      const int32_t* d_rule_off, const int32_t* name_id,
                                      const uint64_t* d_labels, const uint64_t* d_violating,
                                      const uint64_t* d_null, uint64_t* d_viol_out, int64_t cap,
                                      int32_t* d_patch_node, uint64_t* d_patch_add,
                                      uint64_t* d_patch_rem, int64_t* d_n_patches,
                                      int64_t* d_total_out, void* hip_stream);

/* The bodies of a whole patch list in one call: body i is buf[offsets[i] .. offsets[i + 1]),
 * byte-equal to pas_label_patch_json on (add[i], rem[i]); offsets has n_patches + 1 entries.
 * Writes at most cap bytes; *total_len and every offset hold the full sizes also when
 * PAS_ECAPACITY is returned.  PAS_EINVAL (nothing written) for a mask bit at or past
 * n_strategies in any record.  Host-only. */
int pas_label_patch_json_batch(int32_t n_strategies, const char* const* names,
                               int64_t n_patches, const uint64_t* add, const uint64_t* rem,
                               char* buf, int64_t cap, int64_t* offsets, int64_t* total_len);

/* ------------------------------------------------------------------------- */
/* GPU Aware Scheduling                                                      */
/* ------------------------------------------------------------------------- */

#define PAS_GAS_MAX_CARDS 64      /* cards per node (label gpu.intel.com/cards entries) */
#define PAS_GAS_MAX_RES 4         /* gpu.intel.com/ resource kinds per batch */
#define PAS_GAS_MAX_SELECTIONS 64 /* card selections per pod reported in cards / side records;
                                     pods with more are evaluated exactly (PAS_GAS_SEL_LIMIT) */
#define PAS_GAS_PACKED 8          /* selections / card ranks the packed result word holds */
#define PAS_REQ_UNKNOWN_KIND 0x80000000u /* req_mask: requests a kind the snapshot lacks */
/* bits 24-27 of a result word besides a count S <= PAS_GAS_PACKED: */
#define PAS_GAS_SEL_EXTENDED 15   /* the pod fits (bit 31 set) but its card selection does not
                                     pack: more than 8 selections or a card rank >= 8; the
                                     selection is in the side buffer of pas_gas_fit_ex */
#define PAS_GAS_SEL_LIMIT 14      /* the pod fits (bit 31 set) with more than
                                     PAS_GAS_MAX_SELECTIONS selections: neither packed nor in
                                     the side buffer; pas_gas_bind_counts reports them per
                                     container and card.  Such pods are counted by
                                     pas_gas_limit_count */

/* Card selection of one (pod, node) that does not fit the packed word (PAS_GAS_SEL_EXTENDED):
 * card[0 .. n_sel) are the ranks of the node's cards, selection by selection (containers in
 * order), i.e. the "gas-container-cards" annotation (:317-335). */
typedef struct pas_gas_selection {
  int32_t pod;
  int32_t node;
  int32_t n_sel;
  int32_t reserved;
  uint8_t card[PAS_GAS_MAX_SELECTIONS];
} pas_gas_selection;

/* Frozen allocation snapshot (Cache.getNodeResourceStatus,
 * gpuscheduler/node_resource_cache.go:474-491) in node-major SoA:
 *   n_cards     [n_nodes]  unique card names of label gpu.intel.com/cards; 0 = label
 *                          missing (getNodeGPUList -> nil, scheduler.go:132-148,
 *                          errWontFit at :294-298); -1 = node not in the lister
 *                          (FetchNode error, :282-288)
 *   cap_per_gpu [n_nodes][n_res]        AsInt64(allocatable) / len(label split),
 *                                       truncating (getPerGPUResourceCapacity :164-178);
 *                                       0 where the node lacks the resource
 *   used        [n_nodes][max_cards][n_res] usage of the node's cards in lexicographic
 *                                       (sort.Strings, :216-224) order of card name;
 *                                       cards in the usage map but not in the label are
 *                                       left out (skipped at :230-234)
 * max_cards <= PAS_GAS_MAX_CARDS (64), n_res <= PAS_GAS_MAX_RES.  The host form rejects
 * n_cards[n] > max_cards (PAS_EINVAL); the _device form stores such a count as max_cards.
 *
 * Parked card slots.  A node's row used[n][0 .. max_cards) holds its label cards in slots
 * [0, n_cards[n]); the slots at and past n_cards[n] (all of them for n_cards[n] <= 0) are
 * parked: no fit, bind, placement, release or event reads or changes them (a card rank >=
 * n_cards[n] is "a card the label does not list": PAS_GAS_EV_ADD skips it, PAS_GAS_EV_REMOVE
 * and the releases report PAS_GAS_ERR_INPUT).  They may carry the usage of cards the label
 * does not list at the moment, as the reference's nodeStatuses keeps it by card name
 * (node_resource_cache.go:259-272): pas_gas_snapshot_set[_device] stores them as given,
 * pas_gas_snapshot_get returns them, and only pas_gas_nodes_update[_device] and
 * pas_gas_snapshot_resize move them.  Parked usage therefore changes only by being moved. */
int pas_gas_snapshot_set(pas_ctx* ctx, uint64_t gen, int32_t n_nodes, int32_t max_cards,
                         int32_t n_res, const int32_t* n_cards, const int64_t* cap_per_gpu,
                         const int64_t* used);
int pas_gas_snapshot_set_device(pas_ctx* ctx, uint64_t gen, int32_t n_nodes, int32_t max_cards,
                                int32_t n_res, const int32_t* d_n_cards,
                                const int64_t* d_cap_per_gpu, const int64_t* d_used,
                                void* hip_stream);

/* GAS filter for a batch of pods over every node of the snapshot: one
 * runSchedulingLogic (scheduler.go:280-338) per (pod, node), first-fit over cards
 * with checkResourceCapacity (:341-383).
 *   req       [n_pods][max_containers][n_res] AsInt64 container requests
 *             (containerRequests, utils.go:14-32); res_index i915 identifies
 *             gpu.intel.com/i915 among the n_res kinds (or -1 if absent)
 *   req_mask  [n_pods][max_containers] bit q set = container requests kind q
 *             (the key exists in its resourceMap, even with value 0); bit 31
 *             (PAS_REQ_UNKNOWN_KIND) = the container also requests a gpu.intel.com/ kind
 *             outside the snapshot's n_res kinds.  No node's capacity map has that key, so
 *             every checkResourceCapacity of the container fails (:349-354): with
 *             numI915 > 0 the pod fits no node; with numI915 == 0 it makes no selection
 *             and the flag changes nothing (:206-215)
 *   n_containers [n_pods]
 * Output res_out[n_pods][n_nodes], one word per (pod, node):
 *   bit 31     the pod fits (node passes GASExtender.filterNodes, :467-473)
 *   bits 24-27 number of card selections S (= sum of per-container i915 counts) when
 *              S <= 8 and every selected card rank is < 8; else PAS_GAS_SEL_EXTENDED
 *              (fits, selection in pas_gas_fit_ex's side buffer) or PAS_GAS_SEL_LIMIT
 *   bits 0-23  S 3-bit card ranks (lexicographic index into the node's cards),
 *              selection j at bits 3j..3j+2, containers in order, i.e. the
 *              "gas-container-cards" annotation (:317-335) in packed form; 0 otherwise.
 * The reference has no limit on selections per pod or cards per node (scheduler.go:200-257;
 * the GPU plugin's -shared-dev-num lets one card take many selections); here nodes may have
 * up to PAS_GAS_MAX_CARDS cards, and pods any number of selections (numI915 up to INT64_MAX
 * per container): a container's selections are runs on ascending cards (a card first fit
 * passes over never fits again within the container), evaluated in O(cards).  A fitting pod
 * of more than PAS_GAS_MAX_SELECTIONS selections gets bit 31 | PAS_GAS_SEL_LIMIT << 24.
 * The _device forms read d_n_containers[p] clamped into [0, max_containers] (the host form
 * rejects values outside it with PAS_EINVAL). */
int pas_gas_fit(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                int32_t i915_index, const int64_t* req, const uint32_t* req_mask,
                const int32_t* n_containers, uint32_t* res_out);
int pas_gas_fit_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                       int32_t i915_index, const int64_t* d_req, const uint32_t* d_req_mask,
                       const int32_t* d_n_containers, uint32_t* d_res_out, void* hip_stream);

/* pas_gas_fit plus the side buffer of the selections that do not pack: side[0 .. cap) gets
 * one record per PAS_GAS_SEL_EXTENDED word (in no particular order); *side_count = the number
 * of such words (records beyond cap are dropped: call again with a larger buffer). */
int pas_gas_fit_ex(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                   int32_t i915_index, const int64_t* req, const uint32_t* req_mask,
                   const int32_t* n_containers, uint32_t* res_out, pas_gas_selection* side,
                   int64_t side_cap, int64_t* side_count);
/* d_side_count: device int64, zeroed by the call, then the count (read it after the stream). */
int pas_gas_fit_ex_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                          int32_t i915_index, const int64_t* d_req, const uint32_t* d_req_mask,
                          const int32_t* d_n_containers, uint32_t* d_res_out,
                          pas_gas_selection* d_side, int64_t side_cap, int64_t* d_side_count,
                          void* hip_stream);

/* pas_gas_fit_ex_device with a result row pitch: the word of (pod p, node n) goes to
 * d_res_out[p * ld_res + n], ld_res >= n_nodes (words n_nodes .. ld_res - 1 of a row are not
 * written).  A pitch that is a multiple of 32 words starts every row on a 128-byte line: the
 * fit kernels store a wave's 64 node words as one 256-byte piece of a row, and pieces that
 * straddle lines (every other row of an odd-multiple-of-16 dense pitch, e.g. 50 000) are
 * written ~25 % slower.  The selection side buffer is optional (d_side / d_side_count null,
 * side_cap 0).  Same results as pas_gas_fit_ex_device otherwise (scheduler.go:449-482). */
int pas_gas_fit_ld_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                          int32_t i915_index, const int64_t* d_req, const uint32_t* d_req_mask,
                          const int32_t* d_n_containers, uint32_t* d_res_out, int64_t ld_res,
                          pas_gas_selection* d_side, int64_t side_cap, int64_t* d_side_count,
                          void* hip_stream);

/* Pods of the last GAS fit call on this context with more than PAS_GAS_MAX_SELECTIONS
 * selections (their fitting words are PAS_GAS_SEL_LIMIT).  Waits for the call's stream. */
int pas_gas_limit_count(pas_ctx* ctx, int64_t* n_pods_out);

/* GAS filter verdicts only, as node bitmaps fit_out[n_pods][W64(n_nodes)] (bit = bit 31 of
 * the pas_gas_fit word).  Used to intersect GAS with TAS candidates (cand of the TAS calls)
 * without materialising the per-(pod, node) words. */
int pas_gas_fit_bitmap_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t max_containers,
                              int32_t i915_index, const int64_t* d_req,
                              const uint32_t* d_req_mask, const int32_t* d_n_containers,
                              uint64_t* d_fit_out, void* hip_stream);

/* GAS filter of a batch of requests in request terms (the conventions of
 * pas_tas_prioritize_requests above): pod r (row r of req / req_mask / n_containers, as
 * pas_gas_fit) is request r's pod.  Bit j of request r's row = bit 31 of the pas_gas_fit
 * word of (pod r, node req_node[req_off[r] + j]), 0 for a node the snapshot does not hold
 * (the FetchNode error).  Any number of selections, every card count and
 * PAS_REQ_UNKNOWN_KIND mean what they mean to pas_gas_fit.  The host form validates as
 * pas_gas_fit; the _device form clamps n_containers as pas_gas_fit_device. */
int pas_gas_fit_requests(pas_ctx* ctx, uint64_t gen, int32_t n_requests, const int32_t* req_off,
                         const int32_t* req_node, int32_t max_containers, int32_t i915_index,
                         const int64_t* req, const uint32_t* req_mask,
                         const int32_t* n_containers, uint64_t* fit_out, int64_t ld_words);
int pas_gas_fit_requests_device(pas_ctx* ctx, uint64_t gen, int32_t n_requests,
                                const int32_t* req_off, const int32_t* d_req_node,
                                int32_t max_containers, int32_t i915_index, const int64_t* d_req,
                                const uint32_t* d_req_mask, const int32_t* d_n_containers,
                                uint64_t* d_fit_out, int64_t ld_words, void* hip_stream);

/* Bind-time commit (GASExtender.bindNode, scheduler.go:385-445): for binds b in call order,
 * pod bind_pod[b] (an index into the req / req_mask / n_containers batch, as pas_gas_fit)
 * onto node bind_node[b]: runSchedulingLogic on the node's CURRENT resident usage, then
 * Cache.adjustPodResources(add) with the resulting annotation (node_resource_cache.go:
 * 240-287), applied to the resident used[N][K][Q] in place.  Binds to the same node see
 * each other in call order.  res_out[b] = the pas_gas_fit word for that (pod, node) at bind
 * time, status_out[b] = PAS_GAS_OK or PAS_GAS_WONT_FIT (then nothing changes).  The
 * snapshot moves from generation gen_from (PAS_ESTALE otherwise) to gen_to. */
#define PAS_GAS_OK 0
#define PAS_GAS_WONT_FIT 1
#define PAS_GAS_ERR_INPUT 2    /* resource_map.go errInput: nothing changes */
#define PAS_GAS_ERR_OVERFLOW 3 /* resource_map.go errOverflow: nothing changes */
int pas_gas_bind(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_binds,
                 const int32_t* bind_pod, const int32_t* bind_node, int32_t n_pods,
                 int32_t max_containers, int32_t i915_index, const int64_t* req,
                 const uint32_t* req_mask, const int32_t* n_containers, uint32_t* res_out,
                 int32_t* status_out);
/* pas_gas_bind plus every bind's full card selection: cards_out[b][0 .. n_sel_out[b]) (ranks,
 * selection by selection; n_sel_out 0 when it does not fit), for selections that do not
 * pack into the result word.  A bind of more than PAS_GAS_MAX_SELECTIONS selections has
 * n_sel_out -1 and cards_out zero: pas_gas_bind_counts reports it. */
int pas_gas_bind_ex(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_binds,
                    const int32_t* bind_pod, const int32_t* bind_node, int32_t n_pods,
                    int32_t max_containers, int32_t i915_index, const int64_t* req,
                    const uint32_t* req_mask, const int32_t* n_containers, uint32_t* res_out,
                    int32_t* status_out, uint8_t* cards_out /*[n_binds][64]*/,
                    int32_t* n_sel_out);

/* pas_gas_bind with every bind's selection as counts, for any number of selections:
 * counts_out[b][c][k] = the selections container c made on card k (int64; all 0 when the
 * bind does not fit).  Within a container the selections are in ascending card order (first
 * fit with one per-GPU request never returns to a card it has passed), so the counts are the
 * "gas-container-cards" annotation: container c lists card k counts_out[b][c][k] times, in
 * card order (scheduler.go:200-257, 317-335). */
int pas_gas_bind_counts(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_binds,
                        const int32_t* bind_pod, const int32_t* bind_node, int32_t n_pods,
                        int32_t max_containers, int32_t i915_index, const int64_t* req,
                        const uint32_t* req_mask, const int32_t* n_containers,
                        uint32_t* res_out, int32_t* status_out,
                        int64_t* counts_out /*[n_binds][max_containers][max_cards]*/);

/* Batch placement: the pods of a batch bound in order, each along its row of candidate
 * nodes, e.g. the top_node / top_len of pas_tas_gas_topk_device or the out_node / out_len
 * of pas_topk_merge_device, unchanged.  The call is exactly this loop over the resident
 * usage (N = the snapshot's node count), every bind seeing the binds before it as the
 * reference's pod-after-pod bindNode calls do (scheduler.go:385-445):
 *
 *   for p in 0 .. n_pods-1:                      pod order is the priority order
 *     place_node[p] = -1; place_rank[p] = -1; res_out[p] = 0
 *     for j in 0 .. min(k, cand_len ? cand_len[p] : k) - 1:
 *       n = cand_node[p * ld + j] - node_base
 *       if n < 0 or n >= N: continue             -1 / INT32_MAX padding, other shards' ids
 *       the single bind pas_gas_bind(pod p, node n) on the current usage
 *       if its status is PAS_GAS_OK:             committed
 *         place_node[p] = n + node_base; place_rank[p] = j; res_out[p] = its word; break
 *
 * A pod that fits nowhere changes nothing; a node repeated within a row is tried again.
 * cards_out [n_pods][64] with n_sel_out [n_pods] (both or neither) and counts_out
 * [n_pods][max_containers][max_cards] are optional and mean what they mean in
 * pas_gas_bind_ex / pas_gas_bind_counts for the placing bind (zeros for unplaced pods).
 * *n_placed (optional) = pods placed; *n_rounds (optional) = device rounds taken, a
 * diagnostic.  The snapshot moves from gen_from (PAS_ESTALE otherwise, nothing changed) to
 * gen_to.  PAS_EINVAL for k < 1, ld < k, and in the host form n_containers out of range or
 * mask bits >= n_res.  The _device form takes device pointers (n_placed / n_rounds stay host
 * pointers) and cannot validate the arrays: it reads d_n_containers[p] clamped into
 * [0, max_containers] and d_cand_len[p] clamped into [0, k], and skips every candidate id
 * outside the shard.
 * BOTH forms return only when the placement is complete: the work runs in rounds on the
 * stream and the host decides after each round whether another is needed, so the call
 * synchronizes the stream (as pas_gas_bind does); the _device form only saves the copies.
 * If a HIP call fails, or the round bound sum(row lengths) + 1 trips, after commits began,
 * the call returns PAS_EDEVICE and the GAS snapshot is invalid (later calls: PAS_ENOSNAP)
 * until the next pas_gas_snapshot_set[_device]: no half-committed snapshot stays valid. */
int pas_gas_place(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_pods,
                  int32_t max_containers, int32_t i915_index, const int64_t* req,
                  const uint32_t* req_mask, const int32_t* n_containers, int32_t k, int32_t ld,
                  int32_t node_base, const int32_t* cand_node /*[n_pods][ld]*/,
                  const int32_t* cand_len, int32_t* place_node, int32_t* place_rank,
                  uint32_t* res_out, uint8_t* cards_out, int32_t* n_sel_out,
                  int64_t* counts_out, int32_t* n_placed, int32_t* n_rounds);
int pas_gas_place_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_pods,
                         int32_t max_containers, int32_t i915_index, const int64_t* d_req,
                         const uint32_t* d_req_mask, const int32_t* d_n_containers, int32_t k,
                         int32_t ld, int32_t node_base, const int32_t* d_cand_node,
                         const int32_t* d_cand_len, int32_t* d_place_node,
                         int32_t* d_place_rank, uint32_t* d_res_out, uint8_t* d_cards_out,
                         int32_t* d_n_sel_out, int64_t* d_counts_out, int32_t* n_placed,
                         int32_t* n_rounds, void* hip_stream);

/* Pods leaving nodes: Cache.adjustPodResources(remove) (node_resource_cache.go:240-287) with
 * each pod's annotation, in call order.  Container c of release r has cards_per_container
 * [r][c] cards (its "gas-container-cards" segment), listed in container order in
 * cards[r][8] (at most 8 in all; pas_gas_release_ex: 64) as ranks into the node's cards; request / count is subtracted from each card
 * (subtractRM, resource_map.go:55-73,103-127: clamp at 0; a negative amount, or a card the
 * node's label does not list, is an input error and nothing changes).  The snapshot keeps
 * no "key absent" state: a label card has every kind, so subtracting from a kind that was
 * never added clamps at 0 where the reference reports errInput. */
int pas_gas_release(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_releases,
                    const int32_t* rel_pod, const int32_t* rel_node, int32_t n_pods,
                    int32_t max_containers, const int64_t* req, const uint32_t* req_mask,
                    const int32_t* n_containers, const int32_t* cards_per_container,
                    const int32_t* cards, int32_t* status_out);
/* pas_gas_release with cards[r][PAS_GAS_MAX_SELECTIONS] (annotations of up to 64 cards). */
int pas_gas_release_ex(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_releases,
                       const int32_t* rel_pod, const int32_t* rel_node, int32_t n_pods,
                       int32_t max_containers, const int64_t* req, const uint32_t* req_mask,
                       const int32_t* n_containers, const int32_t* cards_per_container,
                       const int32_t* cards, int32_t* status_out);

/* pas_gas_release with each annotation as counts[r][c][k] (container c lists card k that many
 * times; numCards = the row's sum), for annotations of any length.  Negative counts or a row
 * sum past INT64_MAX: PAS_EINVAL; a count on a card rank >= the node's n_cards: input error
 * (status PAS_GAS_ERR_INPUT), as a card the label does not list. */
int pas_gas_release_counts(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                           int32_t n_releases, const int32_t* rel_pod, const int32_t* rel_node,
                           int32_t n_pods, int32_t max_containers, const int64_t* req,
                           const uint32_t* req_mask, const int32_t* n_containers,
                           const int64_t* counts /*[n_releases][max_containers][max_cards]*/,
                           int32_t* status_out);

/* Pod events: the third way the resident usage changes, and the one that keeps it true when
 * this process is not the only writer.  Cache.handlePod (node_resource_cache.go:493-538)
 * sees a pod that already carries a "gas-container-cards" annotation (bound by another
 * extender replica, by an earlier run, or met in the informer's initial list) and calls
 * adjustPodResources(add) straight from the annotation: no fit, no capacity check, only
 * addRM's checks; a completed pod gets adjustPodResources(remove).  One call applies an
 * ordered batch of such events in place; its large case is the cold-start rebuild (zero
 * usage, then every running pod's annotation as one ADD batch).
 *
 * Event e is (ev_kind[e], pod ev_pod[e], node ev_node[e]); req / req_mask / n_containers
 * describe the pods as for pas_gas_fit.  Its annotation has the layout of
 * pas_gas_release_ex with a row length the caller chooses: container c lists
 * cards_per_container[e][c] cards, stored consecutively in cards[e][0 .. cards_ld), in
 * container order, as ranks into the node's label cards.  A rank that is negative or >= the
 * node's card count names a card the label does not list (a node with n_cards <= 0 lists
 * none).  Events are applied in call order: events on one node see each other in that order,
 * events on different nodes are independent.  status_out[e] is PAS_GAS_OK or the error, and
 * an event that fails changes nothing (all or nothing per event).
 *
 * PAS_GAS_EV_ADD (checkPodResourceAdjustment then adjustPodResources, :190-287; addRM / add,
 * resource_map.go:38-53,77-98; divide, :129-145), for containers c in order with numCards =
 * cards_per_container[e][c] > 0: r[q] = req[p][c][q] / numCards (truncating; numCards counts
 * every listed card, also those outside the label) for the kinds q of the container's mask.
 * For each listed card in list order and each masked kind: r[q] < 0 is PAS_GAS_ERR_INPUT;
 * otherwise, on a label card, used + r[q] < 0 (the sum wraps as Go's does) is
 * PAS_GAS_ERR_OVERFLOW; a card listed several times is added to several times.  The first
 * failing (container, listed card) decides the status.  Within one card the reference's
 * order is Go-map order; here a negative amount is reported before an overflow.  A card
 * outside the label is checked for the negative amount and otherwise skipped: the reference
 * would keep usage for a card no fit ever reads.  PAS_REQ_UNKNOWN_KIND is ignored on ADD: the
 * reference adds a key no capacity map has, and because that key's amount is not carried in
 * the batch, its errInput on a negative value is not reproduced.  There is no capacity
 * check: usage may end above capacity, which every fit treats as "does not fit".
 *
 * PAS_GAS_EV_REMOVE is exactly pas_gas_release_ex on the node's current usage, with rows of
 * cards_ld: clamp at 0; PAS_GAS_ERR_INPUT for a negative amount, a card outside the label,
 * or PAS_REQ_UNKNOWN_KIND on a non-empty segment.
 *
 * gen_from is checked (PAS_ESTALE, nothing changed) and the snapshot moves to gen_to in the
 * call.  The host form validates as pas_gas_release does, PAS_EINVAL for: an event kind
 * outside {0, 1}, a node or pod index out of range, n_containers out of range, mask bits >=
 * n_res, a negative card count, a pod's counts summing past cards_ld, cards_ld < 1.  It
 * uploads, runs the _device form's path (the grouping by node is a device sort in both),
 * waits and copies status_out back; a HIP failure in that last step, after the commit kernel
 * was enqueued, returns PAS_EDEVICE and leaves the GAS snapshot invalid (PAS_ENOSNAP until the
 * next pas_gas_snapshot_set), since the statuses of what ran are lost.
 * The _device form takes device pointers, is asynchronous on hip_stream and moves the
 * generation once the commit kernel is enqueued; it does not wait for the device (its sort
 * storage is per stream and allocated when a larger batch first needs it).  A HIP failure
 * before that launch leaves the snapshot and its generation untouched.  It cannot validate
 * the arrays: an event whose kind, node or pod is out of range gets PAS_GAS_ERR_INPUT and
 * changes nothing, n_containers is read clamped into [0, max_containers], negative card
 * counts read as 0, and an event whose running card offset would pass cards_ld gets
 * PAS_GAS_ERR_INPUT; no array is read or written outside its bounds.  As for every snapshot
 * change, the caller orders the call after readers on other streams. */
#define PAS_GAS_EV_ADD 0    /* podAdded / podUpdated: adjustPodResources(add) */
#define PAS_GAS_EV_REMOVE 1 /* podCompleted / podDeleted: adjustPodResources(remove) */
int pas_gas_apply(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_events,
                  const int32_t* ev_kind, const int32_t* ev_pod, const int32_t* ev_node,
                  int32_t n_pods, int32_t max_containers, const int64_t* req,
                  const uint32_t* req_mask, const int32_t* n_containers,
                  const int32_t* cards_per_container /*[n_events][max_containers]*/,
                  const int32_t* cards /*[n_events][cards_ld]*/, int32_t cards_ld,
                  int32_t* status_out /*[n_events]*/);
int pas_gas_apply_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_events,
                         const int32_t* d_ev_kind, const int32_t* d_ev_pod,
                         const int32_t* d_ev_node, int32_t n_pods, int32_t max_containers,
                         const int64_t* d_req, const uint32_t* d_req_mask,
                         const int32_t* d_n_containers,
                         const int32_t* d_cards_per_container, const int32_t* d_cards,
                         int32_t cards_ld, int32_t* d_status_out, void* hip_stream);

/* Pod events from annotation strings.  Cache.handlePod gets a kind, the pod, the node's name
 * and the pod's "gas-container-cards" annotation (node_resource_cache.go:493-538), and
 * adjustPodResources checks its arguments (errBadArgs, :192-196), splits the annotation
 * (strings.Split on "|" and ",", :241,253-256) and finds every listed card by name in the
 * node's usage map.  The calls below take exactly that: per event the kind, the pod, the node
 * (a slot, or its name) and the annotation's bytes; the device splits the annotation, resolves
 * the card names against the resident card-name table (pas_gas_card_names_set below) and hands
 * the ranks to the walker of pas_gas_apply, which runs unchanged.  Event e's annotation is
 * ann_bytes[ann_off[e] .. ann_off[e + 1]) and, in the _names forms, its node's name
 * node_name_bytes[node_name_off[e] .. node_name_off[e + 1]) (lookup only: the name table of
 * pas_names_set does not change).  Host forms return PAS_EINVAL unless both offset arrays start
 * at 0 and never decrease; _device forms read both ends of every span clamped into [0, n_bytes]
 * and the end not before the begin, and n_containers clamped into [0, max_containers].
 *
 * The grammar (csrc/annotation_fixed.h, one routine for host and device): segments = 1 +
 * count('|'), so the empty annotation is one empty segment, as Go's Split gives; an empty
 * segment lists 0 cards; any other lists 1 + count(',') names, the empty names of "a,,b", "a,"
 * and ",a" included.  Names are opaque bytes (byte 0 and bytes >= 0x80 are ordinary).
 *
 * Per event, in this order:
 *   1. a kind outside {ADD, REMOVE} or a pod outside [0, n_pods): PAS_GAS_ERR_INPUT (the host
 *      forms: PAS_EINVAL for the call, nothing changed);
 *   2. segments != n_containers[pod], or (the _names forms) an empty node name:
 *      PAS_GAS_ERR_BAD_ARGS, the reference's errBadArgs (:192-196); a pod without containers is
 *      therefore always bad args;
 *   3. node -1, or a name without a slot: PAS_GAS_OK and nothing changes (a node the snapshot
 *      does not hold has no usage to adjust); any other slot outside [0, n_nodes):
 *      PAS_GAS_ERR_INPUT (the host forms: PAS_EINVAL for the call);
 *   4. no card listed at all: PAS_GAS_OK and nothing changes;
 *   5. otherwise the event is pending (PAS_GAS_ANN_PENDING in verdict_out of the resolve form):
 *      with L = n_cards[node] clamped into [0, k], every listed name gets the lowest rank r < L
 *      whose name in the node's row of the card-name table has the same length and bytes, else
 *      -1 (the names past L, parked cards, never match), and the event, with its counts and
 *      ranks, is applied exactly as pas_gas_apply applies it: its status is that call's.
 * Events are applied in call order, all or nothing per event, as in pas_gas_apply.
 *
 * PAS_ENOSNAP without a GAS snapshot, a card-name table or (the _names forms) a name table;
 * PAS_EINVAL, the message naming the card-name table, unless that table has n_slots == n_nodes
 * and k == max_cards of the resident snapshot.  gen_from is checked (PAS_ESTALE, nothing
 * changed) and the snapshot moves to gen_to when the call returns PAS_OK, also when no event
 * was pending.  The _device forms synchronize hip_stream once: the largest listed count of the
 * pending events comes back to the host and sizes the rank rows (per-stream workspace; if it
 * cannot be allocated: PAS_ENOMEM, nothing changed), as the refresh from Quantity literals
 * reads its summary back.  They cannot validate the arrays: rules 1 and 3 give the statuses
 * above, and nothing outside the call's arrays, the workspace and the resident arrays is read
 * or written. */
#define PAS_GAS_ERR_BAD_ARGS 4 /* node_resource_cache.go errBadArgs: nothing changes */
#define PAS_GAS_ANN_PENDING (-1) /* verdict_out: rules 1-4 did not settle the event */
int pas_gas_apply_annotations(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_events,
                              const int32_t* ev_kind, const int32_t* ev_pod,
                              const int32_t* ev_node, int32_t n_pods, int32_t max_containers,
                              const int64_t* req, const uint32_t* req_mask,
                              const int32_t* n_containers, const int64_t* ann_off,
                              const char* ann_bytes, int32_t* status_out /*[n_events]*/);
int pas_gas_apply_annotations_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                     int32_t n_events, const int32_t* d_ev_kind,
                                     const int32_t* d_ev_pod, const int32_t* d_ev_node,
                                     int32_t n_pods, int32_t max_containers, const int64_t* d_req,
                                     const uint32_t* d_req_mask, const int32_t* d_n_containers,
                                     int64_t n_ann_bytes, const int64_t* d_ann_off,
                                     const char* d_ann_bytes, int32_t* d_status_out,
                                     void* hip_stream);
int pas_gas_apply_annotations_names(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                    int32_t n_events, const int32_t* ev_kind,
                                    const int32_t* ev_pod, const int64_t* node_name_off,
                                    const char* node_name_bytes, int32_t n_pods,
                                    int32_t max_containers, const int64_t* req,
                                    const uint32_t* req_mask, const int32_t* n_containers,
                                    const int64_t* ann_off, const char* ann_bytes,
                                    int32_t* status_out /*[n_events]*/);
int pas_gas_apply_annotations_names_device(
    pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_events, const int32_t* d_ev_kind,
    const int32_t* d_ev_pod, int64_t n_name_bytes, const int64_t* d_node_name_off,
    const char* d_node_name_bytes, int32_t n_pods, int32_t max_containers, const int64_t* d_req,
    const uint32_t* d_req_mask, const int32_t* d_n_containers, int64_t n_ann_bytes,
    const int64_t* d_ann_off, const char* d_ann_bytes, int32_t* d_status_out, void* hip_stream);

/* The parse alone, as pas_quantities_to_wide is for the refresh: reads the resident n_cards and
 * the card-name table, writes nothing resident and has no kinds (rule 1 is the pod's range).
 * verdict_out [E] is the status rules 1-4 give or PAS_GAS_ANN_PENDING, n_listed_out [E] the
 * full listed count; cards_per_container_out [E][max_containers] holds the counts of the first
 * max_containers segments (0 past the annotation's segments) and cards_out [E][cards_ld] the
 * ranks of the first cards_ld listed cards (-1 past them), for every event: a node outside
 * [0, n_nodes) has no label card, so all its ranks are -1.  cards_ld >= 1.  The _device form is
 * asynchronous on hip_stream. */
int pas_gas_annotations_resolve(pas_ctx* ctx, int32_t n_events, const int32_t* ev_pod,
                                const int32_t* ev_node, int32_t n_pods,
                                const int32_t* n_containers, int32_t max_containers,
                                const int64_t* ann_off, const char* ann_bytes, int32_t cards_ld,
                                int32_t* verdict_out, int32_t* n_listed_out,
                                int32_t* cards_per_container_out, int32_t* cards_out);
int pas_gas_annotations_resolve_device(pas_ctx* ctx, int32_t n_events, const int32_t* d_ev_pod,
                                       const int32_t* d_ev_node, int32_t n_pods,
                                       const int32_t* d_n_containers, int32_t max_containers,
                                       int64_t n_ann_bytes, const int64_t* d_ann_off,
                                       const char* d_ann_bytes, int32_t cards_ld,
                                       int32_t* d_verdict_out, int32_t* d_n_listed_out,
                                       int32_t* d_cards_per_container_out, int32_t* d_cards_out,
                                       void* hip_stream);
/* One annotation on the host, the same routine: *n_segments and *n_listed are always the full
 * counts, cards_per_container [max_containers] is filled for the first max_containers segments
 * and name_span [cap][2] = (begin, length) for the first cap names.  No context; PAS_EINVAL for
 * a negative size or a missing array. */
int pas_gas_annotation_parse(const char* bytes, int64_t len, int32_t max_containers,
                             int64_t* n_segments, int32_t* cards_per_container,
                             int64_t* n_listed, int64_t* name_span /*[cap][2]*/, int64_t cap);

/* Bind annotations rendered from the card-name table: the inverse of the calls above.  bindNode
 * writes a pod's cards as the "gas-container-cards" string, card names joined by "," and the
 * containers' segments by "|" (scheduler.go:317-335, 423-431); a placement answers in slots and
 * counts.  Bind b is on node slot bind_node[b] with n_containers[b] containers and renders to
 * ann_bytes_out[ann_off_out[b] .. ann_off_out[b + 1]), from one of two forms:
 *   counts form   counts [B][max_containers][max_cards] as pas_gas_bind_counts / pas_gas_place
 *                 give it (max_cards is the resident snapshot's): container c lists card k
 *                 counts[c][k] times, in ascending k;
 *   ranks form    cards_per_container [B][max_containers] and cards [B][cards_ld], the containers'
 *                 cards consecutively: the arrays pas_gas_annotations_resolve emits and
 *                 pas_gas_apply takes, so the render is the exact inverse of the resident parser.
 * Card k (rank r) of the bind's node is name (node, k) of the card-name table.
 *
 * The grammar (csrc/annotation_fixed.h, one routine for host and device): n_containers segments
 * joined by '|', so n_containers - 1 bars, and 0 containers render ""; a container without cards
 * is an empty segment; the names of a segment are joined by ','.  Names are opaque bytes: the
 * empty name renders as itself, so "a,,b" can come out, as the parser reads it.  (A segment that
 * lists the empty name once and nothing else renders as no bytes, which the parser, like Go's
 * Split, reads as a segment without cards: the one value whose round trip is not exact.)
 *
 * status_out[b]:
 *   PAS_GAS_OK            the bind renders.  Node -1 (an unplaced pod) is PAS_GAS_OK with an
 *                         empty span, told from a rendered "" by the node;
 *   PAS_GAS_ERR_INPUT     with an empty span: any other node outside [0, n_nodes); a negative
 *                         count; a nonzero count on a card slot at or past L = n_cards[node]
 *                         clamped into [0, max_cards] (a parked or unused slot: a bind never
 *                         selects one); a rank outside [0, L); (ranks form) more listed cards
 *                         than cards_ld; a negative cards_per_container reads as 0;
 *   PAS_GAS_ERR_OVERFLOW  with an empty span: otherwise, a rendered length past INT32_MAX bytes.
 *                         The lengths are summed saturating, so counts up to INT64_MAX are
 *                         ordinary input.
 * Statuses, ann_off_out [B + 1] and *n_bytes_out (the byte total; may be NULL) are always
 * delivered, the bytes only when cap >= the total; else the call returns PAS_ECAPACITY with the
 * size in the message and writes no byte.  cap == 0 with ann_bytes_out NULL is the sizing call.
 *
 * PAS_ENOSNAP without a GAS snapshot or a card-name table; PAS_EINVAL, the message naming the
 * card-name table, unless that table has n_slots == n_nodes and k == max_cards of the resident
 * snapshot (the rule of pas_gas_apply_annotations).  The host forms return PAS_EINVAL unless
 * every n_containers is in [0, max_containers] and every node is -1 or in [0, n_nodes); the
 * _device forms clamp n_containers into that range and report the nodes through status_out.
 * The _device forms synchronize hip_stream once: the byte total comes back to the host, which
 * checks cap before the write pass is enqueued (per-stream workspace; PAS_ENOMEM if it cannot be
 * allocated).  Nothing resident is written and no generation moves.  PAS_ABI_VERSION is
 * unchanged: additions only. */
int pas_gas_annotations_render(pas_ctx* ctx, int32_t n_binds, const int32_t* bind_node,
                               const int32_t* n_containers, int32_t max_containers,
                               const int64_t* counts, int32_t* status_out /*[n_binds]*/,
                               int64_t* ann_off_out /*[n_binds + 1]*/, char* ann_bytes_out,
                               int64_t cap, int64_t* n_bytes_out);
int pas_gas_annotations_render_device(pas_ctx* ctx, int32_t n_binds, const int32_t* d_bind_node,
                                      const int32_t* d_n_containers, int32_t max_containers,
                                      const int64_t* d_counts, int32_t* d_status_out,
                                      int64_t* d_ann_off_out, char* d_ann_bytes_out, int64_t cap,
                                      int64_t* n_bytes_out, void* hip_stream);
int pas_gas_annotations_render_ranks(pas_ctx* ctx, int32_t n_binds, const int32_t* bind_node,
                                     const int32_t* n_containers, int32_t max_containers,
                                     const int32_t* cards_per_container, const int32_t* cards,
                                     int32_t cards_ld, int32_t* status_out /*[n_binds]*/,
                                     int64_t* ann_off_out /*[n_binds + 1]*/, char* ann_bytes_out,
                                     int64_t cap, int64_t* n_bytes_out);
int pas_gas_annotations_render_ranks_device(
    pas_ctx* ctx, int32_t n_binds, const int32_t* d_bind_node, const int32_t* d_n_containers,
    int32_t max_containers, const int32_t* d_cards_per_container, const int32_t* d_cards,
    int32_t cards_ld, int32_t* d_status_out, int64_t* d_ann_off_out, char* d_ann_bytes_out,
    int64_t cap, int64_t* n_bytes_out, void* hip_stream);
/* One annotation on the host, the same routine and the twin of pas_gas_annotation_parse: counts
 * [n_containers][k] over a row of k names, name c = name_bytes[name_off[c] .. name_off[c + 1]),
 * of which the first n_cards (clamped into [0, k]) are label cards.  *status_out and
 * *n_bytes_out are as above; PAS_ECAPACITY (nothing written) when the length exceeds cap.  No
 * context; PAS_EINVAL for a negative size, a missing array or offsets that do not start at 0 or
 * decrease. */
int pas_gas_annotation_render(int32_t n_containers, int32_t k, int32_t n_cards,
                              const int64_t* counts, const int64_t* name_off,
                              const char* name_bytes, int32_t* status_out, char* bytes_out,
                              int64_t cap, int64_t* n_bytes_out);

/* Read back the resident usage used[N][K][Q] and its generation. */
int pas_gas_snapshot_get(pas_ctx* ctx, uint64_t* gen, int64_t* used_out);
/* Read back the resident n_cards [N] and cap_per_gpu [N][Q] and the generation. */
int pas_gas_snapshot_get_nodes(pas_ctx* ctx, uint64_t* gen, int32_t* n_cards_out /*[N]*/,
                               int64_t* cap_out /*[N][Q]*/);
/* Generation and shape of the resident GAS snapshot (PAS_ENOSNAP without one); any output may
 * be NULL. */
int pas_gas_snapshot_info(const pas_ctx* ctx, uint64_t* gen, int32_t* n_nodes,
                          int32_t* max_cards, int32_t* n_res);

/* Node events on the resident GAS snapshot, applied in call order.  The reference fetches the
 * node from the lister on every fit (scheduler.go:282-300), so a changed label or allocatable
 * is seen by the next request, and it keeps the usage by node and card name for ever
 * (node_resource_cache.go:64,259-272,474-491).  Here update u rewrites node slot upd_node[u]:
 *   n_cards[n]  = upd_n_cards[u]   -1 node not in the lister (FetchNode error, :282-288),
 *                                   0 label missing (:290-298), 1..max_cards label cards
 *   cap[n][q]   = upd_cap[u][q]    any int64 (AsInt64(allocatable) / len(label split))
 *   used[n][k]  = old used[n][upd_src[u][k]] for every kind when 0 <= upd_src[u][k] < max_cards,
 *                 zeros otherwise (a card first seen: addEmptyResourceMaps, :269-275)
 * for all k in [0, max_cards): label cards first, in sort.Strings order, then the parked cards
 * (see pas_gas_snapshot_set).  The whole old row is read before any slot is written (upd_src
 * may be any permutation).  Several updates of one node see each other in call order: upd_src
 * of a later one indexes the row the earlier one left.  Updates of different nodes are
 * independent.  status_out[u] = PAS_GAS_OK, or PAS_GAS_ERR_INPUT and that update changes
 * nothing.  gen_from is checked (PAS_ESTALE, nothing changed); the snapshot moves to gen_to.
 *
 * The host form validates, PAS_EINVAL for: a node outside [0, n_nodes), n_cards outside
 * [-1, max_cards], a src >= max_cards, a non-negative src repeated within one row (one card's
 * usage must not be duplicated).  It uploads, runs the _device form's path, waits and copies
 * status_out back; a HIP failure after the kernel was enqueued returns PAS_EDEVICE and leaves
 * the GAS snapshot invalid (PAS_ENOSNAP until the next pas_gas_snapshot_set), as pas_gas_apply.
 * The _device form takes device pointers, is asynchronous on hip_stream and moves the
 * generation once the kernel is enqueued (its sort storage is per stream and allocated when a
 * larger batch first needs it).  It cannot validate the arrays: an update whose node is out of
 * range or whose n_cards is outside [-1, max_cards] gets PAS_GAS_ERR_INPUT and changes nothing;
 * a src outside [0, max_cards) reads as "zero usage"; a repeated src copies twice (a caller
 * bug, but no memory outside the row is touched); nothing outside the resident arrays and the
 * call's arrays is read or written.  The next fit derives its per-snapshot values again.  As
 * for every snapshot change, the caller orders the call after readers on other streams. */
int pas_gas_nodes_update(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_updates,
                         const int32_t* upd_node, const int32_t* upd_n_cards,
                         const int64_t* upd_cap /*[n_updates][n_res]*/,
                         const int32_t* upd_src /*[n_updates][max_cards]*/,
                         int32_t* status_out /*[n_updates]*/);
int pas_gas_nodes_update_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                int32_t n_updates, const int32_t* d_upd_node,
                                const int32_t* d_upd_n_cards, const int64_t* d_upd_cap,
                                const int32_t* d_upd_src, int32_t* d_status_out,
                                void* hip_stream);

/* Node events from label and allocatable strings, parsed and resolved on the device
 * (csrc/gas_node_strings.hip): what the informer hands over goes in as it is, and the row walker
 * of pas_gas_nodes_update and the card-name table (below) do the writing.  Update u names its
 * node by slot (upd_node) or, in the _names forms, by name through the name table; gives its
 * state, the "gpu.intel.com/cards" label label_bytes[label_off[u] .. label_off[u + 1]) and one
 * allocatable literal per resource kind q of the snapshot, cap_bytes[cap_off[u * Q + q] ..
 * cap_off[u * Q + q + 1]).  PAS_ABI_VERSION is unchanged: additions only. */
#define PAS_GAS_NODE_GONE (-1)    /* the node is not in the lister (FetchNode error) */
#define PAS_GAS_NODE_NO_LABEL 0   /* no cards label (errWontFit, scheduler.go:290-298) */
#define PAS_GAS_NODE_LABEL 1      /* the label, the empty string included (one card "") */
/* Per update, in this order:
 * 1. A state outside {-1, 0, 1} or a slot outside [0, n_nodes) is PAS_GAS_ERR_INPUT, nothing
 *    changes.  _names forms: an empty name is PAS_GAS_ERR_INPUT; a name without a slot in the
 *    snapshot is PAS_GAS_ERR_INPUT unless the state is GONE (the caller gives first-seen nodes
 *    their slots with pas_names_assign beforehand), and with GONE it is PAS_GAS_OK and nothing
 *    changes (n_cards_out -1).
 * 2. GONE: n_cards -1, cap 0, the row and its names stay where they are; no literal is read.
 * 3. NO_LABEL: n_cards 0, cap 0, the row and its names stay; no literal is read.
 * 4. LABEL: pieces = 1 + count('.') is gpuCount (scheduler.go:132-148); n_cards is the number of
 *    distinct pieces; cap[q] = AsInt64(literal q) / gpuCount, truncating toward zero
 *    (resource_map.go:129-145).  An empty literal span is a resource the node does not have: 0.
 *    A literal ParseQuantity rejects makes the update PAS_GAS_ERR_INPUT, nothing changes.
 * 5. The new row of a LABEL update: the label cards in sort.Strings order (bytewise; a name
 *    before any name it is a prefix of), then the parked cards: the old row's slots, in old slot
 *    order, whose name the label does not list, the first max_cards - n_cards of them; the rest
 *    are dropped and counted in n_dropped_out.  An empty name outside the old label range
 *    [0, max(n_cards_old, 0)) is an unused slot: never parked, never counted.  A label card takes
 *    the usage of the lowest old slot whose name has the same length and bytes (unused slots
 *    included: their usage is zero), else zero usage (src -1).
 * 6. Several updates of one node see each other in call order, as in pas_gas_nodes_update: the
 *    resolve-and-apply steps run once per position in the longest run of one node (one round for
 *    a batch without a repeated node; every further round synchronizes once more).
 * Before anything resident is written the call synchronizes hip_stream once and reads back the
 * largest distinct count, the new rows' byte totals and the longest run.  A distinct count above
 * max_cards: PAS_ECAPACITY, nothing changed, the snapshot stays at gen_from; the caller grows the
 * snapshot and the card-name table by a tier and calls again.  *need_cards (host memory in every
 * form, may be NULL) is the largest distinct count of the call's pending updates, at most
 * PAS_GAS_MAX_CARDS + 1.  The new rows' names are appended to the card-name table's pool on the
 * device and the pool is gathered by the rule of pas_gas_card_names_update.
 * Outputs: status_out [U]; n_cards_out [U], cap_out [U][Q] and n_dropped_out [U] may be NULL
 * (n_cards 0 and cap 0 for a PAS_GAS_ERR_INPUT update).
 * Errors: gen_from is checked and the snapshot moves to gen_to exactly as in
 * pas_gas_nodes_update.  PAS_ENOSNAP without a snapshot, a card-name table or (_names) a name
 * table; PAS_EINVAL unless the card-name table's shape equals the snapshot's.  The host forms
 * return PAS_EINVAL unless every offset array starts at 0 and never decreases, and for a slot or
 * a state out of range.  The _device forms check nothing of the offsets: both ends of every
 * span are read clamped into its blob and the end not before the begin, so nothing outside the
 * call's arrays, the workspace and the resident arrays is read or written.  A HIP failure after
 * the first write leaves the snapshot and the card-name table invalid.  As for every snapshot
 * change, the caller orders the call after readers on other streams. */
int pas_gas_nodes_update_strings(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                 int32_t n_updates, const int32_t* upd_node,
                                 const int32_t* upd_state, const int64_t* label_off,
                                 const char* label_bytes, const int64_t* cap_off /*[U*Q+1]*/,
                                 const char* cap_bytes, int32_t* status_out, int32_t* n_cards_out,
                                 int64_t* cap_out /*[U][Q]*/, int32_t* n_dropped_out,
                                 int32_t* need_cards);
int pas_gas_nodes_update_strings_device(
    pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_updates,
    const int32_t* d_upd_node, const int32_t* d_upd_state, int64_t n_label_bytes,
    const int64_t* d_label_off, const char* d_label_bytes, int64_t n_cap_bytes,
    const int64_t* d_cap_off, const char* d_cap_bytes, int32_t* d_status_out,
    int32_t* d_n_cards_out, int64_t* d_cap_out, int32_t* d_n_dropped_out, int32_t* need_cards,
    void* hip_stream);
int pas_gas_nodes_update_strings_names(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                       int32_t n_updates, const int64_t* node_name_off,
                                       const char* node_name_bytes, const int32_t* upd_state,
                                       const int64_t* label_off, const char* label_bytes,
                                       const int64_t* cap_off, const char* cap_bytes,
                                       int32_t* status_out, int32_t* n_cards_out,
                                       int64_t* cap_out, int32_t* n_dropped_out,
                                       int32_t* need_cards);
int pas_gas_nodes_update_strings_names_device(
    pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_updates, int64_t n_name_bytes,
    const int64_t* d_node_name_off, const char* d_node_name_bytes, const int32_t* d_upd_state,
    int64_t n_label_bytes, const int64_t* d_label_off, const char* d_label_bytes,
    int64_t n_cap_bytes, const int64_t* d_cap_off, const char* d_cap_bytes,
    int32_t* d_status_out, int32_t* d_n_cards_out, int64_t* d_cap_out, int32_t* d_n_dropped_out,
    int32_t* need_cards, void* hip_stream);
/* The parse and the resolve alone: every update against the resident row (no chaining), nothing
 * resident is written and no generation is checked.  gpu_count_out [U] is the number of pieces
 * (0 unless LABEL), src_out [U][max_cards] the slot map pas_gas_nodes_update would take
 * (identity for GONE and NO_LABEL; all -1 for a settled update and for a distinct count above
 * max_cards, which n_cards_out reports, capped at PAS_GAS_MAX_CARDS + 1).  Every output except
 * status_out may be NULL.  The _device form is asynchronous on hip_stream. */
int pas_gas_nodes_resolve_strings(pas_ctx* ctx, int32_t n_updates, const int32_t* upd_node,
                                  const int32_t* upd_state, const int64_t* label_off,
                                  const char* label_bytes, const int64_t* cap_off,
                                  const char* cap_bytes, int32_t* status_out,
                                  int32_t* n_cards_out, int32_t* gpu_count_out, int64_t* cap_out,
                                  int32_t* src_out /*[U][max_cards]*/, int32_t* n_dropped_out);
int pas_gas_nodes_resolve_strings_device(
    pas_ctx* ctx, int32_t n_updates, const int32_t* d_upd_node, const int32_t* d_upd_state,
    int64_t n_label_bytes, const int64_t* d_label_off, const char* d_label_bytes,
    int64_t n_cap_bytes, const int64_t* d_cap_off, const char* d_cap_bytes,
    int32_t* d_status_out, int32_t* d_n_cards_out, int32_t* d_gpu_count_out, int64_t* d_cap_out,
    int32_t* d_src_out, int32_t* d_n_dropped_out, void* hip_stream);
/* One cards label on the host, the same routines (csrc/label_fixed.h): *n_pieces = 1 +
 * count('.'), *n_cards = the distinct pieces, counted up to PAS_GAS_MAX_CARDS + 1 (a label costs
 * time linear in its bytes per card counted), and name_span [cap][2] = (begin, length) of the
 * first cap cards in rank order.  No context; PAS_EINVAL for a negative size or a missing
 * array. */
int pas_gas_label_parse(const char* bytes, int64_t len, int64_t* n_pieces, int32_t* n_cards,
                        int64_t* name_span /*[cap][2]*/, int64_t cap);

/* Grow the resident snapshot in place: n_nodes_new >= n_nodes and max_cards_new >= max_cards,
 * PAS_EINVAL for a smaller value (PAS_ECAPACITY past PAS_GAS_MAX_CARDS).  Content is kept (the
 * rows are re-pitched on the device, no host copy); new node slots have n_cards -1, cap 0 and
 * usage 0; new card slots are zero.  gen_from is checked (PAS_ESTALE) and the snapshot moves
 * to gen_to.  Synchronous on hip_stream: the old storage is freed after the copy kernel has
 * finished.  When the new storage cannot be allocated the old snapshot stays valid and
 * untouched (PAS_ENOMEM).  pas_tas_gas_topk*_device still needs both snapshots to hold the
 * same number of nodes: a caller that grows the GAS snapshot grows its TAS snapshot to the
 * same number of slots with pas_tas_snapshot_reshape (spare slots: no present bit). */
int pas_gas_snapshot_resize(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                            int32_t n_nodes_new, int32_t max_cards_new, void* hip_stream);
/* Renumber the node slots of the resident snapshot on the device, with the arguments and the
 * src_node contract of pas_tas_snapshot_compact: new row j takes n_cards, cap [n_res] and used
 * [max_cards][n_res] of old row src_node[j], or, for -1, n_cards -1, cap 0 and usage 0; a row no
 * entry names is gone with its usage.  The reference keeps usage by node and card name and
 * never deletes it (nodeStatuses, node_resource_cache.go:64,259-272): a caller that wants that
 * keeps the rows that still hold usage.  max_cards is unchanged.  One gather kernel into new
 * storage; generation, errors and the freeing of the old storage as in
 * pas_gas_snapshot_resize, and the fit's derived values are computed again by the next fit.
 * pas_tas_gas_topk*_device still needs equal node counts: a caller compacts both snapshots with
 * the same src_node. */
int pas_gas_snapshot_compact(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                             int32_t n_nodes_new, const int32_t* src_node /* host [n_nodes_new] */,
                             void* hip_stream);

/* ------------------------------------------------------------------------- */
/* Node-sharded snapshots                                  */
/* ------------------------------------------------------------------------- */

/* A GPU holding nodes [node_base, node_base + n_nodes) of the cluster as its resident
 * TAS snapshot evaluates every pod's filter + prioritize over that shard and keeps the
 * first k entries of the shard's HostPriorityList (as pas_tas_eval_device with both flags
 * would list them) as merge records:
 *   top_node [n_pods][k]  global node index (node_base + shard index); INT32_MAX past len
 *   top_key  [n_pods][k]  order key: ~value for GreaterThan, value for LessThan, 0 for any
 *                         other operator (value = the node's v_milli of the prioritize
 *                         metric); INT64_MAX past len
 *   top_len  [n_pods]     min(k, entries)
 * Ascending (key, node) is the HostPriorityList order, so the merge of all shards' records
 * (pas_topk_merge_device) is exactly the first k entries over the whole cluster. */
int pas_tas_topk_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t n_rules,
                        const pas_rule* d_rules, const int32_t* d_rule_off,
                        const pas_rule* d_prio, const uint64_t* d_cand, int32_t k,
                        int32_t node_base, int64_t* d_top_key, int32_t* d_top_node,
                        int32_t* d_top_len, void* hip_stream);

/* Full-list prioritize over node shards: the cluster's whole
 * HostPriorityList per pod from every shard's whole list.  keys / nodes [n_shards][n_pods]
 * [width] are the shards' records as pas_tas_topk_device writes them with k = width (>= the
 * widest shard; INT64_MAX / INT32_MAX past each list).  out_node[p][0 .. out_len[p]) = the
 * merged list (ascending (key, node): the order prioritizeNodesForRule lists,
 * telemetryscheduler.go:128-149), global node ids, -1 in positions
 * [out_len[p], n_shards * width); row pitch out_ld >= n_shards * width.  Exact: no
 * (key, node) pair repeats across shards. */
int pas_list_merge_device(pas_ctx* ctx, int32_t n_pods, int32_t n_shards, int32_t width,
                          const int64_t* d_keys, const int32_t* d_nodes, int32_t* d_out_node,
                          int64_t out_ld, int32_t* d_out_len, void* hip_stream);

/* The same records for the combined TAS + GAS filter (BASELINE configs[4]): the first k
 * entries of the shard's HostPriorityList over the nodes that pass the pod's dontschedule
 * filter (and d_cand when given) AND fit its GPU request (runSchedulingLogic on the
 * context's resident GAS snapshot of the same nodes, gpuscheduler/scheduler.go:280-338).
 * Equal to pas_gas_fit_bitmap_device over the shard followed by pas_tas_topk_device with
 * the fit bitmaps (intersected with d_cand) as candidates, but evaluated along each pod's
 * order: a node is filtered and fitted only until k nodes are kept, so a pod costs about
 * k / (pass rate) node evaluations instead of the shard's n_nodes.  The GAS arguments are
 * those of pas_gas_fit_device (any number of selections).  The two snapshots must hold the
 * same number of nodes (PAS_EINVAL otherwise). */
int pas_tas_gas_topk_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen, int32_t n_pods,
                            int32_t n_rules, const pas_rule* d_rules, const int32_t* d_rule_off,
                            const pas_rule* d_prio, const uint64_t* d_cand,
                            int32_t max_containers, int32_t i915_index, const int64_t* d_req,
                            const uint32_t* d_req_mask, const int32_t* d_n_containers,
                            int32_t k, int32_t node_base, int64_t* d_top_key,
                            int32_t* d_top_node, int32_t* d_top_len, void* hip_stream);

/* Merge of n_shards record sets laid out [n_shards][n_pods][k] (the layout of an
 * all-gather of the per-shard top_key / top_node): out_node[n_pods][k] = the k smallest
 * (key, node) records' nodes in order (-1 past out_len), out_len = min(k, records). */
int pas_topk_merge_device(pas_ctx* ctx, int32_t n_pods, int32_t k, int32_t n_shards,
                          const int64_t* d_keys, const int32_t* d_nodes, int32_t* d_out_node,
                          int32_t* d_out_len, void* hip_stream);

/* Wide merge records: the same node-sharded top-k, exact on snapshots that hold wide columns
 * (pas_tas_snapshot_update_wide) and across shards that hold one metric in different forms.
 * A wide record is (key int64, sub uint32, node int32) in three arrays:
 *   top_key [n_pods][k], top_sub [n_pods][k], top_node [n_pods][k], top_len [n_pods]
 * Every record is in one canonical unit, whatever form the shard holds the prioritize column
 * in.  The value of node n on metric m as the pair (W, F), value = W + F * 10^-9:
 *   wide column    W = whole[m][n], F = nano[m][n]
 *   narrow column  with multiplier 10^s (pas_tas_snapshot_set_scale, s = 0..9; milli: s = 3)
 *                  and v the stored integer: W = floor(v / 10^s) toward -infinity,
 *                  F = (v - W * 10^s) * 10^(9-s), so 0 <= F < 10^9 (-1500 at scale 3 is
 *                  (-2, 500000000)); exact in 64-bit arithmetic
 * Keys:
 *   LessThan        key = W,  sub = F
 *   GreaterThan     key = ~W, sub = ~F (32-bit complement)
 *   other operator  key = 0,  sub = 0
 *   past top_len    key = INT64_MAX, sub = UINT32_MAX, node = INT32_MAX
 * Ascending (key signed, sub unsigned, node) is the HostPriorityList order: the pair order is
 * the exact value order and ~ reverses both fields without overflow.  Because the unit is
 * canonical, shards may hold the same metric narrow at different scales or wide and the
 * merge is still exact (the 64-bit records of pas_tas_topk_device promise that only for one
 * narrow scale on every shard).  The wide entry points work on any snapshot, one without a
 * wide column included; ranks of one merge group must all use the same record form. */

/* pas_tas_topk_device with wide records: the same lists (top_node, top_len), keyed in the
 * canonical unit; d_top_sub [n_pods][k].  Never PAS_ENOTEXACT for a wide column. */
int pas_tas_topk_wide_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods, int32_t n_rules,
                             const pas_rule* d_rules, const int32_t* d_rule_off,
                             const pas_rule* d_prio, const uint64_t* d_cand, int32_t k,
                             int32_t node_base, int64_t* d_top_key, uint32_t* d_top_sub,
                             int32_t* d_top_node, int32_t* d_top_len, void* hip_stream);

/* pas_tas_gas_topk_device with wide records: dontschedule rules on wide columns are compared
 * exactly (the target as it is against the pair), evaluated along each pod's order as there.
 * Equal to pas_gas_fit_bitmap_device followed by pas_tas_topk_wide_device. */
int pas_tas_gas_topk_wide_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                 int32_t n_pods, int32_t n_rules, const pas_rule* d_rules,
                                 const int32_t* d_rule_off, const pas_rule* d_prio,
                                 const uint64_t* d_cand, int32_t max_containers,
                                 int32_t i915_index, const int64_t* d_req,
                                 const uint32_t* d_req_mask, const int32_t* d_n_containers,
                                 int32_t k, int32_t node_base, int64_t* d_top_key,
                                 uint32_t* d_top_sub, int32_t* d_top_node, int32_t* d_top_len,
                                 void* hip_stream);

/* Resuming a top-k list.  d_after_key / [d_after_sub /] d_after_node are [n_pods] contiguous
 * device arrays holding one cursor per pod in the record form the call writes (64-bit records
 * for pas_tas_gas_topk_after_device, the canonical (key, sub, node) unit for the wide form;
 * node ids are global).
 * Definition: the result for pod p is what the entry point without _after would give on the
 * same snapshots and arguments with k unbounded, minus every record that is not strictly after
 * the pod's cursor, cut at k.  "After" is in the ascending (key[, sub], node) order above, the
 * list order.  Nothing else about the cursor matters: it need not be a record of the list, its
 * node need not be in this shard (every shard resumes after the same global cursor, and the
 * merge of the shards' pages is the cluster's page), and the snapshots may have changed since
 * it was produced.  The device cannot validate the cursor arrays and does not need to: every
 * bit pattern has a defined result.  On a pod whose prioritize operator is neither LessThan
 * nor GreaterThan every record has key 0 (sub 0), so a cursor key below that gives the whole
 * list and one above it the empty list.
 *   begin   (INT64_MIN, [0,] -1) gives the whole list: equal to the call without _after.
 *   end     the padding record (INT64_MAX, [UINT32_MAX,] INT32_MAX) gives the empty list
 *           (top_len 0, padding only).  So top_key[p][k-1], [top_sub[p][k-1],] top_node[p][k-1]
 *           of one call is the cursor of the next, and a pod whose list was shorter than k is
 *           finished by construction.
 * The position after the cursor is found by binary search in the pod's order row (the value's
 * tie run, then the node within it), so a page costs what its own records cost, whatever came
 * before it.  The checks are those of the entry points without _after, and null cursor arrays
 * are PAS_EINVAL; the 64-bit form returns PAS_ENOTEXACT on a snapshot with wide columns. */
int pas_tas_gas_topk_after_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                  int32_t n_pods, int32_t n_rules, const pas_rule* d_rules,
                                  const int32_t* d_rule_off, const pas_rule* d_prio,
                                  const uint64_t* d_cand, int32_t max_containers,
                                  int32_t i915_index, const int64_t* d_req,
                                  const uint32_t* d_req_mask, const int32_t* d_n_containers,
                                  int32_t k, int32_t node_base, const int64_t* d_after_key,
                                  const int32_t* d_after_node, int64_t* d_top_key,
                                  int32_t* d_top_node, int32_t* d_top_len, void* hip_stream);
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
                                       void* hip_stream);

/* The top-k entry points by policy id, over the resident policy table (pas_tas_policies_set):
 * each gives exactly the outputs of its counterpart without _policies (top_key, [top_sub,]
 * top_node, top_len, the padding records included) called with pod p's rules and prio being
 * table row d_pod_policy[p].  d_pod_policy is [n_pods] on the device; an id outside
 * [0, n_policies) is read as -1: no dontschedule rules and no prio rule, i.e. the empty list
 * (top_len 0, padding only).  A table with n_policies = 0 is valid: every id is then -1.  No
 * access leaves its array, whatever the ids are.  Unknown operators are skipped, as in the
 * device forms of the counterparts.
 * A node's dontschedule verdict is one bit of the policy's cached violating set (viol
 * [n_policies][W64], above), built by the first policy verb after the snapshot's content or
 * the table changed, on that verb's stream, and ordered before calls on other streams by an
 * event: the rules are not evaluated per pod, and a round of placement on an unchanged TAS
 * snapshot costs no rule evaluation at all.  These calls neither build nor read the node-major
 * snapshot copies the rules forms keep (8 bytes per node and metric).
 * Checks: those of the counterpart (generations, k >= 1, node_base >= 0, node_base + n_nodes
 * within int32, equal node counts of the TAS and GAS snapshots, null arguments: PAS_EINVAL;
 * the 64-bit forms PAS_ENOTEXACT on a snapshot with wide columns) and those of the policy
 * verbs (PAS_EINVAL without a table; PAS_ESTALE, the message naming the policy table, when the
 * table was set before a call that renumbered columns).  Null d_pod_policy with n_pods > 0 is
 * PAS_EINVAL; n_pods = 0 returns PAS_OK.  The _after forms resume as their counterparts
 * ("Resuming a top-k list"); the TAS-only forms walk the pods' orders as the TAS + GAS forms
 * do, without the fit. */
int pas_tas_topk_policies_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods,
                                 const int32_t* d_pod_policy, const uint64_t* d_cand, int32_t k,
                                 int32_t node_base, int64_t* d_top_key, int32_t* d_top_node,
                                 int32_t* d_top_len, void* hip_stream);
int pas_tas_topk_policies_wide_device(pas_ctx* ctx, uint64_t gen, int32_t n_pods,
                                      const int32_t* d_pod_policy, const uint64_t* d_cand,
                                      int32_t k, int32_t node_base, int64_t* d_top_key,
                                      uint32_t* d_top_sub, int32_t* d_top_node,
                                      int32_t* d_top_len, void* hip_stream);
int pas_tas_gas_topk_policies_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                     int32_t n_pods, const int32_t* d_pod_policy,
                                     const uint64_t* d_cand, int32_t max_containers,
                                     int32_t i915_index, const int64_t* d_req,
                                     const uint32_t* d_req_mask, const int32_t* d_n_containers,
                                     int32_t k, int32_t node_base, int64_t* d_top_key,
                                     int32_t* d_top_node, int32_t* d_top_len, void* hip_stream);
int pas_tas_gas_topk_policies_wide_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                          int32_t n_pods, const int32_t* d_pod_policy,
                                          const uint64_t* d_cand, int32_t max_containers,
                                          int32_t i915_index, const int64_t* d_req,
                                          const uint32_t* d_req_mask,
                                          const int32_t* d_n_containers, int32_t k,
                                          int32_t node_base, int64_t* d_top_key,
                                          uint32_t* d_top_sub, int32_t* d_top_node,
                                          int32_t* d_top_len, void* hip_stream);
int pas_tas_gas_topk_policies_after_device(pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen,
                                           int32_t n_pods, const int32_t* d_pod_policy,
                                           const uint64_t* d_cand, int32_t max_containers,
                                           int32_t i915_index, const int64_t* d_req,
                                           const uint32_t* d_req_mask,
                                           const int32_t* d_n_containers, int32_t k,
                                           int32_t node_base, const int64_t* d_after_key,
                                           const int32_t* d_after_node, int64_t* d_top_key,
                                           int32_t* d_top_node, int32_t* d_top_len,
                                           void* hip_stream);
int pas_tas_gas_topk_policies_wide_after_device(
    pas_ctx* ctx, uint64_t tas_gen, uint64_t gas_gen, int32_t n_pods,
    const int32_t* d_pod_policy, const uint64_t* d_cand, int32_t max_containers,
    int32_t i915_index, const int64_t* d_req, const uint32_t* d_req_mask,
    const int32_t* d_n_containers, int32_t k, int32_t node_base, const int64_t* d_after_key,
    const uint32_t* d_after_sub, const int32_t* d_after_node, int64_t* d_top_key,
    uint32_t* d_top_sub, int32_t* d_top_node, int32_t* d_top_len, void* hip_stream);

/* pas_topk_merge_device over wide records: keys / subs / nodes [n_shards][n_pods][k], the k
 * smallest (key, sub, node) records' nodes in order.  PAS_ECAPACITY when n_shards * k > 4096
 * (16 bytes of LDS per record). */
int pas_topk_merge_wide_device(pas_ctx* ctx, int32_t n_pods, int32_t k, int32_t n_shards,
                               const int64_t* d_keys, const uint32_t* d_subs,
                               const int32_t* d_nodes, int32_t* d_out_node, int32_t* d_out_len,
                               void* hip_stream);

/* pas_list_merge_device over wide records (pas_tas_topk_wide_device with k = width): keys /
 * subs / nodes [n_shards][n_pods][width], merged by ascending (key, sub, node); the output
 * is node ids only, as there. */
int pas_list_merge_wide_device(pas_ctx* ctx, int32_t n_pods, int32_t n_shards, int32_t width,
                               const int64_t* d_keys, const uint32_t* d_subs,
                               const int32_t* d_nodes, int32_t* d_out_node, int64_t out_ld,
                               int32_t* d_out_len, void* hip_stream);

/* ------------------------------------------------------------------------- */
/* Wire encoders, host only                                */
/* ------------------------------------------------------------------------- */

/* Response bodies exactly as the reference's handlers write them with
 * json.NewEncoder(w).Encode (encoding/json of Go 1.16, HTML-safe escaping, trailing "\n").
 * Each writes at most cap bytes (no terminator), sets *out_len to the full length, and
 * returns PAS_ECAPACITY when it exceeds cap.  names[i] / node_json[i] are indexed by
 * snapshot node id.
 *
 * HostPriorityList of one pod (WritePrioritizeResponse, telemetryscheduler.go:152-158):
 * order[0 .. len) from pas_tas_eval's order_out row -> [{"Host":..,"Score":10-i},...]. */
int pas_encode_host_priority_list(int32_t len, const int32_t* order, const char* const* names,
                                  char* buf, int64_t cap, int64_t* out_len);

/* TAS FilterResult of one pod (filterNodes + WriteFilterResponse, telemetryscheduler.go:
 * 184-225, 238-244): the request's nodes req_node[0 .. n_req) in request order, the pod's
 * pass_out row; node_json[i] (node_json_len[i] bytes) = the JSON of node i as the Go shim
 * encodes a v1.Node (spliced into "items").  The nil results (no policy label, policy not
 * cached, no dontschedule rules, no nodes: :189-203) are the body "null\n", written by
 * the shim. */
int pas_encode_tas_filter_result(int32_t n_req, const int32_t* req_node, const uint64_t* pass,
                                 const char* const* names, const char* const* node_json,
                                 const int64_t* node_json_len, char* buf, int64_t cap,
                                 int64_t* out_len);

/* GAS FilterResult of one pod (GASExtender.filterNodes, gpuscheduler/scheduler.go:449-482):
 * request node names in order, fit = the pod's row of pas_gas_fit_bitmap_device (or bit 31
 * of the pas_gas_fit words, packed); n_req == 0 gives the reference's error result. */
int pas_encode_gas_filter_result(int32_t n_req, const int32_t* req_node, const uint64_t* fit,
                                 const char* const* names, char* buf, int64_t cap,
                                 int64_t* out_len);

/* BindingResult of GASExtender.bindNode (scheduler.go:385-445): {"Error":"<error>"}; NULL or
 * "" for success. */
int pas_encode_binding_result(const char* error, char* buf, int64_t cap, int64_t* out_len);

/* ------------------------------------------------------------------------- */
/* Wire decoding, host only                                */
/* ------------------------------------------------------------------------- */

/* Snapshot node names -> node ids (the numbering of the TAS / GAS snapshots), built once per
 * snapshot; a repeated name keeps its first id.  Lookup of len bytes: id or -1. */
typedef struct pas_name_table pas_name_table;
int pas_name_table_create(int32_t n_names, const char* const* names, pas_name_table** out);
void pas_name_table_destroy(pas_name_table* table);
int32_t pas_name_table_lookup(const pas_name_table* table, const char* name, int64_t len);

#define PAS_ARGS_NODES 0      /* args.Nodes.Items[].Name: TAS (NodeCacheCapable false) */
#define PAS_ARGS_NODE_NAMES 1 /* *args.NodeNames: GAS (NodeCacheCapable true) */
typedef struct pas_args_info {
  int32_t has_nodes;      /* args.Nodes != nil (TAS: "no nodes in list" otherwise, :74-76) */
  int32_t has_node_names; /* args.NodeNames != nil */
  int32_t n_req;          /* request nodes of the chosen list, in request order */
  int32_t n_unknown;      /* of them not in the table (req_node -1) */
  int64_t pod_off;        /* byte span of the Pod object in the body; pod_len 0: absent / null */
  int64_t pod_len;
} pas_args_info;

/* extender.Args (extender/types.go:36-46) as json.NewDecoder(body).Decode(&args) fills it
 * (telemetryscheduler.go:63-78; gpuscheduler/scheduler.go:486-505), reduced to what the
 * handlers read: the request's node list `which` resolved through the name table into
 * req_node[0 .. n_req) (request order, -1 for a node not in the table), the candidate bitmap
 * cand[W64(table size)] of the known ones (may be NULL), and for PAS_ARGS_NODES the byte span
 * (offset, length) of each item in item_span[n_req][2] (may be NULL).  PAS_EDECODE for what
 * the reference's decode rejects (empty body, syntax, a wrong JSON type on the fields read);
 * PAS_ECAPACITY (info filled) when n_req > node_cap.  Matching of keys, null handling and
 * repeated keys follow encoding/json of Go 1.16 (csrc/wire_decode.cpp). */
int pas_decode_args(const pas_name_table* table, const char* body, int64_t len, int32_t which,
                    int32_t* req_node, int64_t node_cap, int64_t* item_span, uint64_t* cand,
                    pas_args_info* info);

/* The request node names themselves (unescaped, request order), for nodes the table does not
 * know (their FailedNodes / NodeNames entries): name i is buf[offsets[i] .. offsets[i+1]).
 * PAS_ECAPACITY (*total_len, *n_req set) when buf or offsets[n_req + 1] is too small. */
int pas_decode_request_names(const char* body, int64_t len, int32_t which, char* buf,
                             int64_t cap, int64_t* offsets, int64_t offsets_cap,
                             int64_t* total_len, int32_t* n_req);

/* getPolicyFromPod's reads of a v1.Pod JSON (telemetryscheduler.go:103-112): the namespace
 * (*ns_len bytes) and the value of labels[label] (*label_len bytes, -1 if the key is absent).
 * PAS_ECAPACITY (lengths set) when a buffer is too small; PAS_EDECODE as pas_decode_args. */
int pas_decode_pod_policy(const char* pod, int64_t len, const char* label, char* ns_buf,
                          int64_t ns_cap, int64_t* ns_len, char* label_buf, int64_t label_cap,
                          int64_t* label_len);

/* Host threads pas_decode_args may use for one large body: the structural index and the
 * items of a NodeList are split over them (about one per MB of body; results identical to
 * one thread).  n = 0: automatic (up to 16, the GPU box's CPU share per GPU); process-wide.
 * pas_decode_threads: the count a body of that size gets. */
int pas_decode_set_threads(int32_t n);
int32_t pas_decode_threads(int64_t body_len);

/* containerRequests of a v1.Pod JSON (gpuscheduler/utils.go:14-32): per container, the
 * requests named gpu.intel.com/... as AsInt64 values (ok ignored), in the pas_gas_fit layout
 * req[max_containers][n_kinds] / req_mask[max_containers] for kinds[0 .. n_kinds), and
 * *n_containers = len(spec.containers).  gpu.intel.com requests of other kinds are counted
 * in *n_unknown, and such a container's req_mask carries PAS_REQ_UNKNOWN_KIND (with
 * numI915 > 0 it fits no node: capacity lacks the key, scheduler.go:349-354).  n_kinds <= 31.  A quantity ParseQuantity rejects is PAS_EDECODE
 * (Quantity.UnmarshalJSON); PAS_ECAPACITY when n_containers > max_containers.  With
 * n_kinds 0 (req may be NULL) it only validates the quantities, as the TAS decode does. */
int pas_decode_pod_requests(const char* pod, int64_t len, int32_t n_kinds,
                            const char* const* kinds, int32_t max_containers, int64_t* req,
                            uint32_t* req_mask, int32_t* n_containers, int32_t* n_unknown);

/* ------------------------------------------------------------------------- */
/* Resident node-name table: names resolved to slots on the device           */
/* ------------------------------------------------------------------------- */

/* The reference keys everything by node name (NodeMetricsInfo map[string]NodeMetric,
 * metrics/client.go:25-32; args.NodeNames, gpuscheduler/scheduler.go:455-470); node slots exist
 * only here.  The context holds one table from names to slots for all its snapshots (combined
 * contexts share one slot numbering): n_slots slots, each holding one name or spare.  Names are
 * opaque byte strings of any length, bytes >= 0x80 and a byte 0 inside included; the empty name
 * marks a spare slot and so never has a slot itself.  A batch of names is a CSR like a batch of
 * literals: name i is bytes[name_off[i] .. name_off[i + 1]); host forms return PAS_EINVAL
 * unless name_off starts at 0 and never decreases, _device forms read both ends of every span
 * clamped into [0, n_bytes] and the end not before the begin, as pas_quantities_to_wide_device
 * does.  Every entry point answers PAS_ENOSNAP without a table.  Storage only grows and is
 * freed with the context.  PAS_ABI_VERSION is unchanged: additions only.
 *
 * The one hash of names, on the host and on the device (csrc/name_hash.h): the low bits select
 * the home bucket of the table (a power of two >= 2 * n_slots buckets, at least 2, linear
 * probing with wraparound), the high 32 bits are the tag stored beside the slot.  A hit is
 * decided only by comparing all bytes, never by hash bits. */
uint64_t pas_name_hash(const char* bytes, int64_t len);

/* Install the table: slot s holds bytes[name_off[s] .. name_off[s + 1]), an empty span is a
 * spare slot.  Host arrays, synchronous on the context's stream; the hash is built on the
 * device.  A name in two slots is PAS_EINVAL, the message naming the lowest slot whose name
 * also stands in a lower slot; after any error the previous table, if any, is still valid. */
int pas_names_set(pas_ctx* ctx, int32_t n_slots, const int64_t* name_off, const char* bytes);
/* Slots, named slots and the bytes of all names (each output may be NULL). */
int pas_names_info(const pas_ctx* ctx, int32_t* n_slots, int32_t* n_named, int64_t* n_bytes);
/* The names packed in slot order, whatever the table's internal order: name_off_out
 * [n_slots + 1] always, bytes_out [cap] when cap >= n_bytes, else PAS_ECAPACITY (the size
 * needed is name_off_out[n_slots], and in the message). */
int pas_names_get(pas_ctx* ctx, int64_t* name_off_out, char* bytes_out, int64_t cap);
int pas_names_drop(pas_ctx* ctx);

/* slot_out[i] = the slot of name i, or -1 (an empty name: -1).  Reads the table only; n = 0 is
 * valid.  The _device form is asynchronous on hip_stream; on a stream other than that of the
 * last table change it waits for that change's event, not for the host. */
int pas_names_resolve(pas_ctx* ctx, int64_t n, const int64_t* name_off, const char* bytes,
                      int32_t* slot_out);
int pas_names_resolve_device(pas_ctx* ctx, int64_t n, int64_t n_bytes, const int64_t* d_name_off,
                             const char* d_bytes, int32_t* d_slot_out, void* hip_stream);

/* The other direction, for a Binding's target: entry i is the name of slot slot[i] - slot_base,
 * off_out [n + 1] and the bytes (n <= INT32_MAX).  A spare slot and a slot outside the table, -1
 * included, render as an empty span, so the place_node of pas_gas_place goes in unchanged with
 * its node_base; a slot may repeat.  off_out and *n_bytes_out (may be NULL) are always delivered,
 * the bytes only when cap >= the total, else PAS_ECAPACITY with the size in the message; cap == 0
 * with bytes_out NULL is the sizing call.  It is the scan and gather of
 * pas_gas_annotations_render with one name per span.  Reads the table only; the _device form
 * synchronizes hip_stream once (the byte total) and waits for the last table change like
 * pas_names_resolve_device. */
int pas_names_render(pas_ctx* ctx, int64_t n, const int32_t* slot, int32_t slot_base,
                     int64_t* off_out /*[n + 1]*/, char* bytes_out, int64_t cap,
                     int64_t* n_bytes_out);
int pas_names_render_device(pas_ctx* ctx, int64_t n, const int32_t* d_slot, int32_t slot_base,
                            int64_t* d_off_out, char* d_bytes_out, int64_t cap,
                            int64_t* n_bytes_out, void* hip_stream);

/* Lookup plus first-seen assignment (n <= INT32_MAX).  The distinct non-empty names without a
 * slot, in order of first appearance among the entries, receive the spare slots in ascending
 * slot index.  new_entry_out / new_slot_out [new_cap] (host arrays in both forms) list, in
 * ascending entry index, the first appearance of each new name and the slot it got; *n_new_out
 * is the number of distinct new names.  If that exceeds min(spare slots, new_cap) the call
 * returns PAS_ECAPACITY with *n_new_out set, changes nothing, and slot_out holds the plain
 * lookups.  Otherwise the names are appended and inserted and every entry's slot is written,
 * repeats of a new name included.  slot_out (d_slot_out) may be NULL.  Synchronous on the
 * stream: it is a table change, ordered by the caller after readers on other streams like
 * every snapshot change.  With no new name it is one lookup pass and the read-back of one
 * word.  No output depends on the order in which the device happens to process the entries. */
int pas_names_assign(pas_ctx* ctx, int64_t n, const int64_t* name_off, const char* bytes,
                     int32_t* slot_out, int64_t new_cap, int32_t* new_entry_out,
                     int32_t* new_slot_out, int64_t* n_new_out);
int pas_names_assign_device(pas_ctx* ctx, int64_t n, int64_t n_bytes, const int64_t* d_name_off,
                            const char* d_bytes, int32_t* d_slot_out, int64_t new_cap,
                            int32_t* new_entry_out, int32_t* new_slot_out, int64_t* n_new_out,
                            void* hip_stream);

/* Append spare slots (a smaller n_slots_new is PAS_EINVAL); the hash is rebuilt on the device
 * when its load factor would pass 1/2.  Synchronous on hip_stream. */
int pas_names_resize(pas_ctx* ctx, int32_t n_slots_new, void* hip_stream);
/* Renumber the slots with the map of pas_tas_snapshot_compact / pas_gas_snapshot_compact: new
 * slot j holds the name of old slot src_slot[j], or is spare for -1; the entries >= 0 are
 * strictly increasing and below n_slots, anything else is PAS_EINVAL.  The names of the old
 * slots the map does not list leave the table.  The pool is gathered and the hash rebuilt on
 * the device.  Synchronous on hip_stream. */
int pas_names_remap(pas_ctx* ctx, int32_t n_slots_new, const int32_t* src_slot,
                    void* hip_stream);

/* pas_tas_snapshot_update_quantities with each entry's node given by name: entry i's node is
 * the slot of name_bytes[name_off[i] .. name_off[i + 1]) (lookup only: the table does not
 * change).  A name without a slot is entry node -1: its literal is still validated and it
 * takes no further part (rules 1-2 of that call), like a slot >= the snapshot's n_nodes.
 * Both forms read rule 5 as the _device form does: the highest entry index of a (column, node)
 * gives the value.  *n_unknown_out (may be NULL) = the entries whose name has no slot.
 * Everything else, the synchronisation included, is that call's. */
int pas_tas_snapshot_update_quantities_names(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                             int32_t n_cols, const int32_t* cols,
                                             const int64_t* col_off, const int64_t* name_off,
                                             const char* name_bytes, const int64_t* lit_off,
                                             const char* bytes, int32_t* kind_out,
                                             int32_t* scale_out, int64_t* bad_entry,
                                             int64_t* n_unknown_out);
int pas_tas_snapshot_update_quantities_names_device(
    pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_cols, const int32_t* cols,
    const int64_t* col_off, int64_t n_name_bytes, const int64_t* d_name_off,
    const char* d_name_bytes, int64_t n_bytes, const int64_t* d_lit_off, const char* d_bytes,
    int32_t* kind_out, int32_t* scale_out, int64_t* bad_entry, int64_t* n_unknown_out,
    void* hip_stream);

/* ------------------------------------------------------------------------- */
/* Resident card-name table: the names of the GAS snapshot's card slots      */
/* ------------------------------------------------------------------------- */

/* The reference keeps a node's usage by card name (nodeStatuses, node_resource_cache.go:64,
 * 259-272) and reads a pod's cards as names (:253-256); card slots exist only here.  The table
 * names them for pas_gas_apply_annotations: n_slots rows (node slots) of k card slots, row s in
 * the order of used[s][.]: the label cards in sort.Strings order, then whatever the caller
 * keeps behind them (parked cards, which a lookup never matches).  Names are opaque bytes of
 * any length, byte 0 and bytes >= 0x80 included, and the empty name is a name like any other (a
 * label "card0..card1" lists a card ""); an unused slot is an empty name past the node's
 * n_cards.  The table belongs to the context, beside the GAS snapshot (pas_gas_snapshot_resize
 * and _compact do not touch it: the caller resizes and remaps it with the same arguments).
 * Every entry point answers PAS_ENOSNAP without a table and every change is synchronous.
 * Storage is freed with the context.  PAS_ABI_VERSION is unchanged: additions only.
 *
 * set: name (s, c) is bytes[name_off[s * k + c] .. name_off[s * k + c + 1]); 1 <= k <=
 * PAS_GAS_MAX_CARDS, name_off [n_slots * k + 1] starts at 0 and never decreases (PAS_EINVAL
 * otherwise).  Built in fresh storage and swapped in: after any error the previous table, if
 * any, is still valid. */
int pas_gas_card_names_set(pas_ctx* ctx, int32_t n_slots, int32_t k, const int64_t* name_off,
                           const char* bytes);
/* Rewrite whole rows, in call order: row r of the call (name_off [n_rows * k + 1]) replaces slot
 * row_slot[r]; a slot given twice keeps the later row.  A slot outside [0, n_slots) or a bad
 * name_off is PAS_EINVAL, nothing changed.  The new bytes are appended to the table's byte
 * pool and the old ones are dead; when the dead bytes pass the live ones the call gathers the
 * pool on the device, so rows rewritten many times do not grow it without bound. */
int pas_gas_card_names_update(pas_ctx* ctx, int32_t n_rows, const int32_t* row_slot,
                              const int64_t* name_off, const char* bytes);
/* Both sizes may only grow (PAS_EINVAL otherwise, or for k_new > PAS_GAS_MAX_CARDS); the spans
 * are re-pitched on the device and the new entries are empty names. */
int pas_gas_card_names_resize(pas_ctx* ctx, int32_t n_slots_new, int32_t k_new,
                              void* hip_stream);
/* Renumber the rows with the map of pas_gas_snapshot_compact / pas_names_remap: new row j is old
 * row src_slot[j], or k empty names for -1; the entries >= 0 are strictly increasing and below
 * n_slots, anything else is PAS_EINVAL.  The pool is gathered. */
int pas_gas_card_names_remap(pas_ctx* ctx, int32_t n_slots_new, const int32_t* src_slot,
                             void* hip_stream);
/* Rows, card slots per row and the bytes the pool holds, dead ones included (each output may be
 * NULL). */
int pas_gas_card_names_info(const pas_ctx* ctx, int32_t* n_slots, int32_t* k, int64_t* n_bytes);
/* The names packed in (slot, card) order: name_off_out [n_slots * k + 1] always, bytes_out [cap]
 * when cap >= the live bytes, else PAS_ECAPACITY (the size needed is name_off_out[n_slots * k],
 * and in the message; n_bytes of _info is always enough). */
int pas_gas_card_names_get(pas_ctx* ctx, int64_t* name_off_out, char* bytes_out, int64_t cap);
/* The same for the rows row_slot[0 .. n_rows) alone, in call order (a slot may repeat; one outside
 * the table is PAS_EINVAL): name_off_out [n_rows * k + 1], and bytes_out [cap] when cap >= those
 * rows' bytes, else PAS_ECAPACITY with the offsets delivered. */
int pas_gas_card_names_get_rows(pas_ctx* ctx, int32_t n_rows, const int32_t* row_slot,
                                int64_t* name_off_out, char* bytes_out, int64_t cap);
int pas_gas_card_names_drop(pas_ctx* ctx);

/* ------------------------------------------------------------------------- */
/* Instrumentation                                                           */
/* ------------------------------------------------------------------------- */

/* Kernel timing with HIP events on the stream each kernel is launched on.
 * Kernel ids: */
#define PAS_K_TAS_EVAL 1       /* per pod: pass bitmap + ordered host list (fused) */
#define PAS_K_TAS_VIOLATIONS 2 /* deschedule sweep */
#define PAS_K_GAS_PREP 3       /* per-GPU container requests */
#define PAS_K_GAS_FIT 4        /* per (pod, node) first fit */
#define PAS_K_TAS_PREP 5       /* rule ranges + pods bucketed by prioritize order */
#define PAS_K_TAS_LABELS 6     /* deschedule label plan */
#define PAS_K_TAS_SPAN 7       /* whole pas_tas_eval path: first launch start to last launch end */
#define PAS_K_PRIO_REQUEST 8   /* whole pas_tas_prioritize_request path (keys, sort, positions) */
#define PAS_K_TAS_GAS_TOPK 9   /* combined TAS + GAS top-k along each pod's order */
#define PAS_K_COUNT 10
#define PAS_TIMING_SPAN 1    /* whole paths: PAS_K_TAS_SPAN, PAS_K_PRIO_REQUEST, the GAS fit and
                                deschedule launches */
#define PAS_TIMING_KERNELS 2 /* every launch (events between launches add small gaps) */
int pas_set_timing(pas_ctx* ctx, int level); /* 0 = off */
/* Sum of elapsed ms and number of launches recorded for a kernel since the last reset. */
int pas_kernel_time(pas_ctx* ctx, int32_t kernel_id, double* total_ms, int64_t* launches);
int pas_reset_timing(pas_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* PAS_H_ */
