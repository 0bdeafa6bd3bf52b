// tas_ingest.hip — metric columns from resource.Quantity literals, parsed on the device.
//
// A refresh delivers NodeMetricsInfo maps, {node: resource.Quantity}
// (telemetry-aware-scheduling/pkg/metrics/client.go:25-32,64-78), one per metric every sync
// period (cache/autoupdating.go:37-73).  Turning them into columns is per literal independent
// work plus two small reductions per column, so it runs here, next to the sort it feeds:
//   1. parse_literals   one lane per literal: ParseQuantity in fixed-width state
//                       (quantity_fixed.h), giving the wide pair, the decimals and the largest
//                       scale at which the value fits int64;
//   2. ingest_summary   per column the most decimals and the smallest fit of the entries whose
//                       node is in range, and the lowest entry that did not parse; the host
//                       reads these few words back and chooses scale and kind per column as
//                       snapshot.tas_snapshot_from_metrics_wide does (milli floor included);
//   3. ingest_winner / ingest_encode   the column buffers: per (column, node) the entry with
//                       the highest index wins (atomicMax, then only the winner writes), values
//                       at the column's scale or as pairs, presence bits by 64-bit atomicOr;
//   4. the existing column update (tas_snapshot.hip) rebuilds the orders of exactly these
//      columns, narrow and wide ones, and publishes the generation once.
// The literals are adjacent in one blob, so neighbouring lanes read neighbouring bytes; a
// literal is some 8 to 20 bytes and the outputs 20, far below what the order rebuild moves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_staging.h"
#include "pas_internal.h"
#include "quantity_fixed.h"
#include "span_pool.h"

namespace pas {
namespace {

constexpr int kTpb = 256;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTpb - 1) / kTpb); }

// status | decimals << 8 | (fit + 1) << 16 of one parsed literal
__device__ __forceinline__ int32_t pack_meta(const QuantityFixed& r) {
  return (r.status & 0xff) | (r.decimals << 8) | ((r.fit + 1) << 16);
}
__device__ __forceinline__ int32_t meta_status(int32_t m) { return (int32_t)(int8_t)(m & 0xff); }
__device__ __forceinline__ int32_t meta_decimals(int32_t m) { return (m >> 8) & 0xff; }
__device__ __forceinline__ int32_t meta_fit(int32_t m) { return ((m >> 16) & 0xff) - 1; }

// Literal i is entry i of lit, its offsets read clamped (csr_entry.h): no offset takes a read
// outside the blob.  Any output may be null.
__global__ void parse_literals(int64_t n, ByteSpans lit, int64_t* __restrict__ whole,
                               uint32_t* __restrict__ nano, int32_t* __restrict__ decimals,
                               int32_t* __restrict__ status, int32_t* __restrict__ meta) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= n) return;
  int64_t b;
  const int64_t len = lit.span(i, &b);
  const QuantityFixed r = parse_quantity_fixed(lit.bytes + b, len);
  if (whole) whole[i] = r.whole;
  if (nano) nano[i] = r.nano;
  if (decimals) decimals[i] = r.decimals;
  if (status) status[i] = r.status;
  if (meta) meta[i] = pack_meta(r);
}

// The column of entry i: the largest c with col_off[c] <= i (empty columns share an offset
// with their successor and never win).
__device__ __forceinline__ int32_t entry_col(const int64_t* __restrict__ col_off, int32_t n_cols,
                                             int64_t i) {
  int32_t lo = 0, hi = n_cols - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (col_off[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__global__ void summary_init(int32_t n_cols, unsigned long long* __restrict__ bad,
                             int32_t* __restrict__ max_dec, int32_t* __restrict__ min_fit) {
  const int32_t c = blockIdx.x * kTpb + threadIdx.x;
  if (c == 0) *bad = ~0ull;
  if (c < n_cols) {
    max_dec[c] = 0;
    min_fit[c] = 9;
  }
}

// bad = min over the entries that did not parse of (index << 8 | status byte), whatever their
// node; max_dec / min_fit over the entries whose node is in range.  A column's entries are
// adjacent, so a wave nearly always serves one column: it reduces in registers and one lane
// issues the atomics (a million lanes on one address take milliseconds); a wave that spans a
// column boundary falls back to one atomic per lane.  The three values are monotone, so a plain
// read that already shows a value as good skips the atomic.  Every lane runs to the end: the
// shuffles need the whole wave.
__global__ void ingest_summary(int64_t T, int32_t n_cols, int32_t N,
                               const int64_t* __restrict__ col_off,
                               const int32_t* __restrict__ node, const int32_t* __restrict__ meta,
                               unsigned long long* bad, int32_t* max_dec, int32_t* min_fit) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  const bool live = i < T;
  const int32_t m = live ? meta[i] : 0;
  const bool parsed = !live || meta_status(m) == PAS_OK;
  unsigned long long key =
      parsed ? ~0ull : ((unsigned long long)i << 8) | (unsigned long long)(m & 0xff);
  const int32_t nd = live && parsed ? node[i] : -1;
  const bool in = nd >= 0 && nd < N;
  const int32_t c = in ? entry_col(col_off, n_cols, i) : -1;
  int32_t dec = in ? meta_decimals(m) : 0, fit = in ? meta_fit(m) : 9;
  int32_t c_hi = c, c_lo = in ? c : INT32_MAX;  // the wave's columns, lanes out of range aside
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long k2 = __shfl_xor(key, off, 64);
    key = k2 < key ? k2 : key;
    c_hi = max(c_hi, __shfl_xor(c_hi, off, 64));
    c_lo = min(c_lo, __shfl_xor(c_lo, off, 64));
  }
  const bool leader = (threadIdx.x & 63) == 0;
  if (leader && key != ~0ull && key < *(volatile unsigned long long*)bad) atomicMin(bad, key);
  if (c_hi < 0) return;  // no lane in range (wave-uniform)
  bool mine = in;        // this lane issues its own atomics
  int32_t col = c;
  if (c_lo == c_hi) {    // one column (wave-uniform): reduce, the leader issues
    for (int off = 32; off > 0; off >>= 1) {
      dec = max(dec, __shfl_xor(dec, off, 64));
      fit = min(fit, __shfl_xor(fit, off, 64));
    }
    mine = leader;
    col = c_hi;
  }
  if (!mine) return;
  if (dec > ((volatile int32_t*)max_dec)[col]) atomicMax(&max_dec[col], dec);
  if (fit < ((volatile int32_t*)min_fit)[col]) atomicMin(&min_fit[col], fit);
}

// winner [n_cols][N] (-1 before): the highest entry index per (column buffer row, node).
__global__ void ingest_winner(int64_t T, int32_t n_cols, int32_t N,
                              const int64_t* __restrict__ col_off,
                              const int32_t* __restrict__ node, const int32_t* __restrict__ brow,
                              int32_t* winner) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= T) return;
  const int32_t nd = node[i];
  if (nd < 0 || nd >= N) return;
  const int32_t c = entry_col(col_off, n_cols, i);
  atomicMax(&winner[(int64_t)brow[c] * N + nd], (int32_t)i);
}

// The winners into the column buffers (zero before).  mult[c] = 10^scale of a narrow column:
// value * 10^scale = whole * 10^scale + nano / 10^(9 - scale), exact and inside int64 because
// every in-range entry of the column fits that scale (formed modulo 2^64: the floor's product
// alone may pass -2^63).  mult[c] = 0: a wide column keeps the pair.
__global__ void ingest_encode(int64_t T, int32_t n_cols, int32_t N, int64_t W,
                              const int64_t* __restrict__ col_off,
                              const int32_t* __restrict__ node, const int32_t* __restrict__ brow,
                              const int64_t* __restrict__ mult,
                              const int32_t* __restrict__ winner,
                              const int64_t* __restrict__ whole, const uint32_t* __restrict__ nano,
                              int64_t* __restrict__ vals, uint32_t* __restrict__ nano_out,
                              unsigned long long* present) {
  const int64_t i = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (i >= T) return;
  const int32_t nd = node[i];
  if (nd < 0 || nd >= N) return;
  const int32_t c = entry_col(col_off, n_cols, i);
  const int64_t row = brow[c];
  if (winner[row * N + nd] != (int32_t)i) return;
  const int64_t m = mult[c];
  if (m == 0) {
    vals[row * N + nd] = whole[i];
    nano_out[row * N + nd] = nano[i];
  } else {
    const uint32_t div = 1000000000u / (uint32_t)m;
    vals[row * N + nd] = (int64_t)((uint64_t)whole[i] * (uint64_t)m + (uint64_t)(nano[i] / div));
  }
  atomicOr(&present[row * W + (nd >> 6)], 1ull << (nd & 63));
}

// The parse of the n literals of lit on device arrays, enqueued on s; an output may be null.
int quantities_parse_launch(pas_ctx* ctx, int64_t n, ByteSpans lit, int64_t* d_whole,
                            uint32_t* d_nano, int32_t* d_decimals, int32_t* d_status,
                            hipStream_t s) {
  if (n <= 0) return PAS_OK;
  parse_literals<<<blocks_for(n), kTpb, 0, s>>>(n, lit, d_whole, d_nano, d_decimals, d_status,
                                                nullptr);
  PAS_HIP(ctx, hipGetLastError());
  return PAS_OK;
}

// pas_tas_snapshot_update_quantities_device past its argument checks (cols distinct and in
// range, col_off a CSR from 0 with at most INT32_MAX entries): synchronous on s, workspace
// from the slot of s.  A literal that does not parse: its status, *bad_entry its index,
// nothing changed.
int tas_update_quantities_launch(pas_ctx* ctx, uint64_t gen_to, int32_t n_cols,
                                 const int32_t* cols, const int64_t* col_off,
                                 const int32_t* d_entry_node, ByteSpans lit, int32_t* kind_out,
                                 int32_t* scale_out, int64_t* bad_entry, hipStream_t s) {
  TasSnapshot& t = ctx->tas;
  const int32_t N = t.n_nodes;
  const int64_t W = w64(N);
  if (bad_entry) *bad_entry = -1;
  if (n_cols == 0)  // the generation only
    return tas_snapshot_update_mixed(ctx, gen_to, 0, nullptr, 0, nullptr, nullptr, nullptr,
                                     nullptr, s);
  const int64_t T = col_off[n_cols];
  const size_t nc = (size_t)n_cols, cn = nc * (size_t)N, cw = nc * (size_t)W, nt = (size_t)T;
  int rc = PAS_OK;
  SlotScope scope(ctx, s, 0, &rc);
  if (!scope.slot) return rc;
  // parsed entries | column offsets, summary, per-column plan | column buffers
  const size_t summary_bytes = sizeof(unsigned long long) + 2 * sizeof(int32_t) * nc;
  const size_t zero_bytes = sizeof(int64_t) * cn + sizeof(uint64_t) * cw + sizeof(uint32_t) * cn;
  const size_t total = carve_size({sizeof(int64_t) * nt, sizeof(uint32_t) * nt,
                                   sizeof(int32_t) * nt, sizeof(int64_t) * (nc + 1),
                                   summary_bytes, sizeof(int64_t) * nc, sizeof(int32_t) * nc,
                                   zero_bytes, sizeof(int32_t) * cn});
  char* base = static_cast<char*>(slot_buf(ctx, scope.slot, kBufIngest, total, s, &rc));
  if (!base) return rc;
  Carve cv{base};
  int64_t* d_whole = cv.take<int64_t>(nt);
  uint32_t* d_nano = cv.take<uint32_t>(nt);
  int32_t* d_meta = cv.take<int32_t>(nt);
  int64_t* d_col_off = cv.take<int64_t>(nc + 1);
  char* d_summary = cv.take<char>(summary_bytes);
  int64_t* d_mult = cv.take<int64_t>(nc);
  int32_t* d_brow = cv.take<int32_t>(nc);
  char* d_zero = cv.take<char>(zero_bytes);
  int32_t* d_winner = cv.take<int32_t>(cn);
  unsigned long long* d_bad = reinterpret_cast<unsigned long long*>(d_summary);
  int32_t* d_max_dec = reinterpret_cast<int32_t*>(d_summary + sizeof(unsigned long long));
  int32_t* d_min_fit = d_max_dec + nc;
  int64_t* c_vals = reinterpret_cast<int64_t*>(d_zero);  // [n_cols][N], 8-byte parts first
  uint64_t* c_present = reinterpret_cast<uint64_t*>(c_vals + cn);
  uint32_t* c_nano = reinterpret_cast<uint32_t*>(c_present + cw);

  // 1, 2: parse every entry, reduce per column
  PAS_HIP(ctx, hipMemcpyAsync(d_col_off, col_off, sizeof(int64_t) * (nc + 1),
                              hipMemcpyHostToDevice, s));
  summary_init<<<blocks_for(n_cols), kTpb, 0, s>>>(n_cols, d_bad, d_max_dec, d_min_fit);
  PAS_HIP(ctx, hipGetLastError());
  if (T > 0) {
    parse_literals<<<blocks_for(T), kTpb, 0, s>>>(T, lit, d_whole, d_nano, nullptr, nullptr,
                                                  d_meta);
    PAS_HIP(ctx, hipGetLastError());
    ingest_summary<<<blocks_for(T), kTpb, 0, s>>>(T, n_cols, N, d_col_off, d_entry_node, d_meta,
                                                  d_bad, d_max_dec, d_min_fit);
    PAS_HIP(ctx, hipGetLastError());
  }
  std::vector<char> summary(summary_bytes);
  PAS_HIP(ctx, hipMemcpyAsync(summary.data(), d_summary, summary_bytes, hipMemcpyDeviceToHost, s));
  PAS_HIP(ctx, hipStreamSynchronize(s));  // (col_off is the caller's again as well)
  const unsigned long long bad = *reinterpret_cast<const unsigned long long*>(summary.data());
  if (bad != ~0ull) {  // nothing has changed
    const int64_t at = (int64_t)(bad >> 8);
    const int code = (int)(int8_t)(bad & 0xff);
    if (bad_entry) *bad_entry = at;
    return set_error(ctx, code, "pas_tas_snapshot_update_quantities: entry " +
                                    std::to_string(at) +
                                    (code == PAS_ENOTEXACT ? " has its integer part outside int64"
                                                           : " is no resource.Quantity"));
  }
  const int32_t* max_dec =
      reinterpret_cast<const int32_t*>(summary.data() + sizeof(unsigned long long));
  const int32_t* min_fit = max_dec + nc;

  // the plan: scale max(decimals, 3); narrow iff every in-range entry fits it.  Narrow columns
  // take the first buffer rows, wide ones the rest (the two updates read contiguous rows).
  std::vector<int64_t> mult(nc);
  std::vector<int32_t> brow(nc), cols_narrow, cols_wide;
  for (size_t c = 0; c < nc; ++c) {
    const int32_t sc = std::max(max_dec[c], 3);
    const bool narrow = min_fit[c] >= sc;
    int64_t m = 1;
    for (int32_t i = 0; i < sc; ++i) m *= 10;
    mult[c] = narrow ? m : 0;
    (narrow ? cols_narrow : cols_wide).push_back(cols[c]);
  }
  const int32_t n_narrow = (int32_t)cols_narrow.size(), n_wide = (int32_t)cols_wide.size();
  bool rescale = false;
  for (size_t c = 0, in = 0, iw = 0; c < nc; ++c) {
    const size_t m = (size_t)cols[c];
    if (mult[c] != 0) {
      brow[c] = (int32_t)in++;
      rescale |= t.scale_host[2 * m] != mult[c];
      t.scale_host[2 * m] = mult[c];
      t.scale_host[2 * m + 1] = INT64_MAX / mult[c];
    } else {
      brow[c] = n_narrow + (int32_t)iw++;
    }
    int32_t recorded = 0;
    for (int64_t q = t.scale_host[2 * m]; q > 1; q /= 10) ++recorded;
    if (kind_out) kind_out[c] = mult[c] == 0;
    if (scale_out) scale_out[c] = recorded;  // a wide column keeps the scale it had
  }

  // 3: the column buffers
  PAS_HIP(ctx, hipMemcpyAsync(d_mult, mult.data(), sizeof(int64_t) * nc, hipMemcpyHostToDevice, s));
  PAS_HIP(ctx, hipMemcpyAsync(d_brow, brow.data(), sizeof(int32_t) * nc, hipMemcpyHostToDevice, s));
  if (zero_bytes) PAS_HIP(ctx, hipMemsetAsync(d_zero, 0, zero_bytes, s));
  if (cn) PAS_HIP(ctx, hipMemsetAsync(d_winner, 0xff, sizeof(int32_t) * cn, s));
  if (T > 0 && N > 0) {
    ingest_winner<<<blocks_for(T), kTpb, 0, s>>>(T, n_cols, N, d_col_off, d_entry_node, d_brow,
                                                 d_winner);
    PAS_HIP(ctx, hipGetLastError());
    ingest_encode<<<blocks_for(T), kTpb, 0, s>>>(
        T, n_cols, N, W, d_col_off, d_entry_node, d_brow, d_mult, d_winner, d_whole, d_nano,
        c_vals, c_nano, reinterpret_cast<unsigned long long*>(c_present));
    PAS_HIP(ctx, hipGetLastError());
  }
  // 4: the narrow columns' scales, before anything evaluates the new orders; then the orders
  if (rescale)
    PAS_HIP(ctx, hipMemcpyAsync(t.scale_tab, t.scale_host.data(),
                                sizeof(int64_t) * t.scale_host.size(), hipMemcpyHostToDevice, s));
  rc = tas_snapshot_update_mixed(ctx, gen_to, n_narrow, cols_narrow.data(), n_wide,
                                 cols_wide.data(), c_vals, c_nano, c_present, s);
  const hipError_t e = hipStreamSynchronize(s);  // mult / brow / the column lists are locals
  if (rc) return rc;
  PAS_HIP(ctx, e);
  return PAS_OK;
}

// The refresh with each entry's node given by name (name_table.hip): the names are resolved,
// lookup only, into a buffer of the stream's slot and the refresh above runs on it.  The count
// of entries without a slot comes back on s before that launch's own synchronize.
int update_quantities_names_launch(pas_ctx* ctx, uint64_t gen_to, int32_t n_cols,
                                   const int32_t* cols, const int64_t* col_off, ByteSpans names,
                                   ByteSpans lit, int32_t* kind_out, int32_t* scale_out,
                                   int64_t* bad_entry, int64_t* n_unknown_out, hipStream_t s) {
  const int64_t T = n_cols > 0 ? col_off[n_cols] : 0;
  if (n_unknown_out) *n_unknown_out = 0;
  int rc = PAS_OK;
  SlotScope scope(ctx, s, 0, &rc);
  if (!scope.slot) return rc;
  int32_t* d_node = nullptr;
  uint32_t unknown = 0;
  if (T > 0) {
    const size_t total = carve_size({sizeof(uint32_t), sizeof(int32_t) * (size_t)T});
    char* base = static_cast<char*>(slot_buf(ctx, scope.slot, kBufNames, total, s, &rc));
    if (!base) return rc;
    Carve cv{base};
    uint32_t* d_ctr = cv.take<uint32_t>(1);
    d_node = cv.take<int32_t>((size_t)T);
    PAS_HIP(ctx, hipMemsetAsync(d_ctr, 0, sizeof(uint32_t), s));
    rc = names_resolve_launch(ctx, T, names, d_node, nullptr, d_ctr, true, s);
    if (rc) return rc;
    PAS_HIP(ctx, hipMemcpyAsync(&unknown, d_ctr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  rc = tas_update_quantities_launch(ctx, gen_to, n_cols, cols, col_off, d_node, lit, kind_out,
                                    scale_out, bad_entry, s);
  if (T > 0 && rc) (void)hipStreamSynchronize(s);  // (an early error: `unknown` is a local)
  if (n_unknown_out) *n_unknown_out = unknown;
  return rc;
}

// The checks every form of pas_tas_snapshot_update_quantities shares: the snapshot and its
// generation, the columns, and col_off as a CSR of at most INT32_MAX entries; *T = the entries.
int check_update_quantities(pas_ctx* ctx, uint64_t gen_from, int32_t n_cols, const int32_t* cols,
                            const int64_t* col_off, int64_t* T, const std::string& fn) {
  *T = 0;
  int rc = check_update(ctx, gen_from, n_cols, cols, col_off, col_off, fn.c_str());
  if (rc) return rc;
  if (n_cols == 0) return PAS_OK;
  if ((rc = check_host_spans(ctx, n_cols, col_off, nullptr, fn + ": col_off", false))) return rc;
  if (col_off[n_cols] > INT32_MAX)
    return set_error(ctx, PAS_EINVAL, fn + ": more than INT32_MAX entries");
  *T = col_off[n_cols];
  return PAS_OK;
}

}  // namespace
}  // namespace pas

using namespace pas;

extern "C" {

int pas_quantities_to_wide(pas_ctx* ctx, int64_t n, const int64_t* lit_off, const char* bytes,
                           int64_t* whole, uint32_t* nano, int32_t* decimals, int32_t* status) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_quantities_to_wide";
  if (n < 0) return set_error(ctx, PAS_EINVAL, fn + ": n < 0");
  if (n == 0) return PAS_OK;
  int rc = check_host_spans(ctx, n, lit_off, bytes, fn);
  if (rc) return rc;
  if ((rc = activate(ctx))) return rc;
  Staging st(ctx);
  ByteSpans lit;
  int64_t* d_whole;
  uint32_t* d_nano;
  int32_t *d_dec, *d_status;
  st.in_spans(lit, n, lit_off, bytes);
  st.out_opt(d_whole, whole, (size_t)n);
  st.out_opt(d_nano, nano, (size_t)n);
  st.out_opt(d_dec, decimals, (size_t)n);
  st.out_opt(d_status, status, (size_t)n);
  if ((rc = st.upload())) return rc;
  if ((rc = quantities_parse_launch(ctx, n, lit, d_whole, d_nano, d_dec, d_status, ctx->stream)))
    return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_quantities_to_wide_device(pas_ctx* ctx, int64_t n, int64_t n_bytes,
                                  const int64_t* d_lit_off, const char* d_bytes,
                                  int64_t* d_whole, uint32_t* d_nano, int32_t* d_decimals,
                                  int32_t* d_status, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_quantities_to_wide_device";
  const ByteSpans lit{n_bytes, d_lit_off, d_bytes};
  if (n < 0) return set_error(ctx, PAS_EINVAL, fn + ": n < 0");
  int rc = check_device_spans(ctx, n, lit, fn);
  if (rc || n == 0) return rc;
  if ((rc = activate(ctx))) return rc;
  return quantities_parse_launch(ctx, n, lit, d_whole, d_nano, d_decimals, d_status,
                                 pick_stream(ctx, hip_stream));
}

int pas_tas_snapshot_update_quantities_device(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                              int32_t n_cols, const int32_t* cols,
                                              const int64_t* col_off, int64_t n_bytes,
                                              const int32_t* d_entry_node,
                                              const int64_t* d_lit_off, const char* d_bytes,
                                              int32_t* kind_out, int32_t* scale_out,
                                              int64_t* bad_entry, void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_tas_snapshot_update_quantities_device";
  const ByteSpans lit{n_bytes, d_lit_off, d_bytes};
  if (bad_entry) *bad_entry = -1;
  int64_t T;
  int rc = check_update_quantities(ctx, gen_from, n_cols, cols, col_off, &T, fn);
  if (rc) return rc;
  if (T > 0 && !d_entry_node) return set_error(ctx, PAS_EINVAL, fn + ": null input");
  if (T > 0 && (rc = check_device_spans(ctx, T, lit, fn + ": lit_off"))) return rc;
  if ((rc = activate(ctx))) return rc;
  return tas_update_quantities_launch(ctx, gen_to, n_cols, cols, col_off, d_entry_node, lit,
                                      kind_out, scale_out, bad_entry,
                                      pick_stream(ctx, hip_stream));
}

int pas_tas_snapshot_update_quantities(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                       int32_t n_cols, const int32_t* cols,
                                       const int64_t* col_off, const int32_t* entry_node,
                                       const int64_t* lit_off, const char* bytes,
                                       int32_t* kind_out, int32_t* scale_out,
                                       int64_t* bad_entry) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_tas_snapshot_update_quantities";
  if (bad_entry) *bad_entry = -1;
  int64_t T;
  int rc = check_update_quantities(ctx, gen_from, n_cols, cols, col_off, &T, fn);
  if (rc) return rc;
  if (T > 0) {
    if (!entry_node) return set_error(ctx, PAS_EINVAL, fn + ": null input");
    if ((rc = check_host_spans(ctx, T, lit_off, bytes, fn + ": lit_off"))) return rc;
    // updateMetric replaces a node map: a node listed twice in one column is no map
    const int32_t N = ctx->tas.n_nodes;
    std::vector<uint64_t> seen((size_t)w64(N));
    for (int32_t c = 0; c < n_cols; ++c) {
      std::fill(seen.begin(), seen.end(), 0);
      for (int64_t i = col_off[c]; i < col_off[c + 1]; ++i) {
        const int32_t nd = entry_node[i];
        if (nd < 0 || nd >= N) continue;
        uint64_t& w = seen[(size_t)(nd >> 6)];
        if ((w >> (nd & 63)) & 1ull)
          return set_error(ctx, PAS_EINVAL, fn + ": column " + std::to_string(cols[c]) +
                                                " lists node " + std::to_string(nd) + " twice");
        w |= 1ull << (nd & 63);
      }
    }
  }
  if ((rc = activate(ctx))) return rc;
  Staging st(ctx);
  int32_t* d_node;
  ByteSpans lit;
  st.in(d_node, entry_node, (size_t)T);
  st.in_spans(lit, T, lit_off, bytes);
  if ((rc = st.upload())) return rc;
  rc = tas_update_quantities_launch(ctx, gen_to, n_cols, cols, col_off, d_node, lit, kind_out,
                                    scale_out, bad_entry, ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

int pas_tas_snapshot_update_quantities_names_device(
    pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to, int32_t n_cols, const int32_t* cols,
    const int64_t* col_off, int64_t n_name_bytes, const int64_t* d_name_off,
    const char* d_name_bytes, int64_t n_bytes, const int64_t* d_lit_off, const char* d_bytes,
    int32_t* kind_out, int32_t* scale_out, int64_t* bad_entry, int64_t* n_unknown_out,
    void* hip_stream) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_tas_snapshot_update_quantities_names_device";
  const ByteSpans names{n_name_bytes, d_name_off, d_name_bytes}, lit{n_bytes, d_lit_off, d_bytes};
  if (bad_entry) *bad_entry = -1;
  if (n_unknown_out) *n_unknown_out = 0;
  if (!ctx->names.valid) return set_error(ctx, PAS_ENOSNAP, fn + ": no name table");
  int64_t T;
  int rc = check_update_quantities(ctx, gen_from, n_cols, cols, col_off, &T, fn);
  if (rc) return rc;
  if (T > 0 && ((rc = check_device_spans(ctx, T, names, fn + ": name_off")) ||
                (rc = check_device_spans(ctx, T, lit, fn + ": lit_off"))))
    return rc;
  if ((rc = activate(ctx))) return rc;
  return update_quantities_names_launch(ctx, gen_to, n_cols, cols, col_off, names, lit, kind_out,
                                        scale_out, bad_entry, n_unknown_out,
                                        pick_stream(ctx, hip_stream));
}

int pas_tas_snapshot_update_quantities_names(pas_ctx* ctx, uint64_t gen_from, uint64_t gen_to,
                                             int32_t n_cols, const int32_t* cols,
                                             const int64_t* col_off, const int64_t* name_off,
                                             const char* name_bytes, const int64_t* lit_off,
                                             const char* bytes, int32_t* kind_out,
                                             int32_t* scale_out, int64_t* bad_entry,
                                             int64_t* n_unknown_out) {
  if (!ctx) return PAS_EINVAL;
  const std::string fn = "pas_tas_snapshot_update_quantities_names";
  if (bad_entry) *bad_entry = -1;
  if (n_unknown_out) *n_unknown_out = 0;
  if (!ctx->names.valid) return set_error(ctx, PAS_ENOSNAP, fn + ": no name table");
  int64_t T;
  int rc = check_update_quantities(ctx, gen_from, n_cols, cols, col_off, &T, fn);
  if (rc) return rc;
  if (T > 0 && ((rc = check_host_spans(ctx, T, lit_off, bytes, fn + ": lit_off")) ||
                (rc = check_host_spans(ctx, T, name_off, name_bytes, fn + ": name_off"))))
    return rc;
  if ((rc = activate(ctx))) return rc;
  Staging st(ctx);
  ByteSpans names, lit;
  st.in_spans(names, T, name_off, name_bytes);
  st.in_spans(lit, T, lit_off, bytes);
  if ((rc = st.upload())) return rc;
  rc = update_quantities_names_launch(ctx, gen_to, n_cols, cols, col_off, names, lit, kind_out,
                                      scale_out, bad_entry, n_unknown_out, ctx->stream);
  if (rc) return rc;
  PAS_HIP(ctx, st.fetch());
  return PAS_OK;
}

}  // extern "C"
