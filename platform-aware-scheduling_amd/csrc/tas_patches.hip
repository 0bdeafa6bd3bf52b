// tas_patches.hip — the deschedule label plan as a compact patch list: one record per node
// whose PATCH body is not "[]", in ascending node index, built on the device.
//
// The label plan (tas_labels.hip) answers two dense masks per node, and Deschedule.patchNode
// (deschedule/enforce.go:74-86) sends a body only where they are not both zero.  Here the same
// masks are computed per node from the [S][W64] bitmaps and only the nodes that need a PATCH
// leave the device, as (node, add, remove) records.  Two more bitmaps may say which carried
// labels already hold the value the patch would write: a label that is "violating" needs no
// add from any strategy of its name, a label that is "null" needs no remove + add "null".  The
// reduced masks patch a node to the same labels as the full ones.
//
// The masks are computed in the bitmaps' own layout.  A wave takes one 64-node word: lane s
// loads word w of row s of each bitmap, so a lane holds one strategy's bits of 64 nodes.  In that
// layout the plan is a few word operations per lane: a shared name's violated bits are the OR
// of its member lanes, its first strategy's settled bits are broadcast to the members with
// readlane, and add' / rem' come out as one word per strategy.  The OR of those words over the
// wave is the bitmask of the word's nodes that need a patch: its popcount is the count, its
// prefix popcounts are the ranks, and only a word that lists a node is transposed (the 64 x S
// bit transpose of label_plan_kernel: readlane broadcasts row s, lane n takes bit n) to give
// every listed node its two masks.  A settled cluster transposes almost nothing.
//
// Stable stream compaction as in tas_compact.hip, a segment being 1024 nodes (16 bitmap words):
//   count    one workgroup per segment: the number of nodes listed and the segment's violated
//            (node, name) pairs;
//   scan     one workgroup: the exclusive scan of the segment counts in place, and n_patches;
//   scatter  each segment's words computed again, its listed nodes ranked by the words' node
//            masks and prefix popcounts behind the segment's base, and written while the rank
//            is below cap.
// totalViolations comes from the count kernel's per-segment pairs through label_total_launch.
// No atomics and no workgroup waits for another: every output position is computed, so the
// list is reproducible and a truncated list is the first cap records.  Computing the words
// twice reads at most four S x W64 bitmap sets twice, which is less traffic than writing the
// dense masks and reading them back.  All kernels: 256 threads, offsets in 64 bits, 32 bytes
// of LDS at most, no scratch.
//
// pas_label_patch_json_batch below renders the bodies of a whole list on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "json_out.h"
#include "pas_internal.h"

namespace pas {
namespace {

constexpr int kTpb = 256;
constexpr int kWaves = kTpb / 64;
constexpr int kSegNodes = 1024;                  // nodes per segment
constexpr int kSegWords = kSegNodes / 64;        // bitmap words per segment
constexpr int kWaveWords = kSegWords / kWaves;   // consecutive words per wave

// The bitmaps of one call ([S][W] each; labels, violating and null_ may be null, and the value
// bitmaps are null when labels is).
struct PatchIn {
  int32_t n_nodes, n_strat;
  int64_t W;
  NamePlan names;
  const uint64_t* viol;
  const uint64_t* labels;
  const uint64_t* violating;
  const uint64_t* null_;
};

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int s) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, s);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), s);
  return (uint64_t)hi << 32 | lo;
}

// Bit s of the result = bit `lane` of lane s's word, s < n_strat (a wave-wide call).
__device__ __forceinline__ uint64_t transpose_bits(uint64_t word, int n_strat, int lane) {
  uint64_t m = 0;
  for (int s = 0; s < n_strat; ++s) m |= ((readlane64(word, s) >> lane) & 1ull) << s;
  return m;
}

// The OR of x over the wave, in every lane.
__device__ __forceinline__ uint64_t wave_or(uint64_t x) {
  for (int off = 32; off > 0; off >>= 1) x |= __shfl_xor(x, off, 64);
  return x;
}

// Word w (below in.W) in strategy layout, a wave-wide call: lane s gets the nodes of the word
// where strategy s is added (*add) and, s being a name's first strategy, where that name's
// label is removed (*rem) after the reduction by the value bitmaps, both 0 for a lane at or
// past n_strat and for nodes at or past n_nodes, and the violated (node, name) pairs of the
// names lane s stands for.  Returns the nodes of the word with a non-empty patch (uniform).
__device__ __forceinline__ uint64_t word_masks(const PatchIn& in, int64_t w, int lane,
                                               uint64_t* add, uint64_t* rem, int32_t* violated) {
  const NamePlan& np = in.names;
  const int64_t left = (int64_t)in.n_nodes - w * 64;
  const uint64_t valid = left >= 64 ? ~0ull : (1ull << left) - 1ull;
  const bool canon = np.canon >> lane & 1ull;  // (canon has no bit at or past n_strat)
  uint64_t vw = 0, lw = 0, xw = 0, zw = 0;
  if (lane < in.n_strat) {
    const int64_t at = lane * in.W + w;
    vw = in.viol[at] & valid;
    if (in.labels && canon) {  // only the rows of first strategies are read
      lw = in.labels[at] & valid;
      if (in.violating) xw = in.violating[at];
      if (in.null_) zw = in.null_[at];
    }
  }
  uint64_t vn = vw;            // a first strategy's lane: where its name is violated
  uint64_t settled = lw & xw;  // where the lane's name is carried as "violating"
  for (int32_t g = 0; g < np.n_groups; ++g) {  // names of two or more strategies
    const bool member = np.group[g] >> lane & 1ull;
    const uint64_t any = wave_or(member ? vw : 0ull);
    const uint64_t first = readlane64(settled, np.key[g]);
    if (lane == np.key[g]) vn = any;
    if (member) settled = first;
  }
  *add = vw & ~settled;
  *rem = lw & ~vn & ~zw;  // (lw is 0 off the first strategies)
  *violated = canon ? __popcll(vn) : 0;
  const uint64_t keep = wave_or(*add | *rem);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)keep);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(keep >> 32));
  return (uint64_t)hi << 32 | lo;
}

// counts[seg] = the nodes of segment seg with a non-empty patch, part[seg] = its violated pairs.
__global__ __launch_bounds__(kTpb) void patch_count_kernel(const PatchIn in,
                                                           int32_t* __restrict__ counts,
                                                           int64_t* __restrict__ part) {
  __shared__ int32_t wave_n[kWaves], wave_v[kWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w0 = (int64_t)blockIdx.x * kSegWords + wave * kWaveWords;
  int32_t kept = 0, violated = 0;
  for (int i = 0; i < kWaveWords; ++i) {
    if (w0 + i >= in.W) break;  // (wave-uniform)
    uint64_t a, r;
    int32_t v;
    kept += __popcll(word_masks(in, w0 + i, lane, &a, &r, &v));
    violated += v;
  }
  for (int off = 32; off > 0; off >>= 1) violated += __shfl_xor(violated, off, 64);
  if (lane == 0) {
    wave_n[wave] = kept;
    wave_v[wave] = violated;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t n = 0, v = 0;
    for (int i = 0; i < kWaves; ++i) {
      n += wave_n[i];
      v += wave_v[i];
    }
    counts[blockIdx.x] = n;
    part[blockIdx.x] = v;
  }
}

// One workgroup: counts[0 .. segs) become their exclusive scan, *n_patches their sum.
__global__ __launch_bounds__(kTpb) void patch_scan_kernel(int32_t segs,
                                                          int32_t* __restrict__ counts,
                                                          int64_t* __restrict__ n_patches) {
  __shared__ int32_t wave_sum[kWaves];
  const int32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  int32_t carry = 0;  // (at most n_nodes < 2^31)
  for (int32_t at = 0; at < segs; at += kTpb) {
    const int32_t v = t < segs - at ? counts[at + t] : 0;
    int32_t x = v;  // inclusive scan of the wave
#pragma unroll
    for (int32_t off = 1; off < 64; off <<= 1) {
      const int32_t y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    __syncthreads();  // (the previous chunk's sums have been read)
    if (lane == 63) wave_sum[w] = x;
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int32_t i = 0; i < kWaves; ++i) {
      before += i < w ? wave_sum[i] : 0;
      all += wave_sum[i];
    }
    if (t < segs - at) counts[at + t] = carry + before + x - v;
    carry += all;
  }
  if (t == 0) *n_patches = carry;
}

// base[seg]: the scanned counts.  Records at and past cap are not written.
__global__ __launch_bounds__(kTpb) void patch_scatter_kernel(const PatchIn in,
                                                             const int32_t* __restrict__ base,
                                                             int64_t cap,
                                                             int32_t* __restrict__ patch_node,
                                                             uint64_t* __restrict__ patch_add,
                                                             uint64_t* __restrict__ patch_rem) {
  __shared__ int32_t wave_n[kWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w0 = (int64_t)blockIdx.x * kSegWords + wave * kWaveWords;
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t keep[kWaveWords], a[kWaveWords], r[kWaveWords];  // a, r: of node 64 w + lane
  int32_t kept = 0;
#pragma unroll
  for (int i = 0; i < kWaveWords; ++i) {
    keep[i] = a[i] = r[i] = 0;
    if (w0 + i < in.W) {  // (wave-uniform)
      uint64_t add, rem;
      int32_t v;
      keep[i] = word_masks(in, w0 + i, lane, &add, &rem, &v);
      if (keep[i]) {  // (wave-uniform)
        a[i] = transpose_bits(add, in.n_strat, lane);
        r[i] = transpose_bits(rem, in.n_strat, lane);
      }
      kept += __popcll(keep[i]);
    }
  }
  if (lane == 0) wave_n[wave] = kept;
  __syncthreads();
  int64_t pos = base[blockIdx.x];  // of the wave's first listed node
#pragma unroll
  for (int i = 0; i < kWaves; ++i) pos += i < wave ? wave_n[i] : 0;
#pragma unroll
  for (int i = 0; i < kWaveWords; ++i) {
    const int64_t at = pos + __popcll(keep[i] & below);
    if ((keep[i] >> lane & 1ull) && at < cap) {
      patch_node[at] = (int32_t)((w0 + i) * 64 + lane);
      patch_add[at] = a[i];
      patch_rem[at] = r[i];
    }
    pos += __popcll(keep[i]);
  }
}

// {"op":<op>,"path":"/metadata/labels/<name>","value":<value>} (put_patch of tas_labels.hip)
void put_patch(JsonOut& o, const char* op, const char* name, const char* value) {
  o.lit("{\"op\":");
  o.str(op);
  o.lit(",\"path\":\"");
  o.str_body("/metadata/labels/");
  o.str_body(name);
  o.lit("\",\"value\":");
  o.str(value);
  o.put('}');
}

// What one strategy's bit adds to a body: its add entry, or its remove + add "null" pair.
std::string patch_fragment(const char* name, bool remove) {
  std::string out;
  for (int pass = 0; pass < 2; ++pass) {  // the length, then the bytes
    JsonOut o{out.empty() ? nullptr : &out[0], (int64_t)out.size()};
    if (remove) {
      put_patch(o, "remove", name, "");
      o.put(',');
      put_patch(o, "add", name, "null");
    } else {
      put_patch(o, "add", name, "violating");
    }
    if (pass == 0) out.resize((size_t)o.pos);
  }
  return out;
}

}  // namespace

int label_patches_launch(pas_ctx* ctx, int32_t n_nodes, int32_t n_strat, const NamePlan& names,
                         const uint64_t* d_viol, const uint64_t* d_labels,
                         const uint64_t* d_violating, const uint64_t* d_null, int64_t cap,
                         int32_t* d_node, uint64_t* d_add, uint64_t* d_rem, int64_t* d_n_patches,
                         int64_t* d_total, hipStream_t s) {
  if (n_nodes == 0 || n_strat == 0) {  // no pairs: no patch, total 0
    PAS_HIP(ctx, hipMemsetAsync(d_n_patches, 0, sizeof(int64_t), s));
    return label_total_launch(ctx, 0, 0, nullptr, d_total, s);
  }
  const int64_t W = w64(n_nodes);
  const int32_t segs = (int32_t)((W + kSegWords - 1) / kSegWords);
  // the counts are the stream's slot buffer: calls on other streams may run beside
  int rc = PAS_OK;
  SlotScope sc(ctx, s, 0, &rc);
  if (!sc.slot) return rc;
  const size_t cnt_bytes = sizeof(int32_t) * (size_t)segs, part_bytes = sizeof(int64_t) * (size_t)segs;
  void* buf = slot_buf(ctx, sc.slot, kBufPatch, carve_size({cnt_bytes, part_bytes}), s, &rc);
  if (!buf) return rc;
  Carve cv{static_cast<char*>(buf)};
  int32_t* counts = cv.take<int32_t>((size_t)segs);
  int64_t* part = cv.take<int64_t>((size_t)segs);
  const PatchIn in{n_nodes, n_strat, W, names, d_viol, d_labels,
                   d_labels ? d_violating : nullptr, d_labels ? d_null : nullptr};
  TimedLaunch tl;
  timing_begin(ctx, s, PAS_K_TAS_LABELS, &tl);
  patch_count_kernel<<<(unsigned)segs, kTpb, 0, s>>>(in, counts, part);
  patch_scan_kernel<<<1, kTpb, 0, s>>>(segs, counts, d_n_patches);
  if (cap > 0)
    patch_scatter_kernel<<<(unsigned)segs, kTpb, 0, s>>>(in, counts, cap, d_node, d_add, d_rem);
  timing_end(ctx, s, &tl);
  PAS_HIP(ctx, hipGetLastError());
  return label_total_launch(ctx, segs, (int64_t)n_nodes * __builtin_popcountll(names.canon), part,
                            d_total, s);
}

int tas_deschedule_patches_launch(pas_ctx* ctx, int32_t n_strat, int32_t n_rules,
                                  const pas_rule* d_rules, const int32_t* d_rule_off,
                                  uint64_t* d_viol, const NamePlan& names,
                                  const uint64_t* d_labels, const uint64_t* d_violating,
                                  const uint64_t* d_null, int64_t cap, int32_t* d_node,
                                  uint64_t* d_add, uint64_t* d_rem, int64_t* d_n_patches,
                                  int64_t* d_total, hipStream_t s) {
  const int32_t N = ctx->tas.n_nodes;
  if (N > 0 && n_strat > 0) {
    if (!d_viol) {  // the sweep's bitmaps in the stream's slot, a buffer of their own: the
                    // patch launch below finds the same slot (it is this stream's now) and
                    // takes its counts from it
      int rc = PAS_OK;
      SlotScope sc(ctx, s, 0, &rc);
      if (!sc.slot) return rc;
      d_viol = static_cast<uint64_t*>(slot_buf(ctx, sc.slot, kBufPatchViol,
                                               sizeof(uint64_t) * (size_t)n_strat * (size_t)w64(N),
                                               s, &rc));
      if (!d_viol) return rc;
    }
    int rc = tas_violations_launch(ctx, n_strat, n_rules, d_rules, d_rule_off, d_viol, s);
    if (rc) return rc;
  }
  return label_patches_launch(ctx, N, n_strat, names, d_viol, d_labels, d_violating, d_null, cap,
                              d_node, d_add, d_rem, d_n_patches, d_total, s);
}

}  // namespace pas

// The bodies of a whole patch list back to back: body i is pas_label_patch_json of (add[i],
// rem[i]).  Each strategy's entries are rendered (escaped) once, a body is then a copy of the
// fragments its masks name.
extern "C" int pas_label_patch_json_batch(int32_t n_strat, const char* const* names,
                                          int64_t n_patches, const uint64_t* add,
                                          const uint64_t* rem, char* buf, int64_t cap,
                                          int64_t* offsets, int64_t* total_len) {
  if (n_strat < 0 || n_strat > 64 || !names || n_patches < 0 || !offsets || !total_len ||
      cap < 0 || (cap > 0 && !buf) || (n_patches > 0 && (!add || !rem)))
    return PAS_EINVAL;
  const uint64_t live = n_strat == 64 ? ~0ull : ((1ull << n_strat) - 1);
  uint64_t any_add = 0, any_rem = 0;
  for (int64_t i = 0; i < n_patches; ++i) {
    any_add |= add[i];
    any_rem |= rem[i];
  }
  if ((any_add | any_rem) & ~live) return PAS_EINVAL;
  for (int32_t s = 0; s < n_strat; ++s)
    if (((any_add | any_rem) >> s & 1) && !names[s]) return PAS_EINVAL;
  std::string add_frag[64], rem_frag[64];
  for (int32_t s = 0; s < n_strat; ++s) {
    if (any_add >> s & 1) add_frag[s] = pas::patch_fragment(names[s], false);
    if (any_rem >> s & 1) rem_frag[s] = pas::patch_fragment(names[s], true);
  }
  pas::JsonOut o{buf, cap};
  for (int64_t i = 0; i < n_patches; ++i) {
    offsets[i] = o.pos;
    o.put('[');
    bool first = true;
    for (uint64_t m = add[i]; m; m &= m - 1) {
      const std::string& f = add_frag[__builtin_ctzll(m)];
      if (!first) o.put(',');
      o.raw(f.data(), (int64_t)f.size());
      first = false;
    }
    for (uint64_t m = rem[i]; m; m &= m - 1) {
      const std::string& f = rem_frag[__builtin_ctzll(m)];
      if (!first) o.put(',');
      o.raw(f.data(), (int64_t)f.size());
      first = false;
    }
    o.put(']');
  }
  offsets[n_patches] = o.pos;
  *total_len = o.pos;
  return o.pos <= cap ? PAS_OK : PAS_ECAPACITY;
}
