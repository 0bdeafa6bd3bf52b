// annotation_fixed.h — the "gas-container-cards" annotation grammar in fixed-width state, for
// host and device code (plain C++ as well: no HIP header is needed to include this file).
//
// adjustPodResources reads the annotation with two strings.Split calls
// (gpu-aware-scheduling/pkg/gpuscheduler/node_resource_cache.go:241,253-256): on "|" for the
// containers' segments, and on "," for the card names of a segment that is not empty.  Go's
// Split of the empty string gives one empty string, so
//   segments            = 1 + count('|')      the empty annotation is one empty segment
//   names of a segment  = 0                   for the empty segment
//                       = 1 + count(',')      otherwise; the empty names of "a,,b", "a," and
//                                             ",a" are names like any other
// Names are opaque bytes: byte 0 and bytes >= 0x80 have no meaning here, only '|' and ','.
//
// annotation_walk visits the segments and the name spans in order through a visitor, in state
// that does not grow with the annotation: the counting pass and the resolving pass of
// gas_annotations.hip and the host entry point (gas_annotation.cpp) are this one routine with
// three visitors.
//
// annotation_render_len / annotation_render_write are the inverse (bindNode,
// gpu-aware-scheduling/pkg/gpuscheduler/scheduler.go:317-335, 423-431): the bytes of the
// annotation whose segments list given cards, for the host entry point (gas_annotation.cpp, one
// lane) and for a wavefront per bind (gas_render.hip, 64 lanes).
#pragma once

#include <cstdint>

#include "pas.h"

#if defined(__HIP__)
#define PAS_AF_HD __host__ __device__
#else
#define PAS_AF_HD
#endif

namespace pas {

struct AnnotationCounts {
  int64_t n_segments;  // 1 + count('|')
  int64_t n_listed;    // the names of all segments
};

// The annotation p[0 .. n).  For every name, in order, v.name(j, c, beg, len): the j-th listed
// name of the annotation stands in segment c and is p[beg .. beg + len).  After the names of
// segment c, v.segment(c, names): the segment lists `names` names.
template <class Visitor>
PAS_AF_HD inline AnnotationCounts annotation_walk(const char* p, int64_t n, Visitor&& v) {
  int64_t seg = 0, listed = 0, in_seg = 0;
  int64_t seg_beg = 0, name_beg = 0;
  for (int64_t i = 0; i <= n; ++i) {
    const bool end = i == n || p[i] == '|';  // the end of the bytes closes the last segment
    if (!end && p[i] != ',') continue;
    if (!end || i > seg_beg) {  // a ',' always ends a name; a segment's end only if not empty
      v.name(listed, seg, name_beg, i - name_beg);
      ++listed;
      ++in_seg;
    }
    name_beg = i + 1;
    if (end) {
      v.segment(seg, in_seg);
      ++seg;
      in_seg = 0;
      seg_beg = i + 1;
    }
  }
  return AnnotationCounts{seg, listed};
}

// The visitor of a pass that only counts.
struct AnnotationCountOnly {
  PAS_AF_HD void name(int64_t, int64_t, int64_t, int64_t) {}
  PAS_AF_HD void segment(int64_t, int64_t) {}
};

PAS_AF_HD inline AnnotationCounts annotation_counts(const char* p, int64_t n) {
  return annotation_walk(p, n, AnnotationCountOnly{});
}

// ---- rendering ----
//
// A bind is n_containers segments; segment c lists items(c) items, item i being `count` repeats
// of the name `rank` of the node's row.  The counts form has one item per card slot (count =
// counts[c][k], rank = k), the ranks form one item per listed card (count = 1).  Every repeat is
// its name and one separator byte, ',', so an item of `count` repeats of a name of n bytes is
// count * (n + 1) bytes and its byte j is j % (n + 1) == n ? ',' : name[j % (n + 1)].  The
// separator that ends a segment becomes the '|' before the next one, or is dropped after the
// last; a segment without a repeat is that '|' alone.  So with S the item bytes of a segment,
//   bytes of a segment = max(S, 1) - (1 if it is the last one)
// and no byte depends on another segment than its own.  Names are opaque: the empty name
// renders as itself ("a,,b").
//
// Both routines are written for a group of Lanes::kWidth lanes in lockstep, each taking every
// kWidth-th item of a segment, with the group's sums and prefixes behind `Lanes`:
//   int lane()                            this lane, below kWidth
//   int64_t sum(int64_t v)                saturating (render_sat_add) sum over the lanes
//   bool any(bool p)
//   int64_t scan(int64_t v, int64_t* t)   exclusive prefix of v over the lanes, *t the total
//   uint64_t ballot(bool p)
//   T from(T v, int t)                    lane t's v
// Every lane of the group makes the same calls.  Src is the bind:
//   int64_t items(int32_t c)
//   void item(int64_t flat, int64_t i, int64_t* count, int64_t* rank)   item i of its segment,
//                                         the flat-th of the bind; a negative count marks an
//                                         item the source cannot read
// and Names the node's row: int64_t len(int64_t rank), const char* ptr(int64_t rank), read only
// for 0 <= rank < L.

// Item bytes are summed up to this value and stay there: a segment of INT32_MAX + 1 item bytes
// may still render to INT32_MAX bytes (its last separator is dropped), one of INT32_MAX + 2 or
// more never does.
constexpr int64_t kRenderSat = (int64_t)INT32_MAX + 2;

PAS_AF_HD inline int64_t render_sat_add(int64_t a, int64_t b) {  // a, b in [0, kRenderSat]
  return a + b > kRenderSat ? kRenderSat : a + b;
}

// count >= 0 repeats of a name of n >= 0 bytes
PAS_AF_HD inline int64_t render_item_len(int64_t count, int64_t n) {
  if (count == 0) return 0;
  const int64_t unit = n >= kRenderSat ? kRenderSat : n + 1;
  return count > kRenderSat / unit ? kRenderSat : count * unit;
}

PAS_AF_HD inline int64_t render_segment_len(int64_t item_bytes, bool last) {
  if (item_bytes >= kRenderSat) return kRenderSat;
  return (item_bytes > 0 ? item_bytes : 1) - (last ? 1 : 0);
}

// Byte j of an item of `count` repeats (j < count * (n + 1) <= INT32_MAX)
PAS_AF_HD inline char render_item_byte(const char* name, uint32_t n, uint32_t count, uint32_t j) {
  const uint32_t r = count == 1 ? j : j % (n + 1);
  return r == n ? ',' : name[r];
}

// The one-lane group of the host entry point.
struct OneLane {
  static constexpr int kWidth = 1;
  int lane() const { return 0; }
  int64_t sum(int64_t v) const { return v; }
  bool any(bool p) const { return p; }
  int64_t scan(int64_t v, int64_t* total) const {
    *total = v;
    return 0;
  }
  uint64_t ballot(bool p) const { return p ? 1 : 0; }
  template <class T>
  T from(T v, int) const {
    return v;
  }
};

// The status of a bind of nc segments on a node of L label cards and, in *len_out, its rendered
// length (0 unless the status is PAS_GAS_OK):
//   PAS_GAS_ERR_INPUT      a negative count, or a repeat of a rank outside [0, L);
//   PAS_GAS_ERR_OVERFLOW   otherwise, a length past INT32_MAX (the sums saturate, so counts up to
//                          INT64_MAX are ordinary input).
template <class Lanes, class Src, class Names>
PAS_AF_HD inline int32_t annotation_render_len(const Lanes& w, int32_t nc, int64_t L,
                                               const Src& src, const Names& names,
                                               int64_t* len_out) {
  bool bad = false;
  int64_t total = 0, flat = 0;
  for (int32_t c = 0; c < nc; ++c) {
    const int64_t m = src.items(c);
    int64_t seg = 0;
    for (int64_t i = w.lane(); i < m; i += Lanes::kWidth) {
      int64_t count, rank;
      src.item(flat + i, i, &count, &rank);
      if (count < 0 || (count > 0 && (rank < 0 || rank >= L)))
        bad = true;
      else if (count > 0)
        seg = render_sat_add(seg, render_item_len(count, names.len(rank)));
    }
    total = render_sat_add(total, render_segment_len(w.sum(seg), c == nc - 1));
    flat += m;
  }
  bad = w.any(bad);
  const int32_t status =
      bad ? PAS_GAS_ERR_INPUT : total > INT32_MAX ? PAS_GAS_ERR_OVERFLOW : PAS_GAS_OK;
  *len_out = status == PAS_GAS_OK ? total : 0;
  return status;
}

// The bytes of a bind that annotation_render_len found PAS_GAS_OK, into out[0 .. its length);
// nothing is written at or past out[cap] and no name outside [0, L) is read.  Per segment: the
// item bytes S, then the items 64 (one) at a time, their starts from a prefix over the group
// plus what the items before left; the
// lanes then stride over the bytes of each item that has any, so an item of many repeats or a
// long name is stored by all lanes, neighbouring lanes to neighbouring bytes.
template <class Lanes, class Src, class Names>
PAS_AF_HD inline void annotation_render_write(const Lanes& w, int32_t nc, int64_t L,
                                              const Src& src, const Names& names, char* out,
                                              int64_t cap) {
  constexpr int W = Lanes::kWidth;
  int64_t base = 0, flat = 0;
  for (int32_t c = 0; c < nc; ++c) {
    const bool last = c == nc - 1;
    const int64_t m = src.items(c);
    int64_t seg = 0;
    for (int64_t i = w.lane(); i < m; i += W) {
      int64_t count, rank;
      src.item(flat + i, i, &count, &rank);
      if (count > 0 && rank >= 0 && rank < L) seg += render_item_len(count, names.len(rank));
    }
    const int64_t S = w.sum(seg);
    if (S == 0 && !last && w.lane() == 0 && base < cap) out[base] = '|';
    int64_t done = 0;  // the item bytes of the segment's items so far
    for (int64_t i0 = 0; i0 < m; i0 += W) {
      const int64_t i = i0 + w.lane();
      int64_t count = 0, rank = 0, n = 0, r = 0;
      const char* p = nullptr;
      if (i < m) src.item(flat + i, i, &count, &rank);
      if (count > 0 && rank >= 0 && rank < L) {
        n = names.len(rank);
        p = names.ptr(rank);
        r = count * (n + 1);
      }
      int64_t sum;
      const int64_t start = done + w.scan(r, &sum);
      for (uint64_t live = w.ballot(r > 0); live; live &= live - 1) {
        const int t = __builtin_ctzll(live);
        const int64_t start_t = w.from(start, t), r_t = w.from(r, t);
        const uint32_t n_t = (uint32_t)w.from(n, t), count_t = (uint32_t)w.from(count, t);
        const char* p_t = w.from(p, t);
        for (int64_t j = w.lane(); j < r_t; j += W) {
          const int64_t at = start_t + j;  // in the segment
          if (base + at >= cap) continue;
          if (at == S - 1) {
            if (!last) out[base + at] = '|';
          } else {
            out[base + at] = render_item_byte(p_t, n_t, count_t, (uint32_t)j);
          }
        }
      }
      done += sum;
    }
    base += render_segment_len(S, last);
    flat += m;
  }
}

}  // namespace pas
