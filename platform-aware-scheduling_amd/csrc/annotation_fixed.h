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
#pragma once

#include <cstdint>

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

}  // namespace pas
