// gas_annotation.cpp — the annotation grammar of annotation_fixed.h on the host, for one
// annotation given as a byte span (no NUL terminator needed).  The device runs the same walk
// per pod event (gas_annotations.hip).
#include "annotation_fixed.h"
#include "pas.h"

namespace {

struct HostVisitor {
  int32_t max_containers;
  int32_t* cards_per_container;
  int64_t* name_span;
  int64_t cap;
  void name(int64_t j, int64_t, int64_t beg, int64_t len) {
    if (j < cap) {
      name_span[2 * j] = beg;
      name_span[2 * j + 1] = len;
    }
  }
  void segment(int64_t c, int64_t names) {
    if (c < max_containers)
      cards_per_container[c] = names > INT32_MAX ? INT32_MAX : (int32_t)names;
  }
};

}  // namespace

extern "C" {

int pas_gas_annotation_parse(const char* bytes, int64_t len, int32_t max_containers,
                             int64_t* n_segments, int32_t* cards_per_container,
                             int64_t* n_listed, int64_t* name_span, int64_t cap) {
  if (len < 0 || (len > 0 && !bytes) || max_containers < 0 || cap < 0 ||
      (max_containers > 0 && !cards_per_container) || (cap > 0 && !name_span))
    return PAS_EINVAL;
  const pas::AnnotationCounts r = pas::annotation_walk(
      bytes, len, HostVisitor{max_containers, cards_per_container, name_span, cap});
  if (n_segments) *n_segments = r.n_segments;
  if (n_listed) *n_listed = r.n_listed;
  return PAS_OK;
}

}  // extern "C"
