// gas_annotation.cpp — the annotation grammar of annotation_fixed.h on the host, for one
// annotation given as a byte span (no NUL terminator needed).  The device runs the same walk
// per pod event (gas_annotations.hip).  The render of one annotation from counts and a row of
// names is the other direction, which the device runs per bind (gas_render.hip).
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

// One bind in the counts form: every segment has an item per card slot
struct HostCounts {
  const int64_t* counts;
  int32_t k;
  int64_t items(int32_t) const { return k; }
  void item(int64_t flat, int64_t i, int64_t* count, int64_t* rank) const {
    *count = counts[flat];
    *rank = i;
  }
};

struct HostNames {
  const int64_t* off;
  const char* bytes;
  int64_t len(int64_t rank) const { return off[rank + 1] - off[rank]; }
  const char* ptr(int64_t rank) const { return bytes + off[rank]; }
};

}  // namespace

extern "C" {

int pas_gas_annotation_render(int32_t n_containers, int32_t k, int32_t n_cards,
                              const int64_t* counts, const int64_t* name_off,
                              const char* name_bytes, int32_t* status_out, char* bytes_out,
                              int64_t cap, int64_t* n_bytes_out) {
  if (n_containers < 0 || k < 0 || cap < 0 || !status_out || !n_bytes_out ||
      (cap > 0 && !bytes_out) || (n_containers > 0 && k > 0 && !counts) || (k > 0 && !name_off))
    return PAS_EINVAL;
  if (k > 0 && name_off[0] != 0) return PAS_EINVAL;
  for (int32_t c = 0; c < k; ++c)
    if (name_off[c + 1] < name_off[c]) return PAS_EINVAL;
  if (k > 0 && name_off[k] > 0 && !name_bytes) return PAS_EINVAL;
  const int64_t L = n_cards < 0 ? 0 : n_cards > k ? k : n_cards;
  const pas::OneLane w;
  const HostCounts src{counts, k};
  const HostNames names{name_off, name_bytes};
  *status_out = pas::annotation_render_len(w, n_containers, L, src, names, n_bytes_out);
  if (*n_bytes_out > cap) return PAS_ECAPACITY;
  if (*status_out == PAS_GAS_OK)
    pas::annotation_render_write(w, n_containers, L, src, names, bytes_out, cap);
  return PAS_OK;
}

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
