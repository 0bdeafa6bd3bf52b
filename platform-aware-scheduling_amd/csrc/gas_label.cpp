// gas_label.cpp — the cards-label grammar of label_fixed.h on the host, for one label given as a
// byte span (no NUL terminator needed).  The device runs the same routines per node event
// (gas_node_strings.hip).
#include "label_fixed.h"
#include "pas.h"

extern "C" {

int pas_gas_label_parse(const char* bytes, int64_t len, int64_t* n_pieces, int32_t* n_cards,
                        int64_t* name_span, int64_t cap) {
  if (len < 0 || (len > 0 && !bytes) || cap < 0 || (cap > 0 && !name_span)) return PAS_EINVAL;
  if (n_pieces) *n_pieces = pas::label_pieces(bytes, len);
  int32_t cards = 0;
  int64_t b = 0, l = 0;
  while (cards <= PAS_GAS_MAX_CARDS && pas::label_next(bytes, len, cards > 0, b, l, &b, &l)) {
    if (cards < cap) {
      name_span[2 * cards] = b;
      name_span[2 * cards + 1] = l;
    }
    ++cards;
  }
  if (n_cards) *n_cards = cards;
  return PAS_OK;
}

}  // extern "C"
