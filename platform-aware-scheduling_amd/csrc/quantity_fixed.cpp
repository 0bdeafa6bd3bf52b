// quantity_fixed.cpp — the fixed-width ParseQuantity of quantity_fixed.h on the host, for one
// literal given as a byte span (no NUL terminator needed).  The device runs the same code per
// literal (tas_ingest.hip).
#include "quantity_fixed.h"

extern "C" {

int pas_quantity_parse_fixed(const char* bytes, int64_t len, int64_t* whole, uint32_t* nano,
                             int32_t* decimals, int32_t* fit) {
  const pas::QuantityFixed r = pas::parse_quantity_fixed(bytes, len);
  if (whole) *whole = r.whole;
  if (nano) *nano = r.nano;
  if (decimals) *decimals = r.decimals;
  if (fit) *fit = r.fit;
  return r.status;
}

int pas_quantity_as_int64_fixed(const char* bytes, int64_t len, int64_t* out) {
  const pas::QuantityFixed r = pas::parse_quantity_fixed(bytes, len);
  if (out) *out = r.as_int64;
  return r.status;
}

}  // extern "C"
