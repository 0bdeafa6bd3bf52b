// name_hash.h — the one hash of node names, on the host and on the device.
//
// FNV-1a over the bytes (every byte value is ordinary, 0 and >= 0x80 included), then the 64-bit
// finalizer of MurmurHash3 so that both halves of the word are well mixed.  The name table
// (name_table.hip) reads the word as
//   home bucket   h & (buckets - 1)   the low bits (buckets is a power of two, at most 2^32)
//   tag           h >> 32             the high 32 bits, stored in the table word beside the slot
// so the two never overlap.  Equal tags only let a probe go on to the byte compare against the
// pool: a hit is never decided by hash bits.  pas_name_hash (pas.h) exports the function.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PAS_HD __host__ __device__
#else
#define PAS_HD
#endif

namespace pas {

PAS_HD inline uint64_t name_hash(const char* bytes, int64_t len) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (int64_t i = 0; i < len; ++i) {
    h ^= (uint64_t)(uint8_t)bytes[i];
    h *= 0x100000001b3ull;
  }
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

PAS_HD inline uint32_t name_tag(uint64_t h) { return (uint32_t)(h >> 32); }

}  // namespace pas
