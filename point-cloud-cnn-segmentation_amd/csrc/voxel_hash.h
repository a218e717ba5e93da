// Device-side lookup in the occupied-voxel hash table (built by sparse.hip's pcs_voxel_hash_build),
// shared by every kernel that turns a voxel key into a row: open addressing over a power-of-two
// capacity, slot = mix64(key) & (cap - 1), linear probing, all ones = empty.
#pragma once
#include "common.h"

namespace pcs_hash {

constexpr uint64_t EMPTY = ~0ull;

PCS_DEV uint64_t mix64(uint64_t k) {   // splitmix64 finaliser
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

PCS_DEV int32_t hash_find(const uint64_t *__restrict__ tk, const int32_t *__restrict__ tv, uint64_t mask, uint64_t k) {
  uint64_t h = mix64(k) & mask;
  for (uint64_t probe = 0; probe <= mask; ++probe) {
    const uint64_t s = tk[h];
    if (s == k) return tv[h];
    if (s == EMPTY) return -1;
    h = (h + 1) & mask;
  }
  return -1;
}

}  // namespace pcs_hash
