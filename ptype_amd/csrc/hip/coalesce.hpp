// Send coalescing (coalesce.hip, ops/coalesce.py): duplicate calls of a pure method
// in one batch are sent once -- Go's singleflight on the batch path.
//
// A message's key is (actor id as u32, method as u16, a0, a1, a2); a missing a1 / a2
// column counts as 0.  Two messages of a PURE method with equal keys get the same
// reply, so only the one with the lowest index (the group's leader) travels and every
// other member copies its (value, status).  A message of any other method is its own
// leader.  ops/records.py PURE_METHODS and ops/coalesce.py key_hash mirror this file.
#pragma once
#include <stdint.h>

#include "common.hpp"

namespace ptype {

// Reply = f(a0, a1, a2), status = f(actor exists): handlers.hpp.
__host__ __device__ __forceinline__ bool method_pure(uint32_t m) {
  return m == kCalculatorMultiply || m == kPrimeCheck || m == kEcho;
}

// The hash of a key (never its identity: the kernels compare all five fields).  Chained,
// so swapped arguments -- Multiply(a, b) and Multiply(b, a) -- land in different slots.
__host__ __device__ __forceinline__ uint64_t coalesce_hash(uint32_t actor, uint32_t method16, int64_t a0, int64_t a1,
                                                           int64_t a2) {
  uint64_t h = mix64((uint64_t)actor | (uint64_t)(method16 & 0xffffu) << 32);
  h = mix64(h ^ (uint64_t)a0);
  h = mix64(h ^ (uint64_t)a1);
  return mix64(h ^ (uint64_t)a2);
}

// The grouping table: u32 slots holding message index + 1 (0 = empty), a power of two of
// at least 2 M slots, home slot = hash & (slots - 1), linear probing.
constexpr int kCoalesceMinLog2 = 4;
constexpr int kCoalesceMaxLog2 = 31;

}  // namespace ptype
