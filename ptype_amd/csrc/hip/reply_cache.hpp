// Reply cache (reply_cache.hip, ops/reply_cache.py): pure calls answered from HBM
// across the Sends of one runtime -- the cache a Go service keeps next to singleflight.
//
// The key is coalescing's (coalesce.hpp): (actor id as u32, method as u16, a0, a1, a2),
// a missing a1 / a2 column counting as 0.  Only a STATUS_OK reply of a method_pure()
// method is ever stored or served.  The table is direct-mapped: 1 << n entries, slot =
// coalesce_hash(key) & mask, the hash only picks the slot and a hit compares all five
// fields.  ops/reply_cache.py ReplyCacheRef mirrors this file.
#pragma once
#include <stdint.h>

#include "coalesce.hpp"

namespace ptype {

// One aligned 64-B line per entry.
struct alignas(64) ReplyCacheEntry {
  uint64_t k0;     // actor | method << 32
  int64_t a0, a1, a2;
  int64_t value;
  uint64_t claim;  // the lowest (0xFFFFFFFF - seq) << 32 | row that ever asked for this slot
  uint32_t epoch;  // valid iff == the cache's epoch (a cleared entry: 0, claim all ones)
  uint32_t pad[3];
};
static_assert(sizeof(ReplyCacheEntry) == 64, "ReplyCacheEntry must be one 64-B line");

constexpr int kReplyCacheMinLog2 = 4;
constexpr int kReplyCacheMaxLog2 = 26;

constexpr int kReplyCachePending = kPending;  // what the lookup leaves in st[i] for a miss and a non-pure message

__host__ __device__ __forceinline__ uint64_t reply_cache_k0(uint32_t actor, uint32_t method16) {
  return (uint64_t)actor | (uint64_t)(method16 & 0xffffu) << 32;
}

// A newer Send (higher seq) claims with a smaller word than any older one, and within a
// Send the lowest row does: one atomicMin decides a slot's writer, with no per-Send reset.
__host__ __device__ __forceinline__ uint64_t reply_cache_claim(uint32_t seq, uint32_t row) {
  return (uint64_t)(0xffffffffu - seq) << 32 | row;
}

}  // namespace ptype
