// Circuit breaker (breaker.hip, ops/breaker.py): an actor that failed `threshold` times
// in a row is not sent to for `cooldown` guarded Sends; then one probe message decides
// whether it takes traffic again (sony/gobreaker, Akka's CircuitBreaker, per actor and on
// the batch path).  ops/breaker.py BreakerRef mirrors this file.
//
// The key is the logical actor id as u32; the table is dense, n entries.  An id >= n is
// never guarded: it always passes, is never observed and is counted in `oob` by an admit
// pass.  Time is counted in guarded Sends (`now`, 1 .. 2^31 - 1).
//
// State, one u64 per actor:
//   bit 63      open
//   bits 32..62 until: the first tick at which a probe may pass
//   bits 0..31  fails: consecutive failed messages, saturating
// 0 is "closed, clean"; half-open is not stored, it is open && now >= until.
//
// Side tables, n entries each:
//   probe[a]    u64, all ones at rest: lowered (atomicMin) to breaker_claim(now, row) by the
//               rows that address a half-open actor; its owner is the Send's probe
//   obs[a]      u64, 0 between Sends: the Send's failed rows of a (low bits) and
//               kBreakerObsOk once an OK row of a was seen while word or obs was non-zero
//   touched[]   u32: the actors whose obs left 0 in this Send, kBreakerTouched of them
// Counter words (u64): see BreakerCounter.  The step kernel zeroes obs[a] of every touched
// actor and its last block re-arms kBreakerTouched, so no Send starts with a fill.
#pragma once
#include <stdint.h>

#include "common.hpp"

namespace ptype {

constexpr uint64_t kBreakerOpen = 1ull << 63;
constexpr uint64_t kBreakerObsOk = 1ull << 63;
constexpr uint32_t kBreakerMaxTick = 0x7fffffffu;
constexpr int64_t kBreakerMaxActors = 1ll << 28;

constexpr int kBreakerPending = kPending;  // what the admit pass leaves in st[i] for a row that travels

enum BreakerCounter {
  kBreakerNOpen = 0,    // words with bit 63 set
  kBreakerNDirty = 1,   // non-zero words
  kBreakerTrips = 2,    // closed -> open
  kBreakerCloses = 3,   // open -> closed by a probe that answered STATUS_OK
  kBreakerOob = 4,      // rows with an id >= n met by an admit pass
  kBreakerTouched = 5,  // entries of touched[] (0 between Sends)
  kBreakerCounters = 8,
};
// u64 words of the counter block: the counters, then the step kernel's last-block ticket
// (kTicketWords u32, common.hpp)
constexpr int kBreakerCtrWords = kBreakerCounters + 33;

__host__ __device__ __forceinline__ bool breaker_is_open(uint64_t w) { return (w >> 63) != 0; }
__host__ __device__ __forceinline__ uint32_t breaker_until(uint64_t w) { return (uint32_t)(w >> 32) & 0x7fffffffu; }
__host__ __device__ __forceinline__ uint32_t breaker_fails(uint64_t w) { return (uint32_t)w; }
__host__ __device__ __forceinline__ uint64_t breaker_open_word(uint32_t until, uint32_t fails) {
  return kBreakerOpen | (uint64_t)(until & 0x7fffffffu) << 32 | fails;
}
// now + cooldown, held at the last tick (the breaker restarts before the tick passes it)
__host__ __device__ __forceinline__ uint32_t breaker_deadline(uint32_t now, uint32_t cooldown) {
  const uint64_t t = (uint64_t)now + cooldown;
  return t > kBreakerMaxTick ? kBreakerMaxTick : (uint32_t)t;
}
// A later Send claims with a smaller word than any earlier one, and within a Send the
// lowest row does: one atomicMin names the probe, with no per-Send reset.
__host__ __device__ __forceinline__ uint64_t breaker_claim(uint32_t now, uint32_t row) {
  return (uint64_t)(0xffffffffu - now) << 32 | row;
}

}  // namespace ptype
