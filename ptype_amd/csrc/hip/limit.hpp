// Rate limiter (limit.hip, ops/limit.py): a token bucket per actor on the batch path
// (golang.org/x/time/rate, Akka's throttle): an actor gains `rate` tokens per limited Send,
// holds at most `burst`, and every message costs one.  Of an actor whose rows exceed its
// tokens the first ones in message order travel, the others are answered
// (0, kStatusThrottled) and not sent.  ops/limit.py LimiterRef mirrors this file.
//
// The key is the logical actor id as u32; the table is dense, n entries.  An id >= n is
// never limited: it always passes and is counted in `oob` by the demand pass of every
// limited Send.  Time is counted in limited Sends (`now`, 1 .. 2^31 - 1).
//
// State, one u64 per actor:
//   bit 63      0
//   bits 32..62 last: the tick of the last update
//   bits 0..31  spent: burst - tokens at that tick
// and 0 whenever spent == 0: a zero-filled table is every bucket full.
//
// Side tables:
//   demand[a]    u32[n], 0 between Sends: the Send's rows of a; after the step launch 0, or
//                kLimitHot | h for an actor over its quota (h: its hot slot)
//   touched[]    u32[n]: the actors whose demand left 0 in this Send, kLimitTouched of them
//   hot_actor[h] u32[n]: the actor of hot slot h, kLimitOver of them
//   rem[h]       u32[n]: the occurrences still to skip in the radix select (starts at q)
//   prefix[h]    u32[n]: the high digits of the threshold row found so far; after the last
//                level the row of occurrence number q of the actor: rows below it travel
//   slot[i]      i32[M]: the hot slot of row i's actor, or -1
//   bins         u32[over << kLimitDigit], 0 between Sends: the level's counts per hot slot
//   busy         u32[2 * kLimitBusyCap]: two lists of actors with limit_busy_rows(M) or more rows in
//                a Send, a hint from one Send to the next (limit.hip LimitCache); the Send at
//                tick t fills list t & 1 and reads the other
// Counter words (u64): see LimitCounter.  The step kernel zeroes demand[a] of every actor
// within its quota and re-arms kLimitTouched, the resolve kernel zeroes the bins, the rearm
// kernel zeroes demand[a] of the hot actors and kLimitOver: no Send starts with a fill.
#pragma once
#include <stdint.h>

#include "common.hpp"

namespace ptype {

constexpr uint32_t kLimitMaxTick = 0x7fffffffu;
constexpr int64_t kLimitMaxActors = 1ll << 28;
constexpr uint32_t kLimitHot = 1u << 31;  // demand[a] after the step launch: a is over its quota
constexpr int kLimitDigit = 4;            // bits of the row index resolved per level of the radix select
constexpr int kLimitBins = 1 << kLimitDigit;
// An actor with limit_busy_rows(M) or more rows in a Send is named to the next one: 1 / 1024 of
// the batch and at least 1024 rows, so that a list of kLimitBusyCap entries never overflows.
constexpr uint32_t kLimitBusyCap = 1024;
__host__ __device__ __forceinline__ uint32_t limit_busy_rows(int64_t M) {
  const int64_t share = M >> 10;
  return (uint32_t)(share > 1024 ? share : 1024);
}
// hot slots one Send may have: their bins are indexed by an int (slot << kLimitDigit | digit)
constexpr int64_t kLimitMaxHot = (1ll << 31 >> kLimitDigit) - 1;

constexpr int kLimitPending = kPending;  // what the admit pass leaves in st[i] for a row that travels

enum LimitCounter {
  kLimitThrottled = 0,  // rows answered kStatusThrottled, cumulative
  kLimitOob = 1,        // rows with an id >= n, cumulative
  kLimitOver = 2,       // actors over their quota in this Send (0 between Sends)
  kLimitTouched = 3,    // entries of touched[] (0 between Sends)
  kLimitBusyN = 4,      // two words: entries of the two busy lists (the one the Send at tick t fills is t & 1)
  kLimitCounters = 8,
};
// u64 words of the counter block: the counters, then the step kernel's last-block ticket
// (kTicketWords u32, common.hpp)
constexpr int kLimitCtrWords = kLimitCounters + 33;

__host__ __device__ __forceinline__ uint32_t limit_spent(uint64_t w) { return (uint32_t)w; }
__host__ __device__ __forceinline__ uint32_t limit_last(uint64_t w) { return (uint32_t)(w >> 32) & 0x7fffffffu; }
// spent after the refill of the ticks since the word was written (a zero word: a full bucket)
__host__ __device__ __forceinline__ uint32_t limit_refilled(uint64_t w, uint32_t now, uint32_t rate) {
  if (!w) return 0u;
  uint64_t refill = (uint64_t)(now - limit_last(w)) * rate;
  if (refill > 0xffffffffull) refill = 0xffffffffull;
  const uint32_t spent = limit_spent(w);
  return spent > refill ? spent - (uint32_t)refill : 0u;
}
__host__ __device__ __forceinline__ uint64_t limit_word(uint32_t now, uint32_t spent) {
  return spent ? (uint64_t)now << 32 | spent : 0ull;
}
// levels of the radix select over the row indices 0 .. M - 1
__host__ __device__ __forceinline__ int limit_levels(int64_t M) {
  int bits = 0;
  for (int64_t v = M - 1; v > 0; v >>= 1) ++bits;
  const int L = (bits + kLimitDigit - 1) / kLimitDigit;
  return L < 1 ? 1 : L;
}

}  // namespace ptype
