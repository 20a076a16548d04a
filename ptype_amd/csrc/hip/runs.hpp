// Streaming tiles and run combining shared by the per-actor Send wrappers (breaker.hip,
// limit.hip): a column of M int32 is read once with 16-B loads, runs of equal adjacent keys
// are combined per thread by compare and per wave by ballot and a segmented shuffle scan
// (gather.hip's scheme), and each run reaches memory once.
//
// Tile layout as in gather.hip: 256 threads x kBrRows rows; row j of wave w, lane l covers
// the messages  tile * kBrTile + (j * 4 + w) * 256 + l * 4 + {0, 1, 2, 3}: one dwordx4 per
// lane.  A column that is not 16-byte aligned takes the same layout with scalar loads.
#pragma once
#include <stdint.h>

#include "common.hpp"

namespace ptype {

constexpr int kBrThreads = 256;
constexpr int kBrWaves = kBrThreads / kWave;
constexpr int kBrRows = 2;                             // 4-message rows per thread and tile
constexpr int kBrTile = kBrThreads * kBrRows * 4;      // 2048 messages
constexpr int kBrBlocks = 2048;                        // blocks of a streaming launch (they stride over the tiles)
constexpr uint32_t kBrNoActor = 0xffffffffu;           // a row past M (never < n)

__device__ __forceinline__ int64_t br_elem(int64_t tile, int j, unsigned wave, unsigned lane) {
  return tile * kBrTile + (int64_t)(j * kBrWaves + (int)wave) * (kWave * 4) + lane * 4;
}

// Four consecutive elements at index i (a multiple of 4); elements at or past M read as `pad`.
template <bool ALIGNED>
__device__ __forceinline__ void br_load4(const int* __restrict__ p, int64_t i, int64_t M, int pad, int (&o)[4]) {
  if (ALIGNED && i + 4 <= M) {
    const int4 v = *reinterpret_cast<const int4*>(p + i);
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = i + c < M ? p[i + c] : pad;
}

// Every lane of the wave calls this together.  The lanes with `fresh` (their atomic took
// their entry from 0) reserve their places in touched[] with one atomic on *count and write
// a there; cap is the list's length.
__device__ __forceinline__ void br_append(bool fresh, uint32_t a, unsigned long long* __restrict__ count,
                                          uint32_t* __restrict__ touched, uint32_t cap) {
  const uint64_t m = __ballot(fresh);
  if (!m) return;  // (wave-uniform)
  const int leader = __ffsll((long long)m) - 1;
  unsigned long long base = 0;
  if ((int)lane_id() == leader) base = atomicAdd(count, (unsigned long long)__popcll(m));
  base = __shfl(base, leader, kWave);
  if (fresh) {
    const unsigned long long pos = base + mbcnt64(m);
    if (pos < cap) touched[pos] = a;  // (an entry is appended once per Send: pos < cap always)
  }
}

// Every lane of the wave calls this together with the keys of its four consecutive rows
// (g[c] < 0: no key).  Each run of equal adjacent keys within the wave's 256 rows is handed
// to emit(key, rows) once, by one lane; emit is called by every lane of the wave together
// (key < 0: nothing to add), four times per call.
template <class Emit>
__device__ __forceinline__ void br_combine_runs(const int (&g)[4], unsigned lane, Emit&& emit) {
  // the thread's four rows: head run, tail run, runs in between added at once
  int cur_g = g[0], head_g = g[0];
  uint32_t cur_n = g[0] >= 0, head_n = 0;
  bool single = true;
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    int flush_g = -1;
    uint32_t flush_n = 0;
    if (g[c] == cur_g) {
      cur_n += g[c] >= 0;
    } else {
      if (single)
        head_g = cur_g, head_n = cur_n, single = false;
      else
        flush_g = cur_g, flush_n = cur_n;
      cur_g = g[c], cur_n = g[c] >= 0;
    }
    if (c >= 2) emit(flush_g, flush_n);
  }
  const int tail_g = cur_g;
  if (single) head_g = tail_g;

  // across the wave: the items are the tails; an item starts a run unless the lane is
  // one run that continues the previous lane's tail
  const int prev_tail_g = __shfl_up(tail_g, 1, kWave);
  const int next_head_g = __shfl_down(head_g, 1, kWave);
  const bool starts = lane == 0 || !single || tail_g != prev_tail_g;
  const uint64_t heads = __ballot(starts);
  if (heads != ~0ull) {  // (wave-uniform)
    const unsigned first = 63u - (unsigned)__clzll((long long)(heads & ((2ull << lane) - 1ull)));
#pragma unroll
    for (unsigned o = 1; o < (unsigned)kWave; o <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)cur_n, o, kWave);
      if (lane >= first + o) cur_n += up;
    }
  }
  const uint32_t prev_n = (uint32_t)__shfl_up((int)cur_n, 1, kWave);
  if (!single && lane > 0 && head_g == prev_tail_g) head_n += prev_n;
  emit(single ? -1 : head_g, head_n);
  const bool last = lane == (unsigned)kWave - 1 || next_head_g != tail_g;
  emit(last ? tail_g : -1, cur_n);
}

}  // namespace ptype
