// Rate limiter kernels (`DeviceRuntime.send(limit=True)`, ops/limit.py; limit.hpp has the
// state word, the side tables and the counters).  A limited Send runs at tick `now`; all
// launches are on the Send's stream and launch boundaries are the only ordering (as in
// breaker.hip).  No block waits on another, nothing is sorted.
//
// Every limited Send, before the inner Send:
//   limit_demand_kernel   streams actor[M]; each run of equal adjacent ids (combined per thread
//                         and per wave, runs.hpp) adds its length to demand[a] once; the adder
//                         that saw 0 appends a to touched[] (one reservation per wave
//                         instruction); rows with an id >= n counted, one atomic per block
//   limit_step_kernel     grid-stride over touched[0 .. n_touched): the refill, q = min(d,
//                         avail), the new word.  d <= avail: demand[a] = 0.  Else a hot slot h
//                         is reserved from `over` (one atomic per wave instruction),
//                         hot_actor[h] = a, rem[h] = q, prefix[h] = 0, demand[a] = kLimitHot | h
//                         and d - q joins `throttled` (folded per wave); the last block
//                         re-arms n_touched
// then the host reads `over`.  Only when over > 0 the message-order cut runs: per hot actor
// a radix select of the row of its occurrence number q, kLimitDigit bits of the row index
// per level, L = limit_levels(M) levels, most significant digit first:
//   limit_slots_kernel    slot[i] = the hot slot of actor[i] or -1, and the level-0 count
//   limit_count_kernel    levels 1 .. L - 1, over slot[]: at shift s a hot row i counts into
//                         bins[h][(i >> s) & 15] iff (i >> (s + kLimitDigit)) == prefix[h]
//   limit_resolve_kernel  after each count, one thread per hot slot: the smallest digit whose
//                         cumulative count exceeds rem[h] joins prefix[h], the count below it
//                         leaves rem[h], the bins are zeroed
//   limit_admit_kernel    st[i] = kLimitPending if slot[i] < 0 or i < prefix[slot[i]], else
//                         kStatusThrottled; val[i] = 0
//   limit_rearm_kernel    demand[hot_actor[h]] = 0 for every hot slot, then over = 0
//   limit_clear_kernel    every word and demand 0, over / n_touched 0 (reset, tick restart)
//
// Busy keys are counted in LDS first and reach memory once per block: the demand launch keeps
// a small cache of busy actors (LimitCache: the ones the last Send named, and the ones whose
// memory atomic returns a large count), the slots and count launches one of all their keys.
// The counts combine runs of rows that share (slot, digit): at level 0 a digit covers
// 16^(L-1) rows, so a hot actor's rows of one wave are one atomic; at the later levels only
// the rows under the prefix count, at most 16^(L-l) per hot actor.  demand[a] is only
// written by atomics and by the one step thread that owns a; bins by atomics and by the one
// resolve thread that owns the slot.
//
// Tile layout, loads, run combining and the touched[] reservation: runs.hpp.
#include "limit.hpp"
#include "common.hpp"
#include "runs.hpp"

namespace ptype {

constexpr int kLimitStepBlocks = 64;
constexpr int kLimitDigitMask = kLimitBins - 1;
constexpr int kLimitCacheBits = 11;
constexpr int kLimitCacheSlots = 1 << kLimitCacheBits;
constexpr uint32_t kLimitBusy = 256;  // a count in memory from which a key is kept in the blocks' caches

// A block's direct-mapped cache of (key, rows) in LDS in front of a count table in memory,
// for busy keys only.  Same-address atomics serialise at the memory side (about 11 ns each,
// measured: the 840 K runs of one actor's rows, 10 % of 8 Mi, took 9.5 ms).  So a key whose
// memory atomic returned kLimitBusy or more claims its slot in the block's cache, and the
// block's later runs of it are added in LDS and flushed once; a busy key -- a Zipf head, the
// one hot actor -- then reaches memory a few times per block instead of once per run.  Every
// other key pays one LDS read.  A slot is never re-assigned within a launch.  A block is done
// soon after its first atomics return, so the demand launch is also told the busy actors of the
// last Send (limit.hpp `busy`): they are cached from the first row on.
struct LimitCache {
  int key[kLimitCacheSlots];  // -1: empty
  uint32_t rows[kLimitCacheSlots];
};

__device__ __forceinline__ void limit_cache_init(LimitCache& c) {
  for (int s = threadIdx.x; s < kLimitCacheSlots; s += kBrThreads) c.key[s] = -1, c.rows[s] = 0u;
  __syncthreads();
}

__device__ __forceinline__ unsigned limit_cache_slot(int g) {
  return ((uint32_t)g * 0x9e3779b1u) >> (32 - kLimitCacheBits);
}

// Every thread of the block, after limit_cache_init: the keys of `list` (< n) claim their slots.
__device__ __forceinline__ void limit_cache_seed(LimitCache& c, const uint32_t* __restrict__ list, uint32_t count,
                                                 uint32_t n) {
  for (uint32_t i = threadIdx.x; i < count; i += kBrThreads) {
    const uint32_t k = list[i];
    if (k < n) atomicCAS(&c.key[limit_cache_slot((int)k)], -1, (int)k);
  }
  __syncthreads();
}

// true: g is cached in this block and the run was added there
__device__ __forceinline__ bool limit_cache_add(LimitCache& c, int g, uint32_t rows) {
  const unsigned s = limit_cache_slot(g);
  if (__hip_atomic_load(&c.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != g) return false;
  atomicAdd(&c.rows[s], rows);
  return true;
}

// After a memory atomic on g's count returned `old`: a busy key claims its slot, if it is free.
__device__ __forceinline__ void limit_cache_note(LimitCache& c, int g, uint32_t old) {
  if (old >= kLimitBusy) atomicCAS(&c.key[limit_cache_slot(g)], -1, g);
}

template <bool ALIGNED>
__global__ __launch_bounds__(kBrThreads) void limit_demand_kernel(const int* __restrict__ actor, int64_t M,
                                                                   uint32_t* __restrict__ demand,
                                                                   uint32_t* __restrict__ touched,
                                                                   const uint32_t* __restrict__ busy,
                                                                   unsigned long long* __restrict__ ctr, uint32_t n,
                                                                   uint32_t now) {
  __shared__ unsigned oob_wave[kBrWaves];
  __shared__ LimitCache cache;
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (M + kBrTile - 1) / kBrTile;
  unsigned n_oob = 0;
  // the last Send's busy actors; this Send's list starts empty (the step launch fills it)
  const unsigned mine = now & 1u, last = mine ^ 1u;
  unsigned long long hints = ctr[kLimitBusyN + last];
  if (hints > kLimitBusyCap) hints = kLimitBusyCap;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctr[kLimitBusyN + mine] = 0ull;
  limit_cache_init(cache);
  limit_cache_seed(cache, busy + last * kLimitBusyCap, (uint32_t)hints, n);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (block-uniform: every lane shuffles)
#pragma unroll
    for (int j = 0; j < kBrRows; ++j) {
      const int64_t i = br_elem(tile, j, wave, lane);
      int id[4], g[4];
      br_load4<ALIGNED>(actor, i, M, (int)kBrNoActor, id);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t a = (uint32_t)id[c];
        g[c] = a < n ? (int)a : -1;
        n_oob += a >= n && i + c < M;
      }
      br_combine_runs(g, lane, [&](int run_g, uint32_t run_n) {
        bool fresh = false;
        if (run_g >= 0 && !limit_cache_add(cache, run_g, run_n)) {
          const uint32_t old = atomicAdd(&demand[run_g], run_n);
          fresh = old == 0u;
          limit_cache_note(cache, run_g, old);
        }
        br_append(fresh, (uint32_t)run_g, ctr + kLimitTouched, touched, n);
      });
    }
  }
  // the cached rows into demand[]: an actor named by the last Send may be counted here first
  __syncthreads();
  for (int s = threadIdx.x; s < kLimitCacheSlots; s += kBrThreads) {  // (block-uniform: every lane ballots)
    const int g = cache.key[s];
    bool fresh = false;
    if (g >= 0 && cache.rows[s]) fresh = atomicAdd(&demand[g], cache.rows[s]) == 0u;
    br_append(fresh, (uint32_t)g, ctr + kLimitTouched, touched, n);
  }
#pragma unroll
  for (int o = kWave / 2; o; o >>= 1) n_oob += (unsigned)__shfl_xor((int)n_oob, o, kWave);
  if (lane == 0) oob_wave[wave] = n_oob;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = oob_wave[0] + oob_wave[1] + oob_wave[2] + oob_wave[3];
    if (t) atomicAdd(&ctr[kLimitOob], (unsigned long long)t);
  }
}
static_assert(kBrWaves == 4, "the oob reduction reads four waves' partials");
static_assert(kLimitCacheSlots % kBrThreads == 0, "every thread walks the same number of cache slots");

__global__ __launch_bounds__(kBrThreads) void limit_step_kernel(uint64_t* __restrict__ word,
                                                                 uint32_t* __restrict__ demand,
                                                                 const uint32_t* __restrict__ touched,
                                                                 uint32_t* __restrict__ hot_actor,
                                                                 uint32_t* __restrict__ rem,
                                                                 uint32_t* __restrict__ prefix,
                                                                 uint32_t* __restrict__ busy,
                                                                 unsigned long long* __restrict__ ctr, uint32_t n,
                                                                 uint32_t now, uint32_t rate, uint32_t burst,
                                                                 uint32_t busy_rows) {
  unsigned long long count = ctr[kLimitTouched];
  if (count > n) count = n;
  const unsigned lane = lane_id();
  unsigned long long throttled = 0;
  // (the loop is block-uniform: every lane ballots)
  for (unsigned long long base = (unsigned long long)blockIdx.x * kBrThreads; base < count;
       base += (unsigned long long)gridDim.x * kBrThreads) {
    const unsigned long long t = base + threadIdx.x;
    uint32_t a = kBrNoActor, q = 0;
    bool hot = false;
    if (t < count) a = touched[t];
    if (a < n) {
      const uint32_t d = demand[a];
      const uint32_t spent = limit_refilled(word[a], now, rate);
      const uint32_t avail = burst > spent ? burst - spent : 0u;
      q = d < avail ? d : avail;
      word[a] = limit_word(now, spent + q);
      hot = d > avail;
      if (hot)
        throttled += d - q;
      else
        demand[a] = 0u;
      // a busy actor is named to the next Send (at most kLimitBusyCap have busy_rows rows)
      if (d >= busy_rows) {
        const unsigned long long pos = atomicAdd(&ctr[kLimitBusyN + (now & 1u)], 1ull);
        if (pos < kLimitBusyCap) busy[(now & 1u) * kLimitBusyCap + pos] = a;
      }
    }
    const uint64_t m = __ballot(hot);
    if (m) {  // (wave-uniform) the hot slots of this wave instruction: one reservation
      const int leader = __ffsll((long long)m) - 1;
      unsigned long long h0 = 0;
      if ((int)lane == leader) h0 = atomicAdd(&ctr[kLimitOver], (unsigned long long)__popcll(m));
      h0 = __shfl(h0, leader, kWave);
      const unsigned long long h = h0 + mbcnt64(m);
      if (hot && h < n) {  // (an actor is hot once per Send: h < n always)
        hot_actor[h] = a, rem[h] = q, prefix[h] = 0u;
        demand[a] = kLimitHot | (uint32_t)h;
      }
    }
  }
#pragma unroll
  for (int o = kWave / 2; o; o >>= 1) throttled += __shfl_xor(throttled, o, kWave);
  if (lane == 0 && throttled) atomicAdd(&ctr[kLimitThrottled], throttled);
  // the last block out re-arms touched[]: every block has read the count by then
  __syncthreads();
  if (threadIdx.x == 0 && last_block_ticket(reinterpret_cast<unsigned*>(ctr + kLimitCounters)))
    ctr[kLimitTouched] = 0ull;
}
static_assert((kLimitCtrWords - kLimitCounters) * 2 >= (int)kTicketWords, "the ticket words fit the counter block");

// The count launches take every key into the block's cache, first come first kept: their keys
// are (hot slot, digit) pairs, and with few actors over quota -- the one hot actor -- every hot
// row of the batch would otherwise meet the others on 16 addresses.
// true: the run was added to the block's cache; false: its slot holds another key
__device__ __forceinline__ bool limit_cache_take(LimitCache& c, int g, uint32_t rows) {
  const unsigned s = limit_cache_slot(g);
  const int old = atomicCAS(&c.key[s], -1, g);
  if (old != -1 && old != g) return false;
  atomicAdd(&c.rows[s], rows);
  return true;
}

// Every thread of the block, after its last count: the cached rows into the bins.
__device__ __forceinline__ void limit_cache_flush(LimitCache& c, uint32_t* __restrict__ bins) {
  __syncthreads();
  for (int s = threadIdx.x; s < kLimitCacheSlots; s += kBrThreads) {
    const int g = c.key[s];
    if (g >= 0) atomicAdd(&bins[g], c.rows[s]);
  }
}

// Every lane of the wave calls this together: the four consecutive rows at i with the hot
// slots h[c] (< 0: not hot) counted into the level's bins.  FIRST: level 0, no prefix yet.
template <bool FIRST>
__device__ __forceinline__ void limit_count_rows(const int (&h)[4], int64_t i, unsigned lane, int shift,
                                                 const uint32_t* __restrict__ prefix, uint32_t* __restrict__ bins,
                                                 LimitCache& cache) {
  int g[4];
  bool any = false;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    g[c] = -1;
    if (h[c] < 0) continue;
    const uint32_t row = (uint32_t)(i + c);
    if (FIRST || (row >> (shift + kLimitDigit)) == prefix[h[c]])
      g[c] = h[c] << kLimitDigit | (int)((row >> shift) & kLimitDigitMask), any = true;
  }
  if (!__ballot(any)) return;  // (wave-uniform)
  br_combine_runs(g, lane, [&](int run_g, uint32_t run_n) {
    if (run_g >= 0 && !limit_cache_take(cache, run_g, run_n)) atomicAdd(&bins[run_g], run_n);
  });
}

template <bool ALIGNED>
__global__ __launch_bounds__(kBrThreads) void limit_slots_kernel(const int* __restrict__ actor, int64_t M,
                                                                  const uint32_t* __restrict__ demand, uint32_t n,
                                                                  uint32_t over, int shift, int* __restrict__ slot,
                                                                  uint32_t* __restrict__ bins) {
  __shared__ LimitCache cache;
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (M + kBrTile - 1) / kBrTile;
  limit_cache_init(cache);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (block-uniform: every lane shuffles)
#pragma unroll
    for (int j = 0; j < kBrRows; ++j) {
      const int64_t i = br_elem(tile, j, wave, lane);
      int id[4], h[4];
      br_load4<ALIGNED>(actor, i, M, (int)kBrNoActor, id);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t a = (uint32_t)id[c];
        h[c] = -1;
        if (a < n) {
          const uint32_t d = demand[a];
          if ((d & kLimitHot) && (d & ~kLimitHot) < over) h[c] = (int)(d & ~kLimitHot);  // (a slot is < over always)
        }
      }
      if (i + 4 <= M) {  // (slot is the launcher's own 16-byte aligned buffer)
        *reinterpret_cast<int4*>(slot + i) = make_int4(h[0], h[1], h[2], h[3]);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (i + c < M) slot[i + c] = h[c];
      }
      limit_count_rows<true>(h, i, lane, shift, nullptr, bins, cache);
    }
  }
  limit_cache_flush(cache, bins);
}

__global__ __launch_bounds__(kBrThreads) void limit_count_kernel(const int* __restrict__ slot, int64_t M, int shift,
                                                                  const uint32_t* __restrict__ prefix,
                                                                  uint32_t* __restrict__ bins) {
  __shared__ LimitCache cache;
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (M + kBrTile - 1) / kBrTile;
  limit_cache_init(cache);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (block-uniform: every lane shuffles)
#pragma unroll
    for (int j = 0; j < kBrRows; ++j) {
      const int64_t i = br_elem(tile, j, wave, lane);
      int h[4];
      br_load4<true>(slot, i, M, -1, h);
      limit_count_rows<false>(h, i, lane, shift, prefix, bins, cache);
    }
  }
  limit_cache_flush(cache, bins);
}

__global__ __launch_bounds__(kBrThreads) void limit_resolve_kernel(uint32_t* __restrict__ bins,
                                                                    uint32_t* __restrict__ rem,
                                                                    uint32_t* __restrict__ prefix, uint32_t over) {
  for (uint32_t h = blockIdx.x * kBrThreads + threadIdx.x; h < over; h += gridDim.x * kBrThreads) {
    uint4* b = reinterpret_cast<uint4*>(bins + ((size_t)h << kLimitDigit));
    uint32_t cnt[kLimitBins];
#pragma unroll
    for (int k = 0; k < kLimitBins / 4; ++k) {
      const uint4 v = b[k];
      cnt[4 * k] = v.x, cnt[4 * k + 1] = v.y, cnt[4 * k + 2] = v.z, cnt[4 * k + 3] = v.w;
      b[k] = make_uint4(0u, 0u, 0u, 0u);
    }
    // the smallest digit whose cumulative count exceeds rem (one exists: q < demand; the last
    // digit takes it otherwise, so the prefix stays a row index whatever the bins hold)
    const uint32_t r = rem[h];
    uint32_t below = 0, digit = kLimitBins - 1, skipped = 0;
    bool found = false;
#pragma unroll
    for (int k = 0; k < kLimitBins; ++k) {
      if (!found && below + cnt[k] > r) digit = (uint32_t)k, skipped = below, found = true;
      below += cnt[k];
    }
    if (!found) skipped = below - cnt[kLimitBins - 1];
    prefix[h] = prefix[h] << kLimitDigit | digit;
    rem[h] = r - (skipped < r ? skipped : r);
  }
}
static_assert(kLimitBins % 4 == 0, "a slot's bins are read 16 bytes at a time");

__global__ __launch_bounds__(kBrThreads) void limit_admit_kernel(const int* __restrict__ slot, int64_t M,
                                                                  const uint32_t* __restrict__ thr,
                                                                  int64_t* __restrict__ val, int* __restrict__ st) {
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (M + kBrTile - 1) / kBrTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int j = 0; j < kBrRows; ++j) {
      const int64_t i = br_elem(tile, j, wave, lane);
      int h[4], out[4];
      br_load4<true>(slot, i, M, -1, h);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        out[c] = h[c] < 0 || (uint32_t)(i + c) < thr[h[c]] ? kLimitPending : (int)kStatusThrottled;
      if (i + 4 <= M) {  // (val and st are the launcher's own 16-byte aligned buffers)
        *reinterpret_cast<int4*>(st + i) = make_int4(out[0], out[1], out[2], out[3]);
        *reinterpret_cast<int4*>(val + i) = make_int4(0, 0, 0, 0);
        *reinterpret_cast<int4*>(val + i + 2) = make_int4(0, 0, 0, 0);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (i + c < M) st[i + c] = out[c], val[i + c] = 0;
      }
    }
  }
}

__global__ __launch_bounds__(kBrThreads) void limit_rearm_kernel(const uint32_t* __restrict__ hot_actor,
                                                                  uint32_t* __restrict__ demand,
                                                                  unsigned long long* __restrict__ ctr, uint32_t n,
                                                                  uint32_t over) {
  for (uint32_t h = blockIdx.x * kBrThreads + threadIdx.x; h < over; h += gridDim.x * kBrThreads) {
    const uint32_t a = hot_actor[h];
    if (a < n) demand[a] = 0u;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) ctr[kLimitOver] = 0ull;  // (the count came as an argument: nobody reads it here)
}

__global__ __launch_bounds__(kBrThreads) void limit_clear_kernel(uint64_t* __restrict__ word,
                                                                  uint32_t* __restrict__ demand,
                                                                  unsigned long long* __restrict__ ctr, uint32_t n) {
  for (uint32_t a = blockIdx.x * kBrThreads + threadIdx.x; a < n; a += gridDim.x * kBrThreads)
    word[a] = 0ull, demand[a] = 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    ctr[kLimitOver] = 0ull, ctr[kLimitTouched] = 0ull, ctr[kLimitBusyN] = 0ull, ctr[kLimitBusyN + 1] = 0ull;
}

// ---------------------------------------------------------------- launchers
int64_t limit_tile() { return kBrTile; }

static void limit_check(const char* what, int64_t M, uintptr_t actor, int64_t n, uintptr_t ctr, uint32_t now) {
  if (M < 0 || M > 0x7fffffffll) throw std::invalid_argument(std::string(what) + ": M must be in [0, 2^31 - 1]");
  if (n < 1 || n > kLimitMaxActors) throw std::invalid_argument(std::string(what) + ": n must be in [1, 2^28]");
  if (now < 1 || now > kLimitMaxTick) throw std::invalid_argument(std::string(what) + ": now must be in [1, 2^31 - 1]");
  if (M > 0 && !actor) throw std::invalid_argument(std::string(what) + ": null actor column");
  if (!ctr || ctr & 7u || actor & 3u) throw std::invalid_argument(std::string(what) + ": null or misaligned buffer");
}

static unsigned limit_grid(int64_t M) {
  const int64_t tiles = (M + kBrTile - 1) / kBrTile;
  return (unsigned)(tiles < kBrBlocks ? tiles : kBrBlocks);
}

static unsigned limit_list_grid(int64_t count, int64_t most) {
  const int64_t want = (count + kBrThreads - 1) / kBrThreads;
  return (unsigned)(want < most ? want : most);
}

// actor int32[M] (any 4-byte alignment); word u64[n]; demand / touched / hot_actor / rem /
// prefix u32[n]; busy u32[2 * kLimitBusyCap]; ctr u64[kLimitCtrWords].  The demand launch, then the step launch: the
// words are final, ctr[kLimitOver] says how many actors are over their quota.
void launch_limit_demand(uintptr_t actor, int64_t M, uintptr_t word, uintptr_t demand, uintptr_t touched,
                         uintptr_t hot_actor, uintptr_t rem, uintptr_t prefix, uintptr_t busy, uintptr_t ctr, int64_t n,
                         uint32_t now, uint32_t rate, uint32_t burst, uintptr_t stream) {
  limit_check("limit_demand", M, actor, n, ctr, now);
  if (rate < 1 || burst < 1) throw std::invalid_argument("limit_demand: rate and burst must be in [1, 2^32)");
  if (M == 0) return;
  if (!word || word & 7u || !demand || !touched || !hot_actor || !rem || !prefix || !busy
      || (demand | touched | hot_actor | rem | prefix | busy) & 3u)
    throw std::invalid_argument("limit_demand: null or misaligned table");
  const bool aligned = !(actor & 15u);
  const dim3 block(kBrThreads);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(aligned ? limit_demand_kernel<true> : limit_demand_kernel<false>, dim3(limit_grid(M)), block, 0, s,
                     (const int*)actor, M, (uint32_t*)demand, (uint32_t*)touched, (const uint32_t*)busy,
                     (unsigned long long*)ctr, (uint32_t)n, now);
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(limit_step_kernel, dim3(limit_list_grid(n < M ? n : M, kLimitStepBlocks)), block, 0, s,
                     (uint64_t*)word, (uint32_t*)demand, (const uint32_t*)touched, (uint32_t*)hot_actor, (uint32_t*)rem,
                     (uint32_t*)prefix, (uint32_t*)busy, (unsigned long long*)ctr, (uint32_t)n, now, rate, burst,
                     limit_busy_rows(M));
  PT_HIP_CHECK(hipGetLastError());
}

// After launch_limit_demand left `over` > 0 hot slots (the host read it): the radix select
// of every hot actor's threshold row, the admit launch and the re-arm.  slot int32[M], val
// int64[M] and st int32[M] 16-byte aligned; bins u32[bins_words] 16-byte aligned, zero on
// entry and on return, bins_words >= over << kLimitDigit.
void launch_limit_cut(uintptr_t actor, int64_t M, uintptr_t demand, uintptr_t hot_actor, uintptr_t rem, uintptr_t prefix,
                      uintptr_t ctr, int64_t n, int64_t over, uintptr_t slot, uintptr_t bins, int64_t bins_words,
                      uintptr_t val, uintptr_t st, uintptr_t stream) {
  limit_check("limit_cut", M, actor, n, ctr, 1);
  if (!demand || !hot_actor || !rem || !prefix || (demand | hot_actor | rem | prefix) & 3u)
    throw std::invalid_argument("limit_cut: null or misaligned table");
  if (over < 1 || over > n || over > M) throw std::invalid_argument("limit_cut: over must be in [1, min(n, M)]");
  const dim3 block(kBrThreads);
  hipStream_t s = as_stream(stream);
  const dim3 hot_grid(limit_list_grid(over, 1024));
  const auto rearm = [&]() {
    hipLaunchKernelGGL(limit_rearm_kernel, hot_grid, block, 0, s, (const uint32_t*)hot_actor, (uint32_t*)demand,
                       (unsigned long long*)ctr, (uint32_t)n, (uint32_t)over);
    PT_HIP_CHECK(hipGetLastError());
  };
  if (over > kLimitMaxHot || !slot || !bins || !val || !st || (slot | bins | val | st) & 15u
      || bins_words < (over << kLimitDigit)) {
    if (over <= n) rearm();  // (the tables are left at rest; the tokens of this Send are spent)
    throw std::invalid_argument("limit_cut: too many hot actors, or a null, misaligned or short scratch buffer");
  }
  const bool aligned = !(actor & 15u);
  const dim3 grid(limit_grid(M));
  const int L = limit_levels(M);
  hipLaunchKernelGGL(aligned ? limit_slots_kernel<true> : limit_slots_kernel<false>, grid, block, 0, s, (const int*)actor,
                     M, (const uint32_t*)demand, (uint32_t)n, (uint32_t)over, (L - 1) * kLimitDigit, (int*)slot,
                     (uint32_t*)bins);
  PT_HIP_CHECK(hipGetLastError());
  for (int l = 0; l < L; ++l) {
    if (l > 0) {
      hipLaunchKernelGGL(limit_count_kernel, grid, block, 0, s, (const int*)slot, M, (L - 1 - l) * kLimitDigit,
                         (const uint32_t*)prefix, (uint32_t*)bins);
      PT_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(limit_resolve_kernel, hot_grid, block, 0, s, (uint32_t*)bins, (uint32_t*)rem, (uint32_t*)prefix,
                       (uint32_t)over);
    PT_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(limit_admit_kernel, grid, block, 0, s, (const int*)slot, M, (const uint32_t*)prefix, (int64_t*)val,
                     (int*)st);
  PT_HIP_CHECK(hipGetLastError());
  rearm();
}

void launch_limit_clear(uintptr_t word, uintptr_t demand, uintptr_t ctr, int64_t n, uintptr_t stream) {
  if (n < 1 || n > kLimitMaxActors) throw std::invalid_argument("limit_clear: n must be in [1, 2^28]");
  if (!word || !demand || !ctr || (word | ctr) & 7u || demand & 3u)
    throw std::invalid_argument("limit_clear: null or misaligned table");
  hipLaunchKernelGGL(limit_clear_kernel, dim3(limit_list_grid(n, 1024)), dim3(kBrThreads), 0, as_stream(stream),
                     (uint64_t*)word, (uint32_t*)demand, (unsigned long long*)ctr, (uint32_t)n);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
