// Circuit breaker kernels (`DeviceRuntime.send(breaker=True)`, ops/breaker.py; breaker.hpp
// has the state word, the side tables and the counters).  A guarded Send runs at tick
// `now`; all launches are on the Send's stream and launch boundaries are the only ordering
// (as in reply_cache.hip).
//
// Before the inner Send, only when some actor is open:
//   breaker_probe_kernel        rows whose actor is half-open lower probe[a] (u64 atomicMin)
//                               to breaker_claim(now, row); of a run of equal adjacent ids
//                               only the head -- its lowest row -- issues the atomic
//   breaker_admit_kernel        the next launch: st[i] = kBreakerPending for a row that
//                               travels (closed, out of the table, or the probe),
//                               kStatusBreakerOpen for a rejected one; val[i] = 0; rows
//                               with an id >= n counted, one atomic per block
// After it, over the K rows that travelled and their final statuses:
//   breaker_observe_bad_kernel  streams the statuses; a row in trip_on loads its actor,
//                               equal adjacent ids are combined per thread and per wave
//                               (gather.hip's ballot + segmented scan) and each run adds
//                               its count to obs[a] once; the adder that saw 0 appends a to
//                               touched[] (one reservation per wave instruction)
//   breaker_observe_ok_kernel   exits at once when n_dirty == 0 && n_touched == 0 (an OK
//                               reply to a clean actor changes nothing); else an OK row
//                               (the head of a run of equal adjacent ids) whose actor has a
//                               non-zero word or obs sets kBreakerObsOk in obs[a], appending
//                               a when obs was 0.  A launch of its own: it
//                               must see the finished bad counts, so that a clean actor with
//                               bad and OK rows in one Send ends with fails = 0
//   breaker_step_kernel         grid-stride over touched[0 .. n_touched): the transition
//                               of breaker.hpp / BreakerRef._step, obs[a] = 0, the counter
//                               deltas folded per wave; the last block re-arms n_touched
//   breaker_clear_kernel        every word and obs 0, every probe all ones, n_open /
//                               n_dirty / n_touched 0 (reset, and the tick restart)
//
// The cost follows the failures: a healthy Send pays one 4 B/message stream and two
// near-empty launches.  obs[a] is only written by atomics (bad: add, ok: or) and zeroed by
// the one step thread that owns a, so every count is exact whatever the arrival order.
//
// Tile layout, loads, run combining and the touched[] reservation: runs.hpp.
#include "breaker.hpp"
#include "common.hpp"
#include "runs.hpp"

namespace ptype {

constexpr int kBrStepBlocks = 64;

__device__ __forceinline__ bool br_half_open(uint64_t w, uint32_t now) {
  return breaker_is_open(w) && now >= breaker_until(w);
}

template <bool ALIGNED>
__global__ __launch_bounds__(kBrThreads) void breaker_probe_kernel(const int* __restrict__ actor, int64_t M,
                                                                    const uint64_t* __restrict__ word,
                                                                    unsigned long long* __restrict__ probe, uint32_t n,
                                                                    uint32_t now) {
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (M + kBrTile - 1) / kBrTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (block-uniform: every lane shuffles)
#pragma unroll
    for (int j = 0; j < kBrRows; ++j) {
      const int64_t i = br_elem(tile, j, wave, lane);
      int id[4];
      br_load4<ALIGNED>(actor, i, M, (int)kBrNoActor, id);
      const int prev = __shfl_up(id[3], 1, kWave);
      // a run's head: per thread by compare, across the wave against the previous lane's last id
      // (lane 0 cannot see its neighbour: it asks too, with a row no lower than the run's head)
      const uint64_t wave_heads = __ballot(lane == 0 || id[0] != prev);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool head = c == 0 ? ((wave_heads >> lane) & 1ull) != 0 : id[c] != id[c - 1];
        const uint32_t a = (uint32_t)id[c];
        if (!head || a >= n) continue;
        if (br_half_open(word[a], now)) atomicMin(&probe[a], (unsigned long long)breaker_claim(now, (uint32_t)(i + c)));
      }
    }
  }
}

template <bool ALIGNED>
__global__ __launch_bounds__(kBrThreads) void breaker_admit_kernel(const int* __restrict__ actor, int64_t M,
                                                                    const uint64_t* __restrict__ word,
                                                                    const unsigned long long* __restrict__ probe,
                                                                    uint32_t n, uint32_t now,
                                                                    unsigned long long* __restrict__ ctr,
                                                                    int64_t* __restrict__ val, int* __restrict__ st) {
  __shared__ unsigned oob_wave[kBrWaves];
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (M + kBrTile - 1) / kBrTile;
  unsigned n_oob = 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int j = 0; j < kBrRows; ++j) {
      const int64_t i = br_elem(tile, j, wave, lane);
      int id[4], out[4];
      br_load4<ALIGNED>(actor, i, M, (int)kBrNoActor, id);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t a = (uint32_t)id[c];
        bool pass = true;
        if (a < n) {
          const uint64_t w = word[a];
          if (breaker_is_open(w))
            pass = now >= breaker_until(w) && probe[a] == breaker_claim(now, (uint32_t)(i + c));
        } else {
          n_oob += i + c < M;
        }
        out[c] = pass ? kBreakerPending : (int)kStatusBreakerOpen;
      }
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
#pragma unroll
  for (int o = kWave / 2; o; o >>= 1) n_oob += (unsigned)__shfl_xor((int)n_oob, o, kWave);
  if (lane == 0) oob_wave[wave] = n_oob;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = oob_wave[0] + oob_wave[1] + oob_wave[2] + oob_wave[3];
    if (t) atomicAdd(&ctr[kBreakerOob], (unsigned long long)t);
  }
}
static_assert(kBrWaves == 4, "the oob reduction reads four waves' partials");

// Every lane of the wave calls this together: run (g, cnt) of failed rows, g < 0 for none.
__device__ __forceinline__ void br_emit_bad(int g, uint32_t cnt, unsigned long long* __restrict__ obs,
                                            unsigned long long* __restrict__ ctr, uint32_t* __restrict__ touched,
                                            uint32_t n) {
  bool fresh = false;
  if (g >= 0) fresh = atomicAdd(&obs[g], (unsigned long long)cnt) == 0ull;
  br_append(fresh, (uint32_t)g, ctr + kBreakerTouched, touched, n);
}

template <bool ALIGNED>
__global__ __launch_bounds__(kBrThreads) void breaker_observe_bad_kernel(const int* __restrict__ status,
                                                                          const int* __restrict__ actor, int64_t M,
                                                                          uint32_t trip_mask,
                                                                          unsigned long long* __restrict__ obs,
                                                                          uint32_t* __restrict__ touched,
                                                                          unsigned long long* __restrict__ ctr,
                                                                          uint32_t n) {
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (M + kBrTile - 1) / kBrTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (block-uniform: every lane shuffles)
#pragma unroll
    for (int j = 0; j < kBrRows; ++j) {
      const int64_t i = br_elem(tile, j, wave, lane);
      int s[4], g[4];
      br_load4<ALIGNED>(status, i, M, (int)kStatusOk, s);
      bool any = false;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        g[c] = -1;  // not a failed row of a guarded actor
        if ((unsigned)s[c] < 32u && ((trip_mask >> (unsigned)s[c]) & 1u)) {
          const uint32_t a = (uint32_t)actor[i + c];  // (trip_mask has no bit 0: i + c < M)
          if (a < n) g[c] = (int)a, any = true;
        }
      }
      if (!__ballot(any)) continue;  // (wave-uniform) the healthy Send: nothing but the stream

      br_combine_runs(g, lane, [&](int run_g, uint32_t run_n) { br_emit_bad(run_g, run_n, obs, ctr, touched, n); });
    }
  }
}

template <bool ALIGNED>
__global__ __launch_bounds__(kBrThreads) void breaker_observe_ok_kernel(const int* __restrict__ status,
                                                                         const int* __restrict__ actor, int64_t M,
                                                                         const uint64_t* __restrict__ word,
                                                                         unsigned long long* __restrict__ obs,
                                                                         uint32_t* __restrict__ touched,
                                                                         unsigned long long* __restrict__ ctr,
                                                                         uint32_t n) {
  // nothing dirty and no failed row in this Send: no OK reply can change a word.  (Every
  // thread of the grid reads the same answer: n_dirty moves only in the step launch, and
  // n_touched rises in this launch only when this test failed for everybody.)
  if (ctr[kBreakerNDirty] == 0ull && ctr[kBreakerTouched] == 0ull) return;
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (M + kBrTile - 1) / kBrTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (block-uniform: every lane ballots)
#pragma unroll
    for (int j = 0; j < kBrRows; ++j) {
      const int64_t i = br_elem(tile, j, wave, lane);
      int s[4];
      uint32_t a[4];
      br_load4<ALIGNED>(status, i, M, -1, s);
#pragma unroll
      for (int c = 0; c < 4; ++c) a[c] = s[c] == (int)kStatusOk ? (uint32_t)actor[i + c] : kBrNoActor;  // (rows past M read as -1)
      // of a run of equal adjacent ids only the head asks (per thread by compare, across the
      // wave against the previous lane's last id): the bit another XCD set in this launch may
      // not be visible to a plain load yet, and every row that misses it costs an atomic on
      // one address (all OK rows to one dirty actor: 3.7 ms per 8 Mi without this)
      const uint32_t prev = (uint32_t)__shfl_up((int)a[3], 1, kWave);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool head = c == 0 ? (lane == 0 || a[0] != prev) : a[c] != a[c - 1];
        bool fresh = false;
        if (head && a[c] < n) {
          const uint64_t o = obs[a[c]];
          if ((word[a[c]] | o) != 0ull && !(o & kBreakerObsOk))
            fresh = atomicOr(&obs[a[c]], (unsigned long long)kBreakerObsOk) == 0ull;
        }
        br_append(fresh, a[c], ctr + kBreakerTouched, touched, n);
      }
    }
  }
}

__global__ __launch_bounds__(kBrThreads) void breaker_step_kernel(uint64_t* __restrict__ word,
                                                                   unsigned long long* __restrict__ obs,
                                                                   const uint32_t* __restrict__ touched,
                                                                   unsigned long long* __restrict__ ctr, uint32_t n,
                                                                   uint32_t now, uint32_t threshold,
                                                                   uint32_t cooldown) {
  unsigned long long count = ctr[kBreakerTouched];
  if (count > n) count = n;
  const uint32_t until = breaker_deadline(now, cooldown);
  int d_open = 0, d_dirty = 0, trips = 0, closes = 0;
  for (unsigned long long t = (unsigned long long)blockIdx.x * kBrThreads + threadIdx.x; t < count;
       t += (unsigned long long)gridDim.x * kBrThreads) {
    const uint32_t a = touched[t];
    if (a >= n) continue;
    const uint64_t w = word[a], o = obs[a];
    const bool ok = (o & kBreakerObsOk) != 0ull;
    const uint64_t n_bad = o & ~kBreakerObsOk;
    uint64_t nw = w;
    if (!breaker_is_open(w)) {
      if (ok) {
        nw = 0ull;  // any success resets the consecutive failures
      } else {
        uint64_t fails = (uint64_t)breaker_fails(w) + n_bad;
        if (fails > 0xffffffffull) fails = 0xffffffffull;
        nw = fails >= threshold ? breaker_open_word(until, (uint32_t)fails) : fails;
        trips += fails >= threshold;
      }
    } else if (ok) {
      nw = 0ull, closes += 1;
    } else if (n_bad) {
      nw = breaker_open_word(until, breaker_fails(w));
    }
    word[a] = nw;
    obs[a] = 0ull;
    d_open += (int)breaker_is_open(nw) - (int)breaker_is_open(w);
    d_dirty += (int)(nw != 0ull) - (int)(w != 0ull);
  }
#pragma unroll
  for (int o = kWave / 2; o; o >>= 1) {
    d_open += __shfl_xor(d_open, o, kWave);
    d_dirty += __shfl_xor(d_dirty, o, kWave);
    trips += __shfl_xor(trips, o, kWave);
    closes += __shfl_xor(closes, o, kWave);
  }
  if (lane_id() == 0) {  // (a negative delta wraps: the counters are sums mod 2^64)
    if (d_open) atomicAdd(&ctr[kBreakerNOpen], (unsigned long long)(long long)d_open);
    if (d_dirty) atomicAdd(&ctr[kBreakerNDirty], (unsigned long long)(long long)d_dirty);
    if (trips) atomicAdd(&ctr[kBreakerTrips], (unsigned long long)trips);
    if (closes) atomicAdd(&ctr[kBreakerCloses], (unsigned long long)closes);
  }
  // the last block out re-arms touched[]: every block has read the count by then
  __syncthreads();
  if (threadIdx.x == 0 && last_block_ticket(reinterpret_cast<unsigned*>(ctr + kBreakerCounters)))
    ctr[kBreakerTouched] = 0ull;
}
static_assert((kBreakerCtrWords - kBreakerCounters) * 2 >= (int)kTicketWords, "the ticket words fit the counter block");

__global__ __launch_bounds__(kBrThreads) void breaker_clear_kernel(uint64_t* __restrict__ word,
                                                                    unsigned long long* __restrict__ obs,
                                                                    unsigned long long* __restrict__ probe,
                                                                    unsigned long long* __restrict__ ctr, uint32_t n) {
  for (uint32_t a = blockIdx.x * kBrThreads + threadIdx.x; a < n; a += gridDim.x * kBrThreads)
    word[a] = 0ull, obs[a] = 0ull, probe[a] = ~0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    ctr[kBreakerNOpen] = 0ull, ctr[kBreakerNDirty] = 0ull, ctr[kBreakerTouched] = 0ull;
}

// ---------------------------------------------------------------- launchers
int64_t breaker_tile() { return kBrTile; }

static void br_check(const char* what, int64_t M, uintptr_t actor, int64_t n, uintptr_t ctr, uint32_t now) {
  if (M < 0 || M > 0x7fffffffll) throw std::invalid_argument(std::string(what) + ": M must be in [0, 2^31 - 1]");
  if (n < 1 || n > kBreakerMaxActors) throw std::invalid_argument(std::string(what) + ": n must be in [1, 2^28]");
  if (now < 1 || now > kBreakerMaxTick) throw std::invalid_argument(std::string(what) + ": now must be in [1, 2^31 - 1]");
  if (M > 0 && !actor) throw std::invalid_argument(std::string(what) + ": null actor column");
  if (!ctr || ctr & 7u || actor & 3u) throw std::invalid_argument(std::string(what) + ": null or misaligned buffer");
}

static unsigned br_grid(int64_t M) {
  const int64_t tiles = (M + kBrTile - 1) / kBrTile;
  return (unsigned)(tiles < kBrBlocks ? tiles : kBrBlocks);
}

// actor int32[M] (any 4-byte alignment); word / probe u64[n]; ctr u64[kBreakerCtrWords];
// val int64[M] and st int32[M], 16-byte aligned.  The probe launch, then the admit launch.
void launch_breaker_admit(uintptr_t actor, int64_t M, uintptr_t word, uintptr_t probe, int64_t n, uint32_t now,
                          uintptr_t ctr, uintptr_t val, uintptr_t st, uintptr_t stream) {
  br_check("breaker_admit", M, actor, n, ctr, now);
  if (M == 0) return;
  if (!word || !probe || !val || !st || (word | probe) & 7u || (val | st) & 15u)
    throw std::invalid_argument("breaker_admit: null or misaligned table or output");
  const bool aligned = !(actor & 15u);
  const dim3 grid(br_grid(M)), block(kBrThreads);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(aligned ? breaker_probe_kernel<true> : breaker_probe_kernel<false>, grid, block, 0, s,
                     (const int*)actor, M, (const uint64_t*)word, (unsigned long long*)probe, (uint32_t)n, now);
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(aligned ? breaker_admit_kernel<true> : breaker_admit_kernel<false>, grid, block, 0, s,
                     (const int*)actor, M, (const uint64_t*)word, (const unsigned long long*)probe, (uint32_t)n, now,
                     (unsigned long long*)ctr, (int64_t*)val, (int*)st);
  PT_HIP_CHECK(hipGetLastError());
}

// The K rows that travelled (actor int32[K]) and their final statuses (st int32[K], any
// 4-byte alignment): the bad-row launch, the ok launch, the step launch.  obs u64[n] and
// touched u32[n] hold zeros / anything between Sends; trip_mask: bit s set for a status
// that counts as a failure (never bit 0).
void launch_breaker_observe(uintptr_t actor, uintptr_t st, int64_t K, uint32_t trip_mask, uintptr_t word, uintptr_t obs,
                            uintptr_t touched, uintptr_t ctr, int64_t n, uint32_t now, uint32_t threshold,
                            uint32_t cooldown, uintptr_t stream) {
  br_check("breaker_observe", K, actor, n, ctr, now);
  if (K == 0) return;
  if (!st || st & 3u || !word || !obs || !touched || (word | obs) & 7u || touched & 3u)
    throw std::invalid_argument("breaker_observe: null or misaligned table or column");
  if (trip_mask & 1u || !trip_mask || trip_mask >> 7) throw std::invalid_argument("breaker_observe: trip_mask takes statuses 1..6");
  if (threshold < 1 || cooldown < 1 || cooldown > kBreakerMaxTick - 1)
    throw std::invalid_argument("breaker_observe: threshold >= 1, cooldown in [1, 2^31 - 2]");
  const bool aligned = !(st & 15u);
  const dim3 grid(br_grid(K)), block(kBrThreads);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(aligned ? breaker_observe_bad_kernel<true> : breaker_observe_bad_kernel<false>, grid, block, 0, s,
                     (const int*)st, (const int*)actor, K, trip_mask, (unsigned long long*)obs, (uint32_t*)touched,
                     (unsigned long long*)ctr, (uint32_t)n);
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(aligned ? breaker_observe_ok_kernel<true> : breaker_observe_ok_kernel<false>, grid, block, 0, s,
                     (const int*)st, (const int*)actor, K, (const uint64_t*)word, (unsigned long long*)obs,
                     (uint32_t*)touched, (unsigned long long*)ctr, (uint32_t)n);
  PT_HIP_CHECK(hipGetLastError());
  const int64_t want = (n + kBrThreads - 1) / kBrThreads;
  hipLaunchKernelGGL(breaker_step_kernel, dim3((unsigned)(want < kBrStepBlocks ? want : kBrStepBlocks)), block, 0, s,
                     (uint64_t*)word, (unsigned long long*)obs, (const uint32_t*)touched, (unsigned long long*)ctr,
                     (uint32_t)n, now, threshold, cooldown);
  PT_HIP_CHECK(hipGetLastError());
}

void launch_breaker_clear(uintptr_t word, uintptr_t obs, uintptr_t probe, uintptr_t ctr, int64_t n, uintptr_t stream) {
  if (n < 1 || n > kBreakerMaxActors) throw std::invalid_argument("breaker_clear: n must be in [1, 2^28]");
  if (!word || !obs || !probe || !ctr || (word | obs | probe | ctr) & 7u)
    throw std::invalid_argument("breaker_clear: null or misaligned table");
  const int64_t want = (n + kBrThreads - 1) / kBrThreads;
  hipLaunchKernelGGL(breaker_clear_kernel, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(kBrThreads), 0,
                     as_stream(stream), (uint64_t*)word, (unsigned long long*)obs, (unsigned long long*)probe,
                     (unsigned long long*)ctr, (uint32_t)n);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
