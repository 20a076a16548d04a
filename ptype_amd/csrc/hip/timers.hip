// Timer queue (timers.hpp has the record, run-descriptor and control-line layout;
// ops/timers.py the wrapper and the numpy model).
//
// Schedule is a stable counting sort of the accepted rows by delay, straight into the ring:
//
//   timer_count_kernel  launch 1 (a delay column only): one block per tile of kCompactTile
//                       rows (compact.hpp's tile: dwordx4 loads, scalar loads for a view that
//                       is not 16-byte aligned), a histogram over horizon + 1 bins in LDS --
//                       bin 0 is "refused", bin d the delay d -- written to hist[tile][bin]
//   timer_scan_kernel   launch 2, one block of 1024 threads, 1024 / horizon of them per bin,
//                       each with a chunk of the tiles: the exclusive prefix over the tiles,
//                       in place, and the bins' totals scanned into off[0 .. horizon + 1] in
//                       workspace; K, max_delay, the control words the call found and
//                       `refused` as it will be after the call go to the scratch
//                       line, which the host reads before it files anything.  A uniform
//                       delay has one bin: no column, no histogram, no launch 1
//   timer_file_kernel   launch 3, one block per tile: a wave walks its 1024 contiguous rows
//                       in groups of 64; the rows of a group with equal bins find each other
//                       with match_bits (sort_common.hpp), the lowest lane of each bumps the
//                       wave's LDS count of the bin and hands the old value to its peers: a
//                       row's rank inside its (tile, bin) in row order, without an atomic.
//                       The tile's rows are then listed by (bin, row) in LDS, so consecutive
//                       quads of lanes write consecutive tickets of a bin: four lanes per
//                       record, each one 16-byte quarter, at ticket
//                       head + off[d] + prefix[tile][d] + rank.  The last block copies off
//                       into the run's descriptor and commits head, runs_head and refused
//
// Tick:
//
//   timer_due_kernel    one block: now + 1; per live run its due segment (first ticket and
//                       length) from the descriptor alone, an exclusive scan of the lengths
//                       into seg_first[], n_due to the scratch line; retires the leading
//                       finished runs and moves both tails (not without `commit`: a look at
//                       the next tick that changes no control word)
//   timer_take_kernel   output-centric: a wave owns 64 consecutive output rows, finds the
//                       segment of its first one with a ballot search over seg_first and
//                       walks on from there; four lanes per record, the ticket check, SoA
//                       columns out.  It reads segments and due records only
//
// The order of the launches on the stream is the only synchronisation: no block waits for
// another one, no atomic goes to HBM (the torn count of a ring that is not intact aside),
// every store is a plain vector store, and every ring index is masked by entries - 1.
#include "compact.hpp"
#include "sort_common.hpp"
#include "timers.hpp"

namespace ptype {

constexpr int kTmrBins = (int)kTmrMaxHorizon + 1;
constexpr int kTmrWaveRows = kCompactTile / kCompactWaves;  // a wave's contiguous rows of a tile (1024)
constexpr int kTmrGroups = kTmrWaveRows / kWave;            // walked in groups of 64 (16)
constexpr int kTmrScanThreads = (int)kTmrMaxHorizon;
constexpr int kTmrTakeRows = 256;                           // output rows per block of the take

__device__ __forceinline__ unsigned timer_bin(int d, unsigned H) { return (unsigned)(d - 1) < H ? (unsigned)d : 0u; }

// Exclusive prefix of v over the threads of a block of W waves; *total: the block's sum.
template <int W>
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* __restrict__ wave_sum, unsigned* total) {
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const unsigned incl = wave_incl_scan(v);
  if (lane == kWave - 1) wave_sum[wave] = incl;
  __syncthreads();
  unsigned below = 0, all = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const unsigned s = wave_sum[w];
    if (w < (int)wave) below += s;
    all += s;
  }
  *total = all;
  return below + incl - v;
}

// One component of a wave's load into the LDS histogram (called by all 64 lanes; `ok`: the row is
// inside the batch).  Same-address LDS atomics are served one at a time, so when every row of the
// component has the same delay -- a column of one delay, or of a few in a period of 2 or 4 rows, a
// lane's rows being 4 apart -- the lowest lane adds them all at once.
__device__ __forceinline__ void timer_count_add(unsigned* __restrict__ bins, bool ok, int d, unsigned H) {
  const uint64_t act = __ballot(ok);
  if (!act) return;  // (wave-uniform)
  const unsigned bin = timer_bin(d, H);
  const int leader = __builtin_ctzll(act);
  const unsigned first = (unsigned)__shfl((int)bin, leader);
  if (__ballot(ok && bin == first) == act) {
    if ((int)lane_id() == leader) atomicAdd(&bins[first], (unsigned)__popcll(act));
  } else if (ok) {
    atomicAdd(&bins[bin], 1u);
  }
}

template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void timer_count_kernel(const int* __restrict__ delay, int64_t M,
                                                                       unsigned H, uint32_t* __restrict__ hist) {
  __shared__ unsigned bins[kTmrBins];
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tile = blockIdx.x;
  for (unsigned b = threadIdx.x; b <= H; b += kCompactThreads) bins[b] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kCompactLoads; ++j) {
    const int64_t i = compact_elem(tile, j, wave, lane);
    const int4 v = compact_load4<VEC>(delay, i, M);
    timer_count_add(bins, i < M, v.x, H);
    timer_count_add(bins, i + 1 < M, v.y, H);
    timer_count_add(bins, i + 2 < M, v.z, H);
    timer_count_add(bins, i + 3 < M, v.w, H);
  }
  __syncthreads();
  uint32_t* out = hist + tile * (int64_t)(H + 1);
  for (unsigned b = threadIdx.x; b <= H; b += kCompactThreads) out[b] = bins[b];
}

// `hist` null: every row has the delay `uniform`.
__global__ __launch_bounds__(kTmrScanThreads) void timer_scan_kernel(uint32_t* __restrict__ hist, unsigned tiles,
                                                                      unsigned H, int uniform, int64_t M,
                                                                      uint32_t* __restrict__ off,
                                                                      const uint64_t* __restrict__ ctrl,
                                                                      uint64_t* __restrict__ scratch) {
  __shared__ unsigned wave_sum[kTmrScanThreads / kWave];
  __shared__ unsigned chunk_sum[kTmrScanThreads];
  __shared__ unsigned max_delay;
  // the block's threads are C = 1024 / H chunks of H: thread t walks the bin (t % H) + 1 over the
  // tiles of chunk t / H -- first their sum, then, from the sums of the chunks below, the prefix in
  // place, eight independent loads at a time
  const unsigned t = threadIdx.x, b = t & (H - 1), chunk = t / H, C = kTmrScanThreads / H, bin = t + 1;
  const unsigned per = (tiles + C - 1) / C, stride = H + 1;
  const unsigned k0 = chunk * per < tiles ? chunk * per : tiles, k1 = k0 + per < tiles ? k0 + per : tiles;
  if (t == 0) max_delay = 0;
  unsigned mine = 0;
  if (hist && C > 1) {
    const uint32_t* p = hist + (size_t)k0 * stride + b + 1;
#pragma unroll 8
    for (unsigned k = k0; k < k1; ++k, p += stride) mine += *p;
  }
  chunk_sum[t] = mine;
  __syncthreads();
  unsigned total = 0;
  if (hist) {
    unsigned run = 0;
    if (C > 1) {
      for (unsigned c = 0; c < C; ++c) {
        const unsigned s = chunk_sum[c * H + b];
        if (c < chunk) run += s;
        total += s;
      }
    }
    uint32_t* p = hist + (size_t)k0 * stride + b + 1;
    unsigned k = k0;
    for (; k + 8 <= k1; k += 8, p += 8 * stride) {
      unsigned c[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) c[j] = p[j * stride];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[j * stride] = run;
        run += c[j];
      }
    }
    for (; k < k1; ++k, p += stride) {
      const unsigned c = *p;
      *p = run;
      run += c;
    }
    if (C == 1) total = run;
    if (chunk != 0) total = 0;  // (threads 0 .. H - 1 hold their bin's total)
  } else if (t < H && (unsigned)uniform == bin) {
    total = (unsigned)M;
  }
  unsigned K;
  const unsigned below = block_excl_scan<kTmrScanThreads / kWave>(total, wave_sum, &K);
  if (total) atomicMax(&max_delay, bin);  // (LDS; set to 0 before the scan's barrier)
  if (t < H) off[bin + 1] = below + total;
  if (t == 0) off[0] = off[1] = 0;
  __syncthreads();
  if (t == 0) {
    scratch[kTmrSK] = K;
    scratch[kTmrSRefused] = ctrl[kTmrRefused] + ((uint64_t)M - K);
    scratch[kTmrSMaxDelay] = max_delay;
    scratch[kTmrSHead] = ctrl[kTmrHead];
    scratch[kTmrSRunsHead] = ctrl[kTmrRunsHead];
    scratch[kTmrSNow] = ctrl[kTmrNow];
  }
}

struct TimerCols {  // by value
  const int* actor;
  const int16_t* method_col;
  unsigned method_uniform;
  const int64_t* a0;
  const int64_t* a1;
  const int64_t* a2;
  uint64_t tag;
};

// Lane `part` of a record's quad stores words 2 * part and 2 * part + 1 of row i's record.
__device__ __forceinline__ void timer_store_quarter(const TimerCols& c, int64_t i, unsigned d, uint64_t t, uint64_t now,
                                                    unsigned part, uint64_t* __restrict__ ring, uint64_t entries) {
  ulonglong2 w;
  if (part == 0) {
    w.x = t + 1ull;
    w.y = now + d;
  } else if (part == 1) {
    const unsigned m = c.method_col ? (unsigned)(uint16_t)c.method_col[i] : (c.method_uniform & 0xffffu);
    w.x = (uint64_t)(uint32_t)i | (uint64_t)d << 32;
    w.y = (uint64_t)(uint32_t)c.actor[i] | (uint64_t)m << 32;
  } else if (part == 2) {
    w.x = (uint64_t)c.a0[i];
    w.y = c.a1 ? (uint64_t)c.a1[i] : 0ull;
  } else {
    w.x = c.a2 ? (uint64_t)c.a2[i] : 0ull;
    w.y = c.tag;
  }
  *reinterpret_cast<ulonglong2*>(ring + (t & (entries - 1)) * kTmrRecordWords + part * 2) = w;
}

__global__ __launch_bounds__(kCompactThreads) void timer_file_kernel(
    const int* __restrict__ delay, int uniform, int64_t M, unsigned H, unsigned log_bits,
    const uint32_t* __restrict__ hist, const uint32_t* __restrict__ off, TimerCols cols, uint64_t* __restrict__ ring,
    uint64_t entries, uint64_t* __restrict__ runs, uint64_t n_runs, uint64_t* __restrict__ ctrl,
    const uint64_t* __restrict__ scratch) {
  __shared__ unsigned cnt[kCompactWaves][kTmrBins];  // per wave and bin: rows, then the first listed place
  __shared__ unsigned gdelta[kTmrBins];              // per bin: place in the run minus place in the tile's list
  __shared__ unsigned sel[kCompactTile];             // the tile's rows by (bin, row): row | bin << 16
  __shared__ unsigned wave_sum[kCompactWaves];
  __shared__ unsigned n_refused;
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave, part = threadIdx.x & 3u;
  const int64_t tile = blockIdx.x, row0 = tile * kCompactTile;
  const bool last = tile == (int64_t)gridDim.x - 1;
  const uint64_t K = scratch[kTmrSK], head = scratch[kTmrSHead], now = scratch[kTmrSNow];
  const unsigned rows = M - row0 < kCompactTile ? (unsigned)(M - row0) : (unsigned)kCompactTile;

  if (K != 0 && !delay) {
    // one delay (valid, or K were 0): the run is the batch in row order
    for (unsigned k = threadIdx.x >> 2; k < rows; k += kCompactThreads / 4)
      timer_store_quarter(cols, row0 + k, (unsigned)uniform, head + (uint64_t)(row0 + k), now, part, ring, entries);
  } else if (K != 0) {
    for (unsigned b = threadIdx.x; b < kCompactWaves * (unsigned)kTmrBins; b += kCompactThreads) (&cnt[0][0])[b] = 0;
    __syncthreads();
    unsigned kr[kTmrGroups];  // bin | rank within the wave's rows of that bin << 16
#pragma unroll
    for (int g = 0; g < kTmrGroups; ++g) {
      const unsigned k = wave * kTmrWaveRows + g * kWave + lane;
      const bool ok = k < rows;
      const unsigned bin = ok ? timer_bin(delay[row0 + k], H) : 0u;
      const uint64_t peers = match_bits(bin, log_bits, __ballot(ok));
      const unsigned below = mbcnt64(peers);
      const int leader = peers ? __builtin_ctzll(peers) : 0;
      unsigned old = 0;
      if (ok && below == 0) {
        old = cnt[wave][bin];
        cnt[wave][bin] = old + (unsigned)__popcll(peers);
      }
      kr[g] = bin | ((unsigned)__shfl((int)old, leader) + below) << 16;
    }
    __syncthreads();
    // thread t owns the bins [t * P, t * P + P): the waves' counts become each wave's first place in
    // the tile's list, which is ordered by (bin, wave, rank), i.e. by (bin, row)
    const unsigned P = (H + 1 + kCompactThreads - 1) / kCompactThreads;
    const unsigned b0 = threadIdx.x * P, b1 = b0 + P < H + 1 ? b0 + P : H + 1;
    unsigned mine = 0;
    for (unsigned b = b0; b < b1; ++b)
#pragma unroll
      for (int w = 0; w < kCompactWaves; ++w) mine += cnt[w][b];
    unsigned all;
    unsigned place = block_excl_scan<kCompactWaves>(mine, wave_sum, &all);
    const uint32_t* prefix = hist + tile * (int64_t)(H + 1);
    for (unsigned b = b0; b < b1; ++b) {
      gdelta[b] = off[b] + prefix[b] - place;
#pragma unroll
      for (int w = 0; w < kCompactWaves; ++w) {
        const unsigned c = cnt[w][b];
        cnt[w][b] = place;
        place += c;
      }
      if (b == 0) n_refused = place;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < kTmrGroups; ++g) {
      const unsigned k = wave * kTmrWaveRows + g * kWave + lane;
      const unsigned bin = kr[g] & 0xffffu;
      if (k < rows) sel[cnt[wave][bin] + (kr[g] >> 16)] = k | bin << 16;
    }
    __syncthreads();
    for (unsigned k = n_refused + (threadIdx.x >> 2); k < rows; k += kCompactThreads / 4) {
      const unsigned e = sel[k], bin = e >> 16;
      timer_store_quarter(cols, row0 + (e & 0xffffu), bin, head + (uint64_t)(k + gdelta[bin]), now, part, ring,
                          entries);
    }
  }

  if (last) {
    const uint64_t q = scratch[kTmrSRunsHead];
    uint64_t* desc = runs + (q & (n_runs - 1)) * (uint64_t)timer_desc_words(H);
    if (K != 0) {
      uint32_t* o = reinterpret_cast<uint32_t*>(desc + kTmrHeaderWords);
      for (unsigned j = threadIdx.x; j < H + 2; j += kCompactThreads) o[j] = off[j];
    }
    if (threadIdx.x == 0) {
      if (K != 0) {
        desc[kTmrT0] = now;
        desc[kTmrBase] = head;
        desc[kTmrN] = K;
        desc[kTmrMaxDelay] = scratch[kTmrSMaxDelay];
        desc[kTmrSeq] = q + 1ull;
        ctrl[kTmrHead] = head + K;
        ctrl[kTmrRunsHead] = q + 1ull;
      }
      ctrl[kTmrRefused] = scratch[kTmrSRefused];
    }
  }
}

__global__ __launch_bounds__(256) void timer_due_kernel(const uint64_t* __restrict__ runs, uint64_t n_runs, unsigned H,
                                                        uint64_t* __restrict__ ctrl, uint64_t* __restrict__ scratch,
                                                        uint32_t* __restrict__ seg_first,
                                                        uint64_t* __restrict__ seg_ticket, int commit) {
  __shared__ unsigned wave_sum[256 / kWave];
  __shared__ unsigned first_live;
  const uint64_t now = ctrl[kTmrNow] + 1ull, head = ctrl[kTmrHead], rh = ctrl[kTmrRunsHead], rt = ctrl[kTmrRunsTail];
  const uint64_t delivered = ctrl[kTmrDelivered];
  const uint64_t dw = (uint64_t)timer_desc_words(H);
  const unsigned live = rh - rt < n_runs ? (unsigned)(rh - rt) : (unsigned)n_runs;  // (the workspace's size)
  const unsigned per = (live + 255u) / 256u;
  const unsigned j0 = threadIdx.x * per, j1 = j0 + per < live ? j0 + per : live;
  if (threadIdx.x == 0) first_live = live;
  unsigned mine = 0, my_first = live;
  for (unsigned j = j0; j < j1; ++j) {
    const uint64_t* desc = runs + ((rt + j) & (n_runs - 1)) * dw;
    const uint64_t t0 = desc[kTmrT0], d = now - t0;
    if (d >= 1 && d <= H) {
      const uint32_t* o = reinterpret_cast<const uint32_t*>(desc + kTmrHeaderWords);
      mine += o[d + 1] - o[d];
    }
    if (now < t0 + desc[kTmrMaxDelay] && my_first == live) my_first = j;
  }
  unsigned total;
  unsigned first = block_excl_scan<256 / kWave>(mine, wave_sum, &total);  // (its barrier: first_live is set)
  if (my_first < live) atomicMin(&first_live, my_first);                 // (LDS)
  for (unsigned j = j0; j < j1; ++j) {
    const uint64_t* desc = runs + ((rt + j) & (n_runs - 1)) * dw;
    const uint64_t d = now - desc[kTmrT0];
    unsigned len = 0;
    uint64_t ticket = desc[kTmrBase];
    if (d >= 1 && d <= H) {
      const uint32_t* o = reinterpret_cast<const uint32_t*>(desc + kTmrHeaderWords);
      len = o[d + 1] - o[d];
      ticket += o[d];
    }
    seg_first[j] = first;
    seg_ticket[j] = ticket;
    first += len;
  }
  __syncthreads();  // (every thread has read the control words; first_live is final)
  if (threadIdx.x == 0) {
    seg_first[live] = total;
    scratch[kTmrSDue] = total;
    scratch[kTmrSSegs] = live;
    if (commit) {
      const uint64_t nrt = rt + first_live;
      ctrl[kTmrNow] = now;
      ctrl[kTmrDelivered] = delivered + total;
      ctrl[kTmrRunsTail] = nrt;
      ctrl[kTmrTail] = nrt < rh ? runs[(nrt & (n_runs - 1)) * dw + kTmrBase] : head;
    }
  }
}

__global__ __launch_bounds__(kTmrTakeRows) void timer_take_kernel(
    const uint64_t* __restrict__ ring, uint64_t entries, uint64_t* __restrict__ ctrl,
    const uint32_t* __restrict__ seg_first, const uint64_t* __restrict__ seg_ticket, unsigned segs, int64_t n,
    int64_t* __restrict__ ticket, int* __restrict__ row, int* __restrict__ actor, int16_t* __restrict__ method,
    int* __restrict__ delay, int64_t* __restrict__ t0, int64_t* __restrict__ a0, int64_t* __restrict__ a1,
    int64_t* __restrict__ a2, int64_t* __restrict__ tag) {
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave, part = lane & 3u;
  const int64_t first = (int64_t)blockIdx.x * kTmrTakeRows + wave * kWave;  // the wave's first output row
  if (first >= n) return;                                                    // (wave-uniform)
  // the segment of the wave's first row: the last one that starts at or before it (seg_first is
  // ascending and starts at 0, so the ballots are runs of ones and then zeros)
  unsigned at_or_before = 0;
  for (unsigned b = 0; b < segs; b += kWave) {
    const unsigned j = b + lane;
    const uint64_t m = __ballot(j < segs && (int64_t)seg_first[j] <= first);
    at_or_before += (unsigned)__popcll(m);
    if (m != ~0ull) break;
  }
  unsigned j = at_or_before - 1u;
#pragma unroll
  for (int it = 0; it < kWave / 16; ++it) {
    const int64_t o = first + it * 16 + (lane >> 2);
    const bool ok = o < n;
    ulonglong2 w = {0ull, 0ull};
    uint64_t t = 0;
    if (ok) {
      while (j + 1 < segs && (int64_t)seg_first[j + 1] <= o) ++j;  // (empty segments are stepped over)
      t = seg_ticket[j] + (uint64_t)(o - (int64_t)seg_first[j]);
      w = *reinterpret_cast<const ulonglong2*>(ring + (t & (entries - 1)) * kTmrRecordWords + part * 2);
    }
    const int d = __shfl((int)(uint32_t)(w.x >> 32), (int)((lane & ~3u) | 1u));  // the quad's delay
    if (!ok) continue;
    if (part == 0) {
      if (w.x != t + 1ull) atomicAdd((unsigned long long*)&ctrl[kTmrTorn], 1ull);  // (never, for an intact ring)
      ticket[o] = (int64_t)t;
      t0[o] = (int64_t)(w.y - (uint64_t)(uint32_t)d);
    } else if (part == 1) {
      row[o] = (int)(uint32_t)w.x;
      delay[o] = d;
      actor[o] = (int)(uint32_t)w.y;
      method[o] = (int16_t)(uint16_t)(w.y >> 32);
    } else if (part == 2) {
      a0[o] = (int64_t)w.x;
      a1[o] = (int64_t)w.y;
    } else {
      a2[o] = (int64_t)w.x;
      tag[o] = (int64_t)w.y;
    }
  }
}

int64_t timer_tile() { return kCompactTile; }

static unsigned log2_exact(int64_t v) {
  unsigned l = 0;
  while ((1ll << l) < v) ++l;
  return l;
}

static void timer_check_queue(const char* who, uintptr_t ring, uintptr_t runs, uintptr_t ctrl, uintptr_t scratch,
                              int64_t entries, int64_t horizon, int64_t n_runs) {
  const std::string w(who);
  if (entries < kTmrMinEntries || entries > kTmrMaxEntries || (entries & (entries - 1)))
    throw std::invalid_argument(w + ": entries must be a power of two in [64, 2^24]");
  if (horizon < kTmrMinHorizon || horizon > kTmrMaxHorizon || (horizon & (horizon - 1)))
    throw std::invalid_argument(w + ": horizon must be a power of two in [16, 1024]");
  if (n_runs < kTmrMinRuns || n_runs > kTmrMaxRuns || (n_runs & (n_runs - 1)))
    throw std::invalid_argument(w + ": runs must be a power of two in [4, 4096]");
  if (!ring || !runs || !ctrl || !scratch || (ring & 15u) || ((runs | ctrl | scratch) & 7u))
    throw std::invalid_argument(w + ": null or misaligned ring / run table / control line / scratch line");
}

// Launches 1 and 2 of a Schedule.  `delay`: an int32[M] column, or null for the delay `uniform` in
// every row.  `hist`: hist_words u32 of workspace, at least ceil(M / tile) * (horizon + 1) with a
// column; `off`: horizon + 2 u32.  Afterwards the scratch line holds K, the refused count and
// max_delay of the call and the head / runs_head / now it found; nothing of the queue is written.
void launch_timer_count(uintptr_t delay, int64_t uniform, int64_t M, uintptr_t ctrl, uintptr_t scratch,
                        int64_t horizon, uintptr_t hist, int64_t hist_words, uintptr_t off, uintptr_t stream) {
  if (M < 0 || M > 0x7fffffffll) throw std::invalid_argument("timer_count: M must be in [0, 2^31 - 1]");
  if (horizon < kTmrMinHorizon || horizon > kTmrMaxHorizon || (horizon & (horizon - 1)))
    throw std::invalid_argument("timer_count: horizon must be a power of two in [16, 1024]");
  if (!ctrl || !scratch || !off || ((ctrl | scratch) & 7u) || (off & 3u) || (delay & 3u) || (hist & 3u))
    throw std::invalid_argument("timer_count: null or misaligned control line / scratch line / workspace / column");
  const unsigned tiles = (unsigned)((M + kCompactTile - 1) / kCompactTile);
  const bool col = delay != 0 && M > 0;
  if (col && (!hist || hist_words < (int64_t)tiles * (horizon + 1)))
    throw std::invalid_argument("timer_count: the histogram workspace is too small");
  hipStream_t s = as_stream(stream);
  const unsigned H = (unsigned)horizon;
  if (col) {
    hipLaunchKernelGGL((delay & 15u) == 0 ? timer_count_kernel<true> : timer_count_kernel<false>, dim3(tiles),
                       dim3(kCompactThreads), 0, s, (const int*)delay, M, H, (uint32_t*)hist);
    PT_HIP_CHECK(hipGetLastError());
  }
  // without a column: a delay outside [1, horizon] matches no bin, every row is refused
  const int u = delay ? 0 : (uniform >= 1 && uniform <= horizon ? (int)uniform : 0);
  hipLaunchKernelGGL(timer_scan_kernel, dim3(1), dim3(kTmrScanThreads), 0, s, col ? (uint32_t*)hist : nullptr, tiles,
                     H, u, M, (uint32_t*)off, (const uint64_t*)ctrl, (uint64_t*)scratch);
  PT_HIP_CHECK(hipGetLastError());
}

// Launch 3, with the arguments and the workspace of the count before it.  The caller has read the
// scratch line and found room: head + K - tail <= entries and, for K > 0, a free run descriptor.
void launch_timer_file(uintptr_t delay, int64_t uniform, int64_t M, uintptr_t actor, uintptr_t method_col,
                       uint32_t method_uniform, uintptr_t a0, uintptr_t a1, uintptr_t a2, int64_t tag, uintptr_t ring,
                       uintptr_t runs, uintptr_t ctrl, uintptr_t scratch, int64_t entries, int64_t horizon,
                       int64_t n_runs, uintptr_t hist, int64_t hist_words, uintptr_t off, uintptr_t stream) {
  if (M < 0 || M > 0x7fffffffll) throw std::invalid_argument("timer_file: M must be in [0, 2^31 - 1]");
  timer_check_queue("timer_file", ring, runs, ctrl, scratch, entries, horizon, n_runs);
  if (!off || (off & 3u) || (hist & 3u)) throw std::invalid_argument("timer_file: null or misaligned workspace");
  if (M > 0 && (!actor || !a0)) throw std::invalid_argument("timer_file: null column");
  if ((delay | actor) & 3u || (a0 | a1 | a2) & 7u || method_col & 1u)
    throw std::invalid_argument("timer_file: a column is not aligned to its element size");
  const unsigned tiles = M ? (unsigned)((M + kCompactTile - 1) / kCompactTile) : 1u;
  const bool col = delay != 0 && M > 0;
  if (col && (!hist || hist_words < (int64_t)tiles * (horizon + 1)))
    throw std::invalid_argument("timer_file: the histogram workspace is too small");
  const int u = delay ? 0 : (uniform >= 1 && uniform <= horizon ? (int)uniform : 0);
  const TimerCols cols{(const int*)actor, (const int16_t*)method_col, method_uniform, (const int64_t*)a0,
                       (const int64_t*)a1,  (const int64_t*)a2,       (uint64_t)tag};
  hipLaunchKernelGGL(timer_file_kernel, dim3(tiles), dim3(kCompactThreads), 0, as_stream(stream),
                     col ? (const int*)delay : nullptr, u, M, (unsigned)horizon, log2_exact(horizon) + 1u,
                     (const uint32_t*)hist, (const uint32_t*)off, cols, (uint64_t*)ring, (uint64_t)entries,
                     (uint64_t*)runs, (uint64_t)n_runs, (uint64_t*)ctrl, (const uint64_t*)scratch);
  PT_HIP_CHECK(hipGetLastError());
}

// One tick: now + 1, the live runs' due segments into seg_first (runs + 1 u32) and seg_ticket (runs
// u64), n_due and the number of segments into the scratch line.  Without `commit` no control word
// changes: a look at the next tick.
void launch_timer_due(uintptr_t runs, uintptr_t ctrl, uintptr_t scratch, int64_t horizon, int64_t n_runs,
                      uintptr_t seg_first, uintptr_t seg_ticket, bool commit, uintptr_t stream) {
  // (the due launch touches no ring: an aligned placeholder and the smallest size pass that part of the check)
  timer_check_queue("timer_due", 16, runs, ctrl, scratch, kTmrMinEntries, horizon, n_runs);
  if (!seg_first || !seg_ticket || (seg_first & 3u) || (seg_ticket & 7u))
    throw std::invalid_argument("timer_due: null or misaligned segment workspace");
  hipLaunchKernelGGL(timer_due_kernel, dim3(1), dim3(256), 0, as_stream(stream), (const uint64_t*)runs,
                     (uint64_t)n_runs, (unsigned)horizon, (uint64_t*)ctrl, (uint64_t*)scratch, (uint32_t*)seg_first,
                     (uint64_t*)seg_ticket, commit ? 1 : 0);
  PT_HIP_CHECK(hipGetLastError());
}

// The n records due (n and segs as the host read them from the scratch line after the tick's due
// launch) into the ten columns, each n elements.
void launch_timer_take(uintptr_t ring, uintptr_t ctrl, int64_t entries, uintptr_t seg_first, uintptr_t seg_ticket,
                       int64_t segs, int64_t n_runs, int64_t n, uintptr_t ticket, uintptr_t row, uintptr_t actor,
                       uintptr_t method, uintptr_t delay, uintptr_t t0, uintptr_t a0, uintptr_t a1, uintptr_t a2,
                       uintptr_t tag, uintptr_t stream) {
  if (n <= 0) return;
  if (entries < kTmrMinEntries || entries > kTmrMaxEntries || (entries & (entries - 1)))
    throw std::invalid_argument("timer_take: entries must be a power of two in [64, 2^24]");
  if (!ring || !ctrl || (ring & 15u) || (ctrl & 7u))
    throw std::invalid_argument("timer_take: null or misaligned ring / control line");
  if (n > entries || segs < 1 || segs > n_runs || n_runs > kTmrMaxRuns)
    throw std::invalid_argument("timer_take: n must be in [1, entries] and segs in [1, runs]");
  if (!seg_first || !seg_ticket || !ticket || !row || !actor || !method || !delay || !t0 || !a0 || !a1 || !a2 || !tag)
    throw std::invalid_argument("timer_take: null column or segment workspace");
  const unsigned blocks = (unsigned)((n + kTmrTakeRows - 1) / kTmrTakeRows);
  hipLaunchKernelGGL(timer_take_kernel, dim3(blocks), dim3(kTmrTakeRows), 0, as_stream(stream), (const uint64_t*)ring,
                     (uint64_t)entries, (uint64_t*)ctrl, (const uint32_t*)seg_first, (const uint64_t*)seg_ticket,
                     (unsigned)segs, n, (int64_t*)ticket, (int*)row, (int*)actor, (int16_t*)method, (int*)delay,
                     (int64_t*)t0, (int64_t*)a0, (int64_t*)a1, (int64_t*)a2, (int64_t*)tag);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
