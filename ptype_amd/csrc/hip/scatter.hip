// Call scatter kernels (scatter.hpp has the rules; ops/scatter.py the wrapper and the
// numpy reference).  Four launches per expansion, the host reads the counters after
// the third:
//
//   scatter_count_kernel<RULE>   a block per tile of kScatterQTile questions: n[q], the
//                                tile-local exclusive prefix of n into first[q], the tile's
//                                sum and its out-of-range group ids
//   scatter_scan_kernel          one block: the tile sums become tile bases (wave-shuffle
//                                scans, a carry between chunks of 1024 tiles); the total and
//                                oob go to the counters
//   scatter_first_kernel         first[q] += its tile's base
//   scatter_expand_kernel<RULE>  a block per tile of kScatterTile OUTPUT rows, so one
//                                question of millions of rows is spread over as many blocks
//                                as any other million rows
//
// Every u64 add saturates at 2^64 - 1: a total that does not fit is refused by the host
// (it exceeds any capacity), whatever the prefixes below it hold.  Placement needs no
// atomic: rows are in question order by construction.
//
// Expand: the block finds the owners of its first and last row (the last q with
// first[q] <= row: questions without rows share their successor's first and sort before
// it) by a 64-way search -- every lane of a wave probes one point of the range, a ballot
// narrows it 64 times per load -- then every question q in (q_lo, q_hi] with n[q] > 0
// writes q at its head's position in an LDS tile that holds -1 elsewhere and q_lo at
// position 0.  An inclusive max-scan over the tile (four positions per lane, a shuffle
// scan per wave, the eight segment maxima through LDS) gives every row its owner.  A tile
// without a head is all q_lo; zero-row questions never write.
//
// Tile layout as in gather.hip: 256 threads x kScatterQuads quads of 4 rows; quad j of
// wave w, lane l covers the tile's positions (j * 4 + w) * 256 + l * 4 + {0, 1, 2, 3}: one
// dwordx4 store per lane of actor and of group, two of each int64 column (the outputs are
// the wrapper's own buffers, 16-byte aligned at row 0).  The ragged last quad stores
// element by element.  A quad whose four rows have one owner loads its question once.
//
// Topics: a row's actor comes from the strided segment of its topic that holds it, so a
// quad also needs the last segment s with row_off[s] <= row_off[seg_off[g]] + k.  It
// searches once per question it meets (a lane-local bisection over the topic's segments)
// and then walks forward over segment ends: row_off is strictly increasing, every segment
// holds a row.  A tile that lies inside one question narrows the range first, for the whole
// block, to the segments of its first and last row with the 64-way search of the owners:
// a giant topic of a million segments costs a tile two ballot searches and its quads a
// bisection over at most 2048 segments.
//
// Queue subscriptions (QUEUES, a compile-time variant of the topics rule: a table without one
// launches the instantiations it always did).  After the rows of a topic's ordinary
// subscriptions comes one row per queue subscription of the topic.  A row with k >= the
// topic's ordinary rows is queue subscription j = q_off[g] + (k - ordinary rows); its members
// are the segments q_seg[j] .. q_seg[j + 1] - 1 (at most 1024: ten bisection steps), c =
// row_off[q_seg[j + 1]] - row_off[q_seg[j]] of them, and the row goes to member
// m = ((mix64(key[q]) >> 32) * c) >> 32, or (seq + q) % c by index (scatter.hpp).  Ordinary
// rows keep their path; a tile inside one question narrows over the ordinary segments only,
// and only when it starts in them (the queue rows of a question follow its ordinary rows).
#include "common.hpp"
#include "scatter.hpp"

#include <type_traits>

namespace ptype {

constexpr int kScatterThreads = 256;
constexpr int kScatterWaves = kScatterThreads / kWave;
constexpr int kScatterQPer = 4;                                    // questions per thread of the count pass
constexpr int kScatterQTile = kScatterThreads * kScatterQPer;      // 1024 questions
constexpr int kScatterQuads = 2;                                   // 4-row quads per thread and tile
constexpr int kScatterTile = kScatterThreads * kScatterQuads * 4;  // 2048 rows
constexpr int kScatterSegs = kScatterQuads * kScatterWaves;        // 256-row segments of a tile
constexpr int kScatterScanPer = 4;                                 // tile sums per thread and chunk of the scan

struct ScatterRule {
  // ranges
  uint64_t step;
  uint32_t n_actors, actor_base;
  int64_t first_lo;
  int has_lo;
  // members (topics: offsets = seg_off, G = the topics)
  const int64_t* offsets;
  const int* members;
  int64_t G, n_members;
  // topics
  const int64_t* row_off;
  const int* seg_start;
  const int* seg_stride;
  int64_t n_segs;  // (the ordinary segments: seg_off's bound)
};

// Topics with queue subscriptions (QUEUES): row_off / seg_start / seg_stride hold n_all >=
// n_segs segments.  The rule of the QUEUES kernels alone: the others keep their argument.
struct ScatterQueueRule : ScatterRule {
  const int64_t* q_off;
  const int64_t* q_seg;
  const int64_t* key;
  int64_t n_queues, n_all;
  uint64_t seq;
  int by_index;
};
template <bool QUEUES>
using ScatterRuleOf = std::conditional_t<QUEUES, ScatterQueueRule, ScatterRule>;

struct ScatterQuestions {
  const int* actor;
  const int64_t* a0;
  const int64_t* a1;
  const int64_t* a2;
  const int16_t* method;
};

struct ScatterOut {
  int* actor;
  int64_t* a0;
  int64_t* a1;
  int64_t* a2;
  int16_t* method;
  int* group;
};

__device__ __forceinline__ uint64_t scatter_sat_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s < a ? ~0ull : s;
}

// Inclusive saturating sum over the 64 lanes of a wave.
__device__ __forceinline__ uint64_t scatter_wave_scan(uint64_t v, unsigned lane) {
#pragma unroll
  for (unsigned o = 1; o < (unsigned)kWave; o <<= 1) {
    const uint64_t up = (uint64_t)__shfl_up((unsigned long long)v, o, kWave);
    if (lane >= o) v = scatter_sat_add(v, up);
  }
  return v;
}

// A segment index of the table read as one in [0, n_segs]: the launchers take the table's
// word for its own consistency, no kernel reads outside the arrays whatever it holds.
__device__ __forceinline__ int64_t scatter_seg_clamp(int64_t s, int64_t n_segs) {
  return s < 0 ? 0 : s > n_segs ? n_segs : s;
}

template <int RULE, bool QUEUES = false>
__global__ __launch_bounds__(kScatterThreads) void scatter_count_kernel(
    ScatterRuleOf<QUEUES> r, const int* __restrict__ q_actor, const int64_t* __restrict__ q_a0, int64_t Q, int* __restrict__ n,
    unsigned long long* __restrict__ first, unsigned long long* __restrict__ tsum, unsigned long long* __restrict__ toob) {
  __shared__ unsigned long long part[kScatterQPer * kScatterWaves];
  __shared__ unsigned oob_wave[kScatterWaves];
  const unsigned tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
  const int64_t qbase = (int64_t)blockIdx.x * kScatterQTile;

  uint64_t v[kScatterQPer], inc[kScatterQPer];
  unsigned n_oob = 0;
#pragma unroll
  for (int j = 0; j < kScatterQPer; ++j) {  // question j * 256 + tid of the tile: coalesced scalar loads
    const int64_t q = qbase + j * kScatterThreads + tid;
    v[j] = 0;
    if (q < Q) {
      if constexpr (RULE == kScatterRanges) {
        const int64_t t = q_a0[q];
        if (t > 0) v[j] = ((uint64_t)t - 1ull) / r.step + 1ull;
      } else if constexpr (RULE == kScatterMembers) {
        const int64_t g = q_actor[q];
        if (g >= 0 && g < r.G)
          v[j] = (uint64_t)(r.offsets[g + 1] - r.offsets[g]);
        else
          ++n_oob;
      } else {  // the topic's segment range, then the rows at its two ends
        const int64_t g = q_actor[q];
        if (g >= 0 && g < r.G) {
          const int64_t s0 = scatter_seg_clamp(r.offsets[g], r.n_segs), s1 = scatter_seg_clamp(r.offsets[g + 1], r.n_segs);
          if (s1 > s0) v[j] = (uint64_t)(r.row_off[s1] - r.row_off[s0]);
          if constexpr (QUEUES) {  // one row per queue subscription of the topic
            const int64_t j0 = scatter_seg_clamp(r.q_off[g], r.n_queues), j1 = scatter_seg_clamp(r.q_off[g + 1], r.n_queues);
            if (j1 > j0) v[j] += (uint64_t)(j1 - j0);
          }
        } else {
          ++n_oob;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kScatterQPer; ++j) {
    inc[j] = scatter_wave_scan(v[j], lane);
    if (lane == (unsigned)kWave - 1) part[j * kScatterWaves + wave] = inc[j];
  }
#pragma unroll
  for (int o = kWave / 2; o; o >>= 1) n_oob += (unsigned)__shfl_xor((int)n_oob, o, kWave);
  if (lane == 0) oob_wave[wave] = n_oob;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kScatterQPer; ++j) {
    const int64_t q = qbase + j * kScatterThreads + tid;
    uint64_t off = 0;
    for (int s = 0; s < j * kScatterWaves + (int)wave; ++s) off = scatter_sat_add(off, part[s]);
    if (q < Q) {
      n[q] = v[j] > 0x7fffffffull ? 0x7fffffff : (int)v[j];
      first[q] = scatter_sat_add(off, inc[j] - v[j]);
    }
  }
  if (tid == 0) {
    uint64_t sum = 0;
    for (int s = 0; s < kScatterQPer * kScatterWaves; ++s) sum = scatter_sat_add(sum, part[s]);
    tsum[blockIdx.x] = sum;
    toob[blockIdx.x] = (unsigned long long)oob_wave[0] + oob_wave[1] + oob_wave[2] + oob_wave[3];
  }
}
static_assert(kScatterWaves == 4, "the oob reduction reads four waves' partials");

// tsum: the tile sums in, the tile bases (their exclusive prefix) out.
__global__ __launch_bounds__(kScatterThreads) void scatter_scan_kernel(unsigned long long* __restrict__ tsum,
                                                                        const unsigned long long* __restrict__ toob,
                                                                        int64_t tiles,
                                                                        unsigned long long* __restrict__ ctr) {
  __shared__ unsigned long long wtot[kScatterWaves], woob[kScatterWaves];
  const unsigned tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
  uint64_t carry = 0, oob = 0;
  for (int64_t base = 0; base < tiles; base += kScatterThreads * kScatterScanPer) {  // (block-uniform)
    const int64_t i0 = base + (int64_t)tid * kScatterScanPer;
    uint64_t s[kScatterScanPer], t = 0;
#pragma unroll
    for (int c = 0; c < kScatterScanPer; ++c) {
      s[c] = i0 + c < tiles ? tsum[i0 + c] : 0ull;
      if (i0 + c < tiles) oob += toob[i0 + c];
      t = scatter_sat_add(t, s[c]);
    }
    const uint64_t x = scatter_wave_scan(t, lane);
    if (lane == (unsigned)kWave - 1) wtot[wave] = x;
    __syncthreads();
    uint64_t off = carry;
    for (unsigned w = 0; w < wave; ++w) off = scatter_sat_add(off, wtot[w]);
    off = scatter_sat_add(off, x - t);
#pragma unroll
    for (int c = 0; c < kScatterScanPer; ++c) {
      if (i0 + c < tiles) tsum[i0 + c] = off;
      off = scatter_sat_add(off, s[c]);
    }
#pragma unroll
    for (int w = 0; w < kScatterWaves; ++w) carry = scatter_sat_add(carry, wtot[w]);
    __syncthreads();  // wtot is rewritten by the next chunk
  }
#pragma unroll
  for (int o = kWave / 2; o; o >>= 1) oob += (uint64_t)__shfl_xor((unsigned long long)oob, o, kWave);
  if (lane == 0) woob[wave] = oob;
  __syncthreads();
  if (tid == 0) {
    ctr[0] = carry;
    ctr[1] = woob[0] + woob[1] + woob[2] + woob[3];
  }
}

__global__ __launch_bounds__(kScatterThreads) void scatter_first_kernel(unsigned long long* __restrict__ first,
                                                                         const unsigned long long* __restrict__ tbase,
                                                                         int64_t Q) {
  const int64_t q = (int64_t)blockIdx.x * kScatterThreads + threadIdx.x;
  if (q < Q) first[q] = scatter_sat_add(first[q], tbase[q / kScatterQTile]);
}

// The last q in [lo, Q) with first[q] <= row; first is non-decreasing and first[lo] <= row.
// Wave-uniform: every lane probes one point, the ballot picks the sub-range.
__device__ __forceinline__ int scatter_owner(const int64_t* __restrict__ first, int Q, int64_t row, int lo,
                                             unsigned lane) {
  int hi = Q;  // the first index whose first[] exceeds row lies in [lo, hi]
  while (lo < hi) {
    const int step = (hi - lo + kWave - 1) / kWave;
    const int64_t idx = (int64_t)lo + (int64_t)(lane + 1) * step - 1;
    const bool gt = idx >= hi || first[idx] > row;
    const uint64_t b = __ballot(gt);
    if (!b) {
      lo = hi;
      break;
    }
    const int f = __ffsll((unsigned long long)b) - 1;
    const int64_t top = (int64_t)lo + (int64_t)(f + 1) * step - 1;
    lo += f * step;
    hi = top < hi ? (int)top : hi;
  }
  return lo > 0 ? lo - 1 : 0;
}

// What a row needs of its question.
struct ScatterQ {
  int64_t first, a0, a1, a2;  // ranges: a2 = t; members and topics: a0 .. a2 the question's
  int64_t off;                // members: offsets[g]; topics: row_off[seg_off[g]]
  int s0, s1;                 // topics: the topic's segments [s0, s1)
  int16_t method;
};
// Topics with queue subscriptions: also the topic's ordinary rows, its first queue
// subscription, and what picks the member (mix64 of the key, or seq + q by index).
struct ScatterQueueQ : ScatterQ {
  int64_t nord, qj;
  uint64_t pick;
};
template <bool QUEUES>
using ScatterQOf = std::conditional_t<QUEUES, ScatterQueueQ, ScatterQ>;

// The segment a topics quad stands in: its rows [lo, hi) of row_off's space and its actors.
struct ScatterSeg {
  int s;
  int64_t lo, hi;
  int start, stride;
};

__device__ __forceinline__ void scatter_seg_load(const ScatterRule& r, int s, ScatterSeg* g) {
  g->s = s;
  g->lo = r.row_off[s], g->hi = r.row_off[s + 1];
  g->start = r.seg_start[s], g->stride = r.seg_stride[s];
}

// The last s in [lo, hi) with row_off[s] <= at (lo when there is none); 0 <= lo < hi <= n_segs.
__device__ __forceinline__ int scatter_seg_find(const ScatterRule& r, int lo, int hi, int64_t at) {
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (r.row_off[mid] <= at)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

template <int RULE, bool MCOL, bool QUEUES>
__device__ __forceinline__ ScatterQOf<QUEUES> scatter_question(const ScatterRuleOf<QUEUES>& r,
                                                               const ScatterQuestions& qs,
                                                               const int64_t* __restrict__ first, int q) {
  ScatterQOf<QUEUES> d{};
  d.first = first[q];
  if constexpr (RULE == kScatterRanges) {
    d.a2 = qs.a0[q];
  } else {
    const int64_t g = qs.actor[q];
    if constexpr (RULE == kScatterMembers) {
      d.off = g >= 0 && g < r.G ? r.offsets[g] : 0;
    } else if constexpr (QUEUES) {
      // (row_off holds n_all + 1 >= n_segs + 1 entries; a topic may have no ordinary segment, s0 == s1)
      const bool in = g >= 0 && g < r.G;
      d.s0 = in ? (int)scatter_seg_clamp(r.offsets[g], r.n_segs) : 0;
      d.s1 = in ? (int)scatter_seg_clamp(r.offsets[g + 1], r.n_segs) : 0;
      if (d.s1 < d.s0) d.s1 = d.s0;
      d.off = r.row_off[d.s0];
      d.nord = r.row_off[d.s1] - d.off;
      d.qj = in ? scatter_seg_clamp(r.q_off[g], r.n_queues) : 0;
      d.pick = r.by_index ? r.seq + (uint64_t)q : mix64((uint64_t)r.key[q]);
    } else {
      const bool in = g >= 0 && g < r.G;
      d.s0 = in ? (int)scatter_seg_clamp(r.offsets[g], r.n_segs) : 0;
      d.s1 = in ? (int)scatter_seg_clamp(r.offsets[g + 1], r.n_segs) : 0;
      if (d.s0 >= r.n_segs) d.s0 = (int)r.n_segs - 1;  // (a question without rows only: it owns none)
      if (d.s1 <= d.s0) d.s1 = d.s0 + 1;
      d.off = r.row_off[d.s0];
    }
    d.a0 = qs.a0[q];
    d.a1 = qs.a1 ? qs.a1[q] : 0;
    d.a2 = qs.a2 ? qs.a2[q] : 0;
  }
  if constexpr (MCOL) d.method = qs.method[q];
  return d;
}

// The actor a queue row goes to: queue subscription j of the table, picked by `pick`.
__device__ __forceinline__ int scatter_queue_actor(const ScatterQueueRule& r, int64_t j, uint64_t pick) {
  j = j < 0 ? 0 : j >= r.n_queues ? r.n_queues - 1 : j;  // (a row past the total only; n_queues >= 1)
  int64_t a = scatter_seg_clamp(r.q_seg[j], r.n_all), b = scatter_seg_clamp(r.q_seg[j + 1], r.n_all);
  a = a >= r.n_all ? r.n_all - 1 : a;  // (n_all >= 1)
  b = b <= a ? a + 1 : b;
  const int64_t lo = r.row_off[a];
  uint64_t c = (uint64_t)(r.row_off[b] - lo);  // 1 <= c <= 2^31 - 1
  c = c < 1 ? 1 : c > 0x7fffffffull ? 0x7fffffffull : c;  // (never taken: m stays inside the subscription's rows)
  const uint64_t m = r.by_index ? pick % c : ((pick >> 32) * c) >> 32;
  const int64_t at = lo + (int64_t)m;
  const int s = scatter_seg_find(r, (int)a, (int)b, at);
  return (int)((int64_t)r.seg_start[s] + (int64_t)r.seg_stride[s] * (at - r.row_off[s]));
}

template <int RULE, bool MCOL, bool QUEUES = false>
__global__ __launch_bounds__(kScatterThreads) void scatter_expand_kernel(ScatterRuleOf<QUEUES> r, ScatterQuestions qs,
                                                                          const int64_t* __restrict__ first,
                                                                          const int* __restrict__ n, int Q,
                                                                          int64_t total, ScatterOut out) {
  __shared__ __attribute__((aligned(16))) int head[kScatterTile];
  __shared__ int segmax[kScatterSegs];
  const unsigned tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kScatterTile;
  if (row0 >= total) return;  // (block-uniform)
  const int rows = total - row0 < kScatterTile ? (int)(total - row0) : kScatterTile;

  const int q_lo = scatter_owner(first, Q, row0, 0, lane);
  const int q_hi = scatter_owner(first, Q, row0 + rows - 1, q_lo, lane);
#pragma unroll
  for (int j = 0; j < kScatterQuads; ++j) {
    const int p = (j * kScatterWaves + (int)wave) * (kWave * 4) + (int)lane * 4;
    *reinterpret_cast<int4*>(&head[p]) = make_int4(p == 0 ? q_lo : -1, -1, -1, -1);
  }
  // topics, a tile inside one question: the segments of its first and last row bound every quad's search
  int ts_lo = -1, ts_hi = -1;
  if constexpr (RULE == kScatterTopics) {
    if (q_lo == q_hi) {  // (block-uniform)
      const ScatterQOf<QUEUES> d = scatter_question<RULE, false, QUEUES>(r, qs, first, q_lo);
      int64_t at = d.off + (row0 - d.first);
      at = at < d.off ? d.off : at;
      // (QUEUES: a tile that starts in the question's queue rows holds no ordinary row; one that ends
      // in them finds the topic's last ordinary segment for its last row)
      bool narrow = true;
      if constexpr (QUEUES) narrow = at - d.off < d.nord;  // (block-uniform)
      if (narrow) {
        ts_lo = scatter_owner(r.row_off, d.s1, at, d.s0, lane);
        ts_lo = ts_lo < d.s0 ? d.s0 : ts_lo;
        ts_hi = scatter_owner(r.row_off, d.s1, at + rows - 1, ts_lo, lane);
        ts_hi = (ts_hi < ts_lo ? ts_lo : ts_hi) + 1;
      }
    }
  }
  __syncthreads();
  for (int q = q_lo + 1 + (int)tid; q <= q_hi; q += kScatterThreads) {
    if (n[q] > 0) {
      const int64_t pos = first[q] - row0;
      if (pos > 0 && pos < rows) head[pos] = q;
    }
  }
  __syncthreads();

  int own[kScatterQuads][4];
#pragma unroll
  for (int j = 0; j < kScatterQuads; ++j) {
    const int p = (j * kScatterWaves + (int)wave) * (kWave * 4) + (int)lane * 4;
    const int4 h = *reinterpret_cast<const int4*>(&head[p]);
    own[j][0] = h.x;
    own[j][1] = max(own[j][0], h.y);
    own[j][2] = max(own[j][1], h.z);
    own[j][3] = max(own[j][2], h.w);
    int x = own[j][3];
#pragma unroll
    for (unsigned o = 1; o < (unsigned)kWave; o <<= 1) {
      const int up = __shfl_up(x, o, kWave);
      if (lane >= o) x = max(x, up);
    }
    if (lane == (unsigned)kWave - 1) segmax[j * kScatterWaves + wave] = x;
    const int before = __shfl_up(x, 1, kWave);
    if (lane > 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) own[j][c] = max(own[j][c], before);
    }
  }
  __syncthreads();

#pragma unroll
  for (int j = 0; j < kScatterQuads; ++j) {
    const int seg = j * kScatterWaves + (int)wave;
    const int p = seg * (kWave * 4) + (int)lane * 4;
    if (p >= rows) continue;
    int carry = -1;
    for (int s = 0; s < seg; ++s) carry = max(carry, segmax[s]);

    int actor[4], group[4];
    int64_t a0[4], a1[4], a2[4];
    int16_t method[4];
    ScatterQOf<QUEUES> d{};
    ScatterSeg sg{};
    int have = -1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int q = max(own[j][c], carry);
      q = q < 0 ? 0 : q >= Q ? Q - 1 : q;  // (never taken: position 0 holds q_lo <= every owner < Q)
      const bool fresh = q != have;
      if (fresh) d = scatter_question<RULE, MCOL, QUEUES>(r, qs, first, q), have = q;
      const int64_t row = row0 + p + c;
      const int64_t k = row - d.first;
      group[c] = q;
      method[c] = d.method;
      if constexpr (RULE == kScatterRanges) {
        actor[c] = (int)((r.actor_base + (uint32_t)row) % r.n_actors);
        a0[c] = k == 0 && r.has_lo ? r.first_lo : k * (int64_t)r.step;
        a1[c] = (k + 1) * (int64_t)r.step;
        a2[c] = d.a2;
      } else if constexpr (RULE == kScatterMembers) {
        int64_t at = d.off + k;
        at = at < 0 ? 0 : at >= r.n_members ? r.n_members - 1 : at;  // (a row past the total only)
        actor[c] = r.members[at];
        a0[c] = d.a0, a1[c] = d.a1, a2[c] = d.a2;
      } else {
        if constexpr (QUEUES) {
          if (k >= d.nord) {  // a queue row: they follow the question's ordinary rows
            actor[c] = scatter_queue_actor(r, d.qj + (k - d.nord), d.pick);
            a0[c] = d.a0, a1[c] = d.a1, a2[c] = d.a2;
            continue;
          }
        }
        const int64_t at = d.off + k;
        if (fresh) {  // one search per question of the quad ...
          const int lo = ts_lo >= 0 ? ts_lo : d.s0, hi = ts_lo >= 0 ? ts_hi : d.s1;
          scatter_seg_load(r, scatter_seg_find(r, lo, hi, at), &sg);
        }
        while (at >= sg.hi && sg.s + 1 < d.s1) scatter_seg_load(r, sg.s + 1, &sg);  // ... then a walk over segment ends
        actor[c] = (int)((int64_t)sg.start + (int64_t)sg.stride * (at - sg.lo));
        a0[c] = d.a0, a1[c] = d.a1, a2[c] = d.a2;
      }
    }
    const int64_t at = row0 + p;
    if (p + 4 <= rows) {
      *reinterpret_cast<int4*>(out.actor + at) = make_int4(actor[0], actor[1], actor[2], actor[3]);
      *reinterpret_cast<int4*>(out.group + at) = make_int4(group[0], group[1], group[2], group[3]);
      *reinterpret_cast<I64x2*>(out.a0 + at) = I64x2{a0[0], a0[1]};
      *reinterpret_cast<I64x2*>(out.a0 + at + 2) = I64x2{a0[2], a0[3]};
      if (out.a1) {
        *reinterpret_cast<I64x2*>(out.a1 + at) = I64x2{a1[0], a1[1]};
        *reinterpret_cast<I64x2*>(out.a1 + at + 2) = I64x2{a1[2], a1[3]};
      }
      if (out.a2) {
        *reinterpret_cast<I64x2*>(out.a2 + at) = I64x2{a2[0], a2[1]};
        *reinterpret_cast<I64x2*>(out.a2 + at + 2) = I64x2{a2[2], a2[3]};
      }
      if constexpr (MCOL)
        *reinterpret_cast<I16x4*>(out.method + at) = I16x4{method[0], method[1], method[2], method[3]};
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (p + c >= rows) break;
        out.actor[at + c] = actor[c];
        out.group[at + c] = group[c];
        out.a0[at + c] = a0[c];
        if (out.a1) out.a1[at + c] = a1[c];
        if (out.a2) out.a2[at + c] = a2[c];
        if constexpr (MCOL) out.method[at + c] = method[c];
      }
    }
  }
}
static_assert(kScatterTile * 4 + kScatterSegs * 4 <= 16 * 1024, "four blocks per CU keep their LDS tiles");

int64_t scatter_question_tile() { return kScatterQTile; }
int64_t scatter_expand_tile() { return kScatterTile; }

static void scatter_check_rule(int rule, int64_t Q, uintptr_t q_actor, uintptr_t q_a0, int64_t step, uintptr_t offsets,
                               int64_t G, uintptr_t row_off, int64_t n_segs, uintptr_t q_off, int64_t n_queues) {
  if (rule < 0 || rule >= kScatterRules) throw std::invalid_argument("scatter: unknown rule");
  if (Q < 1 || Q > kScatterMaxQuestions) throw std::invalid_argument("scatter: Q must be in [1, 2^26]");
  if ((q_a0 & 7u) || (q_actor & 3u) || (offsets & 7u)) throw std::invalid_argument("scatter: misaligned column");
  if (rule == kScatterRanges) {
    if (!q_a0) throw std::invalid_argument("scatter: ranges needs the a0 column");
    if (step < 1 || step > kScatterMaxStep) throw std::invalid_argument("scatter: step must be in [1, 2^31 - 1]");
  } else {
    if (!q_actor || !offsets) throw std::invalid_argument("scatter: members needs the actor column and the offsets");
    if (G < 0 || G > 0x7fffffffll) throw std::invalid_argument("scatter: G must be in [0, 2^31)");
    if (rule == kScatterTopics) {
      if (!row_off || (row_off & 7u)) throw std::invalid_argument("scatter: topics needs an aligned row_off");
      if (n_segs < 0 || n_segs > kScatterMaxSegments) throw std::invalid_argument("scatter: n_segs must be in [0, 2^24]");
      if (n_queues < 0 || n_queues > kScatterMaxQueues) throw std::invalid_argument("scatter: n_queues must be in [0, 2^24]");
      if (n_queues && (!q_off || (q_off & 7u))) throw std::invalid_argument("scatter: queue subscriptions need an aligned q_off");
    } else if (n_queues) {
      throw std::invalid_argument("scatter: queue subscriptions belong to the topics rule");
    }
  }
}

// Count, scan, first: n int32[Q], first int64[Q], the counters (scatter.hpp).  `tsum` and
// `toob`: `tile_cap` u64 each of scratch, tile_cap >= ceil(Q / scatter_question_tile()).
// The question columns: Q elements, any natural alignment.  Topics with n_queues >= 1 queue
// subscriptions: q_off int64[G + 1], and the count kernel's QUEUES variant runs.
void launch_scatter_count(int rule, uintptr_t q_actor, uintptr_t q_a0, int64_t Q, int64_t step, uintptr_t offsets,
                          int64_t G, uintptr_t n, uintptr_t first, uintptr_t tsum, uintptr_t toob, int64_t tile_cap,
                          uintptr_t ctr, uintptr_t stream, uintptr_t row_off, int64_t n_segs, uintptr_t q_off,
                          int64_t n_queues) {
  scatter_check_rule(rule, Q, q_actor, q_a0, step, offsets, G, row_off, n_segs, q_off, n_queues);
  const int64_t tiles = (Q + kScatterQTile - 1) / kScatterQTile;
  if (tiles > tile_cap) throw std::invalid_argument("scatter: the tile scratch is too small for Q");
  if (!n || !first || !tsum || !toob || !ctr) throw std::invalid_argument("scatter: null output or scratch");
  if ((n & 3u) || ((first | tsum | toob | ctr) & 7u)) throw std::invalid_argument("scatter: misaligned output");
  ScatterRule r{};
  r.step = (uint64_t)(rule == kScatterRanges ? step : 1);
  r.offsets = (const int64_t*)offsets;
  r.G = G;
  r.row_off = (const int64_t*)row_off, r.n_segs = n_segs;
  if (rule == kScatterTopics && n_queues) {  // the table has a queue subscription
    ScatterQueueRule qr{};
    static_cast<ScatterRule&>(qr) = r;
    qr.q_off = (const int64_t*)q_off, qr.n_queues = n_queues;
    hipLaunchKernelGGL((scatter_count_kernel<kScatterTopics, true>), dim3((unsigned)tiles), dim3(kScatterThreads), 0,
                       as_stream(stream), qr, (const int*)q_actor, (const int64_t*)q_a0, Q, (int*)n, (unsigned long long*)first,
                       (unsigned long long*)tsum, (unsigned long long*)toob);
  } else {
    auto kernel = rule == kScatterRanges    ? scatter_count_kernel<kScatterRanges>
                  : rule == kScatterMembers ? scatter_count_kernel<kScatterMembers>
                                            : scatter_count_kernel<kScatterTopics>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(kScatterThreads), 0, as_stream(stream), r,
                       (const int*)q_actor, (const int64_t*)q_a0, Q, (int*)n, (unsigned long long*)first,
                       (unsigned long long*)tsum, (unsigned long long*)toob);
  }
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(scatter_scan_kernel, dim3(1), dim3(kScatterThreads), 0, as_stream(stream),
                     (unsigned long long*)tsum, (const unsigned long long*)toob, tiles, (unsigned long long*)ctr);
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(scatter_first_kernel, dim3((unsigned)((Q + kScatterThreads - 1) / kScatterThreads)),
                     dim3(kScatterThreads), 0, as_stream(stream), (unsigned long long*)first,
                     (const unsigned long long*)tsum, Q);
  PT_HIP_CHECK(hipGetLastError());
}

using ScatterExpandKernel = void (*)(ScatterRule, ScatterQuestions, const int64_t*, const int*, int, int64_t, ScatterOut);

// The expand pass over what launch_scatter_count left in `first` and `n`; `total` is the
// counter the host read (1 <= total <= capacity, the rows the outputs hold).  Outputs:
// actor / group int32, a0 (a1, a2: ranges always, members and topics when the question has them)
// int64, method int16 when the questions carry a method column; all 16-byte aligned (method 8).
// Topics: offsets = seg_off int64[G + 1], row_off int64[n_segs + 1], seg_start / seg_stride
// int32[n_segs], 1 <= n_segs <= 2^24.  Topics with n_queues >= 1 queue subscriptions run the QUEUES
// variant: row_off int64[n_all + 1], seg_start / seg_stride int32[n_all] with the queue segments
// after the n_segs ordinary ones (1 <= n_all <= 2^24, n_segs >= 0), q_off int64[G + 1], q_seg
// int64[n_queues + 1], `key` int64[Q] (by key) or `seq` (by index); without one, today's kernels.
void launch_scatter_expand(int rule, uintptr_t q_actor, uintptr_t q_a0, uintptr_t q_a1, uintptr_t q_a2, uintptr_t q_method,
                           int64_t Q, int64_t step, int64_t n_actors, int64_t actor_base, bool has_lo, int64_t first_lo,
                           uintptr_t offsets, uintptr_t members, int64_t G, int64_t n_members, uintptr_t first,
                           uintptr_t n, int64_t total, int64_t capacity, uintptr_t out_actor, uintptr_t out_a0,
                           uintptr_t out_a1, uintptr_t out_a2, uintptr_t out_method, uintptr_t out_group,
                           uintptr_t stream, uintptr_t row_off, uintptr_t seg_start, uintptr_t seg_stride,
                           int64_t n_segs, uintptr_t q_off, uintptr_t q_seg, int64_t n_queues, int64_t n_all,
                           uintptr_t key, uint64_t seq, bool by_index) {
  scatter_check_rule(rule, Q, q_actor, q_a0, step, offsets, G, row_off, n_segs, q_off, n_queues);
  if (capacity < 1 || capacity > kScatterMaxRows) throw std::invalid_argument("scatter: capacity must be in [1, 2^31 - 2]");
  if (total < 1 || total > capacity) throw std::invalid_argument("scatter: total must be in [1, capacity]");
  if (!first || !n || !out_actor || !out_a0 || !out_group) throw std::invalid_argument("scatter: null output");
  if (((out_actor | out_a0 | out_a1 | out_a2 | out_group) & 15u) || (out_method & 7u) || (first & 7u) || (n & 3u) ||
      ((q_a1 | q_a2) & 7u) || (q_method & 1u) || (members & 3u))
    throw std::invalid_argument("scatter: misaligned output or column");
  if (!q_a0) throw std::invalid_argument("scatter: the questions need an a0 column");
  if ((q_method != 0) != (out_method != 0)) throw std::invalid_argument("scatter: a method column in, a method column out");
  ScatterRule r{};
  ScatterQueueRule qa{};
  r.step = (uint64_t)(rule == kScatterRanges ? step : 1);
  if (rule == kScatterRanges) {
    if (n_actors < 1 || n_actors > 0x7fffffffll) throw std::invalid_argument("scatter: n_actors must be in [1, 2^31 - 1]");
    if (actor_base < 0 || actor_base >= n_actors) throw std::invalid_argument("scatter: actor_base must be in [0, n_actors)");
    if (!out_a1 || !out_a2) throw std::invalid_argument("scatter: ranges writes a1 and a2");
    r.n_actors = (uint32_t)n_actors, r.actor_base = (uint32_t)actor_base;
    r.first_lo = first_lo, r.has_lo = has_lo ? 1 : 0;
  } else {
    if ((q_a1 != 0) != (out_a1 != 0) || (q_a2 != 0) != (out_a2 != 0))
      throw std::invalid_argument("scatter: members and topics copy the columns the questions have");
    r.offsets = (const int64_t*)offsets, r.G = G;
    if (rule == kScatterMembers) {
      if (!members || n_members < 1 || n_members > kScatterMaxRows)
        throw std::invalid_argument("scatter: members needs a non-empty member list");
      r.members = (const int*)members, r.n_members = n_members;
    } else {
      if (!seg_start || !seg_stride || (n_queues ? n_all : n_segs) < 1)
        throw std::invalid_argument("scatter: topics needs a non-empty segment table");
      if ((seg_start | seg_stride) & 3u) throw std::invalid_argument("scatter: misaligned segment table");
      r.row_off = (const int64_t*)row_off, r.seg_start = (const int*)seg_start, r.seg_stride = (const int*)seg_stride;
      r.n_segs = n_segs;
      if (n_queues) {
        if (!q_seg || (q_seg & 7u)) throw std::invalid_argument("scatter: queue subscriptions need an aligned q_seg");
        if (n_all < n_segs || n_all > kScatterMaxSegments)
          throw std::invalid_argument("scatter: n_all must be in [n_segs, 2^24]");
        if (!by_index && (!key || (key & 7u))) throw std::invalid_argument("scatter: by key needs an aligned key column");
        qa.q_off = (const int64_t*)q_off, qa.q_seg = (const int64_t*)q_seg, qa.key = (const int64_t*)key;
        qa.n_queues = n_queues, qa.n_all = n_all, qa.seq = seq, qa.by_index = by_index ? 1 : 0;
      }
    }
  }
  const ScatterQuestions qs{(const int*)q_actor, (const int64_t*)q_a0, (const int64_t*)q_a1, (const int64_t*)q_a2,
                            (const int16_t*)q_method};
  const ScatterOut out{(int*)out_actor,  (int64_t*)out_a0,     (int64_t*)out_a1,
                       (int64_t*)out_a2, (int16_t*)out_method, (int*)out_group};
  const dim3 grid((unsigned)((total + kScatterTile - 1) / kScatterTile));
  if (rule == kScatterTopics && n_queues) {  // the table has a queue subscription
    static_cast<ScatterRule&>(qa) = r;
    auto kernel = q_method ? scatter_expand_kernel<kScatterTopics, true, true> : scatter_expand_kernel<kScatterTopics, false, true>;
    hipLaunchKernelGGL(kernel, grid, dim3(kScatterThreads), 0, as_stream(stream), qa, qs, (const int64_t*)first,
                       (const int*)n, (int)Q, total, out);
    PT_HIP_CHECK(hipGetLastError());
    return;
  }
  ScatterExpandKernel kernel;
  if (rule == kScatterRanges)
    kernel = q_method ? scatter_expand_kernel<kScatterRanges, true> : scatter_expand_kernel<kScatterRanges, false>;
  else if (rule == kScatterMembers)
    kernel = q_method ? scatter_expand_kernel<kScatterMembers, true> : scatter_expand_kernel<kScatterMembers, false>;
  else
    kernel = q_method ? scatter_expand_kernel<kScatterTopics, true> : scatter_expand_kernel<kScatterTopics, false>;
  hipLaunchKernelGGL(kernel, grid, dim3(kScatterThreads), 0, as_stream(stream), r, qs, (const int64_t*)first,
                     (const int*)n, (int)Q, total, out);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
