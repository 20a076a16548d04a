// Reply gather kernels (gather.hpp has the semantics and the accumulator layout;
// ops/gather.py the wrapper and the numpy reference).  Two launches per reduce:
//
//   reply_gather_kernel<OP>      blocks stride over tiles of kGatherTile messages: st,
//                                val and group are read once and folded into the
//                                per-group accumulators
//   reply_gather_finish_kernel   one thread per group: outputs resolved (first_ne
//                                fetches val[hit], every op st[bad]), the group's
//                                accumulator and `oob` written back to their identities
//
// Nothing else writes accumulators or outputs, and launch boundaries are the only
// ordering (as in reply_cache.hip).
//
// Same-address atomics serialise, so equal adjacent group ids -- a fan-out lays its
// groups out as runs -- are combined before anything is added.  A thread folds its
// four consecutive rows into at most a head run, a tail run and (rarely) one or two
// runs of its own in between.  Across the wave, lane l's scan item is its tail run
// (its only run when all four ids are equal); a ballot of "this item starts a run"
// gives every lane its run's first lane, and a segmented shuffle scan bounded by
// that lane folds the items of one run.  The last lane of a run adds it, once; a
// lane whose head run continues the previous lane's folds that scan result into
// its head first.  When no item continues its neighbour's (random ids) the scan is
// skipped.  Every fold is commutative (add, min, max), so the result does not depend
// on which lane adds what.
//
// Where the adds go: with G <= kGatherLdsGroups into LDS arrays indexed by group
// id (LDS atomics); the block flushes every group it touched with one global atomic
// per field when its tiles are done.  With a larger G, run leaders add to HBM.
//
// Tile layout as in ledger.hip / retry.hip: 256 threads x kGatherRows rows; row j of
// wave w, lane l covers the messages  tile * kGatherTile + (j * 4 + w) * 256 + l * 4 +
// {0, 1, 2, 3}: one dwordx4 per lane of st and of group, two of val.  Columns that are
// not 16-byte aligned (a view at an odd offset) take the same layout with scalar loads:
// views of an int64 and an int32 column at one element offset are off by 8 and by 4
// bytes, so no common peel aligns all three (cost: profiles/gather.md).
#include "common.hpp"
#include "gather.hpp"

namespace ptype {

constexpr int kGatherThreads = 256;
constexpr int kGatherWaves = kGatherThreads / kWave;
constexpr int kGatherRows = 2;                                 // 4-message rows per thread and tile
constexpr int kGatherTile = kGatherThreads * kGatherRows * 4;  // 2048 messages
constexpr uint64_t kGatherOne = (1ull << 32) | 1ull;           // one OK row in `count << 32 | n_ok`

// One run's partial result.
struct GatherPart {
  uint64_t val, cnt;
  uint32_t bad, hit;
};

template <int OP>
__device__ __forceinline__ uint64_t gather_identity() {
  if constexpr (OP == kGatherMin) return (uint64_t)INT64_MAX;
  if constexpr (OP == kGatherMax) return (uint64_t)INT64_MIN;
  return 0ull;
}

template <int OP>
__device__ __forceinline__ void gather_merge(GatherPart& a, const GatherPart& b) {
  if constexpr (OP == kGatherSum) a.val += b.val;
  if constexpr (OP == kGatherMin) a.val = (int64_t)b.val < (int64_t)a.val ? b.val : a.val;
  if constexpr (OP == kGatherMax) a.val = (int64_t)b.val > (int64_t)a.val ? b.val : a.val;
  a.cnt += b.cnt;
  a.bad = b.bad < a.bad ? b.bad : a.bad;
  a.hit = b.hit < a.hit ? b.hit : a.hit;
}

__device__ __forceinline__ GatherPart gather_shfl_up(const GatherPart& p, unsigned o) {
  GatherPart r;
  r.val = (uint64_t)__shfl_up((unsigned long long)p.val, o, kWave);
  r.cnt = (uint64_t)__shfl_up((unsigned long long)p.cnt, o, kWave);
  r.bad = (uint32_t)__shfl_up((int)p.bad, o, kWave);
  r.hit = (uint32_t)__shfl_up((int)p.hit, o, kWave);
  return r;
}

// Four consecutive elements at index i (a multiple of 4).  Elements at or past M
// read as 0 and are never used.
template <bool ALIGNED>
__device__ __forceinline__ void gather_load4(const int* __restrict__ p, int64_t i, int64_t M, int (&o)[4]) {
  if (ALIGNED && i + 4 <= M) {
    const int4 v = *reinterpret_cast<const int4*>(p + i);
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = i + c < M ? p[i + c] : 0;
}
template <bool ALIGNED>
__device__ __forceinline__ void gather_load4(const int64_t* __restrict__ p, int64_t i, int64_t M, int64_t (&o)[4]) {
  if (ALIGNED && i + 4 <= M) {
    const I64x2 lo = *reinterpret_cast<const I64x2*>(p + i);
    const I64x2 hi = *reinterpret_cast<const I64x2*>(p + i + 2);
    o[0] = lo.x, o[1] = lo.y, o[2] = hi.x, o[3] = hi.y;
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = i + c < M ? p[i + c] : 0;
}

// Where a block's adds go: LDS arrays indexed by group id, or the accumulator in HBM.
template <bool LDS>
struct GatherSink {
  unsigned long long* val;
  unsigned long long* cnt;
  unsigned* bad;
  unsigned* hit;
  unsigned long long* acc;
};

// Add run `p` of group `gid` (dead runs carry gid < 0; gid < G otherwise).
template <int OP, bool LDS>
__device__ __forceinline__ void gather_emit(const GatherSink<LDS>& s, int gid, const GatherPart& p) {
  if (gid < 0) return;
  [[maybe_unused]] unsigned long long* val = LDS ? &s.val[gid] : &s.acc[(size_t)gid * kGatherAccWords];
  unsigned long long* cnt = LDS ? &s.cnt[gid] : &s.acc[(size_t)gid * kGatherAccWords + 1];
  unsigned* bad = LDS ? &s.bad[gid] : reinterpret_cast<unsigned*>(&s.acc[(size_t)gid * kGatherAccWords + 2]);
  [[maybe_unused]] unsigned* hit = LDS ? &s.hit[gid] : reinterpret_cast<unsigned*>(&s.acc[(size_t)gid * kGatherAccWords + 2]) + 1;
  atomicAdd(cnt, (unsigned long long)p.cnt);
  if ((uint32_t)p.cnt) {  // the run has an OK row
    if constexpr (OP == kGatherSum) atomicAdd(val, (unsigned long long)p.val);
    if constexpr (OP == kGatherMin) atomicMin(reinterpret_cast<long long*>(val), (long long)p.val);
    if constexpr (OP == kGatherMax) atomicMax(reinterpret_cast<long long*>(val), (long long)p.val);
  }
  if (p.bad != kGatherNoRow) atomicMin(bad, p.bad);
  if constexpr (OP == kGatherFirstNe) {
    if (p.hit != kGatherNoRow) atomicMin(hit, p.hit);
  }
}

template <int OP, bool ALIGNED, bool LDS>
__global__ __launch_bounds__(kGatherThreads) void reply_gather_kernel(
    const int64_t* __restrict__ value, const int* __restrict__ status, const int* __restrict__ group, int64_t M,
    unsigned G, const int64_t* __restrict__ sentinel, unsigned long long* __restrict__ acc) {
  constexpr int kLds = LDS ? kGatherLdsGroups : 1;
  __shared__ unsigned long long lval[kLds], lcnt[kLds];
  __shared__ unsigned lbad[kLds], lhit[kLds];
  __shared__ unsigned oob_wave[kGatherWaves];
  const unsigned tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
  const GatherSink<LDS> sink{lval, lcnt, lbad, lhit, acc};

  if constexpr (LDS) {
    for (unsigned k = tid; k < G; k += kGatherThreads)
      lval[k] = gather_identity<OP>(), lcnt[k] = 0, lbad[k] = kGatherNoRow, lhit[k] = kGatherNoRow;
    __syncthreads();
  }

  const int64_t tiles = (M + kGatherTile - 1) / kGatherTile;
  unsigned n_oob = 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (block-uniform: every lane shuffles)
    const int64_t base = tile * kGatherTile;
#pragma unroll 2
    for (int j = 0; j < kGatherRows; ++j) {
      const int64_t i = base + (int64_t)(j * kGatherWaves + (int)wave) * (kWave * 4) + lane * 4;
      int s[4], gid[4];
      int64_t v[4];
      gather_load4<ALIGNED>(status, i, M, s);
      gather_load4<ALIGNED>(group, i, M, gid);
      gather_load4<ALIGNED>(value, i, M, v);

      // the thread's four rows: head run, tail run, runs in between added at once
      GatherPart cur{}, head{};
      int cur_g = -1, head_g = -1;
      bool single = true;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool live = i + c < M;
        const bool in = live && (unsigned)gid[c] < G;
        n_oob += live && gid[c] >= 0 && !in;
        const int g = in ? gid[c] : -1;
        const bool ok = s[c] == kStatusOk;
        GatherPart e;
        e.val = ok && OP != kGatherFirstNe ? (uint64_t)v[c] : gather_identity<OP>();
        e.cnt = in ? (ok ? kGatherOne : 1ull << 32) : 0ull;
        e.bad = in && !ok ? (uint32_t)(i + c) : kGatherNoRow;
        e.hit = kGatherNoRow;
        if constexpr (OP == kGatherFirstNe) {
          if (in && ok && v[c] != sentinel[g]) e.hit = (uint32_t)(i + c);
        }
        if (c == 0) {
          cur = e, cur_g = g, head_g = g;
        } else if (g == cur_g) {
          gather_merge<OP>(cur, e);
        } else {
          if (single)
            head = cur, single = false;
          else
            gather_emit<OP, LDS>(sink, cur_g, cur);
          cur = e, cur_g = g;
        }
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
          const GatherPart up = gather_shfl_up(cur, o);
          if (lane >= first + o) gather_merge<OP>(cur, up);
        }
      }
      const GatherPart prev = gather_shfl_up(cur, 1);
      if (!single) {
        if (lane > 0 && head_g == prev_tail_g) gather_merge<OP>(head, prev);
        gather_emit<OP, LDS>(sink, head_g, head);
      }
      if (lane == (unsigned)kWave - 1 || next_head_g != tail_g) gather_emit<OP, LDS>(sink, tail_g, cur);
    }
  }

  // rows past the table: one global atomic per block
#pragma unroll
  for (int o = kWave / 2; o; o >>= 1) n_oob += (unsigned)__shfl_xor((int)n_oob, o, kWave);
  if (lane == 0) oob_wave[wave] = n_oob;
  __syncthreads();
  if (tid == 0) {
    const unsigned n = oob_wave[0] + oob_wave[1] + oob_wave[2] + oob_wave[3];
    if (n) atomicAdd(&acc[(size_t)G * kGatherAccWords], (unsigned long long)n);
  }
  if constexpr (LDS) {
    // every touched group once; blocks start at different groups so that they do not
    // walk the same addresses in step
    const unsigned rot = (unsigned)(((uint64_t)blockIdx.x * 0x9e3779b1ull) % G);
    for (unsigned k0 = tid; k0 < G; k0 += kGatherThreads) {
      const unsigned k = k0 + rot < G ? k0 + rot : k0 + rot - G;
      const uint64_t c = lcnt[k];
      if (!c) continue;
      unsigned long long* a = &acc[(size_t)k * kGatherAccWords];
      atomicAdd(&a[1], (unsigned long long)c);
      if ((uint32_t)c) {
        if constexpr (OP == kGatherSum) atomicAdd(&a[0], lval[k]);
        if constexpr (OP == kGatherMin) atomicMin(reinterpret_cast<long long*>(&a[0]), (long long)lval[k]);
        if constexpr (OP == kGatherMax) atomicMax(reinterpret_cast<long long*>(&a[0]), (long long)lval[k]);
      }
      if (lbad[k] != kGatherNoRow) atomicMin(reinterpret_cast<unsigned*>(&a[2]), lbad[k]);
      if constexpr (OP == kGatherFirstNe) {
        if (lhit[k] != kGatherNoRow) atomicMin(reinterpret_cast<unsigned*>(&a[2]) + 1, lhit[k]);
      }
    }
  }
}
static_assert(kGatherWaves == 4, "the oob reduction reads four waves' partials");
static_assert(kGatherLdsGroups * 24 <= 64 * 1024, "a block's LDS arrays");

__global__ __launch_bounds__(kGatherThreads) void reply_gather_finish_kernel(
    unsigned long long* __restrict__ acc, unsigned G, int op, const int64_t* __restrict__ value_in,
    const int* __restrict__ status_in, int64_t M, const int64_t* __restrict__ sentinel, int64_t* __restrict__ value,
    int* __restrict__ status, int* __restrict__ n_ok, int* __restrict__ count, int* __restrict__ bad_row,
    int64_t* __restrict__ oob) {
  const unsigned g = blockIdx.x * kGatherThreads + threadIdx.x;
  if (g >= G) return;
  I64x2* a = reinterpret_cast<I64x2*>(acc + (size_t)g * kGatherAccWords);
  const I64x2 lo = a[0], hi = a[1];
  const uint64_t cnt = (uint64_t)lo.y;
  uint32_t bad = (uint32_t)(uint64_t)hi.x;
  const uint32_t hit = (uint32_t)((uint64_t)hi.x >> 32);
  int64_t v = lo.x, identity = 0;
  if (op == kGatherMin) identity = INT64_MAX;
  if (op == kGatherMax) identity = INT64_MIN;
  if (op == kGatherFirstNe) {
    if (bad > hit) bad = kGatherNoRow;  // a failure above the hit: the early return never saw it
    v = sentinel[g];
    if (bad == kGatherNoRow && hit != kGatherNoRow && (int64_t)hit < M) v = value_in[hit];
  }
  value[g] = v;
  status[g] = bad != kGatherNoRow && (int64_t)bad < M ? status_in[bad] : kStatusOk;
  bad_row[g] = bad != kGatherNoRow ? (int)bad : -1;
  n_ok[g] = (int)(uint32_t)cnt;
  count[g] = (int)(cnt >> 32);
  a[0] = I64x2{identity, 0};
  a[1] = I64x2{-1, 0};
  if (g == 0) {
    oob[0] = (int64_t)acc[(size_t)G * kGatherAccWords];
    acc[(size_t)G * kGatherAccWords] = 0;
  }
}

int64_t reply_gather_tile() { return kGatherTile; }

using GatherKernel = void (*)(const int64_t*, const int*, const int*, int64_t, unsigned, const int64_t*,
                              unsigned long long*);
template <int OP>
static GatherKernel gather_variant(bool aligned, bool lds) {
  if (aligned) return lds ? reply_gather_kernel<OP, true, true> : reply_gather_kernel<OP, true, false>;
  return lds ? reply_gather_kernel<OP, false, true> : reply_gather_kernel<OP, false, false>;
}

// `acc`: (G + 1) * kGatherAccWords u64 holding the identities (gather.hpp); `sentinel`:
// G int64 (first_ne; read one element at a time, 8-byte aligned) or null; the outputs: value int64[G], status / n_ok / count /
// bad_row int32[G], oob int64[1].  value / status / group: M elements, any natural
// alignment (16-byte aligned columns take the vector loads).
void launch_reply_gather(uintptr_t value_in, uintptr_t status_in, uintptr_t group, int64_t M, int64_t G, int op,
                         uintptr_t sentinel, uintptr_t acc, uintptr_t value, uintptr_t status, uintptr_t n_ok,
                         uintptr_t count, uintptr_t bad_row, uintptr_t oob, uintptr_t stream) {
  if (M < 0 || M >= 0x7fffffffll) throw std::invalid_argument("reply_gather: M must be in [0, 2^31 - 1)");
  if (G < 1 || G > kGatherMaxGroups) throw std::invalid_argument("reply_gather: G must be in [1, 2^26]");
  if (op < 0 || op >= kGatherOps) throw std::invalid_argument("reply_gather: unknown op");
  if (op == kGatherFirstNe && !sentinel) throw std::invalid_argument("reply_gather: first_ne needs a sentinel");
  if (!acc || !value || !status || !n_ok || !count || !bad_row || !oob)
    throw std::invalid_argument("reply_gather: null accumulator or output");
  if (M > 0 && (!value_in || !status_in || !group)) throw std::invalid_argument("reply_gather: null column");
  if ((value_in | sentinel) & 7u || (status_in | group) & 3u || (acc | value) & 15u)
    throw std::invalid_argument("reply_gather: misaligned column");
  if (M > 0) {
    const bool aligned = !((value_in | status_in | group) & 15u), lds = G <= kGatherLdsGroups;
    const int64_t tiles = (M + kGatherTile - 1) / kGatherTile;
    int64_t cap = kGatherBlocksHbm;
    if (lds) {  // a flush costs G atomics per field and block: at least kGatherFlushRatio * G messages per block
      cap = M / (kGatherFlushRatio * G);
      cap = cap < kGatherBlocksLdsMin ? kGatherBlocksLdsMin : cap > kGatherBlocksLds ? kGatherBlocksLds : cap;
    }
    GatherKernel kernel = op == kGatherSum   ? gather_variant<kGatherSum>(aligned, lds)
                          : op == kGatherMin ? gather_variant<kGatherMin>(aligned, lds)
                          : op == kGatherMax ? gather_variant<kGatherMax>(aligned, lds)
                                             : gather_variant<kGatherFirstNe>(aligned, lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(kGatherThreads), 0, as_stream(stream),
                       (const int64_t*)value_in, (const int*)status_in, (const int*)group, M, (unsigned)G,
                       (const int64_t*)sentinel, (unsigned long long*)acc);
    PT_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(reply_gather_finish_kernel, dim3((unsigned)((G + kGatherThreads - 1) / kGatherThreads)),
                     dim3(kGatherThreads), 0, as_stream(stream), (unsigned long long*)acc, (unsigned)G, op,
                     (const int64_t*)value_in, (const int*)status_in, M, (const int64_t*)sentinel, (int64_t*)value,
                     (int*)status, (int*)n_ok, (int*)count, (int*)bad_row, (int64_t*)oob);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
