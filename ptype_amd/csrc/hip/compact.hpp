// Stable compaction of a batch by a per-row predicate: the rows that satisfy it are
// gathered, in index order, into a sub-batch.  Two instances: retry.hip selects by
// status (the retries, and the reply cache's, the breaker's and the limiter's
// kPending rows), coalesce.hip selects the group leaders (lead[i] == i) and also
// wants every row's place in the sub-batch.  dead_letters.hip ranks its tiles with the
// same device helpers (compact_tile_ballots / _offsets / compact_lane_rank) and writes
// ring records instead of a sub-batch.
//
//   compact_count_kernel   launch 1: one block per tile of kCompactTile keys; the
//                          tile's number of selected rows goes to counts[tile]
//   compact_select_kernel  launch 2: block b sums counts[0 .. b) itself (at most
//                          2048 words for 8 Mi rows, L2-resident), ranks its tile,
//                          writes idx and gathers every column; the last tile's
//                          block writes K.  With POS also pos[i] = i's row in the
//                          sub-batch, -1 for a row that is not selected
//
// The compaction is stable: idx is ascending, i.e. what torch.nonzero returns.
// No block waits for another one (the two launches are the only ordering), and no
// atomic is issued at all: within a wave a row's rank comes from __ballot +
// mbcnt64, across the waves of a block from 16 segment counts in LDS.
//
// Tile layout: 256 threads x 4 dwordx4 loads.  Load j of wave w, lane l covers the
// elements  tile * 4096 + (j * 4 + w) * 256 + l * 4 + {0, 1, 2, 3}:  a wave
// instruction reads 1 KiB contiguously, and the 16 (j, w) segments of 256
// elements are in index order, each ordered by (lane, component).
#pragma once
#include "common.hpp"

namespace ptype {

constexpr int kCompactThreads = 256;
constexpr int kCompactWaves = kCompactThreads / kWave;
constexpr int kCompactLoads = 4;                                     // dwordx4 loads per thread
constexpr int kCompactSegs = kCompactLoads * kCompactWaves;          // 256-element segments per tile
constexpr int kCompactTile = kCompactThreads * kCompactLoads * 4;    // 4096 rows

// The predicates: bool operator()(int key, int index), evaluated on loaded keys only.
struct InMask {  // the key is a status in a 32-bit set
  uint32_t mask;
  __device__ __forceinline__ bool operator()(int s, int) const {
    return (unsigned)s < 32u && ((mask >> (unsigned)s) & 1u);
  }
};
struct OwnIndex {  // the key is the row's own index
  __device__ __forceinline__ bool operator()(int l, int i) const { return l == i; }
};

// The four keys at element index i (a multiple of 4).  With VEC `key` is 16-byte
// aligned and four keys inside M come by one dwordx4 load; without it (a view at an
// odd offset) every key is a load of its own.  Elements at or past M read as -1:
// never selected, by either predicate.
template <bool VEC = true>
__device__ __forceinline__ int4 compact_load4(const int* __restrict__ key, int64_t i, int64_t M) {
  if constexpr (VEC) {
    if (i + 4 <= M) return *reinterpret_cast<const int4*>(key + i);
  }
  int4 v = {-1, -1, -1, -1};
  if (i < M) v.x = key[i];
  if (i + 1 < M) v.y = key[i + 1];
  if (i + 2 < M) v.z = key[i + 2];
  if constexpr (!VEC) {
    if (i + 3 < M) v.w = key[i + 3];
  }
  return v;
}

__device__ __forceinline__ int64_t compact_elem(int64_t tile, int j, unsigned wave, unsigned lane) {
  return tile * kCompactTile + (int64_t)(j * kCompactWaves + (int)wave) * (kWave * 4) + lane * 4;
}

// Ranking of one tile, shared by compact_select_kernel and the dead-letter append
// (dead_letters.hip).  Step 1: the four ballots of each of this wave's segments, and the
// segments' counts into seg_cnt[kCompactSegs] (LDS); a __syncthreads() follows.
template <class Pred, bool VEC = true>
__device__ __forceinline__ void compact_tile_ballots(const int* __restrict__ key, int64_t M, Pred pred, int64_t tile,
                                                     unsigned wave, unsigned lane, uint64_t (&b)[kCompactLoads][4],
                                                     unsigned* __restrict__ seg_cnt) {
#pragma unroll
  for (int j = 0; j < kCompactLoads; ++j) {
    const int64_t i = compact_elem(tile, j, wave, lane);
    const int4 v = compact_load4<VEC>(key, i, M);
    b[j][0] = __ballot(pred(v.x, (int)i));
    b[j][1] = __ballot(pred(v.y, (int)i + 1));
    b[j][2] = __ballot(pred(v.z, (int)i + 2));
    b[j][3] = __ballot(pred(v.w, (int)i + 3));
    if (lane == 0)
      seg_cnt[j * kCompactWaves + wave] =
          __popcll(b[j][0]) + __popcll(b[j][1]) + __popcll(b[j][2]) + __popcll(b[j][3]);
  }
}
// Step 2: the rank within the tile at which each of this wave's segments starts; returns
// the tile's number of selected rows.
__device__ __forceinline__ unsigned compact_tile_offsets(const unsigned* __restrict__ seg_cnt, unsigned wave,
                                                         unsigned (&seg_off)[kCompactLoads]) {
  unsigned total = 0;
#pragma unroll
  for (int s = 0; s < kCompactSegs; ++s) {  // (LDS broadcast reads; s = j * kCompactWaves + wave)
    if ((s % kCompactWaves) == (int)wave) seg_off[s / kCompactWaves] = total;
    total += seg_cnt[s];
  }
  return total;
}
// Step 3: the rank within the tile of this lane's first selected element of segment j
// (selected elements of lower lanes come first, then this lane's lower components).
__device__ __forceinline__ unsigned compact_lane_rank(const uint64_t (&bj)[4], unsigned seg_off_j) {
  return seg_off_j + mbcnt64(bj[0]) + mbcnt64(bj[1]) + mbcnt64(bj[2]) + mbcnt64(bj[3]);
}

template <class Pred>
__global__ __launch_bounds__(kCompactThreads) void compact_count_kernel(const int* __restrict__ key, int64_t M,
                                                                         Pred pred, uint32_t* __restrict__ counts) {
  __shared__ unsigned wave_cnt[kCompactWaves];
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tile = blockIdx.x;
  unsigned n = 0;  // wave-uniform: every term is a popcount of a ballot
#pragma unroll
  for (int j = 0; j < kCompactLoads; ++j) {
    const int64_t i = compact_elem(tile, j, wave, lane);
    const int4 v = compact_load4(key, i, M);
    n += __popcll(__ballot(pred(v.x, (int)i))) + __popcll(__ballot(pred(v.y, (int)i + 1))) +
         __popcll(__ballot(pred(v.z, (int)i + 2))) + __popcll(__ballot(pred(v.w, (int)i + 3)));
  }
  if (lane == 0) wave_cnt[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < kCompactWaves; ++w) t += wave_cnt[w];
    counts[tile] = t;
  }
}

template <class Pred, bool POS>
__global__ __launch_bounds__(kCompactThreads) void compact_select_kernel(
    const int* __restrict__ key, int64_t M, Pred pred, const uint32_t* __restrict__ counts,
    const int* __restrict__ actor, const int64_t* __restrict__ a0, const int64_t* __restrict__ a1,
    const int64_t* __restrict__ a2, const int16_t* __restrict__ method, int* __restrict__ idx,
    int* __restrict__ actor_o, int64_t* __restrict__ a0_o, int64_t* __restrict__ a1_o, int64_t* __restrict__ a2_o,
    int16_t* __restrict__ method_o, int* __restrict__ k_out, int* __restrict__ pos) {
  __shared__ unsigned wave_sum[kCompactWaves];
  __shared__ unsigned seg_cnt[kCompactSegs];
  __shared__ int sel[kCompactTile];  // the tile's selected row indices, in order
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tile = blockIdx.x;

  // this tile's first output row: the sum of the counts of the tiles below it
  unsigned below = 0;
  for (int64_t t = threadIdx.x; t < tile; t += kCompactThreads) below += counts[t];
  below = wave_incl_scan(below);
  if (lane == kWave - 1) wave_sum[wave] = below;

  // rank the tile: per 256-element segment, four ballots
  uint64_t b[kCompactLoads][4];
  compact_tile_ballots(key, M, pred, tile, wave, lane, b, seg_cnt);
  __syncthreads();
  unsigned off = 0;
#pragma unroll
  for (int w = 0; w < kCompactWaves; ++w) off += wave_sum[w];
  unsigned seg_off[kCompactLoads];
  const unsigned total = compact_tile_offsets(seg_cnt, wave, seg_off);
#pragma unroll
  for (int j = 0; j < kCompactLoads; ++j) {
    unsigned r = compact_lane_rank(b[j], seg_off[j]);
    const int64_t i = compact_elem(tile, j, wave, lane);
    int p[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      p[c] = -1;
      if ((b[j][c] >> lane) & 1ull) {
        p[c] = (int)(off + r);
        sel[r++] = (int)i + c;
      }
    }
    if constexpr (POS) {
      if (i + 4 <= M) {
        *reinterpret_cast<int4*>(pos + i) = make_int4(p[0], p[1], p[2], p[3]);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (i + c < M) pos[i + c] = p[c];
      }
    }
  }
  __syncthreads();
  // consecutive threads take consecutive output rows: coalesced stores, scattered loads
  for (unsigned k = threadIdx.x; k < total; k += kCompactThreads) {
    const int i = sel[k];
    const int64_t o = (int64_t)off + k;
    idx[o] = i;
    actor_o[o] = actor[i];
    a0_o[o] = a0[i];
    if (a1) a1_o[o] = a1[i];
    if (a2) a2_o[o] = a2[i];
    if (method) method_o[o] = method[i];
  }
  if (tile == (int64_t)gridDim.x - 1 && threadIdx.x == 0) *k_out = (int)(off + total);
}

// M in [1, 2^31), every buffer checked by the caller.  `counts`: (M + kCompactTile - 1) /
// kCompactTile u32 words of workspace.  The output columns hold up to M rows (K is known only
// afterwards); a null input column leaves its output alone.  `pos` is read only with POS.
template <class Pred, bool POS>
void launch_compact(uintptr_t key, int64_t M, Pred pred, uintptr_t actor, uintptr_t a0, uintptr_t a1, uintptr_t a2,
                    uintptr_t method, uintptr_t idx, uintptr_t pos, uintptr_t actor_o, uintptr_t a0_o, uintptr_t a1_o,
                    uintptr_t a2_o, uintptr_t method_o, uintptr_t counts, uintptr_t k_out, uintptr_t stream) {
  hipStream_t s = as_stream(stream);
  const unsigned tiles = (unsigned)((M + kCompactTile - 1) / kCompactTile);
  hipLaunchKernelGGL(compact_count_kernel<Pred>, dim3(tiles), dim3(kCompactThreads), 0, s, (const int*)key, M, pred,
                     (uint32_t*)counts);
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((compact_select_kernel<Pred, POS>), dim3(tiles), dim3(kCompactThreads), 0, s, (const int*)key, M,
                     pred, (const uint32_t*)counts, (const int*)actor, (const int64_t*)a0, (const int64_t*)a1,
                     (const int64_t*)a2, (const int16_t*)method, (int*)idx, (int*)actor_o, (int64_t*)a0_o,
                     (int64_t*)a1_o, (int64_t*)a2_o, (int16_t*)method_o, (int*)k_out, (int*)pos);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
