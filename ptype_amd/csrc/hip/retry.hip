// Retry selection of a Send (`ActorExchange.send_all(retries=...)`, ops/retry.py):
// the messages whose status is in a retryable set are compacted into a sub-batch
// on the device, and the sub-batch's replies are put back.  The reference retries
// one call at a time on the host (cluster/rpc.go:59-116, withRetry around a
// re-selected connection); here a whole batch's failed messages are picked out
// by two kernels and merged by a third.
//
//   retry_count_kernel   launch 1: one block per tile of kRetryTile statuses; the
//                        tile's number of selected messages goes to counts[tile]
//   retry_select_kernel  launch 2: block b sums counts[0 .. b) itself (at most
//                        2048 words for 8 Mi messages, L2-resident), ranks its
//                        tile, writes idx and gathers every column; the last
//                        tile's block writes K
//   retry_merge_kernel   val[idx[j]] = v2[j], st[idx[j]] = s2[j]
//
// The compaction is stable: idx is ascending, i.e. what torch.nonzero returns.
// No block waits for another one (the two launches are the only ordering), and no
// atomic is issued at all: within a wave a message's rank comes from __ballot +
// mbcnt64, across the waves of a block from 16 segment counts in LDS.
//
// Tile layout: 256 threads x 4 dwordx4 loads.  Load j of wave w, lane l covers the
// elements  tile * 4096 + (j * 4 + w) * 256 + l * 4 + {0, 1, 2, 3}:  a wave
// instruction reads 1 KiB contiguously, and the 16 (j, w) segments of 256
// elements are in index order, each ordered by (lane, component).
#include "common.hpp"

namespace ptype {

constexpr int kRetryThreads = 256;
constexpr int kRetryWaves = kRetryThreads / kWave;
constexpr int kRetryLoads = 4;                                   // dwordx4 loads per thread
constexpr int kRetrySegs = kRetryLoads * kRetryWaves;            // 256-element segments per tile
constexpr int kRetryTile = kRetryThreads * kRetryLoads * 4;      // 4096 statuses

__device__ __forceinline__ bool retry_selected(int s, uint32_t mask) {
  return (unsigned)s < 32u && ((mask >> (unsigned)s) & 1u);
}

// The four statuses at element index i (a multiple of 4; `status` is 16-byte
// aligned).  Elements at or past M read as -1: never selected.
__device__ __forceinline__ int4 retry_load4(const int* __restrict__ status, int64_t i, int64_t M) {
  if (i + 4 <= M) return *reinterpret_cast<const int4*>(status + i);
  int4 v = {-1, -1, -1, -1};
  if (i < M) v.x = status[i];
  if (i + 1 < M) v.y = status[i + 1];
  if (i + 2 < M) v.z = status[i + 2];
  return v;
}

__device__ __forceinline__ int64_t retry_elem(int64_t tile, int j, unsigned wave, unsigned lane) {
  return tile * kRetryTile + (int64_t)(j * kRetryWaves + (int)wave) * (kWave * 4) + lane * 4;
}

__global__ __launch_bounds__(kRetryThreads) void retry_count_kernel(const int* __restrict__ status, int64_t M,
                                                                     uint32_t mask, uint32_t* __restrict__ counts) {
  __shared__ unsigned wave_cnt[kRetryWaves];
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tile = blockIdx.x;
  unsigned n = 0;  // wave-uniform: every term is a popcount of a ballot
#pragma unroll
  for (int j = 0; j < kRetryLoads; ++j) {
    const int4 v = retry_load4(status, retry_elem(tile, j, wave, lane), M);
    n += __popcll(__ballot(retry_selected(v.x, mask))) + __popcll(__ballot(retry_selected(v.y, mask))) +
         __popcll(__ballot(retry_selected(v.z, mask))) + __popcll(__ballot(retry_selected(v.w, mask)));
  }
  if (lane == 0) wave_cnt[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < kRetryWaves; ++w) t += wave_cnt[w];
    counts[tile] = t;
  }
}

__global__ __launch_bounds__(kRetryThreads) void retry_select_kernel(
    const int* __restrict__ status, int64_t M, uint32_t mask, const uint32_t* __restrict__ counts,
    const int* __restrict__ actor, const int64_t* __restrict__ a0, const int64_t* __restrict__ a1,
    const int64_t* __restrict__ a2, const int16_t* __restrict__ method, int* __restrict__ idx,
    int* __restrict__ actor_o, int64_t* __restrict__ a0_o, int64_t* __restrict__ a1_o, int64_t* __restrict__ a2_o,
    int16_t* __restrict__ method_o, int* __restrict__ k_out) {
  __shared__ unsigned wave_sum[kRetryWaves];
  __shared__ unsigned seg_cnt[kRetrySegs];
  __shared__ int sel[kRetryTile];  // the tile's selected message indices, in order
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tile = blockIdx.x;

  // this tile's first output position: the sum of the counts of the tiles below it
  unsigned below = 0;
  for (int64_t t = threadIdx.x; t < tile; t += kRetryThreads) below += counts[t];
  below = wave_incl_scan(below);
  if (lane == kWave - 1) wave_sum[wave] = below;

  // rank the tile: per 256-element segment, four ballots
  int4 v[kRetryLoads];
  uint64_t b[kRetryLoads][4];
#pragma unroll
  for (int j = 0; j < kRetryLoads; ++j) {
    v[j] = retry_load4(status, retry_elem(tile, j, wave, lane), M);
    b[j][0] = __ballot(retry_selected(v[j].x, mask));
    b[j][1] = __ballot(retry_selected(v[j].y, mask));
    b[j][2] = __ballot(retry_selected(v[j].z, mask));
    b[j][3] = __ballot(retry_selected(v[j].w, mask));
    if (lane == 0)
      seg_cnt[j * kRetryWaves + wave] =
          __popcll(b[j][0]) + __popcll(b[j][1]) + __popcll(b[j][2]) + __popcll(b[j][3]);
  }
  __syncthreads();
  unsigned off = 0;
#pragma unroll
  for (int w = 0; w < kRetryWaves; ++w) off += wave_sum[w];
  unsigned seg_off[kRetryLoads], total = 0;
#pragma unroll
  for (int s = 0; s < kRetrySegs; ++s) {  // (LDS broadcast reads; s = j * kRetryWaves + wave)
    if ((s % kRetryWaves) == (int)wave) seg_off[s / kRetryWaves] = total;
    total += seg_cnt[s];
  }
#pragma unroll
  for (int j = 0; j < kRetryLoads; ++j) {
    // selected elements of lower lanes come first, then this lane's lower components
    unsigned r = seg_off[j] + mbcnt64(b[j][0]) + mbcnt64(b[j][1]) + mbcnt64(b[j][2]) + mbcnt64(b[j][3]);
    const int i = (int)retry_elem(tile, j, wave, lane);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if ((b[j][c] >> lane) & 1ull) sel[r++] = i + c;
    }
  }
  __syncthreads();
  // consecutive threads take consecutive output rows: coalesced stores, scattered loads
  for (unsigned k = threadIdx.x; k < total; k += kRetryThreads) {
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

__global__ __launch_bounds__(256) void retry_merge_kernel(int64_t* __restrict__ val, int* __restrict__ st, int64_t M,
                                                           const int* __restrict__ idx,
                                                           const int64_t* __restrict__ v2,
                                                           const int* __restrict__ s2, int64_t K) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < K; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx[j];
    if ((uint64_t)i >= (uint64_t)M) continue;  // (never, for an idx of retry_select over M messages)
    val[i] = v2[j];
    st[i] = s2[j];
  }
}

int64_t retry_tile() { return kRetryTile; }

// `counts`: (M + tile - 1) / tile u32 words of workspace.  The output columns hold up
// to M rows (K is known only afterwards); a null input column leaves its output alone.
void launch_retry_select(uintptr_t status, int64_t M, uint32_t mask, uintptr_t actor, uintptr_t a0, uintptr_t a1,
                         uintptr_t a2, uintptr_t method, uintptr_t idx, uintptr_t actor_o, uintptr_t a0_o,
                         uintptr_t a1_o, uintptr_t a2_o, uintptr_t method_o, uintptr_t counts, uintptr_t k_out,
                         uintptr_t stream) {
  if (M <= 0) return;
  if (M > 0x7fffffffll) throw std::invalid_argument("retry_select: more than 2^31 - 1 messages");
  if (status & 15u) throw std::invalid_argument("retry_select: status must be 16-byte aligned");
  if (!status || !actor || !a0 || !idx || !actor_o || !a0_o || !counts || !k_out || (a1 && !a1_o) || (a2 && !a2_o) ||
      (method && !method_o))
    throw std::invalid_argument("retry_select: null buffer");
  hipStream_t s = as_stream(stream);
  const unsigned tiles = (unsigned)((M + kRetryTile - 1) / kRetryTile);
  hipLaunchKernelGGL(retry_count_kernel, dim3(tiles), dim3(kRetryThreads), 0, s, (const int*)status, M, mask,
                     (uint32_t*)counts);
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(retry_select_kernel, dim3(tiles), dim3(kRetryThreads), 0, s, (const int*)status, M, mask,
                     (const uint32_t*)counts, (const int*)actor, (const int64_t*)a0, (const int64_t*)a1,
                     (const int64_t*)a2, (const int16_t*)method, (int*)idx, (int*)actor_o, (int64_t*)a0_o,
                     (int64_t*)a1_o, (int64_t*)a2_o, (int16_t*)method_o, (int*)k_out);
  PT_HIP_CHECK(hipGetLastError());
}

void launch_retry_merge(uintptr_t val, uintptr_t st, int64_t M, uintptr_t idx, uintptr_t v2, uintptr_t s2, int64_t K,
                        uintptr_t stream) {
  if (K <= 0) return;
  if (!val || !st || !idx || !v2 || !s2) throw std::invalid_argument("retry_merge: null buffer");
  int64_t blocks = (K + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(retry_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (int64_t*)val,
                     (int*)st, M, (const int*)idx, (const int64_t*)v2, (const int*)s2, K);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
