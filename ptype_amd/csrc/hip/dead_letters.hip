// Dead-letter queue (dead_letters.hpp has the record and control-line layout;
// ops/dead_letters.py the wrapper and the numpy model).
//
//   dlq_count_kernel    launch 1: what compact_count_kernel<InMask> does over `status` --
//                       one block per tile of kCompactTile rows, the tile's number of
//                       letters to counts[tile] -- and block 0 copies head to base (and
//                       sends + 1 to seq): launch 2 reads those two scratch words and
//                       never head / sends, which its last block commits
//   dlq_append_kernel   launch 2: a block without a letter returns at once (the last
//                       tile's block stays: it commits).  Otherwise the block sums
//                       counts[0 .. tile) and all of counts (at most 2048 words for 8 Mi
//                       rows, L2-resident) -- of K > entries letters only the last
//                       `entries` are written, so a block whose letters are all older
//                       returns here -- ranks its tile as compact_select_kernel does
//                       (compact.hpp: ballots, mbcnt64, 16 segment counts in LDS) and
//                       writes its letters, four lanes per letter, each lane one 16-byte
//                       quarter: a wave's store covers 16 consecutive slots (1 KiB) and a
//                       lane gathers only the columns of its quarter
//   dlq_take_kernel     the ring from ticket t0 on into SoA columns, with the ticket check
//
// The order of the launches on the stream is the only synchronisation: no atomics in
// the append, no block waits for another one, every store is a plain vector store.
// Tickets are handed out in ascending row order, so the ring's content is a function
// of the Sends alone.  Every ring index is masked by entries - 1.
#include "compact.hpp"
#include "dead_letters.hpp"

namespace ptype {

template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void dlq_count_kernel(const int* __restrict__ status, int64_t M,
                                                                     InMask pred, uint32_t* __restrict__ counts,
                                                                     uint64_t* __restrict__ ctrl) {
  __shared__ unsigned wave_cnt[kCompactWaves];
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tile = blockIdx.x;
  unsigned n = 0;  // wave-uniform: every term is a popcount of a ballot
#pragma unroll
  for (int j = 0; j < kCompactLoads; ++j) {
    const int64_t i = compact_elem(tile, j, wave, lane);
    const int4 v = compact_load4<VEC>(status, i, M);
    n += __popcll(__ballot(pred(v.x, 0))) + __popcll(__ballot(pred(v.y, 0))) + __popcll(__ballot(pred(v.z, 0))) +
         __popcll(__ballot(pred(v.w, 0)));
  }
  if (lane == 0) wave_cnt[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < kCompactWaves; ++w) t += wave_cnt[w];
    counts[tile] = t;
    if (tile == 0) {
      ctrl[kDlqBase] = ctrl[kDlqHead];
      ctrl[kDlqSeqNext] = ctrl[kDlqSends] + 1ull;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kCompactThreads) void dlq_append_kernel(
    const int* __restrict__ status, int64_t M, InMask pred, const uint32_t* __restrict__ counts,
    const int* __restrict__ actor, const int16_t* __restrict__ method_col, unsigned method_uniform,
    const int* __restrict__ attempts, const int64_t* __restrict__ a0, const int64_t* __restrict__ a1,
    const int64_t* __restrict__ a2, uint64_t tag, uint64_t* __restrict__ ring, uint64_t* __restrict__ ctrl,
    uint64_t entries) {
  __shared__ unsigned wave_sum[2][kCompactWaves];
  __shared__ unsigned seg_cnt[kCompactSegs];
  __shared__ int sel[kCompactTile];  // the tile's letters' rows, in order
  const unsigned lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tile = blockIdx.x, tiles = gridDim.x;
  const bool last = tile == tiles - 1;
  const unsigned mine = counts[tile];
  if (mine == 0 && !last) return;  // (block-uniform)

  // this tile's first letter: the sum of the counts below it; K: the sum of them all
  unsigned below = 0, all = 0;
  for (int64_t t = threadIdx.x; t < tiles; t += kCompactThreads) {
    const unsigned c = counts[t];
    all += c;
    if (t < tile) below += c;
  }
  below = wave_incl_scan(below);
  all = wave_incl_scan(all);
  if (lane == kWave - 1) wave_sum[0][wave] = below, wave_sum[1][wave] = all;
  __syncthreads();
  unsigned off = 0, K = 0;
#pragma unroll
  for (int w = 0; w < kCompactWaves; ++w) off += wave_sum[0][w], K += wave_sum[1][w];
  // of K > entries letters only the last `entries` are written: a tile whose newest letter is
  // older than those has nothing to write (block-uniform; never the last tile)
  if (!last && (uint64_t)(K - (off + mine - 1u)) > entries) return;

  uint64_t b[kCompactLoads][4];
  compact_tile_ballots<InMask, VEC>(status, M, pred, tile, wave, lane, b, seg_cnt);
  __syncthreads();
  unsigned seg_off[kCompactLoads];
  const unsigned total = compact_tile_offsets(seg_cnt, wave, seg_off);
#pragma unroll
  for (int j = 0; j < kCompactLoads; ++j) {
    unsigned r = compact_lane_rank(b[j], seg_off[j]);
    const int64_t i = compact_elem(tile, j, wave, lane);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if ((b[j][c] >> lane) & 1ull) sel[r++] = (int)i + c;
  }
  __syncthreads();

  const uint64_t base = ctrl[kDlqBase], seq = ctrl[kDlqSeqNext];
  // four lanes per letter: lane q of a letter stores words 2q and 2q + 1 of its record
  const unsigned part = threadIdx.x & 3u;
  for (unsigned k = threadIdx.x >> 2; k < total; k += kCompactThreads / 4) {
    const unsigned pos = off + k;
    if ((uint64_t)(K - pos) > entries) continue;  // (older than the last `entries` letters of this Send)
    const int i = sel[k];
    const uint64_t t = base + pos;
    ulonglong2 w;
    if (part == 0) {
      w.x = t + 1ull;
      w.y = seq;
    } else if (part == 1) {
      const unsigned m = method_col ? (unsigned)(uint16_t)method_col[i] : (method_uniform & 0xffffu);
      uint64_t att = 1;
      if (attempts) {
        att = (uint64_t)(uint32_t)attempts[i] + 1ull;
        if (att > kDlqMaxAttempts) att = kDlqMaxAttempts;
      }
      w.x = (uint64_t)(uint32_t)i | (uint64_t)(uint32_t)status[i] << 32;
      w.y = (uint64_t)(uint32_t)actor[i] | (uint64_t)m << 32 | att << 48;
    } else if (part == 2) {
      w.x = (uint64_t)a0[i];
      w.y = a1 ? (uint64_t)a1[i] : 0ull;
    } else {
      w.x = a2 ? (uint64_t)a2[i] : 0ull;
      w.y = tag;
    }
    *reinterpret_cast<ulonglong2*>(ring + (t & (entries - 1)) * kDlqRecordWords + part * 2) = w;
  }

  if (last && threadIdx.x == 0) {
    const uint64_t head = base + K;
    uint64_t tail = ctrl[kDlqTail];
    if (head > entries && head - entries > tail) {
      ctrl[kDlqDropped] += head - entries - tail;
      tail = head - entries;
    }
    ctrl[kDlqHead] = head;
    ctrl[kDlqTail] = tail;
    ctrl[kDlqSends] = seq;
  }
}

__global__ __launch_bounds__(256) void dlq_take_kernel(
    const uint64_t* __restrict__ ring, uint64_t* __restrict__ ctrl, uint64_t entries, uint64_t t0, int64_t n,
    bool drain, int64_t* __restrict__ seq, int* __restrict__ row, int* __restrict__ status, int* __restrict__ actor,
    int16_t* __restrict__ method, int* __restrict__ attempts, int64_t* __restrict__ a0, int64_t* __restrict__ a1,
    int64_t* __restrict__ a2, int64_t* __restrict__ tag) {
  const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t q = g; q < n * 4; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = q >> 2;
    const unsigned part = (unsigned)q & 3u;
    const uint64_t t = t0 + (uint64_t)k;
    const ulonglong2 w =
        *reinterpret_cast<const ulonglong2*>(ring + (t & (entries - 1)) * kDlqRecordWords + part * 2);
    if (part == 0) {
      if (w.x != t + 1ull) atomicAdd((unsigned long long*)&ctrl[kDlqTorn], 1ull);  // (never, for an intact ring)
      seq[k] = (int64_t)w.y;
    } else if (part == 1) {
      row[k] = (int)(uint32_t)w.x;
      status[k] = (int)(uint32_t)(w.x >> 32);
      actor[k] = (int)(uint32_t)w.y;
      method[k] = (int16_t)(uint16_t)(w.y >> 32);
      attempts[k] = (int)(w.y >> 48);
    } else if (part == 2) {
      a0[k] = (int64_t)w.x;
      a1[k] = (int64_t)w.y;
    } else {
      a2[k] = (int64_t)w.x;
      tag[k] = (int64_t)w.y;
    }
  }
  // (no block of this launch reads tail: t0 came with the launch)
  if (drain && g == 0) ctrl[kDlqTail] = t0 + (uint64_t)n;
}

int64_t dlq_tile() { return kCompactTile; }

static void dlq_check_ring(const char* who, uintptr_t ring, uintptr_t ctrl, int64_t entries) {
  if (entries < kDlqMinEntries || entries > kDlqMaxEntries || (entries & (entries - 1)))
    throw std::invalid_argument(std::string(who) + ": entries must be a power of two in [64, 2^24]");
  if (!ring || !ctrl || (ring & 15u) || (ctrl & 7u))
    throw std::invalid_argument(std::string(who) + ": null or misaligned ring / control line");
}

// `ring`: entries * kDlqRecordWords u64, 16-byte aligned; `ctrl`: kDlqCtrlWords u64; `counts`:
// max(1, ceil(M / kCompactTile)) u32 words of workspace.  a1 / a2 / method_col / attempts may be
// null.  An empty Send (M = 0) still counts one Send.  A status column that is not 16-byte
// aligned is read with scalar loads.
void launch_dlq_append(uintptr_t status, int64_t M, uint32_t mask, uintptr_t actor, uintptr_t method_col,
                       uint32_t method_uniform, uintptr_t attempts, uintptr_t a0, uintptr_t a1, uintptr_t a2,
                       int64_t tag, uintptr_t ring, uintptr_t ctrl, int64_t entries, uintptr_t counts,
                       uintptr_t stream) {
  if (M < 0 || M > 0x7fffffffll) throw std::invalid_argument("dlq_append: M must be in [0, 2^31 - 1]");
  dlq_check_ring("dlq_append", ring, ctrl, entries);
  if (!counts) throw std::invalid_argument("dlq_append: null workspace");
  if (M > 0 && (!status || !actor || !a0)) throw std::invalid_argument("dlq_append: null column");
  if ((mask & 1u) || mask < 2u) throw std::invalid_argument("dlq_append: the mask names no status, or STATUS_OK");
  if ((status | actor | attempts) & 3u || (a0 | a1 | a2) & 7u || method_col & 1u)
    throw std::invalid_argument("dlq_append: a column is not aligned to its element size");
  hipStream_t s = as_stream(stream);
  const unsigned tiles = M ? (unsigned)((M + kCompactTile - 1) / kCompactTile) : 1u;
  const bool vec = (status & 15u) == 0;
  const InMask pred{mask};
  hipLaunchKernelGGL(vec ? dlq_count_kernel<true> : dlq_count_kernel<false>, dim3(tiles), dim3(kCompactThreads), 0, s,
                     (const int*)status, M, pred, (uint32_t*)counts, (uint64_t*)ctrl);
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(vec ? dlq_append_kernel<true> : dlq_append_kernel<false>, dim3(tiles), dim3(kCompactThreads), 0,
                     s, (const int*)status, M, pred, (const uint32_t*)counts, (const int*)actor,
                     (const int16_t*)method_col, method_uniform, (const int*)attempts, (const int64_t*)a0,
                     (const int64_t*)a1, (const int64_t*)a2, (uint64_t)tag, (uint64_t*)ring, (uint64_t*)ctrl,
                     (uint64_t)entries);
  PT_HIP_CHECK(hipGetLastError());
}

// n letters from ticket t0 (n in [1, entries]) into the ten columns, each n elements.
void launch_dlq_take(uintptr_t ring, uintptr_t ctrl, int64_t entries, int64_t t0, int64_t n, bool drain, uintptr_t seq,
                     uintptr_t row, uintptr_t status, uintptr_t actor, uintptr_t method, uintptr_t attempts,
                     uintptr_t a0, uintptr_t a1, uintptr_t a2, uintptr_t tag, uintptr_t stream) {
  if (n <= 0) return;
  dlq_check_ring("dlq_take", ring, ctrl, entries);
  if (n > entries || t0 < 0) throw std::invalid_argument("dlq_take: n must be in [1, entries] and t0 >= 0");
  if (!seq || !row || !status || !actor || !method || !attempts || !a0 || !a1 || !a2 || !tag)
    throw std::invalid_argument("dlq_take: null column");
  int64_t blocks = (n * 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dlq_take_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const uint64_t*)ring,
                     (uint64_t*)ctrl, (uint64_t)entries, (uint64_t)t0, n, drain, (int64_t*)seq, (int*)row,
                     (int*)status, (int*)actor, (int16_t*)method, (int*)attempts, (int64_t*)a0, (int64_t*)a1,
                     (int64_t*)a2, (int64_t*)tag);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
