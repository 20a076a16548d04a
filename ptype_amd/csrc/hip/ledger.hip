// Send ledger accounting (ledger.hpp has the word layout and the digest formula;
// ops/ledger.py the wrapper and the numpy reference).
//
//   ledger_account_kernel   one launch per Send, one block per tile of kLedgerTile
//                           messages: the tile's replies and batch columns are read
//                           once and folded into the ledger words in HBM
//
// No global atomic per message for the counters.  A block issues at most one global
// atomic per non-empty calls bin, one each for digest_sum / digest_xor and, when
// non-zero, audited / mismatch / load_oob; the block that wins the launch's ticket
// adds the Send itself (sends, messages).  The bin almost every message falls into
// -- (the uniform method, or the method of the tile's first message, OK) -- is
// counted in a register per thread; every other bin goes to a per-wave LDS
// histogram.  Digests and counts are reduced by wave shuffles, then over the four
// waves through LDS.
//
// Per-actor load (optional, the LOAD instantiation): same-address global atomics
// serialise device-wide (7-10 ns each), so the messages of one actor are combined
// before they reach HBM, in two steps.  Per row of 64 ids, up to kLedgerPeel rounds
// take the first pending lane's id as leader, ballot the lanes that hold the same id
// and let the leader add the popcount; lanes still pending add 1 themselves.  These
// adds go to a per-block LDS table of kLedgerSlots (actor id, count) pairs: a slot is
// claimed by compare-and-swap, an id that finds its slot taken by another id adds to
// HBM directly, and at the end of the tile every claimed slot is flushed with one
// global atomic.  A hot actor under Zipf traffic thus costs one global atomic per
// block instead of one per message.  Counts are exact whichever way an add takes.
//
// Tile layout as in retry.hip: 256 threads x kLedgerRows rows; row j of wave w, lane
// l covers the messages  tile * kLedgerTile + (j * 4 + w) * 256 + l * 4 + {0, 1, 2, 3}:
// a wave reads 1 KiB of status (one dwordx4 per lane) and 2 KiB of value (two)
// contiguously.
#include "common.hpp"
#include "ledger.hpp"

namespace ptype {

constexpr int kLedgerThreads = 256;
constexpr int kLedgerWaves = kLedgerThreads / kWave;
constexpr int kLedgerRows = 8;                                     // 4-message rows per thread
constexpr int kLedgerTile = kLedgerThreads * kLedgerRows * 4;      // 8192 messages
constexpr int kLedgerBins = kLedgerMethodSlots * kLedgerStatusSlots;
constexpr int kLedgerPeel = 2;                                     // leader rounds of the load combine
constexpr int kLedgerSlotBits = 11;
constexpr int kLedgerSlots = 1 << kLedgerSlotBits;                 // LDS combine table: 16 KiB
constexpr unsigned kLedgerSlotEmpty = 0xffffffffu;                 // (an id in the load table is below 2^32 - 1)

__device__ __forceinline__ unsigned ledger_method_slot(unsigned m16) {
  return m16 < (unsigned)(kLedgerMethodSlots - 1) ? m16 : (unsigned)(kLedgerMethodSlots - 1);
}
__device__ __forceinline__ unsigned ledger_status_slot(int s) {
  return (unsigned)s < (unsigned)(kLedgerStatusSlots - 1) ? (unsigned)s : (unsigned)(kLedgerStatusSlots - 1);
}

// Four consecutive elements at index i (a multiple of 4; the column is aligned for
// the vector load).  Elements at or past M read as 0 and are never used.
__device__ __forceinline__ void ledger_load4(const int* __restrict__ p, int64_t i, int64_t M, int (&o)[4]) {
  if (i + 4 <= M) {
    const int4 v = *reinterpret_cast<const int4*>(p + i);
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = i + c < M ? p[i + c] : 0;
}
__device__ __forceinline__ void ledger_load4(const int64_t* __restrict__ p, int64_t i, int64_t M, int64_t (&o)[4]) {
  if (i + 4 <= M) {
    const I64x2 lo = *reinterpret_cast<const I64x2*>(p + i);
    const I64x2 hi = *reinterpret_cast<const I64x2*>(p + i + 2);
    o[0] = lo.x, o[1] = lo.y, o[2] = hi.x, o[3] = hi.y;
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = i + c < M ? p[i + c] : 0;
}
__device__ __forceinline__ void ledger_load4(const int16_t* __restrict__ p, int64_t i, int64_t M, int16_t (&o)[4]) {
  if (i + 4 <= M) {
    const I16x4 v = *reinterpret_cast<const I16x4*>(p + i);
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = i + c < M ? p[i + c] : (int16_t)0;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (int o = kWave / 2; o; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, kWave);
  return v;
}
__device__ __forceinline__ uint64_t wave_xor64(uint64_t v) {
#pragma unroll
  for (int o = kWave / 2; o; o >>= 1) v ^= (uint64_t)__shfl_xor((unsigned long long)v, o, kWave);
  return v;
}

// load[id] += n through the block's LDS table (id < n_load).
__device__ __forceinline__ void ledger_slot_add(unsigned* __restrict__ keys, unsigned* __restrict__ cnt,
                                                unsigned long long* __restrict__ load, unsigned id, unsigned n) {
  const unsigned slot = (id * 0x9e3779b1u) >> (32 - kLedgerSlotBits);
  const unsigned old = atomicCAS(&keys[slot], kLedgerSlotEmpty, id);
  if (old == kLedgerSlotEmpty || old == id)
    atomicAdd(&cnt[slot], n);
  else
    atomicAdd(&load[id], (unsigned long long)n);
}

// One id per lane (`live` lanes only): load[id] += 1, exact, repeated ids combined.
__device__ __forceinline__ void ledger_load_add(unsigned* __restrict__ keys, unsigned* __restrict__ cnt,
                                                unsigned long long* __restrict__ load, bool live, unsigned id,
                                                unsigned lane) {
  uint64_t pending = __ballot(live);  // wave-uniform, so the loop is too
#pragma unroll
  for (int r = 0; r < kLedgerPeel; ++r) {
    if (!pending) return;
    const unsigned leader = (unsigned)__ffsll((unsigned long long)pending) - 1u;
    const unsigned lead_id = (unsigned)__builtin_amdgcn_readlane((int)id, (int)leader);
    const uint64_t same = __ballot(((pending >> lane) & 1ull) && id == lead_id);
    if (lane == leader) ledger_slot_add(keys, cnt, load, lead_id, (unsigned)__popcll(same));
    pending &= ~same;
  }
  if ((pending >> lane) & 1ull) ledger_slot_add(keys, cnt, load, id, 1u);
}

template <bool LOAD>
__global__ __launch_bounds__(kLedgerThreads) void ledger_account_kernel(
    const int* __restrict__ status, const int64_t* __restrict__ value, int64_t M, const int* __restrict__ actor,
    const int16_t* __restrict__ method_col, unsigned method_uniform, const int64_t* __restrict__ a0,
    const int64_t* __restrict__ a1, unsigned long long* __restrict__ ledger, unsigned long long* __restrict__ load,
    unsigned n_load, unsigned* __restrict__ ticket) {
  __shared__ unsigned hist[kLedgerWaves][kLedgerBins];
  __shared__ uint64_t red[kLedgerWaves][3];
  __shared__ unsigned keys[LOAD ? kLedgerSlots : 1], cnt[LOAD ? kLedgerSlots : 1];
  const unsigned tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * kLedgerTile;
  ledger += (blockIdx.x % kLedgerCopies) * kLedgerWords;  // this block's copy (ledger.hpp)

  for (unsigned k = tid; k < (unsigned)(kLedgerWaves * kLedgerBins); k += kLedgerThreads) (&hist[0][0])[k] = 0;
  if constexpr (LOAD) {
    for (unsigned k = tid; k < (unsigned)kLedgerSlots; k += kLedgerThreads) keys[k] = kLedgerSlotEmpty, cnt[k] = 0;
  }
  __syncthreads();

  // the bin counted in registers: (uniform method | method of the tile's first message, OK)
  unsigned fast_m = method_uniform & 0xffffu;
  if (method_col && base < M) fast_m = (uint16_t)method_col[base];
  const unsigned fast_bin = ledger_method_slot(fast_m) * kLedgerStatusSlots;
  // a uniform method that is never audited needs no argument column at all
  const bool audit_any = a0 && (method_col || fast_m == kCalculatorMultiply || fast_m == kEcho);

  uint64_t dsum = 0, dxor = 0;
  unsigned n_fast = 0, n_audit = 0, n_bad = 0, n_oob = 0;
#pragma unroll 4
  for (int j = 0; j < kLedgerRows; ++j) {
    const int64_t i = base + (int64_t)(j * kLedgerWaves + (int)wave) * (kWave * 4) + lane * 4;
    int s[4], act[4] = {0, 0, 0, 0};
    int64_t v[4], x0[4] = {0, 0, 0, 0}, x1[4] = {0, 0, 0, 0};
    int16_t mc[4] = {0, 0, 0, 0};
    ledger_load4(status, i, M, s);
    ledger_load4(value, i, M, v);
    if (method_col) ledger_load4(method_col, i, M, mc);
    if (audit_any) ledger_load4(a0, i, M, x0);
    if (audit_any && a1) ledger_load4(a1, i, M, x1);
    if constexpr (LOAD) ledger_load4(actor, i, M, act);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool live = i + c < M;
      const unsigned m = method_col ? (unsigned)(uint16_t)mc[c] : fast_m;
      if (live) {
        const unsigned bin = ledger_method_slot(m) * kLedgerStatusSlots + ledger_status_slot(s[c]);
        if (bin == fast_bin)
          ++n_fast;
        else
          atomicAdd(&hist[wave][bin], 1u);
        const bool ok = s[c] == kStatusOk;
        const uint64_t h = mix64(mix64((uint64_t)(i + c) + 1ull) ^ (ok ? (uint64_t)v[c] : 0ull) ^
                                 ((uint64_t)(uint32_t)s[c] * kLedgerGold));
        dsum += h;
        dxor ^= h;
        if (ok && audit_any && (m == kCalculatorMultiply || m == kEcho)) {
          const uint64_t want = m == kEcho ? (uint64_t)x0[c] : (uint64_t)x0[c] * (uint64_t)x1[c];
          ++n_audit;
          n_bad += want != (uint64_t)v[c];
        }
      }
      if constexpr (LOAD) {  // (every lane of the wave takes part in the ballots)
        const bool in = live && (unsigned)act[c] < n_load;
        n_oob += live && !in;
        ledger_load_add(keys, cnt, load, in, (unsigned)act[c], lane);
      }
    }
  }

  // block totals: four 16-bit counts (each at most kLedgerTile) in one word
  uint64_t packed = (uint64_t)n_fast | (uint64_t)n_audit << 16 | (uint64_t)n_bad << 32 | (uint64_t)n_oob << 48;
  dsum = wave_sum64(dsum);
  dxor = wave_xor64(dxor);
  packed = wave_sum64(packed);
  if (lane == 0) red[wave][0] = dsum, red[wave][1] = dxor, red[wave][2] = packed;
  __syncthreads();
  if constexpr (LOAD) {
    for (unsigned k = tid; k < (unsigned)kLedgerSlots; k += kLedgerThreads) {
      if (keys[k] != kLedgerSlotEmpty) atomicAdd(&load[keys[k]], (unsigned long long)cnt[k]);
    }
  }
  if (tid < (unsigned)kLedgerBins) {
    unsigned n = 0;
#pragma unroll
    for (int w = 0; w < kLedgerWaves; ++w) n += hist[w][tid];
    if (tid == fast_bin) {
#pragma unroll
      for (int w = 0; w < kLedgerWaves; ++w) n += (unsigned)(red[w][2] & 0xffffu);
    }
    if (n) atomicAdd(&ledger[kLedgerCalls + tid], (unsigned long long)n);
  } else if (tid == (unsigned)kLedgerBins) {
    if (base < M) atomicAdd(&ledger[kLedgerDigestSum], (unsigned long long)(red[0][0] + red[1][0] + red[2][0] + red[3][0]));
  } else if (tid == (unsigned)kLedgerBins + 1) {
    if (base < M) atomicXor(&ledger[kLedgerDigestXor], (unsigned long long)(red[0][1] ^ red[1][1] ^ red[2][1] ^ red[3][1]));
  } else if (tid == (unsigned)kLedgerBins + 2) {
    const uint64_t p = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    const unsigned long long au = (p >> 16) & 0xffffu, bad = (p >> 32) & 0xffffu, oob = (p >> 48) & 0xffffu;
    if (au) atomicAdd(&ledger[kLedgerAudited], au);
    if (bad) atomicAdd(&ledger[kLedgerMismatch], bad);
    if (oob) atomicAdd(&ledger[kLedgerLoadOob], oob);
  } else if (tid == (unsigned)kLedgerBins + 3) {
    // one block per launch counts the Send and its messages (the counts order
    // nothing: a reader synchronises with the stream, not with these words)
    if (last_block_ticket(ticket)) {
      atomicAdd(&ledger[kLedgerSends], 1ull);
      if (M) atomicAdd(&ledger[kLedgerMessages], (unsigned long long)M);
    }
  }
}
static_assert(kLedgerWaves == 4, "the block reduction reads four waves' partials");
static_assert(kLedgerTile < (1 << 16), "block totals are packed as 16-bit counts");

int64_t ledger_tile() { return kLedgerTile; }

// `ledger`: kLedgerCopies * kLedgerWords int64; `ticket`: kTicketWords u32, zero between launches;
// `load`: n_load int64 or null.  status / value / actor / a0 / a1 16-byte aligned,
// method_col 8-byte aligned.  An empty Send (M = 0) still counts one Send.
void launch_ledger_account(uintptr_t status, uintptr_t value, int64_t M, uintptr_t actor, uintptr_t method_col,
                           uint32_t method_uniform, uintptr_t a0, uintptr_t a1, uintptr_t ledger, uintptr_t load,
                           int64_t n_load, uintptr_t ticket, uintptr_t stream) {
  if (M < 0 || M > 0x7fffffffll) throw std::invalid_argument("ledger_account: M must be in [0, 2^31 - 1]");
  if (!ledger || !ticket) throw std::invalid_argument("ledger_account: null ledger or ticket buffer");
  if (M > 0 && (!status || !value || (load && !actor))) throw std::invalid_argument("ledger_account: null column");
  if (load && (n_load <= 0 || n_load >= 0xffffffffll)) throw std::invalid_argument("ledger_account: n_load out of range");
  if ((status | value | actor | a0 | a1) & 15u || method_col & 7u)
    throw std::invalid_argument("ledger_account: columns must be 16-byte aligned (the method column 8-byte)");
  const unsigned tiles = M ? (unsigned)((M + kLedgerTile - 1) / kLedgerTile) : 1u;
  auto kernel = load ? ledger_account_kernel<true> : ledger_account_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kLedgerThreads), 0, as_stream(stream), (const int*)status,
                     (const int64_t*)value, M, (const int*)actor, (const int16_t*)method_col, method_uniform,
                     (const int64_t*)a0, (const int64_t*)a1, (unsigned long long*)ledger, (unsigned long long*)load,
                     load ? (unsigned)n_load : 0u, (unsigned*)ticket);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
