// Send coalescing (`DeviceRuntime.send(coalesce=True)`, ops/coalesce.py; coalesce.hpp
// has the key, the pure methods and the hash).  The reference's services are called
// through Go clients whose authors reach for singleflight when many callers ask the
// same pure question at once; on the batch path the duplicates of a pure call are
// found on the device, only each group's first message is sent, and its reply is
// copied to the others.
//
//   coalesce_insert_kernel   launch 1: every pure message's key goes into an open-
//                            addressing table of u32 slots (message index + 1); a key
//                            class keeps ONE slot, which ends up holding the class's
//                            lowest index
//   coalesce_lead_kernel     launch 2: every message re-walks its probe chain and reads
//                            its class's slot: lead[i]; a non-pure message gets lead[i] = i
//   compact.hpp              stable compaction of the messages with lead[i] == i (the one
//                            retry.hip compacts by status with): idx, the gathered columns,
//                            K and pos[i] = i's row in the sub-batch (-1 for a follower)
//   coalesce_fanout_kernel   val[i] = v2[pos[lead[i]]], st[i] = s2[pos[lead[i]]]
//
// Why the table is exact and deterministic.  A slot is claimed by a compare-and-swap
// on 0 and never emptied; afterwards only members of the SAME key class lower it
// (atomicMin), so a slot's class never changes.  A message walks from its home slot
// past slots of other classes and stops at the first slot that is empty (it claims
// it) or of its own class; every slot it passed was occupied and stays occupied by
// that other class, so every member of a class stops at the same slot, whatever the
// scheduling, and that slot's final value is the minimum over the members that
// reached it.  Classes are decided by comparing all five key fields against the batch
// columns at the resident index -- the hash only picks the home slot.  The table has
// at least 2 M slots, so a walk always meets an empty slot.
//
// Every access to the table in launch 1 is a device-scope atomic read-modify-write
// (the per-XCD L2s are not coherent within a launch; an atomic executes at the memory
// side), and launch 2 only reads it after launch 1 has ended.  The batch columns are
// inputs of both launches.
//
// Same-address atomics serialise device-wide (7-11 ns each), so the members of a
// class are thinned out before they reach HBM; dropping any member but the lowest
// leaves the result unchanged, since launch 2 looks every message up again.  (1) Per
// row of 64 messages a wave takes, kCoPeel times, the first pending lane's key,
// ballots the lanes that hold the same key and drops all of them but that first lane
// (a row is in index order, so the first lane is the lowest index).  (2) The lanes
// left go to a per-block LDS table of kCoSlots tile-local indices: claimed by
// compare-and-swap, lowered by atomicMin on an equal key; a message that finds its
// slot held by another class goes to HBM itself.  (3) After the tile, the message
// whose index a slot holds inserts its key into HBM: an all-identical batch costs one
// global atomic per block.
#include "coalesce.hpp"
#include "compact.hpp"

namespace ptype {

constexpr int kCoThreads = 256;
constexpr int kCoWaves = kCoThreads / kWave;
constexpr int kCoRows = 8;                             // messages per thread
constexpr int kCoTile = kCoThreads * kCoRows;          // 2048 messages per block
constexpr int kCoPeel = 2;                             // leader rounds of the wave combine
constexpr int kCoSlotBits = 12;
constexpr int kCoSlots = 1 << kCoSlotBits;             // LDS combine table: 16 KiB, 2 slots per message

struct CoIn {  // by value
  const uint32_t* actor;
  const uint16_t* mcol;  // null: method_uniform
  uint32_t method_uniform;
  const int64_t* a0;
  const int64_t* a1;  // null: 0
  const int64_t* a2;  // null: 0
  int64_t M;
};

struct CoKey {
  uint32_t actor, method;
  int64_t x0, x1, x2;
};

__device__ __forceinline__ CoKey co_load(const CoIn& in, int64_t i) {
  CoKey k;
  k.actor = in.actor[i];
  k.method = in.mcol ? (uint32_t)in.mcol[i] : (in.method_uniform & 0xffffu);
  k.x0 = in.a0[i];
  k.x1 = in.a1 ? in.a1[i] : 0;
  k.x2 = in.a2 ? in.a2[i] : 0;
  return k;
}

__device__ __forceinline__ bool co_eq(const CoKey& a, const CoKey& b) {
  return a.actor == b.actor && a.method == b.method && a.x0 == b.x0 && a.x1 == b.x1 && a.x2 == b.x2;
}

__device__ __forceinline__ uint64_t co_hash(const CoKey& k) {
  return coalesce_hash(k.actor, k.method, k.x0, k.x1, k.x2);
}

__device__ __forceinline__ int64_t co_readlane64(int64_t v, unsigned lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), (int)lane);
  return (int64_t)((uint64_t)hi << 32 | lo);
}

// Message i (key k, hash h) into the HBM table.  Bounded: at most mask + 1 probes.
__device__ __forceinline__ void co_insert(const CoIn& in, unsigned* __restrict__ table, uint32_t mask, uint64_t h,
                                          uint32_t i, const CoKey& k) {
  uint32_t slot = (uint32_t)h & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const unsigned old = atomicCAS(&table[slot], 0u, i + 1u);
    if (old == 0u) return;  // claimed
    const uint32_t j = old - 1u;
    if ((int64_t)j < in.M && co_eq(co_load(in, j), k)) {  // (j < M always: the table was cleared for this batch)
      if (i < j) atomicMin(&table[slot], i + 1u);
      return;
    }
    slot = (slot + 1u) & mask;
  }
}

__global__ __launch_bounds__(kCoThreads) void coalesce_insert_kernel(CoIn in, unsigned* __restrict__ table,
                                                                      uint32_t mask) {
  __shared__ unsigned lds[kCoSlots];
  const unsigned tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * kCoTile;
  for (unsigned s = tid; s < (unsigned)kCoSlots; s += kCoThreads) lds[s] = 0u;
  __syncthreads();

  CoKey key[kCoRows];
  uint64_t hash[kCoRows];
  unsigned how[kCoRows];  // 0: dropped (or not pure), 1: its LDS slot decides, 2: to HBM itself
#pragma unroll
  for (int r = 0; r < kCoRows; ++r) {
    const int64_t i = base + (int64_t)(r * kCoWaves + (int)wave) * kWave + lane;
    const bool live = i < in.M;
    key[r] = live ? co_load(in, i) : CoKey{0u, 0u, 0, 0, 0};
    hash[r] = co_hash(key[r]);
    bool mine = live && method_pure(key[r].method);
    // (1) within the row: the first lane of a repeated key stands for all its lanes
    uint64_t pending = __ballot(mine);  // wave-uniform, so the loop is too
#pragma unroll
    for (int p = 0; p < kCoPeel; ++p) {
      if (!pending) break;
      const unsigned first = (unsigned)__ffsll((unsigned long long)pending) - 1u;
      CoKey f;
      f.actor = (uint32_t)__builtin_amdgcn_readlane((int)key[r].actor, (int)first);
      f.method = (uint32_t)__builtin_amdgcn_readlane((int)key[r].method, (int)first);
      f.x0 = co_readlane64(key[r].x0, first);
      f.x1 = co_readlane64(key[r].x1, first);
      f.x2 = co_readlane64(key[r].x2, first);
      const uint64_t same = __ballot(((pending >> lane) & 1ull) && co_eq(key[r], f));
      if (((same >> lane) & 1ull) && lane != first) mine = false;
      pending &= ~same;
    }
    // (2) within the block
    how[r] = 0u;
    if (mine) {
      const unsigned slot = (unsigned)(hash[r] >> 40) & (unsigned)(kCoSlots - 1);
      const unsigned local = (unsigned)(i - base) + 1u;
      const unsigned old = atomicCAS(&lds[slot], 0u, local);
      if (old == 0u) {
        how[r] = 1u;
      } else if (co_eq(co_load(in, base + (int64_t)old - 1), key[r])) {  // (a live message of this tile)
        atomicMin(&lds[slot], local);
        how[r] = 1u;
      } else {
        how[r] = 2u;
      }
    }
  }
  __syncthreads();
  // (3) the block's lowest member of every key it holds, and the messages the LDS table had no room for
#pragma unroll
  for (int r = 0; r < kCoRows; ++r) {
    const int64_t i = base + (int64_t)(r * kCoWaves + (int)wave) * kWave + lane;
    bool go = how[r] == 2u;
    if (how[r] == 1u) go = lds[(unsigned)(hash[r] >> 40) & (unsigned)(kCoSlots - 1)] == (unsigned)(i - base) + 1u;
    if (go) co_insert(in, table, mask, hash[r], (uint32_t)i, key[r]);
  }
}

__global__ __launch_bounds__(kCoThreads) void coalesce_lead_kernel(CoIn in, const unsigned* __restrict__ table,
                                                                    uint32_t mask, int* __restrict__ lead) {
  const int64_t i = (int64_t)blockIdx.x * kCoThreads + threadIdx.x;
  if (i >= in.M) return;
  const CoKey k = co_load(in, i);
  uint32_t l = (uint32_t)i;
  if (method_pure(k.method)) {
    uint32_t slot = (uint32_t)co_hash(k) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
      const unsigned cur = table[slot];
      if (cur == 0u) break;  // (never: launch 1 left this key's class a slot on this chain)
      const uint32_t j = cur - 1u;
      if (j == (uint32_t)i) break;
      if ((int64_t)j < in.M && co_eq(co_load(in, j), k)) {
        l = j;
        break;
      }
      slot = (slot + 1u) & mask;
    }
  }
  lead[i] = (int)l;
}

// ---------------------------------------------------------------- fan-out
// The reply of message i's leader.  A lead or pos outside its range (never, for the
// outputs of the kernels above) reads nothing and answers kStatusNotDelivered.
__device__ __forceinline__ void co_fetch(int l, const int* __restrict__ pos, const int64_t* __restrict__ v2,
                                         const int* __restrict__ s2, int64_t M, int64_t K, int64_t& v, int& s) {
  v = 0;
  s = kStatusNotDelivered;
  if ((uint64_t)l >= (uint64_t)M) return;
  const int p = pos[l];
  if ((uint64_t)p >= (uint64_t)K) return;
  v = v2[p];
  s = s2[p];
}

__global__ __launch_bounds__(256) void coalesce_fanout_kernel(int64_t* __restrict__ val, int* __restrict__ st,
                                                               int64_t M, const int* __restrict__ lead,
                                                               const int* __restrict__ pos,
                                                               const int64_t* __restrict__ v2,
                                                               const int* __restrict__ s2, int64_t K) {
  const int64_t groups = (M + 3) / 4;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = g * 4;
    int64_t v[4];
    int s[4];
    if (i + 4 <= M) {  // lead, val and st are 16-byte aligned
      const int4 l = *reinterpret_cast<const int4*>(lead + i);
      co_fetch(l.x, pos, v2, s2, M, K, v[0], s[0]);
      co_fetch(l.y, pos, v2, s2, M, K, v[1], s[1]);
      co_fetch(l.z, pos, v2, s2, M, K, v[2], s[2]);
      co_fetch(l.w, pos, v2, s2, M, K, v[3], s[3]);
      *reinterpret_cast<I64x2*>(val + i) = I64x2{v[0], v[1]};
      *reinterpret_cast<I64x2*>(val + i + 2) = I64x2{v[2], v[3]};
      *reinterpret_cast<int4*>(st + i) = make_int4(s[0], s[1], s[2], s[3]);
    } else {
      for (int c = 0; i + c < M; ++c) {
        co_fetch(lead[i + c], pos, v2, s2, M, K, v[0], s[0]);
        val[i + c] = v[0];
        st[i + c] = s[0];
      }
    }
  }
}

// ---------------------------------------------------------------- launchers
int64_t coalesce_tile() { return kCoTile; }

// `table`: (1 << table_log2) u32 words of workspace, at least 2 M of them; cleared here
// by an asynchronous fill on `stream`.  actor int32 / a0..a2 int64 / method_col u16
// columns of M rows (naturally aligned); a null a1 / a2 counts as 0, a null method_col
// means method_uniform.  lead: int32[M].
void launch_coalesce_group(uintptr_t actor, uintptr_t method_col, uint32_t method_uniform, uintptr_t a0, uintptr_t a1,
                           uintptr_t a2, int64_t M, uintptr_t table, int table_log2, uintptr_t lead,
                           uintptr_t stream) {
  if (M <= 0) return;
  if (table_log2 < kCoalesceMinLog2 || table_log2 > kCoalesceMaxLog2)
    throw std::invalid_argument("coalesce_group: table_log2 out of range");
  if (M > (int64_t)1 << (table_log2 - 1))
    throw std::invalid_argument("coalesce_group: the table must have at least 2 M slots");
  if (!actor || !a0 || !table || !lead) throw std::invalid_argument("coalesce_group: null buffer");
  if ((actor | table | lead) & 3u || (a0 | a1 | a2) & 7u || method_col & 1u)
    throw std::invalid_argument("coalesce_group: misaligned column");
  hipStream_t s = as_stream(stream);
  const CoIn in{(const uint32_t*)actor, (const uint16_t*)method_col, method_uniform, (const int64_t*)a0,
                (const int64_t*)a1, (const int64_t*)a2, M};
  const uint32_t mask = (uint32_t)(((uint64_t)1 << table_log2) - 1u);
  PT_HIP_CHECK(hipMemsetAsync((void*)table, 0, (size_t)4 << table_log2, s));
  hipLaunchKernelGGL(coalesce_insert_kernel, dim3((unsigned)((M + kCoTile - 1) / kCoTile)), dim3(kCoThreads), 0, s, in,
                     (unsigned*)table, mask);
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(coalesce_lead_kernel, dim3((unsigned)((M + kCoThreads - 1) / kCoThreads)), dim3(kCoThreads), 0, s,
                     in, (const unsigned*)table, mask, (int*)lead);
  PT_HIP_CHECK(hipGetLastError());
}

// `counts`: ceil(M / retry_tile()) u32 words of workspace.  The output columns
// hold up to M rows; a null input column leaves its output alone.  lead and pos are
// 16-byte aligned.
void launch_coalesce_select(uintptr_t lead, int64_t M, uintptr_t actor, uintptr_t a0, uintptr_t a1, uintptr_t a2,
                            uintptr_t method, uintptr_t idx, uintptr_t pos, uintptr_t actor_o, uintptr_t a0_o,
                            uintptr_t a1_o, uintptr_t a2_o, uintptr_t method_o, uintptr_t counts, uintptr_t k_out,
                            uintptr_t stream) {
  if (M <= 0) return;
  if (M > 0x7fffffffll) throw std::invalid_argument("coalesce_select: more than 2^31 - 1 messages");
  if ((lead | pos) & 15u) throw std::invalid_argument("coalesce_select: lead and pos must be 16-byte aligned");
  if (!lead || !actor || !a0 || !idx || !pos || !actor_o || !a0_o || !counts || !k_out || (a1 && !a1_o) ||
      (a2 && !a2_o) || (method && !method_o))
    throw std::invalid_argument("coalesce_select: null buffer");
  launch_compact<OwnIndex, true>(lead, M, OwnIndex{}, actor, a0, a1, a2, method, idx, pos, actor_o, a0_o, a1_o, a2_o,
                                 method_o, counts, k_out, stream);
}

// val int64[M], st int32[M], lead int32[M]: 16-byte aligned; pos int32[M]; v2 int64[K], s2 int32[K].
void launch_coalesce_fanout(uintptr_t val, uintptr_t st, int64_t M, uintptr_t lead, uintptr_t pos, uintptr_t v2,
                            uintptr_t s2, int64_t K, uintptr_t stream) {
  if (M <= 0) return;
  if (K < 0 || K > M) throw std::invalid_argument("coalesce_fanout: K must be in [0, M]");
  if (!val || !st || !lead || !pos || (K > 0 && (!v2 || !s2))) throw std::invalid_argument("coalesce_fanout: null buffer");
  if ((val | st | lead) & 15u) throw std::invalid_argument("coalesce_fanout: val, st and lead must be 16-byte aligned");
  int64_t blocks = ((M + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(coalesce_fanout_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (int64_t*)val,
                     (int*)st, M, (const int*)lead, (const int*)pos, (const int64_t*)v2, (const int*)s2, K);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
