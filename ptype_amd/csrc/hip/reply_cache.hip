// Reply cache (`DeviceRuntime.send(cache=True)`, ops/reply_cache.py; reply_cache.hpp has
// the entry, the key and the claim word).  The cache that sits next to singleflight in a
// Go service, on the batch path: a pure call whose STATUS_OK reply an earlier Send of this
// runtime stored is answered from HBM and never sent.
//
//   reply_cache_lookup_kernel  over the M messages: key columns loaded coalesced, hashed,
//                              the entry at slot = hash & mask read and all five key
//                              fields and the epoch compared.  A hit writes val[i] and
//                              st[i] = STATUS_OK; a miss and every non-pure message (which
//                              reads no entry) get st[i] = kReplyCachePending, the marker
//                              retry_select compacts by
//   reply_cache_claim_kernel   over the K rows of the sub-batch after the inner Send: a
//                              row that is pure and got STATUS_OK lowers its slot's claim
//                              word (64-bit atomicMin) to (0xFFFFFFFF - seq) << 32 | row
//   reply_cache_write_kernel   the next launch, over the same rows: the row whose claim
//                              word is the slot's writes key, value and epoch
//   reply_cache_clear_kernel   every entry: zero, claim all ones, epoch 0 (the initial
//                              table, and the rewrite when epoch or seq would wrap)
//
// Why the table is exact and deterministic.  seq rises by one per insert, so a newer
// Send's claim words are all smaller than every older one's and the newest Send always
// replaces; within a Send the lowest row wins.  The claim word is only ever lowered by
// device-scope atomics (launch 2) and only read in launch 3; an entry's other words are
// written by exactly one thread of launch 3 (the claim's owner) and read by the next
// lookup.  The launch boundaries are the only ordering.  clear() is epoch += 1 on the
// host: the entries stay, no lookup matches them, and their claim words lose to every
// later Send's.
#include "reply_cache.hpp"

namespace ptype {

constexpr int kRcThreads = 256;
constexpr int kRcRows = 4;                        // messages per thread of the lookup
constexpr int kRcTile = kRcThreads * kRcRows;     // 1024 messages per block
constexpr uint32_t kRcNoSlot = 0xffffffffu;       // not pure, or past M: no entry is read

struct RcIn {  // by value
  const uint32_t* actor;
  const uint16_t* mcol;  // null: method_uniform
  uint32_t method_uniform;
  const int64_t* a0;
  const int64_t* a1;  // null: 0
  const int64_t* a2;  // null: 0
  int64_t M;
};

struct alignas(16) RcKey {  // the first 32 bytes of an entry
  uint64_t k0;
  int64_t x0, x1, x2;
};

__device__ __forceinline__ RcKey rc_load(const RcIn& in, int64_t i, uint32_t& method) {
  method = in.mcol ? (uint32_t)in.mcol[i] : (in.method_uniform & 0xffffu);
  RcKey k;
  k.k0 = reply_cache_k0(in.actor[i], method);
  k.x0 = in.a0[i];
  k.x1 = in.a1 ? in.a1[i] : 0;
  k.x2 = in.a2 ? in.a2[i] : 0;
  return k;
}

__device__ __forceinline__ uint32_t rc_slot(const RcKey& k, uint32_t mask) {
  return (uint32_t)coalesce_hash((uint32_t)k.k0, (uint32_t)(k.k0 >> 32), k.x0, k.x1, k.x2) & mask;
}

__device__ __forceinline__ bool rc_eq4(const uint4& a, const uint4& b) {
  return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
}

// One lane reads its message's entry as four 16-B loads, the loads of its kRcRows messages
// issued together.  (The other shape -- four lanes share an entry, a wave instruction
// touching 16 whole lines, keys staged in LDS and a ballot per quad -- was built and
// timed next to this one: 210.2 us against 207.3 us for 8 Mi cold probes, 27.9 us against
// 26.2 us for 1 Mi, one run each and within the spread between runs, profiles/
// reply_cache.md.  Sharing lines did not help, so the simpler one stayed.)
__global__ __launch_bounds__(kRcThreads) void reply_cache_lookup_kernel(RcIn in,
                                                                         const ReplyCacheEntry* __restrict__ table,
                                                                         uint32_t mask, uint32_t epoch,
                                                                         int64_t* __restrict__ val,
                                                                         int* __restrict__ st) {
  const int64_t base = (int64_t)blockIdx.x * kRcTile;
  RcKey key[kRcRows];
  uint32_t slot[kRcRows];
  uint4 w[kRcRows][4];
#pragma unroll
  for (int r = 0; r < kRcRows; ++r) {
    const int64_t i = base + r * kRcThreads + (int)threadIdx.x;
    slot[r] = kRcNoSlot;
    if (i < in.M) {
      uint32_t method;
      key[r] = rc_load(in, i, method);
      if (method_pure(method)) slot[r] = rc_slot(key[r], mask);
    }
  }
#pragma unroll
  for (int r = 0; r < kRcRows; ++r) {
    if (slot[r] == kRcNoSlot) continue;
    const uint4* e = reinterpret_cast<const uint4*>(table + slot[r]);
#pragma unroll
    for (int c = 0; c < 4; ++c) w[r][c] = e[c];
  }
#pragma unroll
  for (int r = 0; r < kRcRows; ++r) {
    const int64_t i = base + r * kRcThreads + (int)threadIdx.x;
    if (i >= in.M) continue;
    bool hit = false;
    if (slot[r] != kRcNoSlot) {
      const uint4* k = reinterpret_cast<const uint4*>(&key[r]);
      hit = rc_eq4(w[r][0], k[0]) && rc_eq4(w[r][1], k[1]) && w[r][3].x == epoch;
    }
    if (hit) val[i] = (int64_t)((uint64_t)w[r][2].y << 32 | w[r][2].x);
    st[i] = hit ? (int)kStatusOk : kReplyCachePending;
  }
}

// Row j of the sub-batch may be stored: a pure method that got STATUS_OK (in a sub-batch
// of misses every pure row missed).
__device__ __forceinline__ bool rc_storable(const RcIn& in, const int* __restrict__ st, int64_t j, RcKey& k) {
  if (st[j] != (int)kStatusOk) return false;
  uint32_t method;
  k = rc_load(in, j, method);
  return method_pure(method);
}

__global__ __launch_bounds__(kRcThreads) void reply_cache_claim_kernel(RcIn in, const int* __restrict__ st,
                                                                        ReplyCacheEntry* __restrict__ table,
                                                                        uint32_t mask, uint32_t seq) {
  const int64_t j = (int64_t)blockIdx.x * kRcThreads + threadIdx.x;
  if (j >= in.M) return;
  RcKey k;
  if (!rc_storable(in, st, j, k)) return;
  atomicMin(reinterpret_cast<unsigned long long*>(&table[rc_slot(k, mask)].claim),
            (unsigned long long)reply_cache_claim(seq, (uint32_t)j));
}

__global__ __launch_bounds__(kRcThreads) void reply_cache_write_kernel(RcIn in, const int64_t* __restrict__ val,
                                                                        const int* __restrict__ st,
                                                                        ReplyCacheEntry* __restrict__ table,
                                                                        uint32_t mask, uint32_t seq, uint32_t epoch) {
  const int64_t j = (int64_t)blockIdx.x * kRcThreads + threadIdx.x;
  if (j >= in.M) return;
  RcKey k;
  if (!rc_storable(in, st, j, k)) return;
  ReplyCacheEntry* e = table + rc_slot(k, mask);
  if (e->claim != reply_cache_claim(seq, (uint32_t)j)) return;
  *reinterpret_cast<RcKey*>(e) = k;
  e->value = val[j];
  e->epoch = epoch;
}

__global__ __launch_bounds__(kRcThreads) void reply_cache_clear_kernel(uint4* __restrict__ table, int64_t pieces) {
  for (int64_t t = blockIdx.x * (int64_t)kRcThreads + threadIdx.x; t < pieces; t += (int64_t)gridDim.x * kRcThreads)
    table[t] = (t & 3) == 2 ? make_uint4(0u, 0u, 0xffffffffu, 0xffffffffu) : make_uint4(0u, 0u, 0u, 0u);  // (value, claim)
}

// ---------------------------------------------------------------- launchers
int64_t reply_cache_tile() { return kRcTile; }

static RcIn rc_in(const char* what, uintptr_t actor, uintptr_t method_col, uint32_t method_uniform, uintptr_t a0,
                  uintptr_t a1, uintptr_t a2, int64_t M, uintptr_t table, int table_log2) {
  if (M > 0x7fffffffll) throw std::invalid_argument(std::string(what) + ": more than 2^31 - 1 messages");
  if (table_log2 < kReplyCacheMinLog2 || table_log2 > kReplyCacheMaxLog2)
    throw std::invalid_argument(std::string(what) + ": table_log2 out of range");
  if (!actor || !a0 || !table) throw std::invalid_argument(std::string(what) + ": null buffer");
  if (actor & 3u || (a0 | a1 | a2) & 7u || method_col & 1u || table & 63u)
    throw std::invalid_argument(std::string(what) + ": misaligned column or table");
  return RcIn{(const uint32_t*)actor, (const uint16_t*)method_col, method_uniform, (const int64_t*)a0,
              (const int64_t*)a1, (const int64_t*)a2, M};
}

// actor int32 / a0..a2 int64 / method_col u16 columns of M rows (naturally aligned); a
// null a1 / a2 counts as 0, a null method_col means method_uniform.  table: 1 << table_log2
// entries of 64 B, 64-byte aligned.  val int64[M] (written on a hit only), st int32[M].
void launch_reply_cache_lookup(uintptr_t actor, uintptr_t method_col, uint32_t method_uniform, uintptr_t a0,
                               uintptr_t a1, uintptr_t a2, int64_t M, uintptr_t table, int table_log2, uint32_t epoch,
                               uintptr_t val, uintptr_t st, uintptr_t stream) {
  if (M <= 0) return;
  const RcIn in = rc_in("reply_cache_lookup", actor, method_col, method_uniform, a0, a1, a2, M, table, table_log2);
  if (!val || !st || val & 7u || st & 3u) throw std::invalid_argument("reply_cache_lookup: null or misaligned output");
  const uint32_t mask = (uint32_t)(((uint64_t)1 << table_log2) - 1u);
  const dim3 grid((unsigned)((M + kRcTile - 1) / kRcTile));
  hipLaunchKernelGGL(reply_cache_lookup_kernel, grid, dim3(kRcThreads), 0, as_stream(stream), in,
                     (const ReplyCacheEntry*)table, mask, epoch, (int64_t*)val, (int*)st);
  PT_HIP_CHECK(hipGetLastError());
}

// The launches of an insert, one at a time (tools/reply_cache_cost.py times them apart; a
// write without its claim, or a reused seq, breaks the replacement rule).  `phases` 1: the
// claim launch, 2: the write launch, 3: both, in that order.
void launch_reply_cache_insert_phase(uintptr_t actor, uintptr_t method_col, uint32_t method_uniform, uintptr_t a0,
                                     uintptr_t a1, uintptr_t a2, int64_t K, uintptr_t val, uintptr_t st,
                                     uintptr_t table, int table_log2, uint32_t epoch, uint32_t seq, int phases,
                                     uintptr_t stream) {
  if (K <= 0) return;
  const RcIn in = rc_in("reply_cache_insert", actor, method_col, method_uniform, a0, a1, a2, K, table, table_log2);
  if (!val || !st || val & 7u || st & 3u) throw std::invalid_argument("reply_cache_insert: null or misaligned replies");
  const uint32_t mask = (uint32_t)(((uint64_t)1 << table_log2) - 1u);
  const dim3 grid((unsigned)((K + kRcThreads - 1) / kRcThreads));
  hipStream_t s = as_stream(stream);
  if (phases & 1) {
    hipLaunchKernelGGL(reply_cache_claim_kernel, grid, dim3(kRcThreads), 0, s, in, (const int*)st,
                       (ReplyCacheEntry*)table, mask, seq);
    PT_HIP_CHECK(hipGetLastError());
  }
  if (phases & 2) {
    hipLaunchKernelGGL(reply_cache_write_kernel, grid, dim3(kRcThreads), 0, s, in, (const int64_t*)val,
                       (const int*)st, (ReplyCacheEntry*)table, mask, seq, epoch);
    PT_HIP_CHECK(hipGetLastError());
  }
}

// The K rows of a sub-batch and their replies (val int64[K], st int32[K]) into the table:
// the claim launch, then the write launch.  seq rises by one per insert.
void launch_reply_cache_insert(uintptr_t actor, uintptr_t method_col, uint32_t method_uniform, uintptr_t a0,
                               uintptr_t a1, uintptr_t a2, int64_t K, uintptr_t val, uintptr_t st, uintptr_t table,
                               int table_log2, uint32_t epoch, uint32_t seq, uintptr_t stream) {
  launch_reply_cache_insert_phase(actor, method_col, method_uniform, a0, a1, a2, K, val, st, table, table_log2, epoch,
                                  seq, 3, stream);
}

void launch_reply_cache_clear(uintptr_t table, int table_log2, uintptr_t stream) {
  if (table_log2 < kReplyCacheMinLog2 || table_log2 > kReplyCacheMaxLog2)
    throw std::invalid_argument("reply_cache_clear: table_log2 out of range");
  if (!table || table & 63u) throw std::invalid_argument("reply_cache_clear: null or misaligned table");
  const int64_t pieces = (int64_t)4 << table_log2;
  int64_t blocks = (pieces + kRcThreads - 1) / kRcThreads;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(reply_cache_clear_kernel, dim3((unsigned)blocks), dim3(kRcThreads), 0, as_stream(stream),
                     (uint4*)table, pieces);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
