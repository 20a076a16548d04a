// What the launcher TUs of the sorted epoch mailboxes share (design notes:
// mailbox_sort.hip): record forms and decoders, the resolve / rank / reserve
// helpers and the one-pass sort of a tile, the tile drains the fused kernel
// shares with the drain kernels, the LDS sizes, and the variant tables' types.
// A kernel lives in the TU that launches it -- mailbox_sort.hip (sorts, ring /
// message-order drains), mailbox_sort_fused.hip (the fused sort + drain),
// mailbox_sort_ordered.hip (the ordered drain and the ring-order completion),
// mailbox_sort_arrival.hip (arrival sharding) -- so the variants build in
// parallel instead of as one long object.
#pragma once
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "mailbox.hpp"
#include "mailbox_dev.hpp"
#include "route_common.hpp"
#include "sort_common.hpp"
#include "tune.hpp"

namespace ptype {

namespace {
constexpr uint32_t kCompactMark = 0x80000000u;
constexpr uint32_t kCompactLong = 0x80000000u;
}  // namespace

constexpr uint32_t kNoSlot = 0xffffffffu;
// A stateless batch's message whose shard ring is full SPILLS: the parallel drain
// runs it straight from the batch (its route word + argument columns) in message
// order, like any other -- no STATUS_OVERFLOW, so no re-send round and no host
// read of an overflow count.  Ordered batches keep the ring's
// FIFO and answer kStatusOverflow (send_all re-sends the tail).
constexpr uint32_t kSpillSlot = 0xfffffffeu;
constexpr uint32_t kRunSpilled = 0x80000000u;  // tinfo count word: the run did not fit the ring's room
// s_waitcnt vmcnt(0) as the builtin's gfx9 immediate (expcnt and lgkmcnt left at their maxima).
// The builtin, not inline assembly: the compiler's wait insertion reads it and then knows that no
// load is outstanding, so it adds no waits of its own behind it.
constexpr int kWaitVmcnt0 = 0x0f70;

// ---------------------------------------------------------------- K2s one pass: resolve + look-back + scatter
// The count and scatter passes as ONE kernel (a single-pass counting sort with
// decoupled look-back): each block claims the next tile in launch order (a tile
// counter, so every earlier tile's block is already running), resolves its
// messages through the route directory ONCE (the gather is the expensive part:
// 8 Mi random 4-B lookups cost ~27 us of L2 request rate on MI355X,
// tools/gather_probe.hip), ranks them per shard in message order (wave match),
// publishes its per-shard counts, and finds its offset in each shard's epoch run
// by looking back over earlier tiles' descriptors until one carries an
// inclusive prefix.  Descriptors are u64 {epoch tag 24 | status 2 | value 38},
// published and read with memory-side atomics (the per-XCD L2s are not coherent
// within a kernel); the tag (from a device word the drain advances) makes a
// previous Send's descriptors invalid without clearing them, graph replays
// included.  The last tile leaves each shard's epoch total in gsum[0][s] for the
// drains' commit.  The batch's inputs are read once and the route words never
// leave registers (the two-pass form wrote and re-read 4 B per message).
__host__ __device__ constexpr size_t onesweep_lds_bytes(uint32_t S) { return (size_t)S * (8 + 4 + 4 + 4 * (kST / kWave)); }

template <bool A2, bool MC, int SK = kSK>
__device__ __forceinline__ void load_cols(const SortIn& in, uint32_t t, int64_t (&v0)[SK], int64_t (&v1)[SK],
                                          int64_t (&v2)[SK], uint32_t (&meth)[SK]) {
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const int64_t i = tile_index<SK>(t, k);
    const bool ok = i < in.M;
    v0[k] = ok ? __builtin_nontemporal_load(in.a0 + i) : 0;
    v1[k] = ok && in.a1 ? __builtin_nontemporal_load(in.a1 + i) : 0;
    v2[k] = 0;
    if constexpr (A2) v2[k] = ok ? __builtin_nontemporal_load(in.a2 + i) : 0;
    meth[k] = in.method_uniform;
    if constexpr (MC) meth[k] = ok ? (uint32_t)in.mcol[i] : 0u;
  }
}

// The persistent sort's argument columns.  A tile that lies wholly inside the batch, with a1
// present (`full`: every tile of a Multiply batch but its last): the loads without per-item
// bounds branches, so they issue as one run.  Otherwise the guarded form.  (The 4-B actor
// column keeps the guarded form on every tile: without its branches the kernel takes 133
// VGPRs, three waves per SIMD.)
template <int SK>
__device__ __forceinline__ bool tile_is_full(const SortIn& in, uint32_t t) {
  return in.a1 != nullptr && ((int64_t)t + 1) * (kST * SK) <= (int64_t)in.M;
}
template <int SK>
__device__ __forceinline__ void load_args_tile(const SortIn& in, uint32_t t, bool full, int64_t (&v0)[SK],
                                               int64_t (&v1)[SK]) {
  if (full) {
#pragma unroll
    for (int k = 0; k < SK; ++k) {
      const int64_t i = tile_index<SK>(t, k);
      v0[k] = __builtin_nontemporal_load(in.a0 + i);
      v1[k] = __builtin_nontemporal_load(in.a1 + i);
    }
    // (the run stays a run: left to the scheduler, the 16 loads spread over the next tile's resolve and
    // ranking and the kernel takes 130 VGPRs)
    __builtin_amdgcn_sched_barrier(0);
  } else {
    int64_t v2[SK];
    uint32_t meth[SK];
    load_cols<false, false, SK>(in, t, v0, v1, v2, meth);
  }
}

__device__ __forceinline__ uint32_t bitlen64(uint64_t x) { return x ? 64u - (uint32_t)__clzll(x) : 0u; }
// One DPP step of a wave scan or reduction: lane l's source lane's `v` (CTRL: 0x111.. row_shr:1..,
// 0x142 row_bcast:15, 0x143 row_bcast:31), 0 where the lane has no source or its row is not in ROWS.
// The compiler folds the step into the add / max that takes it (v_add_u32_dpp, v_max_u32_dpp).
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ uint32_t dpp_step(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xf, false);
}
// The wave's maximum (wave-uniform): an inclusive max-scan in VALU -- four row shifts, then lane 15
// of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 and 3 -- read from lane 63.  No trip through
// the LDS pipe (six dependent ds_bpermute, each waited for, before).
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = max(v, dpp_step<0x111>(v));
  v = max(v, dpp_step<0x112>(v));
  v = max(v, dpp_step<0x114>(v));
  v = max(v, dpp_step<0x118>(v));
  v = max(v, dpp_step<0x142, 0xa>(v));
  v = max(v, dpp_step<0x143, 0xc>(v));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, kWave - 1);
}

// The next Send's 8-B field widths from this Send's per-tile bit lengths (the last
// block, after every tile's maxima are out): each field as wide as its largest
// value, the slack of the 52 bits split between the arguments.  Fields that no
// longer fit set bit 31 (the host then keeps 16-B records).
__device__ __forceinline__ void rec8_next_from(const uint32_t* r8max, uint32_t* r8w, uint32_t* host, uint32_t tiles);
__device__ __forceinline__ void rec8_next(const SortIn& in, uint32_t* r8w, uint32_t* host, uint32_t tiles) {
  rec8_next_from(in.r8max, r8w, host, tiles);
}
__device__ __forceinline__ void rec8_next_from(const uint32_t* r8max, uint32_t* r8w, uint32_t* host, uint32_t tiles) {
  __shared__ uint32_t mx[3];
  if (threadIdx.x < 3) mx[threadIdx.x] = 0;
  __syncthreads();
  uint32_t bm = 0, b0 = 0, b1 = 0;
  for (uint32_t t = threadIdx.x; t < tiles; t += blockDim.x) {
    const uint32_t x = __hip_atomic_fetch_add(const_cast<uint32_t*>(r8max) + t, 0u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
    bm = max(bm, x & 0xffu), b0 = max(b0, (x >> 8) & 0xffu), b1 = max(b1, (x >> 16) & 0xffu);
  }
  bm = wave_max_u32(bm), b0 = wave_max_u32(b0), b1 = wave_max_u32(b1);
  if (lane_id() == 0) {
    atomicMax(&mx[0], bm);
    atomicMax(&mx[1], b0);
    atomicMax(&mx[2], b1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t wm = max(mx[0], 1u), n0 = max(mx[1], 1u), n1 = max(mx[2], 1u);
    uint32_t w = 0;
    if (wm <= 24 && wm + n0 + n1 <= 52) {
      const uint32_t w0 = n0 + (52 - wm - n0 - n1) / 2;
      w = wm | (w0 << 8) | ((52 - wm - w0) << 16);
    } else {
      const uint32_t wmc = min(wm, 24u), w0 = (52 - wmc) / 2;
      w = wmc | (w0 << 8) | ((52 - wmc - w0) << 16) | 0x80000000u;
    }
    *r8w = w;
    if (host) __hip_atomic_store(host, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Route mode 4 (world-1 stateless Sends on a directory of up to kPresMax ids): the
// directory's rank bytes folded into 2 bits per id for this rank -- 1 here, 2 probe the
// hash table (a rank past 253), 0 anything else -- so a sort block stages the whole map
// in LDS (32 KB for 131072 ids) and resolves each message with an LDS read instead of a
// scattered global gather: 64 lanes gathering from 64 lines kept the sort's address unit
// stalled by the texture cache half its busy time (profiles/r6_pmc_head.txt).
__device__ __forceinline__ void stage_pres(const SortIn& in, uint32_t* lpres) {
  const uint32_t nw = pres_words(in.n_dir);
  for (uint32_t w = threadIdx.x * 4; w < nw; w += blockDim.x * 4)
    *reinterpret_cast<uint4*>(lpres + w) = *reinterpret_cast<const uint4*>(in.pres + w);
}
template <int SK>
__device__ __forceinline__ void resolve_pres(const SortIn& in, const uint32_t* lpres, const uint32_t (&a)[SK],
                                             int (&r)[SK], uint32_t (&mb)[SK]) {
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    mb[k] = a[k];
    if (a[k] < in.n_dir) {
      const uint32_t st = (lpres[a[k] >> 4] >> ((a[k] & 15) * 2)) & 3u;
      r[k] = st == 1 ? in.rank_self : -1;
      if (st == 2) lookup_entry(in.table, in.mask, actor_key(a[k]), r[k], mb[k]);
    } else if (a[k] != 0xffffffffu) {
      lookup_entry(in.table, in.mask, actor_key(a[k]), r[k], mb[k]);
    } else {
      r[k] = -1;
    }
  }
}

// The persistent sort's form of resolve_pres, in place: the tile's actor ids `am` become its
// mailboxes, kNoSlot for a message of another rank, without an actor (past the batch too:
// load_actors gives those 0xffffffff) or with a mailbox past kMaxMbox -- what os_rank would make of
// resolve_pres' (rank, mailbox), so no rank array crosses to the ranking.  The tile's presence
// words are read back to back and classified behind one wait in straight-line code: no branch and
// no LDS latency per item.  An id past the directory reads as state 2 (probe).  The hash-table
// probes -- state 2 on any id but 0xffffffff -- sit behind one wave-uniform test that a wave of
// directory ids never passes; there a lane finds its items again and probes them one at a time
// through ONE inlined lookup_entry (picked and put back by compares), so the fast path carries no
// copies of the arrays and the kernel one probe loop instead of sixteen.
__device__ __forceinline__ uint32_t pres_state(uint32_t n_dir, uint32_t id, uint32_t word) {
  // (v_bfe_u32 takes the low five bits of its offset: id's place in its word needs no mask)
  return __builtin_amdgcn_ubfe(id < n_dir ? word : 0xaaaaaaaau, id << 1, 2u);
}
template <int SK>
__device__ __forceinline__ void resolve_pres_lean(const SortIn& in, const uint32_t* lpres, uint32_t (&am)[SK]) {
  uint32_t pw[SK];
#pragma unroll
  for (int k = 0; k < SK; ++k) pw[k] = lpres[(am[k] < in.n_dir ? am[k] : 0u) >> 4];  // (word 0: inside the staged map)
  bool probes = false;
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const uint32_t st = pres_state(in.n_dir, am[k], pw[k]);
    probes |= st == 2 && am[k] != 0xffffffffu;
    am[k] = st == 0 ? kNoSlot : am[k];  // (state 1: a directory id is its own mailbox, below kPresMax)
  }
  if (__any(probes)) {
    uint32_t todo = 0;  // this lane's items that need the hash table
#pragma unroll
    for (int k = 0; k < SK; ++k) {
      const uint32_t st = pres_state(in.n_dir, am[k], lpres[(am[k] < in.n_dir ? am[k] : 0u) >> 4]);
      todo |= st == 2 && am[k] != 0xffffffffu ? 1u << k : 0u;
    }
    while (todo != 0) {
      const int k = __builtin_ctz(todo);
      todo &= todo - 1;
      uint32_t id = am[0];
#pragma unroll
      for (int j = 1; j < SK; ++j) id = j == k ? am[j] : id;
      int rr;
      uint32_t mm;
      lookup_entry(in.table, in.mask, actor_key(id), rr, mm);
      mm = rr == in.rank_self && mm < kMaxMbox ? mm : kNoSlot;
#pragma unroll
      for (int j = 0; j < SK; ++j) am[j] = j == k ? mm : am[j];
    }
  }
}

// ---- the phases of a one-pass tile, shared by onesweep_tile (one tile per block) and the
// persistent reserving sort (mbx_persist_sort_kernel: a block walks several tiles)
//
// Phase 1: the tile's actors resolved to (rank, mailbox).
template <int MODE, int SK>
__device__ __forceinline__ void os_resolve(const SortIn& in, const uint32_t* lpres, const uint32_t (&a)[SK], int (&r)[SK],
                                           uint32_t (&mb)[SK]) {
  if constexpr (MODE == 4) resolve_pres<SK>(in, lpres, a, r, mb);
  else resolve_k<MODE, SK>(in, a, r, mb);
}

// Phase 2: each message's rank among its wave's earlier messages of its shard (message
// order: item, then lane), counted into this wave's row `wrow` of the wave counts.  A
// message past the batch, of another rank or without an actor leaves with mb = kNoSlot.
template <int SK>
__device__ __forceinline__ void os_rank(const SortIn& in, uint32_t log_s, uint32_t t, const int (&r)[SK],
                                        uint32_t (&mb)[SK], uint32_t* wrow, uint32_t (&wr)[SK]) {
  const uint32_t S = 1u << log_s;
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const bool ok = tile_index<SK>(t, k) < in.M && r[k] == in.rank_self && mb[k] < kMaxMbox;
    if (!ok) mb[k] = kNoSlot;
    const uint32_t sh = mb[k] & (S - 1);
    const uint64_t peers = match_bits(sh, log_s, __ballot(ok));
    const unsigned below = mbcnt64(peers);
    const int leader = peers ? __builtin_ctzll(peers) : 0;
    unsigned old = 0;
    if (ok && below == 0) {
      old = wrow[sh];
      wrow[sh] = old + (unsigned)__popcll(peers);
    }
    wr[k] = (unsigned)__shfl((int)old, leader) + below;
  }
}

// Phase 2 for a view of at most kStatelessShards (8) shards, with os_rank's results: the ranks
// by a scan instead of a match per shard bit and a leader lane's read-modify-write of the LDS row.
// Per item a lane sets a one-hot BYTE counter -- byte sh of a 64-bit word, its low dword for
// shards 0..3 and its high dword for shards 4..7 -- and both dwords are inclusive-scanned across
// the wave by DPP adds (a field reaches 64 at most: no carry leaves a byte).  A lane's own byte,
// less one, is its rank among the item's earlier lanes of its shard; lane 63 holds the item's
// totals.  The wave's running count of shard s stays in lane s of one register (`run`): a lane's
// base is that register read at lane sh before the item's totals are added, and the row of counts
// goes to LDS once per tile, from lanes < S (`wrow` needs no clearing).
// `mb` comes from resolve_pres_lean: kNoSlot marks a message that takes no slot (no bounds test
// here: a message past the batch is among them).
template <int SK>
__device__ __forceinline__ void os_rank_scan(uint32_t S, const uint32_t (&mb)[SK], uint32_t* wrow, uint32_t (&wr)[SK]) {
  static_assert(kStatelessShards == 8, "one byte per shard in two dwords");
  const uint32_t lane = lane_id();
  const uint32_t lsh = (lane & 7u) * 8u;  // (lanes 0..7) the lane's shard's byte in the totals
  uint32_t run = 0;
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const uint32_t sh = mb[k] & (S - 1);
    const uint64_t hot = (uint64_t)(mb[k] != kNoSlot ? 1u : 0u) << (sh * 8u);
    uint32_t lo = (uint32_t)hot, hi = (uint32_t)(hot >> 32);
    lo += dpp_step<0x111>(lo), hi += dpp_step<0x111>(hi);
    lo += dpp_step<0x112>(lo), hi += dpp_step<0x112>(hi);
    lo += dpp_step<0x114>(lo), hi += dpp_step<0x114>(hi);
    lo += dpp_step<0x118>(lo), hi += dpp_step<0x118>(hi);
    lo += dpp_step<0x142, 0xa>(lo), hi += dpp_step<0x142, 0xa>(hi);
    lo += dpp_step<0x143, 0xc>(lo), hi += dpp_step<0x143, 0xc>(hi);
    // (inclusive: a message counts itself; one without a slot leaves with a rank nobody reads)
    const uint32_t below = (((sh & 4u) ? hi : lo) >> ((sh & 3u) * 8u)) & 0xffu;
    const uint32_t base = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(sh << 2), (int)run);
    wr[k] = base + below - 1u;
    const uint64_t tot = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, kWave - 1) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)lo, kWave - 1);
    run += (uint32_t)(tot >> lsh) & 0xffu;
  }
  if (lane < S) wrow[lane] = run;
}

// Phase 3, per shard (one thread each): the wave counts turned into wave offsets (returns
// the tile's count), the run's reservation, the ring's room, and the run's tinfo words.
__device__ __forceinline__ uint32_t os_wave_offsets(uint32_t* wcnt_all, uint32_t S, uint32_t s) {
  uint32_t c = 0;
#pragma unroll
  for (int ww = 0; ww < kST / kWave; ++ww) {
    const uint32_t x = wcnt_all[ww * S + s];
    wcnt_all[ww * S + s] = c;
    c += x;
  }
  return c;
}
__device__ __forceinline__ uint32_t os_reserve(const MboxView& mv, uint32_t s, uint32_t c) {
  return c ? atomicAdd(&mv.resv[s * kResvStride], c) : 0u;
}
__device__ __forceinline__ uint32_t os_ring_room(const MboxView& mv, uint32_t s, uint64_t& tl) {
  const uint64_t Q = 1ull << mv.log_q;
  tl = *ctr_tail(mv, s);
  const uint64_t hd = *ctr_head(mv, s);
  const uint64_t free = hd + Q > tl ? hd + Q - tl : 0;
  return (uint32_t)(free < 0xffffffffull ? free : 0xffffffffull);
}
// (returns whether the run overran the ring's room)
__device__ __forceinline__ int os_run_info(const MboxView& mv, uint32_t* __restrict__ tinfo, uint32_t t, uint32_t S,
                                           uint32_t s, uint64_t tl, uint32_t rm, uint64_t excl, uint32_t c) {
  if (tinfo) {
    const uint32_t cc = excl >= rm ? 0u : (uint32_t)min((uint64_t)c, rm - excl);
    tinfo[(size_t)t * 2 * S + s] = (uint32_t)(tl + excl) + shard_rot(mv, s);
    tinfo[(size_t)t * 2 * S + S + s] = cc | (excl + c > rm ? kRunSpilled : 0u);
  }
  return excl + c > rm;
}

// (in.rec8 / in.recw) the tile's fields OR-ed, their bit lengths max-ed into `tmax` (LDS,
// read past the next barrier); returns the mask of this thread's messages whose fields do
// not fit an 8-B record of widths `w8`.
template <int SK, bool OR_FIRST = false>
__device__ __forceinline__ uint32_t os_fields(const SortIn& in, uint32_t w8, const uint32_t (&mb)[SK],
                                              const int64_t (&v0)[SK], const int64_t (&v1)[SK], uint32_t* tmax) {
  uint32_t escm = 0;
  if (!(in.rec8 || in.recw)) return escm;
  uint64_t or_m = 0, or_0 = 0, or_1 = 0;
  const uint32_t wm = w8 & 0xffu, w0 = (w8 >> 8) & 0xffu, w1 = (w8 >> 16) & 0xffu;
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    if (mb[k] == kNoSlot) continue;
    const uint64_t z0 = ((uint64_t)v0[k] << 1) ^ (uint64_t)(v0[k] >> 63);
    const uint64_t z1 = ((uint64_t)v1[k] << 1) ^ (uint64_t)(v1[k] >> 63);
    or_m |= mb[k], or_0 |= z0, or_1 |= z1;
    if constexpr (!OR_FIRST)
      if (in.rec8 && ((mb[k] >> wm) != 0 || (z0 >> w0) != 0 || (z1 >> w1) != 0)) escm |= 1u << k;
  }
  // OR_FIRST (the persistent sort): the thread's OR-ed fields tested first, and only a thread whose
  // OR does not fit looks for the items (the per-item tests cost the one-block-per-tile kernels a VGPR less)
  if (OR_FIRST && in.rec8 && ((or_m >> wm) | (or_0 >> w0) | (or_1 >> w1)) != 0) {
#pragma unroll
    for (int k = 0; k < SK; ++k) {
      if (mb[k] == kNoSlot) continue;
      const uint64_t z0 = ((uint64_t)v0[k] << 1) ^ (uint64_t)(v0[k] >> 63);
      const uint64_t z1 = ((uint64_t)v1[k] << 1) ^ (uint64_t)(v1[k] >> 63);
      if ((mb[k] >> wm) != 0 || (z0 >> w0) != 0 || (z1 >> w1) != 0) escm |= 1u << k;
    }
  }
  const uint32_t bm = wave_max_u32(bitlen64(or_m)), b0 = wave_max_u32(bitlen64(or_0)),
                 b1 = wave_max_u32(bitlen64(or_1));
  if (lane_id() == 0) {
    atomicMax(&tmax[0], bm);
    atomicMax(&tmax[1], b0);
    atomicMax(&tmax[2], b1);
  }
  return escm;
}

// The one wait for a tile's loads (the persistent sort): its arguments and the coming tile's
// actors used here, on every path, so the compiler waits for them here and not at their
// first uses inside the store loop -- where, the loads sitting in branches, it could only
// write vmcnt(0), behind the previous item's record store.
template <int SK>
__device__ __forceinline__ void os_loads_in(const int64_t (&v0)[SK], const int64_t (&v1)[SK], const uint32_t (&nx)[SK]) {
#pragma unroll
  for (int k = 0; k < SK; ++k) asm volatile("" ::"v"(v0[k]), "v"(v1[k]), "v"(nx[k]));
}

// A tile's ranks (below kST), two to a word: what the persistent sort carries to the store phase.
template <int SK>
struct PackedRanks {
  uint32_t p[SK / 2];
  // (the low halves of a pair, by one byte permute: a message without a slot may carry any rank)
  __device__ __forceinline__ void pack(const uint32_t (&wr)[SK]) {
#pragma unroll
    for (int k = 0; k < SK / 2; ++k) p[k] = __builtin_amdgcn_perm(wr[2 * k + 1], wr[2 * k], 0x05040100u);
  }
  __device__ __forceinline__ uint32_t operator[](int k) const { return (p[k >> 1] >> ((k & 1) * 16)) & 0xffffu; }
};

// ---- the lean bodies of the 8-B stateless Send (profiles/lean_bodies.md): what the persistent
// sort's store loop and the narrow ring drain run per record when nothing of the general case
// can occur, chosen by block-uniform tests.
//
// Rings whose every 8-B cell lies within 4 GB of plane A's start: a slot's byte offset fits
// 32 bits, so a record's address is a scalar base plus a 32-bit offset.
__device__ __forceinline__ bool rings_small(const MboxView& mv) { return mv.log_s + mv.log_q <= 29; }

// 8-B field widths that pack and decode in 32-bit operations: the place and the mailbox lie in
// the low word (12 + wm < 32), a0's field straddles or ends at the words' boundary, a1's lies
// in the high word, and both arguments' zigzags fit 32 bits.
struct Rec8Fast {
  uint32_t s0;   // a0's field starts here (13..31)
  uint32_t s1h;  // a1's field starts here in the high word (0..31)
  uint32_t m0;   // a0's field mask
  uint32_t mm;   // the mailbox's field mask
  bool ok;
};
__device__ __forceinline__ Rec8Fast rec8_fast(uint32_t w8) {
  const uint32_t wm = w8 & 0xffu, w0 = (w8 >> 8) & 0xffu, w1 = (w8 >> 16) & 0xffu;
  Rec8Fast f;
  f.s0 = 12 + wm;
  f.ok = f.s0 < 32 && w0 >= 1 && w0 <= 32 && w1 <= 32 && f.s0 + w0 >= 32 && f.s0 + w0 < 64;
  f.s1h = (f.s0 + w0) & 31u;
  f.m0 = w0 >= 32 ? 0xffffffffu : (1u << (w0 & 31u)) - 1u;
  f.mm = (1u << (wm & 31u)) - 1u;
  return f;
}
// (x fits its field: it is an int32, and its zigzag a u32)
__device__ __forceinline__ uint32_t zigzag32(int64_t x) {
  const uint32_t lo = (uint32_t)x;
  return (lo << 1) ^ (uint32_t)((int32_t)lo >> 31);
}
__device__ __forceinline__ uint64_t pack_rec8_fast(const Rec8Fast& f, uint32_t place, uint32_t mb, int64_t x0, int64_t x1) {
  const uint32_t z0 = zigzag32(x0), z1 = zigzag32(x1);
  const uint32_t lo = place | (mb << 12) | (z0 << f.s0);
  const uint32_t hi = (z0 >> (32u - f.s0)) | (z1 << f.s1h);
  return ((uint64_t)hi << 32) | lo;
}

// The lean store of one message of a tile that did not spill (no run past its room, no field
// past its width): `wpos` is this wave's row of ring positions -- the low word of tail +
// rotation + the tile's prefix + the wave's offset, per shard (built behind the tile's
// barrier) -- so a record's slot is one LDS read, an add, a mask and a shift-or in 32 bits.
// rv.slots is null (the caller's test): a miss's status is a plain store.
template <int SK, bool FAST>
__device__ __forceinline__ void os_store_lean(const SortIn& in, const MboxView& mv, const ReplyView& rv, int64_t i,
                                              uint32_t place, const uint32_t* wpos, uint32_t mbk, uint32_t wrk,
                                              int64_t x0, int64_t x1, const Rec8Fast& f, uint32_t w8, uint32_t& n_miss) {
  if (mbk == kNoSlot) {
    ++n_miss;
    const uint32_t origin = in.origin_base + (uint32_t)i;
    if ((uint64_t)origin < rv.n) {
      rv.val[origin] = 0;
      rv.st[origin] = kStatusNoActor;
    }
    return;
  }
  const uint32_t sh = mbk & ((1u << mv.log_s) - 1u);
  const uint32_t slot = (sh << mv.log_q) | ((wpos[sh] + wrk) & ((1u << mv.log_q) - 1u));
  uint64_t rec;
  if constexpr (FAST) {
    rec = pack_rec8_fast(f, place, mbk, x0, x1);
  } else {
    const uint32_t wm = w8 & 0xffu, w0 = (w8 >> 8) & 0xffu;
    const uint64_t z0 = ((uint64_t)x0 << 1) ^ (uint64_t)(x0 >> 63);
    const uint64_t z1 = ((uint64_t)x1 << 1) ^ (uint64_t)(x1 >> 63);
    rec = (uint64_t)place | ((uint64_t)mbk << 12) | (z0 << (12 + wm)) | (z1 << (12 + wm + w0));
  }
  *reinterpret_cast<uint64_t*>(reinterpret_cast<unsigned char*>(mv.rec) + (slot << 3)) = rec;
}

// Phase 4, per message i of the tile (the caller's unrolled loop over its items: the loop
// inside a shared function cost every sort kernel 5 to 15 VGPRs): the record into its ring
// at the run's prefix + the wave's offset + the message's rank; a message past the ring's
// room (or, stateless, one whose fields do not fit 8 B) spills or overflows.  `wrow` is this
// wave's row of the wave offsets.
template <int SK, typename CT>
__device__ __forceinline__ void os_store_msg(const SortIn& in, const MboxView& mv, const ReplyView& rv, int64_t i,
                                             const unsigned long long* base, const uint32_t* room, const uint32_t* pre,
                                             const uint32_t* wrow, uint32_t mbk, uint32_t wrk, int64_t x0, int64_t x1,
                                             int64_t x2, uint32_t mt, bool esc, uint32_t w8, bool spill, bool wsidx,
                                             uint32_t* __restrict__ sidx, uint32_t* __restrict__ rw, CT& n_enq, CT& n_ovf,
                                             CT& n_miss, CT& n_spill) {
  const uint32_t S = 1u << mv.log_s;
  const uint32_t origin = in.origin_base + (uint32_t)i;
  if (mbk == kNoSlot) {
    ++n_miss;
    if (wsidx) sidx[i] = kNoSlot;
    write_status(rv, origin, kStatusNoActor);
    return;
  }
  const uint32_t sh = mbk & (S - 1);
  const uint32_t off = pre[sh] + wrow[sh] + wrk;
  if (off >= room[sh] || (esc && spill)) {  // the ring is full (or a stateless record, esc: wider than 8 B, spills)
    if (spill) {  // the drain runs it from the batch: its route word is all it needs from here
      ++n_spill;
      sidx[i] = kSpillSlot;
      rw[i] = mbk;
      return;
    }
    ++n_ovf;
    if (wsidx) sidx[i] = kNoSlot;
    write_status(rv, origin, kStatusOverflow);
    return;
  }
  const uint64_t slot = slot_at(mv, sh, base[sh] + off);
  if (wsidx) sidx[i] = (uint32_t)slot;
  if (in.recw) {  // wide pure record: {a0, a1} whole, the place in the tile beside it
    *reinterpret_cast<u32x4*>(rec_a(mv, slot)) =
        u32x4{(uint32_t)x0, (uint32_t)((uint64_t)x0 >> 32), (uint32_t)x1, (uint32_t)((uint64_t)x1 >> 32)};
    rec_place(mv)[slot] = (uint16_t)(i & ((kST * SK) - 1));
  } else if (in.rec8 && esc) {  // (ordered) escape: the place in the tile + bit 63, the fields aside
    reinterpret_cast<uint64_t*>(mv.rec)[slot] = (uint64_t)(i & ((kST * SK) - 1)) | (1ull << 63);
    *reinterpret_cast<u32x4*>(in.r8esc + 2 * slot) =
        u32x4{(uint32_t)x0, (uint32_t)((uint64_t)x0 >> 32), mbk, 0u};
  } else if (in.rec8) {  // 8-B record (uniform method; stateless records that do not fit spilled above)
    const uint32_t wm = w8 & 0xffu, w0 = (w8 >> 8) & 0xffu;
    const uint64_t z0 = ((uint64_t)x0 << 1) ^ (uint64_t)(x0 >> 63);
    const uint64_t z1 = ((uint64_t)x1 << 1) ^ (uint64_t)(x1 >> 63);
    reinterpret_cast<uint64_t*>(mv.rec)[slot] =
        (uint64_t)(i & ((kST * SK) - 1)) | ((uint64_t)mbk << 12) | (z0 << (12 + wm)) | (z1 << (12 + wm + w0));
  } else if (mt < 128u && fits_i32(x0) && fits_i32(x1) && x2 == 0) {
    *reinterpret_cast<u32x4*>(rec_a(mv, slot)) =
        u32x4{origin | kCompactMark, mbk | (mt << 24), (uint32_t)x0, (uint32_t)x1};
  } else {
    const uint32_t fl = x2 != 0 ? (uint32_t)kFlagA2 : 0u;
    *reinterpret_cast<u32x4*>(rec_a(mv, slot)) =
        u32x4{origin | kCompactMark, mbk | kCompactLong, (mt & 0xffffu) | (fl << 16), 0u};
    *reinterpret_cast<u32x4*>(rec_b(mv, slot)) =
        u32x4{(uint32_t)x0, (uint32_t)((uint64_t)x0 >> 32), (uint32_t)x1, (uint32_t)((uint64_t)x1 >> 32)};
    if (fl) mv.a2[slot] = x2;
  }
  ++n_enq;
}

// One tile of the one-pass sort (the block claims it); returns its index.
//
// reserve (stateless batches): no look-back.  A stateless record runs on its
// own, so a ring need not hold its messages in message order -- only each
// tile's run in message order (the drains read a tile's runs through tinfo).
// The tile is the block's index and each shard's run is reserved with ONE
// atomicAdd on the shard's epoch counter (gsum row 0, which then holds the
// epoch's total): 16 device-scope atomics per tile, ~2048 per counter at 8 Mi
// messages -- against a look-back whose walk grows with the tiles in flight
// (each hop a memory-side round trip).
template <int MODE, bool A2, bool MC, int SK = kSK>
__device__ __forceinline__ uint32_t onesweep_tile(const SortIn& in, const MboxView& mv, unsigned long long* __restrict__ desc,
                                                  unsigned* __restrict__ tctr, uint32_t* __restrict__ gsum,
                                                  uint32_t* __restrict__ sidx, uint32_t* __restrict__ tinfo,
                                                  uint32_t* __restrict__ rw, const ReplyView& rv, bool spill,
                                                  bool all_sidx, unsigned char* smem_os, bool reserve = false) {
  const uint32_t S = 1u << mv.log_s;
  unsigned long long* base = reinterpret_cast<unsigned long long*>(smem_os);  // ring position of this tile's run (tail + prefix)
  uint32_t* room = reinterpret_cast<uint32_t*>(base + S);                     // offset limit past the tail
  uint32_t* pre = room + S;                                                   // the tile's prefix per shard
  uint32_t* wcnt_all = pre + S;                                               // [kST / kWave][S]
  auto wcnt = [&](unsigned ww, uint32_t sh) -> uint32_t& { return wcnt_all[ww * S + sh]; };
  __shared__ uint32_t tile_s;
  __shared__ uint32_t tmax[3];  // (in.rec8) the tile's field bit lengths
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  if (threadIdx.x < 3) tmax[threadIdx.x] = 0;  // (ordered before use by the tile's first barrier)
  // this Send's epoch tag, 1..0xffffff (the drain advances tctr[1]; the modulus keeps the tag inside the
  // descriptor's 24-bit field across the counter's wrap -- tag 0 is reserved for never-published words)
  const uint32_t tag = epoch_tag(tctr[1]);
  if (threadIdx.x == 0 && !reserve) {
    const uint32_t t = atomicAdd(&tctr[0], 1u);
    if (t == in.tiles - 1) atomicExch(&tctr[0], 0u);  // every block has claimed: ready for the next Send
    tile_s = t;
  }
  for (uint32_t s = lane; s < S; s += kWave) wcnt(w, s) = 0;
  uint32_t* lpres = reinterpret_cast<uint32_t*>(smem_os + ((onesweep_lds_bytes(S) + 15) & ~(size_t)15));
  if constexpr (MODE == 4) stage_pres(in, lpres);  // (the map, behind the barrier below)
  __syncthreads();
  // (reserve: tiles dealt XCD by XCD, as the ring drain deals them -- its reads of a tile's runs then
  // meet the lines in the L2 that took the sort's stores)
  const uint32_t t = reserve ? virt_block(blockIdx.x, gridDim.x) : tile_s;
  // the tile's columns: actors, then the arguments in flight across the gathers and the ranking
  uint32_t a[SK], mb[SK], meth[SK];
  int64_t v0[SK], v1[SK], v2[SK];
  int r[SK];
  load_actors<SK>(in, t, a);
  load_cols<A2, MC, SK>(in, t, v0, v1, v2, meth);
  os_resolve<MODE, SK>(in, lpres, a, r, mb);
  uint32_t wr[SK];
  // (an ordered batch in 8-B records, !spill: a message whose fields do not fit takes its
  // ring position like any other and is written as an escape record below -- FIFO kept)
  os_rank<SK>(in, mv.log_s, t, r, mb, wcnt_all + w * S, wr);
  __syncthreads();
  // per shard: wave offsets within the tile, publish the tile's count, look back for its prefix
  unsigned long long timeouts = 0;
  int sp = 0;
  for (uint32_t s = threadIdx.x; s < S; s += kST) {
    uint64_t excl = 0;
    unsigned long long* d = desc + (size_t)t * S + s;
    const uint32_t c = os_wave_offsets(wcnt_all, S, s);
    if (reserve) {
      excl = os_reserve(mv, s, c);  // this tile's run of shard s
    } else if (t == 0) {
      __hip_atomic_exchange(d, desc_word(tag, kDescP, c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      __hip_atomic_exchange(d, desc_word(tag, kDescA, c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      excl = lookback(desc + s, S, (int64_t)t - 1, tag, timeouts);
      __hip_atomic_exchange(d, desc_word(tag, kDescP, excl + c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!reserve && t == in.tiles - 1) gsum[s] = (uint32_t)(excl + c);  // the epoch's total of shard s
    uint64_t tl;
    const uint32_t rm = os_ring_room(mv, s, tl);
    base[s] = tl;
    room[s] = rm;
    pre[s] = (uint32_t)excl;
    sp |= os_run_info(mv, tinfo, t, S, s, tl, rm, excl, c);
  }
  // (in.rec8) the messages whose fields do not fit an 8-B record -- they spill -- and
  // the tile's fields OR-ed (their bit lengths size the next Send's records)
  const uint32_t w8 = in.rec8 ? *in.r8w : 0u;  // this Send's 8-B field widths (recw: none, nothing escapes)
  const bool maxima = in.rec8 || in.recw;  // (wide pure records keep the maxima: back to 8 B once they fit)
  const uint32_t escm = os_fields<SK>(in, w8, mb, v0, v1, tmax);
  sp |= escm != 0;
  bool tile_spill = false;
  if (spill) tile_spill = __syncthreads_or(sp) != 0;
  else __syncthreads();
  // a tile spilled by its records' widths (no run overran its ring): flag one of its
  // runs, so the drains take the tile in message order through the slot indices
  // (the thread that wrote shard 0's count word: program order)
  if (tile_spill && tinfo && threadIdx.x == 0) tinfo[(size_t)t * 2 * S + S] |= kRunSpilled;
  const bool wsidx = all_sidx || tile_spill;
  unsigned long long n_enq = 0, n_ovf = 0, n_miss = 0, n_spill = 0;
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const int64_t i = tile_index<SK>(t, k);
    if (i >= in.M) continue;
    os_store_msg<SK>(in, mv, rv, i, base, room, pre, wcnt_all + w * S, mb[k], wr[k], v0[k], v1[k], v2[k], meth[k],
                     (escm >> k) & 1u, w8, spill, wsidx, sidx, rw, n_enq, n_ovf, n_miss, n_spill);
  }
  // the tile's field bit lengths, for the next Send's widths (rec8_next): a memory-side write
  // (the fused kernel's last block reads it within the launch: its ticket follows a vmcnt(0) wait)
  if (maxima && threadIdx.x == 0) (void)atomicExch(&in.r8max[t], tmax[0] | (tmax[1] << 8) | (tmax[2] << 16));
  block_add_stats(mv.stats, n_enq, kMbEnqueued, n_ovf, kMbOverflow, n_miss, kMbNoActor);
  __syncthreads();  // block_add_stats' LDS partials are reused
  block_add_stats(mv.stats, n_spill, kMbSpilled, timeouts, kMbLookback, 0, -1);
  return t;
}

// ---------------------------------------------------------------- compact record decode
struct SortRec {
  uint32_t origin, mb, method, flags;
  int64_t a0, a1, a2;
  bool valid;
};

__device__ __forceinline__ bool rec_is_long(const u32x4& ha) { return (ha.y & kCompactLong) != 0; }

__device__ __forceinline__ SortRec decode_sorted(const u32x4& ha, const u32x4& hb, int64_t a2v) {
  SortRec x;
  x.valid = (ha.x & kCompactMark) != 0;
  x.origin = ha.x & ~kCompactMark;
  if (!rec_is_long(ha)) {
    x.mb = ha.y & 0xffffffu;
    x.method = (ha.y >> 24) & 0x7fu;
    x.flags = 0;
    x.a0 = (int64_t)(int32_t)ha.z;
    x.a1 = (int64_t)(int32_t)ha.w;
    x.a2 = 0;
  } else {
    x.mb = ha.y & 0xffffffu;
    x.method = ha.z & 0xffffu;
    x.flags = ha.z >> 16;
    x.a0 = (int64_t)(((uint64_t)hb.y << 32) | hb.x);
    x.a1 = (int64_t)(((uint64_t)hb.w << 32) | hb.z);
    x.a2 = (x.flags & kFlagA2) ? a2v : 0;
  }
  return x;
}

// An 8-B record (in.rec8) of the tile whose first message is `tile_origin`.
template <bool FRESH, int SK = kSK>
__device__ __forceinline__ SortRec decode_rec8(uint64_t r, const SortIn& in, uint32_t w8, uint32_t tile_origin) {
  const uint32_t wm = w8 & 0xffu, w0 = (w8 >> 8) & 0xffu, w1 = (w8 >> 16) & 0xffu;
  const uint64_t m0 = (1ull << w0) - 1;
  SortRec x;
  x.valid = true;
  x.origin = tile_origin + (uint32_t)(r & ((kST * SK) - 1));
  x.mb = (uint32_t)((r >> 12) & ((1ull << wm) - 1));
  x.method = in.method_uniform;
  x.flags = 0;
  x.a2 = 0;
  const uint64_t z0 = (r >> (12 + wm)) & m0, z1 = (r >> (12 + wm + w0)) & ((1ull << w1) - 1);
  x.a0 = (int64_t)(z0 >> 1) ^ -(int64_t)(z0 & 1);
  x.a1 = (int64_t)(z1 >> 1) ^ -(int64_t)(z1 & 1);
  return x;
}

// A wide pure record (in.recw): no mailbox -- its method reads none.
__device__ __forceinline__ SortRec decode_wide(const u32x4& h, const SortIn& in, uint32_t origin) {
  SortRec x;
  x.valid = true;
  x.origin = origin;
  x.mb = 0;
  x.method = in.method_uniform;
  x.flags = 0;
  x.a0 = (int64_t)(((uint64_t)h.y << 32) | h.x);
  x.a1 = (int64_t)(((uint64_t)h.w << 32) | h.z);
  x.a2 = 0;
  return x;
}

__device__ __forceinline__ SortRec load_sorted(const MboxView& mv, uint64_t slot) {
  const u32x4 ha = *reinterpret_cast<const u32x4*>(rec_a(mv, slot));
  u32x4 hb = {0u, 0u, 0u, 0u};
  int64_t a2v = 0;
  if (rec_is_long(ha)) {
    hb = *reinterpret_cast<const u32x4*>(rec_b(mv, slot));
    if (((ha.z >> 16) & kFlagA2) && mv.a2) a2v = mv.a2[slot];
  }
  return decode_sorted(ha, hb, a2v);
}

// The epoch's total of shard s (group sums) -- and the group words zeroed for
// the next Send once read (`clear`: the caller is the shard's last reader).
__device__ __forceinline__ uint32_t epoch_total(uint32_t* gsum, uint32_t ngroups, uint32_t S, uint32_t s, bool clear) {
  uint32_t t = 0;
  for (uint32_t g = 0; g < ngroups; ++g) {
    t += gsum[(size_t)g * S + s];
    if (clear) gsum[(size_t)g * S + s] = 0u;
  }
  return t;
}

// The epoch's total of shard s, cleared for the next Send: the reservation counter of
// a one-pass stateless Send (memory-side, as its tiles added to it), else the group sums.
__device__ __forceinline__ uint32_t epoch_sum(const MboxView& mv, uint32_t* gsum, uint32_t ngroups, uint32_t S,
                                              uint32_t s) {
  return mv.resv ? atomicExch(&mv.resv[s * kResvStride], 0u) : epoch_total(gsum, ngroups, S, s, true);
}

// The epoch's positions of shard s are consumed: head = tail = tail + total
// (overflowed positions were never written and are skipped with them).
__device__ __forceinline__ void epoch_commit(const MboxView& mv, uint32_t s, uint32_t tot) {
  const uint64_t t = *ctr_tail(mv, s) + tot;
  *ctr_tail(mv, s) = t;
  *ctr_done(mv, s) = t;
  *ctr_head(mv, s) = t;
}

// ---------------------------------------------------------------- K3s parallel drain
// Batches without ordered methods: every record runs on its own.
//
// Ring-order form (default): one block per tile.  The tile's records sit in S
// runs (the scatter's tinfo); the block reads them in RING order -- consecutive
// lanes take consecutive ring slots, so the loads are whole-line runs -- runs
// each handler, stages the reply in LDS at the message's place in the tile
// (origin), and writes the tile's replies out coalesced.  Replaces the
// message-order form's slot-index read (4 B per message) and its 16-B gather per
// message (one line per lane).
//
// Message-order form (tune mbox_drain_msg=1, and any tile with a spilled
// message): each message's record is taken from the ring slot the scatter
// recorded, replies coalesced; a spilled message runs straight from the batch.
//
// The last block commits every shard (and clears the group sums).
// RF: the record form -- 0 compact / long (16 / 32 B), 1 the 8-B record, 2 the wide
// pure record (16 B {a0, a1} + the u16 place)
template <int FIXED, bool FRESH = false, int RF = 0, int SK = kSK>
__device__ __forceinline__ void drain_tile_msg(MboxView mv, SortIn in, uint32_t t,
                                               const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ rw,
                                               int64_t* __restrict__ state, uint32_t n_state, uint64_t delay_ticks,
                                               OutboxView ob, ReplyView rv, unsigned long long& done,
                                               unsigned long long& failed, unsigned long long& holes) {
  uint32_t sl[SK];
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const int64_t i = tile_index<SK>(t, k);
    sl[k] = i < in.M ? __builtin_nontemporal_load(sidx + i) : kNoSlot;
  }
  using RecT = typename std::conditional<RF == 1, uint64_t, u32x4>::type;  // the ring record as loaded
  const uint32_t w8 = RF == 1 ? *in.r8w : 0u;  // the 8-B field widths this Send's sort used
  RecT ha[SK];
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    if constexpr (RF == 1) {
      const uint64_t* rp = reinterpret_cast<const uint64_t*>(mv.rec) + (sl[k] < kSpillSlot ? sl[k] : 0);
      ha[k] = sl[k] < kSpillSlot ? (FRESH ? __builtin_nontemporal_load(rp) : *rp) : 0ull;
    } else {
      const u32x4* rp = reinterpret_cast<const u32x4*>(rec_a(mv, sl[k] < kSpillSlot ? sl[k] : 0));
      ha[k] = sl[k] < kSpillSlot ? (FRESH ? __builtin_nontemporal_load(rp) : *rp) : u32x4{0u, 0u, 0u, 0u};
    }
  }
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    if (sl[k] == kNoSlot) continue;  // answered by the scatter (no actor / ring full)
    SortRec x;
    if (sl[k] == kSpillSlot) {  // its ring was full: the message runs straight from the batch
      const int64_t i = tile_index<SK>(t, k);
      x.valid = true;
      x.mb = rw[i];
      x.method = in.mcol ? (uint32_t)in.mcol[i] : in.method_uniform;
      x.flags = 0;
      x.a0 = in.a0[i];
      x.a1 = in.a1 ? in.a1[i] : 0;
      x.a2 = in.a2 ? in.a2[i] : 0;
    } else if constexpr (RF == 1) {
      x = decode_rec8<FRESH, SK>(ha[k], in, w8, in.origin_base + t * (kST * SK));
    } else if constexpr (RF == 2) {
      x = decode_wide(ha[k], in, 0u);
    } else {
      u32x4 hb = {0u, 0u, 0u, 0u};
      int64_t a2v = 0;
      if (rec_is_long(ha[k])) {
        const u32x4* bp = reinterpret_cast<const u32x4*>(rec_b(mv, sl[k]));
        hb = FRESH ? __builtin_nontemporal_load(bp) : *bp;
        if (((ha[k].z >> 16) & kFlagA2) && mv.a2) a2v = FRESH ? __builtin_nontemporal_load(mv.a2 + sl[k]) : mv.a2[sl[k]];
      }
      x = decode_sorted(ha[k], hb, a2v);
    }
    const uint32_t origin = in.origin_base + (uint32_t)tile_index<SK>(t, k);
    if (!x.valid) {
      ++holes;
      write_status(rv, origin, kStatusNotDelivered);
      continue;
    }
    MsgRecord m;
    m.actor = x.mb;
    m.method = (uint16_t)(FIXED ? FIXED : x.method);
    m.flags = (uint16_t)x.flags;
    m.a0 = x.a0, m.a1 = x.a1, m.a2 = x.a2;
    const ReplyRecord rr = run_handler(m, state, n_state, delay_ticks, ob);
    failed += rr.status != kStatusOk;
    write_reply(rv, origin, rr);
    ++done;
  }
}

// Tile t's runs in LDS: per shard the slot bias (ring slot of run entry j =
// shard base | ((bias + j) & (Q - 1))) and an owner table (run entry j of the
// tile -> its shard), j in [0, total).  Entries past a shard's free room (an
// ordered batch's overflow: never written) are left out (the scatter clamped the
// counts).  Returns the total; `spill` is set when a run overflowed the room (a
// stateless tile's spill).
template <typename OwnT>
struct RunLds {
  uint32_t* bias;  // [S]
  uint32_t* excl;  // [S] exclusive prefix of the (clamped) counts
  OwnT* owner;     // [kSTile]: u8 for up to 256 shards, else u16
};

template <typename OwnT>
__device__ __forceinline__ uint32_t load_tile_runs(const MboxView& mv, const uint32_t* __restrict__ tinfo, uint32_t t,
                                                   const RunLds<OwnT>& L, int& spill) {
  __shared__ uint32_t wsum[kST / kWave];
  __shared__ uint32_t total_s;
  const uint32_t S = 1u << mv.log_s;
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  // thread j owns the shards [j * per, (j + 1) * per): a contiguous scan
  const uint32_t per = (S + kST - 1) / kST, s0 = threadIdx.x * per, s1 = min(S, s0 + per);
  uint32_t cnt[2] = {0u, 0u};  // per <= 2 (S <= 1024)
  uint32_t mine = 0;
  int sp = 0;
  for (uint32_t s = s0, q = 0; s < s1; ++s, ++q) {
    const uint32_t cw = tinfo[(size_t)t * 2 * S + S + s];
    sp |= (cw & kRunSpilled) != 0;
    cnt[q] = cw & ~kRunSpilled;
    mine += cnt[q];
    L.bias[s] = tinfo[(size_t)t * 2 * S + s];
  }
  const uint32_t incl = wave_incl_scan(mine);
  if (lane == kWave - 1) wsum[w] = incl;
  spill = __syncthreads_or(sp);
  uint32_t acc = incl - mine;
  for (unsigned ww = 0; ww < w; ++ww) acc += wsum[ww];
  if (threadIdx.x == kST - 1) total_s = acc + mine;
  for (uint32_t s = s0, q = 0; s < s1; ++s, ++q) {
    L.excl[s] = acc;
    L.bias[s] -= acc;
    for (uint32_t j = acc; j < acc + cnt[q]; ++j) L.owner[j] = (OwnT)s;
    acc += cnt[q];
  }
  __syncthreads();
  return total_s;
}

constexpr uint8_t kAbsent = 0xff;  // staged status: no record of this message in the tile's runs
// NARROW (S <= 256): a 1-B owner table whose bytes are reused for the staged
// statuses once the records are loaded -- 36 KB of LDS instead of 46 KB, four
// blocks per CU (with at most 64 VGPRs: launch bounds 8 waves per SIMD)
__host__ __device__ constexpr size_t ring_drain_lds_bytes(uint32_t S, size_t tile = kSTile) {
  return S <= 256 ? tile * (8 + 1) + (size_t)S * 8 : tile * (8 + 2 + 1) + (size_t)S * 8;
}

// Tile t's records, read in RING order from its runs (tinfo), each through the
// handler table; replies staged in LDS at their place in the tile and written
// out coalesced.  FRESH: the records were written by other waves of THIS block
// in this kernel (the fused sort + drain) -- loaded non-temporal (L1 bypassed:
// served by the XCD's L2, which holds the stores; a line another block of the
// CU cached earlier would be stale in L1).
struct DrainCounts {
  unsigned long long done = 0, failed = 0, holes = 0;
};

// The lean body of the narrow ring drain: a tile of 8-B records on a view of at most
// kStatelessShards small rings (rings_small) with plain reply arrays (no rv.slots).
//
// Its runs (load_tile_runs8).  Wave 0 alone reads the tile's run words, scans the counts and
// leaves in LDS the slot biases, the exclusive prefixes and, per group of 64 run entries (one
// wave's share of one item), the shards of the group's first and last entry; one barrier.
// No owner table and no fill loop (8 lanes wrote 4 KB of owner bytes while seven waves stood at
// the barrier), no three-barrier vote, and the status stage, cleared ahead of that barrier,
// needs no barriers of its own: a tile costs two barriers (was seven).
struct Run8Lds {
  uint32_t bias[kStatelessShards];  // ring slot of run entry j of shard s: s << log_q | ((bias[s] + j) & (Q - 1))
  uint32_t excl[kStatelessShards];  // exclusive prefix of the counts (a shard the view lacks: the total)
  uint32_t grp[(kST * kSK) / kWave];  // entries [64 g, 64 g + 64): shard of the first | shard of the last << 8
  uint32_t total, spill;
};
template <int SK>
__device__ __forceinline__ uint32_t load_tile_runs8(const MboxView& mv, const uint32_t* __restrict__ tinfo, uint32_t t,
                                                    Run8Lds& R, int& spill) {
  static_assert((kST * SK) / kWave <= kWave && kStatelessShards <= kWave, "one lane per group and per shard");
  const uint32_t S = 1u << mv.log_s;
  if (threadIdx.x < kWave) {  // (a whole wave)
    const uint32_t lane = threadIdx.x;
    uint32_t cnt = 0, bw = 0;
    int sp = 0;
    if (lane < S) {
      const uint32_t cw = tinfo[(size_t)t * 2 * S + S + lane];
      sp = (cw & kRunSpilled) != 0;
      cnt = cw & ~kRunSpilled;
      bw = tinfo[(size_t)t * 2 * S + lane];
    }
    const uint32_t incl = wave_incl_scan(cnt), ex = incl - cnt;
    if (lane < kStatelessShards) {
      R.bias[lane] = bw - ex;
      R.excl[lane] = ex;
    }
    // entry j's shard: the number of shards 1.. whose runs start at or below j
    const uint32_t jf = lane * kWave, jl = jf + (kWave - 1);
    uint32_t sf = 0, sl = 0;
#pragma unroll
    for (int q = 1; q < (int)kStatelessShards; ++q) {
      const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)ex, q);
      sf += jf >= e, sl += jl >= e;
    }
    if (lane < (kST * SK) / kWave) R.grp[lane] = sf | (sl << 8);
    const bool any_sp = __any(sp) != 0;
    if (lane == kWave - 1) R.total = incl, R.spill = any_sp;
  }
  __syncthreads();
  spill = (int)R.spill;
  return R.total;
}

// The lean tile body behind its runs, for a tile that did not spill:
//   owner by compare -- this wave's eight groups' shard pairs are read once into scalars; a group
//   inside one run (all but at most seven of a tile's 64) takes its shard and bias as scalars, a
//   group a run ends in compares its entries against the prefixes;
//   slots and record addresses in 32 bits; fields decoded in 32 bits when the widths allow
//   (rec8_fast: Multiply is then one 32 x 32 -> 64 multiply);
//   the reply bounds tested once for the tile.
template <int FIXED, int SK>
__device__ __forceinline__ DrainCounts drain_ring_tile_lean(MboxView mv, SortIn in, uint32_t i0, uint32_t n_t, uint32_t T,
                                                            const Run8Lds& R, int64_t* sval, uint8_t* sst,
                                                            int64_t* __restrict__ state, uint32_t n_state,
                                                            uint64_t delay_ticks, OutboxView ob, ReplyView rv) {
  unsigned long long done = 0, failed = 0, holes = 0;
  const uint32_t w8 = *in.r8w;
  const Rec8Fast f = rec8_fast(w8);
  const uint32_t qmask = (1u << mv.log_q) - 1u;
  const unsigned char* recs = reinterpret_cast<const unsigned char*>(mv.rec);
  const uint32_t wv = threadIdx.x / kWave, lane = lane_id();
  // lanes 0..7: item k = lane's group of this wave (entries k * kST + wv * 64 ...), and shard lane's bias
  const uint32_t gp = R.grp[(lane & (SK - 1)) * (kST / kWave) + wv];
  const uint32_t bl = R.bias[lane & (kStatelessShards - 1)];
  uint64_t ha[SK];
#pragma unroll
  for (int k = 0; k < SK; ++k) {  // ring order: lane-consecutive entries of the runs
    const uint32_t j = (uint32_t)k * kST + threadIdx.x;
    const uint32_t pair = (uint32_t)__builtin_amdgcn_readlane((int)gp, k);
    const uint32_t sf = pair & 0xffu;
    uint32_t slot;
    if (sf == (pair >> 8)) {  // (wave-uniform)
      const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bl, sf);
      slot = (sf << mv.log_q) | ((b + j) & qmask);
    } else {
      uint32_t s = 0;
#pragma unroll
      for (uint32_t q = 1; q < kStatelessShards; ++q) s += j >= R.excl[q];
      slot = (s << mv.log_q) | ((R.bias[s] + j) & qmask);
    }
    if (j < T) ha[k] = *reinterpret_cast<const uint64_t*>(recs + (slot << 3));
  }
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const uint32_t j = (uint32_t)k * kST + threadIdx.x;
    if (j >= T) continue;
    const uint32_t lo = (uint32_t)ha[k], hi = (uint32_t)(ha[k] >> 32);
    const uint32_t local = lo & ((kST * SK) - 1);
    if (local >= n_t) {  // never written this epoch (cannot happen on a spill-free tile)
      ++holes;
      continue;
    }
    MsgRecord m;
    m.method = (uint16_t)(FIXED ? FIXED : in.method_uniform);
    m.flags = 0;
    m.a2 = 0;
    if (f.ok) {
      const uint32_t z0 = __builtin_amdgcn_alignbit(hi, lo, f.s0) & f.m0, z1 = hi >> f.s1h;
      m.actor = (lo >> 12) & f.mm;
      m.a0 = (int64_t)(int32_t)((z0 >> 1) ^ (0u - (z0 & 1u)));
      m.a1 = (int64_t)(int32_t)((z1 >> 1) ^ (0u - (z1 & 1u)));
    } else {
      const SortRec x = decode_rec8<false, SK>(ha[k], in, w8, 0u);
      m.actor = x.mb;
      m.a0 = x.a0, m.a1 = x.a1;
    }
    const ReplyRecord rr = run_handler(m, state, n_state, delay_ticks, ob);
    failed += rr.status != kStatusOk;
    sval[local] = rr.value;
    sst[local] = (uint8_t)rr.status;
    ++done;
  }
  // (every record load is waited for here, on every path: see drain_ring_tile)
  __builtin_amdgcn_s_waitcnt(kWaitVmcnt0);
  __syncthreads();
  uint8_t rst[SK];
  int64_t rval[SK];
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const uint32_t j = (uint32_t)k * kST + threadIdx.x;
    rst[k] = j < n_t ? sst[j] : kAbsent;
    rval[k] = sval[j];
  }
  // the tile's replies: its origins are o0 + j without wrapping and inside the reply arrays
  const uint32_t o0 = in.origin_base + i0;
  const bool whole = (uint64_t)o0 + (kST * SK) <= rv.n && (uint64_t)o0 + (kST * SK) <= 0x100000000ull;
  int64_t* vb = rv.val + o0;
  int32_t* sb = rv.st + o0;
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const uint32_t j = (uint32_t)k * kST + threadIdx.x;
    if (rst[k] == kAbsent) continue;
    if (whole) {
      __builtin_nontemporal_store(rval[k], vb + j);
      __builtin_nontemporal_store((int32_t)rst[k], sb + j);
    } else {
      put_reply_nt(rv, o0 + j, rval[k], rst[k]);
    }
  }
  return DrainCounts{done, failed, holes};
}

// (views and counts by value: references to a kernel's locals or arguments put
// them in scratch)
template <int FIXED, bool NARROW, bool FRESH, int RF = 0, int SK = kSK>
__device__ __forceinline__ DrainCounts drain_ring_tile(MboxView mv, SortIn in, uint32_t t,
                                                       const uint32_t* __restrict__ tinfo,
                                                       const uint32_t* __restrict__ sidx,
                                                       const uint32_t* __restrict__ rw, int64_t* __restrict__ state,
                                                       uint32_t n_state, uint64_t delay_ticks, OutboxView ob,
                                                       ReplyView rv, unsigned char* smem_rd) {
  unsigned long long done = 0, failed = 0, holes = 0;
  using OwnT = typename std::conditional<NARROW, uint8_t, uint16_t>::type;
  const uint32_t S = 1u << mv.log_s;
  int64_t* sval = reinterpret_cast<int64_t*>(smem_rd);  // [(kST * SK)] reply values by place in the tile
  RunLds<OwnT> L;
  L.bias = reinterpret_cast<uint32_t*>(sval + (kST * SK));
  L.excl = L.bias + S;
  L.owner = reinterpret_cast<OwnT*>(L.excl + S);
  // [(kST * SK)] statuses, kAbsent = none (NARROW: the owner table's bytes, once the records are loaded)
  uint8_t* sst = NARROW ? reinterpret_cast<uint8_t*>(L.owner) : reinterpret_cast<uint8_t*>(L.owner + (kST * SK));
  const uint64_t i0 = (uint64_t)t * (kST * SK);
  const uint32_t n_t = (uint32_t)min((uint64_t)(kST * SK), (uint64_t)in.M - i0);
  // the lean body (drain_ring_tile_lean) has no owner table: the status stage is its own from the start
  constexpr bool kLeanForm = NARROW && RF == 1 && !FRESH;
  if constexpr (kLeanForm) {
    if (rv.slots == nullptr && S <= kStatelessShards && rings_small(mv)) {
      __shared__ Run8Lds R8;
      for (uint32_t j = threadIdx.x; j < (kST * SK); j += kST) sst[j] = kAbsent;
      int spill8 = 0;
      const uint32_t T8 = load_tile_runs8<SK>(mv, tinfo, t, R8, spill8);
      if (spill8) {
        drain_tile_msg<FIXED, FRESH, RF, SK>(mv, in, t, sidx, rw, state, n_state, delay_ticks, ob, rv, done, failed,
                                             holes);
        return DrainCounts{done, failed, holes};
      }
      return drain_ring_tile_lean<FIXED, SK>(mv, in, (uint32_t)i0, n_t, T8, R8, sval, sst, state, n_state, delay_ticks,
                                             ob, rv);
    }
  }
  if constexpr (!NARROW)
    for (uint32_t j = threadIdx.x; j < (kST * SK); j += kST) sst[j] = kAbsent;
  int spill = 0;
  const uint32_t T = load_tile_runs(mv, tinfo, t, L, spill);
  if (spill) {  // some message of the tile spilled: the scatter left the tile's slot indices
    drain_tile_msg<FIXED, FRESH, RF, SK>(mv, in, t, sidx, rw, state, n_state, delay_ticks, ob, rv, done, failed, holes);
    return DrainCounts{done, failed, holes};
  }
  const uint64_t sbase_mask = (1ull << mv.log_q) - 1;
  using RecT = typename std::conditional<RF == 1, uint64_t, u32x4>::type;  // the ring record as loaded
  const uint32_t w8 = RF == 1 ? *in.r8w : 0u;  // the 8-B field widths this Send's sort used
  RecT ha[SK];
  uint32_t sl[SK];
  uint16_t pl[SK];  // (RF 2) the places in the tile
#pragma unroll
  for (int k = 0; k < SK; ++k) {  // ring order: lane-consecutive entries of the runs
    const uint32_t j = (uint32_t)k * kST + threadIdx.x;
    sl[k] = kNoSlot;
    if (j < T) {
      const uint32_t s = L.owner[j];
      sl[k] = (uint32_t)(((uint64_t)s << mv.log_q) | ((L.bias[s] + j) & sbase_mask));
      if constexpr (RF == 1) {
        const uint64_t* rp = reinterpret_cast<const uint64_t*>(mv.rec) + sl[k];
        ha[k] = FRESH ? __builtin_nontemporal_load(rp) : *rp;
      } else {
        const u32x4* rp = reinterpret_cast<const u32x4*>(rec_a(mv, sl[k]));
        ha[k] = FRESH ? __builtin_nontemporal_load(rp) : *rp;
        if constexpr (RF == 2) {
          const uint16_t* pp = rec_place(mv) + sl[k];
          pl[k] = FRESH ? __builtin_nontemporal_load(pp) : *pp;
        }
      }
    }
  }
  if constexpr (NARROW) {  // every owner entry is read: its bytes become the status stage
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < (kST * SK); j += kST) sst[j] = kAbsent;
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    if (sl[k] == kNoSlot) continue;
    SortRec x;
    if constexpr (RF == 1) {
      x = decode_rec8<FRESH, SK>(ha[k], in, w8, in.origin_base + (uint32_t)i0);
    } else if constexpr (RF == 2) {
      x = decode_wide(ha[k], in, in.origin_base + (uint32_t)i0 + pl[k]);
    } else {
      u32x4 hb = {0u, 0u, 0u, 0u};
      int64_t a2v = 0;
      if (rec_is_long(ha[k])) {
        const u32x4* bp = reinterpret_cast<const u32x4*>(rec_b(mv, sl[k]));
        hb = FRESH ? __builtin_nontemporal_load(bp) : *bp;
        if (((ha[k].z >> 16) & kFlagA2) && mv.a2) a2v = FRESH ? __builtin_nontemporal_load(mv.a2 + sl[k]) : mv.a2[sl[k]];
      }
      x = decode_sorted(ha[k], hb, a2v);
    }
    const uint32_t local = x.origin - in.origin_base - (uint32_t)i0;
    if (!x.valid || local >= n_t) {  // never written this epoch (cannot happen on a spill-free tile)
      ++holes;
      continue;
    }
    MsgRecord m;
    m.actor = x.mb;
    m.method = (uint16_t)(FIXED ? FIXED : x.method);
    m.flags = (uint16_t)x.flags;
    m.a0 = x.a0, m.a1 = x.a1, m.a2 = x.a2;
    const ReplyRecord rr = run_handler(m, state, n_state, delay_ticks, ob);
    failed += rr.status != kStatusOk;
    sval[local] = rr.value;
    sst[local] = (uint8_t)rr.status;
    ++done;
  }
  // Every record load is waited for here, on every path: a record is loaded under `j < T` and
  // decoded under `sl[k] != kNoSlot`, so the compiler sees a path on which the load is still out
  // when its registers are written again in the write-out below, and -- the outstanding count
  // being unknown behind the branches -- put an s_waitcnt vmcnt(0) in front of each item, behind
  // the previous item's reply stores (stores count in vmcnt on gfx950): a block's 8 store pairs
  // went out one acknowledged round trip after another (profiles/sort_drain_waits.md).
  __builtin_amdgcn_s_waitcnt(kWaitVmcnt0);
  __syncthreads();
  // the tile's replies, coalesced (misses were answered by the scatter): the staged pairs into
  // registers first, then the stores of the present ones back to back
  // (non-temporal: 56.4-58.8 vs 54.1-55.7 G on the headline step, one box, alternated; the
  // same stores measured flat-to-slower in the arrival, SeqFold and N > 1 completions,
  // which keep plain stores -- profiles/r6_small_sends.md)
  uint8_t rst[SK];
  int64_t rval[SK];
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const uint32_t j = (uint32_t)k * kST + threadIdx.x;  // (below kST * SK: inside both stages)
    rst[k] = j < n_t ? sst[j] : kAbsent;
    rval[k] = sval[j];
  }
#pragma unroll
  for (int k = 0; k < SK; ++k) {
    const uint32_t j = (uint32_t)k * kST + threadIdx.x;
    if (rst[k] != kAbsent) put_reply_nt(rv, in.origin_base + (uint32_t)(i0 + j), rval[k], rst[k]);
  }
  return DrainCounts{done, failed, holes};
}

// ---------------------------------------------------------------- kernel variant tables
// A family's instantiations, listed: a row is the key of a variant (vkey of the template
// arguments the family varies, as the plan computes it), the dynamic LDS it may ask for
// past the 64 KB default (0: never more), its name and the kernel.  The tables ARE the set
// of kernels a Send can launch: a variant is added or removed as one row.
template <class Fn>
struct Variant {
  uint32_t key;
  size_t max_lds;
  const char* name;
  Fn* fn;
};
#define MBX_ROW(key, max_lds, ...) {key, max_lds, #__VA_ARGS__, __VA_ARGS__}

struct VariantName {
  int family;
  uint32_t key;
  const char* name;
};

namespace {  // (per TU: a table's once-flag is its own)
template <class Fn, size_t N>
Fn* variant(const Variant<Fn> (&t)[N], uint32_t key) {
  for (const Variant<Fn>& r : t)
    if (r.key == key) return r.fn;
  throw std::logic_error(std::string("mailbox send: no variant of ") + t[0].name + " for key " + std::to_string(key));
}
// once per process, before the first launch that may need it
template <class Fn, size_t N>
void variants_allow_lds(const Variant<Fn> (&t)[N]) {
  static bool done = false;
  if (done) return;
  for (const Variant<Fn>& r : t)
    if (r.max_lds)
      PT_HIP_CHECK(hipFuncSetAttribute((const void*)r.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.max_lds));
  done = true;
}
template <class Fn, size_t N>
void variant_names(int family, const Variant<Fn> (&t)[N], std::vector<VariantName>& out) {
  for (const Variant<Fn>& r : t) out.push_back({family, r.key, r.name});
}
}  // namespace

// ---------------------------------------------------------------- launchers
// What every launcher takes besides the plan, the batch and the ring view: the Send's
// workspaces (Mailboxes::sort_ws) and what the handlers run on.
struct HandlerArgs {
  int64_t* state;
  uint32_t n_state;
  uint64_t delay_ticks;
  OutboxView ob;
  ReplyView rv;
};
// mailbox_sort_fused.hip (route modes 1 and 3) and mailbox_sort_fused_other.hip (0 and 2)
void mbx_launch_fused(const SortPlan& p, const SortIn& in, const MboxView& mv, const SortWs& ws, const HandlerArgs& h,
                      hipStream_t st);
void mbx_launch_fused_other(const SortPlan& p, const SortIn& in, const MboxView& mv, const SortWs& ws,
                            const HandlerArgs& h, hipStream_t st);
// mailbox_sort_ordered.hip: the ordered drain + the ring-order completion
void mbx_launch_ordered(const SortPlan& p, const SortIn& in, const MboxView& mv, const SortWs& ws,
                        const HandlerArgs& h, hipStream_t st);
// mailbox_sort_arrival.hip: a Send on arrival rings, whole
void mbx_launch_arrival(const SortPlan& p, const SortIn& in, const MboxView& mv, const SortWs& ws,
                        const HandlerArgs& h, hipStream_t st);
// each TU's rows (_hip.mailbox_variants)
void mbx_fused_variants(std::vector<VariantName>& out);
void mbx_fused_other_variants(std::vector<VariantName>& out);
void mbx_ordered_variants(std::vector<VariantName>& out);
void mbx_arrival_variants(std::vector<VariantName>& out);

}  // namespace ptype
