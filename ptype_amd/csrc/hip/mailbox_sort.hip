// Sorted epoch mailboxes: K2 as a stable counting sort into the shard rings,
// K3 as a ring-order parallel drain or an LDS-binned ordered drain.
//
// The epoch form of a Send (mailbox.hpp has the ring layout) runs
//
//   sort     every message goes into its shard's ring at (tail + prefix + rank),
//            the rank computed in message order (wave match on the shard bits +
//            per-wave counts), so each ring holds its messages in MESSAGE ORDER:
//            every actor's mailbox is FIFO by construction, with no atomic per
//            message.  Two forms:
//              one pass (batches of >= 1024 tiles): a block claims the next tile,
//              resolves it (one route-directory gather per message), ranks it,
//              and finds its prefix by a decoupled look-back over earlier tiles'
//              descriptors (mbx_onesweep_kernel);
//              count + scatter: the count resolves and histograms per block
//              (+ group sums over 32 blocks); each scatter block's prefix is the
//              group sums before its group plus at most 31 rows inside it (no
//              scan pass);
//            either records each tile's runs (slot bias + count per shard) for
//            the drains;
//   drain    parallel (batches without ordered methods): one block per tile reads
//            the tile's runs in ring order (whole lines), stages the replies in
//            LDS at their place in the tile and writes them out coalesced;
//            ordered: one block owns one shard -- its actors' state staged in
//            LDS -- and runs each actor's records one at a time in ring order,
//            distinct actors side by side (LDS bins), replies staged at their
//            ring slots; a ring-order completion puts them in message order.
//
// Stateless batches use an 8-shard view of the rings (every ring is empty
// between epoch Sends): longer runs per tile and shard.  Arrival sharding
// (stateless only) skips the sort: tile t's messages sit at fixed positions of
// ring t mod S.
//
// Records are 16 B in the common case (compact form, plane A only):
//   w0 = origin | kCompactMark    (bit 31 marks an epoch record; a live ring's
//                                  lap tags never have it)
//   w1 = mailbox (24 bits) | method << 24 (7 bits)
//   w2, w3 = a0, a1 as int32
// 8 B for stateless batches of one method with two arguments (in.rec8, set by
// the host: one u64 per slot of plane A viewed as 8-B cells):
//   bits [0, 12) place in the tile (the drains know the tile) | mailbox (wm bits)
//   | zigzag a0 (w0 bits) | zigzag a1 (w1 bits),   12 + wm + w0 + w1 = 64
// where a message whose mailbox or arguments do not fit the fields SPILLS (its
// tile is drained in message order, the message run straight from the batch).
// The widths are a device word the previous Send's last block sets from that
// Send's per-tile field maxima (no host read): a batch whose values grow spills
// for one Send, then fits;
// and 32 B (+ the a2 side array) when an argument needs 64 bits or a third
// argument is present (long form: w1 bit 31, w2 = method | flags << 16, plane B
// {a0, a1}).  The tagged 32-B records of mailbox.hip stay the format of live
// sessions (persistent consumer) and of delivery on receipt.
//
// XCD-aware placement (MI355X: 8 XCDs, per-XCD L2s, blocks dealt round-robin):
// count / scatter block b takes the range of virtual block (b % 8) * G/8 + b / 8,
// so each XCD owns one contiguous eighth of the batch -- and therefore one
// contiguous part of every shard's run, whose partially written lines meet in
// ONE L2.
//
// Reference: the server's per-request goroutine of stdlib net/rpc
// (example/calculator/server/server.go:16-20, :38; handler
// example/calculator/calculator.go:9-12) -- here an explicit FIFO queue in HBM.
#include "mailbox_sort_dev.hpp"

namespace ptype {

// ---------------------------------------------------------------- K2s pass 1: count
template <int MODE>
__global__ __launch_bounds__(kST) void mbx_count_kernel(SortIn in, uint32_t log_s, uint32_t* __restrict__ hist,
                                                        uint32_t* __restrict__ gsum, uint32_t* __restrict__ rw) {
  __shared__ uint32_t cnt[kMboxSortMaxShards];
  const uint32_t S = 1u << log_s;
  const uint32_t v = virt_block(blockIdx.x, in.G);
  for (uint32_t s = threadIdx.x; s < S; s += kST) cnt[s] = 0;
  __syncthreads();
  const uint32_t t0 = v * in.tpb, t1 = min(t0 + in.tpb, in.tiles);
  uint32_t a[kSK];
  if (t0 < t1) load_actors(in, t0, a);
  for (uint32_t t = t0; t < t1; ++t) {
    int r[kSK];
    uint32_t mb[kSK];
    resolve_k<MODE>(in, a, r, mb);
    if (t + 1 < t1) load_actors(in, t + 1, a);  // next tile's loads in flight while this one counts
#pragma unroll
    for (int k = 0; k < kSK; ++k) {
      const int64_t i = tile_index(t, k);
      const bool ok = r[k] == in.rank_self && mb[k] < kMaxMbox;
      if (i < in.M) rw[i] = ok ? mb[k] : kNoSlot;
      if (ok) atomicAdd(&cnt[mb[k] & (S - 1)], 1u);
    }
  }
  __syncthreads();
  uint32_t* g = gsum + (size_t)(v / kGroupBlocks) * S;
  for (uint32_t s = threadIdx.x; s < S; s += kST) {
    const uint32_t c = cnt[s];
    hist[(size_t)v * S + s] = c;
    if (c) atomicAdd(&g[s], c);
  }
}

// ---------------------------------------------------------------- K2s pass 2: scatter
// The tile's arguments are loaded with its route words, before the ranking (in
// flight across it).  Loading them only once the ranks are known (a smaller
// register file, occupancy 4 -> 5) measured slower: 124 -> 164 us per 8 Mi.
template <bool A2, bool MC>
__device__ __forceinline__ void load_routed(const SortIn& in, const uint32_t* __restrict__ rw, uint32_t t,
                                            uint32_t (&m)[kSK], int64_t (&x0)[kSK], int64_t (&x1)[kSK],
                                            int64_t (&x2)[kSK], uint32_t (&meth)[kSK]) {
#pragma unroll
  for (int k = 0; k < kSK; ++k) {
    const int64_t i = tile_index(t, k);
    const bool ok = i < in.M;
    m[k] = ok ? __builtin_nontemporal_load(rw + i) : kNoSlot;
    x0[k] = ok ? __builtin_nontemporal_load(in.a0 + i) : 0;
    x1[k] = ok && in.a1 ? __builtin_nontemporal_load(in.a1 + i) : 0;
    x2[k] = 0;
    if constexpr (A2) x2[k] = ok ? __builtin_nontemporal_load(in.a2 + i) : 0;
    meth[k] = in.method_uniform;
    if constexpr (MC) meth[k] = ok ? (uint32_t)in.mcol[i] : 0u;
  }
}

// Per-tile runs (`tinfo`, [tiles][2][S] u32): tile t's records of shard s sit at
// ring slots s | ((bias + j) & (Q - 1)), j < count (bias = epoch-start tail +
// the run's offset + the shard's rotation; count clamped to the free room, its
// top bit set when the run spilled / overflowed the room) -- what the ring-order
// drain and completion read instead of a per-message slot index.  The slot
// index `sidx` is written only where a consumer needs it: every message with
// `all_sidx` (the message-order drain, tune mbox_drain_msg=1), and the whole
// tile when some message of it spilled (the drain runs that tile in message
// order).  (An opt-in LDS-staged write-out in ring order measured slower,
// 117 -> 161 us per 8 Mi msgs: the 80 KB stage halved the resident blocks;
// removed, see git history 4c4ea76.)
__host__ __device__ constexpr size_t scatter_lds_bytes(uint32_t S) { return (size_t)S * (16 + 4 * (kST / kWave)); }

template <bool A2, bool MC>
__global__ __launch_bounds__(kST) void mbx_scatter_kernel(SortIn in, MboxView mv, const uint32_t* __restrict__ hist,
                                                          const uint32_t* __restrict__ gsum,
                                                          uint32_t* __restrict__ rw,
                                                          uint32_t* __restrict__ sidx, uint32_t* __restrict__ tinfo,
                                                          ReplyView rv, bool spill, bool all_sidx) {
  // LDS sized by the shard count (16 + 4 * waves B per shard): occupancy is not
  // capped by the 1024-shard maximum
  extern __shared__ __align__(16) unsigned char smem_sc[];
  const uint32_t S = 1u << mv.log_s;
  unsigned long long* base = reinterpret_cast<unsigned long long*>(smem_sc);  // ring position of offset 0 (tail)
  uint32_t* run = reinterpret_cast<uint32_t*>(base + S);  // this block's next offset per shard
  uint32_t* room = run + S;                               // offset limit (free ring slots)
  uint32_t* wcnt_all = room + S;                          // [kST / kWave][S] per-wave counts -> wave offsets
  auto wcnt = [&](unsigned ww, uint32_t sh) -> uint32_t& { return wcnt_all[ww * S + sh]; };
  const uint64_t Q = 1ull << mv.log_q;
  const uint32_t v = virt_block(blockIdx.x, in.G);
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  const uint32_t g0 = v / kGroupBlocks, v0 = g0 * kGroupBlocks;
  for (uint32_t s = threadIdx.x; s < S; s += kST) {
    // this block's prefix: whole groups before it, then the rows before it in its group
    uint32_t p = 0;
    for (uint32_t g = 0; g < g0; ++g) p += gsum[(size_t)g * S + s];
    for (uint32_t u = v0; u < v; ++u) p += hist[(size_t)u * S + s];
    run[s] = p;
    const uint64_t tl = *ctr_tail(mv, s), hd = *ctr_head(mv, s);
    base[s] = tl;
    const uint64_t free = hd + Q > tl ? hd + Q - tl : 0;
    room[s] = (uint32_t)(free < 0xffffffffull ? free : 0xffffffffull);
  }
  unsigned long long n_enq = 0, n_ovf = 0, n_miss = 0, n_spill = 0;
  const uint32_t t0 = v * in.tpb, t1 = min(t0 + in.tpb, in.tiles);
  for (uint32_t t = t0; t < t1; ++t) {
    for (uint32_t s = lane; s < S; s += kWave) wcnt(w, s) = 0;  // this wave's row only
    uint32_t mb[kSK], meth[kSK];
    int64_t v0[kSK], v1[kSK], v2[kSK];
    load_routed<A2, MC>(in, rw, t, mb, v0, v1, v2, meth);
    // rank of each message among this wave's earlier messages of its shard
    uint32_t wr[kSK], sh[kSK];
#pragma unroll
    for (int k = 0; k < kSK; ++k) {
      const bool ok = mb[k] != kNoSlot;
      sh[k] = mb[k] & (S - 1);
      const uint64_t peers = match_bits(sh[k], mv.log_s, __ballot(ok));
      const unsigned below = mbcnt64(peers);
      const int leader = peers ? __builtin_ctzll(peers) : 0;
      unsigned old = 0;
      if (ok && below == 0) {  // group leader: one plain LDS read-add per distinct shard of the wave
        old = wcnt(w, sh[k]);
        wcnt(w, sh[k]) = old + (unsigned)__popcll(peers);
      }
      wr[k] = (unsigned)__shfl((int)old, leader) + below;
    }
    __syncthreads();
    int sp = 0;
    for (uint32_t s = threadIdx.x; s < S; s += kST) {  // wave offsets in message order, then the block's run
      uint32_t rr = run[s];
#pragma unroll
      for (int ww = 0; ww < kST / kWave; ++ww) {
        const uint32_t c = wcnt(ww, s);
        wcnt(ww, s) = rr;
        rr += c;
      }
      run[s] = rr;
      sp |= rr > room[s];
    }
    bool tile_spill = false;  // (either barrier publishes the wave offsets too)
    if (spill) tile_spill = __syncthreads_or(sp) != 0;
    else __syncthreads();
    const bool wsidx = all_sidx || tile_spill;
#pragma unroll
    for (int k = 0; k < kSK; ++k) {
      const int64_t i = tile_index(t, k);
      if (i >= in.M) continue;
      const uint32_t origin = in.origin_base + (uint32_t)i;
      if (mb[k] == kNoSlot) {
        ++n_miss;
        if (wsidx) sidx[i] = kNoSlot;
        write_status(rv, origin, kStatusNoActor);
        continue;
      }
      const uint32_t off = wcnt(w, sh[k]) + wr[k];
      if (off >= room[sh[k]]) {  // the ring is full
        if (spill) {  // stateless batch: the drain runs it from the batch
          ++n_spill;
          sidx[i] = kSpillSlot;
          continue;
        }
        ++n_ovf;  // answered now, re-sent by send_all
        if (wsidx) sidx[i] = kNoSlot;
        write_status(rv, origin, kStatusOverflow);
        continue;
      }
      const int64_t x0 = v0[k], x1 = v1[k], x2 = v2[k];
      const uint32_t mt = meth[k];
      const uint64_t slot = slot_at(mv, sh[k], base[sh[k]] + off);
      if (wsidx) sidx[i] = (uint32_t)slot;
      if (mt < 128u && fits_i32(x0) && fits_i32(x1) && x2 == 0) {
        *reinterpret_cast<u32x4*>(rec_a(mv, slot)) =
            u32x4{origin | kCompactMark, mb[k] | (mt << 24), (uint32_t)x0, (uint32_t)x1};
      } else {
        const uint32_t fl = x2 != 0 ? (uint32_t)kFlagA2 : 0u;
        *reinterpret_cast<u32x4*>(rec_a(mv, slot)) =
            u32x4{origin | kCompactMark, mb[k] | kCompactLong, (mt & 0xffffu) | (fl << 16), 0u};
        *reinterpret_cast<u32x4*>(rec_b(mv, slot)) =
            u32x4{(uint32_t)x0, (uint32_t)((uint64_t)x0 >> 32), (uint32_t)x1, (uint32_t)((uint64_t)x1 >> 32)};
        if (fl) mv.a2[slot] = x2;
      }
      ++n_enq;
    }
    if (tinfo) {  // the tile's runs (after the stores: the messages' registers are dead by now -- +25 VGPRs above)
      // slot bias from the epoch-start tail (a drain may commit before the completion reads it)
      for (uint32_t s = threadIdx.x; s < S; s += kST) {
        const uint32_t r0 = wcnt(0, s), rr = run[s];  // wave 0's offset = the run before this tile
        const uint32_t cc = r0 >= room[s] ? 0u : min(rr - r0, room[s] - r0);
        tinfo[(size_t)t * 2 * S + s] = (uint32_t)(base[s] + r0) + shard_rot(mv, s);
        tinfo[(size_t)t * 2 * S + S + s] = cc | (rr > room[s] ? kRunSpilled : 0u);
      }
    }
    __syncthreads();  // wcnt rows are reused by the next tile
  }
  block_add_stats(mv.stats, n_enq, kMbEnqueued, n_ovf, kMbOverflow, n_miss, kMbNoActor);
  if (spill) {
    __syncthreads();  // block_add_stats' LDS partials are reused
    block_add_stats(mv.stats, n_spill, kMbSpilled, 0, -1, 0, -1);
  }
}

template <int = 0>
__global__ __launch_bounds__(256) void mbx_presence_kernel(const uint8_t* __restrict__ dirr, uint32_t n_dir,
                                                           int rank_self, uint32_t* __restrict__ pres) {
  const uint32_t wi = blockIdx.x * 256u + threadIdx.x;
  if (wi >= pres_words(n_dir)) return;
  alignas(16) uint8_t b[16];
  if (wi * 16 + 16 <= n_dir) {  // (the table is a whole allocation: 16-B aligned)
    *reinterpret_cast<uint4*>(b) = *reinterpret_cast<const uint4*>(dirr + (size_t)wi * 16);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) b[j] = wi * 16 + j < n_dir ? dirr[wi * 16 + j] : kRankMissing;
  }
  uint32_t w = 0;
#pragma unroll
  for (uint32_t j = 0; j < 16; ++j) {
    const uint32_t st = b[j] == (uint8_t)rank_self ? 1u : b[j] == kRankFallback ? 2u : 0u;
    w |= st << (2 * j);
  }
  pres[wi] = w;
}

template <int MODE, bool A2, bool MC>
__global__ __launch_bounds__(kST) void mbx_onesweep_kernel(SortIn in, MboxView mv, unsigned long long* __restrict__ desc,
                                                           unsigned* __restrict__ tctr, uint32_t* __restrict__ gsum,
                                                           uint32_t* __restrict__ sidx, uint32_t* __restrict__ tinfo,
                                                           uint32_t* __restrict__ rw, ReplyView rv, bool spill,
                                                           bool all_sidx, bool reserve) {
  extern __shared__ __align__(16) unsigned char smem_os[];
  (void)onesweep_tile<MODE, A2, MC>(in, mv, desc, tctr, gsum, sidx, tinfo, rw, rv, spill, all_sidx, smem_os, reserve);
}

// ---------------------------------------------------------------- K2s persistent reserving sort
// The reserving one-pass sort of a presence-map Send (route mode 4) as a grid of
// resident blocks, each walking several tiles (tune mbox_persist).  What a tile of
// mbx_onesweep_kernel<4> repeats and a Send needs once is done once per block: the map
// staged in LDS, each ring's tail and room read, the enqueue counters added.  And the
// tile's serial chain of round trips is shortened by running one tile ahead on the cheap
// column: tile i+1's actor loads are issued before tile i's record stores, it is resolved
// and ranked right after them, and its runs' reservations (one returning atomic per shard)
// come back behind tile i+1's argument loads.  Only the next tile's actors / mailboxes and
// packed ranks (12 registers) cross an iteration whole; the arguments are never held a tile
// ahead of their stores (the 208-VGPR form, profiles/r5_mailbox_ab.md).  The prefixes, the
// wave offsets and the spill vote's flag word are double-buffered in LDS, so a tile costs
// two barriers: one between its votes / prefixes and its stores, one between the next
// tile's ranking and its reservations.
//
// What is in flight where (profiles/sort_drain_waits.md).  Tile i+1's 16 argument loads are
// issued directly behind tile i's last record store -- the registers are dead there -- and
// cross tile i+1's resolve, ranking, barrier and reservation, none of which waits for
// memory (the actors came in with tile i's arguments).  A whole tile's argument loads carry
// no bounds branches (load_args_tile).  At the top of iteration i+1 tile i+2's actor loads
// go out behind them; then ONE wait takes in all of them (os_loads_in), on every path, ahead
// of the barrier: from there to the tile's last record store no instruction waits on vmcnt,
// so the stores -- which count in vmcnt on gfx950 -- issue back to back.  The vote is a flag
// word a wave sets before the first barrier when a lane spills, read behind it, cleared
// behind the second (in place of __syncthreads_or: three barriers around an LDS word).
//
// The front half of a tile (profiles/rank_scan.md): the kernel is bound by instruction issue, not
// by memory, so resolve and rank are written for their instruction counts.  resolve_pres_lean
// turns the actor ids into mailboxes in place -- eight presence words read back to back, one
// wait, no branch; the hash-table probes behind one wave-uniform test -- and marks every message
// that takes no slot with kNoSlot, so no rank array exists.  os_rank_scan (a view has at most
// kStatelessShards shards here) ranks by one-hot byte counters scanned across the wave with DPP
// adds and keeps the wave's running counts in a register: one ds_bpermute per item and one LDS
// write of the row per tile, which therefore needs no clearing.  The field maxima are reduced by
// DPP as well (wave_max_u32).
//
// Tiles: no counter, no flag, no block waits for another.  Block b of G (a multiple of 8
// where there are 8 or more) sits on XCD b % 8; with a tile count that is a multiple of 8
// it takes tiles x * T/8 + j, j = b / 8 + i * G/8 -- the XCD virt_block gives each tile in
// the one-tile-per-block form, which is where the ring drain reads its runs.  Otherwise
// tile b + i * G.  A tile's runs land in the rings in the order the blocks reserve them,
// which a stateless ring allows (see onesweep_tile).
__host__ __device__ constexpr size_t persist_lds_bytes(uint32_t S) {
  return (size_t)S * (8 + 4 + 2 * 4 + 2 * 4 * (kST / kWave));
}

// (amdgpu_waves_per_eu: with the lean store loop beside the general one the register allocator, left
// to itself, settles at 137 VGPRs and three waves per SIMD; told the occupancy the kernel is built
// around it fits 128 without scratch)
template <int = 0>
__global__ __launch_bounds__(kST) __attribute__((amdgpu_waves_per_eu(4, 4)))
void mbx_persist_sort_kernel(SortIn in, MboxView mv, uint32_t* __restrict__ sidx, uint32_t* __restrict__ tinfo,
                             uint32_t* __restrict__ rw, ReplyView rv) {
  constexpr int SK = kSK;
  extern __shared__ __align__(16) unsigned char smem_ps[];
  const uint32_t S = 1u << mv.log_s;
  unsigned long long* base = reinterpret_cast<unsigned long long*>(smem_ps);  // each ring's epoch-start tail
  uint32_t* room = reinterpret_cast<uint32_t*>(base + S);                     // offset limit past the tail
  uint32_t* pre2 = room + S;                                                  // [2][S] a tile's prefix per shard
  uint32_t* wcnt2 = pre2 + 2 * S;                                             // [2][kST / kWave][S]
  uint32_t* lpres = reinterpret_cast<uint32_t*>(smem_ps + ((persist_lds_bytes(S) + 15) & ~(size_t)15));
  __shared__ uint32_t tmax[3];
  __shared__ uint32_t vote[2];  // the spill vote's flag word of a tile, double-buffered like pre / wcnt
  __shared__ uint32_t brot[kStatelessShards];  // (lean) each ring's tail + rotation, low word
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  // this block's tiles: first, first + stride, ... (n of them)
  const uint32_t G = gridDim.x, T = in.tiles;
  uint32_t first = blockIdx.x, stride = G, n = blockIdx.x < T ? (T - blockIdx.x + G - 1) / G : 0u;
  if (G >= 8 && (G & 7) == 0 && (T & 7) == 0) {
    const uint32_t j = blockIdx.x >> 3, T8 = T >> 3;
    stride = G >> 3;
    first = (blockIdx.x & 7) * T8 + j;
    n = j < T8 ? (T8 - j + stride - 1) / stride : 0u;
  }
  if (n == 0) return;
  // once per block: the map, the rings' tails and room
  stage_pres(in, lpres);
  for (uint32_t s = threadIdx.x; s < S; s += kST) {
    uint64_t tl;
    room[s] = os_ring_room(mv, s, tl);
    base[s] = tl;
    if (s < kStatelessShards) brot[s] = (uint32_t)tl + shard_rot(mv, s);
  }
  if (threadIdx.x < 3) tmax[threadIdx.x] = 0;
  if (threadIdx.x < 2) vote[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t w8 = in.rec8 ? *in.r8w : 0u;
  const bool maxima = in.rec8 || in.recw;
  // the lean store loop (os_store_lean) serves the 8-B stateless Send on its own rings' runs; a tile
  // that spilled keeps os_store_msg
  const bool lean = in.rec8 && !in.recw && tinfo != nullptr && rv.slots == nullptr && S <= kStatelessShards &&
                    rings_small(mv);
  uint32_t n_enq = 0, n_ovf = 0, n_miss = 0, n_spill = 0;  // (a block's share of a batch: below 2^32)
  // the first tile, up to its reservations in flight; its arguments behind its actors
  uint32_t nx[SK];  // the coming tile: actors, then mailboxes
  int64_t v0[SK], v1[SK];  // the coming tile's arguments, in flight from behind the last tile's stores
  PackedRanks<SK> wrp;
  {
    uint32_t wr[SK];
    const bool full = tile_is_full<SK>(in, first);
    load_actors<SK>(in, first, nx);
    load_args_tile<SK>(in, first, full, v0, v1);
    resolve_pres_lean<SK>(in, lpres, nx);
    os_rank_scan<SK>(S, nx, wcnt2 + w * S, wr);
    wrp.pack(wr);
  }
  __syncthreads();
  // (S <= kST: a shard's thread keeps its run's count and reserved offset in registers)
  uint32_t rc = 0, rx = 0;
  if (threadIdx.x < S) {
    rc = os_wave_offsets(wcnt2, S, threadIdx.x);
    rx = os_reserve(mv, threadIdx.x, rc);
  }
  for (uint32_t it = 0; it < n; ++it) {
    const uint32_t t = first + it * stride, b = it & 1;
    uint32_t* pre = pre2 + b * S;
    uint32_t* wcnt_all = wcnt2 + b * (kST / kWave) * S;
    const bool full = tile_is_full<SK>(in, t);
    uint32_t mb[SK];
#pragma unroll
    for (int k = 0; k < SK; ++k) mb[k] = nx[k];
    // the next tile's actors (in flight across this tile's stores), behind this tile's arguments and its
    // reservations, both issued a tile ago
    const bool more = it + 1 < n;
    const bool full_next = more && tile_is_full<SK>(in, t + stride);
    if (more) load_actors<SK>(in, t + stride, nx);
    // the one wait for the tile's loads, on every path: nothing below, up to the last record store, waits
    // for memory again -- not for the run words' stores either (the next tile's actors are in with the
    // arguments: its ranking follows the stores)
    os_loads_in<SK>(v0, v1, nx);
    int sp = 0;
    if (threadIdx.x < S) {
      const uint32_t s = threadIdx.x;
      pre[s] = rx;
      sp = os_run_info(mv, tinfo, t, S, s, base[s], room[s], rx, rc);
    }
    const uint32_t escm = os_fields<SK, true>(in, w8, mb, v0, v1, tmax);
    sp |= escm != 0;
    // the spill vote: a wave with a spilling lane sets this tile's flag word, read behind the tile's barrier
    if (__any(sp) && lane == 0) vote[b] = 1u;
    __syncthreads();
    const bool tile_spill = __builtin_amdgcn_readfirstlane((int)vote[b]) != 0;  // (block-uniform: a scalar)
    if (threadIdx.x == 0) {
      // (a tile spilled by its records' widths: flagged for the drains, as in onesweep_tile)
      if (tile_spill) tinfo[(size_t)t * 2 * S + S] |= kRunSpilled;
      if (maxima) {  // the tile's field bit lengths; cleared for the next tile (its maxima follow a barrier)
        (void)atomicExch(&in.r8max[t], tmax[0] | (tmax[1] << 8) | (tmax[2] << 16));
        tmax[0] = tmax[1] = tmax[2] = 0;
      }
    }
    if (lean && !tile_spill) {
      // every run fits its room and every field its width: this wave's ring positions per shard, once
      // (its own row of the wave offsets, not read again before the tile after the next clears it), and
      // the enqueued count from the runs' counts
      uint32_t* wpos = wcnt_all + w * S;
      if (lane < S) wpos[lane] += pre[lane] + brot[lane];
      __builtin_amdgcn_wave_barrier();  // (one wave: its LDS accesses are in order)
      if (threadIdx.x < S) n_enq += rc;
      const Rec8Fast f8 = rec8_fast(w8);
      const uint32_t place0 = w * (SK * kWave) + lane;  // this thread's first place in a tile
      if (f8.ok) {
#pragma unroll
        for (int k = 0; k < SK; ++k) {
          const int64_t i = tile_index<SK>(t, k);
          if (!full && i >= in.M) continue;
          os_store_lean<SK, true>(in, mv, rv, i, place0 + k * kWave, wpos, mb[k], wrp[k], v0[k], v1[k], f8, w8, n_miss);
        }
      } else {
#pragma unroll
        for (int k = 0; k < SK; ++k) {
          const int64_t i = tile_index<SK>(t, k);
          if (!full && i >= in.M) continue;
          os_store_lean<SK, false>(in, mv, rv, i, place0 + k * kWave, wpos, mb[k], wrp[k], v0[k], v1[k], f8, w8, n_miss);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < SK; ++k) {
        const int64_t i = tile_index<SK>(t, k);
        if (!full && i >= in.M) continue;
        os_store_msg<SK>(in, mv, rv, i, base, room, pre, wcnt_all + w * S, mb[k], wrp[k], v0[k], v1[k], 0, in.method_uniform,
                         (escm >> k) & 1u, w8, true, tile_spill, sidx, rw, n_enq, n_ovf, n_miss, n_spill);
      }
    }
    if (more) {
      // the next tile's arguments, right behind this tile's stores: in flight across its resolve, rank,
      // barrier and reservation
      load_args_tile<SK>(in, t + stride, full_next, v0, v1);
      // the next tile in the other buffer (last read before this tile's barrier): resolved, ranked, reserved
      uint32_t* wnext = wcnt2 + (b ^ 1) * (kST / kWave) * S;
      uint32_t wr[SK];
      resolve_pres_lean<SK>(in, lpres, nx);
      os_rank_scan<SK>(S, nx, wnext + w * S, wr);
      wrp.pack(wr);
      __syncthreads();
      // (every thread has read this tile's flag word: cleared for the tile after the next, whose votes
      // follow the next tile's barrier)
      if (threadIdx.x == 0) vote[b] = 0u;
      if (threadIdx.x < S) {
        rc = os_wave_offsets(wnext, S, threadIdx.x);
        rx = os_reserve(mv, threadIdx.x, rc);
      }
    }
  }
  // once per block: the enqueue counters
  block_add_stats(mv.stats, n_enq, kMbEnqueued, n_ovf, kMbOverflow, n_miss, kMbNoActor);
  __syncthreads();  // block_add_stats' LDS partials are reused
  block_add_stats(mv.stats, n_spill, kMbSpilled, 0, -1, 0, -1);
}

template <int FIXED>
__global__ __launch_bounds__(kST) void mbx_drain_msg_kernel(MboxView mv, SortIn in, const uint32_t* __restrict__ sidx,
                                                            const uint32_t* __restrict__ rw,
                                                            int64_t* __restrict__ state, uint32_t n_state,
                                                            uint64_t delay_ticks, OutboxView ob, ReplyView rv,
                                                            uint32_t* __restrict__ gsum, uint32_t ngroups,
                                                            unsigned* __restrict__ ticket, unsigned* __restrict__ tctr) {
  // the scatter's block -> tile ranges: a tile's records sit in ~S short runs that
  // this block's waves read whole (line reuse in L1 / L2), not one record per block
  unsigned long long done = 0, failed = 0, holes = 0;
  const uint32_t v = virt_block(blockIdx.x, in.G);
  const uint32_t t0 = v * in.tpb, t1 = min(t0 + in.tpb, in.tiles);
  for (uint32_t t = t0; t < t1; ++t)
    drain_tile_msg<FIXED>(mv, in, t, sidx, rw, state, n_state, delay_ticks, ob, rv, done, failed, holes);
  block_add_stats(mv.stats, done, kMbProcessed, failed, kMbFailed, holes, kMbHoles);
  __shared__ bool last;
  if (threadIdx.x == 0) last = last_block_ticket(ticket);
  __syncthreads();
  if (last) {  // every block's records are read: the rings are consumed
    const uint32_t S = 1u << mv.log_s;
    for (uint32_t s = threadIdx.x; s < S; s += kST) epoch_commit(mv, s, epoch_sum(mv, gsum, ngroups, S, s));
    if (threadIdx.x == 0) tctr[1] += 1u;  // the next Send's one-pass epoch tag
  }
}

template <int FIXED, bool NARROW, int RF, int SK = kSK>
__global__ __launch_bounds__(kST, (NARROW && FIXED) ? 8 : 1) void mbx_drain_ring_kernel(MboxView mv, SortIn in, const uint32_t* __restrict__ tinfo,
                                                             const uint32_t* __restrict__ sidx,
                                                             const uint32_t* __restrict__ rw,
                                                             int64_t* __restrict__ state, uint32_t n_state,
                                                             uint64_t delay_ticks, OutboxView ob, ReplyView rv,
                                                             uint32_t* __restrict__ gsum, uint32_t ngroups,
                                                             unsigned* __restrict__ ticket, unsigned* __restrict__ tctr,
                                                             uint32_t* __restrict__ r8host) {
  extern __shared__ __align__(16) unsigned char smem_rd[];
  const uint32_t S = 1u << mv.log_s;
  DrainCounts dc;
  // tiles dealt XCD by XCD like the scatter's blocks (whose writes the XCD's L2 may still hold)
  const uint32_t t = virt_block(blockIdx.x, gridDim.x);
  if (t < in.tiles)
    dc = drain_ring_tile<FIXED, NARROW, false, RF, SK>(mv, in, t, tinfo, sidx, rw, state, n_state, delay_ticks, ob,
                                                       rv, smem_rd);
  block_add_stats(mv.stats, dc.done, kMbProcessed, dc.failed, kMbFailed, dc.holes, kMbHoles);
  __shared__ bool last;
  if (threadIdx.x == 0) last = last_block_ticket(ticket);
  __syncthreads();
  if (last) {  // every block's records are read: the rings are consumed
    for (uint32_t s = threadIdx.x; s < S; s += kST) epoch_commit(mv, s, epoch_sum(mv, gsum, ngroups, S, s));
    if (threadIdx.x == 0) tctr[1] += 1u;  // the next Send's one-pass epoch tag
    if constexpr (RF != 0) rec8_next(in, const_cast<uint32_t*>(in.r8w), r8host, in.tiles);
  }
}

// Removed variants (measured slower or flat; A/B rows in profiles/r4_mailbox_ab.md and
// profiles/r5_mailbox_ab.md): the look-back sort for stateless batches (run reservations
// won), the persistent reserving sort with ONE block per CU that prefetched whole tiles (42.8
// vs 50.5 G msg/s; the kept one, mbx_persist_sort_kernel, runs two per CU and carries only the
// next tile's actors and ranks), the tile's store loop as one shared function (5-15 VGPRs more
// in every sort kernel; profiles/persistent_sort.md), the persistent sort's whole-tile loads
// on the actor column too and left to the scheduler (133 and 130 VGPRs: three waves per SIMD;
// profiles/sort_drain_waits.md), 1024- and 2048-message tiles for the
// fused / separate sort, arguments loaded after the look-back, the LDS-table count,
// the group look-back, non-temporal directory gathers and reply stores, the binned ordered
// drain (233 vs 175 us), 2048-record ordered windows, the ordered drain without the
// register fold or the prefetched window, 16-B ordered records at 8 Mi, the wide ring
// drain and the 8 / 16 / 32-shard stateless views other than 8.

// ---------------------------------------------------------------- variant tables (keys: mailbox_plan.hpp)
static const Variant<decltype(mbx_count_kernel<0>)> kCount[] = {
    MBX_ROW(vkey(0), 0, mbx_count_kernel<0>),
    MBX_ROW(vkey(1), 0, mbx_count_kernel<1>),
    MBX_ROW(vkey(2), 0, mbx_count_kernel<2>),
};
static const Variant<decltype(mbx_scatter_kernel<false, false>)> kScatter[] = {
    MBX_ROW(vkey(0, 0), 0, mbx_scatter_kernel<false, false>),
    MBX_ROW(vkey(0, 1), 0, mbx_scatter_kernel<false, true>),
    MBX_ROW(vkey(1, 0), 0, mbx_scatter_kernel<true, false>),
    MBX_ROW(vkey(1, 1), 0, mbx_scatter_kernel<true, true>),
};
// (routes 3 and 4: uniform stateless batches of at most two arguments)
static const Variant<decltype(mbx_onesweep_kernel<0, false, false>)> kOnesweep[] = {
    MBX_ROW(vkey(0, 0, 0), 0, mbx_onesweep_kernel<0, false, false>),
    MBX_ROW(vkey(0, 0, 1), 0, mbx_onesweep_kernel<0, false, true>),
    MBX_ROW(vkey(0, 1, 0), 0, mbx_onesweep_kernel<0, true, false>),
    MBX_ROW(vkey(0, 1, 1), 0, mbx_onesweep_kernel<0, true, true>),
    MBX_ROW(vkey(1, 0, 0), 0, mbx_onesweep_kernel<1, false, false>),
    MBX_ROW(vkey(1, 0, 1), 0, mbx_onesweep_kernel<1, false, true>),
    MBX_ROW(vkey(1, 1, 0), 0, mbx_onesweep_kernel<1, true, false>),
    MBX_ROW(vkey(1, 1, 1), 0, mbx_onesweep_kernel<1, true, true>),
    MBX_ROW(vkey(2, 0, 0), 0, mbx_onesweep_kernel<2, false, false>),
    MBX_ROW(vkey(2, 0, 1), 0, mbx_onesweep_kernel<2, false, true>),
    MBX_ROW(vkey(2, 1, 0), 0, mbx_onesweep_kernel<2, true, false>),
    MBX_ROW(vkey(2, 1, 1), 0, mbx_onesweep_kernel<2, true, true>),
    MBX_ROW(vkey(3, 0, 0), 0, mbx_onesweep_kernel<3, false, false>),
    MBX_ROW(vkey(4, 0, 0), ((onesweep_lds_bytes(kMboxSortMaxShards) + 15) & ~(size_t)15) + kPresLdsMax,
            mbx_onesweep_kernel<4, false, false>),
};
// (the persistent form serves stateless views only: at most kStatelessShards shards)
static const Variant<decltype(mbx_persist_sort_kernel<>)> kPersist[] = {
    MBX_ROW(vkey(), ((persist_lds_bytes(kStatelessShards) + 15) & ~(size_t)15) + kPresLdsMax, mbx_persist_sort_kernel<>),
};
static const Variant<decltype(mbx_drain_msg_kernel<0>)> kDrainMsg[] = {
    MBX_ROW(vkey(0), 0, mbx_drain_msg_kernel<0>),
    MBX_ROW(vkey(1), 0, mbx_drain_msg_kernel<kCalculatorMultiply>),
};
// (its LDS stage is sized by the 8-shard view: the narrow form)
static const Variant<decltype(mbx_drain_ring_kernel<0, true, 0>)> kDrainRing[] = {
    MBX_ROW(vkey(0, 0), 0, mbx_drain_ring_kernel<0, true, 0>),
    MBX_ROW(vkey(0, 1), 0, mbx_drain_ring_kernel<0, true, 1>),
    MBX_ROW(vkey(0, 2), 0, mbx_drain_ring_kernel<0, true, 2>),
    MBX_ROW(vkey(1, 0), 0, mbx_drain_ring_kernel<kCalculatorMultiply, true, 0>),
    MBX_ROW(vkey(1, 1), 0, mbx_drain_ring_kernel<kCalculatorMultiply, true, 1>),
    MBX_ROW(vkey(1, 2), 0, mbx_drain_ring_kernel<kCalculatorMultiply, true, 2>),
};

static std::vector<VariantName> all_variants() {
  std::vector<VariantName> v;
  variant_names(kFamCount, kCount, v);
  variant_names(kFamScatter, kScatter, v);
  variant_names(kFamOnesweep, kOnesweep, v);
  variant_names(kFamPersist, kPersist, v);
  v.push_back({kFamPresence, vkey(), "mbx_presence_kernel<>"});
  variant_names(kFamDrainMsg, kDrainMsg, v);
  variant_names(kFamDrainRing, kDrainRing, v);
  mbx_fused_variants(v);
  mbx_fused_other_variants(v);
  mbx_ordered_variants(v);
  mbx_arrival_variants(v);
  return v;
}
std::vector<std::string> mailbox_variant_names() {
  std::vector<std::string> out;
  for (const VariantName& n : all_variants()) out.push_back(n.name);
  return out;
}
std::vector<std::string> mailbox_plan_kernels(const SortPlan& p) {
  static const std::vector<VariantName> all = all_variants();
  std::vector<std::string> out;
  int found[kMbxFamilies] = {};
  for (const VariantName& n : all)
    if (p.key[n.family] == n.key) out.push_back(n.name), ++found[n.family];
  for (int f = 0; f < kMbxFamilies; ++f)
    if (p.key[f] != kNoKernel && found[f] != 1)
      throw std::logic_error("mailbox send: the plan's key " + std::to_string(p.key[f]) + " of family " +
                             std::to_string(f) + " matches " + std::to_string(found[f]) + " variants");
  return out;
}

// ---------------------------------------------------------------- host
// The persistent sort's grid: the blocks the device keeps resident at this LDS size, at most
// one per tile, a multiple of 8 from 8 up (whole XCD rounds).  (The current device is the Send's.)
static uint32_t persist_grid(size_t lds, int64_t tiles) {
  thread_local int c_dev = -1, c_resident = 0;  // the last answer (a Send repeats its device and map size)
  thread_local size_t c_lds = 0;
  int dev = 0;
  PT_HIP_CHECK(hipGetDevice(&dev));
  if (dev != c_dev || lds != c_lds) {
    int cus = 0, per_cu = 0;
    PT_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    PT_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kPersist[0].fn, kST, lds));
    c_resident = std::max(per_cu, 1) * std::max(cus, 1);
    c_dev = dev, c_lds = lds;
  }
  int64_t g = std::min<int64_t>(c_resident, tiles);
  if (g >= 8) g -= g % 8;
  return (uint32_t)g;
}

uint32_t presence_words(uint32_t n_dir) { return n_dir <= kPresMax ? pres_words(n_dir) : 0u; }
void launch_presence(uintptr_t dir_rank, uint32_t n_dir, int rank, uintptr_t out, uintptr_t stream) {
  if (n_dir == 0 || n_dir > kPresMax || !dir_rank || !out) throw std::invalid_argument("presence: 1 <= n_dir <= 2^18");
  const uint32_t nw = pres_words(n_dir);
  hipLaunchKernelGGL(mbx_presence_kernel<>, dim3((nw + 255) / 256), dim3(256), 0, as_stream(stream),
                     (const uint8_t*)dir_rank, n_dir, rank, (uint32_t*)out);
  PT_HIP_CHECK(hipGetLastError());
}

// A workspace is allocated or grown outside graph capture only.
static void no_capture(hipStream_t st, const char* what) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    throw std::runtime_error(std::string("mailbox send: ") + what + " inside a graph capture (warm up first)");
}

// Route mode 4's presence map of this Send's directory: the registry mirror's (rebuilt
// with the directory) when it is kept for this Send's rank, else folded here, every Send
// (the directory may have changed since the last one; 128 KB read for 131072 ids).
const uint32_t* Mailboxes::build_presence(const MboxSend& a, hipStream_t st) {
  if (a.pres && a.pres_rank == a.rank_self) return (const uint32_t*)a.pres;
  const uint32_t nw = pres_words(a.n_dir);
  if (nw > pres_words_) {
    no_capture(st, "first presence-map Send");
    PT_HIP_CHECK(hipStreamSynchronize(st));
    if (pres_) PT_HIP_CHECK(hipFree(pres_));
    PT_HIP_CHECK(hipMalloc((void**)&pres_, (size_t)nw * 4));
    pres_words_ = nw;
  }
  hipLaunchKernelGGL(mbx_presence_kernel<>, dim3((nw + 255) / 256), dim3(256), 0, st, (const uint8_t*)a.dir_rank,
                     a.n_dir, a.rank_self, pres_);
  PT_HIP_CHECK(hipGetLastError());
  return pres_;
}

// The workspaces sized by the batch, grown behind a stream sync; true when it synchronised.
bool Mailboxes::grow_workspaces(const SortPlan& p, const MboxSend& a, hipStream_t st) {
  const uint32_t S = shards();
  bool synced = false;
  // per-message workspace (route words, ring slots) and per-tile runs
  if (p.sort_cap > sort_cap_) {
    no_capture(st, "a larger batch than before");
    PT_HIP_CHECK(hipStreamSynchronize(st));
    for (void** w : {(void**)&sort_rw_, (void**)&sort_sidx_, (void**)&sort_tinfo_, (void**)&sort_desc_})
      if (*w) {
        PT_HIP_CHECK(hipFree(*w));
        *w = nullptr;
      }
    PT_HIP_CHECK(hipMalloc((void**)&sort_rw_, (size_t)p.sort_cap * 4));
    PT_HIP_CHECK(hipMalloc((void**)&sort_sidx_, (size_t)p.sort_cap * 4));
    PT_HIP_CHECK(hipMalloc((void**)&sort_tinfo_, (size_t)p.tiles * 2 * S * 4));
    // look-back descriptors: zero = no tag (every Send's tag is >= 1)
    PT_HIP_CHECK(hipMalloc((void**)&sort_desc_, (size_t)p.tiles * S * 8));
    PT_HIP_CHECK(hipMemsetAsync(sort_desc_, 0, (size_t)p.tiles * S * 8, st));
    PT_HIP_CHECK(hipStreamSynchronize(st));
    sort_cap_ = p.sort_cap;
    synced = true;
  }
  // 8-B records: the widths word and its pinned mirror, the per-tile field maxima
  if (p.r8 && (!r8w_ || r8_tiles_ < (uint64_t)p.tiles)) {
    no_capture(st, "first 8-B-record Send of this size");
    PT_HIP_CHECK(hipStreamSynchronize(st));
    if (!r8w_) {
      // the first Send's widths: the mailbox from the state size or the directory, the rest split
      const uint32_t nmb = std::max(a.n_state, a.n_dir);
      uint32_t wm = 20;
      if (nmb > 1) wm = 32u - (uint32_t)__builtin_clz(nmb - 1);
      wm = std::max(1u, std::min(wm, 24u));
      const uint32_t w0 = (52u - wm) / 2, w = wm | (w0 << 8) | ((52u - wm - w0) << 16);
      PT_HIP_CHECK(hipMalloc((void**)&r8w_, 16));
      PT_HIP_CHECK(hipMemcpy(r8w_, &w, 4, hipMemcpyHostToDevice));
      PT_HIP_CHECK(hipHostMalloc((void**)&r8host_, 64, hipHostMallocMapped));
      *r8host_ = w;
    }
    if (r8max_) PT_HIP_CHECK(hipFree(r8max_));
    PT_HIP_CHECK(hipMalloc((void**)&r8max_, (size_t)p.tiles * 4));
    r8_tiles_ = (uint64_t)p.tiles;
    synced = true;
  }
  return synced;
}

// The workspaces a kind of Send allocates once, sized by the rings.
void Mailboxes::first_use_workspaces(const SortPlan& p, hipStream_t st) {
  const uint64_t n = (uint64_t)shards() * slots();
  if (p.need_stage_rep && !stage_rep_) {
    no_capture(st, "first ordered Send");
    PT_HIP_CHECK(hipMalloc(&stage_rep_, n * 16));
    bytes_ += n * 16;
  }
  if (p.reserve && !sort_resv_) {
    no_capture(st, "first reserving Send");
    PT_HIP_CHECK(hipMalloc((void**)&sort_resv_, (size_t)kMboxSortMaxShards * kResvStride * 4));
    PT_HIP_CHECK(hipMemset(sort_resv_, 0, (size_t)kMboxSortMaxShards * kResvStride * 4));
  }
  if (p.need_r8esc && !r8esc_) {  // escape side array: {a0, mailbox} per ring slot
    no_capture(st, "first ordered 8-B-record Send");
    PT_HIP_CHECK(hipMalloc((void**)&r8esc_, n * 16));
    bytes_ += n * 16;
  }
}

SortWs Mailboxes::sort_ws() const {
  return SortWs{sort_hist_, sort_gsum_, sort_ticket_, sort_rw_, sort_sidx_, sort_tinfo_, sort_desc_,
                sort_tctr_, r8w_,       r8max_,       r8host_,  r8esc_,     stage_rep_};
}

void Mailboxes::send_sorted(const MboxSend& a) {
  const RingGeom g = geometry();
  if (!validate_sorted(a, g, started_ && running())) return;
  PT_HIP_CHECK(hipSetDevice(device_));
  hipStream_t st = as_stream(a.stream);
  const Tune tn = tune();
  SortPlan p = plan_sorted(a, tn, g, widths_overflowed());
  // (behind a stream sync the last Send's verdict on its 8-B widths has landed: read it again)
  if (grow_workspaces(p, a, st)) p = plan_sorted(a, tn, g, widths_overflowed());
  first_use_workspaces(p, st);
  last_plan_ = p;
  const SortWs ws = sort_ws();

  SortIn in{};
  in.actor = (const uint32_t*)a.actor;
  in.a0 = (const int64_t*)a.a0;
  in.a1 = (const int64_t*)a.a1;
  in.a2 = (const int64_t*)a.a2;
  in.mcol = (const uint16_t*)a.method_col;
  in.method_uniform = (uint32_t)a.method_uniform;
  in.M = a.M;
  in.table = (const TableEntry*)a.table;
  in.mask = a.cap - 1;
  in.dir = (const uint32_t*)a.dir;
  in.dirr = (const uint8_t*)a.dir_rank;
  in.n_dir = a.n_dir;
  in.aw = a.affine_w;
  in.aw_shift = (a.affine_w && (a.affine_w & (a.affine_w - 1)) == 0) ? __builtin_ctz(a.affine_w) : -1;
  in.rank_self = a.rank_self;
  in.origin_base = a.origin_base;
  in.tiles = (uint32_t)p.tiles;
  in.G = p.G;
  in.tpb = p.tpb;
  if (p.r8_on) {
    in.rec8 = 1;
    in.r8w = ws.r8w;
    in.r8max = ws.r8max;
    in.r8esc = ws.r8esc;
  } else if (p.rw_on) {
    in.recw = 1;
    in.r8w = ws.r8w;
    in.r8max = ws.r8max;
  }
  if (p.need_pres) in.pres = build_presence(a, st);
  HandlerArgs h{(int64_t*)a.state, a.n_state, a.delay_ticks, OutboxView{},
                ReplyView{(int64_t*)a.out_val, (int32_t*)a.out_st, a.out_n}};
  if (a.outbox_cap) {
    h.ob.actor = (uint32_t*)a.outbox[0];
    h.ob.a0 = (int64_t*)a.outbox[1];
    h.ob.a1 = (int64_t*)a.outbox[2];
    h.ob.a2 = (int64_t*)a.outbox[3];
    h.ob.method = (uint16_t*)a.outbox[4];
    h.ob.count = (unsigned long long*)a.outbox[5];
    h.ob.cap = a.outbox_cap;
  }
  MboxView mv = mv_;  // the plan's view of the rings (stateless batches: coarser)
  mv.log_s -= p.view_shift;
  mv.log_q += p.view_shift;
  if (p.reserve) mv.resv = sort_resv_;
  if (p.arrival) return mbx_launch_arrival(p, in, mv, ws, h, st);
  if (p.fused) return mbx_launch_fused(p, in, mv, ws, h, st);

  const uint32_t Sv = p.view_shards;
  uint32_t* tinfo = p.all_sidx ? nullptr : ws.tinfo;
  if (p.sort_mode == 2) {
    auto* count = variant(kCount, p.key[kFamCount]);
    hipLaunchKernelGGL(count, dim3(in.G), dim3(kST), 0, st, in, mv.log_s, ws.hist, ws.gsum, ws.rw);
    PT_HIP_CHECK(hipGetLastError());
    auto* scatter = variant(kScatter, p.key[kFamScatter]);
    hipLaunchKernelGGL(scatter, dim3(in.G), dim3(kST), scatter_lds_bytes(Sv), st, in, mv, (const uint32_t*)ws.hist,
                       (const uint32_t*)ws.gsum, ws.rw, ws.sidx, tinfo, h.rv, !a.ordered, p.all_sidx);
  } else {
    // route mode 4: the presence map behind the sort's own LDS
    const size_t map_lds = p.pres_route ? (size_t)pres_words(a.n_dir) * 4 : 0;
    if (p.pres_route) {
      variants_allow_lds(kOnesweep);
      variants_allow_lds(kPersist);
    }
    if (p.persist) {  // resident blocks walk the tiles
      const size_t lds = ((persist_lds_bytes(Sv) + 15) & ~(size_t)15) + map_lds;
      auto* sort = variant(kPersist, p.key[kFamPersist]);
      hipLaunchKernelGGL(sort, dim3(persist_grid(lds, p.tiles)), dim3(kST), lds, st, in, mv, ws.sidx, tinfo, ws.rw,
                         h.rv);
    } else {  // one block per tile, claimed in launch order (the grid is exactly the tile count)
      const size_t lds = p.pres_route ? ((onesweep_lds_bytes(Sv) + 15) & ~(size_t)15) + map_lds : onesweep_lds_bytes(Sv);
      auto* sweep = variant(kOnesweep, p.key[kFamOnesweep]);
      hipLaunchKernelGGL(sweep, dim3(in.tiles), dim3(kST), lds, st, in, mv, ws.desc, ws.tctr, ws.gsum, ws.sidx, tinfo,
                         ws.rw, h.rv, !a.ordered, p.all_sidx, p.reserve);
    }
  }
  PT_HIP_CHECK(hipGetLastError());
  if (a.ordered) {
    mbx_launch_ordered(p, in, mv, ws, h, st);
  } else if (p.msg_drain) {
    auto* drain = variant(kDrainMsg, p.key[kFamDrainMsg]);
    hipLaunchKernelGGL(drain, dim3(in.G), dim3(kST), 0, st, mv, in, (const uint32_t*)ws.sidx, (const uint32_t*)ws.rw,
                       h.state, h.n_state, h.delay_ticks, h.ob, h.rv, ws.gsum, p.ngroups, ws.ticket, ws.tctr);
  } else {
    auto* drain = variant(kDrainRing, p.key[kFamDrainRing]);
    hipLaunchKernelGGL(drain, dim3(p.tile_grid), dim3(kST), ring_drain_lds_bytes(Sv, kSTile), st, mv, in,
                       (const uint32_t*)ws.tinfo, (const uint32_t*)ws.sidx, (const uint32_t*)ws.rw, h.state, h.n_state,
                       h.delay_ticks, h.ob, h.rv, ws.gsum, p.ngroups, ws.ticket, ws.tctr, ws.r8host);
  }
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
