// A mailbox Send on arrival rings (stateless batches: tile t's messages at fixed
// positions of ring t mod S, no sort): the fused enqueue + drain
// (mbx_arrival_fused_kernel) or the two kernels (mbx_arrival_enqueue_kernel,
// mbx_arrival_drain_kernel), in their own object.  It shares no launch with the
// sorted path.  Design: mailbox_sort.hip.
#include "mailbox_sort_dev.hpp"

namespace ptype {

// ---------------------------------------------------------------- arrival rings (fixed positions)
// Arrival sharding (batches without ordered methods): tile t's messages go to
// shard t & (S - 1), at ring offsets (t >> log S) * kSTile + (place in the
// tile) past the epoch's tail -- FIXED positions, so there is no count pass and
// no slot index: one enqueue pass resolves each message and writes its record
// (a tile is one contiguous 64 KB run of its ring: whole-line stores), and the
// drain reads the same positions in message order (whole-line loads, replies
// coalesced).  A message with no actor here leaves a zero record (its status is
// written by the enqueue); a tile whose run does not fit the ring's free room
// spills whole -- the drain runs it straight from the batch, re-resolving each
// message -- and tiles spill only as a suffix of a shard's sequence.
__device__ __forceinline__ bool arrival_fits(const MboxView& mv, const SortIn& in, uint32_t t, uint64_t& pos0,
                                             uint32_t tile = kSTile) {
  const uint32_t s = t & ((1u << mv.log_s) - 1);
  const uint64_t Q = 1ull << mv.log_q;
  const uint64_t tl = *ctr_tail(mv, s), hd = *ctr_head(mv, s);
  const uint64_t room = hd + Q > tl ? hd + Q - tl : 0;
  const uint64_t off = (uint64_t)(t >> mv.log_s) * tile;
  const uint64_t n_t = min((uint64_t)tile, (uint64_t)in.M - (uint64_t)t * tile);
  pos0 = tl + off;
  return off + n_t <= room;
}

template <int MODE, bool A2, bool MC>
__global__ __launch_bounds__(kST) void mbx_arrival_enqueue_kernel(SortIn in, MboxView mv, ReplyView rv) {
  unsigned long long n_enq = 0, n_miss = 0, n_spill = 0;
  const uint32_t t = virt_block(blockIdx.x, gridDim.x);
  if (t < in.tiles) {
    uint64_t pos0 = 0;
    const bool fits = arrival_fits(mv, in, t, pos0);
    const uint32_t s = t & ((1u << mv.log_s) - 1);
    uint32_t a[kSK], mb[kSK], meth[kSK];
    int64_t x0[kSK], x1[kSK], x2[kSK];
    int r[kSK];
#pragma unroll
    for (int k = 0; k < kSK; ++k) {
      const int64_t i = tile_index(t, k);
      const bool ok = i < in.M;
      a[k] = ok ? __builtin_nontemporal_load(in.actor + i) : 0xffffffffu;
      x0[k] = ok ? __builtin_nontemporal_load(in.a0 + i) : 0;
      x1[k] = ok && in.a1 ? __builtin_nontemporal_load(in.a1 + i) : 0;
      x2[k] = 0;
      if constexpr (A2) x2[k] = ok ? __builtin_nontemporal_load(in.a2 + i) : 0;
      meth[k] = in.method_uniform;
      if constexpr (MC) meth[k] = ok ? (uint32_t)in.mcol[i] : 0u;
    }
    resolve_k<MODE>(in, a, r, mb);
#pragma unroll
    for (int k = 0; k < kSK; ++k) {
      const int64_t i = tile_index(t, k);
      if (i >= in.M) continue;
      const uint32_t origin = in.origin_base + (uint32_t)i;
      const bool ok = r[k] == in.rank_self && mb[k] < kMaxMbox;
      const uint64_t slot = slot_at(mv, s, pos0 + (uint64_t)(i - (int64_t)t * kSTile));
      if (!ok) {
        ++n_miss;
        write_status(rv, origin, kStatusNoActor);
        if (fits) *reinterpret_cast<u32x4*>(rec_a(mv, slot)) = u32x4{0u, 0u, 0u, 0u};
        continue;
      }
      if (!fits) {
        ++n_spill;
        continue;
      }
      const uint32_t mt = meth[k];
      if (mt < 128u && fits_i32(x0[k]) && fits_i32(x1[k]) && x2[k] == 0) {
        *reinterpret_cast<u32x4*>(rec_a(mv, slot)) =
            u32x4{origin | kCompactMark, mb[k] | (mt << 24), (uint32_t)x0[k], (uint32_t)x1[k]};
      } else {
        const uint32_t fl = x2[k] != 0 ? (uint32_t)kFlagA2 : 0u;
        *reinterpret_cast<u32x4*>(rec_a(mv, slot)) =
            u32x4{origin | kCompactMark, mb[k] | kCompactLong, (mt & 0xffffu) | (fl << 16), 0u};
        *reinterpret_cast<u32x4*>(rec_b(mv, slot)) = u32x4{(uint32_t)x0[k], (uint32_t)((uint64_t)x0[k] >> 32),
                                                           (uint32_t)x1[k], (uint32_t)((uint64_t)x1[k] >> 32)};
        if (fl) mv.a2[slot] = x2[k];
      }
      ++n_enq;
    }
  }
  block_add_stats(mv.stats, n_enq, kMbEnqueued, n_miss, kMbNoActor, n_spill, kMbSpilled);
}

template <int FIXED, int MODE>
__global__ __launch_bounds__(kST) void mbx_arrival_drain_kernel(MboxView mv, SortIn in, int64_t* __restrict__ state,
                                                                uint32_t n_state, uint64_t delay_ticks, OutboxView ob,
                                                                ReplyView rv, unsigned* __restrict__ ticket) {
  unsigned long long done = 0, failed = 0;
  const uint32_t S = 1u << mv.log_s;
  const uint32_t t = virt_block(blockIdx.x, gridDim.x);
  if (t < in.tiles) {
    uint64_t pos0 = 0;
    const bool fits = arrival_fits(mv, in, t, pos0);
    const uint32_t s = t & (S - 1);
    SortRec x[kSK];
    if (fits) {
      u32x4 ha[kSK];
#pragma unroll
      for (int k = 0; k < kSK; ++k) {
        const int64_t i = tile_index(t, k);
        ha[k] = i < in.M ? *reinterpret_cast<const u32x4*>(rec_a(mv, slot_at(mv, s, pos0 + (uint64_t)(i - (int64_t)t * kSTile))))
                         : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int k = 0; k < kSK; ++k) {
        u32x4 hb = {0u, 0u, 0u, 0u};
        int64_t a2v = 0;
        if ((ha[k].x & kCompactMark) && rec_is_long(ha[k])) {
          const uint64_t slot = slot_at(mv, s, pos0 + (uint64_t)(tile_index(t, k) - (int64_t)t * kSTile));
          hb = *reinterpret_cast<const u32x4*>(rec_b(mv, slot));
          if (((ha[k].z >> 16) & kFlagA2) && mv.a2) a2v = mv.a2[slot];
        }
        x[k] = decode_sorted(ha[k], hb, a2v);  // a zero record (no actor): not valid
      }
    } else {  // the tile spilled: run it from the batch
      uint32_t a[kSK], mb[kSK];
      int r[kSK];
#pragma unroll
      for (int k = 0; k < kSK; ++k) {
        const int64_t i = tile_index(t, k);
        a[k] = i < in.M ? in.actor[i] : 0xffffffffu;
      }
      resolve_k<MODE>(in, a, r, mb);
#pragma unroll
      for (int k = 0; k < kSK; ++k) {
        const int64_t i = tile_index(t, k);
        x[k].valid = i < in.M && r[k] == in.rank_self && mb[k] < kMaxMbox;
        if (!x[k].valid) continue;
        x[k].mb = mb[k];
        x[k].method = in.mcol ? (uint32_t)in.mcol[i] : in.method_uniform;
        x[k].flags = 0;
        x[k].a0 = in.a0[i];
        x[k].a1 = in.a1 ? in.a1[i] : 0;
        x[k].a2 = in.a2 ? in.a2[i] : 0;
      }
    }
#pragma unroll
    for (int k = 0; k < kSK; ++k) {
      if (!x[k].valid) continue;  // no actor: answered by the enqueue
      MsgRecord m;
      m.actor = x[k].mb;
      m.method = (uint16_t)(FIXED ? FIXED : x[k].method);
      m.flags = (uint16_t)x[k].flags;
      m.a0 = x[k].a0, m.a1 = x[k].a1, m.a2 = x[k].a2;
      const ReplyRecord rr = run_handler(m, state, n_state, delay_ticks, ob);
      failed += rr.status != kStatusOk;
      write_reply(rv, in.origin_base + (uint32_t)tile_index(t, k), rr);
      ++done;
    }
  }
  block_add_stats(mv.stats, done, kMbProcessed, failed, kMbFailed, 0, -1);
  __shared__ bool last;
  if (threadIdx.x == 0) last = last_block_ticket(ticket);
  __syncthreads();
  if (last) {  // every tile is read: each shard consumed the positions of its tiles that fit
    for (uint32_t s = threadIdx.x; s < S; s += kST) {
      uint64_t used = 0;
      for (uint32_t tt = s; tt < in.tiles; tt += S) {
        uint64_t pos0 = 0;
        if (!arrival_fits(mv, in, tt, pos0)) break;  // the spilled suffix
        used += min((uint64_t)kSTile, (uint64_t)in.M - (uint64_t)tt * kSTile);
      }
      epoch_commit(mv, s, (uint32_t)used);
    }
  }
}

// Arrival rings, enqueue and drain in ONE launch.  Block t writes tile t's records
// into its run of ring t & (S - 1) (the positions mbx_arrival_enqueue_kernel uses) and,
// after a block barrier, drains that run: wave w consumes the records wave w ^ 4 wrote
// -- read back from the ring, decoded, its handler run -- so the ring is the hand-off
// between the block's waves, as it is between the two kernels of the general form (no
// grid-wide phase is needed: an arrival run belongs to one tile).  Uniform batches of at
// most two arguments; MODE 3 (rank byte routes, stateless methods) carries actor ids.
//
// Record format per WAVE (its producer decides with one ballot and tells its consumer
// through LDS, across the barrier the hand-off needs anyway; allow8 -- batches past 512
// tiles, the rule of the sort's 8-B records): 8 B {mailbox 24 | zigzag
// a0 20 | zigzag a1 20} when every message of the wave fits, in the first half of the
// wave's own 512 slots (message j in half j & 1 of slot j / 2 of that range: formats
// never overlap), else the 16-B compact form (32-B long form for a value past 32 bits).
constexpr int kArr8Mb = 24, kArr8Arg = 20;
constexpr uint64_t kArr8Null = ~0ull;  // a slot of no actor (mailbox 2^24 - 1 never fits the 8-B form)
__device__ __forceinline__ bool arr8_fits(uint32_t mb, int64_t x0, int64_t x1) {
  const uint64_t z0 = ((uint64_t)x0 << 1) ^ (uint64_t)(x0 >> 63), z1 = ((uint64_t)x1 << 1) ^ (uint64_t)(x1 >> 63);
  return mb < (1u << kArr8Mb) - 1u && (z0 >> kArr8Arg) == 0 && (z1 >> kArr8Arg) == 0;
}
template <int SK>
__device__ __forceinline__ uint64_t arr8_cell(const MboxView& mv, uint32_t s, uint64_t pos0, uint32_t j) {
  constexpr uint32_t run = SK * kWave;  // a wave's run of the tile
  return 2 * slot_at(mv, s, pos0 + (j & ~(run - 1)) + ((j & (run - 1)) >> 1)) + (j & 1);
}
// SK messages per thread: kSK (4096-message tiles), or 2 (1024) for batches of up to 512
// 4096-message tiles -- one 8-wave block per CU at 1 Mi messages hid too little latency
template <int MODE, int FIXED, int SK = kSK>
__global__ __launch_bounds__(kST) void mbx_arrival_fused_kernel(SortIn in, MboxView mv, int64_t* __restrict__ state,
                                                                uint32_t n_state, uint64_t delay_ticks, OutboxView ob,
                                                                ReplyView rv, unsigned* __restrict__ ticket,
                                                                bool allow8) {
  __shared__ uint32_t wave_rec8[kST / kWave];
  extern __shared__ __align__(16) unsigned char smem_af[];  // MODE 4: the presence map
  uint32_t* lpres = reinterpret_cast<uint32_t*>(smem_af);
  if constexpr (MODE == 4) {
    stage_pres(in, lpres);
    __syncthreads();
  }
  unsigned long long n_enq = 0, n_miss = 0, n_spill = 0, done = 0, failed = 0;
  const uint32_t S = 1u << mv.log_s;
  const uint32_t t = virt_block(blockIdx.x, gridDim.x);
  const unsigned w = threadIdx.x / kWave;
  if (t < in.tiles) {
    uint64_t pos0 = 0;
    constexpr uint32_t kTile = kST * SK;
    const bool fits = arrival_fits(mv, in, t, pos0, kTile);
    const uint32_t s = t & (S - 1);
    uint32_t a[SK], mb[SK];
    int64_t x0[SK], x1[SK];
    int r[SK];
#pragma unroll
    for (int k = 0; k < SK; ++k) {
      const int64_t i = tile_index<SK>(t, k);
      const bool ok = i < in.M;
      a[k] = ok ? __builtin_nontemporal_load(in.actor + i) : 0xffffffffu;
      x0[k] = ok ? __builtin_nontemporal_load(in.a0 + i) : 0;
      x1[k] = ok && in.a1 ? __builtin_nontemporal_load(in.a1 + i) : 0;
    }
    if constexpr (MODE == 4) resolve_pres<SK>(in, lpres, a, r, mb);
    else resolve_k<MODE, SK>(in, a, r, mb);
    bool live[SK];
    bool narrow = allow8 && mv.planar != 0;
#pragma unroll
    for (int k = 0; k < SK; ++k) {
      live[k] = tile_index<SK>(t, k) < in.M && r[k] == in.rank_self && mb[k] < kMaxMbox;
      if (live[k] && !arr8_fits(mb[k], x0[k], x1[k])) narrow = false;
    }
    const bool rec8 = __ballot(!narrow) == 0;  // (wave-uniform)
    if (lane_id() == 0) wave_rec8[w] = rec8;
    uint64_t* cells = reinterpret_cast<uint64_t*>(mv.rec);
#pragma unroll
    for (int k = 0; k < SK; ++k) {  // enqueue: the tile's records at their fixed ring positions
      const int64_t i = tile_index<SK>(t, k);
      if (i >= in.M) continue;
      const uint32_t origin = in.origin_base + (uint32_t)i;
      const uint32_t j = (uint32_t)(i - (int64_t)t * kTile);
      const uint64_t slot = slot_at(mv, s, pos0 + j);
      if (!live[k]) {
        ++n_miss;
        write_status(rv, origin, kStatusNoActor);
        if (fits && rec8) cells[arr8_cell<SK>(mv, s, pos0, j)] = kArr8Null;
        else if (fits) *reinterpret_cast<u32x4*>(rec_a(mv, slot)) = u32x4{0u, 0u, 0u, 0u};
        continue;
      }
      if (!fits) {  // the tile spilled: its messages run from the registers below
        ++n_spill;
        continue;
      }
      const uint32_t mt = in.method_uniform;
      if (rec8) {
        const uint64_t z0 = ((uint64_t)x0[k] << 1) ^ (uint64_t)(x0[k] >> 63);
        const uint64_t z1 = ((uint64_t)x1[k] << 1) ^ (uint64_t)(x1[k] >> 63);
        cells[arr8_cell<SK>(mv, s, pos0, j)] = (uint64_t)mb[k] | (z0 << kArr8Mb) | (z1 << (kArr8Mb + kArr8Arg));
      } else if (mt < 128u && fits_i32(x0[k]) && fits_i32(x1[k])) {
        *reinterpret_cast<u32x4*>(rec_a(mv, slot)) =
            u32x4{origin | kCompactMark, mb[k] | (mt << 24), (uint32_t)x0[k], (uint32_t)x1[k]};
      } else {
        *reinterpret_cast<u32x4*>(rec_a(mv, slot)) =
            u32x4{origin | kCompactMark, mb[k] | kCompactLong, mt & 0xffffu, 0u};
        *reinterpret_cast<u32x4*>(rec_b(mv, slot)) = u32x4{(uint32_t)x0[k], (uint32_t)((uint64_t)x0[k] >> 32),
                                                           (uint32_t)x1[k], (uint32_t)((uint64_t)x1[k] >> 32)};
      }
      ++n_enq;
    }
    __syncthreads();  // the run is in the ring: drain it
    const uint32_t w2 = w ^ 4u;  // (the wave whose records this one consumes)
    const bool rec8_2 = wave_rec8[w2] != 0;
#pragma unroll
    for (int k = 0; k < SK; ++k) {
      SortRec x;
      int64_t i;
      if (fits) {  // wave w2's k-th record of this lane
        const uint32_t j = w2 * (SK * kWave) + (uint32_t)k * kWave + lane_id();
        i = (int64_t)t * kTile + j;
        if (i >= in.M) continue;
        if (rec8_2) {
          const uint64_t c = cells[arr8_cell<SK>(mv, s, pos0, j)];
          if (c == kArr8Null) continue;  // no actor: answered by the enqueue
          x.valid = true, x.method = in.method_uniform, x.flags = 0, x.a2 = 0;
          x.mb = (uint32_t)(c & ((1u << kArr8Mb) - 1));
          const uint64_t z0 = (c >> kArr8Mb) & ((1ull << kArr8Arg) - 1), z1 = c >> (kArr8Mb + kArr8Arg);
          x.a0 = (int64_t)(z0 >> 1) ^ -(int64_t)(z0 & 1);
          x.a1 = (int64_t)(z1 >> 1) ^ -(int64_t)(z1 & 1);
        } else {
          const uint64_t slot = slot_at(mv, s, pos0 + j);
          const u32x4 ha = *reinterpret_cast<const u32x4*>(rec_a(mv, slot));
          const u32x4 hb = rec_is_long(ha) ? *reinterpret_cast<const u32x4*>(rec_b(mv, slot)) : u32x4{0u, 0u, 0u, 0u};
          x = decode_sorted(ha, hb, 0);  // a zero record (no actor): not valid
          if (!x.valid) continue;
        }
      } else {  // a spilled tile: this thread's own messages, from its registers
        if (!live[k]) continue;  // (no actor: answered above)
        i = tile_index<SK>(t, k);
        x.valid = true, x.mb = mb[k], x.method = in.method_uniform, x.flags = 0;
        x.a0 = x0[k], x.a1 = x1[k], x.a2 = 0;
      }
      MsgRecord m;
      m.actor = x.mb;
      m.method = (uint16_t)(FIXED ? FIXED : x.method);
      m.flags = (uint16_t)x.flags;
      m.a0 = x.a0, m.a1 = x.a1, m.a2 = 0;
      const ReplyRecord rr = run_handler(m, state, n_state, delay_ticks, ob);
      failed += rr.status != kStatusOk;
      write_reply(rv, in.origin_base + (uint32_t)i, rr);
      ++done;
    }
  }
  block_add_stats(mv.stats, n_enq, kMbEnqueued, n_miss, kMbNoActor, n_spill, kMbSpilled);
  __syncthreads();  // block_add_stats' LDS partials are reused
  block_add_stats(mv.stats, done, kMbProcessed, failed, kMbFailed, 0, -1);
  __shared__ bool last;
  if (threadIdx.x == 0) last = last_block_ticket(ticket);
  __syncthreads();
  if (last) {  // every tile is read: each shard consumed the positions of its tiles that fit
    for (uint32_t sh = threadIdx.x; sh < S; sh += kST) {
      uint64_t used = 0;
      for (uint32_t tt = sh; tt < in.tiles; tt += S) {
        uint64_t p0 = 0;
        if (!arrival_fits(mv, in, tt, p0, kST * SK)) break;  // the spilled suffix
        used += min((uint64_t)(kST * SK), (uint64_t)in.M - (uint64_t)tt * (kST * SK));
      }
      epoch_commit(mv, sh, (uint32_t)used);
    }
  }
}

// Rows: route, fixed method, 1024-message tiles (batches of up to 512 4096-message tiles).
// Route 4, the presence map in LDS, serves batches past 512 tiles only: it has no
// 1024-message form.
static const Variant<decltype(mbx_arrival_fused_kernel<0, 0>)> kArrFused[] = {
    MBX_ROW(vkey(0, 0, 1), 0, mbx_arrival_fused_kernel<0, 0, 2>),
    MBX_ROW(vkey(0, 0, 0), 0, mbx_arrival_fused_kernel<0, 0>),
    MBX_ROW(vkey(0, 1, 1), 0, mbx_arrival_fused_kernel<0, kCalculatorMultiply, 2>),
    MBX_ROW(vkey(0, 1, 0), 0, mbx_arrival_fused_kernel<0, kCalculatorMultiply>),
    MBX_ROW(vkey(1, 0, 1), 0, mbx_arrival_fused_kernel<1, 0, 2>),
    MBX_ROW(vkey(1, 0, 0), 0, mbx_arrival_fused_kernel<1, 0>),
    MBX_ROW(vkey(1, 1, 1), 0, mbx_arrival_fused_kernel<1, kCalculatorMultiply, 2>),
    MBX_ROW(vkey(1, 1, 0), 0, mbx_arrival_fused_kernel<1, kCalculatorMultiply>),
    MBX_ROW(vkey(2, 0, 1), 0, mbx_arrival_fused_kernel<2, 0, 2>),
    MBX_ROW(vkey(2, 0, 0), 0, mbx_arrival_fused_kernel<2, 0>),
    MBX_ROW(vkey(2, 1, 1), 0, mbx_arrival_fused_kernel<2, kCalculatorMultiply, 2>),
    MBX_ROW(vkey(2, 1, 0), 0, mbx_arrival_fused_kernel<2, kCalculatorMultiply>),
    MBX_ROW(vkey(3, 0, 1), 0, mbx_arrival_fused_kernel<3, 0, 2>),
    MBX_ROW(vkey(3, 0, 0), 0, mbx_arrival_fused_kernel<3, 0>),
    MBX_ROW(vkey(3, 1, 1), 0, mbx_arrival_fused_kernel<3, kCalculatorMultiply, 2>),
    MBX_ROW(vkey(3, 1, 0), 0, mbx_arrival_fused_kernel<3, kCalculatorMultiply>),
    MBX_ROW(vkey(4, 0, 0), kPresLdsMax, mbx_arrival_fused_kernel<4, 0>),
    MBX_ROW(vkey(4, 1, 0), kPresLdsMax, mbx_arrival_fused_kernel<4, kCalculatorMultiply>),
};
// Rows: mode, a2, method column
static const Variant<decltype(mbx_arrival_enqueue_kernel<0, false, false>)> kArrEnqueue[] = {
    MBX_ROW(vkey(0, 0, 0), 0, mbx_arrival_enqueue_kernel<0, false, false>),
    MBX_ROW(vkey(0, 0, 1), 0, mbx_arrival_enqueue_kernel<0, false, true>),
    MBX_ROW(vkey(0, 1, 0), 0, mbx_arrival_enqueue_kernel<0, true, false>),
    MBX_ROW(vkey(0, 1, 1), 0, mbx_arrival_enqueue_kernel<0, true, true>),
    MBX_ROW(vkey(1, 0, 0), 0, mbx_arrival_enqueue_kernel<1, false, false>),
    MBX_ROW(vkey(1, 0, 1), 0, mbx_arrival_enqueue_kernel<1, false, true>),
    MBX_ROW(vkey(1, 1, 0), 0, mbx_arrival_enqueue_kernel<1, true, false>),
    MBX_ROW(vkey(1, 1, 1), 0, mbx_arrival_enqueue_kernel<1, true, true>),
    MBX_ROW(vkey(2, 0, 0), 0, mbx_arrival_enqueue_kernel<2, false, false>),
    MBX_ROW(vkey(2, 0, 1), 0, mbx_arrival_enqueue_kernel<2, false, true>),
    MBX_ROW(vkey(2, 1, 0), 0, mbx_arrival_enqueue_kernel<2, true, false>),
    MBX_ROW(vkey(2, 1, 1), 0, mbx_arrival_enqueue_kernel<2, true, true>),
};
// Rows: fixed method, mode
static const Variant<decltype(mbx_arrival_drain_kernel<0, 0>)> kArrDrain[] = {
    MBX_ROW(vkey(0, 0), 0, mbx_arrival_drain_kernel<0, 0>),
    MBX_ROW(vkey(0, 1), 0, mbx_arrival_drain_kernel<0, 1>),
    MBX_ROW(vkey(0, 2), 0, mbx_arrival_drain_kernel<0, 2>),
    MBX_ROW(vkey(1, 0), 0, mbx_arrival_drain_kernel<kCalculatorMultiply, 0>),
    MBX_ROW(vkey(1, 1), 0, mbx_arrival_drain_kernel<kCalculatorMultiply, 1>),
    MBX_ROW(vkey(1, 2), 0, mbx_arrival_drain_kernel<kCalculatorMultiply, 2>),
};

void mbx_arrival_variants(std::vector<VariantName>& out) {
  variant_names(kFamArrFused, kArrFused, out);
  variant_names(kFamArrEnqueue, kArrEnqueue, out);
  variant_names(kFamArrDrain, kArrDrain, out);
}

void mbx_launch_arrival(const SortPlan& p, const SortIn& in, const MboxView& mv, const SortWs& ws,
                        const HandlerArgs& h, hipStream_t st) {
  if (p.arr_fused) {
    if (p.pres_arr) variants_allow_lds(kArrFused);
    SortIn in1 = in;
    in1.tiles = p.arr_tiles;
    auto* fused = variant(kArrFused, p.key[kFamArrFused]);
    hipLaunchKernelGGL(fused, dim3(p.arr_grid), dim3(kST), p.pres_arr ? (size_t)pres_words(in.n_dir) * 4 : 0, st, in1,
                       mv, h.state, h.n_state, h.delay_ticks, h.ob, h.rv, ws.ticket, p.allow8);
  } else {
    auto* enqueue = variant(kArrEnqueue, p.key[kFamArrEnqueue]);
    hipLaunchKernelGGL(enqueue, dim3(p.tile_grid), dim3(kST), 0, st, in, mv, h.rv);
    PT_HIP_CHECK(hipGetLastError());
    auto* drain = variant(kArrDrain, p.key[kFamArrDrain]);
    hipLaunchKernelGGL(drain, dim3(p.tile_grid), dim3(kST), 0, st, mv, in, h.state, h.n_state, h.delay_ticks, h.ob,
                       h.rv, ws.ticket);
  }
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
