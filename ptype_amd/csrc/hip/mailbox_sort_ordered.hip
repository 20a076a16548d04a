// The ordered drain of a mailbox Send (mbx_drain_ordered_kernel), the next
// Send's 8-B widths behind it (mbx_rec8_next_kernel) and the ring-order
// completion (mbx_complete_ring_kernel): their own object, the variants build
// beside mailbox_sort.hip's.  Design: mailbox_sort.hip.
#include "mailbox_sort_dev.hpp"

namespace ptype {

namespace {
constexpr int kOrdThreads = 512;  // ordered drain: one block per shard, one bin per thread
constexpr int kOrdK = 4;
constexpr int kOrdWin = kOrdThreads * kOrdK;  // records per window (2048)
constexpr int kOrdWaves = kOrdThreads / kWave;
constexpr uint32_t kOrdStateMax = 4096;  // a shard's actors whose state is staged in LDS (32 KB)
}  // namespace

// ---------------------------------------------------------------- K3s ordered drain
// One block owns shard s: its actors' state is staged in LDS (when it fits), and
// the shard's records are taken in windows of kOrdWin in ring order.  A window
// is sorted stably in LDS into kOrdThreads bins by actor (bin = local actor index
// mod bins), then thread b runs bin b's records one at a time in ring order: an
// actor's messages run serially and in FIFO order, distinct bins in parallel.
// Every method of the shard runs here (so a batch mixing ordered and other
// methods keeps per-actor FIFO across all of them).  Replies are staged at the
// records' ring slots (a window's slots are contiguous: whole lines), and
// mbx_complete_kernel gathers them into message order.
// A12: the batch carries a second / third argument column.  Without them (a
// one-argument ordered method, e.g. SeqFold) the window's a1 / a2 arrays are not
// allocated: 68 instead of 100 KB of LDS, so two drain blocks fit a CU.
template <bool A12, int OK = kOrdK>
struct OrdLds {
  static constexpr int kWin = kOrdThreads * OK;
  uint32_t wcnt[kOrdWaves][kOrdThreads];  // per-wave bin counts -> offsets
  uint32_t bstart[kOrdThreads];
  uint32_t bcount[kOrdThreads];
  uint32_t wsum[kOrdWaves];
  uint32_t slot[kWin];
  uint32_t act[kWin];  // actor index for the handler (LDS-local or global mailbox)
  uint32_t meth[kWin];  // method | flags << 16
  uint32_t orig[kWin];  // origin: the completion's place for the reply
  int64_t a0[kWin], a1[A12 ? kWin : 2], a2[A12 ? kWin : 2];
};

// OK: records per thread per window (window = 512 * OK records: OK = 8 for one-argument batches).
// FIXED = kSeqFold: a uniform SeqFold batch.  With every actor of the shard in its
// own bin (at most kOrdThreads of them, state staged), thread b IS actor b's
// consumer for the whole Send: its state stays in a register and each record is
// one fold (reply = the state before, state = state * kFoldMul + a0) -- no handler
// switch, no LDS state round trip per message.
// R8: the sort wrote 8-B records (a uniform one-argument batch): each carries its
// place in its tile (12 bits), the mailbox and the zigzag argument at the widths
// *r8w; mbx_rec8_next_kernel derives the next Send's widths after the drain.
struct R8Args {
  const uint32_t* r8w = nullptr;  // this Send's widths (the sort's)
  uint32_t method = 0;            // the batch's uniform method
  const int64_t* esc = nullptr;   // escape records' {a0, mailbox}, by ring slot (SortIn::r8esc)
};
__device__ __forceinline__ SortRec decode_rec8_ord(uint64_t r, uint32_t w8, uint32_t method, const int64_t* esc,
                                                   uint64_t slot) {
  const uint32_t wm = w8 & 0xffu, w0 = (w8 >> 8) & 0xffu, w1 = (w8 >> 16) & 0xffu;
  SortRec x;
  x.valid = true;
  x.origin = (uint32_t)(r & (kSTile - 1));  // the place in the tile
  x.method = method;
  x.flags = 0;
  x.a2 = 0;
  if (r >> 63) {  // escape record (one-argument batches leave the top bit of a record zero)
    const u32x4 e = *reinterpret_cast<const u32x4*>(esc + 2 * slot);
    x.a0 = (int64_t)(((uint64_t)e.y << 32) | e.x);
    x.mb = e.z;
    x.a1 = 0;
    return x;
  }
  x.mb = (uint32_t)((r >> 12) & ((1ull << wm) - 1));
  const uint64_t z0 = (r >> (12 + wm)) & ((1ull << w0) - 1), z1 = (r >> (12 + wm + w0)) & ((1ull << w1) - 1);
  x.a0 = (int64_t)(z0 >> 1) ^ -(int64_t)(z0 & 1);
  x.a1 = (int64_t)(z1 >> 1) ^ -(int64_t)(z1 & 1);
  return x;
}

// A window's records (their first 16 B; R8: the 8-B record), wave w's positions.
template <bool R8, int OK>
__device__ __forceinline__ void ord_load_win(const MboxView& mv, uint64_t wa, uint64_t n_end, uint64_t sbase,
                                             uint64_t rot, uint64_t qmask, unsigned w, unsigned lane,
                                             typename std::conditional<R8, uint64_t, u32x4>::type (&h)[OK]) {
#pragma unroll
  for (int k = 0; k < OK; ++k) {
    const uint64_t q = wa + (uint64_t)w * (kWave * OK) + (uint64_t)k * kWave + lane;
    const uint64_t sl = sbase | ((q + rot) & qmask);
    const bool in = q < n_end && q < wa + (kOrdThreads * OK);
    if constexpr (R8) h[k] = in ? reinterpret_cast<const uint64_t*>(mv.rec)[sl] : 0ull;
    else h[k] = in ? *reinterpret_cast<const u32x4*>(rec_a(mv, sl)) : u32x4{0u, 0u, 0u, 0u};
  }
}

// (one block per CU whatever its registers -- the window's LDS -- so the register
// budget is that of 2 waves per SIMD: no spill for the prefetched window)
template <bool A12, int OK = kOrdK, int FIXED = 0, bool PF = false, bool R8 = false>
__global__ __launch_bounds__(kOrdThreads) __attribute__((amdgpu_waves_per_eu(1, 2))) void mbx_drain_ordered_kernel(MboxView mv, uint32_t* __restrict__ gsum,
                                                                        uint32_t ngroups, int64_t* __restrict__ state,
                                                                        uint32_t n_state, uint64_t delay_ticks,
                                                                        OutboxView ob, u32x4* __restrict__ srep,
                                                                        uint32_t origin_base, R8Args r8) {
  extern __shared__ __align__(16) unsigned char smem_ord[];
  OrdLds<A12, OK>& L = *reinterpret_cast<OrdLds<A12, OK>*>(smem_ord);
  int64_t* st_lds = reinterpret_cast<int64_t*>(smem_ord + sizeof(OrdLds<A12, OK>));
  const uint32_t s = blockIdx.x;
  const uint32_t S = 1u << mv.log_s;
  const uint64_t Q = 1ull << mv.log_q;
  const unsigned w = threadIdx.x / kWave, lane = lane_id();
  __shared__ uint32_t tot_s;
  if (threadIdx.x == 0) tot_s = epoch_total(gsum, ngroups, S, s, true);
  const uint64_t lo = *ctr_tail(mv, s), hd = *ctr_head(mv, s);
  const uint64_t free = hd + Q > lo ? hd + Q - lo : 0;
  // this shard's actors are mailboxes s, s + S, s + 2S, ...: local index j = mb >> log_s
  const uint32_t n_loc = (state && s < n_state) ? (n_state - 1 - s) / S + 1 : 0;
  const bool in_lds = state && n_loc <= kOrdStateMax;
  if (in_lds)
    for (uint32_t j = threadIdx.x; j < n_loc; j += kOrdThreads) st_lds[j] = state[s + (uint64_t)j * S];
  __syncthreads();
  const bool reg = FIXED == kSeqFold && in_lds && n_loc <= (uint32_t)kOrdThreads;  // actor b's state in thread b
  uint64_t sreg = reg && threadIdx.x < n_loc ? (uint64_t)st_lds[threadIdx.x] : 0ull;
  const uint32_t tot = tot_s;
  const uint64_t n = tot < free ? tot : free;
  const uint64_t sbase = (uint64_t)s << mv.log_q, qmask = Q - 1, rot = shard_rot(mv, s);  // slot_at, hoisted
  unsigned long long done = 0, failed = 0, holes = 0, serial = 0;
  // PF (the fold: the next window's records (their first 16 B) are loaded
  // while this one is binned and run -- one block per CU (the LDS), so the registers are
  // there.  (Round 3, with the handler switch's register file: measured no faster, 188 ->
  // 200 us, and spilled to scratch.)
  const uint64_t n_end = lo + n;
  using RawT = typename std::conditional<R8, uint64_t, u32x4>::type;  // a record's first (R8: only) word
  const uint32_t w8 = R8 ? *r8.r8w : 0u;
  RawT cur[PF ? OK : 1];
  if constexpr (PF) {
    if (lo < n_end) ord_load_win<R8, OK>(mv, lo, n_end, sbase, rot, qmask, w, lane, cur);
  }
  for (uint64_t w0 = lo; w0 < lo + n; w0 += (kOrdThreads * OK)) {
    const uint64_t w1 = lo + n < w0 + (kOrdThreads * OK) ? lo + n : w0 + (kOrdThreads * OK);
    for (uint32_t b = lane; b < kOrdThreads; b += kWave) L.wcnt[w][b] = 0;
    SortRec x[OK];
    uint32_t bin[OK], wr[OK];
    uint64_t slot[OK];
    RawT nxt[PF ? OK : 1];
    if constexpr (PF) {
      if (w0 + (kOrdThreads * OK) < n_end)
        ord_load_win<R8, OK>(mv, w0 + (kOrdThreads * OK), n_end, sbase, rot, qmask, w, lane, nxt);
    }
#pragma unroll
    for (int k = 0; k < OK; ++k) {  // wave w owns window positions [w * 64K, (w+1) * 64K)
      const uint64_t q = w0 + (uint64_t)w * (kWave * OK) + (uint64_t)k * kWave + lane;
      slot[k] = sbase | ((q + rot) & qmask);
      if (q < w1) {
        if constexpr (R8) {
          x[k] = decode_rec8_ord(PF ? (uint64_t)cur[k] : reinterpret_cast<const uint64_t*>(mv.rec)[slot[k]], w8,
                                 r8.method, r8.esc, slot[k]);
        } else if constexpr (PF) {
          u32x4 hb = {0u, 0u, 0u, 0u};
          int64_t a2v = 0;
          if (rec_is_long(cur[k])) {
            hb = *reinterpret_cast<const u32x4*>(rec_b(mv, slot[k]));
            if (((cur[k].z >> 16) & kFlagA2) && mv.a2) a2v = mv.a2[slot[k]];
          }
          x[k] = decode_sorted(cur[k], hb, a2v);
        } else {
          x[k] = load_sorted(mv, slot[k]);
        }
        if (!x[k].valid) ++holes;
      } else {
        x[k].valid = false;
      }
    }
    if constexpr (PF) {
#pragma unroll
      for (int k = 0; k < OK; ++k) cur[k] = nxt[k];
    }
#pragma unroll
    for (int k = 0; k < OK; ++k) {
      bin[k] = (x[k].mb >> mv.log_s) & (kOrdThreads - 1);
      const uint64_t peers = match_bits(bin[k], 9, __ballot(x[k].valid));
      const unsigned below = mbcnt64(peers);
      const int leader = peers ? __builtin_ctzll(peers) : 0;
      unsigned old = 0;
      if (x[k].valid && below == 0) {
        old = L.wcnt[w][bin[k]];
        L.wcnt[w][bin[k]] = old + (unsigned)__popcll(peers);
      }
      wr[k] = (unsigned)__shfl((int)old, leader) + below;
    }
    __syncthreads();
    {  // bin totals and wave offsets (thread b owns bin b), then an exclusive scan over bins
      const unsigned b = threadIdx.x;
      unsigned r = 0;
#pragma unroll
      for (int ww = 0; ww < kOrdWaves; ++ww) {
        const unsigned c = L.wcnt[ww][b];
        L.wcnt[ww][b] = r;
        r += c;
      }
      L.bcount[b] = r;
      const unsigned inc = wave_incl_scan(r);
      if (lane == kWave - 1) L.wsum[w] = inc;
      __syncthreads();
      unsigned off = inc - r;
      for (unsigned ww = 0; ww < w; ++ww) off += L.wsum[ww];
      L.bstart[b] = off;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < OK; ++k) {
      if (!x[k].valid) continue;
      const unsigned d = L.bstart[bin[k]] + L.wcnt[w][bin[k]] + wr[k];
      L.slot[d] = (uint32_t)slot[k];
      L.act[d] = in_lds ? (x[k].mb >> mv.log_s) : x[k].mb;
      if (!reg) L.meth[d] = x[k].method | (x[k].flags << 16);
      // the message's place in its tile (the completion reads the tile's runs)
      L.orig[d] = R8 ? x[k].origin : ((x[k].origin - origin_base) & (uint32_t)(kSTile - 1));
      L.a0[d] = x[k].a0;
      if constexpr (A12) {
        L.a1[d] = x[k].a1;
        L.a2[d] = x[k].a2;
      }
    }
    __syncthreads();
    if (reg) {  // uniform SeqFold, one actor per bin: the folds in a register
      const unsigned b = threadIdx.x, e = L.bstart[b] + L.bcount[b];
      if (L.bcount[b] > 1) serial += L.bcount[b] - 1;
      for (unsigned d = L.bstart[b]; d < e; ++d) {
        const uint64_t prev = sreg;
        uint32_t st = kStatusOk;
        if (L.act[d] == b && b < n_loc) {
          sreg = prev * kFoldMul + (uint64_t)L.a0[d];
        } else {  // a mailbox past the state (routed here by a stale registry entry)
          st = kStatusNoActor;
          ++failed;
        }
        const uint64_t v = st == kStatusOk ? prev : 0ull;
        srep[L.slot[d]] = u32x4{(uint32_t)v, (uint32_t)(v >> 32), st, L.orig[d]};
        ++done;
      }
    } else {  // this thread's bin, serially in ring order
      const unsigned b = threadIdx.x, e = L.bstart[b] + L.bcount[b];
      if (L.bcount[b] > 1) serial += L.bcount[b] - 1;  // records that waited behind their bin's earlier ones
      int64_t* st = in_lds ? st_lds : state;
      const uint32_t nst = in_lds ? n_loc : n_state;
      for (unsigned d = L.bstart[b]; d < e; ++d) {
        MsgRecord m;
        m.actor = L.act[d];
        m.method = (uint16_t)(L.meth[d] & 0xffffu);
        m.flags = (uint16_t)(L.meth[d] >> 16);
        m.a0 = L.a0[d];
        m.a1 = A12 ? L.a1[d] : 0;
        m.a2 = A12 ? L.a2[d] : 0;
        const ReplyRecord rr = run_handler(m, st, nst, delay_ticks, ob, true);
        failed += rr.status != kStatusOk;
        srep[L.slot[d]] = u32x4{(uint32_t)rr.value, (uint32_t)((uint64_t)rr.value >> 32), (uint32_t)rr.status, L.orig[d]};
        ++done;
        if (!in_lds) vm_drain();  // global state: this store lands before the bin's next load
      }
    }
    __syncthreads();  // the window's LDS is reused
  }
  if (reg && threadIdx.x < n_loc) st_lds[threadIdx.x] = (int64_t)sreg;
  if (reg) __syncthreads();
  if (in_lds)
    for (uint32_t j = threadIdx.x; j < n_loc; j += kOrdThreads) state[s + (uint64_t)j * S] = st_lds[j];
  block_add_stats(mv.stats, done, kMbProcessed, failed, kMbFailed, holes, kMbHoles);
  __syncthreads();  // block_add_stats' LDS partials are reused
  block_add_stats(mv.stats, serial, kMbSerial, 0, -1, 0, -1);
  if (threadIdx.x == 0) epoch_commit(mv, s, tot);
}

// The next Send's 8-B field widths after an ordered 8-B-record Send (one block, launched
// after the ordered drain: every block of it has decoded with this Send's widths).
template <int = 0>  // (a template, like every kernel of the sorted mailboxes)
__global__ __launch_bounds__(256) void mbx_rec8_next_kernel(const uint32_t* __restrict__ r8max,
                                                            uint32_t* __restrict__ r8w, uint32_t* __restrict__ host,
                                                            uint32_t tiles) {
  rec8_next_from(r8max, r8w, host, tiles);
}

template <int = 0>
__global__ __launch_bounds__(kST) void mbx_complete_ring_kernel(SortIn in, MboxView mv,
                                                                const uint32_t* __restrict__ tinfo,
                                                                const u32x4* __restrict__ srep, ReplyView rv,
                                                                unsigned* __restrict__ tctr) {
  extern __shared__ __align__(16) unsigned char smem_cr[];
  if (blockIdx.x == 0 && threadIdx.x == 0) tctr[1] += 1u;  // the next Send's one-pass epoch tag (the sort is done)
  const uint32_t S = 1u << mv.log_s;
  int64_t* sval = reinterpret_cast<int64_t*>(smem_cr);
  RunLds<uint16_t> L;
  L.bias = reinterpret_cast<uint32_t*>(sval + kSTile);
  L.excl = L.bias + S;
  L.owner = reinterpret_cast<uint16_t*>(L.excl + S);
  uint8_t* sst = reinterpret_cast<uint8_t*>(L.owner + kSTile);
  const uint32_t t = virt_block(blockIdx.x, gridDim.x);
  if (t >= in.tiles) return;
  const uint64_t i0 = (uint64_t)t * kSTile;
  const uint32_t n_t = (uint32_t)min((uint64_t)kSTile, (uint64_t)in.M - i0);
  for (uint32_t j = threadIdx.x; j < kSTile; j += kST) sst[j] = kAbsent;
  int spill = 0;
  const uint32_t T = load_tile_runs(mv, tinfo, t, L, spill);
  const uint64_t qmask = (1ull << mv.log_q) - 1;
  u32x4 r[kSK];
#pragma unroll
  for (int k = 0; k < kSK; ++k) {
    const uint32_t j = (uint32_t)k * kST + threadIdx.x;
    if (j < T) {
      const uint32_t s = L.owner[j];
      // (read once: non-temporal -- SeqFold 25.64-25.87 vs 25.22-25.57 G and 25.74-25.85 vs
      // 25.35-25.52 G in two sessions, alternated; profiles/r6_small_sends.md)
      r[k] = __builtin_nontemporal_load(srep + (((uint64_t)s << mv.log_q) | ((L.bias[s] + j) & qmask)));
    } else {
      r[k] = u32x4{0u, 0u, 0u, 0xffffffffu};
    }
  }
#pragma unroll
  for (int k = 0; k < kSK; ++k) {
    const uint32_t local = r[k].w;  // the place in the tile (the drains write it; 0xffffffff: none)
    if (local < n_t) {
      sval[local] = (int64_t)(((uint64_t)r[k].y << 32) | r[k].x);
      sst[local] = (uint8_t)r[k].z;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kSK; ++k) {
    const uint32_t j = (uint32_t)k * kST + threadIdx.x;
    if (j < n_t && sst[j] != kAbsent) put_reply(rv, in.origin_base + (uint32_t)(i0 + j), sval[j], sst[j]);
  }
}

// Rows: a1 / a2 staged, register fold, 8-B records.  One-argument batches: 4096-record windows,
// and a uniform SeqFold batch folds in registers with the next window prefetched; two- and
// three-argument batches: 2048-record windows, the handler switch.  Every row may stage a
// shard's state behind its window (above the 64 KB default dynamic LDS).
template <bool A12, int OKV>
constexpr size_t ord_lds_max() {
  return sizeof(OrdLds<A12, OKV>) + (size_t)kOrdStateMax * sizeof(int64_t);
}
static const Variant<decltype(mbx_drain_ordered_kernel<false, 8, 0, false, false>)> kOrdered[] = {
    MBX_ROW(vkey(0, 0, 0), (ord_lds_max<false, 8>()), mbx_drain_ordered_kernel<false, 8, 0, false, false>),
    MBX_ROW(vkey(0, 1, 0), (ord_lds_max<false, 8>()), mbx_drain_ordered_kernel<false, 8, kSeqFold, true, false>),
    MBX_ROW(vkey(0, 0, 1), (ord_lds_max<false, 8>()), mbx_drain_ordered_kernel<false, 8, 0, false, true>),
    MBX_ROW(vkey(0, 1, 1), (ord_lds_max<false, 8>()), mbx_drain_ordered_kernel<false, 8, kSeqFold, true, true>),
    MBX_ROW(vkey(1, 0, 0), (ord_lds_max<true, kOrdK>()), mbx_drain_ordered_kernel<true, kOrdK, 0, false, false>),
};

void mbx_ordered_variants(std::vector<VariantName>& out) {
  variant_names(kFamOrdered, kOrdered, out);
  out.push_back({kFamRec8Next, vkey(), "mbx_rec8_next_kernel<>"});
  out.push_back({kFamCompleteRing, vkey(), "mbx_complete_ring_kernel<>"});
}

void mbx_launch_ordered(const SortPlan& p, const SortIn& in, const MboxView& mv, const SortWs& ws,
                        const HandlerArgs& h, hipStream_t st) {
  const uint32_t Sv = p.view_shards;
  // state staged per shard: what its actors need (mailboxes s, s + S, ...), not the cap
  const uint32_t n_loc = h.state && h.n_state ? std::min<uint32_t>((h.n_state + Sv - 1) / Sv, kOrdStateMax) : 0;
  const size_t st_lds = (size_t)n_loc * sizeof(int64_t);  // (covers every shard the kernel stages: n_loc <= cap)
  const size_t lds = (p.ord_a12 ? sizeof(OrdLds<true, kOrdK>) : sizeof(OrdLds<false, 8>)) + std::max<size_t>(st_lds, 16);
  R8Args r8a;
  if (p.r8_on) {
    r8a.r8w = ws.r8w;
    r8a.method = in.method_uniform;
    r8a.esc = ws.r8esc;
  }
  variants_allow_lds(kOrdered);
  auto* drain = variant(kOrdered, p.key[kFamOrdered]);
  hipLaunchKernelGGL(drain, dim3(Sv), dim3(kOrdThreads), lds, st, mv, ws.gsum, p.ngroups, h.state, h.n_state,
                     h.delay_ticks, h.ob, (u32x4*)ws.stage_rep, in.origin_base, r8a);
  if (p.r8_on)
    hipLaunchKernelGGL(mbx_rec8_next_kernel<>, dim3(1), dim3(256), 0, st, (const uint32_t*)ws.r8max, ws.r8w, ws.r8host,
                       in.tiles);
  PT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(mbx_complete_ring_kernel<>, dim3(p.tile_grid), dim3(kST),
                     (size_t)kSTile * (8 + 2 + 1) + (size_t)Sv * 8, st, in, mv, (const uint32_t*)ws.tinfo,
                     (const u32x4*)ws.stage_rep, h.rv, ws.tctr);
}

}  // namespace ptype
