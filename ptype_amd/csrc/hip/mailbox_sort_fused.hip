// The fused one-pass sort + ring-order drain of a stateless mailbox Send, in two
// objects that build beside mailbox_sort.hip's: this one the directory routes
// (route modes 1 and 3, Join's default), mailbox_sort_fused_other.hip (which
// includes this file with PT_FUSED_OTHER_MODES) the hash-probe and affine ones.
// The kernel (mbx_sortdrain_kernel) shares the sort and the drain of a tile with the
// separate kernels (mailbox_sort_dev.hpp); design: mailbox_sort.hip.
#include "mailbox_sort_dev.hpp"

namespace ptype {

// ---------------------------------------------------------------- fused one-pass sort + ring-order drain
// Batches of stateless methods (the parallel drain): the block that sorts tile t
// into the rings drains tile t's runs right after -- the runs of a tile are
// exactly the records it wrote, so no other block's progress is needed, only a
// barrier between the block's stores and its ring-order reads (FRESH loads).
// The records still go through the rings (written, then read back in ring
// order by other lanes than wrote them), but the Send is one launch instead of
// two, the drain's reads are L2 hits of lines the sort just wrote, and no block
// waits at a kernel boundary for the slowest tile.  The last block to finish
// commits every shard's epoch (tail = head = tail + total) and advances the
// look-back tag.  Tune mbox_fused=0: the separate kernels.
template <int MODE, bool A2, bool MC, int FIXED, int RF, int SK = kSK>
__global__ __launch_bounds__(kST) void mbx_sortdrain_kernel(SortIn in, MboxView mv, unsigned long long* __restrict__ desc,
                                                            unsigned* __restrict__ tctr, uint32_t* __restrict__ gsum,
                                                            uint32_t* __restrict__ sidx, uint32_t* __restrict__ tinfo,
                                                            uint32_t* __restrict__ rw, ReplyView rv,
                                                            int64_t* __restrict__ state, uint32_t n_state,
                                                            uint64_t delay_ticks, OutboxView ob,
                                                            unsigned* __restrict__ ticket, bool reserve,
                                                            uint32_t* __restrict__ r8host) {
  extern __shared__ __align__(16) unsigned char smem_sd[];
  const uint32_t S = 1u << mv.log_s;
  const uint32_t t = onesweep_tile<MODE, A2, MC, SK>(in, mv, desc, tctr, gsum, sidx, tinfo, rw, rv, true, false,
                                                     smem_sd, reserve);
  // every wave's ring stores are out before any wave reads the tile's runs
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const DrainCounts dc = drain_ring_tile<FIXED, true, true, RF, SK>(mv, in, t, tinfo, sidx, rw, state, n_state,
                                                                    delay_ticks, ob, rv, smem_sd);
  block_add_stats(mv.stats, dc.done, kMbProcessed, dc.failed, kMbFailed, dc.holes, kMbHoles);
  __shared__ bool last;
  if (threadIdx.x == 0) {
    // the last tile's block wrote the epoch totals (gsum): release them before its ticket
    if (t == in.tiles - 1) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    last = last_block_ticket(ticket);
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (last) {  // every block's records are read: the rings are consumed
    // (reserve: the totals were built by memory-side atomics in this launch -- read and
    // cleared the same way, not through this XCD's L2)
    for (uint32_t s = threadIdx.x; s < S; s += kST)
      epoch_commit(mv, s, epoch_sum(mv, gsum, 1, S, s));
    if (threadIdx.x == 0) tctr[1] += 1u;  // the next Send's one-pass epoch tag
    if constexpr (RF != 0) rec8_next(in, const_cast<uint32_t*>(in.r8w), r8host, in.tiles);
  }
}

// Rows: route, a2, method column, fixed method, record form.  A method column fixes no method;
// 8-B records (form 1) take uniform batches of at most two arguments, wide pure records (form 2)
// rank routes only.
static const Variant<decltype(mbx_sortdrain_kernel<0, false, false, 0, 0>)> kSortdrain[] = {
#ifndef PT_FUSED_OTHER_MODES
    MBX_ROW(vkey(1, 0, 0, 0, 0), 0, mbx_sortdrain_kernel<1, false, false, 0, 0>),
    MBX_ROW(vkey(1, 0, 0, 0, 1), 0, mbx_sortdrain_kernel<1, false, false, 0, 1>),
    MBX_ROW(vkey(1, 0, 0, 1, 0), 0, mbx_sortdrain_kernel<1, false, false, kCalculatorMultiply, 0>),
    MBX_ROW(vkey(1, 0, 0, 1, 1), 0, mbx_sortdrain_kernel<1, false, false, kCalculatorMultiply, 1>),
    MBX_ROW(vkey(1, 0, 1, 0, 0), 0, mbx_sortdrain_kernel<1, false, true, 0, 0>),
    MBX_ROW(vkey(1, 1, 0, 0, 0), 0, mbx_sortdrain_kernel<1, true, false, 0, 0>),
    MBX_ROW(vkey(1, 1, 0, 1, 0), 0, mbx_sortdrain_kernel<1, true, false, kCalculatorMultiply, 0>),
    MBX_ROW(vkey(1, 1, 1, 0, 0), 0, mbx_sortdrain_kernel<1, true, true, 0, 0>),
    MBX_ROW(vkey(3, 0, 0, 0, 0), 0, mbx_sortdrain_kernel<3, false, false, 0, 0>),
    MBX_ROW(vkey(3, 0, 0, 0, 1), 0, mbx_sortdrain_kernel<3, false, false, 0, 1>),
    MBX_ROW(vkey(3, 0, 0, 0, 2), 0, mbx_sortdrain_kernel<3, false, false, 0, 2>),
    MBX_ROW(vkey(3, 0, 0, 1, 0), 0, mbx_sortdrain_kernel<3, false, false, kCalculatorMultiply, 0>),
    MBX_ROW(vkey(3, 0, 0, 1, 1), 0, mbx_sortdrain_kernel<3, false, false, kCalculatorMultiply, 1>),
    MBX_ROW(vkey(3, 0, 0, 1, 2), 0, mbx_sortdrain_kernel<3, false, false, kCalculatorMultiply, 2>),
#else
    MBX_ROW(vkey(0, 0, 0, 0, 0), 0, mbx_sortdrain_kernel<0, false, false, 0, 0>),
    MBX_ROW(vkey(0, 0, 0, 0, 1), 0, mbx_sortdrain_kernel<0, false, false, 0, 1>),
    MBX_ROW(vkey(0, 0, 0, 1, 0), 0, mbx_sortdrain_kernel<0, false, false, kCalculatorMultiply, 0>),
    MBX_ROW(vkey(0, 0, 0, 1, 1), 0, mbx_sortdrain_kernel<0, false, false, kCalculatorMultiply, 1>),
    MBX_ROW(vkey(0, 0, 1, 0, 0), 0, mbx_sortdrain_kernel<0, false, true, 0, 0>),
    MBX_ROW(vkey(0, 1, 0, 0, 0), 0, mbx_sortdrain_kernel<0, true, false, 0, 0>),
    MBX_ROW(vkey(0, 1, 0, 1, 0), 0, mbx_sortdrain_kernel<0, true, false, kCalculatorMultiply, 0>),
    MBX_ROW(vkey(0, 1, 1, 0, 0), 0, mbx_sortdrain_kernel<0, true, true, 0, 0>),
    MBX_ROW(vkey(2, 0, 0, 0, 0), 0, mbx_sortdrain_kernel<2, false, false, 0, 0>),
    MBX_ROW(vkey(2, 0, 0, 0, 1), 0, mbx_sortdrain_kernel<2, false, false, 0, 1>),
    MBX_ROW(vkey(2, 0, 0, 1, 0), 0, mbx_sortdrain_kernel<2, false, false, kCalculatorMultiply, 0>),
    MBX_ROW(vkey(2, 0, 0, 1, 1), 0, mbx_sortdrain_kernel<2, false, false, kCalculatorMultiply, 1>),
    MBX_ROW(vkey(2, 0, 1, 0, 0), 0, mbx_sortdrain_kernel<2, false, true, 0, 0>),
    MBX_ROW(vkey(2, 1, 0, 0, 0), 0, mbx_sortdrain_kernel<2, true, false, 0, 0>),
    MBX_ROW(vkey(2, 1, 0, 1, 0), 0, mbx_sortdrain_kernel<2, true, false, kCalculatorMultiply, 0>),
    MBX_ROW(vkey(2, 1, 1, 0, 0), 0, mbx_sortdrain_kernel<2, true, true, 0, 0>),
#endif
};

#ifndef PT_FUSED_OTHER_MODES
void mbx_fused_variants(std::vector<VariantName>& out) { variant_names(kFamSortdrain, kSortdrain, out); }
void mbx_launch_fused(const SortPlan& p, const SortIn& in, const MboxView& mv, const SortWs& ws, const HandlerArgs& h,
                      hipStream_t st) {
  if (p.route != 1 && p.route != 3) return mbx_launch_fused_other(p, in, mv, ws, h, st);
#else
void mbx_fused_other_variants(std::vector<VariantName>& out) { variant_names(kFamSortdrain, kSortdrain, out); }
void mbx_launch_fused_other(const SortPlan& p, const SortIn& in, const MboxView& mv, const SortWs& ws,
                            const HandlerArgs& h, hipStream_t st) {
#endif
  const size_t lds = std::max(onesweep_lds_bytes(p.view_shards), ring_drain_lds_bytes(p.view_shards, kSTile));
  auto* sortdrain = variant(kSortdrain, p.key[kFamSortdrain]);
  hipLaunchKernelGGL(sortdrain, dim3(in.tiles), dim3(kST), lds, st, in, mv, ws.desc, ws.tctr, ws.gsum, ws.sidx,
                     ws.tinfo, ws.rw, h.rv, h.state, h.n_state, h.delay_ticks, h.ob, ws.ticket, p.reserve, ws.r8host);
  PT_HIP_CHECK(hipGetLastError());
}

}  // namespace ptype
