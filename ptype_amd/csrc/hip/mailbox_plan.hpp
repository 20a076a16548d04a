// What one sorted mailbox Send will do, decided before anything is allocated or
// launched: the argument checks, and every choice among the sort, route, record
// and drain variants (design notes: mailbox_sort.hip).  Host code free of HIP, so
// the policy is testable without a GPU (_hip.mailbox_send_plan).
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "records.hpp"
#include "sort_limits.hpp"
#include "tune.hpp"

namespace ptype {

// One epoch Send through the sorted mailboxes (Mailboxes::send_sorted).
struct MboxSend {
  uintptr_t actor = 0, a0 = 0, a1 = 0, a2 = 0, method_col = 0;
  int method_uniform = 0;
  int64_t M = 0;
  uintptr_t table = 0;
  uint64_t cap = 0;
  uintptr_t dir = 0;
  uint32_t n_dir = 0, affine_w = 0;
  int rank_self = 0;
  uint32_t origin_base = 0;
  uintptr_t out_val = 0, out_st = 0;
  uint64_t out_n = 0;
  uintptr_t state = 0;
  uint32_t n_state = 0;
  uint64_t delay_ticks = 0;
  std::vector<uintptr_t> outbox;
  uint64_t outbox_cap = 0;
  bool arrival = false;  // shard by arrival tile (batches without ordered methods)
  bool ordered = true;   // ordered drain: per-actor serial, FIFO; else the parallel drain
  int fixed_method = 0;  // every message carries this method (constant-folded handler)
  // sort kernels: 0 auto (tune mbox_sort, else one-pass for stateless batches and from 1024
  // tiles on), 1 one-pass (stateless: run reservations; ordered: look-back), 2 count + scatter
  int sort_mode = 0;
  uintptr_t stream = 0;
  // the directory's rank byte table (one byte per id): a stateless uniform batch
  // resolves only its rank (1 MB at 1 M ids, L2-resident, against the 4 MB
  // directory) and its records carry the actor id, which no stateless handler reads
  uintptr_t dir_rank = 0;
  // route mode 4's presence map of the directory, kept by the registry mirror for
  // rank pres_rank (rebuilt with the directory; RegistryTable.presence): used when it is
  // this Send's rank, else the Send folds its own from dir_rank
  uintptr_t pres = 0;
  int pres_rank = -1;
};

// The rings a Send goes through, as far as the plan depends on them.
struct RingGeom {
  uint32_t log_s = 0, log_q = 0;
  bool planar = false;  // two record planes: 8-B cells can view plane A
  bool has_a2 = false;  // the a2 side array exists
};

// The kernel families of a sorted Send.  Every family with more than one
// instantiation has a variant table next to its launcher; a row's key packs the
// template arguments the table varies, in their order (vkey).
enum MbxFamily : int {
  kFamCount,         // mode
  kFamScatter,       // a2, method column
  kFamOnesweep,      // route 0..4, a2, method column
  kFamPersist,
  kFamPresence,
  kFamSortdrain,     // route 0..3, a2, method column, fixed method, record form
  kFamDrainMsg,      // fixed method
  kFamDrainRing,     // fixed method, record form
  kFamOrdered,       // a1 / a2 staged, register fold, 8-B records
  kFamRec8Next,
  kFamCompleteRing,
  kFamArrFused,      // route 0..4, fixed method, 1024-message tiles
  kFamArrEnqueue,    // mode, a2, method column
  kFamArrDrain,      // fixed method, mode
  kMbxFamilies
};
constexpr uint32_t kNoKernel = ~0u;
constexpr uint32_t kStatelessShards = 8;  // the ring view of a stateless Send
constexpr uint32_t vkey(uint32_t a = 0, uint32_t b = 0, uint32_t c = 0, uint32_t d = 0, uint32_t e = 0) {
  return a | b << 4 | c << 8 | d << 12 | e << 16;
}

struct SortPlan {
  int64_t tiles = 0;
  // count / scatter blocks: as many as the histogram holds (it stays L2-resident for the
  // prefixes), a multiple of 8 (one contiguous eighth of the batch per XCD); tiles per block
  uint32_t G = 0, tpb = 0;
  uint32_t tile_grid = 0;  // one block per tile, dealt XCD by XCD: a multiple of 8
  uint32_t ngroups = 1;    // group sums the drains add up (count + scatter only)
  int sort_mode = 0;       // 1 one pass, 2 count + scatter
  int mode = 0;            // base route: 0 hash probe, 1 directory, 2 affine rule
  int route = -1;          // the route taken: mode, 3 rank byte table, 4 presence map in LDS
  uint32_t view_shards = 0, view_shift = 0;  // the rings as Sv shards of Q << shift slots
  bool arrival = false;
  bool reserve = false, msg_drain = false, all_sidx = false;
  bool rank_route = false, pres_route = false, persist = false, fused = false;
  bool r8 = false;                     // 8-B records allowed (the width workspace exists)
  bool r8_on = false, rw_on = false;   // 8-B records / wide pure records written
  int rf = 0;                          // the drains' record form: 0 compact / long, 1 8-B, 2 wide pure
  int rec_bytes = 0;                   // 8, 18, 16 or 32
  bool ord_a12 = false;                // ordered drain: a second / third argument column is staged
  // arrival sharding
  bool arr_fused = false, rank_arr = false, pres_arr = false, allow8 = false, small_tiles = false;
  uint32_t arr_tiles = 0, arr_grid = 0;
  // what must exist before the first launch
  uint64_t sort_cap = 0;  // messages the per-message workspace holds (0: none needed)
  bool need_stage_rep = false, need_r8esc = false;  // (and the run reservations with `reserve`, the widths with `r8`)
  bool need_pres = false;   // a presence map: the registry mirror's, or
  bool build_pres = false;  // folded by this Send (mbx_presence_kernel)
  uint32_t key[kMbxFamilies];  // the variant launched per family; kNoKernel: none
  SortPlan() { std::fill(key, key + kMbxFamilies, kNoKernel); }
};

// The argument checks of a Send; false: an empty batch, nothing to do.
inline bool validate_sorted(const MboxSend& a, const RingGeom& g, bool consumer_running) {
  const uint64_t S = 1ull << g.log_s;
  if (S > (uint64_t)kMboxSortMaxShards) throw std::invalid_argument("sorted mailboxes: at most 1024 shards");
  if (S << g.log_q > 0xfffffffeull) throw std::invalid_argument("sorted mailboxes: shards * slots < 2^32");
  if (consumer_running) throw std::runtime_error("mailbox send: a persistent consumer owns the rings");
  if (a.M <= 0) return false;
  if (!a.actor || !a.a0) throw std::invalid_argument("mailbox send: missing column");
  if (a.a2 && !g.has_a2) throw std::invalid_argument("mailbox send: 3-argument batch but the rings have no a2 array");
  if (a.cap == 0 || (a.cap & (a.cap - 1))) throw std::invalid_argument("table capacity must be a power of two");
  if (!a.out_val || !a.out_st) throw std::invalid_argument("mailbox send: reply outputs required");
  if ((uint64_t)a.origin_base + (uint64_t)a.M > a.out_n) throw std::invalid_argument("mailbox send: reply view too small");
  if ((uint64_t)a.origin_base + (uint64_t)a.M > 0x7fffffffull) throw std::invalid_argument("mailbox send: origin >= 2^31");
  if (a.arrival && a.ordered) throw std::invalid_argument("mailbox send: arrival sharding cannot serve ordered methods");
  if (a.outbox_cap && a.outbox.size() != 6) throw std::invalid_argument("outbox: [actor, a0, a1, a2, method, count]");
  return true;
}

// `widths_overflowed`: the last 8-B Send's fields outgrew 64 bits (bit 31 of the widths
// word the device left): 16-B records from here on.
inline SortPlan plan_sorted(const MboxSend& a, const Tune& tn, const RingGeom& g, bool widths_overflowed) {
  SortPlan p;
  const uint32_t S = 1u << g.log_s;
  const int64_t tiles = p.tiles = (a.M + kSTile - 1) / kSTile;
  int64_t G = std::min<int64_t>({tiles, (int64_t)(kMboxSortHistWords / S), (int64_t)1024,
                                 (int64_t)kMboxSortGroups * kGroupBlocks});
  if (G >= 8) G -= G % 8;
  G = std::max<int64_t>(G, 1);
  p.G = (uint32_t)G;
  p.tpb = (uint32_t)((tiles + G - 1) / G);
  p.tile_grid = (uint32_t)(tiles >= 8 ? (tiles + 7) / 8 * 8 : tiles);
  // the sort: one pass, or count + scatter.  Stateless batches always take the one pass (each
  // tile reserves its runs: no look-back); ordered ones look back, which a grid under 1024
  // tiles cannot hide (8 Mi msgs 0.212-0.221 vs 0.228-0.230 ms per Send; 1 Mi msgs 0.047-0.049
  // vs 0.043 for count + scatter).  Tune mbox_sort=1 / 2 forces either.
  p.sort_mode = a.sort_mode ? a.sort_mode
                : tn.mbox_sort ? tn.mbox_sort
                : (tiles >= 1024 || (!a.ordered && !a.arrival)) ? 1 : 2;
  if (p.sort_mode < 1 || p.sort_mode > 2) throw std::invalid_argument("mailbox send: sort_mode 0..2");
  const bool two_pass = p.sort_mode == 2;
  p.ngroups = two_pass ? (uint32_t)((G + kGroupBlocks - 1) / kGroupBlocks) : 1u;
  const int mode = p.mode = (a.affine_w && a.n_dir) ? 2 : (a.dir && a.n_dir) ? 1 : 0;
  const bool a2 = a.a2 != 0, mc = a.method_col != 0;
  const uint32_t fixed_mul = a.fixed_method == kCalculatorMultiply;
  p.arrival = a.arrival;

  if (a.arrival) {  // fixed positions: enqueue + drain, no count pass
    p.rec_bytes = (a2 || mc) ? 32 : 16;
    p.view_shards = S;
    p.route = mode;
    // both in one launch (mbx_arrival_fused_kernel): an arrival run belongs to one tile, so the
    // fused form needs no grid-wide phase at any size (tune mbox_fused=0: the two kernels)
    p.arr_fused = !a2 && !mc && tn.mbox_fused != 0;
    if (!p.arr_fused) {
      p.key[kFamArrEnqueue] = vkey(mode, a2, mc);
      p.key[kFamArrDrain] = vkey(fixed_mul, mode);
      return p;
    }
    // rank byte routes for a stateless method on the directory: the records carry actor ids
    p.rank_arr = mode == 1 && a.dir_rank && a.n_dir <= kMaxMbox && method_stateless((uint32_t)a.method_uniform);
    // route mode 4 (the directory's presence map in LDS) when it fits -- for batches past 512
    // tiles: below, the map's staging per block (1024 blocks x 32 KB at 1 Mi) outweighs the
    // gathers it replaces (config 2: 31.2 vs 29.5 G msg/s)
    p.pres_arr = p.rank_arr && a.n_dir <= kPresMax && tiles > 512;
    p.route = p.pres_arr ? 4 : p.rank_arr ? 3 : mode;
    // 8-B records past 512 tiles (tune mbox_rec8: the sort's rule; per wave, 16 B when a value
    // of the wave does not fit)
    p.allow8 = g.planar && (tn.mbox_rec8 == 1 || (tn.mbox_rec8 < 0 && tiles > 512));
    if (p.allow8) p.rec_bytes = 8;
    // batches of up to 512 4096-message tiles: 1024-message tiles (four times the blocks)
    p.small_tiles = tiles <= 512;
    p.arr_tiles = p.small_tiles ? (uint32_t)((a.M + kST * 2 - 1) / (kST * 2)) : (uint32_t)tiles;
    p.arr_grid = p.arr_tiles >= 8 ? (p.arr_tiles + 7) / 8 * 8 : p.arr_tiles;
    p.key[kFamArrFused] = vkey((uint32_t)p.route, fixed_mul, p.small_tiles);
    p.need_pres = p.pres_arr;
    p.build_pres = p.need_pres && !(a.pres && a.pres_rank == a.rank_self);
    if (p.build_pres) p.key[kFamPresence] = vkey();
    return p;
  }

  p.sort_cap = (uint64_t)a.M;
  p.need_stage_rep = a.ordered;
  // Stateless batches run on a COARSER view of the same rings: 8 shards of Q * S / 8
  // slots (every ring is empty between epoch Sends, so any view keeps each actor's
  // messages in one ring, in message order; ordered batches keep the full S for the
  // ordered drain's one block per shard).  Longer runs per tile and shard: whole lines
  // for the sort's stores and the drain's loads (8 Mi msgs, 256 shards -> 32 / 16 / 8:
  // 0.222 -> 0.186 / 0.179 / 0.180 ms per Send; round 4 with run reservations and 8-B
  // records: 8 shards 2-3 % faster per bench step than 16, profiles/r4_mailbox_ab.md).
  p.view_shards = S;
  if (!a.ordered && kStatelessShards < S) {
    p.view_shift = g.log_s - (uint32_t)__builtin_ctz(kStatelessShards);
    p.view_shards = kStatelessShards;
  }
  // the stateless drain: ring order (default) or message order (tune mbox_drain_msg: every slot index written)
  p.msg_drain = tn.mbox_drain_msg != 0;
  p.all_sidx = p.msg_drain && !a.ordered;
  p.reserve = !a.ordered && !two_pass;  // (one-pass stateless: tiles reserve runs)
  // Rank byte gathers (route mode 3) for a stateless uniform one-pass Send on the
  // directory: 1 B per id (L2-resident) instead of the 4-B route word, and the
  // records carry the actor id -- every actor's messages still meet in one ring
  // (the shard is a function of the id), and no stateless handler reads a mailbox.
  p.rank_route = mode == 1 && a.dir_rank && a.n_dir <= kMaxMbox && !a.ordered && !p.all_sidx && !a2 && !mc &&
                 method_stateless((uint32_t)a.method_uniform) && !two_pass;
  // 8-B ring records: one-pass sort of a batch of one method, at most two arguments for
  // stateless batches (the ring-order drain) and one for ordered ones (the windowed drain:
  // 25.5 vs 24.5 G msg/s per 8 Mi SeqFold step, round 5).  Batches up to 512 tiles, which
  // take the fused kernel, keep 16-B records (1 Mi bench step 24.1 vs 21.9 G msg/s).  Field
  // widths: the mailbox from the state size or the directory, the rest split between the
  // zigzag arguments; a stateless record that does not fit spills, an ordered one escapes.
  p.r8 = (tn.mbox_rec8 == 1 || (tn.mbox_rec8 < 0 && tiles > 512)) && !two_pass && (!a.ordered || !a.a1) && !a2 &&
         !mc && g.planar && !p.all_sidx;
  p.r8_on = p.r8 && !widths_overflowed;
  // fields that outgrew 8 B in a stateless batch of a PURE method (its handler reads no actor):
  // wide pure records, 16 B {a0, a1} + a u16 place, instead of the 32-B long form (the 8 Mi
  // full-range int64 step writes and reads 18 B per message, not 32)
  p.rw_on = p.r8 && !p.r8_on && p.rank_route;  // (rank routes: stateless methods only)
  p.rf = p.r8_on ? 1 : p.rw_on ? 2 : 0;
  p.rec_bytes = p.r8_on ? 8 : p.rw_on ? 18 : ((a2 || mc) ? 32 : 16);  // (16: compact unless a value is wide)
  p.need_r8esc = p.r8_on && a.ordered;  // escape side array: {a0, mailbox} per ring slot
  // The sort + ring-order drain in one launch: slower than the two kernels for large batches once
  // the sort reserves its runs (8 Mi: 149 vs 95 + 39 us; its register file halves the drain's
  // occupancy), faster for small ones, where a launch and a kernel boundary weigh more (1 Mi bench
  // step: 5-7 % in three sessions).  Fused up to 512 tiles (2 Mi messages); tune mbox_fused=1 / 0
  // forces it.
  p.fused = !two_pass && !a.ordered && !p.all_sidx && (tn.mbox_fused == 1 || (tn.mbox_fused < 0 && tiles <= 512));
  // route mode 4: a rank-routed Send on a directory whose presence map fits LDS (a fused Send
  // stays at route 3); its persistent form (tune mbox_persist): auto past 512 tiles, where every
  // resident block has more than one tile to walk
  p.pres_route = !p.fused && p.rank_route && a.n_dir <= kPresMax;
  p.persist = p.pres_route && (tn.mbox_persist == 1 || (tn.mbox_persist < 0 && tiles > 512));
  p.route = p.pres_route ? 4 : p.rank_route ? 3 : mode;
  p.need_pres = p.pres_route;
  p.build_pres = p.need_pres && !(a.pres && a.pres_rank == a.rank_self);
  if (p.build_pres) p.key[kFamPresence] = vkey();

  if (two_pass) {
    p.key[kFamCount] = vkey(mode);
    p.key[kFamScatter] = vkey(a2, mc);
  } else if (p.fused) {
    // (a method column fixes no method; the record forms 1 and 2 imply no a2 and no column)
    p.key[kFamSortdrain] = vkey((uint32_t)p.route, a2, mc, mc ? 0u : fixed_mul, (uint32_t)p.rf);
    return p;
  } else if (p.persist) {
    p.key[kFamPersist] = vkey();
  } else {
    p.key[kFamOnesweep] = vkey((uint32_t)p.route, a2, mc);
  }
  if (a.ordered) {
    // one-argument batches: 4096-record windows, and a uniform SeqFold batch folds in
    // registers with the next window prefetched (0.341 vs 0.357 ms per 8 Mi SeqFold step,
    // round 5); two- and three-argument batches: 2048-record windows, the handler switch
    const bool a12 = p.ord_a12 = a.a1 || a2;  // (a column given: staged; none: the handlers see zeros)
    const bool fold = a.fixed_method == kSeqFold && !mc;
    p.key[kFamOrdered] = vkey(a12, a12 ? 0u : fold, p.r8_on);
    if (p.r8_on) p.key[kFamRec8Next] = vkey();
    p.key[kFamCompleteRing] = vkey();
  } else if (p.msg_drain) {
    p.key[kFamDrainMsg] = vkey(fixed_mul);
  } else {
    p.key[kFamDrainRing] = vkey(fixed_mul, (uint32_t)p.rf);
  }
  return p;
}

}  // namespace ptype
