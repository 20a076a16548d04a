"""The plan of a sorted mailbox Send (csrc/hip/mailbox_plan.hpp) through
``_hip.mailbox_send_plan``: host code, no GPU.  Every expectation below is
written out from the rules the Send has always followed (tile counts 512 / 513
and 1023 / 1024, directory sizes 2^18 and 2^24, the 8-shard stateless view, the
record forms, the tune switches); none is computed."""
import pytest

from ptype_amd.ops import hip
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_SEQ_FOLD

T = 4096  # messages per tile
MUL = "kCalculatorMultiply"


def plan(**kw):
    return hip().mailbox_send_plan(**kw)


def check(kw, **expected):
    p = plan(**kw)
    got = {k: p[k] for k in expected}
    assert got == expected, (kw, p)
    return p


def stateless(tiles, **kw):
    """A uniform Multiply batch of exactly `tiles` tiles on a directory with its rank byte table."""
    base = dict(M=tiles * T, ordered=False, method_uniform=METHOD_CALC_MULTIPLY, fixed_method=METHOD_CALC_MULTIPLY,
                a1=1, dir=1, n_dir=1000, dir_rank=1)
    base.update(kw)
    return base


def ordered(tiles, **kw):
    """A uniform SeqFold batch (one argument) on a directory."""
    base = dict(M=tiles * T, ordered=True, method_uniform=METHOD_SEQ_FOLD, fixed_method=METHOD_SEQ_FOLD, dir=1,
                n_dir=1000, n_state=1000)
    base.update(kw)
    return base


def arrival(tiles, **kw):
    return stateless(tiles, arrival=True, **kw)


# ---------------------------------------------------------------- stateless batches
def test_stateless_512_tiles_is_fused_on_rank_routes():
    check(stateless(512), tiles=512, G=512, tpb=1, tile_grid=512, ngroups=1, sort_mode=1, mode=1, route=3,
          view_shards=8, view_shift=5, arrival=False, reserve=True, msg_drain=False, all_sidx=False, rank_route=True,
          pres_route=False, persist=False, fused=True, r8=False, r8_on=False, rw_on=False, rf=0, rec_bytes=16,
          sort_cap=512 * T, need_stage_rep=False, need_r8esc=False, need_pres=False, build_pres=False,
          kernels=[f"mbx_sortdrain_kernel<3, false, false, {MUL}, 0>"])


def test_stateless_513_tiles_is_the_persistent_presence_sort_with_8_byte_records():
    check(stateless(512, M=512 * T + 1), tiles=513, G=512, tpb=2, tile_grid=520, sort_mode=1, route=4, reserve=True,
          rank_route=True, pres_route=True, persist=True, fused=False, r8=True, r8_on=True, rw_on=False, rf=1,
          rec_bytes=8, need_pres=True, build_pres=True,
          kernels=["mbx_persist_sort_kernel<>", "mbx_presence_kernel<>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"])
    # the registry mirror keeps the map for this rank: none is folded
    check(stateless(513, pres=1, pres_rank=0), need_pres=True, build_pres=False,
          kernels=["mbx_persist_sort_kernel<>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"])
    check(stateless(513, pres=1, pres_rank=1), build_pres=True)


def test_stateless_1023_and_1024_tiles_stay_one_pass():
    check(stateless(1023), G=1016, tpb=2, tile_grid=1024, sort_mode=1, persist=True, ngroups=1)
    check(stateless(1024), G=1024, tpb=1, tile_grid=1024, sort_mode=1, persist=True, ngroups=1)


def test_stateless_columns_and_methods():
    M = 3 * T + 17
    check(stateless(1, M=M), tiles=4, G=4, tpb=1, tile_grid=4, kernels=[f"mbx_sortdrain_kernel<3, false, false, {MUL}, 0>"])
    check(stateless(1, M=M, a1=0), route=3, rec_bytes=16, kernels=[f"mbx_sortdrain_kernel<3, false, false, {MUL}, 0>"])
    check(stateless(1, M=M, a2=1), route=1, rank_route=False, rec_bytes=32,
          kernels=[f"mbx_sortdrain_kernel<1, true, false, {MUL}, 0>"])
    check(stateless(1, M=M, method_col=1, method_uniform=0, fixed_method=0), route=1, rec_bytes=32,
          kernels=["mbx_sortdrain_kernel<1, false, true, 0, 0>"])
    check(stateless(1, M=M, a2=1, method_col=1, method_uniform=0, fixed_method=0), route=1, rec_bytes=32,
          kernels=["mbx_sortdrain_kernel<1, true, true, 0, 0>"])
    # a stateful uniform method keeps its mailbox route, and no fixed-method handler
    check(stateless(1, M=M, method_uniform=METHOD_COUNTER_ADD, fixed_method=METHOD_COUNTER_ADD, n_state=1000),
          route=1, rank_route=False, rec_bytes=16, kernels=["mbx_sortdrain_kernel<1, false, false, 0, 0>"])
    # no directory: the hash probe; an affine rule
    check(stateless(1, M=M, dir=0, n_dir=0, dir_rank=0), mode=0, route=0,
          kernels=[f"mbx_sortdrain_kernel<0, false, false, {MUL}, 0>"])
    check(stateless(1, M=M, affine_w=4), mode=2, route=2, kernels=[f"mbx_sortdrain_kernel<2, false, false, {MUL}, 0>"])


@pytest.mark.parametrize("n_dir, dir_rank, route, kernels", [
    (1 << 18, 1, 4, ["mbx_persist_sort_kernel<>", "mbx_presence_kernel<>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"]),
    ((1 << 18) + 1, 1, 3, ["mbx_onesweep_kernel<3, false, false>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"]),
    (1 << 18, 0, 1, ["mbx_onesweep_kernel<1, false, false>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"]),
    ((1 << 18) + 1, 0, 1, ["mbx_onesweep_kernel<1, false, false>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"]),
    (1 << 24, 1, 3, ["mbx_onesweep_kernel<3, false, false>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"]),
    ((1 << 24) + 1, 1, 1, ["mbx_onesweep_kernel<1, false, false>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"]),
    (1 << 24, 0, 1, ["mbx_onesweep_kernel<1, false, false>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"]),
    ((1 << 24) + 1, 0, 1, ["mbx_onesweep_kernel<1, false, false>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"]),
])
def test_directory_size_thresholds(n_dir, dir_rank, route, kernels):
    check(stateless(513, n_dir=n_dir, dir_rank=dir_rank), route=route, rank_route=route >= 3, pres_route=route == 4,
          rec_bytes=8, kernels=kernels)


@pytest.mark.parametrize("n_dir, route, kernel", [
    (1 << 18, 3, f"mbx_sortdrain_kernel<3, false, false, {MUL}, 0>"),  # (a fused Send stays at route 3)
    ((1 << 18) + 1, 3, f"mbx_sortdrain_kernel<3, false, false, {MUL}, 0>"),
    (1 << 24, 3, f"mbx_sortdrain_kernel<3, false, false, {MUL}, 0>"),
    ((1 << 24) + 1, 1, f"mbx_sortdrain_kernel<1, false, false, {MUL}, 0>"),
])
def test_directory_size_thresholds_fused(n_dir, route, kernel):
    check(stateless(4, n_dir=n_dir), route=route, fused=True, need_pres=False, kernels=[kernel])


@pytest.mark.parametrize("shards, view_shards, view_shift", [(8, 8, 0), (16, 8, 1), (256, 8, 5), (1024, 8, 7)])
def test_stateless_view_of_the_rings(shards, view_shards, view_shift):
    check(stateless(4, shards=shards, slots=4096), view_shards=view_shards, view_shift=view_shift)
    check(ordered(4, shards=shards, slots=4096), view_shards=shards, view_shift=0)
    check(arrival(4, shards=shards, slots=4096), view_shards=shards, view_shift=0)


def test_count_scatter_grid_is_bounded_by_the_histogram():
    # 2^18 histogram words / 1024 shards = 256 blocks
    check(ordered(600, shards=1024, slots=4096), G=256, tpb=3, ngroups=8, sort_mode=2)


def test_widths_overflowed():
    # with a rank route: wide pure records, 18 B
    check(stateless(513, widths_overflowed=True), r8=True, r8_on=False, rw_on=True, rf=2, rec_bytes=18,
          kernels=["mbx_persist_sort_kernel<>", "mbx_presence_kernel<>", f"mbx_drain_ring_kernel<{MUL}, true, 2>"])
    check(stateless(513, widths_overflowed=False), r8=True, r8_on=True, rw_on=False, rf=1, rec_bytes=8)
    # without one: compact records, 16 B
    check(stateless(513, dir_rank=0, widths_overflowed=True), r8=True, r8_on=False, rw_on=False, rf=0, rec_bytes=16,
          kernels=["mbx_onesweep_kernel<1, false, false>", f"mbx_drain_ring_kernel<{MUL}, true, 0>"])
    check(stateless(513, dir_rank=0, widths_overflowed=False), r8_on=True, rec_bytes=8,
          kernels=["mbx_onesweep_kernel<1, false, false>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"])
    # fused, forced: the wide pure form exists on rank routes only
    check(stateless(513, tune="mbox_fused=1", widths_overflowed=True), rec_bytes=18,
          kernels=[f"mbx_sortdrain_kernel<3, false, false, {MUL}, 2>"])
    # rings of 32-B records have no 8-B cells
    check(stateless(513, planar=False), r8=False, rec_bytes=16)


# ---------------------------------------------------------------- ordered batches
FOLD = "mbx_drain_ordered_kernel<false, 8, kSeqFold, true, false>"
DONE = "mbx_complete_ring_kernel<>"


def test_ordered_512_and_513_tiles_count_and_scatter():
    check(ordered(512), tiles=512, G=512, tpb=1, tile_grid=512, ngroups=16, sort_mode=2, route=1, view_shards=256,
          view_shift=0, reserve=False, rank_route=False, fused=False, r8=False, rec_bytes=16, need_stage_rep=True,
          need_r8esc=False, ord_a12=False,
          kernels=["mbx_count_kernel<1>", "mbx_scatter_kernel<false, false>", FOLD, DONE])
    check(ordered(513), tiles=513, G=512, tpb=2, tile_grid=520, ngroups=16, sort_mode=2, r8=False, rec_bytes=16,
          kernels=["mbx_count_kernel<1>", "mbx_scatter_kernel<false, false>", FOLD, DONE])


def test_ordered_1023_tiles_count_and_scatter_1024_one_pass():
    check(ordered(1023), G=1016, tpb=2, ngroups=32, sort_mode=2, r8=False, rec_bytes=16,
          kernels=["mbx_count_kernel<1>", "mbx_scatter_kernel<false, false>", FOLD, DONE])
    check(ordered(1024), G=1024, tpb=1, ngroups=1, sort_mode=1, reserve=False, r8=True, r8_on=True, rec_bytes=8,
          need_r8esc=True,
          kernels=["mbx_onesweep_kernel<1, false, false>", "mbx_drain_ordered_kernel<false, 8, kSeqFold, true, true>",
                   "mbx_rec8_next_kernel<>", DONE])
    check(ordered(1024, widths_overflowed=True), r8=True, r8_on=False, rw_on=False, rec_bytes=16, need_r8esc=False,
          kernels=["mbx_onesweep_kernel<1, false, false>", FOLD, DONE])


def test_ordered_columns_and_methods():
    # a second argument: 2048-record windows, 16-B records at any size
    check(ordered(1024, a1=1), ord_a12=True, r8=False, rec_bytes=16,
          kernels=["mbx_onesweep_kernel<1, false, false>", "mbx_drain_ordered_kernel<true, kOrdK, 0, false, false>", DONE])
    check(ordered(4, a2=1), ord_a12=True, rec_bytes=32,
          kernels=["mbx_count_kernel<1>", "mbx_scatter_kernel<true, false>",
                   "mbx_drain_ordered_kernel<true, kOrdK, 0, false, false>", DONE])
    # a method column: no register fold
    check(ordered(4, method_col=1, method_uniform=0), ord_a12=False, rec_bytes=32,
          kernels=["mbx_count_kernel<1>", "mbx_scatter_kernel<false, true>",
                   "mbx_drain_ordered_kernel<false, 8, 0, false, false>", DONE])
    check(ordered(1024, method_uniform=METHOD_COUNTER_ADD, fixed_method=METHOD_COUNTER_ADD), rec_bytes=8,
          kernels=["mbx_onesweep_kernel<1, false, false>", "mbx_drain_ordered_kernel<false, 8, 0, false, true>",
                   "mbx_rec8_next_kernel<>", DONE])
    check(ordered(4, dir=0, n_dir=0), mode=0, route=0,
          kernels=["mbx_count_kernel<0>", "mbx_scatter_kernel<false, false>", FOLD, DONE])
    check(ordered(4, affine_w=4), mode=2, route=2,
          kernels=["mbx_count_kernel<2>", "mbx_scatter_kernel<false, false>", FOLD, DONE])


# ---------------------------------------------------------------- arrival sharding
def test_arrival_512_tiles_takes_1024_message_tiles():
    check(arrival(512), arrival=True, arr_fused=True, rank_arr=True, pres_arr=False, route=3, allow8=False,
          rec_bytes=16, small_tiles=True, arr_tiles=2048, arr_grid=2048, view_shards=256, sort_cap=0, sort_mode=2,
          need_pres=False, need_stage_rep=False, kernels=[f"mbx_arrival_fused_kernel<3, {MUL}, 2>"])
    check(arrival(1, M=3 * T + 17), arr_tiles=13, arr_grid=16, tile_grid=4, small_tiles=True,
          kernels=[f"mbx_arrival_fused_kernel<3, {MUL}, 2>"])


def test_arrival_513_tiles_takes_the_presence_map_and_8_byte_records():
    check(arrival(513), arr_fused=True, rank_arr=True, pres_arr=True, route=4, allow8=True, rec_bytes=8,
          small_tiles=False, arr_tiles=513, arr_grid=520, need_pres=True, build_pres=True,
          kernels=["mbx_presence_kernel<>", f"mbx_arrival_fused_kernel<4, {MUL}>"])
    check(arrival(513, n_dir=(1 << 18) + 1), pres_arr=False, route=3, kernels=[f"mbx_arrival_fused_kernel<3, {MUL}>"])
    check(arrival(513, n_dir=1 << 18), pres_arr=True, route=4)
    check(arrival(513, n_dir=1 << 24), rank_arr=True, route=3)
    check(arrival(513, n_dir=(1 << 24) + 1), rank_arr=False, route=1, kernels=[f"mbx_arrival_fused_kernel<1, {MUL}>"])
    check(arrival(513, dir_rank=0), rank_arr=False, route=1, kernels=[f"mbx_arrival_fused_kernel<1, {MUL}>"])
    check(arrival(513, planar=False), allow8=False, rec_bytes=16)


def test_arrival_1023_and_1024_tiles():
    same = dict(arr_fused=True, route=4, small_tiles=False, kernels=["mbx_presence_kernel<>", f"mbx_arrival_fused_kernel<4, {MUL}>"])
    check(arrival(1023), sort_mode=2, arr_tiles=1023, arr_grid=1024, **same)
    check(arrival(1024), sort_mode=1, arr_tiles=1024, arr_grid=1024, **same)


def test_arrival_columns_and_methods():
    check(arrival(4, a2=1), arr_fused=False, route=1, rec_bytes=32, tile_grid=4,
          kernels=["mbx_arrival_enqueue_kernel<1, true, false>", f"mbx_arrival_drain_kernel<{MUL}, 1>"])
    check(arrival(4, method_col=1, method_uniform=0, fixed_method=0), arr_fused=False, rec_bytes=32,
          kernels=["mbx_arrival_enqueue_kernel<1, false, true>", "mbx_arrival_drain_kernel<0, 1>"])
    check(arrival(4, a2=1, method_col=1, method_uniform=0, fixed_method=0), arr_fused=False,
          kernels=["mbx_arrival_enqueue_kernel<1, true, true>", "mbx_arrival_drain_kernel<0, 1>"])
    check(arrival(4, a1=0), arr_fused=True, kernels=[f"mbx_arrival_fused_kernel<3, {MUL}, 2>"])
    check(arrival(4, method_uniform=METHOD_COUNTER_ADD, fixed_method=METHOD_COUNTER_ADD), rank_arr=False, route=1,
          kernels=["mbx_arrival_fused_kernel<1, 0, 2>"])
    check(arrival(4, dir=0, n_dir=0, dir_rank=0), route=0, kernels=[f"mbx_arrival_fused_kernel<0, {MUL}, 2>"])
    check(arrival(4, affine_w=4), route=2, kernels=[f"mbx_arrival_fused_kernel<2, {MUL}, 2>"])


# ---------------------------------------------------------------- tune switches
def test_mbox_sort():
    check(ordered(4, tune="mbox_sort=0"), sort_mode=2)
    check(ordered(4, tune="mbox_sort=1"), sort_mode=1, ngroups=1, kernels=["mbx_onesweep_kernel<1, false, false>", FOLD, DONE])
    check(ordered(1024, tune="mbox_sort=2"), sort_mode=2, ngroups=32, r8=False,
          kernels=["mbx_count_kernel<1>", "mbx_scatter_kernel<false, false>", FOLD, DONE])
    check(stateless(4, tune="mbox_sort=0"), sort_mode=1, fused=True)
    check(stateless(4, tune="mbox_sort=2"), sort_mode=2, reserve=False, rank_route=False, route=1, fused=False,
          ngroups=1, kernels=["mbx_count_kernel<1>", "mbx_scatter_kernel<false, false>",
                              f"mbx_drain_ring_kernel<{MUL}, true, 0>"])
    # the argument overrides the tune
    check(stateless(4, tune="mbox_sort=2", sort_mode=1), sort_mode=1, fused=True)
    check(ordered(1024, tune="mbox_sort=1", sort_mode=2), sort_mode=2)
    check(ordered(4, tune="mbox_sort=2", sort_mode=1), sort_mode=1)


def test_mbox_fused():
    check(stateless(4, tune="mbox_fused=-1"), fused=True, route=3)
    check(stateless(4, tune="mbox_fused=0"), fused=False, route=4, pres_route=True, persist=False,
          kernels=["mbx_onesweep_kernel<4, false, false>", "mbx_presence_kernel<>", f"mbx_drain_ring_kernel<{MUL}, true, 0>"])
    check(stateless(513, tune="mbox_fused=-1"), fused=False)
    check(stateless(513, tune="mbox_fused=1"), fused=True, route=3, pres_route=False, rec_bytes=8, need_pres=False,
          kernels=[f"mbx_sortdrain_kernel<3, false, false, {MUL}, 1>"])
    check(ordered(4, tune="mbox_fused=1"), fused=False)
    check(arrival(4, tune="mbox_fused=1"), arr_fused=True)
    check(arrival(4, tune="mbox_fused=0"), arr_fused=False, route=1, rec_bytes=16,
          kernels=["mbx_arrival_enqueue_kernel<1, false, false>", f"mbx_arrival_drain_kernel<{MUL}, 1>"])


def test_mbox_rec8():
    check(stateless(513, tune="mbox_rec8=-1"), r8=True, rec_bytes=8)
    check(stateless(513, tune="mbox_rec8=0"), r8=False, rec_bytes=16,
          kernels=["mbx_persist_sort_kernel<>", "mbx_presence_kernel<>", f"mbx_drain_ring_kernel<{MUL}, true, 0>"])
    check(stateless(4, tune="mbox_rec8=-1"), r8=False, rec_bytes=16)
    check(stateless(4, tune="mbox_rec8=1"), r8=True, rec_bytes=8, kernels=[f"mbx_sortdrain_kernel<3, false, false, {MUL}, 1>"])
    check(stateless(4, tune="mbox_rec8=1", dir_rank=0), kernels=[f"mbx_sortdrain_kernel<1, false, false, {MUL}, 1>"])
    check(ordered(4, tune="mbox_rec8=1"), r8=False)  # (count + scatter)
    check(ordered(4, tune="mbox_rec8=1,mbox_sort=1"), r8=True, need_r8esc=True)
    check(ordered(1024, tune="mbox_rec8=0"), r8=False, rec_bytes=16)
    check(arrival(4, tune="mbox_rec8=1"), allow8=True, rec_bytes=8)
    check(arrival(513, tune="mbox_rec8=0"), allow8=False, rec_bytes=16)


def test_mbox_persist():
    check(stateless(513, tune="mbox_persist=-1"), persist=True)
    check(stateless(513, tune="mbox_persist=0"), persist=False, route=4,
          kernels=["mbx_onesweep_kernel<4, false, false>", "mbx_presence_kernel<>", f"mbx_drain_ring_kernel<{MUL}, true, 1>"])
    check(stateless(4, tune="mbox_persist=-1,mbox_fused=0"), persist=False)
    check(stateless(4, tune="mbox_persist=1,mbox_fused=0"), persist=True,
          kernels=["mbx_persist_sort_kernel<>", "mbx_presence_kernel<>", f"mbx_drain_ring_kernel<{MUL}, true, 0>"])
    check(stateless(4, tune="mbox_persist=1"), persist=False, fused=True)  # (a fused Send has no presence route)
    check(stateless(513, tune="mbox_persist=1", n_dir=(1 << 18) + 1), persist=False)


def test_mbox_drain_msg():
    check(stateless(4, tune="mbox_drain_msg=0"), msg_drain=False, all_sidx=False)
    check(stateless(4, tune="mbox_drain_msg=1"), msg_drain=True, all_sidx=True, rank_route=False, route=1, fused=False,
          r8=False, kernels=["mbx_onesweep_kernel<1, false, false>", f"mbx_drain_msg_kernel<{MUL}>"])
    check(stateless(513, tune="mbox_drain_msg=1", fixed_method=0), r8=False, rec_bytes=16,
          kernels=["mbx_onesweep_kernel<1, false, false>", "mbx_drain_msg_kernel<0>"])
    # an ordered batch keeps its drain (and its slot indices)
    check(ordered(4, tune="mbox_drain_msg=1"), msg_drain=True, all_sidx=False,
          kernels=["mbx_count_kernel<1>", "mbx_scatter_kernel<false, false>", FOLD, DONE])


# ---------------------------------------------------------------- the tables
def test_variant_tables_hold_the_104_kernels():
    names = hip().mailbox_variants()
    assert len(names) == 104 and len(set(names)) == 104
    # the presence map on 1024-message arrival tiles cannot be reached (past 512 tiles / up to 512): no such row
    assert not [n for n in names if n.startswith("mbx_arrival_fused_kernel<4") and n.endswith(", 2>")]
    fam = sorted({n.split("<")[0] for n in names})
    assert fam == ["mbx_arrival_drain_kernel", "mbx_arrival_enqueue_kernel", "mbx_arrival_fused_kernel",
                   "mbx_complete_ring_kernel", "mbx_count_kernel", "mbx_drain_msg_kernel", "mbx_drain_ordered_kernel",
                   "mbx_drain_ring_kernel", "mbx_onesweep_kernel", "mbx_persist_sort_kernel", "mbx_presence_kernel",
                   "mbx_rec8_next_kernel", "mbx_scatter_kernel", "mbx_sortdrain_kernel"]


# ---------------------------------------------------------------- argument checks
@pytest.mark.parametrize("kw, exc, message", [
    (dict(shards=2048), ValueError, "sorted mailboxes: at most 1024 shards"),
    (dict(shards=1024, slots=1 << 22), ValueError, "sorted mailboxes: shards * slots < 2^32"),
    (dict(consumer_running=True), RuntimeError, "mailbox send: a persistent consumer owns the rings"),
    (dict(actor=0), ValueError, "mailbox send: missing column"),
    (dict(a0=0), ValueError, "mailbox send: missing column"),
    (dict(a2=1, with_a2=False), ValueError, "mailbox send: 3-argument batch but the rings have no a2 array"),
    (dict(cap=0), ValueError, "table capacity must be a power of two"),
    (dict(cap=48), ValueError, "table capacity must be a power of two"),
    (dict(out_val=0), ValueError, "mailbox send: reply outputs required"),
    (dict(out_st=0), ValueError, "mailbox send: reply outputs required"),
    (dict(out_n=99), ValueError, "mailbox send: reply view too small"),
    (dict(origin_base=1, out_n=100), ValueError, "mailbox send: reply view too small"),
    (dict(origin_base=0x7fffffff, out_n=1 << 32), ValueError, "mailbox send: origin >= 2^31"),
    (dict(arrival=True, ordered=True), ValueError, "mailbox send: arrival sharding cannot serve ordered methods"),
    (dict(outbox_cap=16, outbox=[1, 2, 3, 4, 5]), ValueError, "outbox: [actor, a0, a1, a2, method, count]"),
    (dict(sort_mode=3), ValueError, "mailbox send: sort_mode 0..2"),
    (dict(sort_mode=-1), ValueError, "mailbox send: sort_mode 0..2"),
    (dict(tune="mbox_sort=3"), ValueError, "mailbox send: sort_mode 0..2"),
])
def test_argument_checks(kw, exc, message):
    with pytest.raises(exc) as e:
        plan(**dict(dict(M=100), **kw))
    assert str(e.value) == message


def test_argument_checks_order_and_the_empty_batch():
    assert plan(M=0) is None and plan(M=-1) is None
    assert plan(M=0, actor=0, cap=3) is None  # (an empty batch is no error: nothing is looked at)
    with pytest.raises(RuntimeError):  # the rings come first
        plan(M=0, consumer_running=True)
    with pytest.raises(ValueError, match="missing column"):
        plan(M=100, actor=0, cap=3, out_val=0)
    assert plan(M=100, out_n=100, outbox_cap=16, outbox=[1, 2, 3, 4, 5, 6])["tiles"] == 1
