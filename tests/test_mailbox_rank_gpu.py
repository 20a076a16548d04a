"""The persistent mailbox sort's front half (csrc/hip/mailbox_sort_dev.hpp: os_rank_scan, the
ranking by scanned byte counters; resolve_pres_lean, the presence-map resolve with its probes on
a slow path; wave_max_u32 by DPP) against the closed form -- status by the known-id mask,
``a0 * a1`` as torch int64, every message checked -- and, for the mailbox statistics, the record
sizes and the next widths, against the same Sends under ``mbox_persist=0``: the one-block-per-
tile sort, which keeps os_rank and resolve_pres (it shares wave_max_u32, so the width cases also
assert the closed form of the widths).

In-process, ``mbox_fused=0,mbox_rec8=1,mbox_persist=1``; every Send asserts that its plan ran
``mbx_persist_sort_kernel<>``.  Two messages ranked alike would overwrite each other and show as
a missing reply or a hole; what is established is distinct, in-range slots and right counts.

A message at position i of the batch has lane i % 64, item (i / 64) % 8, wave (i / 512) % 8 of
tile i / 4096; a directory id's view shard is id & (S - 1).  The table: ids 0..N-1 registered in
the directory; N..N+49 in the directory, unregistered, of which N+10..N+19 are registered on
rank 300 (presence state 2: probed, another rank's); N+100..N+1099 registered past the directory
(probed); the rest unknown (probed when past the directory, and missed)."""
import pytest
import torch

from ptype_amd.ops import batch as B
from ptype_amd.ops import hip
from ptype_amd.ops.mailbox import Mailboxes
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, STATUS_NO_ACTOR, STATUS_OK
from ptype_amd.ops.table import RegistryTable, actor_keys

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = 1 << 15
TILE = 4096
M3 = 3 * TILE + 17
STAT_KEYS = ("enqueued", "processed", "spilled", "overflow", "no_actor", "holes")
TUNE = "mbox_fused=0,mbox_rec8=1,mbox_persist=%d"
PERSIST = "mbx_persist_sort_kernel<>"
LANES8 = (0, 15, 16, 31, 32, 47, 48, 63)


@pytest.fixture(scope="module")
def table():
    t = RegistryTable(4 * N, device=DEV)
    ids = torch.cat([torch.arange(N), torch.arange(N + 100, N + 1100)])
    perm = torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(31))
    t.upsert(actor_keys(ids), torch.zeros(ids.numel(), dtype=torch.int32), perm.to(torch.int32))
    far = torch.arange(N + 10, N + 20)
    t.upsert(actor_keys(far), torch.full((10,), 300, dtype=torch.int32), torch.arange(10, dtype=torch.int32))
    t.enable_directory(N + 50)
    yield t
    hip().set_tune("")


def known_of(actor):
    return ((actor >= 0) & (actor < N)) | ((actor >= N + 100) & (actor < N + 1100))


def places(M):
    i = torch.arange(M)
    return i % 64, (i // 64) % 8, (i // 512) % 8, i // TILE  # lane, item, wave, tile


def registered(shard, g):
    """A registered directory id of view shard `shard` (a tensor of shards) each."""
    return (torch.randint(0, N // 8, shard.shape, generator=g) * 8 + shard).to(torch.int32)


def no_probe_miss(M, g):
    """Ids that miss without a probe: unregistered directory ids and 0xffffffff."""
    a = (N + 20 + torch.randint(0, 30, (M,), generator=g)).to(torch.int32)
    return torch.where(torch.rand(M, generator=g) < 0.25, torch.tensor(-1, dtype=torch.int32), a)


def probed(M, g):
    return (N + 100 + torch.randint(0, 1000, (M,), generator=g)).to(torch.int32)


def mixed(M, g):
    """Registered, unregistered, state-2, hash-probed and unknown ids, and 0xffffffff."""
    a = torch.randint(0, N + 3000, (M,), generator=g, dtype=torch.int32)
    a[torch.rand(M, generator=g) < 0.02] = -1
    return a


def batch(actor, seed, n0=16, n1=16):
    g = torch.Generator().manual_seed(seed)
    M = actor.numel()
    a0 = torch.randint(-(1 << (n0 - 1)), (1 << (n0 - 1)) - 1, (M,), generator=g, dtype=torch.int64)
    a1 = torch.randint(-(1 << (n1 - 1)), (1 << (n1 - 1)) - 1, (M,), generator=g, dtype=torch.int64)
    return B.MsgBatch(actor.clone().to(DEV), a0.to(DEV), a1.to(DEV), None, METHOD_CALC_MULTIPLY)


def check(req, val, st):
    known = known_of(req.actor)
    assert torch.equal(st, torch.where(known, STATUS_OK, STATUS_NO_ACTOR).to(torch.int32))
    assert torch.equal(val[known], (req.a0 * req.a1)[known])
    return int(known.sum())


class Run:
    """One pass over a case's Sends under mbox_persist=`persist`."""

    def __init__(self, table, persist):
        self.table, self.persist = table, persist
        self.stats, self.rec_bytes, self.widths, self.known = [], [], [], 0
        assert hip().set_tune(TUNE % persist)

    def send(self, mb, req):
        val, st = mb.send(req, self.table, None, ordered=False)
        torch.cuda.synchronize()
        assert mb.last_route == 4, mb.last_route
        kernels = set(mb._m.last_plan["kernels"])
        assert (PERSIST in kernels) == bool(self.persist), kernels
        self.known += check(req, val, st)
        self.rec_bytes.append(int(mb.last_record_bytes))
        self.widths.append(mb.next_record_widths)

    def finish(self, mb):  # every ring drained (head == tail), no hole, every known id enqueued
        ctr = mb.shard_counters()
        assert (ctr[:, 0] == ctr[:, 2]).all(), ctr
        s = mb.stats()
        assert s["holes"] == 0, s
        assert s["enqueued"] + s["spilled"] == self.known and s["overflow"] == 0, (s, self.known)
        self.stats.append({k: s[k] for k in STAT_KEYS})
        return s


def both(table, case):
    """`case(run)` under the persistent sort and under the one-block-per-tile sort: the same
    statistics, record sizes and next widths."""
    new = Run(table, 1)
    case(new)
    ref = Run(table, 0)
    case(ref)
    assert new.stats == ref.stats, (new.stats, ref.stats)
    assert new.rec_bytes == ref.rec_bytes, (new.rec_bytes, ref.rec_bytes)
    assert new.widths == ref.widths, (new.widths, ref.widths)
    return new


def two_sends(table, actor, seed, shards=256, slots=1 << 14, spill_free=True):
    def case(run):
        mb = Mailboxes(DEV, shards=shards, slots=slots)
        for k in range(2):
            run.send(mb, batch(actor, seed + k))
        s = run.finish(mb)
        if spill_free:
            assert s["spilled"] == 0 and s["enqueued"] == run.known, (s, run.known)

    return both(table, case)


# ---------------------------------------------------------------- 1. full byte fields
@pytest.mark.parametrize("shard", [0, 3, 4, 7])
def test_rank_one_view_shard(table, shard):
    """Every message in one view shard: the lowest / highest byte of either dword counts 64 per
    item, and a wave's running count reaches 512."""
    g = torch.Generator().manual_seed(100 + shard)
    actor = registered(torch.full((M3,), shard), g)
    new = two_sends(table, actor, 110 + 2 * shard)
    assert new.stats[0]["enqueued"] == 2 * M3


# ---------------------------------------------------------------- 2. row and half crossings of the scan
def lane_pattern(name, M, g):
    lane, item, wave, tile = places(M)
    if name == "lanes8":  # one shard at the rows' first and last lanes, misses elsewhere
        reg = registered(torch.full((M,), 5), g)
        at = torch.zeros(M, dtype=torch.bool)
        for l in LANES8:
            at |= lane == l
        return torch.where(at, reg, no_probe_miss(M, g))
    if name == "lane>>3":
        return registered(lane >> 3, g)
    if name == "lane&7":
        return registered(lane & 7, g)
    if name == "lane>>4":
        return registered(lane >> 4, g)
    if name == "by_item":  # another pattern in every item and wave; some lanes of an item miss
        reg = registered((lane * (item + 1) + 3 * item + wave + tile) & 7, g)
        return torch.where((lane + 5 * item) % 11 == 0, no_probe_miss(M, g), reg)
    raise AssertionError(name)


@pytest.mark.parametrize("name", ["lanes8", "lane>>3", "lane&7", "lane>>4", "by_item"])
def test_rank_lane_patterns(table, name):
    g = torch.Generator().manual_seed(7)
    two_sends(table, lane_pattern(name, M3, g), 130)


# ---------------------------------------------------------------- 3. views below 8 shards
@pytest.mark.parametrize("shards", [4, 2, 1])
def test_rank_small_views(table, shards):
    g = torch.Generator().manual_seed(40 + shards)
    lane, item, wave, tile = places(M3)
    for actor in (mixed(M3, g), registered(torch.full((M3,), shards - 1), g), registered((lane + item) & 7, g)):
        def case(run):
            mb = Mailboxes(DEV, shards=shards, slots=1 << 15)
            for k in range(2):
                run.send(mb, batch(actor, 140 + k))
                assert mb.last_view_shards == shards
            s = run.finish(mb)
            assert s["spilled"] == 0, s

        both(table, case)


# ---------------------------------------------------------------- 4. ragged ends
@pytest.mark.parametrize("M", [1, 63, 65, TILE - 1, TILE + 1])
def test_rank_ragged_ends(table, M):
    g = torch.Generator().manual_seed(50 + M)
    # (a short first Send leaves narrow widths: the second may spill, as under mbox_persist=0)
    two_sends(table, mixed(M, g), 150, spill_free=False)
    two_sends(table, registered(torch.full((M,), 7), g), 152, spill_free=False)


# ---------------------------------------------------------------- 5. the resolve's slow path
def test_resolve_probes_by_wave(table):
    """Tile 0: no wave holds an id that probes.  Tile 1: exactly one lane of one wave does.
    Tile 2: every lane of wave 5 does, in every item, and wave 2 holds state-2 ids and unknown
    ids past the directory in some lanes.  The partial tile: mixed."""
    g = torch.Generator().manual_seed(60)
    lane, item, wave, tile = places(M3)
    actor = torch.where(torch.rand(M3, generator=g) < 0.2, no_probe_miss(M3, g), registered((lane ^ item) & 7, g))
    one = TILE + 3 * 512 + 2 * 64 + 37
    actor[one] = N + 100 + 123
    w5 = (tile == 2) & (wave == 5)
    actor[w5] = probed(M3, g)[w5]
    w2 = (tile == 2) & (wave == 2) & (lane % 5 == 0)
    far = (N + 10 + torch.randint(0, 10, (M3,), generator=g)).to(torch.int32)  # state 2, rank 300
    unknown = (N + 1100 + torch.randint(0, 1900, (M3,), generator=g)).to(torch.int32)
    actor[w2] = torch.where(item % 2 == 0, far, unknown)[w2]
    actor[3 * TILE:] = mixed(17, g)
    two_sends(table, actor, 160)


def test_resolve_tile_of_misses(table):
    """The middle tile holds only ids that miss: unregistered directory ids, 0xffffffff, state-2
    ids of another rank, unknown ids past the directory."""
    g = torch.Generator().manual_seed(61)
    actor = mixed(M3, g)
    miss = no_probe_miss(TILE, g)
    far = (N + 10 + torch.randint(0, 10, (TILE,), generator=g)).to(torch.int32)
    unknown = (N + 1100 + torch.randint(0, 1900, (TILE,), generator=g)).to(torch.int32)
    pick = torch.randint(0, 3, (TILE,), generator=g)
    actor[TILE:2 * TILE] = torch.where(pick == 0, miss, torch.where(pick == 1, far, unknown))
    assert not known_of(actor[TILE:2 * TILE]).any()
    new = two_sends(table, actor, 162)
    assert new.stats[0]["no_actor"] >= 2 * TILE


# ---------------------------------------------------------------- 6. width maxima
@pytest.mark.parametrize("lane", [0, 63, 37])
def test_rank_width_maxima_one_lane(table, lane):
    """The extremes of the three fields sit in one lane of one wave only (tile 1, wave 2, items 0,
    3 and 7); a message without an actor carries a wider value, which counts for nothing."""
    n0, n1, big_id = 20, 11, 20001  # 15-bit id
    g = torch.Generator().manual_seed(70 + lane)
    actor = registered(torch.randint(0, 8, (M3,), generator=g), g) % 256  # 8-bit ids
    at = TILE + 2 * 512 + lane

    def case(run):
        mb = Mailboxes(DEV, shards=256, slots=1 << 14)
        req = batch(actor, 170, 4, 4)
        req.actor[at] = big_id
        req.a0[at + 3 * 64] = -(1 << (n0 - 1))
        req.a1[at + 7 * 64] = (1 << (n1 - 1)) - 1
        req.actor[at + 64] = N + 30  # unregistered: its arguments are no record's
        req.a0[at + 64] = 1 << 40
        run.send(mb, req)
        wm, w0, w1, wide = run.widths[-1]
        assert (wm, wide) == (15, False) and w0 == n0 + (52 - wm - n0 - n1) // 2 and w1 == 52 - wm - w0, run.widths
        spilled = mb.stats()["spilled"]
        req = batch(actor, 171, w0, w1)  # the second Send runs on those widths: nothing of it spills
        req.actor[at] = big_id
        run.send(mb, req)
        s = run.finish(mb)
        assert s["spilled"] == spilled, (s, spilled)

    both(table, case)
