"""The lean bodies of the 8-B stateless Send (csrc/hip/mailbox_sort_dev.hpp: os_store_lean in
the persistent sort, drain_ring_tile_lean in the narrow ring drain) against the closed form
-- status by the known-id mask, ``a0 * a1`` as torch int64, every message checked -- and,
for the mailbox statistics and the record size, against the same Sends under
``mbox_persist=0``: the one-block-per-tile sort, which keeps the general store loop.

In-process, ``mbox_fused=0,mbox_rec8=1,mbox_persist=1``, on the table of
test_mailbox_persist_gpu.py (registered, unregistered, hash-probed and unknown ids).  The
shapes are the smallest at which the lean paths can go wrong:

* tile shapes: one message, one short of / exactly / one past a tile, three tiles and a
  partial one, a middle tile of unknown ids only, every id in one view shard;
* width edges: a Send's field widths come from the previous Send's maxima, so a case is a
  pair of Sends; the second holds in every tile the extremes of both argument fields.
  With a 16-bit mailbox field the arguments share 36 bits: a0's field ends below, at and
  above the record's word boundary (w0 = 3, 4, 5), either argument is 32 or 33 bits wide
  (the 32- / 64-bit boundary of pack, decode and multiply), a1 is all zero, a0 is wide
  beside a narrow a1;
* rings about 1.5 x a Send's load per view shard, three Sends: runs cross the rings' ends;
* a tile that spills (one 2^40 value) between two that do not, and rings the runs overrun
  (three tiles into 4 x 1024 slots): lean and general tiles in one launch;
* a captured two-step graph of the bench's step, replayed three times."""
import pytest
import torch

from ptype_amd.ops import batch as B
from ptype_amd.ops import hip
from ptype_amd.ops.mailbox import Mailboxes
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, STATUS_NO_ACTOR, STATUS_OK
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = 1 << 15
TILE = 4096
M3 = 3 * TILE + 17
STAT_KEYS = ("enqueued", "processed", "spilled", "overflow", "no_actor", "holes")
TUNE = "mbox_fused=0,mbox_rec8=1,mbox_persist=%d"
LEAN_KERNELS = {"mbx_persist_sort_kernel<>", "mbx_drain_ring_kernel<kCalculatorMultiply, true, 1>"}


@pytest.fixture(scope="module")
def table():
    t = RegistryTable(4 * N, device=DEV)
    ids = torch.cat([torch.arange(N), torch.arange(N + 100, N + 1100)])
    perm = torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(31))
    t.upsert(actor_keys(ids), torch.zeros(ids.numel(), dtype=torch.int32), perm.to(torch.int32))
    t.enable_directory(N + 50)  # ids N..N+49: in the directory, unregistered; N+100..: hash probes
    yield t
    hip().set_tune("")


def known_of(actor):
    return (actor < N) | ((actor >= N + 100) & (actor < N + 1100))


def signed_range(bits):
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


def batch(M, seed, n0=16, n1=16, actor=None):
    """M messages; a0 / a1 uniform over the signed n0- / n1-bit range (n1 = 0: all zero)."""
    g = torch.Generator().manual_seed(seed)
    if actor is None:
        actor = torch.randint(0, N + 3000, (M,), generator=g, dtype=torch.int32)
    lo, hi = signed_range(n0)
    a0 = torch.randint(lo, hi, (M,), generator=g, dtype=torch.int64)
    a1 = torch.zeros(M, dtype=torch.int64)
    if n1:
        lo, hi = signed_range(n1)
        a1 = torch.randint(lo, hi, (M,), generator=g, dtype=torch.int64)
    return B.MsgBatch(actor.to(DEV), a0.to(DEV), a1.to(DEV), None, METHOD_CALC_MULTIPLY)


def with_extremes(req, n0, n1):
    """Both extremes of each argument field in every tile, on known actors."""
    M = req.M
    for t0 in range(0, M, TILE):
        for off, col, v in ((5, req.a0, signed_range(n0)[0]), (70, req.a0, signed_range(n0)[1]),
                            (600, req.a1, signed_range(max(n1, 1))[0] if n1 else 0),
                            (3000, req.a1, signed_range(max(n1, 1))[1] if n1 else 0)):
            if t0 + off < M:
                col[t0 + off] = v
                req.actor[t0 + off] = (t0 // TILE) * 8 + off % 8  # registered
    return req


def check(req, val, st):
    known = known_of(req.actor)
    assert torch.equal(st, torch.where(known, STATUS_OK, STATUS_NO_ACTOR).to(torch.int32))
    assert torch.equal(val[known], (req.a0 * req.a1)[known])


class Run:
    """One pass over a case's Sends under mbox_persist=`persist`."""

    def __init__(self, table, persist):
        self.table, self.persist = table, persist
        self.stats, self.rec_bytes, self.widths = [], [], []
        assert hip().set_tune(TUNE % persist)

    def send(self, mb, req):
        val, st = mb.send(req, self.table, None, ordered=False)
        torch.cuda.synchronize()
        assert mb.last_route == 4, mb.last_route
        if self.persist:
            assert LEAN_KERNELS <= set(mb._m.last_plan["kernels"]) or mb.last_record_bytes != 8, mb._m.last_plan["kernels"]
        check(req, val, st)
        self.rec_bytes.append(int(mb.last_record_bytes))
        self.widths.append(mb.next_record_widths)

    def finish(self, mb):  # every ring drained (head == tail), no hole
        ctr = mb.shard_counters()
        assert (ctr[:, 0] == ctr[:, 2]).all(), ctr
        s = mb.stats()
        assert s["holes"] == 0, s
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


# ---------------------------------------------------------------- 1. tile shapes
@pytest.mark.parametrize("M", [1, TILE - 1, TILE, TILE + 1, M3])
def test_lean_tile_shapes(table, M):
    def case(run):
        mb = Mailboxes(DEV, shards=256, slots=1 << 14)
        for k in range(2):
            run.send(mb, batch(M, 32 + k))
        # (a short first Send leaves narrow widths: the second may spill, as under mbox_persist=0)
        s = run.finish(mb)
        assert s["overflow"] == 0 and (M < TILE or s["spilled"] == 0), s

    new = both(table, case)
    assert new.rec_bytes == [8, 8]


def test_lean_middle_tile_unknown_only(table):
    g = torch.Generator().manual_seed(3)
    actor = torch.randint(0, N + 3000, (M3,), generator=g, dtype=torch.int32)
    actor[TILE:2 * TILE] = torch.randint(N + 1100, N + 3000, (TILE,), generator=g, dtype=torch.int32)

    def case(run):
        mb = Mailboxes(DEV, shards=256, slots=1 << 14)
        for k in range(2):
            run.send(mb, batch(M3, 36 + k, actor=actor.clone()))
        s = run.finish(mb)
        assert s["overflow"] == 0 and s["no_actor"] >= 2 * TILE, s

    both(table, case)


def test_lean_one_view_shard(table):
    g = torch.Generator().manual_seed(4)
    actor = (torch.randint(0, N // 8, (M3,), generator=g, dtype=torch.int32) * 8 + 3)  # registered, view shard 3

    def case(run):
        mb = Mailboxes(DEV, shards=256, slots=1 << 14)
        for k in range(2):
            run.send(mb, batch(M3, 38 + k, actor=actor.clone()))
        s = run.finish(mb)
        assert s["spilled"] == 0 and s["enqueued"] == 2 * M3, s

    both(table, case)


# ---------------------------------------------------------------- 2. width edges
# (n0, n1): the bit lengths of the first Send's zigzag arguments.  With the 16-bit mailbox
# field they leave no slack, so the second Send's fields are exactly (n0, max(n1, 1)) wide
# where n0 + n1 = 36; the rows with slack split it as rec8_next does.
WIDTH_CASES = [(3, 33), (4, 32), (5, 31), (32, 4), (33, 3), (35, 1), (35, 0), (16, 0), (16, 16)]


@pytest.mark.parametrize("n0, n1", WIDTH_CASES)
def test_lean_width_edges(table, n0, n1):
    def case(run):
        mb = Mailboxes(DEV, shards=256, slots=1 << 14)
        run.send(mb, with_extremes(batch(M3, 50, n0, n1), n0, n1))
        wm, w0, w1, wide = run.widths[-1]
        m1 = max(n1, 1)
        assert (wm, wide) == (16, False) and w0 == n0 + (52 - wm - n0 - m1) // 2 and w1 == 52 - wm - w0, run.widths
        # the second Send: the extremes of the fields it runs on, in every tile; its values fit, so
        # nothing of it spills (the first may, on the widths a fresh Mailboxes starts with)
        spilled = mb.stats()["spilled"]
        run.send(mb, with_extremes(batch(M3, 51, w0, w1 if n1 else 0), w0, w1 if n1 else 0))
        s = run.finish(mb)
        assert s["overflow"] == 0 and s["spilled"] == spilled, (s, spilled)

    new = both(table, case)
    assert new.rec_bytes == [8, 8]


# ---------------------------------------------------------------- 3. ring wrap
def test_lean_ring_wrap(table):
    def case(run):
        mb = Mailboxes(DEV, shards=8, slots=2048)  # ~1450 records per shard and Send
        for k in range(3):
            run.send(mb, batch(M3, 60 + k))
        s = run.finish(mb)
        assert s["spilled"] == 0 and s["overflow"] == 0, s
        assert int(mb.shard_counters()[:, 0].min()) > 2048  # every ring's positions passed its end

    both(table, case)


# ---------------------------------------------------------------- 4. lean and general tiles in one launch
def test_lean_and_spilled_tiles(table):
    def case(run):
        mb = Mailboxes(DEV, shards=256, slots=1 << 14)
        run.send(mb, batch(M3, 70))
        req = batch(M3, 71)
        req.a0[TILE + 1234] = 1 << 40
        req.actor[TILE + 1234] = 77
        run.send(mb, req)
        s = run.finish(mb)
        assert s["spilled"] == 1 and s["overflow"] == 0, s
        mb = Mailboxes(DEV, shards=4, slots=1024)  # three tiles into 4096 slots: the later runs overrun
        for k in range(2):
            run.send(mb, batch(M3, 72 + k))
        s = run.finish(mb)
        assert s["spilled"] > 0 and s["overflow"] == 0, s

    both(table, case)


# ---------------------------------------------------------------- 5. a captured graph of the bench's step
def test_lean_captured_graph(table):
    M, U = M3, 2

    def case(run):
        ex = ActorExchange(table, M, chunks=1, delivery="mailbox", mailbox_shards=256, mailbox_slots=1 << 14)
        rq = B.MsgBatch(torch.empty(M, dtype=torch.int32, device=DEV), torch.empty(M, dtype=torch.int64, device=DEV),
                        torch.empty(M, dtype=torch.int64, device=DEV), None, METHOD_CALC_MULTIPLY)
        val = torch.empty(M, dtype=torch.int64, device=DEV)
        st = torch.empty(M, dtype=torch.int32, device=DEV)
        seed_t = torch.tensor([7 + j * 0x1000193 for j in range(U)], dtype=torch.int64, device=DEV)

        def prologue(j=0):
            B.gen_requests(M, N + 3000, METHOD_CALC_MULTIPLY, device=DEV, out=rq, seed_tensor=seed_t[j:j + 1])
            if j == U - 1:
                seed_t.add_(U * 0x1000193)

        graph = ex.capture(rq, val, st, prologue=prologue, repeat=U)
        mb = ex.mailboxes
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            assert mb.last_route == 4, mb.last_route
            check(rq, val, st)
            run.rec_bytes.append(int(mb.last_record_bytes))
        run.finish(mb)

    # (up to 2 Mi messages an exchange takes the arrival rings by default: the sorted kernels asked for)
    from ptype_amd.ops import tune

    tune.set("auto_arrival=0")
    try:
        both(table, case)
    finally:
        tune.set("auto_arrival=1")
