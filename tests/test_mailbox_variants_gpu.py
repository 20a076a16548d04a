"""Every row of the sorted mailboxes' kernel variant tables (csrc/hip/mailbox_sort*.hip)
runs, and runs right: one small Send per row, forced by the batch's shape, the table's
route and the tune switches; ``last_plan`` must name the row, the replies must be exact,
and the union of everything launched must be ``_hip.mailbox_variants()`` -- a key that
picked the wrong instantiation would answer with another method's handler, another
route's mailboxes or another record form.

Shapes: M = 3 * 4096 + 17 messages (a first, a middle and a partial last tile); the
arrival kernels on 4096-message tiles take batches past 512 tiles only, so their rows
use M = 512 * 4096 + 17.  Actor ids run past the registry: those messages answer
STATUS_NO_ACTOR.  References: the closed forms of Multiply and Echo, and ``send_ref``
(a serial execution in message order, which is the order an ordered drain gives every
actor) for batches that carry SeqFold -- computed once in actor-id space and shared."""
import pytest
import torch

from ptype_amd.ops import _ptr, hip, raw_stream
from ptype_amd.ops import batch as B
from ptype_amd.ops.mailbox import Mailboxes, send_ref
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY as MULM, METHOD_ECHO as ECHOM, METHOD_SEQ_FOLD as FOLDM,
                                   STATUS_NO_ACTOR, STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = 1000                     # registered actors: ids [0, N); the batches draw from [0, N + 100)
M_SMALL = 3 * 4096 + 17
M_BIG = 512 * 4096 + 17
MUL = "kCalculatorMultiply"


class World:
    """The tables (one per route), the batches' columns and the shared references."""

    def __init__(self):
        g = torch.Generator().manual_seed(5)
        self.perm = torch.randperm(N, generator=g)
        self.tables = {}
        for kind in ("hash", "dir", "bigdir", "affine"):
            t = RegistryTable(4 * N, device=DEV)
            mbox = torch.arange(N) if kind == "affine" else self.perm
            t.upsert(actor_keys(torch.arange(N)), torch.zeros(N, dtype=torch.int32), mbox.to(torch.int32))
            if kind == "dir":
                t.enable_directory(N + 50)  # ids N..N+49: in the directory, unregistered
            elif kind == "bigdir":
                t.enable_directory((1 << 18) + 64)  # past the presence map's 2^18 ids
            elif kind == "affine":
                t.enable_directory(N, affine_world=1)
            self.tables[kind] = t
        assert self.tables["affine"].directory()[2] == 1
        self.cols = {M: self._columns(M, 11 + M) for M in (M_SMALL, M_BIG)}
        self.state0 = torch.randint(0, 1 << 30, (N,), generator=g, dtype=torch.int64)  # by actor id
        self.mix = torch.tensor([FOLDM, ECHOM], dtype=torch.int32)[torch.randint(0, 2, (M_SMALL,), generator=g)]
        self._refs = {}

    @staticmethod
    def _columns(M, seed):
        g = torch.Generator().manual_seed(seed)
        cols = [torch.randint(0, N + 100, (M,), generator=g, dtype=torch.int32)]
        cols += [torch.randint(-(1 << 15), 1 << 15, (M,), generator=g, dtype=torch.int64) for _ in range(3)]
        return [c.to(DEV) for c in cols]

    def mailbox_of(self, kind):  # actor id -> mailbox
        return torch.arange(N) if kind == "affine" else self.perm

    def ordered_ref(self, method):
        """(replies, statuses, final state by actor id) of the small batch run in message order."""
        if method not in self._refs:
            actor, a0 = self.cols[M_SMALL][0].cpu(), self.cols[M_SMALL][1].cpu()
            col = method if isinstance(method, int) else self.mix
            known = actor < N
            state = self.state0.clone()
            val, st = send_ref(B.MsgBatch(actor, a0, None, None, col), torch.where(known, 0, -1),
                               torch.where(known, actor, 0).to(torch.int64), state)
            self._refs[method] = (val, st, state)
        return self._refs[method]


@pytest.fixture(scope="module")
def world():
    w = World()
    w.small = Mailboxes(DEV, shards=16, slots=4096)
    w.big = Mailboxes(DEV, shards=64, slots=1 << 16)
    w.launched = set()
    yield w
    hip().set_tune("")


def send(mb, t, req, state, ordered, arrival, dir_rank, kept, sort_mode):
    """Mailboxes.send on the sorted kernels, with the rank byte table and the kept presence
    map given or withheld (the routes 1 / 3 / 4 on one directory)."""
    M = req.M
    val = torch.empty(M, dtype=torch.int64, device=DEV)
    st = torch.empty(M, dtype=torch.int32, device=DEV)
    uniform = isinstance(req.method, int)
    mcol = None if uniform else req.method.to(torch.int16).contiguous()
    d, n_dir, affine = t.directory()
    mb._m.send_sorted(_ptr(req.actor), _ptr(req.a0), _ptr(req.a1), _ptr(req.a2), _ptr(mcol),
                      int(req.method) if uniform else 0, M, _ptr(t.table), t.cap, _ptr(d), n_dir, affine, 0, 0,
                      _ptr(val), _ptr(st), M, _ptr(state), 0 if state is None else state.numel(), 0, [], 0, arrival,
                      ordered, int(req.method) if uniform else 0, raw_stream(DEV), sort_mode,
                      _ptr(t.dir_rank) if d is not None and dir_rank else 0,
                      _ptr(t.presence) if kept and t.presence is not None else 0, t.presence_rank)
    torch.cuda.synchronize()
    return val, st


def run(world, targets, table, method, *, M=M_SMALL, a1=True, a2=False, ordered=False, arrival=False, dir_rank=False,
        kept=True, sort_mode=0, tune="", widen_first=False):
    """One Send that must launch every kernel of `targets`; `method`: MULM, ECHOM, FOLDM, "mc"
    (a column of Multiply and Echo) or "mix" (a column of SeqFold and Echo, ordered)."""
    t = world.tables[table]
    actor, c0, c1, c2 = world.cols[M]
    if method == "mc":
        col = torch.where(c0 % 2 == 0, MULM, ECHOM).to(torch.int32)
    else:
        col = world.mix.to(DEV) if method == "mix" else method
    req = B.MsgBatch(actor, c0, c1 if a1 else None, c2 if a2 else None, col)
    mb = world.small if M == M_SMALL else world.big
    assert hip().set_tune(tune)
    if widen_first:  # a Send whose values outgrow the 8-B fields: the next one takes the wide pure form
        mb = Mailboxes(DEV, shards=16, slots=4096)
        wide = torch.full_like(c0, (1 << 62) + 3)
        send(mb, t, B.MsgBatch(actor, wide, wide, None, method), None, False, arrival, dir_rank, kept, sort_mode)
    state = None
    if ordered:
        state = torch.zeros(N, dtype=torch.int64)
        state[world.mailbox_of(table)] = world.state0
        state = state.to(DEV)
    val, st = send(mb, t, req, state, ordered, arrival, dir_rank, kept, sort_mode)
    kernels = mb._m.last_plan["kernels"]
    assert set(targets) <= set(kernels), (targets, kernels)
    world.launched.update(kernels)

    known = actor < N
    if method in (FOLDM, "mix"):
        rval, rst, rstate = world.ordered_ref(method)
        assert torch.equal(st.cpu(), rst) and torch.equal(val.cpu()[known.cpu()], rval[known.cpu()])
        assert torch.equal(state.cpu()[world.mailbox_of(table)], rstate)
    else:
        assert torch.equal(st, torch.where(known, STATUS_OK, STATUS_NO_ACTOR).to(torch.int32))
        mul = (col == MULM) if method == "mc" else torch.full_like(known, method == MULM)
        want = torch.where(mul, c0 * (c1 if a1 else 0), c0)
        assert torch.equal(val[known], want[known])
    s = mb.stats()
    assert s["holes"] == 0 and s["overflow"] == 0, s


ROUTES = [(0, "hash"), (1, "dir"), (2, "affine")]  # (without the rank byte table a directory is route 1)


def b(x):
    return "true" if x else "false"


# ---------------------------------------------------------------- the fused sort + drain
@pytest.mark.parametrize("mo, table", ROUTES)
def test_sortdrain_rows(world, mo, table):
    k = "mbx_sortdrain_kernel<%d, %s, %s, %s, %d>"
    run(world, [k % (mo, "false", "false", MUL, 0)], table, MULM)
    run(world, [k % (mo, "false", "false", "0", 0)], table, ECHOM)
    run(world, [k % (mo, "false", "false", MUL, 1)], table, MULM, tune="mbox_rec8=1")
    run(world, [k % (mo, "false", "false", "0", 1)], table, ECHOM, tune="mbox_rec8=1")
    run(world, [k % (mo, "false", "true", "0", 0)], table, "mc")
    run(world, [k % (mo, "true", "false", MUL, 0)], table, MULM, a2=True)
    run(world, [k % (mo, "true", "false", "0", 0)], table, ECHOM, a2=True)
    run(world, [k % (mo, "true", "true", "0", 0)], table, "mc", a2=True)


def test_sortdrain_rank_route_rows(world):
    for method, fx in ((MULM, MUL), (ECHOM, "0")):
        k = f"mbx_sortdrain_kernel<3, false, false, {fx}, %d>"
        run(world, [k % 0], "dir", method, dir_rank=True)
        run(world, [k % 1], "dir", method, dir_rank=True, tune="mbox_rec8=1")
        run(world, [k % 2], "dir", method, dir_rank=True, tune="mbox_rec8=1", widen_first=True)
        run(world, [k % 0], "bigdir", method, dir_rank=True)  # (fused: route 3 past 2^18 ids as below them)


# ---------------------------------------------------------------- the separate sorts and drains
@pytest.mark.parametrize("mo, table", ROUTES)
def test_onesweep_count_and_ordered_rows(world, mo, table):
    fold = "mbx_drain_ordered_kernel<false, 8, kSeqFold, true, false>"
    done = "mbx_complete_ring_kernel<>"
    for a2 in (False, True):
        for method in (FOLDM, "mix"):
            sweep = f"mbx_onesweep_kernel<{mo}, {b(a2)}, {b(method == 'mix')}>"
            drain = ("mbx_drain_ordered_kernel<true, kOrdK, 0, false, false>" if a2
                     else fold if method == FOLDM else "mbx_drain_ordered_kernel<false, 8, 0, false, false>")
            run(world, [sweep, drain, done], table, method, a1=False, a2=a2, ordered=True, sort_mode=1)
    # (an ordered batch of this size counts and scatters by default)
    run(world, [f"mbx_count_kernel<{mo}>", "mbx_scatter_kernel<false, false>", fold, done], table, FOLDM, a1=False,
        ordered=True)


def test_scatter_rows(world):
    for a2 in (False, True):
        for method in (FOLDM, "mix"):
            run(world, ["mbx_count_kernel<1>", f"mbx_scatter_kernel<{b(a2)}, {b(method == 'mix')}>"], "dir", method,
                a2=a2, ordered=True)
    # a stateless batch through count + scatter
    run(world, ["mbx_count_kernel<1>", "mbx_scatter_kernel<false, false>", f"mbx_drain_ring_kernel<{MUL}, true, 0>"],
        "dir", MULM, dir_rank=True, tune="mbox_sort=2")


def test_ordered_8_byte_record_rows(world):
    nxt, done = "mbx_rec8_next_kernel<>", "mbx_complete_ring_kernel<>"
    run(world, ["mbx_onesweep_kernel<1, false, false>", "mbx_drain_ordered_kernel<false, 8, kSeqFold, true, true>", nxt,
                done], "dir", FOLDM, a1=False, ordered=True, sort_mode=1, tune="mbox_rec8=1")
    run(world, ["mbx_onesweep_kernel<1, false, false>", "mbx_drain_ordered_kernel<false, 8, 0, false, true>", nxt, done],
        "dir", ECHOM, a1=False, ordered=True, sort_mode=1, tune="mbox_rec8=1")
    # an ordered batch of a stateless method and two arguments: the handler switch
    run(world, ["mbx_drain_ordered_kernel<true, kOrdK, 0, false, false>", done], "dir", MULM, ordered=True)


def test_rank_and_presence_sort_rows_and_ring_drain_rows(world):
    for method, fx in ((MULM, MUL), (ECHOM, "0")):
        ring = f"mbx_drain_ring_kernel<{fx}, true, %d>"
        run(world, ["mbx_onesweep_kernel<3, false, false>", ring % 0], "bigdir", method, dir_rank=True,
            tune="mbox_fused=0")
        run(world, ["mbx_onesweep_kernel<4, false, false>", "mbx_presence_kernel<>", ring % 0], "dir", method,
            dir_rank=True, kept=False, tune="mbox_fused=0")
        run(world, ["mbx_onesweep_kernel<4, false, false>", ring % 1], "dir", method, dir_rank=True,
            tune="mbox_fused=0,mbox_rec8=1")
        run(world, ["mbx_persist_sort_kernel<>", ring % 1], "dir", method, dir_rank=True,
            tune="mbox_fused=0,mbox_rec8=1,mbox_persist=1")
        run(world, ["mbx_persist_sort_kernel<>", ring % 2], "dir", method, dir_rank=True,
            tune="mbox_fused=0,mbox_rec8=1,mbox_persist=1", widen_first=True)
        run(world, ["mbx_onesweep_kernel<1, false, false>", f"mbx_drain_msg_kernel<{fx}>"], "dir", method,
            dir_rank=True, tune="mbox_drain_msg=1")


# ---------------------------------------------------------------- arrival rings
@pytest.mark.parametrize("mo, table, dir_rank", [(0, "hash", False), (1, "dir", False), (2, "affine", False),
                                                 (3, "dir", True)])
def test_arrival_fused_1024_message_tile_rows(world, mo, table, dir_rank):
    run(world, [f"mbx_arrival_fused_kernel<{mo}, {MUL}, 2>"], table, MULM, arrival=True, dir_rank=dir_rank)
    run(world, [f"mbx_arrival_fused_kernel<{mo}, 0, 2>"], table, ECHOM, arrival=True, dir_rank=dir_rank)


@pytest.mark.parametrize("mo, table, dir_rank", [(0, "hash", False), (1, "dir", False), (2, "affine", False),
                                                 (3, "bigdir", True), (4, "dir", True)])
def test_arrival_fused_4096_message_tile_rows(world, mo, table, dir_rank):
    run(world, [f"mbx_arrival_fused_kernel<{mo}, {MUL}>"], table, MULM, M=M_BIG, arrival=True, dir_rank=dir_rank)
    run(world, [f"mbx_arrival_fused_kernel<{mo}, 0>"], table, ECHOM, M=M_BIG, arrival=True, dir_rank=dir_rank)


@pytest.mark.parametrize("mo, table", ROUTES)
def test_arrival_enqueue_and_drain_rows(world, mo, table):
    enq, drain = f"mbx_arrival_enqueue_kernel<{mo}, %s, %s>", f"mbx_arrival_drain_kernel<%s, {mo}>"
    run(world, [enq % ("false", "false"), drain % MUL], table, MULM, arrival=True, tune="mbox_fused=0")
    run(world, [enq % ("false", "true"), drain % "0"], table, "mc", arrival=True)
    run(world, [enq % ("true", "false"), drain % MUL], table, MULM, a2=True, arrival=True)
    run(world, [enq % ("true", "true"), drain % "0"], table, "mc", a2=True, arrival=True)


# ---------------------------------------------------------------- and nothing else
def test_every_row_was_launched(world):
    """Runs last in this module: the Sends above launched every row of the tables."""
    rows = set(hip().mailbox_variants())
    assert len(rows) == 104
    assert world.launched == rows, (sorted(rows - world.launched), sorted(world.launched - rows))
