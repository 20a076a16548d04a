"""Every device-side resolver of a message's actor field, on hostile registry tables.

The resolvers do not share one lookup (``table_lookup_kernel`` probes slot by slot, the
route kernels probe 4-slot groups with selects, and the directory-with-fallback logic
exists in several copies), so each is run on the same tables -- a wrapped probe chain,
tombstones inside a chain, values that fit no route word, keys at the edges of the key
space with id 2^32 - 1 registered -- with a directory shorter than the id range, and one
actor column holding every registered, deleted, swept and never-registered id, ids past
the directory and the field 0xffffffff.  Each resolver's answer per message must equal
``Model.resolve`` (tests/_registry_model.py); an entry a path cannot carry (a mailbox
>= 2^24, a rank outside the world) is ``no such actor`` with no handler run.  All
comparisons are exact.  Batches: M = 513 (one 512-message scatter tile plus one) and
M = 4096 + 17."""
import numpy as np
import pytest
import torch

import _registry_model as RM
from ptype_amd import ops
from ptype_amd.ops import batch as B
from ptype_amd.ops import hip
from ptype_amd.ops.mailbox import Mailboxes, send_ref
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY as MULM, METHOD_COUNTER_ADD as CADD, METHOD_SEQ_FOLD as FOLDM,
                                   STATUS_NO_ACTOR, STATUS_OK)
from ptype_amd.ops.table import RegistryTable
from ptype_amd.parallel.exchange import ActorExchange
from test_device_kernels import _regions_equal
from test_mailbox_variants_gpu import send as sorted_send
from test_sorted_exchange_gpu import _run_ranks

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U32 = RM.U32
SIZES = [513, 4096 + 17]
N_DIR = {"wrap": 64, "tombs": 64, "values": 20, "keys": 2, "affine1": 51, "affine2": 51}
N_STATE = {"values": 1 << 24}  # (a registered mailbox 2^24 - 1 must be a real state word)
TABLES = ["wrap", "tombs", "values", "keys"]


def ops_of(name):
    if name.startswith("affine"):  # the strided placement for W ranks, one id past the directory, id 2^32 - 1
        W, n = int(name[-1]), N_DIR[name]
        ids = list(range(n))
        return [("upsert", RM._ids(ids + [n + 3, U32]), [i % W for i in ids] + [0, 0],
                 [i // W for i in ids] + [900, 901], None)]
    return RM.scenarios()[name]["ops"]


def build(name, device, directory):
    """The scenario's table on `device` (with its short directory, or none) and its model."""
    cap = 64 if name.startswith("affine") else RM.scenarios()[name]["cap"]
    t, m = RegistryTable(cap, device=device), RM.Model(cap)
    for op in ops_of(name):
        RM.drive(t, m, op)
    if directory:
        t.enable_directory(N_DIR[name], affine_world=int(name[-1]) if name.startswith("affine") else 0)
        if name.startswith("affine"):
            assert t.directory()[2] == int(name[-1])
    return t, m


def actor_column(name, M, seed=0):
    """int64[M] actor fields: every id the ops ever named, never-registered ids, ids on
    both sides of the directory's end, the field 0xffffffff (and 2^32 - 2): each at least
    once, the rest drawn from them."""
    n_dir = N_DIR[name]
    ever = {k - 1 for op in ops_of(name) for k in RM.op_keys(op) if 1 <= k <= 1 << 32}
    base = sorted(ever | {0, 1, 12, n_dir - 1, n_dir, n_dir + 1, 118, 5000, 1 << 24, U32 - 1, U32})
    rng = np.random.default_rng(1000 + seed)
    col = np.concatenate([rng.permutation(base), rng.choice(base, M - len(base))])
    return torch.from_numpy(col.astype(np.int64))


def batch(actors, method, seed, device=DEV, a1=False):
    g = torch.Generator().manual_seed(seed)
    M = actors.numel()
    a0 = torch.randint(-(1 << 15), 1 << 15, (M,), generator=g, dtype=torch.int64)
    c1 = torch.randint(-(1 << 15), 1 << 15, (M,), generator=g, dtype=torch.int64) if a1 else None
    return B.MsgBatch(actors.to(torch.int32).to(device), a0.to(device), None if c1 is None else c1.to(device), None,
                      method)


def want_route(m, actors, R):
    """The model's (rank, mbox) per message as the paths may carry it: rank -1 unless the
    rank is below R and the mailbox below 2^24."""
    rank, mbox = m.resolve_many(actors.numpy())
    ok = (rank >= 0) & (rank < R) & (mbox < RM.MAX_MBOX)
    return torch.from_numpy(np.where(ok, rank, -1)), torch.from_numpy(np.where(ok, mbox, 0))


def test_tables_are_hostile():
    """The columns and tables carry what the module says they do."""
    for name in TABLES:
        _, m = build(name, "cpu", False)
        a = actor_column(name, 513)
        rank, mbox = m.resolve_many(a.numpy())
        assert (rank < 0).any() and (rank == 0).any() and (a == U32).any() and (a >= N_DIR[name]).any()
        a = a.numpy()
        assert ((a < N_DIR[name]) & (rank >= 0)).any() and ((a >= N_DIR[name]) & (rank >= 0)).any()
    _, m = build("keys", "cpu", False)
    assert m.lookup([1 << 32])[0].tolist() == [0] and m.resolve(U32) is None and m.resolve(U32 - 1) == (0, 6)
    _, m = build("values", "cpu", False)
    d = m.dir_words(N_DIR["values"])
    assert (d == RM.DIR_FALLBACK).any() and (d < RM.DIR_FALLBACK).any()  # fallback words inside the directory


# ---------------------------------------------------------------- a. the table's own lookup
@pytest.mark.parametrize("name", TABLES + ["affine2"])
def test_lookup_kernel(name):
    g, m = build(name, DEV, False)
    a = actor_column(name, SIZES[1])
    rank, mbox = g.lookup(a + 1)
    mr, mm = m.lookup((a + 1).numpy())  # by key: key 2^32 is a key like any other here
    assert np.array_equal(rank.cpu().numpy(), mr) and np.array_equal(mbox.cpu().numpy(), mm)
    wr, _ = m.resolve_many(a.numpy())
    field = (a != U32).numpy()
    assert np.array_equal((mr != -1)[field], (wr >= 0)[field])


# ---------------------------------------------------------------- b / c. the routes
def route_both(name, M, directory, tuning, R=2):
    g, m = build(name, DEV, directory)
    c, _ = build(name, "cpu", False)
    a = actor_column(name, M, seed=M)
    req, ref = batch(a, MULM, M, DEV, a1=True), batch(a, MULM, M, "cpu", a1=True)
    C = M
    rsend, rperm, rstats = B.route(ref, c, R, C)
    # the CPU route against the model: delivered iff the paths can carry the model's answer,
    # in message order per destination, with the model's mailbox in the record
    rank, mbox = want_route(m, a, R)
    W = B.FULL_FORMAT.req_words(C)
    for d in range(R):
        idx = torch.nonzero(rank == d).flatten()
        assert rperm[idx].tolist() == (d * C + torch.arange(idx.numel())).tolist()
        got = rsend[d * W + 4:d * W + 4 + idx.numel() * B.FULL_FORMAT.stride:B.FULL_FORMAT.stride]
        assert (got.to(torch.int64) & U32).tolist() == mbox[idx].tolist()
    assert bool((rperm[rank < 0] == -2).all()) and int(rstats[B.STAT_NOMATCH]) == int((rank < 0).sum()) > 0
    for items, mode, pipe in tuning:
        try:
            ops.hip().set_route_tuning(items, mode, pipe)
            for _ in range(2):  # (the look-back epoch must advance cleanly between launches)
                send, perm, stats = B.route(req, g, R, C)
        finally:
            ops.hip().set_route_tuning(0, 0, 0)
        torch.cuda.synchronize()
        what = f"{name} M={M} dir={directory} tuning={(items, mode, pipe)}"
        assert torch.equal(perm.cpu(), rperm), what
        assert _regions_equal(send, rsend, R, C, B.FULL_FORMAT), what
        assert stats.cpu().tolist()[:2] == rstats.tolist()[:2], what


THREE_PASS_DIR = [(1, 0, -1), (2, 0, -1), (4, 0, -1), (8, 0, -1), (0, 0, 0), (8, 0, 0)]


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name", TABLES)
def test_three_pass_route(name, M):
    route_both(name, M, False, [(0, 0, 0), (2, 0, -1)])  # hash probe
    route_both(name, M, True, THREE_PASS_DIR)  # directory, 1 / 2 / 4 / 8 items per thread


@pytest.mark.parametrize("M", SIZES)
def test_three_pass_route_affine(M):
    route_both("affine2", M, True, [(0, 0, 0), (4, 0, -1)])


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name", TABLES)
def test_single_pass_route(name, M):
    route_both(name, M, False, [(0, 1, 0)])
    route_both(name, M, True, [(0, 1, 0)])


def test_probe_stops_at_the_first_empty_slot():
    """A slot image no sequence of ops produces: a key behind an EMPTY slot of its own probe
    group.  The slot-by-slot lookup and the CPU table do not see it; neither may the
    group probes of the routes, the fused pass and the mailbox sends."""
    ids = np.arange(400, dtype=np.int64)
    from ptype_amd.ops import table as T
    start = T.probe_start(T.mix64((ids + 1).astype(np.uint64)), 15)
    x, y, z = ids[start == 4][:3].tolist()
    g, c = RegistryTable(16, device=DEV), RegistryTable(16, device="cpu")
    for t in (g, c):
        img = torch.zeros(16, 2, dtype=torch.int64)
        img[4] = torch.tensor([x + 1, 3 << 32])  # rank 0, mailbox 3
        img[6] = torch.tensor([y + 1, 5 << 32])  # behind the EMPTY slot 5
        img[8] = torch.tensor([z + 1, 7 << 32])  # in the next group
        t.table.copy_(img)
    a = torch.tensor([x, y, z] * 171, dtype=torch.int64)
    assert g.lookup(a[:3] + 1)[0].tolist() == c.lookup(a[:3] + 1)[0].tolist() == [0, -1, -1]
    req, ref = batch(a, MULM, 1, DEV, a1=True), batch(a, MULM, 1, "cpu", a1=True)
    _, rperm, _ = B.route(ref, c, 1, 513)
    assert (rperm >= 0).tolist() == [True, False, False] * 171
    for mode in (0, 1):
        ops.hip().set_route_tuning(0, mode, 0)
        try:
            _, perm, _ = B.route(req, g, 1, 513)
        finally:
            ops.hip().set_route_tuning(0, 0, 0)
        assert torch.equal(perm.cpu(), rperm), f"route mode {mode}"
    want = torch.tensor([STATUS_OK, STATUS_NO_ACTOR, STATUS_NO_ACTOR] * 171, dtype=torch.int32)
    ex = ActorExchange(g, 513, state=torch.zeros(16, dtype=torch.int64, device=DEV), delivery="direct")
    assert torch.equal(ex.send(req)[1].cpu(), want)
    mb = Mailboxes(DEV, shards=16, slots=4096)
    for sort in (False, True):
        _, st = mb.send(req, g, None, sort=sort, ordered=False)
        torch.cuda.synchronize()
        assert torch.equal(st.cpu(), want), f"mailbox send sort={sort}"


# ---------------------------------------------------------------- d / e. world-1 deliveries
class World1:
    """One table (one route) of a scenario with its column, batches and references."""

    def __init__(self, name, kind, M):
        self.name, self.kind, self.M = name, kind, M
        self.t, self.m = build(name, DEV, kind != "hash")
        self.n_state = N_STATE.get(name, 1024)
        self.a = actor_column(name, M, seed=7 * M)
        self.rank, self.mbox = want_route(self.m, self.a, 1)
        g = torch.Generator().manual_seed(M)
        self.state0 = torch.randint(0, 1 << 30, (self.n_state,), generator=g, dtype=torch.int64)

    def ref(self, method, a1=False):
        req = batch(self.a, method, self.M, "cpu", a1=a1)
        state = self.state0.clone()
        val, st = send_ref(req, self.rank, self.mbox, state)
        # no state word other than the model's targets changed
        touched = torch.zeros(self.n_state, dtype=torch.bool)
        touched[self.mbox[(self.rank == 0) & (self.mbox < self.n_state)]] = True
        assert torch.equal(state[~touched], self.state0[~touched])
        return val, st, state

    def check(self, got, method, values=True, what=""):
        val, st, state = got
        rval, rst, rstate = self.ref(method, a1=method == MULM)
        what = f"{self.name}/{self.kind} M={self.M} {what}"
        assert torch.equal(st.cpu(), rst), what
        if values:
            assert torch.equal(val.cpu()[rst == STATUS_OK], rval[rst == STATUS_OK]), what
        if state is not None:
            assert torch.equal(state.cpu(), rstate), what
        assert int((rst == STATUS_OK).sum()) > 0 and int((rst == STATUS_NO_ACTOR).sum()) > 0


W1_CASES = [(n, k) for n in TABLES for k in ("hash", "dir")] + [("affine1", "affine")]


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name,kind", W1_CASES)
def test_world1_fused_pass(name, kind, M):
    """local_send_kernel through ActorExchange at world 1 (hash probe / directory / affine rule)."""
    w = World1(name, kind, M)
    state = w.state0.clone().to(DEV)
    ex = ActorExchange(w.t, M, state=state, delivery="direct")
    val, st = ex.send(batch(w.a, CADD, M))  # commutative: the final state shows where every message ran
    torch.cuda.synchronize()
    w.check((val, st, state), CADD, values=False, what="Counter.Add")
    val, st = ex.send(batch(w.a, MULM, M, a1=True))
    torch.cuda.synchronize()
    w.check((val, st, None), MULM, what="Multiply")


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name,kind", W1_CASES)
def test_world1_tagged_mailbox_enqueue(name, kind, M):
    """mailbox.hip: the tagged reservation enqueue + drain."""
    w = World1(name, kind, M)
    mb = Mailboxes(DEV, shards=16, slots=8192)
    state = w.state0.clone().to(DEV)
    val, st = mb.send(batch(w.a, CADD, M), w.t, state, sort=False, ordered=True)
    torch.cuda.synchronize()
    w.check((val, st, state), CADD, values=False, what="Counter.Add")
    s = mb.stats()
    assert s["overflow"] == 0 and s["holes"] == 0, s


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name,kind", W1_CASES)
def test_world1_sorted_mailbox_ordered_routes_0_1_2(name, kind, M):
    """The sorted mailbox Send of an ordered stateful method: route 0 (hash), 1 (directory,
    the rank byte table withheld) or 2 (affine); SeqFold's replies and final state are
    those of a serial run in message order on the model's mailboxes."""
    w = World1(name, kind, M)
    mb = Mailboxes(DEV, shards=16, slots=8192)
    for sort_mode in (0, 1):
        state = w.state0.clone().to(DEV)
        val, st = sorted_send(mb, w.t, batch(w.a, FOLDM, M), state, True, False, False, True, sort_mode)
        assert mb.last_route == {"hash": 0, "dir": 1, "affine": 2}[kind]
        w.check((val, st, state), FOLDM, what=f"SeqFold sort_mode={sort_mode}")
        s = mb.stats()
        assert s["overflow"] == 0 and s["holes"] == 0, s


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name", TABLES)
def test_world1_sorted_mailbox_stateless_routes_3_4(name, M):
    """Stateless Multiply through the rank byte table (route 3) and the presence map (route
    4, kept and built by the Send).  These routes read one rank byte per id of the
    directory and no mailbox -- the stateless handler needs none -- so an id inside the
    directory is answered by its rank alone (README, parity decisions); ids the byte table
    sends to the hash table and ids past the directory keep the mailbox bound."""
    w = World1(name, "dir", M)
    n_dir = N_DIR[name]
    rank, mbox = w.m.resolve_many(w.a.numpy())
    inside = (w.a.numpy() < n_dir) & (rank < RM.RANK_FALLBACK)
    ok = np.where(inside, rank == 0, (rank == 0) & (mbox < RM.MAX_MBOX))
    req = batch(w.a, MULM, M, a1=True)
    want_st = torch.from_numpy(np.where(ok, STATUS_OK, STATUS_NO_ACTOR).astype(np.int32))
    want_v = (req.a0 * req.a1).cpu()
    mb = Mailboxes(DEV, shards=16, slots=8192)
    try:
        for route, kept, tune in ((3, True, ""), (4, True, "mbox_fused=0"), (4, False, "mbox_fused=0"),
                                  (4, True, "mbox_fused=0,mbox_rec8=1,mbox_persist=1")):
            assert hip().set_tune(tune)
            val, st = sorted_send(mb, w.t, req, None, False, False, True, kept, 0)
            what = f"{name} M={M} route {route} kept={kept} tune={tune!r}"
            assert mb.last_route == route, (what, mb.last_route, mb._m.last_plan["kernels"])
            assert torch.equal(st.cpu(), want_st), what
            assert torch.equal(val.cpu()[ok], want_v[ok]), what
    finally:
        hip().set_tune("")
    assert ok.any() and not ok.all()


# ---------------------------------------------------------------- f. the sorted exchange
@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name,directory", [(n, True) for n in TABLES] + [("tombs", False), ("keys", False)])
def test_sorted_exchange_route_words(name, directory, M):
    """Two in-process ranks, each sending the hostile column with Counter.Add through the
    sorted exchange (sx_count_kernel's route words): every message whose model rank is 0
    or 1 and whose mailbox fits adds to that rank's state word; every other one is ``no
    such actor`` and touches nothing."""
    R = 2
    n_state = N_STATE.get(name, 1024)
    _, m = build(name, "cpu", False)
    cols = [actor_column(name, M, seed=31 * M + r) for r in range(R)]

    def body(r, fc, start, s):
        tab, _ = build(name, DEV, directory)
        st = torch.zeros(n_state, dtype=torch.int64, device=DEV)
        ex = ActorExchange(tab, M, chunks=1, state=st, fake=(fc, r), delivery="mailbox")
        start.wait()
        req = batch(cols[r], CADD, 50 + r)
        # (send_all: a mailbox wider than the start-up layout's field is answered
        # STATUS_OVERFLOW once and re-sent, exactly once, under the layout that grew)
        v, sts = ex.send_all(req)
        s.synchronize()
        return sts.cpu(), st.cpu(), req.a0.cpu(), ex.last_wire["engine"]

    res = _run_ranks(R, body, timeout=60)
    want_state = [torch.zeros(n_state, dtype=torch.int64) for _ in range(R)]
    for r in range(R):
        sts, _, a0, engine = res[r]
        assert engine == "sorted"
        rank, mbox = want_route(m, cols[r], R)
        ok = (rank >= 0) & (mbox < n_state)
        assert torch.equal(sts, torch.where(ok, STATUS_OK, STATUS_NO_ACTOR).to(torch.int32)), f"sender {r}"
        assert bool(ok.any()) and not bool(ok.all())
        for d in range(R):
            sel = ok & (rank == d)
            want_state[d].index_add_(0, mbox[sel], a0[sel])
    for d in range(R):
        assert torch.equal(res[d][1], want_state[d]), f"state of rank {d}"
