"""Device-side sends on every dispatcher, against tests/_outbox_spec.py.

Every kernel that compiles ``run_handler`` with an outbox runs the same hostile Forward
corpus; statuses, replies, the final state, the outbox's count words and the sorted
multiset of emitted records are compared with the spec, exactly.  The outbox's banks are
unaligned views (element offset 1) into larger tensors filled with a sentinel: whatever
lies outside the slots the Send had to fill must still hold it.  Sorted-mailbox cases
also assert that ``last_plan`` names the drain they mean to test.  Every case runs once
more with no outbox bound: senders answer FAILED, the visit counted, the banks untouched.
"""
import threading

import numpy as np
import pytest
import torch

from _outbox_spec import (METHOD_FORWARD, METHOD_SEQ_FOLD, NO_ACTOR, OK, OVERFLOW, corpus_rows, forward_corpus,
                          forward_spec, simulate_pump)
from ptype_amd.ops import batch as B
from ptype_amd.ops import hip
from ptype_amd.ops.mailbox import Mailboxes
from ptype_amd.ops.outbox import DeviceOutbox
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange
from test_outbox_spec import _batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N, NSTATE = 1000, 900
M_LOCAL = 3 * 2048 + 17      # the local pass: three 2048-record stages and a partial tile
M_SORT = 3 * 4096 + 17       # the sorted mailboxes: a first, a middle and a partial last tile
SENT = {torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int16: 0x5A5A}
COLS = (("actor", torch.int32), ("a0", torch.int64), ("a1", torch.int64), ("a2", torch.int64),
        ("method", torch.int16))


class GuardedOutbox(DeviceOutbox):
    """A DeviceOutbox whose bank tensors are views at element offset 1 into sentinel-filled parents."""

    PAD = 5

    def _bank(self) -> dict:
        if not hasattr(self, "parents"):
            self.parents = []
        p = {name: torch.full((self.cap + 1 + self.PAD,), SENT[dt], dtype=dt, device=self.device) for name, dt in COLS}
        p["count"] = torch.tensor([SENT[torch.int64], 0, 0, SENT[torch.int64]], dtype=torch.int64, device=self.device)
        self.parents.append(p)
        b = {name: p[name][1:1 + self.cap] for name, _ in COLS}
        b["count"] = p["count"][1:3]
        return b

    def check_guards(self, filled: int) -> None:
        """Outside the active bank's first ``filled`` slots every parent element is the sentinel."""
        for k, p in enumerate(self.parents):
            n = filled if k == self.active else 0
            for name, dt in COLS:
                t = p[name].cpu()
                bad = torch.nonzero(torch.cat([t[:1], t[1 + n:]]) != SENT[dt]).flatten()
                assert bad.numel() == 0, (k, name, n, (bad[:8] + n).tolist())
            c = p["count"].cpu().tolist()
            assert c[0] == c[3] == SENT[torch.int64] and (k == self.active or c[1:3] == [0, 0]), (k, c)

    def records(self, n: int):
        b = self.bank
        return list(zip((b["actor"][:n].cpu().to(torch.int64) & 0xFFFFFFFF).tolist(), b["method"][:n].cpu().tolist(),
                        b["a0"][:n].cpu().tolist(), b["a1"][:n].cpu().tolist(), b["a2"][:n].cpu().tolist()))


def state0_of(n=NSTATE):
    return (torch.arange(n, dtype=torch.int64) * 1000 + 5)


_tables = {}


def table_of(c, kind="hash", R=1):
    """The registry of a corpus: slot g = mbox_of[id] lives on rank g % R as mailbox g // R."""
    key = (c["mbox_of"].tobytes(), kind, R)
    if key not in _tables:
        n = c["N"]
        t = RegistryTable(4 * n, device=DEV)
        g = torch.from_numpy(c["mbox_of"])
        t.upsert(actor_keys(torch.arange(n)), (g % R).to(torch.int32), (g // R).to(torch.int32))
        if kind == "dir":
            t.enable_directory(n + 50)  # ids n..n+49: in the directory, unregistered
        elif kind == "affine":
            t.enable_directory(n, affine_world=1)
            assert t.directory()[2] == 1
        _tables[key] = t
    return _tables[key]


def verify(sp, ob, bound, st, val, state):
    torch.cuda.synchronize()
    sp.check_replies(st.cpu().tolist(), val.cpu().tolist())
    assert state.cpu().tolist() == sp.state_after
    if not bound:
        assert ob.bank["count"].cpu().tolist() == [0, 0]
        ob.check_guards(0)
        return
    want = sp.outbox_after(ob.cap)
    sp.check_outbox(ob.cap, ob.bank["count"].cpu().tolist(), ob.records(want["filled"]))
    ob.check_guards(want["filled"])


def run_case(c, send, cap_of=lambda E: E + 1, ordered=False, ran_of=None, bounds=(True, False), n_state=NSTATE):
    """``send(batch, state, outbox or None) -> (val, st)`` with and without an outbox bound."""
    batch = _batch(c, DEV)
    first = None
    for bound in bounds:
        ran = None
        state = state0_of(n_state).to(DEV)
        sp = forward_spec(corpus_rows(c), c["resolve"], n_state, state0_of(n_state).tolist(), bound, ordered=ordered)
        ob = GuardedOutbox(max(1, cap_of(sp.E)), device=DEV)
        val, st = send(batch, state, ob if bound else None)
        if ran_of is not None:  # rows the rings had no room for: first checked against the capacity rule
            torch.cuda.synchronize()
            ran = ran_of(st.cpu())
            sp = forward_spec(corpus_rows(c), c["resolve"], n_state, state0_of(n_state).tolist(), bound, ran=ran,
                              ordered=ordered)
        verify(sp, ob, bound, st, val, state)
        first = first or sp
    return first


@pytest.fixture(autouse=True)
def _tune_reset():
    yield
    hip().set_tune("")


# ---------------------------------------------------------------- the fused local pass
def local_send(kind="hash", max_batch=None):
    def send(batch, state, ob):
        ex = ActorExchange(table_of(send.c, kind), max_batch or max(batch.M, 64), state=state)
        ex.outbox = ob
        out = ex.send(batch)
        assert ex._engine is not None
        return out
    return send


def _local(c, kind="hash", **kw):
    s = local_send(kind)
    s.c = c
    return run_case(c, s, **kw)


@pytest.mark.parametrize("mcol", [False, True], ids=["fwd", "mcol"])
@pytest.mark.parametrize("M", [1, 64, 1023, 1024, 1025, 2048, 2049, M_LOCAL])
def test_local_pass(M, mcol):
    assert hip().tune()["local"] != 0
    sp = _local(forward_corpus(M, N, NSTATE, 100 + M, method_column=mcol))
    assert M < 1000 or sp.E > 0


CAPS = {"E": lambda E: E, "E-1": lambda E: E - 1, "E+1": lambda E: E + 1, "1": lambda E: 1,
        "E-1000": lambda E: E - 1000}  # (the last one ends inside one block's flush)


@pytest.mark.parametrize("cap", list(CAPS))
def test_local_pass_outbox_capacity_edges(cap):
    c = forward_corpus(M_LOCAL, N, NSTATE, 7)
    sp = _local(c, cap_of=CAPS[cap], bounds=(True,))
    assert sp.E > 1001


@pytest.mark.parametrize("kind", ["hash", "dir", "affine"])
def test_local_pass_routes(kind):
    _local(forward_corpus(M_LOCAL, N, NSTATE, 8, identity=kind == "affine"), kind)


def test_local_pass_all_lanes_emit():
    """Every row sends: each block's stage fills to its 2048 records before it publishes."""
    sp = _local(forward_corpus(M_LOCAL, N, NSTATE, 9, emit="all"), cap_of=lambda E: E - 1000)
    assert sp.E == M_LOCAL


def test_slot_pipeline_at_world_1(monkeypatch):
    """local=0: route into the epoch slot, then dispatch_kernel over it."""
    monkeypatch.setenv("PTYPE_TUNE", "local=0")
    assert hip().tune()["local"] == 0
    _local(forward_corpus(2049, N, NSTATE, 10))
    _local(forward_corpus(2049, N, NSTATE, 11, method_column=True))


# ---------------------------------------------------------------- v2 dispatch_kernel: the stage's edges
@pytest.mark.parametrize("count, cap", [(1023, None), (1024, None), (1025, None), (3000, None), (3000, 1500)])
def test_v2_dispatch_stage_edges(count, cap):
    """One block walks the whole slot (expected_per_rank=1): 1024 records fill its stage exactly,
    the rest go through the per-wave reservations in HBM; with 1500 slots the drops split
    between the block's flush and those reservations."""
    c = forward_corpus(count, N, NSTATE, 20 + count, emit="all")
    C = count + 8
    fmt = B.FULL_FORMAT

    def send(batch, state, ob):
        sendbuf, perm, _ = B.route(batch, table_of(c), 1, C, fmt=fmt)
        reply = B.dispatch(sendbuf, 1, C, state, fmt=fmt, expected_per_rank=1, outbox=ob)
        return B.complete(reply, perm, C)

    sp = run_case(c, send, cap_of=(lambda E: E + 1) if cap is None else (lambda E: cap))
    assert sp.E == count


# ---------------------------------------------------------------- the mailboxes
def mailbox_send(c, mb, kernels=(), **kw):
    def send(batch, state, ob):
        out = mb.send(batch, table_of(c), state, outbox=ob, **kw)
        torch.cuda.synchronize()
        if kw.get("sort", True):
            launched = mb._m.last_plan["kernels"]
            assert set(kernels) <= set(launched), (kernels, launched)
        s = mb.stats()
        assert s["holes"] == 0, s
        return out
    return send


@pytest.fixture(scope="module")
def rings():
    return Mailboxes(DEV, shards=16, slots=4096)


@pytest.mark.parametrize("ordered, sharding", [(True, "actor"), (False, "actor"), (False, "arrival")])
def test_tagged_rings(rings, ordered, sharding):
    """sort=False: the tagged reservation enqueue with the ordered and the streaming drain.
    (Tiles reserve their ring slots with an atomic each, so a ring's order is message order
    within a tile only: the replies are held to the per-mailbox multiset in both drains.)"""
    c = forward_corpus(5000, N, NSTATE, 30)
    run_case(c, mailbox_send(c, rings, sort=False, ordered=ordered, sharding=sharding))


SORTED = {
    # case: (tune, corpus knobs, send arguments, kernels the plan must name)
    "fused": ("", {}, {}, ["mbx_sortdrain_kernel<0, true, false, 0, 0>"]),
    "fused-two_args": ("", {"two_args": True}, {}, ["mbx_sortdrain_kernel<0, false, false, 0, 0>"]),
    "fused-mcol": ("", {"method_column": True}, {}, ["mbx_sortdrain_kernel<0, true, true, 0, 0>"]),
    "ring": ("mbox_fused=0", {}, {}, ["mbx_onesweep_kernel<0, true, false>", "mbx_drain_ring_kernel<0, true, 0>"]),
    "ring-two_args": ("mbox_fused=0", {"two_args": True}, {},
                      ["mbx_onesweep_kernel<0, false, false>", "mbx_drain_ring_kernel<0, true, 0>"]),
    "msg": ("mbox_drain_msg=1", {}, {}, ["mbx_onesweep_kernel<0, true, false>", "mbx_drain_msg_kernel<0>"]),
    "twopass": ("", {}, {"sort_mode": "twopass"},
                ["mbx_count_kernel<0>", "mbx_scatter_kernel<true, false>", "mbx_drain_ring_kernel<0, true, 0>"]),
    "ordered": ("", {}, {"ordered": True},
                ["mbx_drain_ordered_kernel<true, kOrdK, 0, false, false>", "mbx_complete_ring_kernel<>"]),
    "ordered-two_args": ("", {"two_args": True}, {"ordered": True},
                         ["mbx_drain_ordered_kernel<true, kOrdK, 0, false, false>", "mbx_complete_ring_kernel<>"]),
    "arrival": ("", {}, {"sharding": "arrival"},
                ["mbx_arrival_enqueue_kernel<0, true, false>", "mbx_arrival_drain_kernel<0, 0>"]),
    "arrival-mcol": ("", {"method_column": True}, {"sharding": "arrival"},
                     ["mbx_arrival_enqueue_kernel<0, true, true>", "mbx_arrival_drain_kernel<0, 0>"]),
    "arrival-fused": ("", {"two_args": True}, {"sharding": "arrival"}, ["mbx_arrival_fused_kernel<0, 0, 2>"]),
    "arrival-two_args": ("mbox_fused=0", {"two_args": True}, {"sharding": "arrival"},
                         ["mbx_arrival_enqueue_kernel<0, false, false>", "mbx_arrival_drain_kernel<0, 0>"]),
}


@pytest.mark.parametrize("case", list(SORTED))
def test_sorted_mailboxes(rings, case):
    tune, knobs, args, kernels = SORTED[case]
    assert hip().set_tune(tune)
    c = forward_corpus(M_SORT, N, NSTATE, 40, **knobs)
    ordered = bool(args.get("ordered"))
    run_case(c, mailbox_send(c, rings, kernels, **({"ordered": False} | args)), ordered=ordered)


def test_sorted_ordered_windows_seqfold_and_forward(rings):
    """A method column of SeqFold and Forward through the ordered windows: every reply exact,
    each mailbox's rows run one at a time in message order."""
    c = forward_corpus(M_SORT, N, NSTATE, 41)
    rng = np.random.default_rng(41)
    c["method"] = np.where(rng.random(M_SORT) < 0.4, METHOD_SEQ_FOLD, METHOD_FORWARD).astype(np.int64)
    kernels = ["mbx_scatter_kernel<true, true>", "mbx_drain_ordered_kernel<true, kOrdK, 0, false, false>"]
    sp = run_case(c, mailbox_send(c, rings, kernels, ordered=True), ordered=True)
    assert all(v is not None for v, s in zip(sp.value, sp.status) if s == OK)


def test_sorted_8_byte_records(rings):
    """8-B ring records (two arguments, one method): the rows whose a0 is too wide for the
    record's fields spill to the drain and still emit exactly once."""
    assert hip().set_tune("mbox_rec8=1,mbox_fused=0")
    c = forward_corpus(M_SORT, N, NSTATE, 42, two_args=True, narrow=True)
    kernels = ["mbx_onesweep_kernel<0, false, false>", "mbx_drain_ring_kernel<0, true, 1>"]
    seen = []

    def send(batch, state, ob):
        # (fresh rings: a Send whose values outgrow the 8-B fields moves the next one to 16-B records)
        mb = Mailboxes(DEV, shards=16, slots=4096)
        out = mailbox_send(c, mb, kernels, ordered=False)(batch, state, ob)
        seen.append((mb.last_record_bytes, mb.stats()["spilled"]))
        return out

    run_case(c, send)
    assert seen[0][0] == 8 and seen[0][1] > 0, seen


def test_ring_full_spill():
    """Stateless drain, rings far smaller than the batch: the rows past the rings run from the
    batch; none answers OVERFLOW and each sender emits exactly once."""
    c = forward_corpus(M_SORT, N, NSTATE, 43)
    mb = Mailboxes(DEV, shards=4, slots=1024)
    sp = run_case(c, mailbox_send(c, mb, ordered=False))
    assert mb.stats()["spilled"] > 0 and OVERFLOW not in sp.status


def test_ring_full_overflow_ordered():
    """Ordered drain, rings of 1024 slots: exactly the rows past each ring's capacity, in message
    order, answer OVERFLOW -- no visit, no emit -- and the rest behave as the spec says."""
    c = forward_corpus(M_SORT, N, NSTATE, 44)
    mb = Mailboxes(DEV, shards=4, slots=1024)
    mbox = np.array([-1 if m is None else m for m in c["resolve"]])
    want_ran = np.ones(M_SORT, bool)
    for s in range(4):
        idx = np.nonzero((mbox >= 0) & (mbox % 4 == s))[0]
        assert len(idx) > 1024
        want_ran[idx[1024:]] = False

    def ran_of(st):
        over = (st == OVERFLOW).numpy()
        assert np.array_equal(over, ~want_ran), np.nonzero(over != ~want_ran)[0][:8]
        return ~over

    sp = run_case(c, mailbox_send(c, mb, ordered=True), ordered=True, ran_of=ran_of)
    assert sp.status.count(OVERFLOW) == int((~want_ran).sum()) > 0


# ---------------------------------------------------------------- the engine across ranks (in-process ranks)
def run_ranks(R, corpora, n_state, bound, **ex_kw):
    """One ``send`` per rank (FakeComm ranks on threads); returns per rank (val, st, state, outbox)
    and the per-destination specs over the concatenation of every rank's rows."""
    cat = lambda k: (None if corpora[0][k] is None else np.concatenate([c[k] for c in corpora]))  # noqa: E731
    method = corpora[0]["method"] if isinstance(corpora[0]["method"], int) else cat("method")
    rows = (cat("actor"), method, cat("a0"), cat("a1"), cat("a2"))
    slot = [g for c in corpora for g in c["resolve"]]
    specs = []
    for d in range(R):
        res = [g // R if g is not None and g % R == d else None for g in slot]
        specs.append(forward_spec(rows, res, n_state, (state0_of(n_state) + d).tolist(), bound))
    fc = hip().FakeComm(R)
    out, errors, start = [None] * R, [], threading.Barrier(R)
    Mmax = max(len(c["a0"]) for c in corpora)

    def run(r):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                state = (state0_of(n_state) + r).to(DEV)
                ob = GuardedOutbox(specs[r].E + 3, device=DEV)
                ex = ActorExchange(table_of(corpora[0], "hash", R), 2 * Mmax, state=state, fake=(fc, r), **ex_kw)
                ex.outbox = ob if bound else None
                req = _batch(corpora[r], DEV)
                s.synchronize()
                start.wait()
                val, st = ex.send(req)
                s.synchronize()
                out[r] = (val.cpu(), st.cpu(), state, ob, ex)
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errors.append((r, repr(e)))
            start.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(R)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank hung"
    assert not errors, errors
    torch.cuda.synchronize()
    val = torch.cat([o[0] for o in out]).tolist()
    st = torch.cat([o[1] for o in out]).tolist()
    assert OVERFLOW not in st  # (the slots and rings were sized so that nothing overflows)
    for i, g in enumerate(slot):
        want = NO_ACTOR if g is None else specs[g % R].status[i]
        assert st[i] == want, (i, st[i], want)
    for d in range(R):
        sp, (_, _, state, ob, ex) = specs[d], out[d]
        sp.check_values(val)
        assert state.cpu().tolist() == sp.state_after, d
        if bound:
            sp.check_outbox(ob.cap, ob.bank["count"].cpu().tolist(), ob.records(sp.E))
            ob.check_guards(sp.E)
        else:
            assert ob.bank["count"].cpu().tolist() == [0, 0]
            ob.check_guards(0)
        if ex.mailboxes is not None:
            assert ex.mailboxes.stats()["holes"] == 0
    return specs, out


def rank_corpora(R, M, n_state, seed, **knobs):
    """One corpus per rank over the same registry (same seed-0 permutation, other rows)."""
    base = forward_corpus(M, N, n_state * R, seed, **knobs)
    out = [base]
    for r in range(1, R):
        c = forward_corpus(M, N, n_state * R, seed, **knobs)
        p = np.random.default_rng(seed + r).permutation(M)  # the same rows in another order, other a0
        for k in ("actor", "a0", "a1", "a2", "emits"):
            c[k] = None if c[k] is None else c[k][p]
        if not isinstance(c["method"], int):
            c["method"] = c["method"][p]
        c["resolve"] = [c["resolve"][i] for i in p]
        out.append(c)
    return out


@pytest.mark.parametrize("bound", [True, False], ids=["outbox", "none"])
@pytest.mark.parametrize("packed", [True, False], ids=["v3", "v2"])
def test_engine_dispatch_two_ranks(packed, bound):
    """dispatch_packed_kernel (wire v3) and the engine's v2 dispatch_kernel, 2049 rows per rank."""
    specs, _ = run_ranks(2, rank_corpora(2, 2049, 420, 50), 420, bound, packed=packed, delivery="direct")
    assert not bound or all(sp.E > 0 for sp in specs)


def test_engine_dispatch_four_ranks_one_destination():
    """Every rank sends 1024 sending rows to rank 0's actors: the one block that serves a
    source region there (expected rows per rank: 256) stages exactly 1024 records."""
    R, n_state = 4, 200
    corpora = []
    for r in range(R):
        c = forward_corpus(1024, N, n_state * R, 60, emit="all")
        on0 = np.nonzero((c["mbox_of"] % R == 0) & (c["mbox_of"] // R < n_state))[0]
        c["actor"] = on0[np.random.default_rng(60 + r).integers(0, len(on0), 1024)].astype(np.int32)
        c["resolve"] = [int(c["mbox_of"][a]) for a in c["actor"]]
        corpora.append(c)
    specs, _ = run_ranks(R, corpora, n_state, True, packed=True, delivery="direct")
    assert [sp.E for sp in specs] == [4096, 0, 0, 0]


@pytest.mark.parametrize("bound", [True, False], ids=["outbox", "none"])
@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "streaming"])
@pytest.mark.parametrize("packed", [True, False], ids=["v3", "v2"])
def test_engine_mailbox_on_receipt(packed, ordered, bound, monkeypatch):
    """delivery="mailbox" on the epoch engine: K2 from the received regions, then the tagged
    drains with the rank's outbox."""
    monkeypatch.setenv("PTYPE_TUNE", "sorted_exchange=0")  # (the sorted exchange takes no outbox)
    specs, out = run_ranks(2, rank_corpora(2, 2049, 420, 51), 420, bound, packed=packed, delivery="mailbox",
                           mailbox_ordered=ordered, mailbox_shards=16, mailbox_slots=4096)
    assert all(o[4].mailboxes is not None and not o[4]._last_sorted for o in out)


# ---------------------------------------------------------------- end to end: the host pump through the mailboxes
def test_mailbox_pump_end_to_end():
    c = forward_corpus(5000, N, NSTATE, 70, max_a1=3)
    epochs, delivered, final = simulate_pump(c, state0_of().tolist())
    assert epochs >= 2
    state = state0_of().to(DEV)
    ex = ActorExchange(table_of(c), 16384, state=state, delivery="mailbox", mailbox_shards=16, mailbox_slots=4096)
    ob = GuardedOutbox(16384, device=DEV)
    got = ex.pump(ob, initial=_batch(c, DEV))
    torch.cuda.synchronize()
    assert got == (epochs, delivered) and ob.dropped == 0
    assert state.cpu().tolist() == final
    assert ex.mailboxes.stats()["holes"] == 0
