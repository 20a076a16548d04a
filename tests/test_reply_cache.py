"""The reply cache on CPU tensors (``ops/reply_cache.py``): the host reference
against a dict model written here, the key, the direct-mapped slot and winner
rules, what is never stored, ``clear()`` and both 32-bit wraps; then the runtime's
``cache=`` switch (repeat Sends, stateful methods, stale statuses, coalescing,
retries, a ledger, capture), the public API and the ``gpu.cache`` /
``gpu.cache_entries`` config keys.  All comparisons are exact integer equality."""
import time

import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import coalesce as CO
from ptype_amd.ops import ledger as L
from ptype_amd.ops import reply_cache as RC
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_ECHO, METHOD_PRIME_CHECK,
                                   METHOD_RETRY_TEST, METHOD_SEQ_FOLD, PURE_METHODS, STATUS_FAILED, STATUS_NO_ACTOR,
                                   STATUS_OK)
from ptype_amd.ops.table import actor_keys

from test_coalesce import multiply_batch, random_batch, retry_mix, runtime
from test_send_retries import join_world1

U32 = 0xFFFFFFFF


# ---------------------------------------------------------------- a dict model of the table
def rows_of(batch):
    """Every message's key as Python ints: (actor u32, method u16, a0, a1, a2)."""
    M = batch.M
    actor = batch.actor.numpy().view(np.uint32).tolist()
    method = ([batch.method & 0xFFFF] * M if isinstance(batch.method, int)
              else batch.method.numpy().view(np.uint16).tolist())
    arg = (lambda t: [0] * M if t is None else t.tolist())
    return list(zip(actor, method, arg(batch.a0), arg(batch.a1), arg(batch.a2)))


def home(key, entries):
    return int(CO.key_hash(np.array([key[0]], dtype=np.uint32), key[1], key[2], key[3], key[4])[0]) & (entries - 1)


class DictCache:
    """slot -> (key, value): the newest insert replaces, the lowest row of an insert wins."""

    def __init__(self, entries):
        self.entries, self.slots = entries, {}

    def lookup(self, batch):
        out = []
        for key in rows_of(batch):
            e = self.slots.get(home(key, self.entries)) if key[1] in PURE_METHODS else None
            out.append((e[1], STATUS_OK) if e is not None and e[0] == key else (None, RC.PENDING))
        return out

    def insert(self, sub, val, st):
        taken = set()
        for key, v, s in zip(rows_of(sub), val.tolist(), st.tolist()):
            slot = home(key, self.entries)
            if key[1] in PURE_METHODS and s == STATUS_OK and slot not in taken:
                taken.add(slot)
                self.slots[slot] = (key, v)

    def clear(self):
        self.slots = {}


def fake_replies(sub):
    """A stand-in for the inner Send: a value from the arguments, every fifth a0 failing."""
    z = torch.zeros(sub.M, dtype=torch.int64)
    val = sub.a0 * 3 + (z if sub.a1 is None else sub.a1) * 5 + (z if sub.a2 is None else sub.a2) * 7 + 11
    st = torch.where(sub.a0 % 5 == 0, STATUS_FAILED, STATUS_OK).to(torch.int32)
    return val, st


def expected_counters(steps, entries):
    """What a cached runtime counts for ``steps`` -- batches whose every call answers
    STATUS_OK, and "clear" -- worked out by the host reference: ``key_hash`` decides
    which keys share a slot, so the hit count is exact."""
    ref = RC.ReplyCacheRef(entries=entries)
    ok = (lambda sub: (sub.a0.clone(), torch.zeros(sub.M, dtype=torch.int32)))
    for b in steps:
        if isinstance(b, str):
            ref.clear()
        else:
            ref.send(b, ok)
    return dict(ref.counters, entries=ref.entries)


def step(cache, model, batch):
    """One cached Send on the ops level against the dict model; returns (hits, K)."""
    val, st = cache.lookup(batch)
    want = model.lookup(batch)
    assert st.dtype == torch.int32 and st.tolist() == [s for _, s in want]
    hit = st == STATUS_OK
    assert val[hit].tolist() == [v for v, s in want if s == STATUS_OK]
    idx = torch.nonzero(~hit).flatten()
    sub = batch.index_select(idx)
    v2, s2 = fake_replies(sub)
    cache.insert(sub, v2, s2)
    model.insert(sub, v2, s2)
    return int(hit.sum()), sub.M


def check_table(cache, model):
    """The valid entries of the table are exactly the model's slots."""
    w = cache.words()
    valid = np.flatnonzero((w[:, RC.W_EPOCH] & np.uint64(U32)) == np.uint64(cache.epoch))
    assert sorted(valid.tolist()) == sorted(model.slots)
    for slot, (key, v) in model.slots.items():
        e = w[slot]
        assert int(e[RC.W_K0]) == key[0] | key[1] << 32
        assert [int(x) for x in e[[RC.W_A0, RC.W_A1, RC.W_A2, RC.W_VALUE]].view(np.int64)] == list(key[2:]) + [v]


@pytest.mark.parametrize("entries", [1 << 4, 1 << 8, 1 << 12])
@pytest.mark.parametrize("M", [0, 1, 65, 1500])
def test_reference_against_a_dict_model(M, entries):
    cache, model = RC.ReplyCacheRef(entries=entries), DictCache(entries)
    hits = 0
    for send in range(3):
        kw = ({}, {"a2": False}, {"a1": False, "a2": False, "methods": METHOD_PRIME_CHECK})[send]
        h, K = step(cache, model, random_batch(M, 10 * M + send, **kw))
        hits += h
        check_table(cache, model)
    if M == 1500 and entries == 1 << 12:
        assert hits > 300  # (the inputs: Send 2 repeats keys of Send 1)
    assert cache.seq == 3 and cache.epoch == 1


def test_entries_are_rounded_and_clamped():
    for n, want in ((0, 4), (1, 4), (16, 4), (17, 5), (1000, 10), (1 << 20, 20), ((1 << 20) + 1, 21), (1 << 40, 26)):
        assert RC.entries_log2(n) == want
    c = RC.ReplyCacheRef(entries=1000)
    assert c.entries == 1024 and c.words().shape == (1024, 8) and RC.DEFAULT_ENTRIES == 1 << 20
    assert bool((c.words()[:, RC.W_CLAIM] == np.uint64((1 << 64) - 1)).all())  # cleared: claim all ones, epoch 0
    assert int(c.words().sum(dtype=np.uint64)) == (1024 * ((1 << 64) - 1)) % (1 << 64)


def _one(actor, method, a0, a1=None, a2=None, column=False):
    t = (lambda x: None if x is None else torch.tensor([x], dtype=torch.int64))
    m = torch.tensor([method], dtype=torch.int16) if column else method
    return MsgBatch(torch.tensor([actor], dtype=torch.int32), t(a0), t(a1), t(a2), m)


def test_each_key_field_alone_distinguishes_two_keys():
    i64 = torch.iinfo(torch.int64)
    base = (7, METHOD_ECHO, 3, 4, 5)
    others = [(7 - 2**31, METHOD_ECHO, 3, 4, 5), (7, METHOD_CALC_MULTIPLY, 3, 4, 5), (7, METHOD_ECHO, 3 + (1 << 32), 4, 5),
              (7, METHOD_ECHO, 3, i64.min, 5), (7, METHOD_ECHO, 3, 4, -1)]
    for other in others:
        # in a table of 16 two keys often share the slot: the hit must come from the field compare
        for entries in (16, 1 << 12):
            c = RC.ReplyCacheRef(entries=entries)
            c.insert(_one(*base), torch.tensor([99]), torch.tensor([STATUS_OK], dtype=torch.int32))
            assert c.lookup(_one(*base))[1].tolist() == [STATUS_OK] and c.lookup(_one(*base))[0].tolist() == [99]
            assert c.lookup(_one(*other))[1].tolist() == [RC.PENDING], other


def test_missing_columns_are_zero_and_a_uniform_method_is_a_column():
    c = RC.ReplyCacheRef(entries=64)
    c.insert(_one(2, METHOD_ECHO, 9), torch.tensor([9]), torch.tensor([STATUS_OK], dtype=torch.int32))
    for b in (_one(2, METHOD_ECHO, 9, 0), _one(2, METHOD_ECHO, 9, None, 0), _one(2, METHOD_ECHO, 9, 0, 0),
              _one(2, METHOD_ECHO, 9, column=True), _one(2, METHOD_ECHO, 9, 0, 0, column=True)):
        assert c.lookup(b)[1].tolist() == [STATUS_OK] and c.lookup(b)[0].tolist() == [9]
    assert c.lookup(_one(2, METHOD_ECHO, 9, 1))[1].tolist() == [RC.PENDING]
    w1 = c.words().copy()
    d = RC.ReplyCacheRef(entries=64)
    d.insert(_one(2, METHOD_ECHO, 9, 0, 0, column=True), torch.tensor([9]), torch.tensor([STATUS_OK], dtype=torch.int32))
    assert np.array_equal(d.words(), w1)


def colliding_keys(entries, n=2, method=METHOD_CALC_MULTIPLY, actor=9):
    """``n`` distinct a0 whose keys (actor, method, a0, 5, 0) share one home slot."""
    cand = np.arange(100_000, dtype=np.int64)
    slot = CO.key_hash(actor, method, cand, 5, 0) & np.uint64(entries - 1)
    same = cand[slot == slot[0]][:n]
    assert same.size == n
    return [int(x) for x in same], int(slot[0])


def test_slot_collisions_evict_the_older_and_the_lower_row_wins():
    entries = 1 << 4
    (x, y, z), slot = colliding_keys(entries, 3)
    ok = (lambda n: torch.full((n,), STATUS_OK, dtype=torch.int32))
    mk = (lambda a0s: MsgBatch(torch.full((len(a0s),), 9, dtype=torch.int32), torch.tensor(a0s),
                               torch.full((len(a0s),), 5), None, METHOD_CALC_MULTIPLY))
    c = RC.ReplyCacheRef(entries=entries)
    c.insert(mk([x]), torch.tensor([5 * x]), ok(1))
    assert c.lookup(mk([x, y]))[1].tolist() == [STATUS_OK, RC.PENDING]
    # a newer Send's key with the same home slot evicts it
    c.insert(mk([y]), torch.tensor([5 * y]), ok(1))
    val, st = c.lookup(mk([x, y]))
    assert st.tolist() == [RC.PENDING, STATUS_OK] and int(val[1]) == 5 * y
    # within one Send the lowest row wins, whatever the order of the keys
    c.insert(mk([z, x, y]), torch.tensor([5 * z, 5 * x, 5 * y]), ok(3))
    val, st = c.lookup(mk([x, y, z]))
    assert st.tolist() == [RC.PENDING, RC.PENDING, STATUS_OK] and int(val[2]) == 5 * z
    e = c.words()[slot]
    assert int(e[RC.W_CLAIM]) == (U32 - 2) << 32 | 0 and int(e[RC.W_A0]) == z and int(e[RC.W_EPOCH]) == 1
    # a row that may not be stored does not take the slot from a higher row
    c.insert(mk([x, y]), torch.tensor([5 * x, 5 * y]), torch.tensor([STATUS_FAILED, STATUS_OK], dtype=torch.int32))
    assert c.lookup(mk([x, y, z]))[1].tolist() == [RC.PENDING, STATUS_OK, RC.PENDING]
    assert int(c.words()[slot][RC.W_CLAIM]) == (U32 - 3) << 32 | 1


def test_non_pure_and_non_ok_replies_are_never_stored():
    M = 300
    ids = torch.arange(M, dtype=torch.int32) % 7
    a = torch.arange(M, dtype=torch.int64)
    blank = RC.ReplyCacheRef(entries=256).words().copy()
    for m in (0, METHOD_RETRY_TEST, METHOD_COUNTER_ADD, METHOD_SEQ_FOLD, 0x7E, 0x7FFF, -1):
        for method in (m, torch.full((M,), m, dtype=torch.int16)):
            c = RC.ReplyCacheRef(entries=256)
            b = MsgBatch(ids, a, a, None, method)
            c.insert(b, a, torch.zeros(M, dtype=torch.int32))
            assert np.array_equal(c.words(), blank), m
            assert bool((c.lookup(b)[1] == RC.PENDING).all())
    for s in (1, 2, 3, 4, 5, 6, RC.PENDING, -1):
        c = RC.ReplyCacheRef(entries=256)
        b = MsgBatch(ids, a, a, None, METHOD_ECHO)
        c.insert(b, a, torch.full((M,), s, dtype=torch.int32))
        assert np.array_equal(c.words(), blank), s
    # a method column: the Echo rows with STATUS_OK only
    col = torch.tensor([METHOD_ECHO, METHOD_COUNTER_ADD], dtype=torch.int16)[torch.arange(M) % 2]
    st = torch.where(torch.arange(M) % 3 == 0, STATUS_OK, STATUS_NO_ACTOR).to(torch.int32)
    c = RC.ReplyCacheRef(entries=1 << 12)
    b = MsgBatch(ids, a, None, None, col)
    c.insert(b, a, st)
    got = c.lookup(b)[1]
    want = (col == METHOD_ECHO) & (st == STATUS_OK)
    assert int(want.sum()) == M // 6 and torch.equal(got == STATUS_OK, want)  # (no two of these keys share a slot)


def test_clear_and_both_wraps():
    ok = (lambda n: torch.full((n,), STATUS_OK, dtype=torch.int32))
    b = MsgBatch(torch.arange(8, dtype=torch.int32), torch.arange(8, dtype=torch.int64), None, None, METHOD_ECHO)
    c = RC.ReplyCacheRef(entries=1 << 10)
    c.clear()  # before the table exists: nothing to do
    assert c.epoch == 1 and c.counters["clears"] == 1
    c.insert(b, b.a0, ok(8))
    before = c.words().copy()
    assert bool((c.lookup(b)[1] == STATUS_OK).all())
    c.clear()  # O(1): the table is untouched, nothing matches
    assert c.epoch == 2 and np.array_equal(c.words(), before) and bool((c.lookup(b)[1] == RC.PENDING).all())
    c.insert(b, b.a0 + 1, ok(8))  # the stale entries' claims lose to the newer insert
    assert c.lookup(b)[0].tolist() == (b.a0 + 1).tolist()
    # the epoch wrap: clear() at 0xFFFFFFFF rewrites the table and starts over
    c = RC.ReplyCacheRef(entries=1 << 10, _start=(U32 - 1, 5))
    c.insert(b, b.a0, ok(8))
    c.clear()
    assert c.epoch == U32 and bool((c.lookup(b)[1] == RC.PENDING).all())
    c.insert(b, b.a0, ok(8))
    assert bool((c.lookup(b)[1] == STATUS_OK).all())
    c.clear()
    assert (c.epoch, c.seq) == (1, 0) and np.array_equal(c.words(), RC.ReplyCacheRef(entries=1 << 10).words())
    c.insert(b, b.a0, ok(8))
    assert bool((c.lookup(b)[1] == STATUS_OK).all()) and c.seq == 1
    # the sequence wrap: seq 0xFFFFFFFF is used (claim high word 0), the next insert rewrites first
    c = RC.ReplyCacheRef(entries=1 << 10, _start=(7, U32 - 1))
    c.insert(b.slice(0, 4), b.a0[:4], ok(4))
    c.insert(b.slice(4, 8), b.a0[4:], ok(4))
    assert c.seq == U32 + 1 and bool((c.lookup(b)[1] == STATUS_OK).all())
    claims = c.words()[:, RC.W_CLAIM]
    assert sorted(int(x) for x in claims[claims != np.uint64((1 << 64) - 1)]) == [0, 1, 2, 3] + [
        1 << 32 | r for r in range(4)]
    c.insert(b.slice(0, 2), b.a0[:2] + 40, ok(2))
    assert (c.epoch, c.seq) == (1, 1)
    val, st = c.lookup(b)
    assert st.tolist() == [STATUS_OK] * 2 + [RC.PENDING] * 6 and val[:2].tolist() == [40, 41]
    with pytest.raises(ValueError):
        RC.ReplyCacheRef(_start=(0, 0))
    with pytest.raises(ValueError):
        c.insert(b, b.a0[:3], ok(3))


def test_send_calls_the_inner_send_once_or_never():
    calls = []

    def inner(sub):
        calls.append(sub.M)
        return fake_replies(sub)

    b = MsgBatch(torch.arange(40, dtype=torch.int32), torch.arange(40, dtype=torch.int64) * 5 + 1, None, None,
                 METHOD_ECHO)  # (a0 % 5 == 1: fake_replies answers STATUS_OK)
    c = RC.ReplyCache("cpu", entries=1 << 12)
    first = c.send(b, inner)
    assert calls == [40] and torch.equal(first[0], fake_replies(b)[0])
    again = c.send(b, inner)  # all hits: the inner Send is skipped
    assert calls == [40] and torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    again = c.send(b, inner, collective=True)  # all hits on a rank of a group: an empty batch goes out
    assert calls == [40, 0] and torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    half = MsgBatch(torch.arange(20, 60, dtype=torch.int32), torch.arange(20, 60, dtype=torch.int64) * 5 + 1, None,
                    None, METHOD_ECHO)
    out = c.send(half, inner)
    assert calls == [40, 0, 20] and torch.equal(out[0], fake_replies(half)[0])
    add = MsgBatch(b.actor, b.a0, None, None, METHOD_COUNTER_ADD)  # a uniform non-pure method: the batch as it is
    table = c.words().copy()
    out = c.send(add, inner)
    assert calls[-1] == 40 and np.array_equal(c.words(), table)
    assert c.counters == {"sends": 5, "messages": 200, "hits": 100, "sent": 100, "clears": 0}


# ---------------------------------------------------------------- a CPU runtime
def test_runtime_second_send_is_all_hits_cpu():
    M, keys = 5000, 300
    b = multiply_batch(M, keys, 64)
    rt = runtime()
    plain = rt.send("calculator", b)
    assert rt._cache is None  # a Send without the option creates nothing
    assert rt.stats()["cache"] == {"sends": 0, "messages": 0, "hits": 0, "sent": 0, "clears": 0, "entries": 0}
    sent = rt.exchange.counters.sent
    val, st = rt.send("calculator", b, cache=True)
    assert torch.equal(val, plain[0]) and torch.equal(st, plain[1]) and bool((st == STATUS_OK).all())
    assert rt.exchange.counters.sent - sent == M  # cold: every message is a miss (duplicates included)
    val, st = rt.send("calculator", b, cache=True)
    assert torch.equal(val, plain[0]) and torch.equal(st, plain[1])
    assert rt.exchange.counters.sent - sent == M  # nothing was sent
    assert rt.stats()["cache"] == {"sends": 2, "messages": 2 * M, "hits": M, "sent": M, "clears": 0,
                                   "entries": 1 << 20}
    rt.send("calculator", b, cache=False)
    rt.send("calculator", b)  # None: the runtime's default, off
    assert rt.stats()["cache"]["sends"] == 2
    val, st = rt.send("calculator", b.slice(0, 0), cache=True)  # an empty Send
    assert val.numel() == 0 and st.numel() == 0 and rt.stats()["cache"]["sends"] == 3
    rt.cache_clear()
    rt.send("calculator", b, cache=True)
    assert rt.stats()["cache"]["sent"] == 2 * M and rt.stats()["cache"]["clears"] == 1
    rt.close()
    # the runtime default and the table size
    rt = runtime(cache=True, cache_entries=1000)
    rt.send("calculator", b)
    val, st = rt.send("calculator", b)
    assert torch.equal(val, plain[0]) and rt.stats()["cache"]["entries"] == 1024
    assert 0 < rt.stats()["cache"]["hits"] <= M  # (300 keys in 1024 direct-mapped slots: some evict each other)
    rt.send("calculator", b, cache=False)
    assert rt.stats()["cache"]["sends"] == 2
    rt.close()


def test_an_all_hit_rank_of_a_group_joins_with_an_empty_send_cpu():
    """At world > 1 the runtime's cached Send reaches ``_send`` exactly once, with an
    empty batch when everything hit (here the world is only claimed: the exchange
    stays the local one)."""
    rt = runtime()
    b = multiply_batch(500, 50, 64)
    rt.exchange  # (built at world 1)
    rt.world = 2
    calls, inner = [], rt._send

    def counted(service, sub, *a, **kw):
        calls.append((sub.M, kw.get("final")))
        return inner(service, sub, *a, **kw)

    rt._send = counted
    first = rt.send("calculator", b, cache=True)
    again = rt.send("calculator", b, cache=True)
    assert calls == [(500, True), (0, True)]
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    assert rt.stats()["cache"]["hits"] == 500 and rt.stats()["cache"]["sent"] == 500
    rt.close()


def test_no_cache_object_without_the_option_cpu():
    rt = runtime(coalesce=True, ledger=True)
    b = multiply_batch(500, 50, 64)
    rt.send("calculator", b)
    rt.send("calculator", b, retries=1)
    rt.send("calculator", b, coalesce=False)
    rt.cache_clear()
    assert rt._cache is None and rt.cache is False
    rt.close()


def test_stateful_methods_run_every_time_cpu():
    M = 400
    g = torch.Generator().manual_seed(1)
    col = torch.tensor([METHOD_COUNTER_ADD, METHOD_CALC_MULTIPLY, METHOD_SEQ_FOLD], dtype=torch.int16)[
        torch.randint(0, 3, (M,), generator=g)]
    b = MsgBatch(torch.randint(0, 8, (M,), generator=g).to(torch.int32), torch.randint(1, 4, (M,), generator=g),
                 torch.randint(1, 4, (M,), generator=g), None, col)
    rt, rt_plain = runtime(), runtime()
    for send in range(2):
        want = rt_plain.send("calculator", b)
        val, st = rt.send("calculator", b, cache=True)
        assert torch.equal(val, want[0]) and torch.equal(st, want[1]) and torch.equal(rt.state, rt_plain.state), send
    mul = int((col == METHOD_CALC_MULTIPLY).sum())
    assert rt.stats()["cache"]["hits"] == mul and rt.stats()["cache"]["sent"] == 2 * M - mul
    # Counter.Add alone: its state advances once per appearance in both Sends
    add = MsgBatch(torch.full((M,), 5, dtype=torch.int32), torch.ones(M, dtype=torch.int64), None, None,
                   METHOD_COUNTER_ADD)
    s0 = int(rt.state[5])
    rt.send("calculator", add, cache=True)
    rt.send("calculator", add, cache=True)
    assert int(rt.state[5]) == s0 + 2 * M
    rt.close()
    rt_plain.close()


def _until(cond, what, limit=10.0):
    t0 = time.time()
    while not cond():
        assert time.time() - t0 < limit, what
        time.sleep(0.02)


def stale_status_scenario(c, rt, client, dev="cpu"):
    """Cache an OK reply, delete the actor's shard record: the next Send answers
    STATUS_NO_ACTOR.  Register an unknown actor: its earlier STATUS_NO_ACTOR was
    not cached, it answers OK.  ``rt`` hosts ids [0, 64); the records published
    here say 32, nothing, then 64 again."""
    from ptype_amd.mirror import ShardLease

    kv, service, node = rt._kv, rt.service, rt._node
    known = (lambda a: rt.table.lookup(actor_keys(torch.tensor([a])))[0].tolist() != [-1])
    rt.shard_lease.close()
    small = ShardLease(kv, service, node, 0, 1, 32)
    _until(lambda: (rt.sync(), known(3) and not known(40))[1], "the 32-actor record")
    b = MsgBatch(torch.tensor([3, 40, 3], dtype=torch.int32, device=dev), torch.tensor([6, 6, 6], device=dev),
                 torch.tensor([7, 7, 7], device=dev), None, METHOD_CALC_MULTIPLY)
    val, st = client.Send(b, cache=True)
    assert st.tolist() == [STATUS_OK, STATUS_NO_ACTOR, STATUS_OK] and val.tolist()[0] == 42
    n0 = rt.stats()["cache"]
    val, st = client.Send(b, cache=True)  # 3 from the cache, 40 asked again
    assert st.tolist() == [STATUS_OK, STATUS_NO_ACTOR, STATUS_OK]
    n = rt.stats()["cache"]
    assert (n["hits"] - n0["hits"], n["sent"] - n0["sent"], n["clears"] - n0["clears"]) == (2, 1, 0)
    small.close()
    _until(lambda: (rt.sync(), not known(3))[1], "the record's removal")
    val, st = client.Send(b, cache=True)
    assert st.tolist() == [STATUS_NO_ACTOR] * 3 and torch.equal(st, client.Send(b)[1])
    assert rt.stats()["cache"]["clears"] == n0["clears"] + 1
    full = ShardLease(kv, service, node, 0, 1, 64)
    _until(lambda: (rt.sync(), known(40))[1], "the 64-actor record")
    val, st = client.Send(b, cache=True)
    assert st.tolist() == [STATUS_OK] * 3 and val.tolist() == [42] * 3
    rt.shard_lease = full  # closed with the runtime


def test_stale_status_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, srv, c = join_world1(C, tmp_path, ports)
    try:
        client = c.NewClient("w1", C.ConnConfig())
        stale_status_scenario(c, c.runtime, client)
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_registry_change_counter_and_router_counter_cpu():
    from ptype_amd.parallel.replicas import ReplicaRouter

    rt = runtime()
    n0 = rt._registry_changes
    rt.host("other")
    assert rt._registry_changes == n0 + 1
    rt.restore_from({"state": rt.state.clone(), "table": torch.empty(0), "expiry": torch.empty(0)})
    assert rt._registry_changes == n0 + 2
    rt.place_local()
    b = multiply_batch(200, 20, 64)
    rt.send("calculator", b, cache=True)
    rt.send("calculator", b, cache=True)
    assert rt.stats()["cache"]["hits"] == 200 and rt.stats()["cache"]["clears"] == 0
    rt.host("third")  # may change which actors answer: the next cached Send starts cold
    rt.send("calculator", b, cache=True)
    assert rt.stats()["cache"]["hits"] == 200 and rt.stats()["cache"]["clears"] == 1
    rt.close()
    recs = [{"replica": True, "node": f"n{i}", "address": "127.0.0.1", "port": 7000 + i, "rank": i, "count": 8}
            for i in range(2)]
    r = ReplicaRouter("svc", 2, "10.0.0.1", 0, records=recs)
    assert r.changes == 1
    r.set_records(list(reversed(recs)))  # the same set
    assert r.changes == 1
    r.set_records(recs[:1])
    assert r.changes == 2
    # another router object with the same count of changes is another replica set: the cache starts cold,
    # and so it does when a Send without a router follows
    rt = runtime()
    one = recs[:1]
    r1, r2 = (ReplicaRouter("calculator", 1, "10.0.0.1", 0, records=one) for _ in range(2))
    assert r1.changes == r2.changes == 1
    b = MsgBatch(torch.arange(8, dtype=torch.int32), torch.arange(8, dtype=torch.int64), None, None, METHOD_ECHO)
    for router, hits, clears in ((r1, 0, 0), (r1, 8, 0), (r2, 8, 1), (r2, 16, 1), (None, 16, 2), (None, 24, 2)):
        val, st = rt.send("calculator", b, router=router, cache=True)
        assert val.tolist() == list(range(8)) and bool((st == STATUS_OK).all())
        n = rt.stats()["cache"]
        assert (n["hits"], n["clears"]) == (hits, clears), (router, n)
    assert rt._cache_seen[1] is None
    rt.close()


def test_cache_with_coalesce_cpu():
    M, keys = 5000, 300
    b = multiply_batch(M, keys, 64, seed=3)
    rt = runtime()
    plain = rt.send("calculator", b)
    sent = rt.exchange.counters.sent
    val, st = rt.send("calculator", b, coalesce=True, cache=True)
    assert torch.equal(val, plain[0]) and torch.equal(st, plain[1])
    assert rt.exchange.counters.sent - sent == keys  # the cache saw coalescing's leaders
    assert rt.stats()["cache"] == {"sends": 1, "messages": keys, "hits": 0, "sent": keys, "clears": 0,
                                   "entries": 1 << 20}
    val, st = rt.send("calculator", b, coalesce=True, cache=True)
    assert torch.equal(val, plain[0]) and torch.equal(st, plain[1])
    assert rt.exchange.counters.sent - sent == keys
    assert rt.stats()["cache"]["hits"] == keys and rt.stats()["coalesce"]["executed"] == 2 * keys
    rt.close()


def test_cache_with_retries_cpu():
    b, where = retry_mix()
    rt_plain, rt = runtime(), runtime()
    for send in range(2):
        want = rt_plain.send("calculator", b, retries=2)
        val, st = rt.send("calculator", b, retries=2, cache=True)
        assert torch.equal(val, want[0]) and torch.equal(st, want[1]) and torch.equal(rt.state, rt_plain.state), send
        if send == 0:
            assert int((st[where] == STATUS_FAILED).sum()) == 16 and rt.exchange.stats().retries == 2
    n = rt.stats()["cache"]  # the 64 RetryTest messages are sent both times, the Multiply ones once
    assert n["hits"] == b.M - 64 and n["sent"] == b.M + 64
    rt.close()
    rt_plain.close()


def test_cache_with_a_ledger_cpu():
    M, keys = 2000, 100
    b = multiply_batch(M, keys, 64, seed=2)
    rt_plain, rt = runtime(ledger=True), runtime(ledger=True)
    for send in range(2):
        rt_plain.send("calculator", b)
        val, st = rt.send("calculator", b, cache=True, coalesce=bool(send))
    want, r = rt_plain.stats()["ledger"], rt.stats()["ledger"]
    assert r == want and r["sends"] == 2 and r["messages"] == 2 * M
    assert r["calls"] == {"Calculator.Multiply": {"ok": 2 * M}} and r["audited"] == 2 * M and r["mismatch"] == 0
    assert rt.stats()["cache"]["hits"] == keys
    rt.send("calculator", b, cache=True, account=False)
    assert rt.stats()["ledger"] == r
    # the digest of one cached Send is the digest of its replies
    rt2 = runtime(ledger=True)
    rt2.send("calculator", b, cache=True, account=False)
    val, st = rt2.send("calculator", b, cache=True)
    r2 = rt2.stats()["ledger"]
    assert (r2["digest_sum"], r2["digest_xor"]) == L.digest(val, st) and r2["sends"] == 1
    for x in (rt, rt_plain, rt2):
        x.close()
    rt = runtime()
    with pytest.raises(ValueError, match="ledger"):
        rt.send("calculator", b, cache=True, account=True)
    rt.close()


def test_cached_send_is_refused_under_capture_cpu():
    rt = runtime()
    b = multiply_batch(100, 10, 64)
    rt.send("calculator", b)
    rt.exchange._capturing = True
    with pytest.raises(ValueError, match="captur"):
        rt.send("calculator", b, cache=True)
    with pytest.raises(ValueError, match="captur"):
        rt.send("calculator", b, cache=True, coalesce=True)
    rt.send("calculator", b)  # a plain Send is not
    assert rt.stats()["cache"]["sends"] == 0
    rt.exchange._capturing = False
    rt.close()


# ---------------------------------------------------------------- the public API and the config keys
def test_client_send_cache_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    M, keys = 3000, 200
    cfg, srv, c = join_world1(C, tmp_path, ports, form_group=True, grace_s=0.3)
    try:
        rt = c.runtime
        assert rt.cache is False and rt.cache_entries == 1 << 20
        b = multiply_batch(M, keys, rt.total_actors, seed=5)
        client = c.NewClient("w1", C.ConnConfig())
        plain = client.Send(b)
        assert rt._cache is None
        for send in range(2):
            val, st = client.Send(b, cache=True)
            assert torch.equal(val, plain[0]) and torch.equal(st, plain[1]) and torch.equal(val, b.a0 * b.a1)
        assert c.Stats()["runtime"]["cache"] == {"sends": 2, "messages": 2 * M, "hits": M, "sent": M, "clears": 0,
                                                 "entries": 1 << 20}
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_gpu_cache_config_default_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    M, keys = 1000, 50
    cfg, srv, c = join_world1(C, tmp_path, ports, cache=True, cache_entries=5000)
    try:
        assert c.runtime.cache is True
        b = multiply_batch(M, keys, c.runtime.total_actors, seed=6)
        client = c.NewClient("w1", C.ConnConfig())
        client.Send(b)  # no argument: gpu.cache
        val, st = client.Send(b)
        assert torch.equal(val, b.a0 * b.a1) and bool((st == STATUS_OK).all())
        n = c.Stats()["runtime"]["cache"]  # (50 keys in 8192 slots: the host reference says which collide)
        assert n == expected_counters([b, b], 5000) and n["entries"] == 8192 and n["hits"] > M // 2
        client.Send(b, cache=False)
        assert c.Stats()["runtime"]["cache"]["sends"] == 2
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_config_gpu_cache_keys(tmp_path):
    (tmp_path / "m.yml").write_text("name: x\n")
    p = tmp_path / "a.yml"
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu: {cache: true, cache_entries: 4096}\n")
    g = C.ConfigFromFile(str(p)).gpu
    assert g.cache is True and g.cache_entries == 4096
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu:\n  actors: 64\n")
    g = C.ConfigFromFile(str(p)).gpu
    assert g.cache is False and g.cache_entries == 1 << 20
    assert C.Config().gpu.cache is False and C.Config().gpu.cache_entries == 1 << 20
    for bad in ("cache: 3", "cache_entries: true", "cache_entries: 0", "cache_entries: -8", "cache_entries: many"):
        p.write_text(f"service_name: calc\netcd_config_file: m.yml\ngpu:\n  {bad}\n")
        with pytest.raises(C.ConfigError):
            C.ConfigFromFile(str(p))
