"""The reply cache on a real MI355X: the lookup, claim + write and clear kernels
(csrc/hip/reply_cache.hip) against the host reference (``ops.reply_cache.
ReplyCacheRef``), the whole table compared after every Send, and ``cache=True``
through world-1 runtimes, in-process multi-rank FakeComm exchanges and
``Client.Send``.  All comparisons are exact integer equality."""
import threading

import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import coalesce as CO
from ptype_amd.ops import hip
from ptype_amd.ops import ledger as L
from ptype_amd.ops import reply_cache as RC
from ptype_amd.ops import retry as RT
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_ECHO, METHOD_PRIME_CHECK,
                                   STATUS_FAILED, STATUS_OK)
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

from test_coalesce import multiply_batch, random_batch, retry_mix
from test_coalesce import runtime as cpu_runtime
from test_coalesce_gpu import _cuda
from test_coalesce_gpu import runtime as gpu_runtime
from test_reply_cache import U32, colliding_keys, expected_counters, fake_replies, stale_status_scenario

pytestmark = pytest.mark.gpu

T = 1024  # messages per block of the lookup kernel (checked below against the module)


def step(cache, ref, b, bg=None):
    """One cached Send on the ops level, on the GPU and on the host reference: the
    lookup's outputs, the compacted misses and, after the insert, the whole table.
    Returns (hits, K)."""
    bg = _cuda(b) if bg is None else bg
    val, st = cache.lookup(bg)
    rval, rst = ref.lookup(b)
    assert st.dtype == torch.int32 and val.dtype == torch.int64 and st.is_cuda
    assert torch.equal(st.cpu(), rst)
    hit = rst == STATUS_OK
    assert torch.equal(val.cpu()[hit], rval[hit])
    sub, idx, K = RT.select_mask(bg, st, 1 << RC.PENDING)
    rsub, ridx, rK = RT.select_mask(b, rst, 1 << RC.PENDING)
    assert K == rK == b.M - int(hit.sum()) and torch.equal(idx.cpu(), ridx)
    v2, s2 = fake_replies(rsub)
    cache.insert(sub, v2.cuda(), s2.cuda())
    ref.insert(rsub, v2, s2)
    assert (cache.epoch, cache.seq) == (ref.epoch, ref.seq)
    assert np.array_equal(cache.words(), ref.words())
    return int(hit.sum()), K


def pair(entries, **kw):
    return RC.ReplyCache("cuda", entries=entries, **kw), RC.ReplyCacheRef(entries=entries, **kw)


# ---------------------------------------------------------------- the kernels
@pytest.mark.parametrize("entries", [1 << 4, 1 << 8, 1 << 12])
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_three_sends_against_the_reference(M, entries):
    assert hip().reply_cache_tile() == T and hip().REPLY_CACHE_PENDING == RC.PENDING
    cache, ref = pair(entries)
    assert np.array_equal(cache.words(), ref.words())  # the clear kernel: zero, claim all ones
    hits = 0
    # a method column with pure and stateful methods and all three arguments; then a uniform pure method
    # without a2, and Prime.Check alone: ~300 pure keys, so a table of 16 evicts all the time and one of
    # 4096 answers most of a repeated batch
    for send, kw in enumerate(({}, {}, {"a2": False, "methods": METHOD_CALC_MULTIPLY},
                               {"a1": False, "a2": False, "methods": METHOD_PRIME_CHECK})):
        h, K = step(cache, ref, random_batch(M, 7 * M + send // 2, **kw))
        hits += h
    assert cache.seq == 4
    if M > 1000 and entries == 1 << 12:
        assert hits > M // 5  # (the inputs: Send 1 repeats Send 0, half of it pure, two thirds of that STATUS_OK)


def test_all_identical_and_all_distinct_batches():
    M = 3 * T + 17
    one = (lambda v, dt: torch.full((M,), v, dtype=dt))
    for entries in (1 << 4, 1 << 12):
        cache, ref = pair(entries)
        for method in (METHOD_PRIME_CHECK, one(METHOD_ECHO, torch.int16)):
            b = MsgBatch(one(7, torch.int32), one(-3, torch.int64), one(1 << 40, torch.int64), one(6, torch.int64),
                         method)  # (a0 % 5 != 0: fake_replies answers STATUS_OK)
            assert step(cache, ref, b) == (0, M)  # every row claims one slot: row 0 writes
            assert step(cache, ref, b) == (M, 0)
    g = torch.Generator().manual_seed(3)
    b = MsgBatch(torch.randint(0, 50, (M,), generator=g).to(torch.int32), torch.randperm(M, generator=g) * 5 - 999,
                 None, None, METHOD_CALC_MULTIPLY)
    cache, ref = pair(1 << 12)
    assert step(cache, ref, b) == (0, M)
    h, K = step(cache, ref, b)  # 3089 distinct keys into 4096 direct-mapped slots
    assert h + K == M and M // 3 < h < M
    # a uniform non-pure method: nothing is looked up and nothing stored
    add = MsgBatch(b.actor, b.a0, None, None, METHOD_COUNTER_ADD)
    before = cache.words().copy()
    assert step(cache, ref, add) == (0, M) and np.array_equal(cache.words(), before)


def test_colliding_keys_in_a_table_of_16():
    entries = 1 << 4
    (x, y, z), slot = colliding_keys(entries, 3)
    for a0 in (x, y, z):  # the numpy hash is the device's, bit for bit
        assert hip().coalesce_hash(9, METHOD_CALC_MULTIPLY, a0, 5, 0) & (entries - 1) == slot
    ok = (lambda n: torch.full((n,), STATUS_OK, dtype=torch.int32))
    mk = (lambda a0s: MsgBatch(torch.full((len(a0s),), 9, dtype=torch.int32), torch.tensor(a0s),
                               torch.full((len(a0s),), 5), None, METHOD_CALC_MULTIPLY))
    cache, ref = pair(entries)

    def insert(a0s, st):
        b = mk(a0s)
        cache.insert(_cuda(b), (b.a0 * 5).cuda(), st.cuda())
        ref.insert(b, b.a0 * 5, st)
        assert np.array_equal(cache.words(), ref.words())

    def lookup(a0s):
        val, st = cache.lookup(_cuda(mk(a0s)))
        return [v if s == STATUS_OK else None for v, s in zip(val.tolist(), st.tolist())]

    insert([x], ok(1))
    assert lookup([x, y]) == [5 * x, None]
    insert([y], ok(1))  # the newer Send evicts the older entry
    assert lookup([x, y]) == [None, 5 * y]
    insert([z, x, y], ok(3))  # the lowest row wins within one Send
    assert lookup([x, y, z]) == [None, None, 5 * z]
    insert([x, y], torch.tensor([STATUS_FAILED, STATUS_OK], dtype=torch.int32))  # a row that is not stored claims nothing
    assert lookup([x, y, z]) == [None, 5 * y, None]
    assert int(cache.words()[slot][RC.W_CLAIM]) == (U32 - 3) << 32 | 1


def test_unaligned_column_views():
    M = T + 9
    view = (lambda x: MsgBatch(x.actor[1:], x.a0[1:], x.a1[1:], x.a2[1:], x.method[1:]))  # odd element offsets
    cache, ref = pair(1 << 10)
    for seed in (35, 35, 36):
        b = random_batch(M + 1, seed)
        step(cache, ref, view(b), bg=view(_cuda(b)))
    # replies given as views at an odd offset
    b = random_batch(M, 37, methods=METHOD_ECHO)
    v2, s2 = fake_replies(b)
    pad = (lambda t: torch.cat([t[:1], t]).cuda()[1:])
    cache.insert(_cuda(b), pad(v2), pad(s2))
    ref.insert(b, v2, s2)
    assert np.array_equal(cache.words(), ref.words())


def test_clear_and_both_wraps():
    entries = 1 << 8
    b = random_batch(T + 65, 41, methods=METHOD_ECHO, span=30)
    cache, ref = pair(entries)
    step(cache, ref, b)
    h, _ = step(cache, ref, b)
    assert h > 0
    cache.clear()
    ref.clear()
    assert cache.epoch == 2 and np.array_equal(cache.words(), ref.words())  # O(1): the table is untouched
    assert step(cache, ref, b)[0] == 0
    assert step(cache, ref, b)[0] == h
    # the epoch wrap
    cache, ref = pair(entries, _start=(U32, 9))
    step(cache, ref, b)
    assert step(cache, ref, b)[0] == h
    cache.clear()
    ref.clear()
    assert (cache.epoch, cache.seq) == (1, 0) and np.array_equal(cache.words(), ref.words())
    assert np.array_equal(cache.words(), RC.ReplyCacheRef(entries=entries).words())
    assert step(cache, ref, b)[0] == 0
    # the sequence wrap: 0xFFFFFFFE and 0xFFFFFFFF are used, the next insert rewrites the table first
    cache, ref = pair(entries, _start=(5, U32 - 1))
    step(cache, ref, b)
    assert step(cache, ref, b)[0] == h and cache.seq == U32 + 1
    other = random_batch(T + 65, 42, methods=METHOD_ECHO, span=30)
    step(cache, ref, other)
    assert (cache.epoch, cache.seq) == (1, 1)
    assert step(cache, ref, b)[0] < h  # only what `other` left of b's keys


# ---------------------------------------------------------------- world 1 on the GPU
@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_runtime_send_cache_world1_gpu(delivery):
    M, keys = 5000, 300
    b = multiply_batch(M, keys, 64, seed=8)
    bg = _cuda(b)
    rt = gpu_runtime(delivery, cache_entries=1 << 14)
    try:
        plain = rt.send("calculator", bg)
        assert rt._cache is None  # a Send without the option creates nothing
        sent = rt.exchange.counters.sent
        val, st = rt.send("calculator", bg, cache=True)
        assert torch.equal(val, plain[0]) and torch.equal(st, plain[1])
        assert torch.equal(val.cpu(), b.a0 * b.a1) and bool((st == STATUS_OK).all())
        assert rt.exchange.counters.sent - sent == M  # cold: all misses
        val, st = rt.send("calculator", bg, cache=True)
        assert torch.equal(val, plain[0]) and torch.equal(st, plain[1])
        n = rt.stats()["cache"]
        assert n["sends"] == 2 and n["entries"] == 1 << 14 and n["hits"] + n["sent"] == 2 * M
        assert rt.exchange.counters.sent - sent == n["sent"]
        # a table every key has a slot of its own in: the second Send is all hits and sends nothing
        rt.close()
        rt = gpu_runtime(delivery)
        rt.send("calculator", bg, cache=True)
        sent = rt.exchange.counters.sent
        val, st = rt.send("calculator", bg, cache=True)
        n = rt.stats()["cache"]
        assert torch.equal(val, plain[0]) and torch.equal(st, plain[1]) and n["hits"] == M and n["sent"] == M
        assert rt.exchange.counters.sent == sent  # the inner Send was skipped
        # an unregistered actor: STATUS_NO_ACTOR is never stored, so it is asked every time
        actor = b.actor.clone()
        actor[::5] = 9999
        ug = MsgBatch(actor.cuda(), bg.a0, bg.a1, None, METHOD_CALC_MULTIPLY)
        want = rt.send("calculator", ug)
        for _ in range(2):
            val, st = rt.send("calculator", ug, cache=True)
            assert torch.equal(st, want[1]) and torch.equal(val, want[0])
        assert rt.stats()["cache"]["sent"] == M + 2 * (M // 5)
        rt.exchange._capturing = True  # as inside ActorExchange.capture
        try:
            with pytest.raises(ValueError, match="captur"):
                rt.send("calculator", bg, cache=True)
        finally:
            rt.exchange._capturing = False
    finally:
        rt.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_stateful_methods_run_every_time_gpu(delivery):
    M = 5000
    g = torch.Generator().manual_seed(12)
    col = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_COUNTER_ADD], dtype=torch.int16)[
        torch.randint(0, 3, (M,), generator=g)]
    actor = torch.randint(0, 70, (M,), generator=g).to(torch.int32)  # ids 64..69 are not registered
    b = MsgBatch(actor, torch.randint(0, 3, (M,), generator=g), torch.randint(0, 3, (M,), generator=g), None, col)
    bg = _cuda(b)
    rt, rt_plain, rt_cpu = gpu_runtime(delivery), gpu_runtime(delivery), cpu_runtime()
    try:
        for send in range(2):
            want = rt_plain.send("calculator", bg)
            val, st = rt.send("calculator", bg, cache=True)
            rt_cpu.send("calculator", b, cache=True)
            assert torch.equal(st, want[1]) and torch.equal(rt.state, rt_plain.state), send
            # (a Counter.Add reply is the running sum: it depends on the order within the batch, the state does not)
            pure = (col != METHOD_COUNTER_ADD).cuda()
            assert torch.equal(val[pure], want[0][pure])
        ok_pure = int(((st.cpu() == STATUS_OK) & (col != METHOD_COUNTER_ADD)).sum())
        n = rt.stats()["cache"]  # (two of the ~1100 keys may share one of the 1 Mi slots: the host reference says)
        assert n == rt_cpu.stats()["cache"] and n["hits"] + n["sent"] == 2 * M and ok_pure - 20 < n["hits"] <= ok_pure
        add = MsgBatch(torch.full((M,), 11, dtype=torch.int32, device="cuda"),
                       torch.ones(M, dtype=torch.int64, device="cuda"), None, None, METHOD_COUNTER_ADD)
        s0 = int(rt.state[11])
        rt.send("calculator", add, cache=True)
        rt.send("calculator", add, cache=True)
        assert int(rt.state[11]) == s0 + 2 * M
    finally:
        rt.close()
        rt_plain.close()
        rt_cpu.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_cache_with_coalesce_retries_and_a_ledger_gpu(delivery):
    M, keys = 5000, 300
    b = multiply_batch(M, keys, 64, seed=8)
    bg = _cuda(b)
    rt, rt_plain = gpu_runtime(delivery, ledger=True), gpu_runtime(delivery, ledger=True)
    try:
        sent = rt.exchange.counters.sent
        for send in range(2):
            want = rt_plain.send("calculator", bg)
            val, st = rt.send("calculator", bg, coalesce=True, cache=True)
            assert torch.equal(val, want[0]) and torch.equal(st, want[1])
        assert rt.exchange.counters.sent - sent == keys  # the leaders, once
        n = rt.stats()["cache"]
        assert (n["messages"], n["hits"], n["sent"]) == (2 * keys, keys, keys)
        r, want = rt.stats()["ledger"], rt_plain.stats()["ledger"]
        assert r == want and r["messages"] == 2 * M and r["mismatch"] == 0
        assert (r["digest_sum"], r["digest_xor"]) != L.digest(val, st)  # (two Sends folded)
        rt.send("calculator", bg, cache=True, account=False)
        assert rt.stats()["ledger"] == r
    finally:
        rt.close()
        rt_plain.close()
    rb, where = retry_mix(5000)
    rg = _cuda(rb)
    rt, rt_plain, rt_cpu = gpu_runtime(delivery), gpu_runtime(delivery), cpu_runtime()
    try:
        for send in range(2):
            want = rt_plain.send("calculator", rg, retries=2)
            val, st = rt.send("calculator", rg, retries=2, cache=True)
            rt_cpu.send("calculator", rb, retries=2, cache=True)
            assert torch.equal(val, want[0]) and torch.equal(st, want[1]) and torch.equal(rt.state, rt_plain.state)
            if send == 0:
                assert int((st.cpu()[where] == STATUS_FAILED).sum()) == 16 and rt.exchange.stats().retries == 2
        n = rt.stats()["cache"]  # the 64 RetryTest messages are sent both times, the Multiply ones once
        assert n == rt_cpu.stats()["cache"] and n["hits"] + n["sent"] == 2 * rb.M and n["hits"] > rb.M - 64 - 20
    finally:
        rt.close()
        rt_plain.close()
        rt_cpu.close()


# ---------------------------------------------------------------- R in-process ranks (FakeComm)
@pytest.mark.parametrize("through_runtime", [False, True])
@pytest.mark.parametrize("R_", [2, 4])
def test_cached_sends_multirank_fakecomm(R_, through_runtime):
    """Every rank caches batches of its own over three Sends, drawn from keys that
    all have a slot of their own.  Send 1 repeats half of Send 0; in Send 2 rank 0
    repeats Send 0 (all hits: it joins with an empty batch) while every other rank
    sends new keys (all misses).  Every rank issues exactly one inner Send per
    cached Send, so the ranks stay in step.  ``through_runtime``: the cached Sends
    go through ``DeviceRuntime.send(cache=True)`` of a runtime that is given the
    rank's FakeComm exchange (its own wiring at world > 1: the sync and clear
    prelude, ``collective``, the final inner ``_send``), not ``ReplyCache.send``."""
    from ptype_amd.runtime import DeviceRuntime

    M, n, sends, entries = 3000, 6000, 3, 1 << 16
    fc = hip().FakeComm(R_)

    def keys(r, a):
        a = torch.as_tensor(a, dtype=torch.int64)
        return MsgBatch(((a + r) % n).to(torch.int32), a - 7, torch.full_like(a, r + 2), None, METHOD_CALC_MULTIPLY)

    pools = []
    for r in range(R_):  # 3 M values of a whose keys fall into pairwise different slots
        cand = keys(r, torch.arange(40_000))
        slot = CO.key_hash(cand.actor.numpy(), METHOD_CALC_MULTIPLY, cand.a0.numpy(), cand.a1.numpy(), 0) \
            & np.uint64(entries - 1)
        first = np.sort(np.unique(slot, return_index=True)[1])
        assert first.size >= 3 * M
        pools.append(torch.from_numpy(first[:3 * M]))

    def batch(r, send):
        p = pools[r]
        if send == 0 or (send == 2 and r == 0):
            return keys(r, p[:M])
        if send == 1:
            return keys(r, torch.cat([p[:M // 2], p[M:M + M // 2]]))
        return keys(r, p[2 * M:])

    results, counters, inner, errors = [None] * R_, [None] * R_, [None] * R_, []
    start = threading.Barrier(R_)

    def run(r):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                tab = RegistryTable(2 * n, device="cuda")
                ids = torch.arange(n)
                tab.upsert(actor_keys(ids), (ids % R_).to(torch.int32), (ids // R_).to(torch.int32))
                tab.enable_directory(n, affine_world=R_)
                st = torch.zeros(n // R_, dtype=torch.int64, device="cuda")
                ex = ActorExchange(tab, M, chunks=1, state=st, fake=(fc, r), delivery="direct")
                calls = []
                rt = None
                if through_runtime:
                    rt = DeviceRuntime(torch.device("cuda", 0), actors=n // R_, service="calculator", shm=False,
                                       max_batch=M, cache_entries=entries)
                    rt.rank, rt.world, rt.world0, rt.table, rt._exchange = r, R_, R_, tab, ex
                    inner_send = rt._send

                    def counted(service, sub, *a, **kw):
                        calls.append(sub.M)
                        return inner_send(service, sub, *a, **kw)

                    rt._send = counted
                    send = (lambda b: rt.send("calculator", b, cache=True))
                else:
                    cache = RC.ReplyCache("cuda", entries=entries)

                    def send_all(sub):
                        calls.append(sub.M)
                        return ex.send_all(sub)

                    send = (lambda b: cache.send(b, send_all, collective=True))
                try:
                    start.wait(timeout=60)
                    out = []
                    for k in range(sends):
                        val, sts = send(_cuda(batch(r, k)))[:2]
                        out.append((val.cpu(), sts.cpu()))
                    s.synchronize()
                    results[r], inner[r] = out, calls
                    counters[r] = dict((rt._cache if through_runtime else cache).counters)
                finally:
                    if rt is not None:
                        rt.close()
        except BaseException as e:  # noqa: BLE001 - surfaced below
            errors.append((r, repr(e)))
            start.abort()

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(R_)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank hung"
    assert not errors, errors
    for r in range(R_):
        for k, (val, sts) in enumerate(results[r]):
            b = batch(r, k)
            assert bool((sts == STATUS_OK).all()) and torch.equal(val, b.a0 * b.a1), (r, k)
        # exactly one inner Send per cached Send; rank 0's third one carried nothing
        assert inner[r] == [M, M // 2, 0 if r == 0 else M], r
        assert counters[r] == {"sends": sends, "messages": sends * M, "hits": sends * M - sum(inner[r]),
                               "sent": sum(inner[r]), "clears": 0}, r


# ---------------------------------------------------------------- Client.Send through Join
@pytest.mark.parametrize("default", [False, True])
def test_client_send_cache_through_join_gpu(tmp_path, ports, monkeypatch, default):
    """``Client.Send(batch, cache=True)`` with ``gpu.cache`` unset (direct delivery),
    and ``gpu.cache: true`` with no argument (mailbox delivery); then the stale-status
    scenario on this runtime, under either delivery."""
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    from ptype_amd.models import calculator

    pp, pc = ports(), ports()
    cfg = C.Config()
    cfg.service_name, cfg.node_name, cfg.port = "calculator", "gpu0", ports()
    cfg.member = C.member_config(name="m0", dir=str(tmp_path / "m0"), lpurls=[f"http://127.0.0.1:{pp}"],
                                 apurls=[f"http://127.0.0.1:{pp}"], lcurls=[f"http://127.0.0.1:{pc}"],
                                 acurls=[f"http://127.0.0.1:{pc}"], initial_cluster=f"m0=http://127.0.0.1:{pp}",
                                 heartbeat_ms=50, election_ms=500, unsafe_no_fsync=True)
    cfg.has_gpu = True
    cfg.gpu.device, cfg.gpu.actors, cfg.gpu.max_batch = 0, 64, 1 << 13
    cfg.gpu.delivery = "mailbox" if default else "direct"
    cfg.gpu.cache_entries = 1 << 16
    if default:
        cfg.gpu.cache = True
    c = C.Join(C.background(), cfg)
    server = C.Server()  # NewClient dials the registered node, as the reference does
    try:
        calculator.serve_device(c.runtime, server)
        server.Listen(cfg.port, "127.0.0.1")
        assert c.runtime.cache is default
        M, keys = 5000, 300
        b = multiply_batch(M, keys, c.runtime.total_actors, seed=9)
        bg = _cuda(b)
        client = c.NewClient("calculator", C.ConnConfig())
        for send in range(2):
            val, st = client.Send(bg) if default else client.Send(bg, cache=True)
            assert torch.equal(val.cpu(), b.a0 * b.a1) and bool((st == STATUS_OK).all())
        n = c.Stats()["runtime"]["cache"]  # (300 keys in 64 Ki slots: the host reference says which collide)
        assert n == expected_counters([b, b], 1 << 16) and n["entries"] == 1 << 16 and n["hits"] > M // 2
        plain = client.Send(bg, cache=False)
        assert torch.equal(val, plain[0]) and torch.equal(st, plain[1])
        assert c.Stats()["runtime"]["cache"]["sends"] == 2
        c.runtime.cache_clear()
        client.Send(bg, cache=True)
        assert c.Stats()["runtime"]["cache"] == expected_counters([b, b, "clear", b], 1 << 16)
        stale_status_scenario(c, c.runtime, client, dev="cuda")
        client.Close()
    finally:
        server.Close()
        c.Close()
