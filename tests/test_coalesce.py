"""Send coalescing on CPU tensors (``ops/coalesce.py``): the host references
against an independent ``numpy.unique``, the runtime's ``coalesce=`` switch with
retries, a ledger and the public API, the ``gpu.coalesce`` config key and the
capture refusal.  All comparisons are exact integer equality."""
import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import coalesce as CO
from ptype_amd.ops import hip
from ptype_amd.ops import ledger as L
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_ECHO, METHOD_FORWARD,
                                   METHOD_PRIME_CHECK, METHOD_RELAY, METHOD_RETRY_TEST, METHOD_SEQ_FOLD, PURE_METHODS,
                                   STATUS_FAILED, STATUS_NO_ACTOR, STATUS_OK)

from test_send_retries import join_world1

U64 = (1 << 64) - 1


def mix64(x):  # splitmix64 finalizer on Python ints (csrc/hip/common.hpp)
    x &= U64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & U64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & U64
    return x ^ (x >> 31)


def unique_leaders(batch):
    """lead[M] by ``numpy.unique`` over the rows of the pure messages (first
    occurrence), every other message its own leader."""
    M = batch.M
    actor = batch.actor.numpy().view(np.uint32).astype(np.int64)
    method = (np.full(M, batch.method, dtype=np.int64) if isinstance(batch.method, int)
              else batch.method.numpy().view(np.uint16).astype(np.int64))
    z = np.zeros(M, dtype=np.int64)
    arg = (lambda t: z if t is None else t.numpy())
    rows = np.stack([actor, method, arg(batch.a0), arg(batch.a1), arg(batch.a2)], axis=1)
    lead = np.arange(M)
    pure = np.flatnonzero(np.isin(method, sorted(PURE_METHODS)))
    if pure.size:
        _, first, inv = np.unique(rows[pure], axis=0, return_index=True, return_inverse=True)
        lead[pure] = pure[first[inv.reshape(-1)]]
    return torch.from_numpy(lead.astype(np.int32))


def random_batch(M, seed, span=3, a1=True, a2=True, methods=(1, 2, 3, 4, 5, 7), actors=4):
    g = torch.Generator().manual_seed(seed)
    col = (lambda: torch.randint(-1, span - 1, (M,), generator=g))
    method = methods if isinstance(methods, int) else torch.tensor(methods, dtype=torch.int16)[
        torch.randint(0, len(methods), (M,), generator=g)]
    return MsgBatch(torch.randint(0, actors, (M,), generator=g).to(torch.int32), col(), col() if a1 else None,
                    col() if a2 else None, method)


# ---------------------------------------------------------------- the references
@pytest.mark.parametrize("M", [0, 1, 2, 65, 1000, 5000])
def test_group_ref_against_numpy_unique(M):
    for seed, kw in enumerate(({}, {"a1": False}, {"a2": False, "a1": False}, {"methods": METHOD_CALC_MULTIPLY},
                               {"methods": METHOD_PRIME_CHECK, "span": 2, "actors": 2}, {"span": 40, "actors": 50})):
        b = random_batch(M, 100 * M + seed, **kw)
        lead = CO.group_ref(b)
        assert lead.dtype == torch.int32 and torch.equal(lead, unique_leaders(b)), (M, kw)
        assert torch.equal(CO.group(b), lead)  # CPU tensors run the reference
        if M >= 1000 and "span" not in kw:
            assert int((lead != torch.arange(M)).sum()) > M // 8  # (the inputs: the small range gives duplicates)


def test_non_pure_methods_are_their_own_leader():
    M = 600
    ids = torch.zeros(M, dtype=torch.int32)
    a = torch.ones(M, dtype=torch.int64)
    own = torch.arange(M, dtype=torch.int32)
    for m in (0, METHOD_RETRY_TEST, METHOD_COUNTER_ADD, METHOD_FORWARD, METHOD_SEQ_FOLD, METHOD_RELAY, 0x7D, 9, 0x7FFF):
        assert m not in PURE_METHODS
        assert torch.equal(CO.group_ref(MsgBatch(ids, a, a, a, m)), own), m
        assert torch.equal(CO.group_ref(MsgBatch(ids, a, a, a, torch.full((M,), m, dtype=torch.int16))), own), m
    assert PURE_METHODS == {METHOD_CALC_MULTIPLY, METHOD_PRIME_CHECK, METHOD_ECHO}
    for m in PURE_METHODS:
        assert bool((CO.group_ref(MsgBatch(ids, a, a, a, m)) == 0).all()), m
    # a method column: only the Multiply rows of the same (actor, args) group
    col = torch.tensor([METHOD_COUNTER_ADD, METHOD_CALC_MULTIPLY] * (M // 2), dtype=torch.int16)
    lead = CO.group_ref(MsgBatch(ids, a, a, None, col))
    assert torch.equal(lead[0::2], own[0::2]) and bool((lead[1::2] == 1).all())
    # -1 as a method column entry is 0xffff: not pure, and no match for a uniform 0xffff either way
    assert torch.equal(CO.group_ref(MsgBatch(ids, a, None, None, torch.full((M,), -1, dtype=torch.int16))), own)


def test_key_fields_and_missing_columns():
    i64 = torch.iinfo(torch.int64)
    # pairs that differ in exactly one field (index 2k, 2k + 1): never one group
    actor = torch.tensor([5, 5 - 2**31, 7, 7, 7, 7, 7, 7, 7, 7], dtype=torch.int32)  # bit 31 only
    a0 = torch.tensor([1, 1, 1, 1 + (1 << 32), i64.min, i64.max, 3, 3, 3, 3])       # above bit 31; min / max
    a1 = torch.tensor([2, 2, 2, 2, 2, 2, -1, 0, 4, 4])
    a2 = torch.tensor([0, 0, 0, 0, 0, 0, 0, 0, i64.min, -1])
    lead = CO.group_ref(MsgBatch(actor, a0, a1, a2, METHOD_ECHO))
    assert torch.equal(lead, torch.arange(10, dtype=torch.int32))
    col = torch.tensor([METHOD_ECHO, METHOD_CALC_MULTIPLY] * 5, dtype=torch.int16)
    same = MsgBatch(torch.zeros(10, dtype=torch.int32), torch.ones(10, dtype=torch.int64), None, None, col)
    assert CO.group_ref(same).tolist() == [0, 1] * 5  # the method is part of the key
    # a missing a1 / a2 column counts as 0
    z = torch.zeros(10, dtype=torch.int64)
    for b in (MsgBatch(same.actor, same.a0, z, None, col), MsgBatch(same.actor, same.a0, None, z, col),
              MsgBatch(same.actor, same.a0, z, z, col)):
        assert CO.group_ref(b).tolist() == [0, 1] * 5
    assert CO.key_hash(3, 1, 9).tolist() == CO.key_hash(3, 1, 9, 0, 0).tolist()


def test_key_hash_by_hand():
    for actor, method, a0, a1, a2 in ((0, 0, 0, 0, 0), (7, 1, 3, 4, 0), (0xFFFFFFFF, 3, -1, -2**63, 2**63 - 1),
                                      (1 << 31, 2, 1 << 32, 5, -7)):
        h = mix64(actor | method << 32)
        for x in (a0, a1, a2):
            h = mix64(h ^ (x & U64))
        got = CO.key_hash(np.array([actor], dtype=np.uint32), method, a0, a1, a2)
        assert got.dtype == np.uint64 and int(got[0]) == h
        assert hip().coalesce_hash(actor, method, a0, a1, a2) == h  # coalesce.hpp, compiled for the host
    assert [bool(hip().coalesce_pure(m)) for m in range(10)] == [m in PURE_METHODS for m in range(10)]
    # swapped arguments hash differently (the chain is not symmetric)
    assert int(CO.key_hash(0, 1, 3, 4)) != int(CO.key_hash(0, 1, 4, 3))
    assert CO.table_log2_for(0) == 4 and CO.table_log2_for(8) == 4 and CO.table_log2_for(9) == 5
    assert CO.table_log2_for(2048) == 12 and CO.table_log2_for(2049) == 13


def test_select_and_fanout_references():
    M = 3000
    b = random_batch(M, 7)
    lead = CO.group_ref(b)
    sub, idx, pos, K = CO.select(b, lead)
    want = torch.nonzero(lead == torch.arange(M)).flatten()
    assert K == want.numel() and idx.dtype == torch.int32 and torch.equal(idx.to(torch.int64), want)
    assert pos.dtype == torch.int32 and torch.equal(pos[want], torch.arange(K, dtype=torch.int32))
    assert bool((pos[lead != torch.arange(M)] == -1).all())
    assert torch.equal(sub.actor, b.actor[want]) and torch.equal(sub.a0, b.a0[want])
    assert torch.equal(sub.a1, b.a1[want]) and torch.equal(sub.a2, b.a2[want])
    assert torch.equal(sub.method, b.method[want])
    v2, s2 = torch.arange(K, dtype=torch.int64) * 3 - 5, (torch.arange(K) % 7).to(torch.int32)
    val, st = CO.fanout(lead, pos, v2, s2)
    j = pos.to(torch.int64)[lead.to(torch.int64)]
    assert torch.equal(val, v2[j]) and torch.equal(st, s2[j]) and st.dtype == torch.int32
    with pytest.raises(TypeError):
        CO.select(b, lead.to(torch.int64))
    with pytest.raises(ValueError):
        CO.fanout(lead, pos[:5], v2, s2)


# ---------------------------------------------------------------- a CPU runtime
def runtime(actors=64, **kw):
    from ptype_amd.runtime import DeviceRuntime

    rt = DeviceRuntime(torch.device("cpu"), actors=actors, service="calculator", **kw)
    rt.place_local()
    return rt


def multiply_batch(M, keys, actors, seed=0):
    """M Multiply messages drawn from ``keys`` distinct (actor, a0, a1)."""
    g = torch.Generator().manual_seed(seed)
    ka = torch.randperm(actors * 100, generator=g)[:keys]  # distinct (actor, a0) pairs
    k1 = torch.randint(-2**40, 2**40, (keys,), generator=g)
    pick = torch.cat([torch.arange(keys), torch.randint(0, keys, (M - keys,), generator=g)])[
        torch.randperm(M, generator=g)]
    return MsgBatch((ka % actors).to(torch.int32)[pick], (ka // actors - 50)[pick], k1[pick], None,
                    METHOD_CALC_MULTIPLY)


def test_runtime_send_coalesce_equals_plain_and_counts_cpu():
    M, keys = 5000, 300
    b = multiply_batch(M, keys, 64)
    rt = runtime()
    plain = rt.send("calculator", b)
    sent = rt.exchange.counters.sent
    assert rt.stats()["coalesce"] == {"sends": 0, "messages": 0, "executed": 0}
    val, st = rt.send("calculator", b, coalesce=True)
    assert torch.equal(val, plain[0]) and torch.equal(st, plain[1]) and bool((st == STATUS_OK).all())
    assert torch.equal(val, b.a0 * b.a1)
    assert rt.exchange.counters.sent - sent == keys  # the leaders only
    assert rt.stats()["coalesce"] == {"sends": 1, "messages": M, "executed": keys}
    rt.send("calculator", b, coalesce=False)
    rt.send("calculator", b)  # None: the runtime's default, off
    assert rt.stats()["coalesce"]["sends"] == 1
    # no duplicates: the batch as it is (K == M)
    u = MsgBatch(torch.arange(64, dtype=torch.int32), torch.arange(64, dtype=torch.int64), None, None, METHOD_ECHO)
    val, st = rt.send("calculator", u, coalesce=True)
    assert torch.equal(val, u.a0) and rt.stats()["coalesce"] == {"sends": 2, "messages": M + 64, "executed": keys + 64}
    val, st = rt.send("calculator", u.slice(0, 0), coalesce=True)  # an empty Send
    assert val.numel() == 0 and st.numel() == 0 and rt.stats()["coalesce"]["sends"] == 3
    rt.close()
    # the runtime default
    rt = runtime(coalesce=True)
    val, st = rt.send("calculator", b)
    assert torch.equal(val, plain[0]) and rt.stats()["coalesce"]["executed"] == keys
    rt.send("calculator", b, coalesce=False)
    assert rt.stats()["coalesce"]["sends"] == 1
    rt.close()


def test_stateful_methods_run_as_often_as_they_appear_cpu():
    M = 777
    rt = runtime()
    b = MsgBatch(torch.full((M,), 5, dtype=torch.int32), torch.ones(M, dtype=torch.int64), None, None,
                 METHOD_COUNTER_ADD)
    val, st = rt.send("calculator", b, coalesce=True)
    assert int(rt.state[5]) == M and sorted(val.tolist()) == list(range(1, M + 1))
    assert rt.stats()["coalesce"] == {"sends": 1, "messages": M, "executed": M}
    rt.close()


def test_followers_inherit_the_leaders_status_cpu():
    rt = runtime(actors=8)
    actor = torch.tensor([3, 99, 3, 99, 99, 2], dtype=torch.int32)  # 99 is not registered
    b = MsgBatch(actor, torch.full((6,), 4, dtype=torch.int64), None, None, METHOD_ECHO)
    val, st = rt.send("calculator", b, coalesce=True)
    assert st.tolist() == [STATUS_OK, STATUS_NO_ACTOR, STATUS_OK, STATUS_NO_ACTOR, STATUS_NO_ACTOR, STATUS_OK]
    plain = rt.send("calculator", b)
    assert torch.equal(st, plain[1]) and torch.equal(val, plain[0])
    assert rt.stats()["coalesce"]["executed"] == 3
    rt.close()


def retry_mix(M=600, actors=64):
    """RetryTest messages (one per actor, callsBeforePass 1..4) between duplicated
    Multiply messages, as a method column."""
    g = torch.Generator().manual_seed(4)
    method = torch.full((M,), METHOD_CALC_MULTIPLY, dtype=torch.int16)
    actor = torch.randint(0, actors, (M,), generator=g).to(torch.int32)
    a0 = torch.randint(0, 3, (M,), generator=g)
    a1 = torch.randint(0, 3, (M,), generator=g)
    where = torch.randperm(M, generator=g)[:actors]
    method[where] = METHOD_RETRY_TEST
    actor[where] = torch.arange(actors, dtype=torch.int32)
    a0[where] = 1 + torch.arange(actors) % 4
    a1[where] = 0
    return MsgBatch(actor, a0, a1, None, method), where


def test_coalesce_with_retries_cpu():
    b, where = retry_mix()
    rt_plain, rt = runtime(), runtime()
    want = rt_plain.send("calculator", b, retries=2)
    val, st = rt.send("calculator", b, retries=2, coalesce=True)
    assert torch.equal(val, want[0]) and torch.equal(st, want[1]) and torch.equal(rt.state, rt_plain.state)
    assert int((st[where] == STATUS_FAILED).sum()) == 16 and rt.exchange.stats().retries == 2  # callsBeforePass 4
    K = rt.stats()["coalesce"]["executed"]
    assert 64 < K < 64 + 64 * 9 + 1 and K < b.M
    rt.close()
    rt_plain.close()


def test_coalesce_with_a_ledger_cpu():
    M, keys = 2000, 100
    b = multiply_batch(M, keys, 64, seed=2)
    rt = runtime(ledger=True)
    val, st = rt.send("calculator", b, coalesce=True)
    r = rt.stats()["ledger"]
    assert r["sends"] == 1 and r["messages"] == M and r["calls"] == {"Calculator.Multiply": {"ok": M}}
    assert r["audited"] == M and r["mismatch"] == 0
    assert (r["digest_sum"], r["digest_xor"]) == L.digest(val, st)
    rt.send("calculator", b, coalesce=True, account=False)
    assert rt.stats()["ledger"] == r
    rt.close()
    rt = runtime()
    with pytest.raises(ValueError, match="ledger"):
        rt.send("calculator", b, coalesce=True, account=True)
    rt.close()


def test_coalesced_send_is_refused_under_capture_cpu():
    rt = runtime()
    b = multiply_batch(100, 10, 64)
    rt.send("calculator", b)
    rt.exchange._capturing = True
    with pytest.raises(ValueError, match="captur"):
        rt.send("calculator", b, coalesce=True)
    rt.send("calculator", b)  # a plain Send is not
    assert rt.stats()["coalesce"]["sends"] == 0
    rt.exchange._capturing = False
    rt.close()


# ---------------------------------------------------------------- the public API and the config key
def test_client_send_coalesce_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    M, keys = 3000, 200
    cfg, srv, c = join_world1(C, tmp_path, ports, form_group=True, grace_s=0.3)
    try:
        rt = c.runtime
        assert rt.coalesce is False
        b = multiply_batch(M, keys, rt.total_actors, seed=5)
        client = c.NewClient("w1", C.ConnConfig())
        plain = client.Send(b)
        val, st = client.Send(b, coalesce=True)
        assert torch.equal(val, plain[0]) and torch.equal(st, plain[1]) and torch.equal(val, b.a0 * b.a1)
        assert c.Stats()["runtime"]["coalesce"] == {"sends": 1, "messages": M, "executed": keys}
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_gpu_coalesce_config_default_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    M, keys = 1000, 50
    cfg, srv, c = join_world1(C, tmp_path, ports, coalesce=True)
    try:
        assert c.runtime.coalesce is True
        b = multiply_batch(M, keys, c.runtime.total_actors, seed=6)
        client = c.NewClient("w1", C.ConnConfig())
        val, st = client.Send(b)  # no argument: gpu.coalesce
        assert torch.equal(val, b.a0 * b.a1) and bool((st == STATUS_OK).all())
        assert c.Stats()["runtime"]["coalesce"] == {"sends": 1, "messages": M, "executed": keys}
        client.Send(b, coalesce=False)
        assert c.Stats()["runtime"]["coalesce"]["sends"] == 1
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_config_gpu_coalesce_key(tmp_path):
    (tmp_path / "m.yml").write_text("name: x\n")
    p = tmp_path / "a.yml"
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu: {coalesce: true}\n")
    assert C.ConfigFromFile(str(p)).gpu.coalesce is True
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu:\n  actors: 64\n")
    assert C.ConfigFromFile(str(p)).gpu.coalesce is False
    assert C.Config().gpu.coalesce is False
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu:\n  coalesce: 3\n")
    with pytest.raises(C.ConfigError):
        C.ConfigFromFile(str(p))
