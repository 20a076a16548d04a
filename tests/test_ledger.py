"""The Send ledger on CPU tensors (``ops/ledger.py``): the numpy reference against
values written out by hand, the digest's properties, a world-1 exchange with
retries, the runtime's ``account=`` switch and the ``gpu.ledger`` config key.
All comparisons are exact integer equality."""
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import ledger as L
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_ECHO, METHOD_RELAY,
                                   METHOD_RETRY_TEST, STATUS_FAILED)

from test_send_retries import join_world1, retry_scenario, world1

U64 = (1 << 64) - 1


def mix64(x):  # splitmix64 finalizer on Python ints (csrc/hip/common.hpp)
    x &= U64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & U64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & U64
    return x ^ (x >> 31)


def digest_by_hand(value, status):
    """(sum, xor) of h(i, v, s) = mix64(mix64(i + 1) ^ u64(v') ^ (u64(u32(s)) * GOLD))."""
    dsum = dxor = 0
    for i, (v, s) in enumerate(zip(value, status)):
        h = mix64(mix64(i + 1) ^ ((v & U64) if s == 0 else 0) ^ ((s & 0xFFFFFFFF) * 0x9E3779B97F4A7C15 & U64))
        dsum, dxor = (dsum + h) & U64, dxor ^ h
    return dsum, dxor


# twelve messages: every method class and every status class at least once
METHODS = [1, 3, 5, 0, 0x7E, 0x7FFF, -1, 1, 3, 1, 1, 5]
STATUS = [0, 0, 0, 1, 2, 3, 4, 5, 6, -1, 7, 40]
A0 = [3, 9, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
A1 = [4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
VALUE = [12, 8, 77, 5, 5, 5, 5, 5, 5, 5, 5, 5]  # Multiply 3 * 4 right, Echo 9 answered 8, CounterAdd not audited
ACTOR = [0, 1, 1, 5, 7, 8, -1, 3, 3, 3, 100, 2]


def hand_batch(method=None, a1=True):
    return MsgBatch(torch.tensor(ACTOR, dtype=torch.int32), torch.tensor(A0), torch.tensor(A1) if a1 else None, None,
                    torch.tensor(METHODS, dtype=torch.int16) if method is None else method)


def calls_of(words):
    c = words[L.W_CALLS:L.W_CALLS + 128].view(16, 8)
    return {(m, s): int(c[m, s]) for m in range(16) for s in range(8) if c[m, s]}


def test_account_ref_hand_built_method_column():
    value, status = torch.tensor(VALUE), torch.tensor(STATUS, dtype=torch.int32)
    words, load = L.account_ref(hand_batch(), value, status, n_load=8)
    assert words.dtype == torch.int64 and words.numel() == L.LEDGER_WORDS == 136
    # 0x7e, 0x7fff and -1 (0xffff as u16) are "other" (slot 15); statuses -1, 7 and 40 are slot 7
    assert calls_of(words) == {(1, 0): 1, (3, 0): 1, (5, 0): 1, (0, 1): 1, (15, 2): 1, (15, 3): 1, (15, 4): 1,
                               (1, 5): 1, (3, 6): 1, (1, 7): 2, (5, 7): 1}
    assert int(words[L.W_MESSAGES]) == 12 and int(words[L.W_SENDS]) == 1
    assert int(words[L.W_AUDITED]) == 2 and int(words[L.W_MISMATCH]) == 1  # the Multiply and the Echo row; Echo differs
    assert load.tolist() == [1, 2, 1, 3, 0, 1, 0, 1] and int(words[L.W_LOAD_OOB]) == 3  # ids 8, 100 and -1 (as u32)
    dsum, dxor = digest_by_hand(VALUE, STATUS)
    assert int(words[L.W_DIGEST_SUM]) & U64 == dsum and int(words[L.W_DIGEST_XOR]) & U64 == dxor
    assert L.digest(value, status) == (dsum, dxor)
    # without a load table nothing about actors is counted
    words, load = L.account_ref(hand_batch(), value, status)
    assert load is None and int(words[L.W_LOAD_OOB]) == 0


def test_account_ref_uniform_methods_and_null_a1():
    status = torch.tensor(STATUS, dtype=torch.int32)
    # uniform Multiply with a null a1 (reads as 0): the three OK rows expect 0; value 0 only in row 1
    value = torch.tensor([12, 0, 77] + [5] * 9)
    words, _ = L.account_ref(hand_batch(METHOD_CALC_MULTIPLY, a1=False), value, status)
    assert calls_of(words) == {(1, 0): 3, (1, 1): 1, (1, 2): 1, (1, 3): 1, (1, 4): 1, (1, 5): 1, (1, 6): 1, (1, 7): 3}
    assert int(words[L.W_AUDITED]) == 3 and int(words[L.W_MISMATCH]) == 2
    # uniform Multiply with a1: row 0 is 3 * 4 = 12, rows 1 and 2 expect 0
    words, _ = L.account_ref(hand_batch(METHOD_CALC_MULTIPLY), value, status)
    assert int(words[L.W_AUDITED]) == 3 and int(words[L.W_MISMATCH]) == 1
    # wrapping product: 2**62 * 4 == 0 (mod 2**64)
    b = MsgBatch(torch.zeros(2, dtype=torch.int32), torch.tensor([1 << 62, 3]), torch.tensor([4, -5]), None,
                 METHOD_CALC_MULTIPLY)
    words, _ = L.account_ref(b, torch.tensor([0, -15]), torch.zeros(2, dtype=torch.int32))
    assert int(words[L.W_AUDITED]) == 2 and int(words[L.W_MISMATCH]) == 0
    # uniform Echo: a0 = 3, 9, 1 against 12, 0, 77
    words, _ = L.account_ref(hand_batch(METHOD_ECHO), value, status)
    assert calls_of(words)[(3, 0)] == 3 and int(words[L.W_AUDITED]) == 3 and int(words[L.W_MISMATCH]) == 3
    # CounterAdd, the relay id and an unnamed id: never audited
    for m, slot in ((METHOD_COUNTER_ADD, 5), (METHOD_RELAY, 15), (9, 9)):
        words, _ = L.account_ref(hand_batch(m), value, status)
        assert calls_of(words)[(slot, 0)] == 3 and int(words[L.W_AUDITED]) == 0 and int(words[L.W_MISMATCH]) == 0


def test_ledger_accumulates_resets_and_names():
    value, status = torch.tensor(VALUE), torch.tensor(STATUS, dtype=torch.int32)
    led = L.Ledger("cpu", actors=8)
    led.account(hand_batch(), value, status)
    r = led.read()
    assert r["calls"] == {"Calculator.Multiply": {"ok": 1, "not_delivered": 1, "other": 2},
                          "Echo": {"ok": 1, "rank_lost": 1}, "Counter.Add": {"ok": 1, "other": 1},
                          "none": {"no_method": 1}, "other": {"failed": 1, "no_actor": 1, "overflow": 1}}
    dsum, dxor = digest_by_hand(VALUE, STATUS)
    assert (r["sends"], r["messages"], r["audited"], r["mismatch"], r["load_oob"]) == (1, 12, 2, 1, 3)
    assert (r["digest_sum"], r["digest_xor"]) == (dsum, dxor)
    # busiest first, actors nobody addressed left out (the order among equal counts is topk's)
    assert r["hot"][:2] == [[3, 3], [1, 2]] and sorted(r["hot"][2:]) == [[0, 1], [2, 1], [5, 1], [7, 1]]
    assert led.read(top=1)["hot"] == [[3, 3]]
    led.account(hand_batch(9), value, status)  # the same replies again: the sum doubles, the xor cancels
    r = led.read()
    assert (r["sends"], r["messages"]) == (2, 24) and r["calls"]["method_9"]["ok"] == 3
    assert r["digest_sum"] == 2 * dsum & U64 and r["digest_xor"] == 0
    led.reset()
    r = led.read()
    assert r["calls"] == {} and r["hot"] == [] and all(r[k] == 0 for k in (
        "sends", "messages", "digest_sum", "digest_xor", "audited", "mismatch", "load_oob"))
    assert L.Ledger("cpu").read()["hot"] == []  # no load table
    with pytest.raises(TypeError):
        led.account(hand_batch(), value, status.to(torch.int64))
    with pytest.raises(TypeError):
        led.account(hand_batch(), value[:5], status)


def test_digest_sees_swaps_and_statuses_but_no_failed_value():
    g = torch.Generator().manual_seed(3)
    M = 300
    value = torch.randint(-2**62, 2**62, (M,), generator=g)
    status = torch.zeros(M, dtype=torch.int32)
    status[7], status[200] = STATUS_FAILED, 40
    base = L.digest(value, status)
    assert base == digest_by_hand(value.tolist(), status.tolist())
    v = value.clone()
    v[3], v[4] = value[4], value[3]  # two replies swapped between indices
    d = L.digest(v, status)
    assert d[0] != base[0] and d[1] != base[1]
    s = status.clone()
    s[10] = STATUS_FAILED  # a changed status
    d = L.digest(value, s)
    assert d[0] != base[0] and d[1] != base[1]
    v = value.clone()
    v[11] += 1  # a changed OK value
    d = L.digest(v, status)
    assert d[0] != base[0] and d[1] != base[1]
    v = value.clone()
    v[7], v[200] = 123, -9  # values of non-OK replies: no part of any contract
    assert L.digest(v, status) == base
    assert L.digest(value[:0], status[:0]) == (0, 0)


def test_send_all_with_retries_counts_every_message_once_cpu():
    M, n_c = 64, 16
    sc = retry_scenario(M, n_c)
    ex, state = world1(M + n_c, M + n_c)
    led = L.Ledger("cpu", actors=M + n_c)
    req = MsgBatch(sc["actor"], sc["a0"], None, None, sc["method"])
    val, st = ex.send_all(req, retries=2, ledger=led)
    assert torch.equal(st, sc["st"]) and torch.equal(val, sc["val"]) and ex.stats().retries == 2
    r = led.read()
    assert r["sends"] == 1 and r["messages"] == 80
    want = torch.bincount(sc["method"].to(torch.int64) * 8 + sc["st"].to(torch.int64), minlength=128)
    assert torch.equal(led.words[:128], want)
    n_failed = int((sc["st"] == STATUS_FAILED).sum())
    assert r["calls"] == {"RPCRetryTest.Call": {"ok": M - n_failed, "failed": n_failed}, "Counter.Add": {"ok": n_c}}
    assert (r["digest_sum"], r["digest_xor"]) == L.digest(val, st)
    assert r["audited"] == 0 and r["load_oob"] == 0 and torch.equal(led.load, torch.ones(M + n_c, dtype=torch.int64))
    # send() accounts too; without a ledger nothing changes
    ex.send(req, ledger=led)
    ex.send(req)
    ex.send_all(req)
    assert led.read()["sends"] == 2 and led.read()["messages"] == 160


def test_runtime_account_switch_cpu():
    from ptype_amd.runtime import DeviceRuntime

    M = 64
    ids = torch.arange(M, dtype=torch.int32)
    a = torch.arange(M, dtype=torch.int64) - 7
    b = MsgBatch(ids, a, a + 3, None, METHOD_CALC_MULTIPLY)
    rt = DeviceRuntime(torch.device("cpu"), actors=M, service="calculator", ledger=True)
    rt.place_local()
    for _ in range(2):
        val, st = rt.send("calculator", b)
    before = rt.stats()["ledger"]
    assert before["calls"] == {"Calculator.Multiply": {"ok": 2 * M}} and before["sends"] == 2
    assert before["audited"] == 2 * M and before["mismatch"] == 0 and before["digest_xor"] == 0
    assert before["digest_sum"] == 2 * L.digest(val, st)[0] & U64
    rt.send("calculator", b, account=False)
    assert rt.stats()["ledger"] == before
    rt.send("calculator", b, account=True, resend_overflow=False)
    rt.send("calculator", MsgBatch(ids, a, None, None, METHOD_RETRY_TEST), retries=1)
    after = rt.stats()["ledger"]
    assert after["sends"] == 4 and after["calls"]["Calculator.Multiply"]["ok"] == 3 * M
    assert sum(after["calls"]["RPCRetryTest.Call"].values()) == M
    assert after["hot"][0][1] == 4 and len(after["hot"]) == 8
    rt.close()
    rt = DeviceRuntime(torch.device("cpu"), actors=M, service="calculator")
    rt.place_local()
    rt.send("calculator", b)
    assert rt.ledger is None and "ledger" not in rt.stats()
    with pytest.raises(ValueError, match="ledger"):
        rt.send("calculator", b, account=True)
    rt.close()


def test_client_send_ledger_through_join_cpu(tmp_path, ports, monkeypatch):
    """Join -> NewClient -> Client.Send with ``gpu.ledger`` on a CPU runtime whose
    group Join formed: the elastic Send loop accounts the Send itself, once, after
    the retry rounds."""
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")

    cfg, srv, c = join_world1(C, tmp_path, ports, form_group=True, grace_s=0.3, ledger=True)
    try:
        rt = c.runtime
        assert rt.membership is not None and rt.ledger is not None
        M = rt.total_actors
        sc = retry_scenario(M)
        client = c.NewClient("w1", C.ConnConfig(retries=2))
        b = MsgBatch(sc["actor"], sc["a0"], None, None, METHOD_RETRY_TEST)
        val, st = client.Send(b, retries=2)
        assert torch.equal(st, sc["st"]) and torch.equal(val, sc["val"])
        led = c.Stats()["runtime"]["ledger"]
        n_failed = int((sc["st"] == STATUS_FAILED).sum())
        assert led["calls"] == {"RPCRetryTest.Call": {"ok": M - n_failed, "failed": n_failed}}
        assert led["sends"] == 1 and led["messages"] == M and led["hot"][0][1] == 1
        assert (led["digest_sum"], led["digest_xor"]) == L.digest(val, st)
        client.Send(b, account=False)
        assert c.Stats()["runtime"]["ledger"] == led
        mul = MsgBatch(sc["actor"], sc["a0"], sc["a0"], None, METHOD_CALC_MULTIPLY)
        client.Send(mul)
        led = c.Stats()["runtime"]["ledger"]
        assert led["calls"]["Calculator.Multiply"] == {"ok": M} and led["audited"] == M and led["mismatch"] == 0
        assert led["sends"] == 2
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_config_gpu_ledger_key(tmp_path):
    (tmp_path / "m.yml").write_text("name: x\n")
    p = tmp_path / "a.yml"
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu: {ledger: true}\n")
    assert C.ConfigFromFile(str(p)).gpu.ledger is True
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu:\n  actors: 64\n")
    assert C.ConfigFromFile(str(p)).gpu.ledger is False
    assert C.Config().gpu.ledger is False
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu:\n  ledger: 3\n")
    with pytest.raises(C.ConfigError):
        C.ConfigFromFile(str(p))
