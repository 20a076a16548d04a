"""The circuit breaker on CPU tensors (``ops/breaker.py``): the numpy model's
transitions one by one, a scripted sequence that goes through all of them (shared with
the GPU tests), then the runtime's ``breaker=`` switch with ``RPCRetryTest`` actors, its
order with coalescing, the cache, retries, the ledger and a gather, the resets, the
public API and the ``gpu.breaker*`` config keys.  All comparisons are exact integer
equality."""
import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import breaker as BR
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.gather import Gather
from ptype_amd.ops.records import (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_RETRY_TEST, METHOD_SEQ_FOLD, STATUS_BREAKER_OPEN,
                                   STATUS_FAILED, STATUS_NAMES, STATUS_NO_ACTOR, STATUS_NO_METHOD, STATUS_NOT_DELIVERED,
                                   STATUS_OK, STATUS_OVERFLOW, STATUS_RANK_LOST)

from test_coalesce import multiply_batch, runtime
from test_send_retries import join_world1

OPEN = 1 << 63
REJ = STATUS_BREAKER_OPEN


def ids_batch(actor, method=METHOD_RETRY_TEST):
    """A batch to ``actor`` whose a0 is the row index (the fake inner Sends echo it)."""
    actor = torch.as_tensor(actor, dtype=torch.int32)
    return MsgBatch(actor, torch.arange(actor.numel(), dtype=torch.int64), None, None, method)


def guarded(br, actor, status_of):
    """One guarded Send to ``actor`` whose inner Send answers ``(row, status_of(sub))``;
    returns ``(val, st)`` as lists."""
    val, st = br.send(ids_batch(actor), lambda sub: (sub.a0.clone(), status_of(sub).to(torch.int32)))[:2]
    return val.tolist(), st.tolist()


def fail_actor(*bad, status=STATUS_FAILED):
    return lambda sub: torch.where(torch.isin(sub.actor, torch.tensor(bad, dtype=torch.int32)), status, STATUS_OK)


def word(br, a):
    w = int(br.words()[a])
    return (w >> 63, (w >> 32) & 0x7FFFFFFF, w & 0xFFFFFFFF)


# ---------------------------------------------------------------- the model's transitions
def test_status_7_and_its_name():
    assert STATUS_BREAKER_OPEN == 7 and STATUS_NAMES[7] == "breaker_open" and BR.PENDING == 31
    assert BR.DEFAULT_TRIP_ON == (STATUS_FAILED, STATUS_NO_ACTOR, STATUS_NOT_DELIVERED)


def test_trips_at_exactly_threshold():
    br = BR.BreakerRef(actors=8, threshold=3, cooldown=4)
    assert guarded(br, [1, 2, 1], fail_actor(1))[1] == [STATUS_FAILED, STATUS_OK, STATUS_FAILED]
    assert word(br, 1) == (0, 0, 2) and br.read() == {"open": 0, "dirty": 1, "trips": 0, "closes": 0, "oob": 0}
    guarded(br, [2, 1], fail_actor(1))
    assert word(br, 1) == (1, 2 + 4, 3) and word(br, 2) == (0, 0, 0)
    assert br.read() == {"open": 1, "dirty": 1, "trips": 1, "closes": 0, "oob": 0} and br.tick == 3


def test_an_ok_in_the_same_send_resets_instead_of_tripping():
    br = BR.BreakerRef(actors=8, threshold=3, cooldown=4)
    st = (lambda sub: torch.where(sub.a0 == 4, STATUS_OK, STATUS_FAILED))
    guarded(br, [5] * 9, st)  # eight failures and one success to a clean actor
    assert word(br, 5) == (0, 0, 0) and br.read()["trips"] == 0 and br.read()["dirty"] == 0
    guarded(br, [5] * 2, fail_actor(5))
    assert word(br, 5) == (0, 0, 2)
    guarded(br, [5, 5], st)  # rows 0, 1 fail ... no row 4: still failing
    assert word(br, 5)[0] == 1
    # a success in a later Send resets the count of a dirty, closed actor
    br = BR.BreakerRef(actors=8, threshold=3, cooldown=4)
    guarded(br, [5, 5], fail_actor(5))
    guarded(br, [5], fail_actor())
    assert word(br, 5) == (0, 0, 0) and br.read()["dirty"] == 0


def test_rejects_for_the_cooldown_then_the_lowest_row_probes():
    br = BR.BreakerRef(actors=8, threshold=2, cooldown=3)
    guarded(br, [6, 6, 0], fail_actor(6))  # tick 1: opens until 4
    assert word(br, 6) == (1, 4, 2)
    sent = []

    def inner(sub):
        sent.append(sub.actor.tolist())
        return sub.a0.clone(), fail_actor(6)(sub).to(torch.int32)

    for tick in (2, 3):  # cooldown - 1 Sends reject everything to 6
        val, st = br.send(ids_batch([0, 6, 6, 1]), inner)[:2]
        assert st.tolist() == [STATUS_OK, REJ, REJ, STATUS_OK] and val.tolist() == [0, 0, 0, 3]
        assert sent[-1] == [0, 1] and word(br, 6) == (1, 4, 2)
    # tick 4: half-open -- row 2, the lowest row to 6, is the probe; it fails: open until 4 + 3
    val, st = br.send(ids_batch([0, 1, 6, 6, 6]), inner)[:2]
    assert st.tolist() == [STATUS_OK, STATUS_OK, STATUS_FAILED, REJ, REJ] and val.tolist() == [0, 1, 2, 0, 0]
    assert sent[-1] == [0, 1, 6] and word(br, 6) == (1, 7, 2) and br.read()["trips"] == 1
    assert guarded(br, [6], fail_actor(6))[1] == [REJ] and guarded(br, [6], fail_actor(6))[1] == [REJ]
    # tick 7: the probe succeeds: the word is 0 again
    val, st = guarded(br, [6, 6], fail_actor())
    assert st == [STATUS_OK, REJ] and word(br, 6) == (0, 0, 0)
    assert br.read() == {"open": 0, "dirty": 0, "trips": 1, "closes": 1, "oob": 0}
    assert guarded(br, [6, 6], fail_actor())[1] == [STATUS_OK, STATUS_OK]
    assert br.counters == {"sends": 8, "messages": 22, "rejected": 9, "sent": 13}


def test_a_probe_with_another_status_leaves_the_word():
    br = BR.BreakerRef(actors=4, threshold=1, cooldown=1)
    guarded(br, [2], fail_actor(2))  # tick 1: open until 2
    before = br.words().copy()
    for status in (STATUS_NO_METHOD, STATUS_OVERFLOW, STATUS_RANK_LOST):  # not in trip_on, not OK
        assert guarded(br, [2, 2], fail_actor(2, status=status))[1] == [status, REJ]
        assert np.array_equal(br.words(), before)
    # trip_on decides what a failure is
    br = BR.BreakerRef(actors=4, threshold=1, cooldown=1, trip_on=(STATUS_NO_METHOD,))
    guarded(br, [2], fail_actor(2))
    assert word(br, 2) == (0, 0, 0)
    guarded(br, [2], fail_actor(2, status=STATUS_NO_METHOD))
    assert word(br, 2) == (1, 3, 1)
    for bad in ((), (0,), (7,), (31,), (-1,)):
        with pytest.raises(ValueError):
            BR.BreakerRef(trip_on=bad)
    assert BR.trip_mask((1, 2, 3, 4, 5, 6)) == 0x7E and BR.trip_mask(STATUS_NOT_DELIVERED) == 1 << 5


def test_fails_saturate():
    br = BR.BreakerRef(actors=4, threshold=2**32 - 1, cooldown=1)
    br._ready()
    br.table[1] = np.uint64(2**32 - 3)
    br.ctr[BR.C_DIRTY] = 1
    guarded(br, [1], fail_actor(1))
    assert word(br, 1) == (0, 0, 2**32 - 2)
    guarded(br, [1] * 5, fail_actor(1))  # 2**32 - 2 + 5 saturates at 2**32 - 1: the threshold
    assert word(br, 1) == (1, 3, 2**32 - 1)
    assert guarded(br, [1] * 3, fail_actor(1))[1] == [STATUS_FAILED, REJ, REJ]
    assert word(br, 1) == (1, 4, 2**32 - 1)


def test_ids_outside_the_table_are_never_guarded():
    br = BR.BreakerRef(actors=4, threshold=1, cooldown=5)
    ids = [4, -1, 2, 1000, -2**31, 3]
    for _ in range(3):
        st = guarded(br, ids, lambda sub: torch.full((sub.M,), STATUS_FAILED))[1]
        assert [s for s, a in zip(st, ids) if not 0 <= a < 4] == [STATUS_FAILED] * 4
    assert st == [STATUS_FAILED, STATUS_FAILED, REJ, STATUS_FAILED, STATUS_FAILED, REJ]
    # counted by the admit passes only: the first Send had nothing open and ran none
    assert br.read() == {"open": 2, "dirty": 2, "trips": 2, "closes": 0, "oob": 8}
    assert br.words().shape == (4 + 5,) and br.words()[[0, 1]].tolist() == [0, 0]


def test_tick_restart():
    last = BR.MAX_TICK
    br = BR.BreakerRef(actors=4, threshold=1, cooldown=7, _start=last - 1)
    guarded(br, [1, 2], fail_actor(1))  # tick 2**31 - 2: until is held at the last tick
    assert word(br, 1) == (1, last, 1) and br.tick == last
    assert guarded(br, [1, 1], fail_actor(1))[1] == [STATUS_FAILED, REJ]  # the last tick: half-open
    assert br.tick == last + 1 and br.read()["open"] == 1
    st = guarded(br, [1, 1], fail_actor())[1]  # the tick would pass 2**31 - 1: everything closes, tick 1
    assert st == [STATUS_OK, STATUS_OK] and br.tick == 2 and int(br.words()[:4].sum()) == 0
    assert br.read() == {"open": 0, "dirty": 0, "trips": 1, "closes": 0, "oob": 0}
    guarded(br, [1], fail_actor(1))
    assert word(br, 1) == (1, 2 + 7, 1)
    assert guarded(br, [3, 1, 1], fail_actor(1))[1] == [STATUS_OK, REJ, REJ]  # (no stale probe claim passes)
    for bad in (0, last + 2):
        with pytest.raises(ValueError):
            BR.BreakerRef(_start=bad)
    for kw in ({"actors": 0}, {"threshold": 0}, {"cooldown": 0}, {"cooldown": last}):
        with pytest.raises(ValueError):
            BR.BreakerRef(**kw)


def test_the_tick_advances_when_the_inner_send_raises():
    br = BR.BreakerRef(actors=4)

    def boom(sub):
        raise RuntimeError("inner")

    with pytest.raises(RuntimeError, match="inner"):
        br.send(ids_batch([1]), boom)
    assert br.tick == 2 and br.counters["sends"] == 1


def test_send_calls_the_inner_send_once_or_never():
    calls = []

    def inner(sub):
        calls.append(sub.M)
        return sub.a0.clone(), torch.full((sub.M,), STATUS_FAILED, dtype=torch.int32)

    br = BR.Breaker("cpu", actors=4, threshold=1, cooldown=3)
    b = ids_batch([0, 1, 2, 3])
    assert br.send(b, inner)[1].tolist() == [STATUS_FAILED] * 4 and calls == [4]
    val, st = br.send(b, inner)  # K == 0 at world 1: skipped
    assert st.tolist() == [REJ] * 4 and val.tolist() == [0] * 4 and calls == [4]
    val, st = br.send(b, inner, collective=True)  # a rank of a group joins with an empty batch
    assert st.tolist() == [REJ] * 4 and calls == [4, 0]
    out = br.send(ids_batch([5, 6]), inner)  # K == M: the batch as it is
    assert calls == [4, 0, 2] and out[1].tolist() == [STATUS_FAILED] * 2
    assert br.counters == {"sends": 4, "messages": 14, "rejected": 8, "sent": 6}


# ---------------------------------------------------------------- a scripted sequence (shared with the GPU tests)
SCRIPT = {"threshold": 3, "cooldown": 2}


def script_batch(M, n, send, spread=48):
    """Send number ``send`` of the script: ids below ``min(n, spread)``, the second half of
    the batch sorted (runs of equal ids), a few ids outside the table, and exactly one
    message per Send to every actor of class 5 (see ``script_replies``)."""
    g = torch.Generator().manual_seed(1000 * M + send)
    ids = torch.randint(0, min(n, spread), (M,), generator=g)
    ids[M // 2:] = torch.sort(ids[M // 2:])[0]
    ids[ids % 8 == 5] += 1
    if M > 2:
        ids[M // 3] = 5
    if M > 40:
        ids[7], ids[M - 9], ids[M // 2 + 3] = n + 5, -1, -2**31
    return MsgBatch(ids.to(torch.int32), torch.randint(0, 4, (M,), generator=g), None, None, METHOD_RETRY_TEST)


def script_replies(sub, tick):
    """The inner Send of the script, a function of (actor, a0, tick).  By actor id mod 8:
    0 always fails (trips, every probe fails); 1 fails up to tick 3 (trips, a failed probe,
    then a successful one); 2 fails on odd a0 (failures and successes in one Send); 3
    answers STATUS_NO_METHOD (counts as neither); 4 answers STATUS_NO_ACTOR; 5 fails at
    tick 1 only (one message per Send: a count reset by a later OK); 6, 7 succeed."""
    a = sub.actor.to(torch.int64) & 0xFFFFFFFF
    k = a % 8
    st = torch.zeros(sub.M, dtype=torch.int64)
    st[k == 0] = STATUS_FAILED
    st[(k == 1) & (tick <= 3)] = STATUS_NOT_DELIVERED
    st[(k == 2) & (sub.a0 % 2 == 1)] = STATUS_FAILED
    st[k == 3] = STATUS_NO_METHOD
    st[k == 4] = STATUS_NO_ACTOR
    st[(k == 5) & (tick == 1)] = STATUS_FAILED
    return a * 1000 + sub.a0 * 10 + tick, st.to(torch.int32)


def run_script(ref, M, sends=9, also=None, to_device=None):
    """``sends`` guarded Sends of the script through ``ref`` (the numpy model) and, when
    given, through ``also`` (a ``Breaker`` on a GPU) with every output and the words
    compared after each.  Returns what the model went through."""
    seen = {"trips": 0, "resets_by_ok": 0, "probes_ok": 0, "probes_failed": 0, "rejected": 0}
    for send in range(sends):
        b = script_batch(M, ref.n, send)
        before = ref.words()[:ref.n].copy()
        now = ref.begin()
        inner = (lambda sub: script_replies(sub, now))
        val, st = ref.send(b, inner)[:2]
        if also is not None:
            assert also.begin() == now

            def inner_dev(sub):
                v, s = script_replies(MsgBatch(sub.actor.cpu(), sub.a0.cpu(), None, None, sub.method), now)
                return v.to(also.device), s.to(also.device)

            gval, gst = also.send(to_device(b), inner_dev)[:2]
            assert gst.dtype == torch.int32 and gval.dtype == torch.int64
            assert torch.equal(gst.cpu(), st) and torch.equal(gval.cpu(), val), (M, send)
            assert np.array_equal(also.words(), ref.words()), (M, send)
            assert also.counters == ref.counters and also.tick == ref.tick
            # the step kernel left its workspace as it found it: nothing touched, nothing observed
            assert int(also.ctr[BR.C_TOUCHED]) == 0 and not bool(also.obs.any()), (M, send)
        after = ref.words()[:ref.n]
        was_open, is_open_ = BR.is_open(before), BR.is_open(after)
        seen["trips"] += int((~was_open & is_open_).sum())
        seen["resets_by_ok"] += int((~was_open & (before != 0) & (after == 0)).sum())
        seen["probes_ok"] += int((was_open & ~is_open_).sum())
        seen["probes_failed"] += int((was_open & is_open_ & (BR.until_of(before) != BR.until_of(after))).sum())
        seen["rejected"] += int((st == REJ).sum())
    return seen


@pytest.mark.parametrize("n", [16, 4096])
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17])
def test_the_script_goes_through_every_transition(M, n):
    ref = BR.BreakerRef(actors=n, **SCRIPT)
    seen = run_script(ref, M)
    r = ref.read()
    assert r["trips"] == seen["trips"] and r["closes"] == seen["probes_ok"]
    if M >= 63:  # the inputs reach every transition, or the GPU comparison would show nothing
        assert all(v > 0 for v in seen.values()), seen
        assert r["oob"] > 0 and r["open"] > 0
    assert ref.counters["sends"] == 9 and ref.counters["rejected"] == seen["rejected"]


# ---------------------------------------------------------------- a CPU runtime with RPCRetryTest actors
def retry_batch(actors, passes_at, repeat=1):
    """``repeat`` RPCRetryTest messages to each of ``actors``, which answer OK from their
    ``passes_at``-th call on (the reply value is the actor's call count)."""
    a = torch.as_tensor(actors, dtype=torch.int32).repeat_interleave(repeat)
    return MsgBatch(a, torch.full((a.numel(),), passes_at, dtype=torch.int64), None, None, METHOD_RETRY_TEST)


def breaker_scenario(rt, dev="cpu", send=None):
    """Actor 5 fails until its 4th call, the others pass at once.  threshold 2, cooldown 3:
    it trips in Send 2, is rejected in Sends 3 and 4, probes and fails in Send 5, is
    rejected in 6 and 7 and probes OK in Send 8 -- its 4th call, which shows that no
    rejected call ever ran."""
    send = send or (lambda b: rt.send("calculator", b, breaker=True))
    ids = [5, 9, 5, 11]
    a = torch.tensor(ids, dtype=torch.int32, device=dev)
    b = MsgBatch(a, torch.tensor([4, 1, 4, 1], dtype=torch.int64, device=dev), None, None, METHOD_RETRY_TEST)
    want = [
        ([0, 1, 0, 1], [STATUS_FAILED, STATUS_OK, STATUS_FAILED, STATUS_OK]),      # calls 1, 2 of actor 5: trips
        ([0, 2, 0, 2], [REJ, STATUS_OK, REJ, STATUS_OK]),
        ([0, 3, 0, 3], [REJ, STATUS_OK, REJ, STATUS_OK]),
        ([0, 4, 0, 4], [STATUS_FAILED, STATUS_OK, REJ, STATUS_OK]),                # the probe: call 3 fails
        ([0, 5, 0, 5], [REJ, STATUS_OK, REJ, STATUS_OK]),
        ([0, 6, 0, 6], [REJ, STATUS_OK, REJ, STATUS_OK]),
        ([4, 7, 0, 7], [STATUS_OK, STATUS_OK, REJ, STATUS_OK]),                    # the probe: call 4 passes
        ([5, 8, 6, 8], [STATUS_OK] * 4),
    ]
    sent0 = rt.exchange.counters.sent
    for k, (wv, ws) in enumerate(want):
        val, st = send(b)[:2]
        assert st.tolist() == ws and val.tolist() == wv, k
    assert int(rt.state[5]) == 6 and rt.exchange.counters.sent - sent0 == 4 * 8 - 10
    n = rt.stats()["breaker"]
    assert n == {"sends": 8, "messages": 32, "rejected": 10, "sent": 22, "open": 0, "trips": 1, "closes": 1, "oob": 0,
                 "actors": rt.total_actors, "threshold": 2, "cooldown": 3}


def test_runtime_trips_rejects_and_probes_cpu():
    rt = runtime(breaker_threshold=2, breaker_cooldown=3)
    assert rt.breaker is False
    breaker_scenario(rt)
    rt.close()
    rt = runtime(breaker=True, breaker_threshold=2, breaker_cooldown=3)  # the runtime's default
    breaker_scenario(rt, send=lambda b: rt.send("calculator", b))
    rt.send("calculator", ids_batch([1]), breaker=False)
    assert rt.stats()["breaker"]["sends"] == 8
    rt.close()


def test_no_breaker_object_without_the_option_cpu():
    rt = runtime(coalesce=True, ledger=True)
    b = multiply_batch(500, 50, 64)
    rt.send("calculator", b)
    rt.send("calculator", b, retries=1)
    rt.send("calculator", b, cache=True)
    rt.send("calculator", b, coalesce=False, breaker=False)
    rt.breaker_reset()
    assert rt._breaker is None and rt.breaker is False and rt._breaker_seen is None
    assert rt.stats()["breaker"] == {"sends": 0, "messages": 0, "rejected": 0, "sent": 0, "open": 0, "trips": 0,
                                     "closes": 0, "oob": 0, "actors": 0, "threshold": 0, "cooldown": 0}
    rt.close()


@pytest.mark.parametrize("delivery", ["direct", "mailbox"])
def test_a_batch_that_trips_nothing_equals_the_plain_send_cpu(delivery):
    M = 3000
    g = torch.Generator().manual_seed(21)
    col = torch.tensor([METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_SEQ_FOLD], dtype=torch.int16)[
        torch.randint(0, 3, (M,), generator=g)]
    b = MsgBatch(torch.randint(0, 64, (M,), generator=g).to(torch.int32), torch.randint(1, 9, (M,), generator=g),
                 torch.randint(1, 9, (M,), generator=g), None, col)
    rt, rt_plain = runtime(delivery=delivery), runtime(delivery=delivery)
    for send in range(3):
        want = rt_plain.send("calculator", b)
        val, st = rt.send("calculator", b, breaker=True)
        # SeqFold replies are the actor's state before each fold: equal only if every actor saw its rows in order
        assert torch.equal(val, want[0]) and torch.equal(st, want[1]) and torch.equal(rt.state, rt_plain.state), send
    n = rt.stats()["breaker"]
    assert (n["sends"], n["messages"], n["rejected"], n["sent"], n["open"], n["trips"]) == (3, 3 * M, 0, 3 * M, 0, 0)
    rt.close()
    rt_plain.close()


def test_ordered_rows_keep_their_fifo_around_rejected_ones_cpu():
    """SeqFold rows to healthy actors between rows to an open actor: the admitted rows are
    compacted in message order, so every fold sees the state the plain Send gives it."""
    M = 900
    g = torch.Generator().manual_seed(22)
    actor = torch.randint(0, 6, (M,), generator=g).to(torch.int32)
    col = torch.where(actor == 0, METHOD_RETRY_TEST, METHOD_SEQ_FOLD).to(torch.int16)
    a0 = torch.where(actor == 0, 10**9, torch.randint(1, 99, (M,), generator=g))  # actor 0 never passes
    b = MsgBatch(actor, a0, None, None, col)
    rt, rt_plain = runtime(breaker_threshold=1, breaker_cooldown=50), runtime()
    folds = actor != 0
    for send in range(3):
        want = rt_plain.send("calculator", b)
        val, st = rt.send("calculator", b, breaker=True)
        assert torch.equal(val[folds], want[0][folds]) and torch.equal(st[folds], want[1][folds]), send
        assert bool((st[~folds] == (STATUS_FAILED if send == 0 else REJ)).all())
    assert torch.equal(rt.state[1:], rt_plain.state[1:]) and int(rt.state[0]) == int((~folds).sum())
    rt.close()
    rt_plain.close()


# ---------------------------------------------------------------- the order with the other wrappers
def test_coalesced_followers_inherit_the_rejection_cpu():
    rt = runtime(breaker_threshold=1, breaker_cooldown=9)
    bad = MsgBatch(torch.tensor([70, 70, 3], dtype=torch.int32), torch.tensor([2, 2, 2]), torch.tensor([3, 3, 3]), None,
                   METHOD_CALC_MULTIPLY)  # actor 70 is not registered: STATUS_NO_ACTOR trips it
    rt2 = runtime(actors=128, breaker_threshold=1, breaker_cooldown=9, breaker_actors=100)
    for r in (rt, rt2):
        sent = r.exchange.counters.sent
        val, st = r.send("calculator", bad, coalesce=True, breaker=True)
        want = [STATUS_NO_ACTOR, STATUS_NO_ACTOR, STATUS_OK] if r is rt else [STATUS_OK] * 3
        assert st.tolist() == want and r.exchange.counters.sent - sent == 2  # the leaders
        val, st = r.send("calculator", bad, coalesce=True, breaker=True)
        if r is rt:  # ids >= total_actors (64) are outside the table: never guarded
            assert st.tolist() == want and r.stats()["breaker"]["open"] == 0
    # a guarded id: the leader is rejected, the follower inherits (0, 7), nothing travels for them
    rt2.close()
    rt.close()
    rt = runtime(breaker_threshold=1, breaker_cooldown=9)
    b = MsgBatch(torch.tensor([7, 7, 3, 7], dtype=torch.int32), torch.tensor([10**9, 10**9, 1, 10**9]), None, None,
                 torch.tensor([METHOD_RETRY_TEST] * 4, dtype=torch.int16))
    rt.send("calculator", b, breaker=True)
    assert rt.stats()["breaker"]["open"] == 1
    echo = MsgBatch(b.actor, torch.tensor([4, 4, 4, 5]), None, None, METHOD_ECHO)
    sent = rt.exchange.counters.sent
    val, st = rt.send("calculator", echo, coalesce=True, breaker=True)
    assert st.tolist() == [REJ, REJ, STATUS_OK, REJ] and val.tolist() == [0, 0, 4, 0]
    assert rt.exchange.counters.sent - sent == 1 and rt.stats()["coalesce"]["executed"] == 3
    assert rt.stats()["breaker"]["messages"] == 4 + 3  # the breaker saw the leaders
    rt.close()


def test_the_cache_never_stores_a_rejection_and_a_hit_bypasses_the_breaker_cpu():
    rt = runtime(breaker_threshold=1, breaker_cooldown=2)
    echo = MsgBatch(torch.tensor([7, 3], dtype=torch.int32), torch.tensor([4, 4]), None, None, METHOD_ECHO)
    val, st = rt.send("calculator", echo, cache=True, breaker=True)  # both stored
    assert st.tolist() == [STATUS_OK] * 2
    rt.send("calculator", retry_batch([7], 10**9), breaker=True)  # actor 7 opens (tick 2, until 4)
    assert rt.stats()["breaker"]["open"] == 1
    other = MsgBatch(echo.actor, torch.tensor([5, 5]), None, None, METHOD_ECHO)
    sent = rt.exchange.counters.sent
    val, st = rt.send("calculator", other, cache=True, breaker=True)  # a miss to an open actor: rejected, not stored
    assert st.tolist() == [REJ, STATUS_OK] and val.tolist() == [0, 5] and rt.exchange.counters.sent - sent == 1
    val, st = rt.send("calculator", echo, cache=True, breaker=True)  # a hit is never sent: no breaker in its way
    assert st.tolist() == [STATUS_OK] * 2 and val.tolist() == [4, 4] and rt.exchange.counters.sent - sent == 1
    # tick 5: half-open.  Were the rejection cached, this would be a hit with status 7; it is the probe
    val, st = rt.send("calculator", other, cache=True, breaker=True)
    assert st.tolist() == [STATUS_OK] * 2 and val.tolist() == [5, 5]
    n = rt.stats()
    assert n["breaker"]["closes"] == 1 and n["breaker"]["open"] == 0 and n["cache"]["hits"] == 3
    rt.close()


def test_the_probe_is_retried_inside_and_its_final_status_decides_cpu():
    rt = runtime(breaker_threshold=1, breaker_cooldown=2)
    b = retry_batch([5, 6], 4)  # both pass at their 4th call
    val, st = rt.send("calculator", b, breaker=True, retries=1)  # calls 1, 2: the final status is FAILED
    assert st.tolist() == [STATUS_FAILED] * 2 and rt.stats()["breaker"]["trips"] == 2
    assert rt.send("calculator", b, breaker=True, retries=1)[1].tolist() == [REJ] * 2
    assert rt.state[5:7].tolist() == [2, 2]  # a breaker wraps the retried call: no attempt ran
    val, st = rt.send("calculator", b, breaker=True, retries=1)  # the probes: call 3 fails, the retry's call 4 passes
    assert st.tolist() == [STATUS_OK] * 2 and val.tolist() == [4, 4]
    assert rt.stats()["breaker"]["closes"] == 2 and rt.stats()["breaker"]["open"] == 0
    rt.close()


def test_the_ledger_counts_rejections_as_other_and_a_gather_sees_non_ok_rows_cpu():
    rt = runtime(ledger=True, breaker_threshold=1, breaker_cooldown=9)
    rt.send("calculator", retry_batch([5], 10**9), breaker=True, account=False)
    b = MsgBatch(torch.tensor([5, 6, 5, 6], dtype=torch.int32), torch.tensor([1, 2, 3, 4]), None, None, METHOD_ECHO)
    g = Gather(torch.tensor([0, 0, 1, 1], dtype=torch.int32), 2, "sum")
    val, st = rt.send("calculator", b, breaker=True, gather=g)
    assert st.tolist() == [REJ, STATUS_OK, REJ, STATUS_OK]
    r = rt.stats()["ledger"]
    assert r["calls"] == {"Echo": {"ok": 2, "other": 2}} and r["messages"] == 4 and r["sends"] == 1
    assert g.value.tolist() == [2, 4] and g.n_ok.tolist() == [1, 1] and g.count.tolist() == [2, 2]
    assert g.status.tolist() == [REJ, REJ] and g.bad_row.tolist() == [0, 2]
    rt.close()
    rt = runtime()
    with pytest.raises(ValueError, match="ledger"):
        rt.send("calculator", b, breaker=True, account=True)
    rt.close()


def test_breaker_with_every_wrapper_equals_itself_without_them_cpu():
    """coalesce + cache + retries + ledger + gather around the breaker: the statuses are
    those of the guarded Send alone.  (Pure rows only, so coalescing and the cache cannot
    change what runs on an actor; the rows to unregistered actors have keys of their own,
    so none of them is a follower that would inherit a probe's reply.)"""
    M = 2000
    g = torch.Generator().manual_seed(23)
    actor = torch.randint(0, 80, (M,), generator=g).to(torch.int32)  # 64..79 are not registered: they trip
    a0 = torch.where(actor >= 64, torch.arange(M), torch.randint(0, 5, (M,), generator=g))
    b = MsgBatch(actor, a0, torch.randint(0, 5, (M,), generator=g), None, METHOD_CALC_MULTIPLY)
    kw = {"breaker_threshold": 2, "breaker_cooldown": 2, "breaker_actors": 72}
    rt, rt_alone = runtime(ledger=True, **kw), runtime(**kw)
    grp = Gather((actor % 16).to(torch.int32), 16, "sum")
    for send in range(5):
        want = rt_alone.send("calculator", b, breaker=True)
        val, st = rt.send("calculator", b, breaker=True, coalesce=True, cache=True, retries=2, gather=grp)
        assert torch.equal(st, want[1]) and torch.equal(val, want[0]), send
        ok = st == STATUS_OK
        assert int(grp.n_ok.sum()) == int(ok.sum()) and int(grp.value.sum()) == int(val[ok].sum())
    n = rt.stats()["breaker"]
    assert n["trips"] == 8 and n["oob"] > 0 and n["rejected"] > 0 and n["open"] == 8
    assert int((st == REJ).sum()) > 0 and int((st == STATUS_NO_ACTOR).sum()) > 0  # ids 72..79 are never guarded
    assert rt.stats()["ledger"]["messages"] == 5 * M
    rt.close()
    rt_alone.close()


# ---------------------------------------------------------------- resets
def test_breaker_reset_and_the_registry_change_cpu():
    from ptype_amd.parallel.replicas import ReplicaRouter

    rt = runtime(breaker_threshold=1, breaker_cooldown=9)
    fail = retry_batch([5], 10**9)
    probe = retry_batch([5], 1)
    rt.send("calculator", fail, breaker=True)
    assert rt.send("calculator", probe, breaker=True)[1].tolist() == [REJ]
    rt.breaker_reset()
    assert rt.stats()["breaker"]["open"] == 0 and rt._breaker.tick == 3  # the tick goes on
    assert rt.send("calculator", probe, breaker=True)[1].tolist() == [STATUS_OK]
    rt.send("calculator", fail, breaker=True)
    assert rt.send("calculator", probe, breaker=True)[1].tolist() == [REJ]
    rt.host("other")  # may change which actors answer: the next guarded Send starts closed
    assert rt.send("calculator", probe, breaker=True)[1].tolist() == [STATUS_OK]
    assert rt.stats()["breaker"]["trips"] == 2 and rt.stats()["breaker"]["open"] == 0
    rt.close()
    # the same router whose record set moved resets; another router object alone does not
    recs = [{"replica": True, "node": f"n{i}", "address": "127.0.0.1", "port": 7000 + i, "rank": 0, "count": 64}
            for i in range(2)]
    rt = runtime(breaker_threshold=1, breaker_cooldown=9)
    r1, r2 = (ReplicaRouter("calculator", 1, "10.0.0.1", 0, records=recs[:1]) for _ in range(2))
    rt.send("calculator", fail, router=r1, breaker=True)
    assert rt.send("calculator", probe, router=r1, breaker=True)[1].tolist() == [REJ]
    assert rt.send("calculator", probe, router=r2, breaker=True)[1].tolist() == [REJ]
    assert rt.send("calculator", probe, breaker=True)[1].tolist() == [REJ]
    assert rt.send("calculator", probe, router=r2, breaker=True)[1].tolist() == [REJ]
    r2.set_records(recs)
    assert rt.send("calculator", probe, router=r2, breaker=True)[1].tolist() == [STATUS_OK]
    rt.close()


def test_guarded_send_is_refused_under_capture_cpu():
    rt = runtime()
    b = multiply_batch(100, 10, 64)
    rt.send("calculator", b)
    rt.exchange._capturing = True
    with pytest.raises(ValueError, match="breaker=True.*captur"):
        rt.send("calculator", b, breaker=True)
    with pytest.raises(ValueError, match="captur"):
        rt.send("calculator", b, breaker=True, cache=True)
    rt.send("calculator", b)  # a plain Send is not
    assert rt._breaker is None
    rt.exchange._capturing = False
    rt.close()


def test_bad_runtime_settings_are_refused():
    for kw in ({"breaker_threshold": 0}, {"breaker_cooldown": 0}, {"breaker_cooldown": 2**31 - 1},
               {"breaker_actors": -1}, {"breaker_trip_on": (0,)}, {"breaker_trip_on": (7,)}):
        with pytest.raises(ValueError):
            runtime(**kw)
    rt = runtime(breaker_trip_on=(STATUS_NO_METHOD,), breaker_threshold=1)
    rt.send("calculator", MsgBatch(torch.tensor([3], dtype=torch.int32), torch.tensor([1]), None, None, 99),
            breaker=True)
    assert rt.stats()["breaker"]["open"] == 1
    rt.close()


# ---------------------------------------------------------------- the public API and the config keys
def test_client_send_breaker_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, srv, c = join_world1(C, tmp_path, ports, form_group=True, grace_s=0.3, breaker_threshold=2,
                              breaker_cooldown=3)
    try:
        rt = c.runtime
        assert rt.breaker is False and (rt.breaker_threshold, rt.breaker_cooldown, rt.breaker_actors) == (2, 3, 0)
        client = c.NewClient("w1", C.ConnConfig())
        client.Send(multiply_batch(300, 20, rt.total_actors))
        assert rt._breaker is None
        assert c.Stats()["runtime"]["breaker"]["sends"] == 0
        b = retry_batch([5, 9, 5, 11], 1)
        b = MsgBatch(b.actor, torch.tensor([4, 1, 4, 1]), None, None, METHOD_RETRY_TEST)
        statuses = [client.Send(b, breaker=True)[1].tolist() for _ in range(8)]
        assert statuses[1] == [REJ, STATUS_OK, REJ, STATUS_OK] and statuses[3][0] == STATUS_FAILED
        assert statuses[6] == [STATUS_OK, STATUS_OK, REJ, STATUS_OK] and statuses[7] == [STATUS_OK] * 4
        n = c.Stats()["runtime"]["breaker"]
        assert n == {"sends": 8, "messages": 32, "rejected": 10, "sent": 22, "open": 0, "trips": 1, "closes": 1,
                     "oob": 0, "actors": rt.total_actors, "threshold": 2, "cooldown": 3}
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_gpu_breaker_config_default_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, srv, c = join_world1(C, tmp_path, ports, breaker=True, breaker_threshold=1, breaker_cooldown=4,
                              breaker_actors=32)
    try:
        assert c.runtime.breaker is True
        client = c.NewClient("w1", C.ConnConfig())
        b = retry_batch([5, 40], 10**9)
        assert client.Send(b)[1].tolist() == [STATUS_FAILED] * 2  # no argument: gpu.breaker
        assert client.Send(b)[1].tolist() == [REJ, STATUS_FAILED]  # id 40 is past gpu.breaker_actors
        assert client.Send(b, breaker=False)[1].tolist() == [STATUS_FAILED] * 2
        n = c.Stats()["runtime"]["breaker"]
        assert (n["sends"], n["open"], n["oob"], n["actors"], n["cooldown"]) == (2, 1, 1, 32, 4)
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_config_gpu_breaker_keys(tmp_path):
    (tmp_path / "m.yml").write_text("name: x\n")
    p = tmp_path / "a.yml"
    p.write_text("service_name: calc\netcd_config_file: m.yml\n"
                 "gpu: {breaker: true, breaker_threshold: 3, breaker_cooldown: 2147483646, breaker_actors: 4096}\n")
    g = C.ConfigFromFile(str(p)).gpu
    assert g.breaker is True and (g.breaker_threshold, g.breaker_cooldown, g.breaker_actors) == (3, 2**31 - 2, 4096)
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu:\n  actors: 64\n")
    g = C.ConfigFromFile(str(p)).gpu
    assert g.breaker is False and (g.breaker_threshold, g.breaker_cooldown, g.breaker_actors) == (5, 8, 0)
    d = C.Config().gpu
    assert d.breaker is False and (d.breaker_threshold, d.breaker_cooldown, d.breaker_actors) == (5, 8, 0)
    for bad in ("breaker: 3", "breaker_threshold: 0", "breaker_threshold: -1", "breaker_threshold: true",
                "breaker_cooldown: 0", "breaker_cooldown: 2147483647", "breaker_cooldown: soon", "breaker_actors: -1",
                "breaker_actors: 268435457"):
        p.write_text(f"service_name: calc\netcd_config_file: m.yml\ngpu:\n  {bad}\n")
        with pytest.raises(C.ConfigError):
            C.ConfigFromFile(str(p))
