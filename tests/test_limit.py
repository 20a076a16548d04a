"""The rate limiter on CPU tensors (``ops/limit.py``): the numpy model against an
independent oracle -- a plain Python loop over the messages, one dict of buckets -- over a
scripted sequence that reaches every case (shared with the GPU tests), ``send()``'s
plumbing, then the runtime's ``limit=`` switch, its place among the other wrappers, the
public API and the ``gpu.limit*`` config keys.  All comparisons are exact integer equality.

Two cases the bucket arithmetic cannot reach through ``send()`` alone, because a limited
Send always refills at least ``rate >= 1`` tokens before it spends: ``q == 0`` (and with
it K == 0) needs two admissions at one tick, which ``admit()`` allows and the script does
once; and no admission can leave a word 0 (``spent' + q == 0`` needs ``q == 0`` with a
full bucket, but a full bucket admits a row), so "the word becoming 0" is reached by the
tick restart and ``reset()`` only.  ``spent`` returning to 0 by a refill is reached and
asserted."""
import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import limit as LM
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.gather import Gather
from ptype_amd.ops.records import (METHOD_ECHO, METHOD_RETRY_TEST, STATUS_BREAKER_OPEN, STATUS_FAILED, STATUS_NAMES,
                                   STATUS_OK, STATUS_THROTTLED)

from test_breaker import ids_batch, retry_batch
from test_coalesce import multiply_batch, runtime
from test_send_retries import join_world1

THR = STATUS_THROTTLED
_U32 = 0xFFFFFFFF


# ---------------------------------------------------------------- the oracle
class Oracle:
    """The limiter as a sequential loop: message by message, one token at a time."""

    def __init__(self, n, rate, burst, tick=1):
        self.n, self.rate, self.burst, self.tick = n, rate, burst, tick
        self.buckets = {}  # actor -> [last, spent]
        self.throttled = self.oob = 0
        self.seen = {"full": 0, "partial": 0, "q0": 0, "capped": 0, "idle_refill": 0, "spent_to_zero": 0, "oob": 0,
                     "restart": 0}

    def begin(self):
        if self.tick > LM.MAX_TICK:
            self.buckets.clear()
            self.tick = 1
            self.seen["restart"] += 1
        return self.tick

    def admit(self, ids):
        """True per message that travels, at the current tick."""
        now, first, took, lost, out = self.begin(), set(), {}, {}, []
        for a in ids:
            a &= _U32
            if a >= self.n:
                self.oob += 1
                self.seen["oob"] += 1
                out.append(True)
                continue
            if a not in first:  # the bucket's refill, once per admission
                first.add(a)
                last, spent = self.buckets.get(a, (0, 0))
                if spent:
                    refill = min((now - last) * self.rate, _U32)
                    self.seen["capped"] += refill > spent
                    self.seen["idle_refill"] += now - last >= 2 and refill < spent
                    spent = max(spent - refill, 0)
                    self.seen["spent_to_zero"] += spent == 0
                self.buckets[a] = [now, spent]
                took[a] = lost[a] = 0
                self.seen["full"] += spent == 0
            b = self.buckets[a]
            if b[1] < self.burst:
                b[1] += 1
                took[a] += 1
                out.append(True)
            else:
                self.throttled += 1
                lost[a] += 1
                out.append(False)
        self.seen["partial"] += sum(1 for a in first if took[a] and lost[a])
        self.seen["q0"] += sum(1 for a in first if not took[a])
        return out

    def end(self):
        self.tick += 1

    def words(self):
        w = np.zeros(self.n + 2, dtype=np.uint64)
        for a, (last, spent) in self.buckets.items():
            if spent:
                w[a] = np.uint64(last << 32 | spent)
        w[self.n], w[self.n + 1] = self.throttled, self.oob
        return w


# ---------------------------------------------------------------- a scripted sequence (shared with the GPU tests)
SCRIPT = {"rate": 1, "burst": 5}
DOUBLE = 4  # the Send of the script whose tokens are spent twice at one tick


def script_batch(M, n, send, spread=48):
    """Send number ``send`` of the script: half of the rows to four busy ids, the others
    below ``min(n, spread)``, the second half of the batch sorted (runs of equal ids), ids
    that are 1 mod 4 only in every third Send (idle Sends in between), one id with a single
    row in the Sends 0, 2, 4, ... and a few ids outside the table."""
    g = torch.Generator().manual_seed(1000 * M + send)
    ids = torch.randint(0, min(n, spread), (M,), generator=g)
    busy = torch.randint(0, 4, (M,), generator=g)
    ids = torch.where(torch.rand(M, generator=g) < 0.5, busy, ids)
    ids[M // 2:] = torch.sort(ids[M // 2:])[0]
    if send % 3:
        ids[ids % 4 == 1] += 1
    ids[ids == 7] = 6
    if M > 2 and send % 2 == 0:
        ids[M // 3] = 7
    if M > 40:
        ids[7], ids[M - 9], ids[M // 2 + 3] = n + 5, -1, -2**31
    return MsgBatch(ids.to(torch.int32), torch.randint(0, 4, (M,), generator=g), None, None, METHOD_RETRY_TEST)


def script_replies(sub, tick):
    """The inner Send of the script, a function of (actor, a0, tick): odd a0 fails."""
    a = sub.actor.to(torch.int64) & _U32
    return a * 1000 + sub.a0 * 10 + tick % 7, torch.where(sub.a0 % 2 == 1, STATUS_FAILED, STATUS_OK).to(torch.int32)


def run_script(ref, M, sends=9, also=None, to_device=None):
    """``sends`` limited Sends of the script through ``ref`` (the numpy model) and the
    oracle, and, when given, through ``also`` (a ``Limiter`` on a GPU), with every output,
    the words and the counters compared after each.  Returns what the oracle went through."""
    orc = Oracle(ref.n, ref.rate, ref.burst, ref.tick)

    def same_state(send):
        assert np.array_equal(ref.words(), orc.words()), (M, send)
        if also is not None:
            assert np.array_equal(also.words(), ref.words()), (M, send)
            assert also.counters == ref.counters and also.tick == ref.tick and also.over == ref.over
            assert also.at_rest(), (M, send)  # demand, bins, over and n_touched are zero again

    same_state(-1)
    for send in range(sends):
        b = script_batch(M, ref.n, send)
        ids = b.actor.tolist()
        if send == DOUBLE:  # spend this batch's tokens, and stay at the tick: the Send below finds what is left
            orc.admit(ids)
            ref.begin()
            ref.admit(b)
            if also is not None:
                also.begin()
                also.admit(to_device(b))
            same_state(send)
        now = ref.begin()
        assert orc.begin() == now
        passes = torch.tensor(orc.admit(ids), dtype=torch.bool)
        orc.end()
        v, s = script_replies(b, now)
        want_val, want_st = torch.where(passes, v, 0), torch.where(passes, s, THR).to(torch.int32)
        val, st = ref.send(b, lambda sub: script_replies(sub, now))[:2]
        assert torch.equal(st, want_st) and torch.equal(val, want_val), (M, send)
        assert ref.tick == orc.tick
        if also is not None:
            assert also.begin() == now

            def inner_dev(sub):
                v, s = script_replies(MsgBatch(sub.actor.cpu(), sub.a0.cpu(), None, None, sub.method), now)
                return v.to(also.device), s.to(also.device)

            gval, gst = also.send(to_device(b), inner_dev)[:2]
            assert gst.dtype == torch.int32 and gval.dtype == torch.int64
            assert torch.equal(gst.cpu(), st) and torch.equal(gval.cpu(), val), (M, send)
        same_state(send)
    return orc.seen


@pytest.mark.parametrize("start", [None, LM.MAX_TICK - 2])
@pytest.mark.parametrize("n", [16, 4096])
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17])
def test_the_model_against_the_oracle_and_the_script_reaches_every_case(M, n, start):
    ref = LM.LimiterRef(actors=n, _start=start, **SCRIPT)
    seen = run_script(ref, M)
    if M >= 63:  # the inputs reach every case, or the comparisons would show nothing
        want = set(seen) - ({"restart"} if start is None else set())
        assert all(seen[k] > 0 for k in want), seen
        assert ref.read()["throttled"] > 0 and ref.read()["oob"] == seen["oob"]
    assert seen["restart"] == (0 if start is None else 1)
    assert ref.counters["sends"] == 9 and ref.tick == (10 if start is None else 7)
    assert ref.counters["sent"] + ref.counters["rejected"] == ref.counters["messages"] == 9 * M


# ---------------------------------------------------------------- the model by hand
def echo(sub):
    return sub.a0.clone(), torch.zeros(sub.M, dtype=torch.int32)


def limited(lim, actor, inner=echo, **kw):
    val, st = lim.send(ids_batch(actor), inner, **kw)[:2]
    return val.tolist(), st.tolist()


def word(lim, a):
    w = int(lim.words()[a])
    return (w >> 32, w & _U32)


def test_status_8_and_its_name():
    assert STATUS_THROTTLED == 8 and STATUS_NAMES[8] == "throttled" and LM.PENDING == 31
    assert (LM.levels(1), LM.levels(16), LM.levels(17), LM.levels(3 * 2048 + 17), LM.levels(2**31 - 1)) == (1, 1, 2, 4, 8)


def test_buckets_by_hand():
    lim = LM.LimiterRef(actors=8, rate=2, burst=3)
    assert limited(lim, [1, 2, 1, 1, 1, 9]) == ([0, 1, 2, 3, 0, 5], [0, 0, 0, 0, THR, 0])  # the first three rows of 1
    assert word(lim, 1) == (1, 3) and word(lim, 2) == (1, 1) and lim.read() == {"throttled": 1, "oob": 1}
    assert limited(lim, [1, 1, 1])[1] == [0, 0, THR] and word(lim, 1) == (2, 3)  # two tokens gained
    assert limited(lim, [3])[1] == [0] and limited(lim, [3])[1] == [0]  # actor 1 idle: ticks 3, 4
    assert limited(lim, [1, 1, 1, 1])[1] == [0, 0, 0, THR] and word(lim, 1) == (5, 3)  # the refill stops at burst
    assert limited(lim, [2])[1] == [0] and word(lim, 2) == (6, 1)  # spent went back to 0, then one token
    assert lim.counters == {"sends": 6, "messages": 16, "rejected": 3, "sent": 13} and lim.tick == 7
    lim.reset()
    assert not lim.words()[:8].any() and lim.tick == 7 and lim.read() == {"throttled": 3, "oob": 1}
    # negative ids and ids >= n are never limited
    assert limited(lim, [-1, -1, -1, -1, 8, 8, 8, 8, -2**31])[1] == [0] * 9 and lim.read()["oob"] == 10


def test_the_refill_saturates_at_32_bits():
    lim = LM.LimiterRef(actors=4, rate=2**32 - 1, burst=2**32 - 1)
    lim._ready()
    lim.table[1] = np.uint64(1 << 32 | (2**32 - 1))  # empty since tick 1
    lim.tick = 3
    assert limited(lim, [1, 1])[1] == [0, 0] and word(lim, 1) == (3, 2)  # min(2 * rate, 2^32 - 1) refills all of it


def test_tick_restart():
    last = LM.MAX_TICK
    lim = LM.LimiterRef(actors=4, rate=1, burst=2, _start=last)
    assert limited(lim, [1, 1, 1])[1] == [0, 0, THR] and word(lim, 1) == (last, 2) and lim.tick == last + 1
    assert limited(lim, [1, 1, 1])[1] == [0, 0, THR]  # the tick would pass 2**31 - 1: every bucket full, tick 1
    assert word(lim, 1) == (1, 2) and lim.tick == 2
    for bad in (0, last + 2):
        with pytest.raises(ValueError):
            LM.LimiterRef(_start=bad)


def test_setting_validation():
    for kw in ({"actors": 0}, {"actors": 2**28 + 1}, {"rate": 0}, {"rate": 2**32}, {"burst": 0}, {"burst": 2**32},
               {"rate": -1}):
        with pytest.raises(ValueError):
            LM.LimiterRef(**kw)
    LM.LimiterRef(actors=2**28, rate=2**32 - 1, burst=2**32 - 1)


# ---------------------------------------------------------------- send() plumbing
def test_the_untouched_batch_is_passed_on_when_nothing_is_over_quota():
    got = []

    def inner(sub):
        got.append(sub)
        return sub.a0.clone(), torch.zeros(sub.M, dtype=torch.int32), "more"

    lim = LM.Limiter("cpu", actors=8, rate=1, burst=2)
    b = ids_batch([1, 2, 1, 3])
    out = lim.send(b, inner)
    assert got[0] is b and out[2] == "more" and lim.over == 0
    out = lim.send(b, inner)  # actor 1 has one token: a sub-batch travels, the tail of the result is kept
    assert got[1] is not b and got[1].actor.tolist() == [1, 2, 3] and out[1].tolist() == [0, 0, THR, 0]
    assert out[2] == "more" and lim.over == 1
    empty = ids_batch([])
    assert lim.send(empty, inner)[1].numel() == 0 and got[2] is empty  # M == 0: nothing is over quota


def test_k_0_with_and_without_collective():
    calls = []

    def inner(sub):
        calls.append(sub.M)
        return sub.a0.clone(), torch.zeros(sub.M, dtype=torch.int32)

    lim = LM.Limiter("cpu", actors=8, rate=1, burst=2)
    b = ids_batch([1, 1, 2, 2])
    lim.begin()
    assert lim.admit(b) is None  # the tokens of this tick are gone
    val, st = lim.send(b, inner)  # K == 0 at world 1: skipped
    assert st.tolist() == [THR] * 4 and val.tolist() == [0] * 4 and calls == []
    lim.begin()
    lim.admit(ids_batch([1, 2]))  # one token each per tick
    val, st = lim.send(b, inner, collective=True)  # a rank of a group joins with an empty batch
    assert st.tolist() == [THR] * 4 and calls == [0]
    assert lim.counters == {"sends": 2, "messages": 8, "rejected": 8, "sent": 0} and lim.tick == 3


def test_the_tick_advances_when_the_inner_send_raises():
    lim = LM.LimiterRef(actors=4, burst=1)

    def boom(sub):
        raise RuntimeError("inner")

    for ids in ([1], [1, 1]):  # the untouched batch, and a cut one
        with pytest.raises(RuntimeError, match="inner"):
            lim.send(ids_batch(ids), boom)
    assert lim.tick == 3 and lim.counters["sends"] == 2 and word(lim, 1) == (2, 1)  # the tokens are spent


# ---------------------------------------------------------------- a CPU runtime
def echo_batch(actor, a0=None, dev="cpu"):
    actor = torch.as_tensor(actor, dtype=torch.int32)
    a0 = torch.arange(actor.numel(), dtype=torch.int64) if a0 is None else torch.as_tensor(a0, dtype=torch.int64)
    return MsgBatch(actor.to(dev), a0.to(dev), None, None, METHOD_ECHO)


def limit_scenario(rt, dev="cpu", send=None, sends=4):
    """``limit=True`` through a runtime with rate 2 and burst 3 against the model: Echo rows
    (value a0, STATUS_OK) to ids of which some are over their quota in every Send, and ids
    outside the table when ``limit_actors`` is smaller than the service."""
    send = send or (lambda b: rt.send("calculator", b, limit=True))
    n = rt.limit_actors or rt.total_actors
    ref = LM.LimiterRef(actors=n, rate=rt.limit_rate, burst=rt.limit_burst)
    g = torch.Generator().manual_seed(41)
    sent0 = rt.exchange.counters.sent
    for k in range(sends):
        ids = torch.randint(0, rt.total_actors, (300,), generator=g)
        ids[torch.rand(300, generator=g) < 0.3] = 5
        ids[100:160] = torch.sort(ids[100:160])[0]
        b = echo_batch(ids)
        want = ref.send(b, echo)
        val, st = send(echo_batch(ids, dev=dev))[:2]
        assert torch.equal(st.cpu(), want[1]) and torch.equal(val.cpu(), want[0]), k
        assert int((st == THR).sum()) > 0 and int((st == STATUS_OK).sum()) > 0
    assert np.array_equal(rt._limiter.words(), ref.words())
    assert rt.exchange.counters.sent - sent0 == ref.counters["sent"]  # a throttled row never travelled
    r = ref.read()
    assert rt.stats()["limit"] == dict(ref.counters, throttled=r["throttled"], oob=r["oob"], actors=n,
                                       rate=rt.limit_rate, burst=rt.limit_burst)
    return ref


def test_runtime_send_limit_against_the_model_cpu():
    rt = runtime(limit_rate=2, limit_burst=3)
    assert rt.limit is False
    plain = rt.send("calculator", echo_batch([5] * 9))
    assert rt._limiter is None and plain[1].tolist() == [STATUS_OK] * 9  # a Send without the option creates nothing
    assert rt.stats()["limit"] == {"sends": 0, "messages": 0, "rejected": 0, "sent": 0, "throttled": 0, "oob": 0,
                                   "actors": 0, "rate": 0, "burst": 0}
    ref = limit_scenario(rt)
    assert ref.read()["oob"] == 0
    rt.send("calculator", echo_batch([1]), limit=False)
    assert rt.stats()["limit"]["sends"] == 4
    rt.close()
    rt = runtime(limit=True, limit_rate=2, limit_burst=3, limit_actors=40)  # the runtime's default, a smaller table
    ref = limit_scenario(rt, send=lambda b: rt.send("calculator", b))
    assert ref.read()["oob"] > 0
    rt.close()


def test_neither_a_breaker_rejection_nor_a_cached_hit_spends_a_token_cpu():
    rt = runtime(breaker_threshold=1, breaker_cooldown=9, limit_rate=1, limit_burst=2)
    both = {"cache": True, "breaker": True, "limit": True}
    b = echo_batch([7, 3], [4, 4])
    assert rt.send("calculator", b, **both)[1].tolist() == [STATUS_OK] * 2  # both stored, a token each
    lim = rt._limiter
    assert word(lim, 7) == (1, 1) and word(lim, 3) == (1, 1) and lim.counters["messages"] == 2
    sent = rt.exchange.counters.sent
    assert rt.send("calculator", b, **both)[1].tolist() == [STATUS_OK] * 2  # two hits: the limiter sees nothing
    assert rt.exchange.counters.sent == sent and lim.counters == {"sends": 1, "messages": 2, "rejected": 0, "sent": 2}
    assert lim.tick == 2 and word(lim, 7) == (1, 1)
    rt.send("calculator", retry_batch([5], 10**9), breaker=True)  # actor 5 opens
    assert rt.stats()["breaker"]["open"] == 1
    val, st = rt.send("calculator", echo_batch([5, 5, 6, 6, 6, 5], [9, 8, 7, 6, 5, 4]), **both)
    # the breaker answers actor 5 before the limiter counts: 6 alone pays, two tokens for three rows
    assert st.tolist() == [STATUS_BREAKER_OPEN] * 2 + [STATUS_OK, STATUS_OK, THR] + [STATUS_BREAKER_OPEN]
    assert val.tolist() == [0, 0, 7, 6, 0, 0]
    assert word(lim, 5) == (0, 0) and word(lim, 6) == (2, 2) and lim.counters["messages"] == 2 + 3
    # the cache stored the two OK rows and not the throttled one: asked again, that row travels
    sent = rt.exchange.counters.sent
    val, st = rt.send("calculator", echo_batch([6, 6, 6], [7, 6, 5]), **both)
    assert st.tolist() == [STATUS_OK] * 3 and rt.exchange.counters.sent - sent == 1 and lim.counters["messages"] == 6
    rt.close()


def test_a_throttled_probe_leaves_its_actor_half_open_cpu():
    rt = runtime(breaker_threshold=1, breaker_cooldown=1, limit_rate=1, limit_burst=1)
    rt.send("calculator", retry_batch([5], 10**9), breaker=True)  # opens until tick 2
    lim_first = echo_batch([5, 5], [1, 2])
    # spend actor 5's token of this limiter tick, then probe: the probe is throttled
    rt.send("calculator", echo_batch([6]), limit=True)
    lim = rt._limiter
    lim.begin()
    lim.admit(echo_batch([5]))
    before = rt._breaker.words().copy()
    val, st = rt.send("calculator", lim_first, breaker=True, limit=True)
    assert st.tolist() == [THR, STATUS_BREAKER_OPEN] and np.array_equal(rt._breaker.words(), before)
    val, st = rt.send("calculator", lim_first, breaker=True, limit=True)  # the next probe has a token: closes
    assert st.tolist() == [STATUS_OK, STATUS_BREAKER_OPEN] and rt.stats()["breaker"]["closes"] == 1
    rt.close()


def test_a_coalesced_follower_inherits_status_8_cpu():
    rt = runtime(limit_rate=1, limit_burst=1)
    b = echo_batch([7, 7, 7, 3, 7], [4, 5, 5, 4, 4])  # leaders: rows 0, 1, 3; actor 7 has one token
    sent = rt.exchange.counters.sent
    val, st = rt.send("calculator", b, coalesce=True, limit=True)
    assert st.tolist() == [STATUS_OK, THR, THR, STATUS_OK, STATUS_OK] and val.tolist() == [4, 0, 0, 4, 4]
    assert rt.exchange.counters.sent - sent == 2 and rt.stats()["limit"]["messages"] == 3  # the limiter saw the leaders
    rt.close()


def test_a_retried_row_costs_one_token_cpu():
    rt = runtime(limit_rate=1, limit_burst=2)
    b = retry_batch([5, 5, 5], 2)  # actor 5 passes from its 2nd call on
    val, st = rt.send("calculator", b, retries=3, limit=True)
    assert st.tolist() == [STATUS_OK, STATUS_OK, THR] and word(rt._limiter, 5) == (1, 2)
    assert int(rt.state[5]) == 3  # row 0 ran twice, row 1 once, row 2 never
    rt.close()


def test_the_ledger_counts_status_8_as_other_and_a_gather_sees_a_non_ok_row_cpu():
    rt = runtime(ledger=True, limit_rate=1, limit_burst=1)
    b = echo_batch([5, 6, 5, 6], [1, 2, 3, 4])
    g = Gather(torch.tensor([0, 0, 1, 1], dtype=torch.int32), 2, "sum")
    val, st = rt.send("calculator", b, limit=True, gather=g)
    assert st.tolist() == [STATUS_OK, STATUS_OK, THR, THR]
    r = rt.stats()["ledger"]
    assert r["calls"] == {"Echo": {"ok": 2, "other": 2}} and r["messages"] == 4 and r["sends"] == 1
    assert g.value.tolist() == [3, 0] and g.n_ok.tolist() == [2, 0] and g.count.tolist() == [2, 2]
    assert g.status.tolist() == [STATUS_OK, THR] and g.bad_row.tolist()[1] == 2
    rt.close()
    rt = runtime()
    with pytest.raises(ValueError, match="ledger"):
        rt.send("calculator", b, limit=True, account=True)
    rt.close()


def test_limited_send_is_refused_under_capture_cpu():
    rt = runtime()
    b = multiply_batch(100, 10, 64)
    rt.send("calculator", b)
    rt.exchange._capturing = True
    with pytest.raises(ValueError, match="limit=True.*captur.*over their quota is read on the host"):
        rt.send("calculator", b, limit=True)
    with pytest.raises(ValueError, match="breaker=True.*captur"):
        rt.send("calculator", b, limit=True, breaker=True)
    rt.send("calculator", b)  # a plain Send is not
    assert rt._limiter is None
    rt.exchange._capturing = False
    rt.close()


def test_limit_reset_and_no_reset_by_the_registry_cpu():
    rt = runtime(limit_rate=1, limit_burst=3)
    rt.limit_reset()  # no limiter yet: nothing
    b = echo_batch([5] * 3)
    assert rt.send("calculator", b, limit=True)[1].tolist() == [STATUS_OK] * 3
    assert rt.send("calculator", b, limit=True)[1].tolist() == [STATUS_OK, THR, THR]
    rt.host("other")  # a registry change resets nothing
    assert rt.send("calculator", b, limit=True)[1].tolist() == [STATUS_OK, THR, THR]
    rt.limit_reset()
    assert not rt._limiter.words()[:64].any() and rt._limiter.tick == 4  # the tick goes on
    assert rt.send("calculator", b, limit=True)[1].tolist() == [STATUS_OK] * 3
    assert rt.stats()["limit"]["throttled"] == 4
    rt.close()


def test_bad_runtime_settings_are_refused():
    for kw in ({"limit_rate": 0}, {"limit_rate": 2**32}, {"limit_burst": 0}, {"limit_burst": 2**32}, {"limit_actors": -1}):
        with pytest.raises(ValueError):
            runtime(**kw)


# ---------------------------------------------------------------- the public API and the config keys
def test_client_send_limit_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, srv, c = join_world1(C, tmp_path, ports, form_group=True, grace_s=0.3, limit_rate=2, limit_burst=3)
    try:
        rt = c.runtime
        assert rt.limit is False and (rt.limit_rate, rt.limit_burst, rt.limit_actors) == (2, 3, 0)
        client = c.NewClient("w1", C.ConnConfig())
        client.Send(multiply_batch(300, 20, rt.total_actors))
        assert rt._limiter is None and c.Stats()["runtime"]["limit"]["sends"] == 0
        limit_scenario(rt, send=lambda b: client.Send(b, limit=True))
        assert c.Stats()["runtime"]["limit"]["sends"] == 4
        client.Send(echo_batch([1]), limit=False)
        assert c.Stats()["runtime"]["limit"]["sends"] == 4
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_gpu_limit_config_default_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, srv, c = join_world1(C, tmp_path, ports, limit=True, limit_burst=2, limit_actors=32)
    try:
        assert c.runtime.limit is True
        client = c.NewClient("w1", C.ConnConfig())
        b = echo_batch([5, 5, 5, 40, 40, 40])
        assert client.Send(b)[1].tolist() == [0, 0, THR, 0, 0, 0]  # no argument: gpu.limit; id 40 is past gpu.limit_actors
        assert client.Send(b, limit=False)[1].tolist() == [0] * 6
        n = c.Stats()["runtime"]["limit"]
        assert (n["sends"], n["throttled"], n["oob"], n["actors"], n["rate"], n["burst"]) == (1, 1, 3, 32, 1, 2)
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_config_gpu_limit_keys(tmp_path):
    (tmp_path / "m.yml").write_text("name: x\n")
    p = tmp_path / "a.yml"
    p.write_text("service_name: calc\netcd_config_file: m.yml\n"
                 "gpu: {limit: true, limit_rate: 4294967295, limit_burst: 7, limit_actors: 268435456}\n")
    g = C.ConfigFromFile(str(p)).gpu
    assert g.limit is True and (g.limit_rate, g.limit_burst, g.limit_actors) == (2**32 - 1, 7, 2**28)
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu:\n  actors: 64\n")
    g = C.ConfigFromFile(str(p)).gpu
    assert g.limit is False and (g.limit_rate, g.limit_burst, g.limit_actors) == (1, 1, 0)
    d = C.Config().gpu
    assert d.limit is False and (d.limit_rate, d.limit_burst, d.limit_actors) == (1, 1, 0)
    for bad in ("limit: 3", "limit_rate: 0", "limit_rate: -1", "limit_rate: true", "limit_rate: 4294967296",
                "limit_burst: 0", "limit_burst: 4294967296", "limit_burst: many", "limit_actors: -1",
                "limit_actors: 268435457"):
        p.write_text(f"service_name: calc\netcd_config_file: m.yml\ngpu:\n  {bad}\n")
        with pytest.raises(C.ConfigError):
            C.ConfigFromFile(str(p))
