"""The timer queue on CPU tensors (``ops/timers.py``): the numpy model (``TimerRef``) against
an independent oracle -- a Python list of ``(due, call, row)`` that is sorted and popped per
tick -- over random sequences of Schedules and Ticks (shared with the GPU tests), one record
and one descriptor written out by hand, then the runtime's ``schedule`` / ``tick`` /
``timers``, the public API and the ``gpu.timer*`` config keys.  All comparisons are exact
integer equality."""
import numpy as np
import pytest
import torch

from ptype_amd import cluster as C
from ptype_amd.ops import timers as TM
from ptype_amd.ops.batch import MsgBatch
from ptype_amd.ops.dead_letters import fnv1a64
from ptype_amd.ops.records import (METHOD_COUNTER_ADD, METHOD_ECHO, METHOD_RETRY_TEST, STATUS_FAILED, STATUS_NO_ACTOR,
                                   STATUS_OK)

from test_coalesce import runtime
from test_send_retries import join_world1

U64 = (1 << 64) - 1


# ---------------------------------------------------------------- the oracle
class Oracle:
    """One pending list of ``(due, call, row, ticket)``; a tick sorts it and pops what is due.
    The ring is written one record at a time; a run is a dict, the live runs a list."""

    def __init__(self, entries, horizon, runs):
        self.E, self.H, self.R = entries, horizon, runs
        self.ring = [[0] * 8 for _ in range(entries)]
        self.pending, self.live = [], []
        self.now = self.head = self.calls = self.refused = self.delivered = 0

    @property
    def tail(self):
        return self.live[0]["base"] if self.live else self.head

    def schedule(self, batch, delay, tag=0):
        M = batch.M
        dl = delay.tolist() if isinstance(delay, torch.Tensor) else [int(delay)] * M
        rows = sorted((d, i) for i, d in enumerate(dl) if 1 <= d <= self.H)
        K = len(rows)
        if self.head + K - self.tail > self.E or (K and len(self.live) == self.R):
            raise TM.TimerQueueFull("oracle")
        col = (lambda t, i: 0 if t is None else int(t[i]) & U64)
        for k, (d, i) in enumerate(rows):
            t = self.head + k
            m = batch.method if isinstance(batch.method, int) else int(batch.method[i])
            self.ring[t % self.E] = [t + 1, self.now + d, i | d << 32, (int(batch.actor[i]) & 0xFFFFFFFF) | (m & 0xFFFF) << 32,
                                     col(batch.a0, i), col(batch.a1, i), col(batch.a2, i), tag & U64]
            self.pending.append((self.now + d, self.calls, i, t))
        if K:
            self.live.append({"q": self.calls, "t0": self.now, "base": self.head, "n": K, "max": rows[-1][0],
                              "delays": [d for d, _ in rows]})
            self.calls += 1
            self.head += K
        self.refused += M - K
        return K, M - K

    def tick(self):
        self.now += 1
        self.pending.sort()
        due = [p for p in self.pending if p[0] == self.now]
        self.pending = self.pending[len(due):]
        assert all(p[0] > self.now for p in self.pending)
        self.delivered += len(due)
        while self.live and self.now >= self.live[0]["t0"] + self.live[0]["max"]:
            self.live.pop(0)
        return [self.ring[t % self.E] for _, _, _, t in due], [t for _, _, _, t in due]


def random_call(M, seed, horizon, a1=True, a2=True, method="col", delays="mixed", device="cpu"):
    """A batch of M rows and a delay column: ``mixed`` draws from the whole horizon and the
    refused values ``0, -1, H + 1, 2^31 - 1``, ``valid`` from ``[1, H]`` only, ``short`` from
    ``[1, 3]``."""
    g = torch.Generator().manual_seed(seed)
    big = (lambda: torch.randint(-2**62, 2**62, (M,), generator=g))
    m = torch.randint(-2**15, 2**15, (M,), generator=g).to(torch.int16) if method == "col" else method
    b = MsgBatch(torch.randint(-2**31, 2**31, (M,), generator=g).to(torch.int32), big(), big() if a1 else None,
                 big() if a2 else None, m)
    if delays == "short":
        d = torch.randint(1, 4, (M,), generator=g)
    else:
        d = torch.randint(1, horizon + 1, (M,), generator=g)
        if delays == "mixed":
            bad = torch.tensor([0, -1, horizon + 1, 2**31 - 1])[torch.randint(0, 4, (M,), generator=g)]
            d = torch.where(torch.rand(M, generator=g) < 0.2, bad, d)
    to = (lambda t: t.to(device) if isinstance(t, torch.Tensor) else t)
    return MsgBatch(to(b.actor), to(b.a0), to(b.a1), to(b.a2), to(b.method)), d.to(torch.int32).to(device)


def snapshot(ref):
    return ref.ring.copy(), ref.runs.copy(), ref.ctrl.copy()


def unchanged(ref, snap):
    return all(np.array_equal(a, b) for a, b in zip(snapshot(ref), snap))


def check_against_oracle(ref, o):
    assert ref.ring.tolist() == o.ring
    c = [int(x) for x in ref.ctrl]
    assert c == [o.now, o.head, o.tail, o.calls, o.live[0]["q"] if o.live else o.calls, o.refused, o.delivered, 0]
    for run in o.live:
        slot = run["q"] & (o.R - 1)
        assert [int(x) for x in ref.runs[slot, :5]] == [run["t0"], run["base"], run["n"], run["max"], run["q"] + 1]
        assert ref.off(slot).tolist() == [sum(1 for d in run["delays"] if d < j) for j in range(o.H + 2)]


def tick_both(ref, o):
    r = ref.tick()
    recs, tickets = o.tick()
    assert r["n"] == len(recs) and r["torn"] == 0 and r["ticket"].tolist() == tickets
    s64 = (lambda x: x - (1 << 64) if x >> 63 else x)
    assert r["row"].tolist() == [w[2] & 0xFFFFFFFF for w in recs]
    assert r["delay"].tolist() == [w[2] >> 32 for w in recs]
    assert r["t0"].tolist() == [w[1] - (w[2] >> 32) for w in recs]
    assert (r["actor"].astype(np.int64) & 0xFFFFFFFF).tolist() == [w[3] & 0xFFFFFFFF for w in recs]
    assert (r["method"].astype(np.int64) & 0xFFFF).tolist() == [w[3] >> 32 for w in recs]
    for k, w in (("a0", 4), ("a1", 5), ("a2", 6), ("tag", 7)):
        assert r[k].tolist() == [s64(x[w]) for x in recs]
    check_against_oracle(ref, o)
    return r["n"]


# ---------------------------------------------------------------- the model against the oracle
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_model_equals_the_oracle_over_random_schedules_and_ticks(seed):
    E, H, R = 64, 16, 4
    ref, o = TM.TimerRef(E, H, R), Oracle(E, H, R)
    rng = np.random.default_rng(seed)
    full = {"ring": 0, "runs": 0}
    for step in range(400):
        if rng.random() < 0.45:
            M = int(rng.choice([0, 1, 3, 9, 20, 40]))
            kind = ["mixed", "short", "valid"][int(rng.integers(3))]
            b, d = random_call(M, 1000 * seed + step, H, a1=bool(step & 1), a2=bool(step & 2),
                               method="col" if step & 4 else int(rng.integers(0, 1 << 16)), delays=kind)
            delay = d if step % 5 else int(rng.choice([0, -1, 1, 2, H, H + 1, 2**31 - 1]))
            snap = snapshot(ref)
            try:
                want = o.schedule(b, delay, tag=step)
            except TM.TimerQueueFull:
                K = int(((d >= 1) & (d <= H)).sum()) if isinstance(delay, torch.Tensor) else M
                full["ring" if o.head + K - o.tail > E else "runs"] += 1
                with pytest.raises(TM.TimerQueueFull):
                    ref.schedule(b, delay, tag=step)
                assert unchanged(ref, snap)
                continue
            got = ref.schedule(b, delay, tag=step)
            assert (got.n, got.refused, got.first_ticket, got.now) == (want[0], want[1], o.head - want[0], o.now)
            if want[0] == 0:  # K = 0 files no run: only `refused` moved
                snap[2][TM.C_REFUSED] += np.uint64(want[1])
                assert unchanged(ref, snap)
            check_against_oracle(ref, o)
        else:
            for _ in range(int(rng.integers(1, 4))):
                tick_both(ref, o)
    assert o.head > 4 * E and full["ring"] and full["runs"] and o.refused and ref.full == full["ring"] + full["runs"]
    for _ in range(H):
        tick_both(ref, o)
    assert ref.read()["live"] == 0 and ref.read()["runs"] == 0 and ref.read()["tail"] == o.head


def test_a_long_delay_run_holds_the_tail_and_releases_it():
    E, H, R = 64, 16, 4
    ref, o = TM.TimerRef(E, H, R), Oracle(E, H, R)
    long_b, _ = random_call(8, 1, H)
    for q in (ref, o):
        q.schedule(long_b, H)  # tickets 0..7, due at tick 16
    for k in range(3):  # three short runs behind it: finished after one tick each
        b, _ = random_call(16, 10 + k, H)
        for q in (ref, o):
            q.schedule(b, 1)
        assert tick_both(ref, o) == 16
        assert ref.read()["tail"] == 0 and ref.read()["runs"] == k + 2  # the finished runs stay behind the tail
    b, _ = random_call(16, 20, H)
    snap = snapshot(ref)
    with pytest.raises(TM.TimerQueueFull):  # 56 held + 16 > 64, though only 8 records are live
        ref.schedule(b, 1)
    assert unchanged(ref, snap) and ref.read()["live"] == 8 and ref.read()["full"] == 1
    for _ in range(H - 3):
        tick_both(ref, o)
    assert ref.read() == dict(ref.read(), now=16, tail=56, head=56, live=0, runs=0, delivered=56)
    ref.schedule(b, 1)
    o.schedule(b, 1)
    check_against_oracle(ref, o)


def test_runs_behind_a_live_tail_run_are_retired_with_it():
    ref, o = TM.TimerRef(64, 16, 4), Oracle(64, 16, 4)
    b, _ = random_call(4, 3, 16)
    for q in (ref, o):
        q.schedule(b, 3)
        q.schedule(b, 1)
        q.schedule(b, 2)
    assert [tick_both(ref, o) for _ in range(2)] == [4, 4] and ref.read()["runs"] == 3
    b2, _ = random_call(1, 4, 16)
    for q in (ref, o):
        q.schedule(b2, 1)
    snap = snapshot(ref)
    with pytest.raises(TM.TimerQueueFull):  # four descriptors in use, two of them finished
        ref.schedule(b2, 1)
    assert unchanged(ref, snap)
    ref.schedule(b2, 0)  # no accepted row: no descriptor needed
    o.schedule(b2, 0)
    assert tick_both(ref, o) == 5 and ref.read()["runs"] == 0 and ref.read()["tail"] == 13


def test_one_record_and_one_descriptor_by_hand():
    H = 16
    ref = TM.TimerRef(64, H, 4)
    ref.tick()
    ref.tick()  # now = 2
    b = MsgBatch(torch.tensor([7, -2, 9], dtype=torch.int32), torch.tensor([11, -1, 13]), None, torch.tensor([5, 6, 7]),
                 torch.tensor([3, -1, 4], dtype=torch.int16))
    s = ref.schedule(b, torch.tensor([5, 2, 17], dtype=torch.int32), tag=-3)
    assert (s.n, s.refused, s.first_ticket, s.now) == (2, 1, 0, 2)
    # ticket 0 is row 1 (delay 2), ticket 1 is row 0 (delay 5)
    assert [hex(int(x)) for x in ref.ring[0]] == [hex(x) for x in (
        1, 4, 1 | 2 << 32, 0xFFFFFFFE | 0xFFFF << 32, U64, 0, 6, U64 - 2)]
    assert [int(x) for x in ref.ring[1]] == [2, 7, 0 | 5 << 32, 7 | 3 << 32, 11, 0, 5, U64 - 2]
    assert not ref.ring[2:].any()
    assert TM.desc_words(H) == 8 + 16 and ref.runs.shape == (4, 24)
    assert [int(x) for x in ref.runs[0, :8]] == [2, 0, 2, 5, 1, 0, 0, 0]
    # off[d]: records with a delay below d, d = 0 .. H + 1, then the padding
    off = [0, 0, 0, 1, 1, 1] + [2] * 12
    assert ref.runs[0, 8:].view(np.uint32).tolist() == off + [0] * (32 - len(off))
    assert ref.runs[0, 8 + 1] == 1 << 32 and not ref.runs[1:].any()
    assert [int(x) for x in ref.ctrl] == [2, 2, 0, 1, 0, 1, 0, 0]
    assert [int(x) for x in ref.scratch[:6]] == [2, 1, 5, 0, 0, 2]
    assert TM.desc_words(256) == 8 + 136 and TM.desc_words(1024) == 8 + 520


def test_settings_and_arguments_are_checked():
    for f, bad in ((TM.check_entries, (0, 32, 100, 2**25)), (TM.check_horizon, (0, 8, 100, 2048)),
                   (TM.check_runs, (0, 2, 100, 8192))):
        for v in bad:
            with pytest.raises(ValueError, match="power of two"):
                f(v)
    assert (TM.check_entries(2**24), TM.check_horizon(1024), TM.check_runs(4096)) == (2**24, 1024, 4096)
    for kw in ({"timer_entries": 100}, {"timer_horizon": 8}, {"timer_runs": 3}):
        with pytest.raises(ValueError):
            runtime(**kw)
    ref = TM.TimerRef(64, 16, 4)
    b, d = random_call(4, 0, 16)
    for bad in (d.to(torch.int64), d[:3], 1.5, True, None):
        with pytest.raises(TypeError):
            ref.schedule(b, bad)


# ---------------------------------------------------------------- the runtime
def echo_batch(actors, values, dev="cpu"):
    return MsgBatch(torch.tensor(actors, dtype=torch.int32).to(dev), torch.tensor(values).to(dev), None, None, METHOD_ECHO)


def schedule_and_tick_scenario(rt, dev="cpu", tick=None, schedule=None, tag=0):
    """Two Schedules with delay columns, ticks in between; what is due comes back in ticket
    order with its call, through ``send``."""
    tick = tick or (lambda **kw: rt.tick("calculator", **kw))
    schedule = schedule or rt.schedule
    b1 = echo_batch([1, 2, 3, 900, 5], [10, 20, 30, 40, 50], dev)
    s1 = schedule(b1, torch.tensor([2, 1, 2, 1, 99999], dtype=torch.int32).to(dev))
    assert (s1.n, s1.refused, s1.first_ticket, s1.now) == (4, 1, 0, 0)
    t = tick()
    assert t.n == 2 and t.due.row.tolist() == [1, 3] and t.due.actor.tolist() == [2, 900] and t.due.torn == 0
    assert t.value.tolist() == [20, 0] and t.status.tolist() == [STATUS_OK, STATUS_NO_ACTOR]
    assert t.due.tag.tolist() == [tag - (1 << 64) if tag >> 63 else tag] * 2 and t.due.t0.tolist() == [0, 0]
    s2 = schedule(echo_batch([7, 8], [70, 80], dev), 1)
    assert (s2.n, s2.refused, s2.first_ticket, s2.now) == (2, 0, 4, 1)
    t = tick()
    assert t.due.ticket.tolist() == [2, 3, 4, 5] and t.due.a0.tolist() == [10, 30, 70, 80]
    assert t.due.delay.tolist() == [2, 2, 1, 1] and t.due.t0.tolist() == [0, 0, 1, 1]
    assert t.due.method.tolist() == [METHOD_ECHO] * 4 and t.value.tolist() == [10, 30, 70, 80]
    t = tick()
    assert t.n == 0 and t.value.numel() == 0 and t.status.dtype == torch.int32
    got = rt.timers()
    assert got == dict(got, now=3, head=6, tail=6, live=0, runs=0, refused=1, delivered=6, full=0, torn=0)
    assert rt.stats()["timers"] == got


def retries_and_dead_letters_scenario(rt, dev="cpu"):
    """``rt``: ``timers=True, dead_letters=True``.  A tick's Send takes every keyword: the rows
    that still failed after the retries are letters."""
    b = MsgBatch(torch.arange(6, dtype=torch.int32).to(dev), torch.tensor([1, 2, 3, 4, 5, 3]).to(dev), None, None,
                 METHOD_RETRY_TEST)
    rt.schedule(b, 2, tag=5)
    assert rt.tick("calculator", retries=2, dead_letter=True).n == 0
    t = rt.tick("calculator", retries=2, dead_letter=True, dead_letter_tag=9)
    assert t.status.tolist() == [0, 0, 0, STATUS_FAILED, STATUS_FAILED, 0] and t.due.tag.tolist() == [5] * 6
    lt = rt.dead_letters(drain=True)
    assert lt.row.tolist() == [3, 4] and lt.actor.tolist() == [3, 4] and lt.tag.tolist() == [9, 9]


def backoff_scenario(rt, dev="cpu"):
    """Redrive with back-off: the letters are scheduled ``min(2 ** attempts, H)`` ticks ahead
    and re-sent by the tick, dead-lettered again with their attempts."""
    H = rt.timer_horizon
    b = MsgBatch(torch.tensor([1, 2, 3], dtype=torch.int32).to(dev), torch.tensor([1, 3, 9]).to(dev), None, None,
                 METHOD_RETRY_TEST)
    st = rt.send("calculator", b, dead_letter=True)[1]
    assert st.tolist() == [0, STATUS_FAILED, STATUS_FAILED]
    attempts_seen, sent_at = [], []
    for _ in range(3):
        letters = rt.dead_letters(drain=True)
        if not letters.n:
            break
        attempts_seen.append(letters.attempts.tolist())
        delay = torch.clamp(2 ** letters.attempts, max=H).to(torch.int32)
        assert rt.schedule(letters.batch(), delay).n == letters.n
        for _ in range(int(delay.max())):
            t = rt.tick("calculator", dead_letter=True)
            if t.n:
                sent_at.append((rt.timers()["now"], t.due.actor.tolist(), t.status.tolist()))
    # actor 2 passes at its third call; actor 3 (a0 = 9) is still failing
    assert attempts_seen == [[1, 1], [1, 1], [1]]
    assert sent_at == [(2, [2, 3], [STATUS_FAILED] * 2), (4, [2, 3], [0, STATUS_FAILED]), (6, [3], [STATUS_FAILED])]
    assert rt.dead_letters().n == 1 and rt.state[:4].tolist() == [0, 1, 3, 4]


def bad_keywords_scenario(rt, dev="cpu"):
    """``rt``: ``timers=True``, no ledger, no dead-letter queue.  A refused tick leaves the
    clock and the queue as they were."""
    from ptype_amd.ops.gather import Gather

    rt.schedule(echo_batch([1, 2, 3], [4, 5, 6], dev), 1)
    before = rt.timers()
    bad = [({"no_such_keyword": 1}, TypeError, "no_such_keyword"), ({"account": True}, ValueError, "ledger"),
           ({"dead_letter": True}, ValueError, "dead-letter queue"), ({"dead_letter_attempts": None}, ValueError, "attempts"),
           ({"gather": Gather(torch.zeros(2, dtype=torch.int32).to(dev), 1, "sum")}, ValueError, "."),
           ({"retries": 2, "resend_overflow": False}, ValueError, "resend_overflow"),
           ({"retries": 1, "retry_on": (STATUS_OK,)}, ValueError, "retry_on"), ({"retries": -1}, ValueError, "retries"),
           ({"ticks": -1}, ValueError, "ticks")]
    for kw, err, match in bad:
        with pytest.raises(err, match=match):
            rt.tick("calculator", **kw)
    with pytest.raises(ValueError, match="hosts"):
        rt.tick("another-service")
    assert rt.timers() == before and before["now"] == 0 and before["live"] == 3
    g = Gather(torch.zeros(3, dtype=torch.int32).to(dev), 1, "sum")  # the size of what is due: accepted
    assert rt.tick("calculator", gather=g).n == 3 and int(g.count[0]) == 3 and int(g.value[0]) == 15


def test_schedule_and_tick_cpu():
    schedule_and_tick_scenario(runtime(timers=True, timer_entries=64, timer_horizon=16, timer_runs=4))


def test_tick_with_retries_and_dead_letters_cpu():
    retries_and_dead_letters_scenario(runtime(timers=True, dead_letters=True))


def test_redrive_with_back_off_end_to_end_cpu():
    backoff_scenario(runtime(timers=True, timer_horizon=16, dead_letters=True))


def test_a_refused_tick_leaves_the_clock_and_the_queue_as_they_were_cpu():
    bad_keywords_scenario(runtime(timers=True))


def test_ticks_is_a_loop_and_a_large_tick_is_sent_in_slices_cpu():
    rt = runtime(timers=True, max_batch=4)
    cap = rt.exchange.max_chunk * rt.exchange.chunks
    M = 2 * cap + 3
    b = MsgBatch((torch.arange(M, dtype=torch.int32) % 64), torch.arange(M) + 100, None, None, METHOD_COUNTER_ADD)
    rt.schedule(b, 2)
    sizes, send = [], rt.send
    rt.send = lambda service, batch, **kw: (sizes.append(batch.M), send(service, batch, **kw))[1]
    out = rt.tick("calculator", ticks=2)
    assert [t.n for t in out] == [0, M] and sizes == [cap, cap, 3]
    assert out[1].due.row.tolist() == list(range(M)) and out[1].status.tolist() == [0] * M
    state = [0] * 64
    want = []
    for i in range(M):  # Counter.Add replies the running sum: the slices went in ticket order
        state[i % 64] += 100 + i
        want.append(state[i % 64])
    assert out[1].value.tolist() == want and rt.tick("calculator", ticks=0) == []


def test_no_queue_without_the_setting_and_refusal_under_capture_cpu():
    rt = runtime()
    b = echo_batch([1], [2])
    assert rt._timers is None and rt.stats()["timers"]["now"] == 0 and rt.stats()["timers"]["entries"] == 0
    for call in (lambda: rt.schedule(b, 1), lambda: rt.tick("calculator"), rt.timers):
        with pytest.raises(ValueError, match="timer queue"):
            call()
    rt = runtime(timers=True)
    rt.schedule(b, 1)
    before = rt.timers()
    rt.exchange._capturing = True  # as inside ActorExchange.capture
    try:
        with pytest.raises(ValueError, match="captur"):
            rt.schedule(b, 1)
        with pytest.raises(ValueError, match="captur"):
            rt.tick("calculator")
    finally:
        rt.exchange._capturing = False
    assert rt.timers() == before and rt.tick("calculator").value.tolist() == [2]


# ---------------------------------------------------------------- the public API and the config keys
def test_client_schedule_tick_and_timers_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, srv, c = join_world1(C, tmp_path, ports, form_group=True, grace_s=0.3, timers=True, timer_entries=128,
                              timer_horizon=32, timer_runs=8)
    try:
        rt = c.runtime
        assert (rt._timers.entries, rt._timers.horizon, rt._timers.n_runs) == (128, 32, 8)
        client = c.NewClient("w1", C.ConnConfig())
        schedule_and_tick_scenario(rt, tick=client.Tick, schedule=client.Schedule, tag=fnv1a64("w1"))
        assert client.Timers() == c.Stats()["runtime"]["timers"] and client.Timers()["horizon"] == 32
        assert client.Schedule(echo_batch([1], [2]), 33, tag=4).refused == 1
        assert [t.n for t in client.Tick(ticks=3)] == [0, 0, 0] and client.Timers()["now"] == 6
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_no_timer_queue_without_the_key_through_join_cpu(tmp_path, ports, monkeypatch):
    monkeypatch.setenv("PTYPE_ADVERTISE_ADDR", "127.0.0.1")
    cfg, srv, c = join_world1(C, tmp_path, ports)
    try:
        client = c.NewClient("w1", C.ConnConfig())
        assert c.runtime._timers is None and c.Stats()["runtime"]["timers"]["head"] == 0
        for call in (lambda: client.Schedule(echo_batch([1], [2]), 1), client.Tick, client.Timers):
            with pytest.raises(ValueError, match="timer queue"):
                call()
        client.Close()
    finally:
        c.Close()
        srv.Close()


def test_config_gpu_timer_keys(tmp_path):
    (tmp_path / "m.yml").write_text("name: x\n")
    p = tmp_path / "a.yml"
    p.write_text("service_name: calc\netcd_config_file: m.yml\n"
                 "gpu: {timers: true, timer_entries: 16777216, timer_horizon: 1024, timer_runs: 4096}\n")
    g = C.ConfigFromFile(str(p)).gpu
    assert g.timers is True and (g.timer_entries, g.timer_horizon, g.timer_runs) == (2**24, 1024, 4096)
    p.write_text("service_name: calc\netcd_config_file: m.yml\ngpu: {timer_entries: 64, timer_horizon: 16, timer_runs: 4}\n")
    g = C.ConfigFromFile(str(p)).gpu
    assert g.timers is False and (g.timer_entries, g.timer_horizon, g.timer_runs) == (64, 16, 4)
    d = C.Config().gpu
    assert d.timers is False and (d.timer_entries, d.timer_horizon, d.timer_runs) == (1 << 20, 256, 256)
    for bad in ("timers: 3", "timer_entries: 0", "timer_entries: 32", "timer_entries: 100", "timer_entries: 33554432",
                "timer_entries: many", "timer_horizon: 8", "timer_horizon: 100", "timer_horizon: 2048",
                "timer_horizon: -16", "timer_runs: 2", "timer_runs: 100", "timer_runs: 8192", "timer_runs: true"):
        p.write_text(f"service_name: calc\netcd_config_file: m.yml\ngpu:\n  {bad}\n")
        with pytest.raises(C.ConfigError):
            C.ConfigFromFile(str(p))
