"""The Forward / outbox contract (tests/_outbox_spec.py) against hand-written rows, and
the CPU reference (``_handler_ref`` + ``DeviceOutbox.emit_cpu``, the CPU ``ActorExchange``)
against the contract over a hostile corpus.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from _outbox_spec import (FAILED, INT64_MAX, INT64_MIN, METHOD_CALC_MULTIPLY, METHOD_COUNTER_ADD, METHOD_ECHO,
                          METHOD_FORWARD, METHOD_SEQ_FOLD, NO_ACTOR, OK, OVERFLOW, corpus_rows, forward_corpus,
                          forward_spec, simulate_pump, wants_emit)
from ptype_amd.ops import batch as B
from ptype_amd.ops import records as R
from ptype_amd.ops.outbox import DeviceOutbox
from ptype_amd.ops.table import RegistryTable, actor_keys
from ptype_amd.parallel.exchange import ActorExchange

FWD = METHOD_FORWARD
RING = 7 | (10 << 32)  # stride 7 over n = 10


def test_spec_constants_are_the_projects():
    assert (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_COUNTER_ADD, METHOD_FORWARD, METHOD_SEQ_FOLD) == (
        R.METHOD_CALC_MULTIPLY, R.METHOD_ECHO, R.METHOD_COUNTER_ADD, R.METHOD_FORWARD, R.METHOD_SEQ_FOLD)
    assert (OK, FAILED, NO_ACTOR, OVERFLOW) == (R.STATUS_OK, R.STATUS_FAILED, R.STATUS_NO_ACTOR, R.STATUS_OVERFLOW)


# (a0, a1, a2) -> the emitted record, typed out
HAND = [
    ((4, 1, RING), (4, FWD, 1, 0, RING)),                                        # the ordinary hop
    ((4, INT64_MAX, RING), (4, FWD, 1, INT64_MAX - 1, RING)),
    ((4, 2, 0), (4, FWD, 4, 1, 0)),                                              # a2 = 0: next = a0
    ((4, 2, 5), (4, FWD, 4, 1, 5)),                                              # stride only (n = 0)
    ((4, 2, 3 | (1 << 32)), (4, FWD, 0, 1, 3 | (1 << 32))),                      # n = 1
    ((-3, 2, 1 | (10 << 32)), (0xFFFFFFFF, FWD, 4, 1, 1 | (10 << 32))),          # u64: (2^64 - 3 + 1) % 10 = 4
    ((-1, 2, 1 | (10 << 32)), (0xFFFFFFFF, FWD, 0, 1, 1 | (10 << 32))),          # a0 + stride wraps 2^64
    ((2**32 - 2, 1, 0), (2**32 - 2, FWD, 2**32 - 2, 0, 0)),                      # the last id
    ((2**32 - 1, 1, 0), (0xFFFFFFFF, FWD, 2**32 - 1, 0, 0)),                     # the field that names no actor
    ((2**32 + 5, 1, 0), (0xFFFFFFFF, FWD, 2**32 + 5, 0, 0)),                     # not actor 5
    ((INT64_MIN, 1, 5 | (7 << 32)), (0xFFFFFFFF, FWD, (2**63 + 5) % 7, 0, 5 | (7 << 32))),
    ((INT64_MAX, 1, -1), (0xFFFFFFFF, FWD, (2**63 - 1 + 2**32 - 1) % (2**32 - 1), 0, -1)),  # stride = n = 2^32 - 1
    ((6, 1, -(1 << 63) | (9 << 32) | 4), (6, FWD, 10, 0, -(1 << 63) | (9 << 32) | 4)),  # top bit: n = 2^31 + 9
]


def test_spec_on_hand_written_rows():
    n = len(HAND)
    a0, a1, a2 = ([h[0][k] for h in HAND] for k in range(3))
    # + rows that do not emit: a1 = 0, -1, INT64_MIN; an unknown actor; a mailbox past the state
    a0 += [1, 1, 1, 1, 1]
    a1 += [0, -1, INT64_MIN, 5, 5]
    a2 += [RING] * 5
    resolve = [0] * n + [1, 1, 1, None, 9]
    sp = forward_spec((None, FWD, a0, a1, a2), resolve, 4, [100, 200, 0, 0], True, ordered=True)
    assert sp.emitted == [h[1] for h in HAND] and sp.E == n and sp.emitters == list(range(n))
    assert sp.status == [OK] * (n + 3) + [NO_ACTOR, NO_ACTOR]
    assert sp.value[:n] == list(range(101, 101 + n)) and sp.value[n:n + 3] == [201, 202, 203]
    assert sp.visits == [n, 3, 0, 0] and sp.state_after == [100 + n, 203, 0, 0]
    assert sp.outbox_after(n) == {"count": (n, 0), "filled": n}
    assert sp.outbox_after(5) == {"count": (n, n - 5), "filled": 5}
    sp.check_outbox(n, (n, 0), list(reversed(sp.emitted)))
    sp.check_outbox(5, (n, n - 5), sp.emitted[3:8])
    with pytest.raises(AssertionError):
        sp.check_outbox(n, (n, 0), sp.emitted[:-1] + [(4, FWD, 1, 0, 0)])
    with pytest.raises(AssertionError):
        sp.check_outbox(5, (n, n - 5), [sp.emitted[0]] * 5)

    # no outbox: the senders answer FAILED with the visit counted; unordered replies per mailbox
    un = forward_spec((None, FWD, a0, a1, a2), resolve, 4, [100, 200, 0, 0], False)
    assert un.status == [FAILED] * n + [OK] * 3 + [NO_ACTOR, NO_ACTOR] and un.E == 0
    assert un.state_after == sp.state_after and un.value_sets == {1: ([n, n + 1, n + 2], [201, 202, 203])}
    # rows that did not run
    ran = [True] * (n + 5)
    ran[0] = ran[n] = False
    part = forward_spec((None, FWD, a0, a1, a2), resolve, 4, [100, 200, 0, 0], True, ran=ran)
    assert part.status[0] == OVERFLOW and part.status[n] == OVERFLOW and part.E == n - 1
    assert part.state_after == [100 + n - 1, 202, 0, 0]
    # the other methods: closed forms, never an emit
    mix = forward_spec((None, [METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_COUNTER_ADD, METHOD_SEQ_FOLD, FWD],
                        [3, -9, 5, 11, 2], [1 << 62, 7, 7, 7, 0], None), [9, 9, 1, 0, 0], 4, [2, 50, 0, 0], True,
                       ordered=True)
    assert mix.status == [OK] * 5 and mix.E == 0
    assert mix.value == [-(1 << 62), -9, 55, 2, 2 * R.FOLD_MUL + 11 + 1]


def test_corpus_holds_every_edge():
    c = forward_corpus(5000, 400, 350, 1, method_column=True)
    a0, a1, a2 = c["a0"], c["a1"], c["a2"]
    for v in (0, 399, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 5, -1, -3, INT64_MIN, INT64_MAX):
        assert (a0 == v).any(), v
    for v in (INT64_MIN, -1, 0, 1, 2, INT64_MAX):
        assert (a1 == v).any(), v
    assert (a2 == 0).any() and (a2 < 0).any() and ((a2 >> 32) == 1).any() and (((a2 >> 32) == 0) & (a2 > 0)).any()
    assert (c["actor"] >= 400).any() and any(m is not None and m >= 350 for m in c["resolve"])
    assert np.bincount(c["actor"]).max() >= 200
    assert set(np.unique(c["method"])) == {METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_COUNTER_ADD, FWD}
    w = wants_emit(5000).reshape(-1)[:4992].reshape(-1, 64)
    kinds = {tuple(np.nonzero(g)[0]) for g in w}
    assert {tuple(range(64)), (), (0,), (63,), tuple(range(0, 64, 2))} <= kinds
    assert not wants_emit(5000)[2048:3072].any()
    blk = wants_emit(5000)[768:1024].reshape(4, 64).all(axis=1)
    assert blk.tolist() == [False, True, False, False]
    sp = forward_spec(corpus_rows(c), c["resolve"], 350, [0] * 350, True)
    assert 500 < sp.E < 4000 and forward_corpus(5000, 400, 350, 1, two_args=True)["a2"] is None


def _t(x, dtype=torch.int64):
    return None if x is None else torch.from_numpy(np.asarray(x)).to(dtype)


def _cpu_send(c, state, outbox):
    """(value, status) of the corpus through the CPU reference handlers, as send_ref drives them."""
    M = len(c["a0"])
    mbox = torch.tensor([-1 if m is None else m for m in c["resolve"]])
    idx = torch.nonzero(mbox >= 0).flatten()
    method = torch.full((M,), int(c["method"])) if isinstance(c["method"], int) else _t(c["method"])
    a2 = torch.zeros(M, dtype=torch.int64) if c["a2"] is None else _t(c["a2"])
    val = torch.zeros(M, dtype=torch.int64)
    st = torch.full((M,), NO_ACTOR, dtype=torch.int64)
    v, s = B._handler_ref(method[idx], mbox[idx], _t(c["a0"])[idx], _t(c["a1"])[idx], a2[idx], state, outbox)
    val[idx], st[idx] = v, s
    return val, st


def _records(outbox, n):
    b = outbox.bank
    return list(zip((b["actor"][:n].to(torch.int64) & 0xFFFFFFFF).tolist(), b["method"][:n].tolist(),
                    b["a0"][:n].tolist(), b["a1"][:n].tolist(), b["a2"][:n].tolist()))


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("knobs", [{}, {"method_column": True}, {"two_args": True}], ids=["fwd", "mcol", "two_args"])
def test_handler_ref_against_spec(seed, knobs):
    N, n_state, M = 400, 350, 5000
    c = forward_corpus(M, N, n_state, seed, **knobs)
    state0 = torch.arange(n_state, dtype=torch.int64) * 1000
    for cap_of in (lambda E: E + 3, lambda E: E // 2, None):
        sp = forward_spec(corpus_rows(c), c["resolve"], n_state, state0.tolist(), cap_of is not None, ordered=True)
        state = state0.clone()
        if cap_of is None:
            val, st = _cpu_send(c, state, None)
        else:
            cap = cap_of(sp.E)
            ob = DeviceOutbox(cap, device="cpu")
            for k in ("a0", "a1", "a2"):
                ob.bank[k].fill_(-77)
            val, st = _cpu_send(c, state, ob)
            want = sp.outbox_after(cap)
            sp.check_outbox(cap, ob.bank["count"].tolist(), _records(ob, want["filled"]))
            assert all(bool((ob.bank[k][want["filled"]:] == -77).all()) for k in ("a0", "a1", "a2"))
        sp.check_replies(st.tolist(), val.tolist())
        assert state.tolist() == sp.state_after


def _exchange(c, state0):
    N = c["N"]
    table = RegistryTable(4 * N, device="cpu")
    ids = torch.arange(N, dtype=torch.int64)
    table.upsert(actor_keys(ids), torch.zeros(N, dtype=torch.int32), _t(c["mbox_of"], torch.int32))
    state = torch.tensor(state0, dtype=torch.int64)
    return ActorExchange(table, 8192, state=state), state


def _batch(c, device="cpu"):
    m = c["method"] if isinstance(c["method"], int) else _t(c["method"], torch.int16).to(device)
    f = (lambda x, dt=torch.int64: None if x is None else _t(x, dt).to(device))
    return B.MsgBatch(f(c["actor"], torch.int32), f(c["a0"]), f(c["a1"]), f(c["a2"]), m)


@pytest.mark.parametrize("knobs", [{}, {"method_column": True}, {"two_args": True}], ids=["fwd", "mcol", "two_args"])
def test_cpu_exchange_send_against_spec(knobs):
    c = forward_corpus(5000, 400, 350, 4, **knobs)
    state0 = list(range(0, 3500, 10))
    sp = forward_spec(corpus_rows(c), c["resolve"], 350, state0, True, ordered=True)
    ex, state = _exchange(c, state0)
    ex.outbox = DeviceOutbox(sp.E - 10, device="cpu")
    val, st = ex.send(_batch(c))
    sp.check_replies(st.tolist(), val.tolist())
    sp.check_outbox(sp.E - 10, ex.outbox.bank["count"].tolist(), _records(ex.outbox, sp.E - 10))
    assert state.tolist() == sp.state_after


def test_cpu_pump_against_simulation():
    c = forward_corpus(5000, 400, 350, 5, max_a1=3)
    state0 = [0] * 350
    epochs, delivered, final = simulate_pump(c, state0)
    assert 2 <= epochs <= 3 and delivered > 5000
    ex, state = _exchange(c, state0)
    ob = DeviceOutbox(8192, device="cpu")
    got = ex.pump(ob, initial=_batch(c))
    assert got == (epochs, delivered) and ob.dropped == 0
    assert state.tolist() == final
