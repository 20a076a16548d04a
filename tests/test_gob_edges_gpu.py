"""K4 on the GPU (csrc/hip/gob.hip, csrc/hip/gob_bridge.hpp) against the one spec of the
gob value-message format (tests/_gob_spec.py, pinned by tests/test_gob_spec.py).  Every
comparison is exact equality: bytes, offsets, statuses, columns, replies, actor state.

* encode at the width edges: every 1..8-byte zigzag payload's first and last value in
  every field position, every present / absent field pattern (deltas 1..8), type ids of
  1, 2, 3 and 5 wire bytes, batch sizes around the 256-thread block and the 1024-message
  tile with 3-byte and longest messages alternating, and the output bound with a canary;
* the two loops no smaller batch reaches: ``gob_scan_kernel``'s second trip (more than
  1024 tiles of 1024 messages) and ``gob_decode_kernel``'s second grid stride (more than
  8192 blocks of 256 messages);
* decode on the malformed-input corpus, each bad message between two good ones and the
  batch's last message cut short at the very end of the buffer;
* the bridge on the same corpus, called as the net/rpc server calls it: a message that
  does not decode runs no handler and changes no actor state, the others' replies and the
  final state are a sequential model's, and an actor field outside [0, 2^32 - 1) names
  no actor (2^32 + 3 is not actor 3).
"""
import numpy as np
import pytest
import torch

import _gob_spec as S
from ptype_amd.ops import _ptr, _stream, hip
from ptype_amd.ops import gob as G
from ptype_amd.ops.records import METHOD_COUNTER_ADD, STATUS_NO_ACTOR, STATUS_OK

pytestmark = pytest.mark.gpu

TILE, BLOCK = 1024, 256          # gob.hip kGobTile, kGobThreads
SCAN_TRIP = 1024                 # tiles per trip of gob_scan_kernel's loop
DECODE_GRID = 8192 * 256         # messages per grid stride of gob_decode_kernel
TYPE_IDS = (1, 63, 64, 65, 127, 8191, 8192, (1 << 31) - 1, (1 << 32) - 1)
ACTORS = 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_encode(cols_np, want_bytes, want_offs, tid):
    """GPU encode == (want_bytes, want_offs), then the GPU decode of it == the columns."""
    nf = len(cols_np)
    cols = [_dev(c) for c in cols_np]
    buf, offs = G.encode_structs(cols, tid)
    assert offs.shape == (cols_np[0].shape[0] + 1,) and torch.equal(offs, _dev(want_offs))
    assert buf.shape == (want_bytes.shape[0],) and torch.equal(buf, _dev(want_bytes))
    back, st = G.decode_structs(buf, offs, nf, tid)
    assert st.shape == (cols_np[0].shape[0],) and not bool(st.any())
    for a, b in zip(cols, back):
        assert torch.equal(a, b)


def _check_rows(rows, nf, tid):
    want_bytes, want_offs = S.encode_rows(rows, tid)
    _check_encode(S.columns(rows, nf), want_bytes, want_offs, tid)


# ----------------------------------------------------------------- encode at its width edges
@pytest.mark.parametrize("nf", range(1, 9))
def test_encode_every_width_edge_in_every_field(nf):
    _check_rows(S.edge_rows(nf), nf, 65)


@pytest.mark.parametrize("nf", [1, 2, 3, 4, 8])
def test_encode_every_zero_mask(nf):
    _check_rows(S.mask_rows(nf), nf, 65)


@pytest.mark.parametrize("tid", TYPE_IDS)
def test_encode_type_id_widths(tid):
    wire = 1 if tid < 64 else 2 if tid < 128 else 3 if tid < 1 << 15 else 5 if tid < 1 << 31 else 6
    assert len(S.put_int(tid)) == wire
    _check_rows(S.edge_rows(2) + S.mask_rows(2), 2, tid)


@pytest.mark.parametrize("tid", [1, (1 << 32) - 1])
@pytest.mark.parametrize("M", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, TILE - 1, TILE, TILE + 1, 4 * TILE + 1])
def test_encode_batch_sizes_at_block_and_tile_edges(M, tid):
    """The shortest message (no field written) and the longest (eight 10-byte fields)
    alternate, so every prefix inside the block scan differs from its neighbours."""
    rows = [(0,) * 8, (S.INT64_MIN,) * 8]
    msgs = [S.encode_message(r, tid) for r in rows]
    assert len(msgs[1]) == 2 + len(S.put_int(tid)) + 80 and (tid != 1 or len(msgs[0]) == 3)
    want_bytes, want_offs = S.tile_messages(msgs, M)
    cols = [S.tile_rows(c, M) for c in S.columns(rows, 8)]
    assert np.array_equal(S.message_lengths(cols, tid), np.diff(want_offs))
    _check_encode(cols, want_bytes, want_offs, tid)


@pytest.mark.parametrize("tid", [65, (1 << 32) - 1])
def test_encode_stays_inside_its_bound(tid):
    """The longest batch there is (every field int64 min) written into a buffer longer
    than ``gob_max_bytes`` says it needs: the total is within the bound and no byte at
    or past the total is touched."""
    h, M, nf, canary = hip(), 1500, 8, 0xA5
    cols = [torch.full((M,), S.INT64_MIN, dtype=torch.int64, device="cuda") for _ in range(nf)]
    bound = h.gob_max_bytes(M, nf, tid)
    out = torch.full((bound + 4096,), canary, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(M + 1, dtype=torch.int64, device="cuda")
    ws = torch.empty(h.gob_ws_words(M), dtype=torch.int64, device="cuda")
    h.gob_encode([_ptr(c) for c in cols], M, tid, _ptr(out), _ptr(offsets), _ptr(ws), _stream(cols[0]))
    total = int(offsets[M].item())
    one = S.encode_message((S.INT64_MIN,) * nf, tid)
    assert total == M * len(one) and total <= bound
    assert bool((out[total:] == canary).all())
    assert torch.equal(out[:total], _dev(np.tile(np.frombuffer(one, dtype=np.uint8), M)))


# ----------------------------------------------------------------- the two loops' second trips
def _scan_pattern():
    ev = S.edge_values()
    rows = [(ev[(5 * i) % len(ev)] if i % 4 else 0, ev[(7 * i + 3) % len(ev)] if i % 3 else 0) for i in range(37)]
    assert len({len(S.encode_message(r, 65)) for r in rows}) >= 8  # mixed lengths
    return rows


@pytest.mark.parametrize("M", [SCAN_TRIP * TILE + 1, 2 * SCAN_TRIP * TILE + TILE + 1])
def test_encode_scan_takes_a_second_trip(M):
    """More than 1024 tiles: the one-block scan of the tile totals loops, and its carry
    hands the running total from one trip to the next (M = 1024 * 1024 + 1 is the
    smallest batch with a second trip; the larger one has a third, of two tiles)."""
    rows = _scan_pattern()
    assert (M + TILE - 1) // TILE > SCAN_TRIP
    cols = [S.tile_rows(c, M) for c in S.columns(rows, 2)]
    want_bytes, want_offs = S.tile_messages([S.encode_message(r, 65) for r in rows], M)
    assert np.array_equal(S.message_lengths(cols, 65), np.diff(want_offs))
    _check_encode(cols, want_bytes, want_offs, 65)


def test_decode_grid_stride_takes_a_second_trip():
    """More than 8192 * 256 messages: the capped decode grid strides.  The corpus, good
    and bad messages alike, tiled; statuses and columns are the tiled spec results."""
    M = DECODE_GRID + BLOCK + 1
    msgs, _ = S.corpus(3)
    data, offs = S.pack(msgs)
    st1, cols1 = S.parse_batch(data, offs, 3, 65)
    big, big_offs = S.tile_messages(msgs, M)
    cols, st = G.decode_structs(_dev(big), _dev(big_offs), 3, 65)
    assert torch.equal(st, _dev(S.tile_rows(st1, M)))
    for got, want in zip(cols, cols1):
        assert torch.equal(got, _dev(S.tile_rows(want, M)))


# ----------------------------------------------------------------- decode on the corpus
@pytest.mark.parametrize("nf", [1, 2, 3, 8])
def test_decode_equals_spec_on_corpus(nf):
    data, offs, nf, tid, labels = S.corpus_batch(nf)
    want_st, want_cols = S.parse_batch(data, offs, nf, tid)
    cols, st = G.decode_structs(_dev(data), _dev(offs), nf, tid)
    st = st.cpu().numpy()
    bad = [(labels[i], int(st[i]), int(want_st[i])) for i in np.flatnonzero(st != want_st)]
    assert not bad, bad[:10]
    for got, want in zip(cols, want_cols):
        assert np.array_equal(got.cpu().numpy(), want)


# ----------------------------------------------------------------- the bridge
def _wrap(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def _counter_model(state, st, cols, actor_f):
    """Counter.Add over the OK messages in message order: (reply value or None, reply
    status) per message; ``state`` (a list) is updated in place.  A message that did
    not decode, or names no actor of the runtime, runs no handler."""
    out = []
    for i in range(len(st)):
        actor = int(cols[actor_f][i])
        if st[i] != S.OK or not 0 <= actor < len(state):
            out.append((None, STATUS_NO_ACTOR))
            continue
        state[actor] = _wrap(state[actor] + int(cols[0][i]))
        out.append((state[actor], STATUS_OK))
    return out


def _one_per_actor(st, cols, actor_f, n_actors):
    """Message ranges in which no actor is addressed by two OK messages: Counter.Add is
    not an ordered method (records.hpp method_ordered), so only across Sends is the
    order of two adds to one actor -- and with it each reply -- defined."""
    cuts, seen = [0], set()
    for i in range(len(st)):
        actor = int(cols[actor_f][i])
        if st[i] == S.OK and 0 <= actor < n_actors:
            if actor in seen:
                cuts.append(i)
                seen = set()
            seen.add(actor)
    return list(zip(cuts, cuts[1:] + [len(st)]))


class _Bridge:
    def __init__(self):
        from ptype_amd.runtime import DeviceRuntime

        self.rt = DeviceRuntime(torch.device("cuda", 0), actors=ACTORS, shm=False)
        self.handle = self.rt.gob_bridge(METHOD_COUNTER_ADD).handle()
        self.model = [0] * ACTORS

    def state(self):
        torch.cuda.synchronize()
        return self.rt.state.cpu().tolist()

    def send(self, data, offs, nf, tid, labels, replies_exact):
        """One batch through the bridge; checks the statuses, the replies (values too
        where the batch defines them) and the actor state against the model."""
        want_st, want_cols = S.parse_batch(data, offs, nf, tid)
        rc, gst, rep = S.call_batch(self.handle, data, offs, nf, tid, [0, -1, -1, nf - 1])
        assert rc == 0
        bad = [(labels[i], int(gst[i]), int(want_st[i])) for i in np.flatnonzero(gst != want_st)]
        assert not bad, bad[:10]
        want = _counter_model(self.model, want_st, want_cols, nf - 1)
        assert rep["status"].tolist() == [s for _, s in want]
        if replies_exact:
            ok = [i for i, (_, s) in enumerate(want) if s == STATUS_OK]
            assert rep["value"][ok].tolist() == [want[i][0] for i in ok]
        assert self.state() == self.model

    def close(self):
        self.rt.close()


@pytest.fixture(scope="module")
def bridge():
    b = _Bridge()
    yield b
    b.close()


@pytest.mark.parametrize("nf", [1, 2, 3, 8])
def test_bridge_runs_no_handler_for_a_message_that_failed_to_decode(bridge, nf):
    data, offs, nf, tid, labels = S.corpus_batch(nf)
    st, cols = S.parse_batch(data, offs, nf, tid)
    assert (st != S.OK).sum() > 100 and (st == S.OK).sum() > 100
    # the whole corpus as one batch: statuses and the final state (adds commute)
    bridge.send(data, offs, nf, tid, labels, replies_exact=False)
    # and in batches that address an actor once: every reply is the model's
    for lo, hi in _one_per_actor(st, cols, nf - 1, ACTORS):
        a, b = int(offs[lo]), int(offs[hi])
        bridge.send(data[a:b].copy(), offs[lo:hi + 1] - a, nf, tid, labels[lo:hi], replies_exact=True)


def test_bridge_actor_field_out_of_range_names_no_actor(bridge):
    """An int64 actor field below 0 or from 2^32 - 1 up is answered no-actor and changes
    no state: never the actor its low 32 bits spell (2^32 + 3 -> 3, 2^32 -> 0)."""
    outside = [-1, (1 << 32) - 1, 1 << 32, (1 << 32) + 3, (1 << 63) - 1, -(1 << 63), ACTORS, (1 << 32) - 2]
    rows, labels = [], []
    for k, actor in enumerate(outside):
        rows += [(1000 + k, k % 4), (1 << 20, actor)]  # a good neighbour on actors 0..3
        labels += ["good", f"actor{actor}"]
    data, offs = S.encode_rows(rows, 65)
    before = list(bridge.model)
    bridge.send(data, offs, 2, 65, labels, replies_exact=False)
    moved = [i for i in range(ACTORS) if bridge.model[i] != before[i]]
    assert moved == [0, 1, 2, 3] and sum(bridge.model) - sum(before) == sum(1000 + k for k in range(len(outside)))
