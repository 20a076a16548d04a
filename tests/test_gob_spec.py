"""The gob value-message contract (tests/_gob_spec.py) pinned by hand, and the two host
parsers held to it on the malformed-input corpus.

The spec is pinned from outside so it does not validate itself: a table of hand-written
messages with the status and values they must parse to, and ``encode_message`` byte for
byte against the host codec (``_core.gob_encode``, itself pinned by the golden bytes of
tests/test_gob.py) on every width-edge value.  Then every parser equals the spec on every
corpus message, by exact equality:

* ``decode_structs_ref`` (ptype_amd/ops/gob.py), the oracle of tests/test_gob_gpu.py;
* ``host_batch_multiply`` (csrc/core/netrpc.cpp), called by address as the net/rpc
  server calls it: status per message, and the product of the two argument fields for
  the OK ones.  A delta past 2^31 once indexed its value array from below (the
  ``gobparse`` scenario of tests/native/core_stress.cpp runs that under ASan).

The GPU decoder and the bridge meet the same corpus in tests/test_gob_edges_gpu.py.
"""
import numpy as np
import pytest
import torch

import _gob_spec as S
from ptype_amd import _core
from ptype_amd.ops import gob as G

NFS = (1, 2, 3, 8)

# (hex message, nf, type id) -> (status, values); written by hand from the format
PINNED = [
    ("07ff82010e011000", 2, 65, S.OK, [7, 8]),                       # Args{7, 8}: the golden of test_gob_gpu
    ("03ff8200", 2, 65, S.OK, [0, 0]),                               # Args{0, 0}: no field written
    ("09ff82fcffffffff0e00", 2, 65, S.BAD_FIELD, [0, 0]),            # delta 0xFFFFFFFF
    ("09ff82fb01000000010e00", 2, 65, S.TRUNCATED, [0, 0]),          # delta 2^32 + 1, length one short
    ("0aff82fb01000000010e00", 2, 65, S.BAD_FIELD, [0, 0]),          # delta 2^32 + 1: not delta 1
    ("05ff82020e00", 2, 65, S.OK, [0, 7]),                           # delta 2 from -1: field 1
    ("05ff82030e00", 2, 65, S.BAD_FIELD, [0, 0]),                    # delta 3: field 2 of 2
    ("04ff820300", 2, 65, S.BAD_FIELD, [0, 0]),                      # bad delta decided before its value
    ("04ff8201fe", 2, 65, S.TRUNCATED, [0, 0]),                      # value's count byte, no payload
    ("0eff8201f701010101010101010100", 2, 65, S.TRUNCATED, [0, 0]),  # a 9-byte value
    ("0dff8201f8ffffffffffffffff00", 2, 65, S.OK, [-(1 << 63), 0]),  # int64 min: 8 bytes of ones
    ("0dff8201f8fffffffffffffffe00", 2, 65, S.OK, [(1 << 63) - 1, 0]),
    ("04ff82017f", 1, 65, S.TRUNCATED, [0]),                         # no terminator
    ("05ff82017f00", 1, 65, S.OK, [-64]),                            # zigzag 127: the last 1-byte value
    ("06ff8201ff8000", 1, 65, S.OK, [64]),                           # zigzag 128: the first 2-byte value
    ("06ff8201fe007f00", 1, 65, S.TRUNCATED, [0]),                   # non-minimal value, length one short
    ("07ff8201fe007f00", 1, 65, S.OK, [-64]),                        # non-minimal value: accepted
    ("ff05ff82017f00", 1, 65, S.OK, [-64]),                          # non-minimal length: accepted
    ("06ff82017f0000", 1, 65, S.TRAILING, [0]),                      # a byte after the terminator
    ("03ff8400", 1, 65, S.WRONG_TYPE, [0]),                          # type id 66
    ("03ff8100", 1, 65, S.WRONG_TYPE, [0]),                          # type id -65
    ("020200", 1, 1, S.OK, [0]),                                     # type id 1: one byte
    ("00", 1, 65, S.WRONG_TYPE, [0]),                                # length 0: no type id to read
    ("", 1, 65, S.TRUNCATED, [0]),                                   # the empty message
    ("04ff82", 1, 65, S.TRUNCATED, [0]),                             # length says 4, 2 follow
    ("f7010101010101010101", 1, 65, S.TRUNCATED, [0]),               # a 9-byte length
]


def test_statuses_are_the_packages():
    assert (S.OK, S.TRUNCATED, S.WRONG_TYPE, S.BAD_FIELD, S.TRAILING) == (
        G.STATUS_OK, G.STATUS_TRUNCATED, G.STATUS_WRONG_TYPE, G.STATUS_BAD_FIELD, G.STATUS_TRAILING)
    assert S.MAX_FIELDS == G.MAX_FIELDS and S.REPLY.itemsize == _core.REPLY_RECORD_BYTES == 16


@pytest.mark.parametrize("hexmsg,nf,tid,status,values", PINNED)
def test_spec_parses_hand_written_messages(hexmsg, nf, tid, status, values):
    assert S.parse_message(bytes.fromhex(hexmsg), nf, tid) == (status, values)


def test_spec_encodes_hand_written_messages():
    assert S.encode_message((7, 8), 65).hex() == "07ff82010e011000"
    assert S.encode_message((0, 0), 65).hex() == "03ff8200"
    assert S.encode_message((0, 7), 65).hex() == "05ff82020e00"
    assert S.encode_message((-(1 << 63), 0), 65).hex() == "0dff8201f8ffffffffffffffff00"
    assert S.encode_message((64,), 65).hex() == "06ff8201ff8000"
    assert S.encode_message((0,), 1).hex() == "020200"
    assert S.GOLDEN_OVERRUN.hex() == PINNED[2][0]


@pytest.mark.parametrize("nf", range(1, 9))
def test_spec_encode_equals_the_host_codec(nf):
    rows = S.edge_rows(nf) + (S.mask_rows(nf) if nf in (1, 2, 3, 4, 8) else [])
    data, offs = S.encode_rows(rows, 65)
    ref, ref_offs = G.encode_structs_ref([torch.from_numpy(c) for c in S.columns(rows, nf)], 65)
    assert ref_offs.tolist() == offs.tolist()
    assert bytes(ref.tolist()) == data.tobytes()
    st, cols = S.parse_batch(data, offs, nf, 65)  # and the spec reads back what it wrote
    assert not st.any()
    for got, want in zip(cols, S.columns(rows, nf)):
        assert np.array_equal(got, want)


def test_vectorised_helpers_equal_the_scalar_spec():
    rows = S.edge_rows(3) + S.mask_rows(3)
    for tid in (1, 65, 8192, (1 << 32) - 1):
        data, offs = S.encode_rows(rows, tid)
        assert np.array_equal(S.message_lengths(S.columns(rows, 3), tid), np.diff(offs))
        msgs = [S.encode_message(r, tid) for r in rows]
        for M in (0, 1, len(rows) - 1, len(rows), 3 * len(rows) + 7):
            tb, to = S.tile_messages(msgs, M)
            eb, eo = S.pack([msgs[i % len(msgs)] for i in range(M)])
            assert np.array_equal(to, eo) and np.array_equal(tb, eb)
            assert np.array_equal(S.tile_rows(np.arange(len(rows)), M), np.arange(M) % len(rows))


@pytest.mark.parametrize("nf", NFS)
def test_corpus_covers_every_status_and_keeps_its_neighbours(nf):
    data, offs, nf, tid, labels = S.corpus_batch(nf)
    st, cols = S.parse_batch(data, offs, nf, tid)
    assert len(labels) == len(st) < 6000 and int(offs[-1]) == data.shape[0]
    assert set(st.tolist()) == {S.OK, S.TRUNCATED, S.WRONG_TYPE, S.BAD_FIELD, S.TRAILING}
    good = np.array([x == "good" for x in labels])
    assert not st[good].any() and labels[-1] == "last:cut" and st[-1] == S.TRUNCATED
    assert good[:-1:2].all() and not good[1::2].any()  # every mutated message between two untouched ones
    for c in cols:
        assert not c[st != S.OK].any()


@pytest.mark.parametrize("nf", NFS)
def test_oracle_equals_spec_on_corpus(nf):
    data, offs, nf, tid, labels = S.corpus_batch(nf)
    want_st, want_cols = S.parse_batch(data, offs, nf, tid)
    cols, st = G.decode_structs_ref(torch.from_numpy(data), torch.from_numpy(offs), nf, tid)
    bad = [(labels[i], int(st[i]), int(want_st[i])) for i in np.flatnonzero(st.numpy() != want_st)]
    assert not bad, bad[:10]
    for got, want in zip(cols, want_cols):
        assert np.array_equal(got.numpy(), want)


def test_oracle_answers_a_nine_byte_value_with_a_status():
    msg = bytes.fromhex("0eff8201f701010101010101010100")
    cols, st = G.decode_structs_ref(torch.tensor(list(msg), dtype=torch.uint8), torch.tensor([0, len(msg)]), 2, 65)
    assert st.tolist() == [S.TRUNCATED] and [c.tolist() for c in cols] == [[0], [0]]


@pytest.mark.parametrize("nf", NFS)
def test_host_batch_parser_equals_spec_on_corpus(nf):
    data, offs, nf, tid, labels = S.corpus_batch(nf)
    want_st, want_cols = S.parse_batch(data, offs, nf, tid)
    field_col = [0, 1 if nf > 1 else -1, -1, -1]
    rc, gst, rep = S.call_batch(_core.host_batch_multiply(), data, offs, nf, tid, field_col)
    assert rc == 0
    bad = [(labels[i], int(gst[i]), int(want_st[i])) for i in np.flatnonzero(gst != want_st)]
    assert not bad, bad[:10]
    a = want_cols[0].astype(np.uint64)
    b = want_cols[1].astype(np.uint64) if nf > 1 else np.zeros_like(a)
    ok = want_st == S.OK
    assert np.array_equal(rep["value"][ok].astype(np.uint64), (a * b)[ok])  # mod 2^64
    assert not rep["value"][~ok].any() and not rep["status"].any()


def test_host_batch_parser_bounds_the_delta_as_a_u64():
    """The deltas a truncating ``field += (int)delta`` lets through: 0xFFFFFFFF moved the
    index to -2 and the value was written below the array; 2^32 + 1 counted as 1."""
    big = [S.frame(S.put_int(65) + S.put_uint(d) + b"\x0e\x00") for d in S.BIG_DELTAS]
    short = bytes.fromhex("04ff8201fe")  # a value cut short is TRUNCATED, as in the kernel
    msgs = [S.encode_message((7, 8), 65), S.GOLDEN_OVERRUN] + big + [short, S.encode_message((-3, 5), 65)]
    data, offs = S.pack(msgs)
    rc, gst, rep = S.call_batch(_core.host_batch_multiply(), data, offs, 2, 65, [0, 1, -1, -1])
    assert rc == 0
    assert gst.tolist() == [S.OK] + [S.BAD_FIELD] * 6 + [S.TRUNCATED, S.OK]
    assert rep["value"].tolist() == [56] + [0] * 7 + [-15]
