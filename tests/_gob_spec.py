"""The gob value-message format, written once from its rules -- the contract the three
parsers of this project are held to (``gob_decode_kernel`` of csrc/hip/gob.hip,
``host_batch_multiply`` of csrc/core/netrpc.cpp, ``decode_structs_ref`` of
ptype_amd/ops/gob.py) and the GPU encoder is compared with.  Plain Python on unbounded
ints; nothing here calls a parser or an encoder of the package.

    message = uint(len) int(type id) { uint(delta) int(value) }* 0
    uint(x) = x < 128 ? byte(x) : byte(256 - n) + the n big-endian bytes of x
    int(i)  = uint(i < 0 ? ~i << 1 | 1 : i << 1)

Encoding: zero fields are omitted, a delta counts from the last written field (from -1),
the struct ends with 0, the length counts everything after it.

Parsing (``parse_message``), in this order:

* a ``uint`` read fails on no bytes left, on a count byte meaning more than 8 bytes, or
  on fewer bytes left than the count; non-minimal encodings are accepted, as Go does;
* length: a failed read, or ``len != bytes remaining`` -> TRUNCATED;
* type id: a failed read, or an id ``!= type_id`` -> WRONG_TYPE;
* delta: a failed read -> TRUNCATED; 0 ends the struct; ``delta > 8`` or
  ``field + delta >= nf`` -> BAD_FIELD, on the untruncated integers and before the value
  is looked at; a failed value read -> TRUNCATED;
* bytes left after the terminator -> TRAILING;
* any status but OK: all values zero.

The numpy half builds the large batches (lengths from bit lengths, a short pattern of
messages tiled to M rows) without a Python loop over the rows, and ``call_batch`` calls a
``DeviceBatchFn`` (csrc/core/netrpc.hpp) by address.
"""
from __future__ import annotations

import ctypes

import numpy as np

OK, TRUNCATED, WRONG_TYPE, BAD_FIELD, TRAILING = 0, 1, 2, 3, 4
MAX_FIELDS = 8
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


# ----------------------------------------------------------------- the format
def put_uint(x: int) -> bytes:
    assert 0 <= x < 1 << 64, x
    if x < 128:
        return bytes([x])
    n = (x.bit_length() + 7) // 8
    return bytes([256 - n]) + x.to_bytes(n, "big")


def zz(i: int) -> int:
    return ((~i) << 1) | 1 if i < 0 else i << 1


def unzz(u: int) -> int:
    return ~(u >> 1) if u & 1 else u >> 1


def put_int(i: int) -> bytes:
    return put_uint(zz(i))


def tokens(row, type_id: int) -> list[tuple[str, bytes]]:
    """The message body of ``row`` as (kind, bytes) pieces: tid, (delta, value)*, end."""
    out = [("tid", put_int(type_id))]
    last = -1
    for f, v in enumerate(row):
        assert INT64_MIN <= v <= INT64_MAX, v
        if v == 0:
            continue
        out += [("delta", put_uint(f - last)), ("value", put_int(v))]
        last = f
    return out + [("end", b"\x00")]


def frame(body: bytes) -> bytes:
    return put_uint(len(body)) + body


def encode_message(row, type_id: int) -> bytes:
    return frame(b"".join(t for _, t in tokens(row, type_id)))


def get_uint(b: bytes, pos: int):
    """(value, next pos), or None where the read fails."""
    if pos >= len(b):
        return None
    c0 = b[pos]
    if c0 < 0x80:
        return c0, pos + 1
    n = 256 - c0
    if n > 8 or len(b) - (pos + 1) < n:
        return None
    return int.from_bytes(b[pos + 1:pos + 1 + n], "big"), pos + 1 + n


def parse_message(b: bytes, nf: int, type_id: int) -> tuple[int, list[int]]:
    zero = [0] * nf
    r = get_uint(b, 0)
    if r is None or r[0] != len(b) - r[1]:
        return TRUNCATED, zero
    r = get_uint(b, r[1])
    if r is None or unzz(r[0]) != type_id:
        return WRONG_TYPE, zero
    pos, field, vals = r[1], -1, list(zero)
    while True:
        r = get_uint(b, pos)
        if r is None:
            return TRUNCATED, zero
        delta, pos = r
        if delta == 0:
            break
        if delta > MAX_FIELDS or field + delta >= nf:
            return BAD_FIELD, zero
        field += delta
        r = get_uint(b, pos)
        if r is None:
            return TRUNCATED, zero
        vals[field], pos = unzz(r[0]), r[1]
    if pos != len(b):
        return TRAILING, zero
    return OK, vals


# ----------------------------------------------------------------- values at the width edges
def edge_values() -> list[int]:
    """0, +-1, the 1/2-byte edge (63 | 64, -64 | -65), and for every k in 1..8 the four
    values around a k-byte zigzag payload's ends (2^(8k-1) - 1 | 2^(8k-1) and
    -2^(8k-1) | -2^(8k-1) - 1, where int64 holds them), int64 min and max."""
    vals = {0, 1, -1, 63, 64, -64, -65, INT64_MIN, INT64_MAX}
    for k in range(1, 9):
        h = 1 << (8 * k - 1)
        vals |= {h - 1, h, -h, -h - 1}
    return sorted(v for v in vals if INT64_MIN <= v <= INT64_MAX)


def edge_rows(nf: int) -> list[tuple[int, ...]]:
    """Every edge value in every field position (the other fields zero), and in all at once."""
    rows = []
    for v in edge_values():
        for f in range(nf):
            rows.append(tuple(v if k == f else 0 for k in range(nf)))
        rows.append((v,) * nf)
    return rows


MASK_VALUES = (1, -65, 1 << 15, -(1 << 23) - 1, 1 << 31, (1 << 47) - 1, -(1 << 55), INT64_MIN)


def mask_rows(nf: int) -> list[tuple[int, ...]]:
    """All 2^nf present / absent patterns (field f present = MASK_VALUES[f], a width of its own)."""
    return [tuple(MASK_VALUES[f] if m >> f & 1 else 0 for f in range(nf)) for m in range(1 << nf)]


def encode_rows(rows, type_id: int) -> tuple[np.ndarray, np.ndarray]:
    """(bytes uint8, offsets int64[M + 1]) of a small batch, message by message."""
    msgs = [encode_message(r, type_id) for r in rows]
    return pack(msgs)


def pack(msgs) -> tuple[np.ndarray, np.ndarray]:
    offs = np.zeros(len(msgs) + 1, dtype=np.int64)
    if msgs:
        offs[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b"".join(msgs), dtype=np.uint8).copy(), offs


def columns(rows, nf: int) -> list[np.ndarray]:
    a = np.array([[int(v) for v in r] for r in rows], dtype=np.int64).reshape(len(rows), nf)
    return [np.ascontiguousarray(a[:, f]) for f in range(nf)]


# ----------------------------------------------------------------- vectorised (numpy)
def _uint_len(x: np.ndarray) -> np.ndarray:
    """Wire bytes of uint(x), x uint64: 1 below 128, else 1 + the bytes its bit length needs."""
    nbytes = np.ones(x.shape, dtype=np.int64)
    for k in range(1, 8):
        nbytes += x >= np.uint64(1 << (8 * k))
    return np.where(x < np.uint64(128), 1, 1 + nbytes)


def _zz_np(v: np.ndarray) -> np.ndarray:
    return ((v << 1) ^ (v >> 63)).view(np.uint64)


def message_lengths(cols, type_id: int) -> np.ndarray:
    """Whole-message lengths (length byte included) of the rows of int64 columns ``cols``."""
    M = cols[0].shape[0]
    body = np.full(M, len(put_int(type_id)) + 1, dtype=np.int64)
    for c in cols:
        body += np.where(c != 0, 1 + _uint_len(_zz_np(c)), 0)  # a delta is 1..8: one byte
    assert int(body.max(initial=0)) < 128  # one length byte
    return body + 1


def tile_messages(msgs, M: int) -> tuple[np.ndarray, np.ndarray]:
    """The pattern ``msgs`` repeated to M messages: (bytes, offsets int64[M + 1])."""
    P = len(msgs)
    reps, rem = divmod(M, P)
    lens = np.array([len(m) for m in msgs], dtype=np.int64)
    all_lens = np.concatenate([np.tile(lens, reps), lens[:rem]])
    offs = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(all_lens, out=offs[1:])
    pat = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    tail = np.frombuffer(b"".join(msgs[:rem]), dtype=np.uint8)
    return np.concatenate([np.tile(pat, reps), tail]), offs


def tile_rows(a, M: int) -> np.ndarray:
    """A per-message array of the pattern repeated to M entries."""
    a = np.asarray(a)
    reps, rem = divmod(M, a.shape[0])
    return np.concatenate([np.tile(a, reps), a[:rem]])


def parse_batch(data, offs, nf: int, type_id: int) -> tuple[np.ndarray, list[np.ndarray]]:
    """The spec's (status int32[M], columns int64[nf][M]) of a small batch."""
    raw = bytes(np.asarray(data, dtype=np.uint8).tobytes())
    o = [int(x) for x in offs]
    res = [parse_message(raw[o[i]:o[i + 1]], nf, type_id) for i in range(len(o) - 1)]
    st = np.array([r[0] for r in res], dtype=np.int32)
    cols = [np.array([r[1][f] for r in res], dtype=np.int64) for f in range(nf)]
    return st, cols


# ----------------------------------------------------------------- the malformed-input corpus
BASE_ROWS = {
    1: [(5,), (300,), (0,), (-70000,)],
    2: [(7, 3), (-129, 40), (0, 9), (1 << 40, 0), (INT64_MIN, 63)],
    3: [(1, 2, 3), (0, 0, 17), (-5, 0, 0), (1 << 31, -(1 << 31), 33)],
    8: [(1, 0, -2, 0, 0, 300, 0, 21), (0,) * 7 + (4,), (1, 2, 3, 4, 5, 6, 7, 8),
        (INT64_MAX, INT64_MIN, 0, 0, 0, 0, -1, 62)],
}
BIG_DELTAS = (0xFFFFFFFF, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1)
GOLDEN_OVERRUN = bytes.fromhex("09ff82fcffffffff0e00")  # delta 0xFFFFFFFF: index -2 of a truncating parser


def mutations(row, nf: int, type_id: int) -> list[tuple[str, bytes]]:
    """(label, message) for every malformation of the message of ``row``.  Some stay
    well-formed on purpose (a non-minimal length, delta 0 first): the spec says which."""
    toks = tokens(row, type_id)
    body = b"".join(t for _, t in toks)
    full = frame(body)
    out = []
    # truncation at every byte, the length byte as it was / corrected
    for cut in range(len(full)):
        out.append((f"cut{cut}", full[:cut]))
    for k in range(len(body)):
        out.append((f"cut{k}-relen", frame(body[:k])))
    # the length byte
    n = len(body)
    out += [("len+1", put_uint(n + 1) + body), ("len-1", put_uint(n - 1) + body), ("len0", b"\x00" + body),
            ("len0-alone", b"\x00"), ("len-ff", b"\xff" + bytes([n]) + body),
            ("len-fe00", b"\xfe\x00" + bytes([n]) + body), ("empty", b"")]
    # count bytes at each uint position: 9 bytes, 128 bytes, a legal count with its payload cut short
    for where in ("f7", "80", "fe"):
        bad = {"f7": b"\xf7" + b"\x01" * 9, "80": b"\x80" + b"\x01" * 3, "fe": b"\xfe\x01"}[where]
        out.append((f"len-{where}", bad + body))
        out.append((f"len-{where}-alone", bad[:2]))
        for j, (kind, _) in enumerate(toks):
            if kind == "end":
                continue
            head = b"".join(t for _, t in toks[:j])
            rest = b"".join(t for _, t in toks[j + 1:])
            out.append((f"{kind}{j}-{where}", frame(head + bad + rest)))
            out.append((f"{kind}{j}-{where}-last", frame(head + bad)))
            out.append((f"{kind}{j}-{where}-oldlen", put_uint(n) + head + bad + rest))
    # deltas, first and after field 0
    tid = toks[0][1]
    for d in (0, nf, nf + 1, 8, 9) + BIG_DELTAS:
        out.append((f"delta{d}", frame(tid + put_uint(d) + b"\x0e\x00")))
        out.append((f"delta{d}-novalue", frame(tid + put_uint(d))))
        out.append((f"delta1+{d}", frame(tid + b"\x01\x10" + put_uint(d) + b"\x0e\x00")))
    out.append(("delta0-only", frame(tid + b"\x00")))
    # type ids
    for t in (64, 66, -65):
        out.append((f"tid{t}", frame(put_int(t) + body[len(tid):])))
    z = zz(type_id)
    wide = bytes([256 - ((z.bit_length() + 7) // 8 + 1)]) + z.to_bytes((z.bit_length() + 7) // 8 + 1, "big")
    out.append(("tid-nonminimal", frame(wide + body[len(tid):])))
    # trailing bytes
    out += [("trail1", frame(body + b"\x00")), ("trail1-oldlen", full + b"\x00"),
            ("trail20", frame(body + bytes(range(1, 21)))), ("trail-struct", frame(body + body[len(tid):]))]
    return out


def corpus(nf: int, type_id: int = 65, actors: int = 64):
    """The corpus for ``nf`` fields: (messages, labels).  Every mutated message stands
    between two untouched ones -- a base row with its last field set to a rotating id
    below ``actors``, so a bridge test spreads them over its actors -- and the last
    message of the batch is a truncated one: its missing bytes lie past the buffer."""
    msgs, labels = [], []
    k = 0
    for bi, row in enumerate(BASE_ROWS[nf]):
        for label, m in mutations(row, nf, type_id):
            good = BASE_ROWS[nf][k % len(BASE_ROWS[nf])][:-1] + (k % actors,)
            msgs += [encode_message(good, type_id), m]
            labels += ["good", f"row{bi}:{label}"]
            k += 1
    full = encode_message(BASE_ROWS[nf][-1], type_id)
    msgs.append(full[:-2])
    labels.append("last:cut")
    return msgs, labels


def corpus_batch(nf: int, type_id: int = 65):
    """(bytes uint8, offsets int64[M + 1], nf, type_id, labels), the buffer exactly as
    long as its messages."""
    msgs, labels = corpus(nf, type_id)
    data, offs = pack(msgs)
    return data, offs, nf, type_id, labels


# ----------------------------------------------------------------- a DeviceBatchFn by address
REPLY = np.dtype([("value", "<i8"), ("status", "<i4"), ("actor", "<u4")])
_BATCH_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                             ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)


def call_batch(handle, data, offs, nf: int, type_id: int, field_col):
    """Call the ``DeviceBatchFn`` ``handle = (fn, ctx)`` on a batch: (rc, gob status
    int32[n], replies REPLY[n]).  The byte buffer handed over is exactly as long as the
    batch; the replies are 16-byte aligned like ``ReplyRecord``."""
    assert REPLY.itemsize == 16
    fn, ctx = handle
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n = offs.shape[0] - 1
    assert int(offs[n]) == data.shape[0]
    col = np.array(list(field_col), dtype=np.int32)
    assert col.shape == (4,)
    gst = np.full(max(n, 1), -1, dtype=np.int32)
    raw = np.zeros((max(n, 1) + 1) * 16, dtype=np.uint8)
    skew = (-raw.ctypes.data) % 16
    rep = raw[skew:skew + max(n, 1) * 16].view(REPLY)
    rep["status"] = -1
    keep = data if data.shape[0] else np.zeros(1, dtype=np.uint8)
    rc = _BATCH_FN(fn)(ctx, keep.ctypes.data, offs.ctypes.data, n, type_id, nf, col.ctypes.data, gst.ctypes.data,
                       rep.ctypes.data)
    return rc, gst[:n], rep[:n]
