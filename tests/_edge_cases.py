"""Integer models of the data plane's width-adaptive encodings, and boundary-value
batches for them.  Plain Python ints, written from the documented rules (never by
calling a kernel), so a test can predict -- before a Send -- which messages fit the
widths in force, how many take the fallback (spill, escape, overflow, long form) and
which widths the Send leaves behind.

Every encoding stores signed arguments zigzag-encoded (gob's signed-int form,
csrc/hip/packed.hpp zz_enc): a value fits a w-bit field iff zz(v) < 2**w, i.e. iff
-(2**(w-1)) <= v <= 2**(w-1) - 1.
"""
from __future__ import annotations

import torch

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
U64 = (1 << 64) - 1

TILE = 4096        # messages per sort tile (csrc/hip/sort_common.hpp kSTile)
SMALL_TILE = 1024  # the small-batch kernels' tile
REC8_PAYLOAD = 52  # 8-B ring record: 12-bit place in the tile + 52 bits of fields
REC8_MAX_WM = 24


def zz(v: int) -> int:
    """Zigzag of an int64 as an unsigned 64-bit int: 0, -1, 1, -2 ... -> 0, 1, 2, 3 ..."""
    assert INT64_MIN <= v <= INT64_MAX, v
    return ((v << 1) ^ (v >> 63)) & U64


def unzz(z: int) -> int:
    assert 0 <= z <= U64, z
    return (z >> 1) ^ -(z & 1)


def bit_len(x: int) -> int:
    return int(x).bit_length()


def fits(v: int, w: int) -> bool:
    """Whether int64 ``v`` fits a ``w``-bit zigzag field."""
    return zz(v) < (1 << w)


def fits_i32(v: int) -> bool:
    """The compact 16-B ring record's argument test (two's complement, not zigzag)."""
    return INT32_MIN <= v <= INT32_MAX


def edge_values(w: int, extremes: bool = False) -> list[int]:
    """The values around a ``w``-bit zigzag field's two ends, clipped to int64 and in
    ascending order: {-(2^(w-1)) - 1, -(2^(w-1)), -1, 0, 1, 2^(w-1) - 1, 2^(w-1)}.  The
    outer pair does not fit the field, its neighbours are the widest values that do.
    ``extremes``: INT64_MIN and INT64_MAX as well."""
    assert 1 <= w <= 64, w
    h = 1 << (w - 1)
    vals = {-h - 1, -h, -1, 0, 1, h - 1, h}
    if extremes:
        vals |= {INT64_MIN, INT64_MAX}
    return sorted(v for v in vals if INT64_MIN <= v <= INT64_MAX)


# ----------------------------------------------------------------- 8-B ring records
def rec8_first(n_state: int, n_dir: int) -> tuple[int, int, int]:
    """(wm, w0, w1) of a mailbox set's first 8-B Send: the mailbox field from the state
    size or the directory (20 bits when neither says more than one), clamped to 1..24,
    the other 52 - wm bits split between the arguments (a1 takes the odd one)."""
    nmb = max(n_state, n_dir)
    wm = bit_len(nmb - 1) if nmb > 1 else 20
    wm = max(1, min(wm, REC8_MAX_WM))
    w0 = (REC8_PAYLOAD - wm) // 2
    return wm, w0, REC8_PAYLOAD - wm - w0


def rec8_next(bm: int, b0: int, b1: int) -> tuple[int, int, int, bool]:
    """(wm, w0, w1, wide) after a Send whose OR-ed mailbox / zigzag a0 / zigzag a1 fields
    have bit lengths (bm, b0, b1): each field as wide as its largest value (at least
    1 bit), the slack of the 52 payload bits split between the arguments (a1 takes the
    odd bit).  ``wide``: the mailbox passes 24 bits or the sum passes 52 -- the next
    Send gives up 8-B records (the widths reported then are the clamped split)."""
    wm, n0, n1 = max(bm, 1), max(b0, 1), max(b1, 1)
    if wm <= REC8_MAX_WM and wm + n0 + n1 <= REC8_PAYLOAD:
        w0 = n0 + (REC8_PAYLOAD - wm - n0 - n1) // 2
        return wm, w0, REC8_PAYLOAD - wm - w0, False
    wmc = min(wm, REC8_MAX_WM)
    w0 = (REC8_PAYLOAD - wmc) // 2
    return wmc, w0, REC8_PAYLOAD - wmc - w0, True


def rec8_fits(field: int, a0: int, a1: int, widths) -> bool:
    """Whether a message (mailbox or actor-id field, a0, a1) fits the 8-B widths."""
    wm, w0, w1 = widths[:3]
    return field < (1 << wm) and fits(a0, w0) and fits(a1, w1)


def or_bits(values, zigzag: bool = True) -> int:
    """Bit length of the OR of a column's (zigzag) fields: what a Send measures."""
    acc = 0
    for v in values:
        acc |= zz(int(v)) if zigzag else int(v)
    return bit_len(acc)


# ----------------------------------------------------------------- wire v3 reply bound
def multiply_reply_bits(a0: int, a1: int) -> int:
    """packed_reply_bits' Multiply bound on one message: bits of 2 |a0| |a1| (64 when
    it passes 64), at least the 8 a status code needs."""
    mag = lambda z: z // 2 + (z & 1)  # noqa: E731
    p = 2 * mag(zz(a0)) * mag(zz(a1))
    return max(8, 64 if p >> 64 else bit_len(p))


def sx_arg_caps(w, vb: int, z0_agreed: int, z1_agreed: int, saw_multiply: bool = True) -> tuple[int, int]:
    """The sorted exchange's admission caps on zigzag a0 / a1 of a Multiply message under
    the layout in force (field widths ``w`` = [method, mailbox, a0, a1, a2], ``vb`` reply
    bytes, the agreed zigzag maxima): the fields' all-ones under an 8-byte reply plane;
    else the largest pair with 2 |a0| |a1| < 2^(8 vb) reached from the agreed maxima
    (when that agreement saw Multiply; else from zero) by raising a0's cap as far as
    its field and the bound allow, then a1's."""
    f0, f1 = (1 << w[2]) - 1, (1 << w[3]) - 1
    if vb >= 8:
        return f0, f1
    lim = 1 << (8 * vb)
    mag = lambda z: z // 2 + (z & 1)  # noqa: E731
    ok = lambda x, y: 2 * mag(x) * mag(y) < lim  # noqa: E731

    def widest(f, y):  # the largest x <= f with ok(x, y): mag(2 q) = q
        return f if ok(f, y) else min(f, 2 * ((lim - 1) // (2 * mag(y))))

    a0, a1 = (min(z0_agreed, f0), min(z1_agreed, f1)) if saw_multiply else (0, 0)
    assert ok(a0, a1)
    a0 = max(a0, widest(f0, a1))
    a1 = max(a1, widest(f1, a0))
    return a0, a1


def sx_admits(caps, a0: int, a1: int) -> bool:
    """Whether the sender admits a Multiply message: both arguments within the caps."""
    return zz(a0) <= caps[0] and zz(a1) <= caps[1]


# ----------------------------------------------------------------- batches
def edge_positions(M: int, count: int, tile: int = TILE) -> list[int]:
    """``count`` distinct message indices for edge messages: first the places where a
    sort goes wrong -- lanes 0, 63 and 64 and the last place of tile 0, the first of
    tile 1, the batch's last message -- then their neighbours outwards."""
    anchors = [0, 63, 64, tile - 1, tile, M - 1]
    out: list[int] = []
    step = 0
    while len(out) < min(count, M):
        for a in anchors:
            for p in ((a + step,) if step == 0 else (a + step, a - step)):
                if 0 <= p < M and p not in out and len(out) < count:
                    out.append(p)
        step += 1
        assert step <= M + tile, "edge_positions: batch too small"
    assert len(out) == count, f"{count} edge messages do not fit a batch of {M}"
    return out


def place(M: int, edges, n_actors: int, seed: int, small: int = 100, tile: int = TILE):
    """A batch of ``M`` (actor, a0, a1) messages: ``edges`` -- (actor or None, a0, a1)
    triples -- at ``edge_positions``, everything else small values (|a| < ``small``)
    and actors below ``n_actors`` from a seeded generator.  An edge without an actor
    keeps the random one.  Returns CPU tensors (actor int32, a0, a1 int64) and the
    positions."""
    g = torch.Generator().manual_seed(seed)
    actor = torch.randint(0, n_actors, (M,), generator=g, dtype=torch.int32)
    a0 = torch.randint(-small + 1, small, (M,), generator=g, dtype=torch.int64)
    a1 = torch.randint(-small + 1, small, (M,), generator=g, dtype=torch.int64)
    pos = edge_positions(M, len(edges), tile)
    for p, (x, v0, v1) in zip(pos, edges):
        if x is not None:
            actor[p] = int(x)
        a0[p], a1[p] = int(v0), int(v1)
    return actor, a0, a1, pos


def pairs(values0, values1):
    """Edge triples without an actor: every a0 of ``values0`` with every a1 of ``values1``."""
    return [(None, int(x), int(y)) for x in values0 for y in values1]
