"""The width rules of the record encodings at their edges, on the CPU.

The models of tests/_edge_cases.py (what the GPU boundary tests predict with) are
checked against brute force on Python ints, the reply-width rule of wire v3 is pinned
at the argument maxima where a field-admitted request outgrows the reply plane of a
lagged layout (the sorted exchange's sender has to refuse those), and the 8-B ring
record width rule at the sums that keep or give up 8-B records.
"""
import numpy as np
import pytest

import _edge_cases as E
from ptype_amd.ops import hip
from ptype_amd.ops import packed as P
from ptype_amd.ops.records import METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_PRIME_CHECK


def test_zigzag_model_matches_numpy_and_round_trips():
    for w in range(1, 65):
        for v in E.edge_values(w, extremes=True):
            z = E.zz(v)
            assert 0 <= z <= E.U64 and E.unzz(z) == v, (w, v)
            assert z == (2 * v if v >= 0 else -2 * v - 1), (w, v)  # gob's signed-int form
            assert z == int(P.zz(np.array([v], dtype=np.int64))[0]), (w, v)
    assert E.zz(E.INT64_MIN) == 2**64 - 1 and E.zz(E.INT64_MAX) == 2**64 - 2


@pytest.mark.parametrize("w", range(1, 65))
def test_fits_flips_between_the_outer_pairs(w):
    vals = E.edge_values(w)
    h = 1 << (w - 1)
    if w < 64:
        assert vals[0] == -h - 1 and vals[1] == -h and vals[-2] == h - 1 and vals[-1] == h
        assert [E.fits(v, w) for v in vals] == [False] + [True] * (len(vals) - 2) + [False], (w, vals)
    else:  # 2^63 and -(2^63) - 1 are no int64: every int64 fits 64 bits
        assert vals[0] == E.INT64_MIN and vals[-1] == E.INT64_MAX
        assert all(E.fits(v, w) for v in vals)
    for v in vals:  # fits against the definition: the value's own zigzag bit length
        assert E.fits(v, w) == (E.bit_len(E.zz(v)) <= w), (w, v)
    if w > 1:  # the widest fitting values need every bit of the field
        assert not E.fits(-h, w - 1) and not E.fits(h - 1, w - 1)


def test_edge_values_are_unique_sorted_and_clipped():
    assert E.edge_values(1) == [-2, -1, 0, 1]
    assert E.edge_values(2) == [-3, -2, -1, 0, 1, 2]
    assert E.edge_values(64, extremes=True) == [E.INT64_MIN, -1, 0, 1, E.INT64_MAX]
    assert E.edge_values(20, extremes=True)[0] == E.INT64_MIN


def _calc_meta(amax):
    m = [0] * P.META_WORDS
    m[P.META_ARG0] = m[P.META_ARG0 + 1] = max(E.zz(amax), E.zz(-amax))
    m[P.META_FLAGS + METHOD_CALC_MULTIPLY] = 1
    m[P.META_METHOD] = METHOD_CALC_MULTIPLY
    return m


# agreed max |a0| = |a1|, argument field bits, reply bytes, zigzag bits of the worst product the fields admit
LAGGED_REPLY_CASES = [(8, 5, 1, 10), (64, 8, 2, 16), (128, 9, 2, 18), (32768, 17, 4, 34)]


@pytest.mark.parametrize("amax,w,vb,worst_bits", LAGGED_REPLY_CASES)
def test_fields_admit_products_wider_than_the_reply_plane(amax, w, vb, worst_bits):
    """The layout's request fields admit by bit width, its reply plane is sized from the
    maxima's values: the widest arguments that fit the fields can need more reply bits
    than ``vb`` holds.  (The sorted exchange runs a Send on the maxima of two Sends ago;
    its sender refuses such a message -- tests/test_encoding_edges_gpu.py.)"""
    m = _calc_meta(amax)
    L = P.layout_reference(m)
    assert L["w"][2:4] == [w, w] and L["vb"] == vb
    assert P.reply_bits_reference(m) == E.multiply_reply_bits(amax, amax) == E.multiply_reply_bits(-amax, amax)
    lo, hi = -(1 << (w - 1)), (1 << (w - 1)) - 1  # the widest values the fields hold
    assert E.fits(lo, w) and E.fits(hi, w) and not E.fits(lo - 1, w) and not E.fits(hi + 1, w)
    worst = max(E.bit_len(E.zz(x * y)) for x in (lo, hi) for y in (lo, hi))
    assert worst == worst_bits
    assert (worst <= 8 * vb) == (amax == 64)
    # the per-message bound never understates the product it admits
    for x in (lo, hi, amax, -amax):
        for y in (lo, hi, amax, -amax):
            assert E.bit_len(E.zz(x * y)) <= E.multiply_reply_bits(x, y)
            if max(abs(x), abs(y)) <= amax:
                assert E.multiply_reply_bits(x, y) <= 8 * vb


def test_sorted_exchange_argument_caps_model():
    """The sender's admission caps: at least the agreed maxima, at most the fields, and
    whatever pair they admit keeps the Multiply bound within the reply plane -- while
    one step past either cap (where the field allows it) does not."""
    for amax, w, vb, _ in LAGGED_REPLY_CASES:
        z = max(E.zz(amax), E.zz(-amax))
        c0, c1 = E.sx_arg_caps([0, 13, w, w, 0], vb, z, z)
        f = (1 << w) - 1
        assert z <= c0 <= f and z <= c1 <= f
        assert E.multiply_reply_bits(E.unzz(c0), E.unzz(c1)) <= 8 * vb
        assert (c0, c1) == (f, f) if amax == 64 else (c0 < f or c1 < f)
        mag = lambda c: c // 2 + (c & 1)  # noqa: E731
        if c1 < f:  # maximal: one more in magnitude on a1 breaks the bound 2 |a0| |a1| < 2^(8 vb)
            assert 2 * mag(c0) * (mag(c1) + 1) >= 1 << (8 * vb)
        if c0 < f:  # (a0 was raised first, against the agreed a1)
            assert 2 * (mag(c0) + 1) * mag(z) >= 1 << (8 * vb)
        for x in (c0, c0 - 1, 0):
            for y in (c1, c1 - 1, 0):
                assert E.bit_len(E.zz(E.unzz(x) * E.unzz(y))) <= 8 * vb
    assert E.sx_arg_caps([0, 13, 5, 5, 0], 1, 16, 16) == (30, 16)
    # the headline's 16 + 17-bit layout (A in [-2^15, 2^15), B in [0, 2^16)): nothing it sends is refused
    assert E.sx_arg_caps([0, 17, 16, 17, 0], 4, 65535, 131070) == (65535, 131070)
    # an agreement that saw no Multiply: from zero -- a0's whole field, a1 what the bound leaves
    assert E.sx_arg_caps([0, 13, 8, 8, 0], 2, 255, 255, saw_multiply=False) == (255, 255)
    assert E.sx_arg_caps([0, 13, 9, 9, 0], 2, 0, 0, saw_multiply=False) == (511, 254)
    assert E.sx_arg_caps([0, 13, 40, 40, 0], 8, 5, 5) == ((1 << 40) - 1, (1 << 40) - 1)


@pytest.mark.parametrize("bits,want", [
    ((13, 17, 17), (13, 19, 20, False)),
    ((13, 20, 19), (13, 20, 19, False)),  # the sum is exactly 52
    ((13, 20, 20), (13, 19, 20, True)),
    ((24, 14, 14), (24, 14, 14, False)),
    ((24, 15, 14), (24, 14, 14, True)),
    ((0, 0, 0), (1, 25, 26, False)),
    ((13, 64, 1), (13, 19, 20, True)),
    ((25, 1, 1), (24, 14, 14, True)),  # a mailbox field past 24 bits
])
def test_rec8_width_rule(bits, want):
    got = E.rec8_next(*bits)
    assert got == want
    assert sum(got[:3]) == E.REC8_PAYLOAD and min(got[:3]) >= 1
    if not got[3]:  # kept: every field at least as wide as what was seen
        assert got[0] >= bits[0] and got[1] >= bits[1] and got[2] >= bits[2]


def test_rec8_width_rule_brute_force():
    for bm in range(0, 33):
        for b0 in range(0, 65, 3):
            for b1 in range(0, 65):
                wm, w0, w1, wide = E.rec8_next(bm, b0, b1)
                assert wm + w0 + w1 == 52
                need = max(bm, 1) + max(b0, 1) + max(b1, 1)
                assert wide == (bm > 24 or need > 52)
                if not wide:
                    assert wm == max(bm, 1) and w0 >= b0 and w1 >= b1 and 0 <= (w1 - max(b1, 1)) - (w0 - max(b0, 1)) <= 1


@pytest.mark.parametrize("n_state,n_dir,want", [
    (0, 0, (20, 16, 16)), (1, 0, (20, 16, 16)), (2, 0, (1, 25, 26)), (1000, 0, (10, 21, 21)),
    (0, 8192, (13, 19, 20)), (8193, 4096, (14, 19, 19)), (1 << 24, 0, (24, 14, 14)), (0, (1 << 24) + 1, (24, 14, 14)),
])
def test_rec8_first_send_widths(n_state, n_dir, want):
    assert E.rec8_first(n_state, n_dir) == want


def test_edge_positions_and_place():
    M = 2 * E.TILE + 1
    assert E.edge_positions(M, 6) == [0, 63, 64, 4095, 4096, M - 1]
    pos = E.edge_positions(M, 40)
    assert len(set(pos)) == 40 and all(0 <= p < M for p in pos)
    assert E.edge_positions(1, 1) == [0]
    assert E.edge_positions(2049, 6, tile=E.SMALL_TILE) == [0, 63, 64, 1023, 1024, 2048]
    edges = E.pairs(E.edge_values(20), [3]) + [(7, E.INT64_MIN, E.INT64_MAX)]
    actor, a0, a1, pos = E.place(M, edges, 64, seed=1)
    assert actor.shape == (M,) and int(actor.max()) < 64
    for p, (x, v0, v1) in zip(pos, edges):
        assert int(a0[p]) == v0 and int(a1[p]) == v1 and (x is None or int(actor[p]) == x)
    rest = np.setdiff1d(np.arange(M), np.array(pos))
    assert int(a0[rest].abs().max()) < 100 and int(a1[rest].abs().max()) < 100


def _boundary_metas():
    """Metas whose argument maxima sit at 2^k - 1, 2^k and 2^64 - 1 for k around every
    8 / 16 / 32-bit reply boundary of Multiply (2 |a| |b|), Echo (a0) and PrimeCheck."""
    zs = {2**64 - 1, 2**64 - 2, 0, 1}
    for k in (3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63):
        zs |= {2**k - 1, 2**k}
    zs = sorted(zs)
    for meth in (METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_PRIME_CHECK):
        for z0 in zs:
            for z1 in (zs if meth != METHOD_ECHO else [0, 255]):
                m = [0] * P.META_WORDS
                m[P.META_ARG0], m[P.META_ARG0 + 1] = z0, z1
                m[P.META_ARG0 + 2] = z1 if meth == METHOD_PRIME_CHECK else 0
                m[P.META_FLAGS + meth] = 1
                m[P.META_METHOD] = meth
                yield m


def test_reply_bits_reference_at_the_byte_boundaries():
    """The reference rule itself against big-int arithmetic at the boundaries."""
    vb_of = lambda bits: 1 if bits <= 8 else 2 if bits <= 16 else 4 if bits <= 32 else 8  # noqa: E731
    steps = set()
    for m in _boundary_metas():
        z0, z1 = m[P.META_ARG0], m[P.META_ARG0 + 1]
        mag = lambda z: (z + 1) // 2  # noqa: E731
        if m[P.META_FLAGS + METHOD_CALC_MULTIPLY]:
            want = min(64, (2 * mag(z0) * mag(z1)).bit_length())
        elif m[P.META_FLAGS + METHOD_ECHO]:
            want = z0.bit_length()
        else:
            want = min(64, (max(z0, z1) + 1).bit_length())
        want = max(8, want)
        assert P.reply_bits_reference(m) == want, m
        assert P.layout_reference(m)["vb"] == vb_of(want)
        steps.add(vb_of(want))
    assert steps == {1, 2, 4, 8}
    # Echo's reply byte count steps exactly where its argument's zigzag passes a byte boundary
    for b, (below, above) in {8: (1, 2), 16: (2, 4), 32: (4, 8)}.items():
        for z, vb in ((2**b - 1, below), (2**b, above)):
            m = [0] * P.META_WORDS
            m[P.META_ARG0], m[P.META_FLAGS + METHOD_ECHO] = z, 1
            assert P.layout_reference(m)["vb"] == vb, (b, z)


def test_native_layout_matches_reference_at_the_byte_boundaries():
    h = hip()  # (host code of the extension: no GPU needed)
    n = 0
    for m in _boundary_metas():
        assert h.packed_reply_bits(m) == P.reply_bits_reference(m), m
        assert h.packed_layout(m) == P.layout_reference(m), m
        n += 1
    assert n > 1000
    for amax, w, vb, _ in LAGGED_REPLY_CASES:
        L = h.packed_layout(_calc_meta(amax))
        assert L["w"][2:4] == [w, w] and L["vb"] == vb
