"""The registry mirror's specification, written without a hash table.

``Model`` is a dict ``key -> (rank, mbox, deadline)`` plus a tombstone count, a capacity
and a generation: what ``ptype_amd.ops.table.RegistryTable`` must answer on either
device, with no probing, no slots and nothing imported from ``ops/table.py``.  The
directory forms (route words, rank bytes, presence map, affine verdict) and the
per-message resolution are derived from the dict alone.

``scenarios()`` returns the hostile op sequences the registry tests share; ``apply`` and
``run_op`` drive a model and a table through one op.  Keys are signed 64-bit integers
as the tables hold them (actor id + 1, or a 64-bit service hash); ranks and mailboxes
are kept as unsigned 32-bit values and deadlines as given.

Left unspecified on purpose (and never asserted): which of two rows with one key in one
upsert is stored, which of two equal keys in one delete is reported found, the order of
``pack()`` and which slot a key occupies.
"""
from __future__ import annotations

import numpy as np

U32 = 0xFFFFFFFF
NO_FIELD = 0xFFFFFFFF  # the actor field that names no actor
DIR_MISSING, DIR_FALLBACK = 0xFFFFFFFF, 0xFFFFFFFE
RANK_MISSING, RANK_FALLBACK = 0xFF, 0xFE
MAX_MBOX = 1 << 24
PRESENCE_MAX_IDS = 1 << 18


def key_of(actor_id: int) -> int:
    """Table key of an actor id, as int64: id + 1 (0 is the empty slot)."""
    return int(actor_id) + 1


def fnv1a64(s: str) -> int:
    """64-bit FNV-1a of a service node name as a signed table key (0 and ~0 fold to 1)."""
    h = 0xCBF29CE484222325
    for b in s.encode():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    if h in (0, 0xFFFFFFFFFFFFFFFF):
        h = 1
    return h - (1 << 64) if h >= (1 << 63) else h


def _pow2(n: int) -> int:
    c = 1
    while c < n:
        c <<= 1
    return c


def _i32(x):
    return np.asarray(x, dtype=np.uint32).view(np.int32)


class Model:
    def __init__(self, capacity: int):
        self.cap = _pow2(max(16, int(capacity)))
        self.d: dict[int, tuple[int, int, int]] = {}
        self.tombstones = 0
        self.generation = 0

    # ------------------------------------------------------------------ table operations
    @property
    def live(self) -> int:
        return len(self.d)

    def upsert(self, keys, ranks, mboxes, deadlines=None) -> None:
        keys = [int(k) for k in np.asarray(keys, dtype=np.int64).tolist()]
        n = len(keys)
        if self.live + self.tombstones + n > self.cap * 3 // 4:  # counted per input row, before the insert
            self.rebuild(min_capacity=max(self.cap, 2 * (self.live + n)))
        if n == 0:
            return
        ranks = np.asarray(ranks, dtype=np.int64).tolist()
        mboxes = np.asarray(mboxes, dtype=np.int64).tolist()
        dl = [0] * n if deadlines is None else np.asarray(deadlines, dtype=np.int64).tolist()
        for k, r, m, e in zip(keys, ranks, mboxes, dl):
            if k in (0, -1):
                continue
            self.d[k] = (int(r) & U32, int(m) & U32, int(e))
        self.generation += 1

    def delete(self, keys) -> np.ndarray:
        """Found flags; a key given twice is found at its first position here (either is allowed)."""
        keys = np.asarray(keys, dtype=np.int64).tolist()
        found = np.zeros(len(keys), dtype=bool)
        for i, k in enumerate(keys):
            if k not in (0, -1) and k in self.d:
                del self.d[k]
                found[i] = True
        self.tombstones += int(found.sum())
        if len(keys):
            self.generation += 1
        return found

    def sweep(self, now: int) -> None:
        dead = [k for k, v in self.d.items() if v[2] != 0 and v[2] < now]
        for k in dead:
            del self.d[k]
        self.tombstones += len(dead)
        self.generation += 1

    def pack(self):
        """Sorted list of (key, rank, mbox, deadline): the multiset a pack must hold."""
        return sorted((k,) + v for k, v in self.d.items())

    def clear(self) -> None:
        self.d.clear()
        self.tombstones = 0
        self.generation += 1

    def rebuild(self, min_capacity: int | None = None) -> None:
        """Drops the tombstones, keeps every entry; a clear plus a re-insert for the generation."""
        if min_capacity and _pow2(min_capacity) > self.cap:
            self.cap = _pow2(min_capacity)
        self.tombstones = 0
        self.generation += 1
        if self.d:
            self.generation += 1

    def load_packed(self, rows) -> None:
        """``rows``: (key, rank, mbox, deadline) tuples, as ``pack`` returns them."""
        rows = list(rows)
        if not rows:
            return
        k, r, m, e = zip(*rows)
        self.upsert(k, r, m, e)

    # ------------------------------------------------------------------ lookups
    def _arrays(self):
        n = len(self.d)
        keys = np.fromiter(self.d.keys(), dtype=np.int64, count=n)
        vals = np.array(list(self.d.values()), dtype=np.int64).reshape(n, 3)
        return keys, vals

    def _find(self, q: np.ndarray):
        """``(hit bool[n], rank int64[n], mbox int64[n])`` (unsigned values) of int64 keys."""
        n = q.shape[0]
        hit, rank, mbox = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        if not self.d or n == 0:
            return hit, rank, mbox
        k, v = self._arrays()
        order = np.argsort(k)
        k, v = k[order], v[order]
        pos = np.clip(np.searchsorted(k, q), 0, k.shape[0] - 1)
        hit = (k[pos] == q) & (q != 0) & (q != -1)
        rank[hit] = v[pos[hit], 0]
        mbox[hit] = v[pos[hit], 1]
        return hit, rank, mbox

    def lookup(self, keys):
        """``(rank int32[n], mbox int32[n])``, -1 / -1 for a key the table does not hold."""
        hit, r, m = self._find(np.asarray(keys, dtype=np.int64).reshape(-1))
        return np.where(hit, _i32(r), np.int32(-1)), np.where(hit, _i32(m), np.int32(-1))

    def resolve(self, actor_u32: int):
        """``(rank, mbox)`` of a message's 32-bit actor field, or None.  The field
        0xffffffff names no actor, whether or not key 2^32 is registered."""
        a = int(actor_u32) & U32
        if a == NO_FIELD:
            return None
        v = self.d.get(a + 1)
        return None if v is None else (v[0], v[1])

    def resolve_many(self, actors):
        """Vectorised ``resolve``: ``(rank int64[n], mbox int64[n])`` as unsigned values, rank -1 for a miss."""
        a = np.asarray(actors).astype(np.int64).reshape(-1) & U32
        hit, r, m = self._find(a + 1)
        hit &= a != NO_FIELD
        return np.where(hit, r, -1), np.where(hit, m, 0)

    # ------------------------------------------------------------------ directory forms
    def _dir_entries(self, n: int):
        k, v = self._arrays() if self.d else (np.zeros(0, np.int64), np.zeros((0, 3), np.int64))
        sel = (k >= 1) & (k <= n)
        return k[sel] - 1, v[sel, 0], v[sel, 1]

    def dir_words(self, n: int) -> np.ndarray:
        out = np.full(n, DIR_MISSING, dtype=np.uint32)
        ids, r, m = self._dir_entries(n)
        fits = (r < RANK_FALLBACK) & (m < MAX_MBOX)
        out[ids] = np.where(fits, r | (m << 8), DIR_FALLBACK).astype(np.uint32)
        return out

    def rank_bytes(self, n: int) -> np.ndarray:
        out = np.full(n, RANK_MISSING, dtype=np.uint8)
        ids, r, _ = self._dir_entries(n)
        out[ids] = np.where(r < RANK_FALLBACK, r, RANK_FALLBACK).astype(np.uint8)
        return out

    def presence(self, n: int, rank_self: int) -> np.ndarray:
        words = ((n + 15) // 16 + 3) & ~3
        rb = self.rank_bytes(n)
        f = np.zeros(words * 16, dtype=np.uint32)
        f[:n] = np.where(rb == (rank_self & 0xFF), 1, np.where(rb == RANK_FALLBACK, 2, 0))
        shifts = (2 * np.arange(16, dtype=np.uint32))[None, :]
        return (f.reshape(words, 16) << shifts).sum(axis=1, dtype=np.uint64).astype(np.uint32)

    def affine(self, n: int, W: int) -> bool:
        ids, r, m = self._dir_entries(n)
        return ids.shape[0] == n and bool(np.all(r == ids % W)) and bool(np.all(m == ids // W))


# ---------------------------------------------------------------------- ops
# An op is a tuple: ("upsert", keys, ranks, mboxes, deadlines | None), ("delete", keys),
# ("sweep", now), ("clear",), ("rebuild",) or ("upsert_free", key, [(rank, mbox), ...]):
# one upsert holding `key` once per candidate; the table may keep any of them.
def apply(model: Model, op, chosen=None):
    """Run `op` on the model; returns the found flags of a delete.  `chosen`: the
    candidate an ``upsert_free`` kept on the table under test."""
    kind = op[0]
    if kind == "upsert":
        return model.upsert(*op[1:])
    if kind == "delete":
        return model.delete(op[1])
    if kind == "sweep":
        return model.sweep(op[1])
    if kind == "clear":
        return model.clear()
    if kind == "rebuild":
        return model.rebuild()
    if kind == "upsert_free":
        n = len(op[2])
        rows = [chosen] * n  # n rows enter the growth check; the value is the one observed
        return model.upsert([op[1]] * n, [r[0] for r in rows], [r[1] for r in rows])
    raise ValueError(kind)


def drive(table, model: Model, op) -> None:
    """Run `op` on a RegistryTable (either device) and on the model, and check what the
    call itself answers: the found flags of a delete, per distinct key."""
    import torch

    kind = op[0]
    i64 = lambda x: torch.tensor(list(x), dtype=torch.int64)
    i32 = lambda x: torch.tensor(list(x), dtype=torch.int64).to(torch.int32)
    if kind == "upsert":
        _, k, r, m, e = op
        table.upsert(i64(k), i32(r), i32(m), None if e is None else i64(e))
        apply(model, op)
    elif kind == "delete":
        found = table.delete(i64(op[1])).cpu().numpy().astype(bool)
        want = apply(model, op)
        keys = np.asarray(op[1], dtype=np.int64).reshape(-1)
        for k in set(keys.tolist()):  # a repeated key: found exactly once, at either position
            assert int(found[keys == k].sum()) == int(want[keys == k].sum()), (k, found, want)
    elif kind == "sweep":
        table.sweep(op[1])
        apply(model, op)
    elif kind == "clear":
        table.clear()
        apply(model, op)
    elif kind == "rebuild":
        table.rebuild()
        apply(model, op)
    elif kind == "upsert_free":
        _, key, cands = op
        table.upsert(i64([key] * len(cands)), i32(c[0] for c in cands), i32(c[1] for c in cands))
        r, m = table.lookup(i64([key]))
        chosen = (int(r[0]) & U32, int(m[0]) & U32)
        assert chosen in [(c[0] & U32, c[1] & U32) for c in cands], (chosen, cands)
        apply(model, op, chosen)
    else:
        raise ValueError(kind)


def op_keys(op):
    kind = op[0]
    if kind in ("upsert", "delete"):
        return [int(k) for k in np.asarray(op[1], dtype=np.int64).tolist()]
    if kind == "upsert_free":
        return [int(op[1])]
    return []


# The 12 lowest actor ids whose probe start (splitmix64 finalizer of id + 1, masked to a
# 64-slot table, rounded down to its group of 4) is slot 60: a chain that wraps to slot 0.
WRAP_IDS = [11, 15, 16, 26, 33, 34, 60, 69, 90, 104, 112, 117]
NOW = 1000


def _ids(ids):
    return [key_of(i) for i in ids]


def _wrap_ops():
    n = len(WRAP_IDS)
    return [("upsert", _ids(WRAP_IDS), [i % 3 for i in range(n)], [100 + i for i in range(n)],
             [100 * (i + 1) for i in range(n)])]


def service_keys():
    """Two service node keys with the top bit set (negative as int64)."""
    out = []
    i = 0
    while len(out) < 2:
        k = fnv1a64(f"calculator/node{i}")
        if k < 0:
            out.append(k)
        i += 1
    return out


VALUE_RANKS = [0, 1, 0xFD, 0xFE, 0xFF, 300, (1 << 31) - 1]
VALUE_MBOXES = [0, (1 << 24) - 1, 1 << 24, (1 << 31) - 1]


def scenarios() -> dict:
    """name -> {"cap": initial capacity, "ops": [...], "absent": keys never registered}."""
    s = {}
    s["wrap"] = {"cap": 64, "ops": _wrap_ops(), "absent": _ids([0, 1, 12, 118, 5000])}
    w4, w8 = key_of(WRAP_IDS[3]), key_of(WRAP_IDS[7])
    s["tombs"] = {"cap": 64, "absent": _ids([0, 1, 12, 118, 5000]), "ops": _wrap_ops() + [
        ("delete", [w4, w8]),
        ("upsert", [w4], [2], [777], None),
        ("sweep", 500),  # deadlines 100, 200, 300 go; 400 was re-upserted without one; 500 == now stays
    ]}
    s["threshold"] = {"cap": 16, "absent": _ids([13, 14, 99]), "ops": [
        ("upsert", _ids(range(12)), [0] * 12, list(range(12)), None),
        ("upsert", _ids([12]), [1], [12], None),
    ]}
    vr = [r for r in VALUE_RANKS for _ in VALUE_MBOXES]
    vm = [m for _ in VALUE_RANKS for m in VALUE_MBOXES]
    s["values"] = {"cap": 64, "absent": _ids([28, 29, 1000]),
                   "ops": [("upsert", _ids(range(len(vr))), vr, vm, None)]}
    sk = service_keys()
    keys = [key_of(0), 0, key_of(U32 - 1), -1, key_of(U32)] + sk + [-2]
    s["keys"] = {"cap": 16, "absent": [key_of(1), key_of(U32 - 2), -3, sk[0] + 1, (1 << 62)], "ops": [
        ("upsert", keys, [0, 9, 0, 9, 0, 1, 0, 1], [5, 9, 6, 9, 7, 8, 9, 10], None),
        ("delete", [0, -1, key_of(7)]),
    ]}
    s["deadlines"] = {"cap": 16, "absent": _ids([20, 21]), "ops": [
        ("upsert", _ids(range(7)), [0] * 7, list(range(7)), [0, NOW - 1, NOW, NOW + 1, NOW - 1, NOW - 500, NOW - 1]),
        ("upsert", _ids([4]), [0], [44], [NOW + 1000]),  # extended before the sweep
        ("upsert", _ids([6]), [0], [66], None),  # no deadline column: the deadline becomes 0
        ("sweep", NOW),  # ids 1 and 5 go
        ("upsert", _ids([5]), [1], [55], [NOW + 5]),  # a swept key comes back
        ("sweep", NOW + 1),  # 2 (deadline == NOW) goes now, 3 (== NOW + 1) stays
    ]}
    s["dups"] = {"cap": 16, "absent": _ids([30, 31]), "ops": [
        ("upsert", _ids(range(6)), [0] * 6, list(range(6)), None),
        ("delete", _ids([2, 2])),
        ("upsert", _ids([7, 7]), [1, 1], [70, 70], None),
        ("upsert_free", key_of(8), [(0, 80), (1, 81)]),
        ("delete", _ids([8, 3, 8, 30])),
    ]}
    return s


FULL_KEYS = _ids(range(40, 60))  # 20 distinct keys for a capacity-16 table


def random_ops(seed: int, n_ops: int = 120, universe: int = 80):
    """A fixed-seed mix of ops over ``universe`` actor ids and two service keys; no key
    appears twice in one upsert (that outcome is unspecified), deletes may repeat one."""
    rng = np.random.default_rng(seed)
    pool = np.array(_ids(range(universe)) + service_keys() + [0, -1], dtype=np.int64)
    ops, now = [], 100
    for _ in range(n_ops):
        x = rng.random()
        if x < 0.5:
            k = rng.choice(pool, size=int(rng.integers(0, 9)), replace=False)
            dl = None if rng.random() < 0.4 else rng.integers(0, 3, k.shape[0]) * (now + rng.integers(-40, 60))
            ops.append(("upsert", k.tolist(), rng.integers(0, 4, k.shape[0]).tolist(),
                        rng.integers(0, 1 << 20, k.shape[0]).tolist(), None if dl is None else dl.tolist()))
        elif x < 0.8:
            ops.append(("delete", rng.choice(pool, size=int(rng.integers(0, 7)), replace=True).tolist()))
        elif x < 0.93:
            now += int(rng.integers(0, 30))
            ops.append(("sweep", now))
        elif x < 0.98:
            ops.append(("rebuild",))
        else:
            ops.append(("clear",))
    return ops, pool.tolist()
