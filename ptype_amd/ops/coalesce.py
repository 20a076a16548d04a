"""Send coalescing (``DeviceRuntime.send(coalesce=True)``): duplicate calls of a
pure method in one batch are sent once.

Go service authors reach for ``singleflight`` when many callers ask the same
pure question at the same time: the question is executed once and every caller
gets that answer.  On the batch path the same is done per Send.  A message's key
is ``(actor id as the caller wrote it, method, a0, a1, a2)`` (a missing ``a1`` /
``a2`` column counts as 0, actor ids compare as uint32); messages of a method in
``records.PURE_METHODS`` with equal keys form a group whose *leader* is the
message with the lowest index, and a message of any other method is its own
leader.  Three steps (``csrc/hip/coalesce.hip``):

* ``group``: ``lead int32[M]``, every message's leader
* ``select``: the stable compaction of the leaders -- the sub-batch of K rows,
  ``idx int32[K]`` ascending and ``pos int32[M]`` with ``pos[idx[j]] = j`` (-1 for
  a follower); the host learns K by one 4-byte read
* ``fanout``: ``val[i] = v2[pos[lead[i]]]``, ``st[i] = s2[pos[lead[i]]]``

CUDA tensors run the kernels; CPU tensors run the host references (``group_ref``
and torch indexing), which are also what the kernels are tested against.
``key_hash`` is the numpy mirror of the device hash (``coalesce.hpp``): the tests
build probe chains with it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _ptr, hip, raw_stream
from .batch import MsgBatch
from .records import PURE_METHODS
from .retry import _aligned, _cols, _compact
from .table import mix64

MIN_LOG2, MAX_LOG2 = 4, 31  # coalesce.hpp kCoalesceMinLog2 / kCoalesceMaxLog2


def table_log2_for(M: int) -> int:
    """log2 of the smallest grouping table for M messages: a power of two of at
    least 2 M slots."""
    return max(MIN_LOG2, (2 * max(int(M), 1) - 1).bit_length())


def _key_columns(batch: MsgBatch):
    """The five key fields as numpy arrays: actor uint32, method uint16, a0..a2 int64."""
    M = batch.M
    cpu = (lambda t: t.detach().cpu())
    actor = cpu(batch.actor).to(torch.int32).numpy().view(np.uint32)
    if isinstance(batch.method, int):
        method = np.full(M, int(batch.method) & 0xFFFF, dtype=np.uint16)
    else:
        method = cpu(batch.method).to(torch.int16).numpy().view(np.uint16)
    z = np.zeros(M, dtype=np.int64)
    arg = (lambda t: z if t is None else cpu(t).to(torch.int64).numpy())
    return actor, method, arg(batch.a0), arg(batch.a1), arg(batch.a2)


def key_hash(actor, method, a0, a1=0, a2=0) -> np.ndarray:
    """The device's key hash (``coalesce_hash``), bit for bit, as uint64: the home
    slot of a key in a table of ``1 << n`` slots is ``key_hash(...) & ((1 << n) - 1)``."""
    u64 = (lambda x: np.asarray(x).astype(np.int64).view(np.uint64))
    k0 = (u64(actor) & np.uint64(0xFFFFFFFF)) | ((u64(method) & np.uint64(0xFFFF)) << np.uint64(32))
    h = mix64(k0)
    for x in (a0, a1, a2):
        h = mix64(h ^ u64(x))
    return h


def group_ref(batch: MsgBatch) -> torch.Tensor:
    """``lead int32[M]`` on the host: the first occurrence of every pure message's
    key (a stable lexicographic sort of the key columns), ``i`` for any other."""
    M = batch.M
    lead = np.arange(M, dtype=np.int64)
    if M:
        actor, method, a0, a1, a2 = _key_columns(batch)
        order = np.lexsort((a2, a1, a0, method, actor))  # stable: equal keys stay in index order
        new = np.ones(M, dtype=bool)
        for c in (actor, method, a0, a1, a2):
            s = c[order]
            new[1:] &= s[1:] == s[:-1]
        new[1:] = ~new[1:]
        first = order[np.flatnonzero(new)]  # every run's lowest index
        lead[order] = first[np.cumsum(new) - 1]
        pure = np.isin(method, np.array(sorted(PURE_METHODS), dtype=np.uint16))
        lead = np.where(pure, lead, np.arange(M, dtype=np.int64))
    return torch.from_numpy(lead.astype(np.int32))


class Coalescer:
    """The grouping workspace of one rank on ``device``: a table of u32 slots sized
    for ``max_batch`` messages (it grows for a larger batch).  Each ``group`` clears
    the part it uses with an asynchronous fill -- no host wait between Sends."""

    def __init__(self, device, max_batch: int = 1 << 20):
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        self.table = None  # allocated by the first group() on a GPU
        # host counters (K is on the host anyway): coalesced Sends, their messages, the leaders sent
        self.counters = {"sends": 0, "messages": 0, "executed": 0}

    def send(self, batch: MsgBatch, send):
        """One coalesced Send: group ``batch``, select the leaders, ``send(sub)`` them
        -- ``send`` takes a MsgBatch and returns ``(value, status, ...)``, final on
        return, and is called exactly once whatever K is -- and fan the replies out.
        A batch without duplicates (K == M) is handed to ``send`` as it is and its
        result returned unchanged.  Returns ``(result, fanned)``: ``fanned`` says
        whether the replies are fan-out copies (new tensors) or ``send``'s own."""
        lead = group(batch, self)
        sub, _, pos, K = select(batch, lead)
        c = self.counters
        c["sends"] += 1
        c["messages"] += batch.M
        c["executed"] += K
        if K == batch.M:
            return send(batch), False
        out = send(sub)
        return fanout(lead, pos, out[0], out[1]) + tuple(out[2:]), True

    def workspace(self, log2: int) -> torch.Tensor:
        if not MIN_LOG2 <= log2 <= MAX_LOG2:
            raise ValueError(f"coalesce: table_log2 must be in [{MIN_LOG2}, {MAX_LOG2}]")
        want = 1 << max(log2, table_log2_for(self.max_batch))
        if self.table is None or self.table.numel() < want:
            self.table = torch.empty(want, dtype=torch.int32, device=self.device)
        return self.table


def group(batch: MsgBatch, coalescer: Coalescer | None = None, table_log2: int | None = None) -> torch.Tensor:
    """``lead int32[M]``: for a pure message the lowest ``j`` whose key equals message
    ``i``'s, ``i`` for any other.  ``table_log2`` forces the table's size (at least
    2 M slots; the tests build long probe chains in a small one)."""
    M = batch.M
    dev = batch.actor.device
    if dev.type != "cuda":
        return group_ref(batch)
    actor, a0, a1, a2, method, uniform = _cols(batch)
    lead = torch.empty(M, dtype=torch.int32, device=dev)
    if M == 0:
        return lead
    log2 = table_log2_for(M) if table_log2 is None else int(table_log2)
    if M > 1 << (log2 - 1):
        raise ValueError("coalesce: the table must have at least 2 M slots")
    table = (coalescer or Coalescer(dev, M)).workspace(log2)
    hip().coalesce_group(_ptr(actor), _ptr(method), int(batch.method) & 0xFFFF if uniform else 0, _ptr(a0), _ptr(a1),
                         _ptr(a2), M, _ptr(table), log2, _ptr(lead), raw_stream(dev))
    return lead


def select(batch: MsgBatch, lead: torch.Tensor):
    """The leaders of ``batch`` (``lead[i] == i``): ``(sub, idx, pos, K)`` with ``idx``
    int32[K] ascending, ``sub`` the K gathered rows of every column and ``pos``
    int32[M], ``pos[idx[j]] = j`` and -1 for a follower.  On a GPU ``sub`` and ``idx``
    are views of M-row buffers, since K is known only after the kernels ran."""
    M = batch.M
    if lead.dtype != torch.int32 or lead.numel() != M:
        raise TypeError("select: lead must be int32[M]")
    if lead.device.type != "cuda":
        idx = torch.nonzero(lead.to(torch.int64) == torch.arange(M)).flatten()
        K = int(idx.numel())
        pos = torch.full((M,), -1, dtype=torch.int32)
        pos[idx] = torch.arange(K, dtype=torch.int32)
        return batch.index_select(idx), idx.to(torch.int32), pos, K
    return _compact(batch, lead, None)


def fanout(lead: torch.Tensor, pos: torch.Tensor, v2: torch.Tensor, s2: torch.Tensor):
    """``(val int64[M], st int32[M])`` with ``val[i] = v2[pos[lead[i]]]`` and
    ``st[i] = s2[pos[lead[i]]]``: every member of a group gets its leader's reply."""
    M, K = lead.numel(), v2.numel()
    if pos.numel() != M or s2.numel() != K:
        raise ValueError("fanout: lead / pos have M entries, v2 / s2 K")
    dev = lead.device
    if dev.type != "cuda":
        p = pos.to(torch.int64)[lead.to(torch.int64)]
        return v2[p], s2[p]
    if (lead.dtype != torch.int32 or pos.dtype != torch.int32 or v2.dtype != torch.int64
            or s2.dtype != torch.int32):
        raise TypeError("fanout: lead / pos / s2 int32, v2 int64")
    val = torch.empty(M, dtype=torch.int64, device=dev)
    st = torch.empty(M, dtype=torch.int32, device=dev)
    if M:
        lead, pos, v2, s2 = _aligned(lead), pos.contiguous(), v2.contiguous(), s2.contiguous()
        hip().coalesce_fanout(_ptr(val), _ptr(st), M, _ptr(lead), _ptr(pos), _ptr(v2), _ptr(s2), K, raw_stream(dev))
    return val, st
