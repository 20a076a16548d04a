"""Retry selection of a batched Send (``ActorExchange.send_all(retries=...)``).

The reference client retries a failed call up to ``Retries`` times, each attempt
on a re-selected connection (cluster/rpc.go:59-116, ``withRetry`` around
``c.conns.Get()``).  On the batch path the failed messages of a Send are picked
out of the batch on the device (``select``: a stable compaction by status, see
``csrc/hip/compact.hpp``), sent again as a sub-batch, and their replies put back
into the caller's outputs (``merge``).

CUDA tensors run the kernels; the host learns K, the number of selected
messages, by one 4-byte read.  CPU tensors run the torch reference
(``nonzero`` + ``index_select``), which is also what the kernels are tested
against.
"""
from __future__ import annotations

import torch

from . import _ptr, hip, raw_stream
from .batch import MsgBatch
from .records import (ORDERED_METHODS, PENDING, STATUS_FAILED, STATUS_NO_ACTOR, STATUS_NO_METHOD, STATUS_NOT_DELIVERED,
                      STATUS_OVERFLOW, STATUS_RANK_LOST, method_ordered)

RETRYABLE = frozenset({STATUS_FAILED, STATUS_NOT_DELIVERED, STATUS_NO_ACTOR, STATUS_NO_METHOD})
DEFAULT_RETRY_ON = (STATUS_FAILED,)


def retry_mask(retry_on=DEFAULT_RETRY_ON) -> int:
    """The 32-bit mask of ``retry_on`` (bit s set: status s is retried), validated:
    STATUS_OVERFLOW belongs to the re-send rounds and STATUS_RANK_LOST to the
    elastic path, and a successful message is never run again."""
    if isinstance(retry_on, int):
        retry_on = (retry_on,)
    codes = [int(s) for s in retry_on]
    if not codes:
        raise ValueError("retry_on: at least one status")
    mask = 0
    for s in codes:
        if s in (STATUS_OVERFLOW, STATUS_RANK_LOST):
            raise ValueError(f"retry_on: status {s} is not retried here (STATUS_OVERFLOW is re-sent by send_all's "
                             "rounds, STATUS_RANK_LOST by the elastic Send)")
        if s not in RETRYABLE:
            raise ValueError(f"retry_on: status {s} is not retryable (STATUS_FAILED, STATUS_NOT_DELIVERED, "
                             "STATUS_NO_ACTOR, STATUS_NO_METHOD)")
        mask |= 1 << s
    return mask


def carries_ordered(batch: MsgBatch) -> bool:
    """Whether ``batch`` carries an ordered method: the uniform method, or any
    entry of its method column (one host read on a GPU: only a Send with retries
    asks)."""
    if isinstance(batch.method, int):
        return method_ordered(batch.method)
    m = batch.method
    hit = torch.zeros((), dtype=torch.bool, device=m.device)
    for o in ORDERED_METHODS:
        hit = hit | (m == o).any()
    return bool(hit)


def _selected(status: torch.Tensor, mask: int) -> torch.Tensor:
    s = status.to(torch.int64)
    bit = torch.bitwise_right_shift(torch.full_like(s, mask), s.clamp(0, 31)) & 1
    return (s >= 0) & (s < 32) & (bit != 0)


def select(batch: MsgBatch, status: torch.Tensor, retry_on=DEFAULT_RETRY_ON):
    """The messages of ``batch`` whose ``status`` (int32[M]) is in ``retry_on``:
    ``(sub, idx, K)`` with ``idx`` int32[K] their indices in ascending order (what
    ``torch.nonzero`` returns) and ``sub`` the K gathered rows of every column.
    On a GPU the outputs are views of M-row buffers, since K is known only after
    the kernels ran."""
    return select_mask(batch, status, retry_mask(retry_on))


TILE = 4096  # rows per block of the compaction (compact.hpp kCompactTile, ``hip().retry_tile()``)


def _cols(batch: MsgBatch):
    M = batch.M
    if batch.actor.dtype != torch.int32 or batch.a0.dtype != torch.int64:
        raise TypeError("MsgBatch: actor must be int32 and a0..a2 int64")
    for t in (batch.a0, batch.a1, batch.a2):
        if t is not None and (t.dtype != torch.int64 or t.numel() != M):
            raise TypeError("MsgBatch: actor must be int32 and a0..a2 int64")
    c = (lambda t: None if t is None else t.contiguous())  # (a view at an odd offset stays naturally aligned)
    uniform = isinstance(batch.method, int)
    if not uniform and batch.method.numel() != M:
        raise TypeError("MsgBatch: the method column must have M entries")
    method = None if uniform else batch.method.to(torch.int16).contiguous()
    return c(batch.actor), c(batch.a0), c(batch.a1), c(batch.a2), method, uniform


def _aligned(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()  # the kernels read 16 bytes at a time (a view at an odd offset: copy)
    return t.clone() if t.data_ptr() % 16 else t


def _compact(batch: MsgBatch, key: torch.Tensor, mask: int | None):
    """The stable compaction on a GPU (``csrc/hip/compact.hpp``): the rows of ``batch``
    whose ``key`` (int32[M]) is a status in ``mask`` or, with ``mask`` None, the row's own
    index.  ``(sub, idx, pos, K)``: ``sub`` and ``idx`` are views of M-row buffers, since K
    is known only after the kernels ran; ``pos`` int32[M] (the row's place in ``sub``, or
    -1) only without a mask, else None."""
    M, dev = batch.M, key.device
    actor, a0, a1, a2, method, uniform = _cols(batch)
    new = (lambda t: None if t is None else torch.empty(M, dtype=t.dtype, device=dev))
    pos = torch.empty(M, dtype=torch.int32, device=dev) if mask is None else None
    idx = torch.empty(M, dtype=torch.int32, device=dev)
    o_actor, o_a0, o_a1, o_a2, o_m = new(actor), new(a0), new(a1), new(a2), new(method)
    K = 0
    if M:
        key = _aligned(key)
        counts = torch.empty((M + TILE - 1) // TILE, dtype=torch.int32, device=dev)
        k = torch.empty(1, dtype=torch.int32, device=dev)
        cols = (_ptr(actor), _ptr(a0), _ptr(a1), _ptr(a2), _ptr(method), _ptr(idx))
        outs = (_ptr(o_actor), _ptr(o_a0), _ptr(o_a1), _ptr(o_a2), _ptr(o_m), _ptr(counts), _ptr(k), raw_stream(dev))
        if mask is None:
            hip().coalesce_select(_ptr(key), M, *cols, _ptr(pos), *outs)
        else:
            hip().retry_select(_ptr(key), M, mask, *cols, *outs)
        K = int(k.item())  # the one host read
    n = (lambda t: None if t is None else t[:K])
    return MsgBatch(o_actor[:K], o_a0[:K], n(o_a1), n(o_a2), batch.method if uniform else o_m[:K]), idx[:K], pos, K


def select_mask(batch: MsgBatch, status: torch.Tensor, mask: int):
    """``select`` by a raw 32-bit mask (bit s set: status s is selected), unvalidated:
    the Send wrappers compact their rows by a marker status of their own
    (``send_pending``)."""
    if status.dtype != torch.int32 or status.numel() != batch.M:
        raise TypeError("select: status must be int32[M]")
    if status.device.type != "cuda":
        idx = torch.nonzero(_selected(status, mask)).flatten()
        return batch.index_select(idx), idx.to(torch.int32), int(idx.numel())
    sub, idx, _, K = _compact(batch, status, mask)
    return sub, idx, K


def send_pending(batch: MsgBatch, val: torch.Tensor, st: torch.Tensor, send, collective: bool, count, after=None):
    """The Send of a wrapper that answered some rows itself (reply cache, breaker,
    limiter): ``(val, st)`` are the batch's outputs so far, with ``st[i] == PENDING`` on
    the rows that still travel.  Those are compacted (stably, in message order),
    ``count(M - K, K)`` tells the wrapper how many were held back and how many go on,
    then ``send(sub)`` -- it takes a MsgBatch and returns ``(value, status, ...)``, final
    on return -- ``after(sub, out)``, and the replies are merged into ``(val, st)``.
    ``send`` is called at most once: exactly once when ``collective`` (a rank with
    nothing to send joins with an empty batch), not at all for K == 0 otherwise.  With
    K == M the batch itself is sent, and ``send``'s result returned unchanged."""
    M = batch.M
    sub, idx, K = select_mask(batch, st, 1 << PENDING)
    count(M - K, K)
    if K == 0 and not collective:
        return val, st
    out = send(batch if K == M else sub)
    if after is not None:
        after(batch if K == M else sub, out)
    if K == M:
        return out
    merge(val, st, idx, out[0], out[1])
    return (val, st) + tuple(out[2:])


def merge(val: torch.Tensor, st: torch.Tensor, idx: torch.Tensor, v2: torch.Tensor, s2: torch.Tensor) -> None:
    """``val[idx[j]] = v2[j]; st[idx[j]] = s2[j]``: a sub-batch's replies back into
    the batch's outputs (in place)."""
    K = idx.numel()
    if v2.numel() != K or s2.numel() != K:
        raise ValueError("merge: idx, v2 and s2 must have the same length")
    if val.device.type != "cuda":
        i = idx.to(torch.int64)
        val[i] = v2
        st[i] = s2
        return
    if (val.dtype != torch.int64 or v2.dtype != torch.int64 or st.dtype != torch.int32 or s2.dtype != torch.int32
            or idx.dtype != torch.int32):
        raise TypeError("merge: val / v2 int64, st / s2 / idx int32")
    if not (val.is_contiguous() and st.is_contiguous()) or val.numel() != st.numel():
        raise ValueError("merge: val and st must be contiguous and of one length")
    if K == 0:
        return
    idx, v2, s2 = idx.contiguous(), v2.contiguous(), s2.contiguous()
    hip().retry_merge(_ptr(val), _ptr(st), val.numel(), _ptr(idx), _ptr(v2), _ptr(s2), K, raw_stream(val.device))
