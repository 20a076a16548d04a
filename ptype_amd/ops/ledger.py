"""Send ledger: what a rank's Sends carried, kept on the device.

The reference's stdlib ``/debug/rpc`` page lists every method with its number of
calls; a batched Send never passes the host net/rpc server, so here the counts
live in HBM.  A ``Ledger`` owns one block of int64 words (layout:
``csrc/hip/ledger.hpp``, mirrored below; kept in ``COPIES`` copies that spread
the kernel's atomics and are folded on read).  ``account`` folds a Send's final
replies into it with one kernel (``csrc/hip/ledger.hip``) -- no host read, no
allocation, capturable into a hipGraph -- and ``read`` is the only place the
host looks at it (``DeviceRuntime.stats()``):

* ``calls``: messages per (method, status); method ids 0..14 have a slot each,
  every other id is "other"; statuses 0..6 have a slot each, anything else is
  "other"
* ``sends`` / ``messages``
* ``digest_sum`` / ``digest_xor``: the wrapping sum and the xor over all messages of
  ``h(i, v, s) = mix64(mix64(i + 1) ^ uint64(v') ^ (uint64(uint32(s)) * GOLD))``,
  ``i`` the message's index in its Send, ``v'`` the value of an OK reply and 0 for
  any other status: a checksum of every reply of every Send, graph replays
  included
* ``audited`` / ``mismatch``: OK replies of ``Calculator.Multiply`` (``a0 * a1``,
  wrapping) and ``Echo`` (``a0``) recomputed from the batch
* ``load`` (with ``actors > 0``): messages per logical actor id, ``load_oob``
  those addressed past the table

The ledger is the caller's view: a rank accounts the batches it sent.  CPU
tensors run the numpy reference (``account_ref``), which is also what the kernel
is tested against.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _ptr, hip, raw_stream
from .batch import MsgBatch
from .records import METHOD_CALC_MULTIPLY, METHOD_ECHO, METHOD_NAMES, STATUS_NAMES, STATUS_OK
from .table import mix64

# csrc/hip/ledger.hpp (checked against _hip.ledger_words() by the GPU tests)
METHOD_SLOTS, STATUS_SLOTS = 16, 8
W_CALLS = 0
W_MESSAGES = METHOD_SLOTS * STATUS_SLOTS
W_SENDS, W_DIGEST_SUM, W_DIGEST_XOR, W_AUDITED, W_MISMATCH, W_LOAD_OOB = (W_MESSAGES + k for k in range(1, 7))
LEDGER_WORDS = W_MESSAGES + 8
COPIES = 16  # kLedgerCopies: block b of a launch adds to copy b % COPIES, readers fold them
TICKET_WORDS = 65  # common.hpp kTicketWords
GOLD = 0x9E3779B97F4A7C15
_U64 = (1 << 64) - 1


def _i64(x: int) -> int:
    """The int64 with the bit pattern of ``x`` mod 2**64."""
    x &= _U64
    return x - (1 << 64) if x >> 63 else x


def digest(value: torch.Tensor, status: torch.Tensor) -> tuple[int, int]:
    """``(digest_sum, digest_xor)`` of one Send's replies, as unsigned ints."""
    s = status.detach().cpu().to(torch.int32).numpy()
    v = value.detach().cpu().to(torch.int64).numpy().view(np.uint64)
    i = np.arange(1, s.size + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        st = s.view(np.uint32).astype(np.uint64) * np.uint64(GOLD)
        h = mix64(mix64(i) ^ np.where(s == STATUS_OK, v, np.uint64(0)) ^ st)
        return int(h.sum(dtype=np.uint64)), int(np.bitwise_xor.reduce(h, initial=np.uint64(0)))


def _validate(batch: MsgBatch, value: torch.Tensor, status: torch.Tensor) -> None:
    M = batch.M
    if status.dtype != torch.int32 or status.numel() != M:
        raise TypeError("ledger: status must be int32[M]")
    if value.dtype != torch.int64 or value.numel() != M:
        raise TypeError("ledger: value must be int64[M]")
    if batch.actor.dtype != torch.int32 or batch.a0.dtype != torch.int64 or batch.a0.numel() != M:
        raise TypeError("MsgBatch: actor must be int32 and a0..a2 int64")
    if batch.a1 is not None and (batch.a1.dtype != torch.int64 or batch.a1.numel() != M):
        raise TypeError("MsgBatch: actor must be int32 and a0..a2 int64")
    if not isinstance(batch.method, int) and batch.method.numel() != M:
        raise TypeError("MsgBatch: the method column must have M entries")


def account_ref(batch: MsgBatch, value: torch.Tensor, status: torch.Tensor, n_load: int = 0):
    """One Send's contribution, computed on the host: ``(words int64[LEDGER_WORDS],
    load int64[n_load] or None)``.  ``bincount`` for the counts, numpy uint64
    arithmetic for the digest."""
    _validate(batch, value, status)
    M = batch.M
    cpu = (lambda t: t.detach().cpu())
    s = cpu(status).to(torch.int64)
    v = cpu(value)
    if isinstance(batch.method, int):
        m = torch.full((M,), int(batch.method) & 0xFFFF, dtype=torch.int64)
    else:
        m = cpu(batch.method).to(torch.int16).to(torch.int64) & 0xFFFF
    words = torch.zeros(LEDGER_WORDS, dtype=torch.int64)
    ms = torch.where(m < METHOD_SLOTS - 1, m, torch.full_like(m, METHOD_SLOTS - 1))
    ss = torch.where((s >= 0) & (s < STATUS_SLOTS - 1), s, torch.full_like(s, STATUS_SLOTS - 1))
    words[W_CALLS:W_CALLS + W_MESSAGES] = torch.bincount(ms * STATUS_SLOTS + ss, minlength=W_MESSAGES)
    words[W_MESSAGES], words[W_SENDS] = M, 1
    dsum, dxor = digest(v, cpu(status))
    words[W_DIGEST_SUM], words[W_DIGEST_XOR] = _i64(dsum), _i64(dxor)
    a0 = cpu(batch.a0)
    a1 = torch.zeros_like(a0) if batch.a1 is None else cpu(batch.a1)
    ok = s == STATUS_OK
    mul, echo = ok & (m == METHOD_CALC_MULTIPLY), ok & (m == METHOD_ECHO)
    want = torch.where(mul, a0 * a1, a0)  # (int64 products wrap)
    words[W_AUDITED] = int((mul | echo).sum())
    words[W_MISMATCH] = int(((mul | echo) & (want != v)).sum())
    load = None
    if n_load > 0:
        ids = cpu(batch.actor).to(torch.int64) & 0xFFFFFFFF
        inside = ids < n_load
        load = torch.bincount(ids[inside], minlength=n_load)
        words[W_LOAD_OOB] = int((~inside).sum())
    return words, load


class Ledger:
    """The ledger words (and, with ``actors > 0``, the per-actor load table) of one
    rank, on ``device``."""

    def __init__(self, device, actors: int = 0):
        self.device = torch.device(device)
        self.copies = torch.zeros(COPIES, LEDGER_WORDS, dtype=torch.int64, device=self.device)
        self.load = torch.zeros(int(actors), dtype=torch.int64, device=self.device) if actors > 0 else None
        self.ticket = None
        if self.device.type == "cuda":  # last_block_ticket words: zero between launches
            self.ticket = torch.zeros(TICKET_WORDS, dtype=torch.int32, device=self.device)

    def account(self, batch: MsgBatch, value: torch.Tensor, status: torch.Tensor) -> None:
        """Fold one Send -- its batch and its final ``(value int64[M], status
        int32[M])`` -- into the ledger, on the current stream of the tensors'
        device.  No host read and, for contiguous 16-byte aligned columns (what a
        Send returns), no allocation; legal under graph capture."""
        _validate(batch, value, status)
        if status.device != self.copies.device or value.device != self.copies.device:
            raise ValueError("ledger: the replies live on another device than the ledger")
        if self.device.type != "cuda":
            words, load = account_ref(batch, value, status, 0 if self.load is None else self.load.numel())
            mine = self.copies[0]
            dxor = mine[W_DIGEST_XOR] ^ words[W_DIGEST_XOR]
            mine += words  # (int64 adds wrap, as the kernel's do)
            mine[W_DIGEST_XOR] = dxor
            if load is not None:
                self.load += load
            return

        def col(t):  # the kernel reads 16 bytes at a time (a view at an odd offset: copy)
            if t is None:
                return None
            t = t.contiguous()
            return t.clone() if t.data_ptr() % 16 else t

        uniform = isinstance(batch.method, int)
        method = None if uniform else col(batch.method.to(torch.int16))
        status, value, actor, a0, a1 = col(status), col(value), col(batch.actor), col(batch.a0), col(batch.a1)
        hip().ledger_account(_ptr(status), _ptr(value), batch.M, _ptr(actor), _ptr(method),
                             int(batch.method) & 0xFFFF if uniform else 0, _ptr(a0), _ptr(a1), _ptr(self.copies),
                             _ptr(self.load), 0 if self.load is None else self.load.numel(), _ptr(self.ticket),
                             raw_stream(self.device))

    @property
    def words(self) -> torch.Tensor:
        """The ledger words, int64[LEDGER_WORDS] on the host: the copies folded (a
        host read)."""
        c = self.copies.cpu()
        w = c.sum(0)  # (int64 sums wrap)
        w[W_DIGEST_XOR] = int(np.bitwise_xor.reduce(c[:, W_DIGEST_XOR].numpy()))
        return w

    def reset(self) -> None:
        """Zero every counter (asynchronous fills, no synchronisation)."""
        self.copies.zero_()
        if self.load is not None:
            self.load.zero_()

    def read(self, top: int = 8) -> dict:
        """The ledger as a dict (the only host reads): ``sends``, ``messages``,
        ``calls`` as ``{method name: {status name: count}}`` (non-zero entries),
        the digests as unsigned ints, ``audited``, ``mismatch``, ``load_oob`` and
        ``hot``: ``[actor id, count]`` of the ``top`` busiest actors (empty without
        a load table)."""
        w = self.words.tolist()
        calls: dict = {}
        for ms in range(METHOD_SLOTS):
            for ss in range(STATUS_SLOTS):
                n = w[W_CALLS + ms * STATUS_SLOTS + ss]
                if n:
                    mname = "other" if ms == METHOD_SLOTS - 1 else METHOD_NAMES.get(ms, f"method_{ms}")
                    sname = "other" if ss == STATUS_SLOTS - 1 else STATUS_NAMES.get(ss, f"status_{ss}")
                    calls.setdefault(mname, {})[sname] = n
        hot = []
        if self.load is not None and top > 0:
            cnt, ids = torch.topk(self.load, min(int(top), self.load.numel()))
            hot = [[int(i), int(c)] for i, c in zip(ids.tolist(), cnt.tolist()) if c > 0]
        return {"sends": w[W_SENDS], "messages": w[W_MESSAGES], "calls": calls,
                "digest_sum": w[W_DIGEST_SUM] & _U64, "digest_xor": w[W_DIGEST_XOR] & _U64,
                "audited": w[W_AUDITED], "mismatch": w[W_MISMATCH], "load_oob": w[W_LOAD_OOB], "hot": hot}
