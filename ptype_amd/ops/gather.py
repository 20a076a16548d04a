"""Reply gather: the M replies of one Send folded into G groups, on the device.

The reference's headline example is a scatter-gather: the optimus coordinator
fans one question out as many ``Prime.Check`` calls and folds the replies into one
answer (``splitWork`` / ``watchReplies``, coordinator.go:67-98).  ``Client.Send`` is
the batched scatter; a ``Gather`` handed to it (``Send(batch, gather=g)``) is the
gather: how the batch's replies fold into one result per question.

``Gather(group, groups, op, sentinel=None)``: ``group`` int32[M] names the group of
every message of the batch (a negative id takes no part; an id ``>= groups`` takes no
part either and is counted in ``oob``).  For group g, with R its rows in message
order and OK meaning ``st[i] == STATUS_OK``:

* ``count[g]`` = ``|R|``, ``n_ok[g]`` = the OK rows of R (for every op)
* ``sum``: ``value[g]`` = the sum of ``val`` over the OK rows, wrapping mod 2**64 (0
  without one); ``min`` / ``max``: the signed minimum / maximum over the OK rows
  (``INT64_MAX`` / ``INT64_MIN`` without one)
* ``first_ne``: ``hit`` = the lowest OK row of R with ``val != sentinel[g]``;
  ``value[g] = val[hit]`` unless there is no hit or a non-OK row of R lies below it --
  then ``value[g] = sentinel[g]``.  Non-OK rows above ``hit`` are ignored
  (``watchReplies`` returns at the first reply that differs)
* ``bad_row[g]``: the lowest non-OK row of R, or -1 (``first_ne``: only a row below
  ``hit`` counts); ``status[g]`` = ``st[bad_row[g]]``, or ``STATUS_OK``: the first
  error in message order.  ``sum`` / ``min`` / ``max`` still fold the OK rows of a
  group whose status is bad

Every operation is an integer operation that does not depend on arrival order, so
the kernels (``csrc/hip/gather.hip``) equal ``gather_ref`` exactly.  The outputs are
device tensors owned by the object, allocated once: valid in stream order after
the Send, overwritten by the next Send that carries the object.  ``reduce`` reads
nothing on the host and allocates nothing, so it is legal under graph capture.
CPU tensors run ``gather_ref`` (the CPU suite, the gloo paths).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _ptr, hip, raw_stream
from .records import STATUS_OK

OPS = ("sum", "min", "max", "first_ne")  # gather.hpp kGatherSum .. kGatherFirstNe
ACC_WORDS = 4           # kGatherAccWords: value, count << 32 | n_ok, (bad, hit) u32 pair, spare
LDS_GROUPS = 2048       # kGatherLdsGroups
MAX_GROUPS = 1 << 26    # kGatherMaxGroups
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
IDENTITY = {"sum": 0, "min": INT64_MAX, "max": INT64_MIN, "first_ne": 0}


def _sentinel(sentinel, groups: int) -> np.ndarray:
    if isinstance(sentinel, torch.Tensor):
        s = sentinel.detach().cpu().numpy()
    else:
        s = np.asarray(sentinel, dtype=np.int64)
    return np.ascontiguousarray(np.broadcast_to(s.astype(np.int64), (groups,)))


def gather_ref(val, st, group, groups: int, op: str, sentinel=None) -> dict:
    """The spec in numpy: ``{"value" int64[G], "status" int32[G], "n_ok" int32[G],
    "count" int32[G], "bad_row" int32[G], "oob" int64[1]}`` as CPU tensors."""
    if op not in OPS:
        raise ValueError(f"gather: op must be one of {OPS}")
    G = int(groups)
    v = val.detach().cpu().numpy().astype(np.int64)
    s = st.detach().cpu().numpy().astype(np.int32)
    g = group.detach().cpu().numpy().astype(np.int64)
    M = v.size
    none = np.int64(M)  # "no such row"
    rows = np.arange(M, dtype=np.int64)
    inside = (g >= 0) & (g < G)
    ok = inside & (s == STATUS_OK)
    gi, go = g[inside], g[ok]
    count = np.bincount(gi, minlength=G)
    n_ok = np.bincount(go, minlength=G)
    value = np.full(G, IDENTITY[op], dtype=np.int64)
    bad = np.full(G, none, dtype=np.int64)
    np.minimum.at(bad, g[inside & ~ok], rows[inside & ~ok])
    if op == "sum":
        acc = np.zeros(G, dtype=np.uint64)
        np.add.at(acc, go, v[ok].view(np.uint64))  # (uint64 adds wrap)
        value = acc.view(np.int64)
    elif op == "min":
        np.minimum.at(value, go, v[ok])
    elif op == "max":
        np.maximum.at(value, go, v[ok])
    else:
        if sentinel is None:
            raise ValueError("gather: first_ne needs a sentinel")
        sen = _sentinel(sentinel, G)
        ne = ok.copy()
        ne[ok] = v[ok] != sen[go]
        hit = np.full(G, none, dtype=np.int64)
        np.minimum.at(hit, g[ne], rows[ne])
        bad = np.where(bad < hit, bad, none)  # a failure above the hit was never looked at
        value = np.where((bad == none) & (hit < none), v[np.minimum(hit, max(M - 1, 0))] if M else sen, sen)
    status = np.where(bad < none, s[np.minimum(bad, max(M - 1, 0))] if M else STATUS_OK, STATUS_OK)
    t = torch.from_numpy
    return {"value": t(np.ascontiguousarray(value, dtype=np.int64)), "status": t(status.astype(np.int32)),
            "n_ok": t(n_ok.astype(np.int32)), "count": t(count.astype(np.int32)),
            "bad_row": t(np.where(bad < none, bad, -1).astype(np.int32)),
            "oob": torch.tensor([int((g >= G).sum())], dtype=torch.int64)}


class Gather:
    """How one batch's replies fold into ``groups`` results (module docstring).
    Outputs -- ``value`` int64[G], ``status`` / ``n_ok`` / ``count`` / ``bad_row``
    int32[G], ``oob`` int64[1] -- live on ``group``'s device."""

    FIELDS = ("value", "status", "n_ok", "count", "bad_row", "oob")

    def __init__(self, group: torch.Tensor, groups: int, op: str, sentinel=None):
        if not isinstance(group, torch.Tensor) or group.dtype != torch.int32 or group.dim() != 1:
            raise ValueError("Gather: group must be an int32[M] tensor")
        if op not in OPS:
            raise ValueError(f"Gather: op must be one of {OPS}")
        G = int(groups)
        if not 1 <= G <= MAX_GROUPS:
            raise ValueError(f"Gather: groups must be in [1, {MAX_GROUPS}]")
        dev = group.device
        self.group, self.groups, self.op, self.device, self.M = group.contiguous(), G, op, dev, int(group.numel())
        self.sentinel = None
        if op == "first_ne":
            if sentinel is None:
                raise ValueError("Gather: first_ne needs a sentinel (int64[groups] or one int)")
            if isinstance(sentinel, torch.Tensor):
                if sentinel.dtype != torch.int64 or sentinel.numel() not in (1, G):
                    raise ValueError("Gather: sentinel must be int64[groups] (or one int)")
                if sentinel.device != dev:
                    raise ValueError("Gather: the sentinel lives on another device than group")
                self.sentinel = sentinel.reshape(-1).expand(G).contiguous()
            else:
                self.sentinel = torch.full((G,), int(sentinel), dtype=torch.int64, device=dev)
        self.value = torch.full((G,), IDENTITY[op], dtype=torch.int64, device=dev)
        self.status = torch.full((G,), STATUS_OK, dtype=torch.int32, device=dev)
        self.n_ok = torch.zeros(G, dtype=torch.int32, device=dev)
        self.count = torch.zeros(G, dtype=torch.int32, device=dev)
        self.bad_row = torch.full((G,), -1, dtype=torch.int32, device=dev)
        self.oob = torch.zeros(1, dtype=torch.int64, device=dev)
        self.acc = None
        if dev.type == "cuda":
            # the first image of the accumulators (csrc/hip/gather.hpp); the finish kernel
            # writes it back after every reduce
            self.acc = self.acc_image(G, op).to(dev)

    @staticmethod
    def acc_image(groups: int, op: str) -> torch.Tensor:
        """The accumulator buffer between reduces, int64[(G + 1) * ACC_WORDS] on the host."""
        img = torch.zeros(groups + 1, ACC_WORDS, dtype=torch.int64)
        img[:groups, 0] = IDENTITY[op]
        img[:groups, 2] = -1  # two u32 "no row"
        return img.reshape(-1)

    def check_batch(self, M: int) -> None:
        """Raise unless a batch of ``M`` messages is the one ``group`` describes (a Send
        checks before it sends anything)."""
        if int(M) != self.M:
            raise ValueError(f"Gather: the batch has {int(M)} messages, group has {self.M}")

    def reduce(self, val: torch.Tensor, st: torch.Tensor) -> "Gather":
        """Fold ``(val int64[M], st int32[M])`` into the outputs, on the current
        stream of the tensors' device: two kernel launches, no host read, no
        allocation (contiguous columns of any element alignment)."""
        if val.dtype != torch.int64 or st.dtype != torch.int32:
            raise ValueError("Gather: replies must be (int64 value, int32 status)")
        if val.numel() != self.M or st.numel() != self.M:
            raise ValueError(f"Gather: the batch has {val.numel()} messages, group has {self.M}")
        if val.device != self.device or st.device != self.device:
            raise ValueError("Gather: the replies live on another device than group")
        if self.device.type != "cuda":
            ref = gather_ref(val, st, self.group, self.groups, self.op, self.sentinel)
            for f in self.FIELDS:
                getattr(self, f).copy_(ref[f])
            return self
        val, st = val.contiguous(), st.contiguous()
        hip().reply_gather(_ptr(val), _ptr(st), _ptr(self.group), self.M, self.groups, OPS.index(self.op),
                           _ptr(self.sentinel), _ptr(self.acc), _ptr(self.value), _ptr(self.status), _ptr(self.n_ok),
                           _ptr(self.count), _ptr(self.bad_row), _ptr(self.oob), raw_stream(self.device))
        return self

    def outputs(self) -> dict:
        """The outputs as a dict of CPU tensors (a host read): ``gather_ref``'s shape."""
        return {f: getattr(self, f).detach().cpu() for f in self.FIELDS}
