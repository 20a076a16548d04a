#!/usr/bin/env python3
"""retry_select + retry_merge (csrc/hip/retry.hip) against the torch sequence the
overflow re-send path uses (``nonzero`` + ``index_select`` per column + indexed
stores), on the same tensors: M messages, a fraction of them failed.

Both sides are timed with a host clock around work that ends in a device
synchronise (the selection needs K on the host either way), after warm-up, and
their results are compared.  Host syncs are counted from what each sequence
does: one ``.item()`` for the kernels, one ``nonzero`` for torch.

    python tools/retry_select_bench.py [--msgs 8388608] [--failed 0.01] [--iters 50] [--md FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ptype_amd.ops import retry as R  # noqa: E402
from ptype_amd.ops.batch import MsgBatch  # noqa: E402
from ptype_amd.ops.records import METHOD_RETRY_TEST, STATUS_FAILED, STATUS_OK  # noqa: E402


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--msgs", type=int, default=8 << 20)
    ap.add_argument("--failed", type=float, default=0.01)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--md", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("retry_select_bench: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    M = a.msgs
    g = torch.Generator(device=dev).manual_seed(1)
    st0 = torch.where(torch.rand(M, generator=g, device=dev) < a.failed, STATUS_FAILED, STATUS_OK).to(torch.int32)
    col = (lambda: torch.randint(-2**40, 2**40, (M,), generator=g, device=dev))
    batch = MsgBatch(torch.randint(0, 1 << 20, (M,), generator=g, device=dev).to(torch.int32), col(), col(), None,
                     METHOD_RETRY_TEST)
    val0 = col()
    K = int((st0 == STATUS_FAILED).sum())
    v2, s2 = torch.arange(K, dtype=torch.int64, device=dev), torch.zeros(K, dtype=torch.int32, device=dev)
    val_k, st_k, val_t, st_t = val0.clone(), st0.clone(), val0.clone(), st0.clone()
    out = {}

    def kernels():
        st_k.copy_(st0)
        sub, idx, k = R.select(batch, st_k, (STATUS_FAILED,))
        R.merge(val_k, st_k, idx, v2, s2)
        out["k"] = (sub, idx)

    def torch_seq():  # ActorExchange._resend_rounds
        st_t.copy_(st0)
        idx = torch.nonzero(st_t == STATUS_FAILED).flatten()
        sub = batch.index_select(idx)
        val_t[idx] = v2
        st_t[idx] = s2
        out["t"] = (sub, idx)

    def restore():  # what both timed sequences include
        st_k.copy_(st0)

    tr = timed(restore, a.iters)
    tk, tt = timed(kernels, a.iters), timed(torch_seq, a.iters)
    (sk, ik), (stt, it) = out["k"], out["t"]
    same = (torch.equal(ik.to(torch.int64), it) and torch.equal(sk.actor, stt.actor) and torch.equal(sk.a0, stt.a0)
            and torch.equal(sk.a1, stt.a1) and torch.equal(val_k, val_t) and torch.equal(st_k, st_t))
    rows = [("retry_select + retry_merge (3 kernels)", tk, 1), ("torch nonzero + index_select x3 + 2 indexed stores", tt, 1)]
    lines = [f"M = {M} messages, K = {K} failed ({100.0 * K / M:.2f} %), columns actor / a0 / a1, {a.iters} timed calls "
             "after 5 warm-up calls, host clock around the sequence + a device synchronise; every call first restores",
             f"the status column with a device copy (median {tr[0]:.3f} ms alone, included in both rows).", "",
             "| sequence | median ms | min ms | max ms | host syncs per call |", "|---|---|---|---|---|"]
    for name, (med, lo, hi), syncs in rows:
        lines.append(f"| {name} | {med:.3f} | {lo:.3f} | {hi:.3f} | {syncs} |")
    lines += ["", f"results identical: {same}"]
    text = "\n".join(lines)
    print(text)
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
