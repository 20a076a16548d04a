#!/usr/bin/env python3
"""Redrive with back-off: dead letters re-sent through the timer queue.

    python examples/actors/timers.py             # one GPU
    python examples/actors/timers.py --cpu       # the numpy models, no GPU

The counters example with a rate limit: every counter actor takes one ``CounterAdd`` per
Send (``limit_rate=1, limit_burst=1``), and one batch carries ``--adds`` of them for every
actor.  The first of each actor travels, the others are answered ``STATUS_THROTTLED`` and --
the dead-letter mask names that status -- kept in the dead-letter queue in HBM.  Re-sending
them at once (``redrive``) would throttle all but one per actor again, in a tight loop; here
each round takes the letters and schedules them ``min(2 ** round, horizon)`` ticks ahead
(``schedule(letters.batch(), delay)``), and the ticks in between send nothing.  A record has
no ``attempts`` field -- a letter that fails again after a scheduled re-send is filed with
``attempts`` 1 -- so the back-off grows with the caller's round, not with the letter's count.
In the end every counter holds ``--adds``.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))

import torch  # noqa: E402

from ptype_amd.ops.batch import MsgBatch  # noqa: E402
from ptype_amd.ops.records import METHOD_COUNTER_ADD, STATUS_OK, STATUS_THROTTLED  # noqa: E402
from ptype_amd.runtime import DeviceRuntime  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--actors", type=int, default=4096)
    p.add_argument("--adds", type=int, default=4, help="CounterAdd(+1) messages per actor in the one batch")
    p.add_argument("--horizon", type=int, default=16)
    p.add_argument("--cpu", action="store_true")
    a = p.parse_args()
    dev = torch.device("cpu") if a.cpu else torch.device("cuda", 0)
    M = a.actors * a.adds
    rt = DeviceRuntime(dev, actors=a.actors, max_batch=M, service="counters", shm=False, limit_rate=1, limit_burst=1,
                       dead_letters=True, dead_letter_entries=max(64, 1 << (M - 1).bit_length()),
                       dead_letter_mask=[STATUS_THROTTLED], timers=True,
                       timer_entries=max(64, 1 << (M - 1).bit_length()), timer_horizon=a.horizon)
    rt.place_local()
    actors = (torch.arange(M, dtype=torch.int32) % a.actors).to(dev)
    batch = MsgBatch(actors, torch.ones(M, dtype=torch.int64, device=dev), None, None, METHOD_COUNTER_ADD)
    _, st = rt.send("counters", batch, limit=True, dead_letter=True)
    print(f"first Send: {int((st == STATUS_OK).sum())} of {M} travelled, "
          f"{rt.stats()['dead_letters']['unread']} throttled calls are dead letters", flush=True)
    rounds = 0
    while True:
        letters = rt.dead_letters(drain=True)
        if not letters.n:
            break
        rounds += 1
        delay = min(2 ** rounds, a.horizon)
        s = rt.schedule(letters.batch(), delay)
        ticked = rt.tick("counters", ticks=delay, limit=True, dead_letter=True)
        sent = [t.n for t in ticked]
        ok = int((ticked[-1].status == STATUS_OK).sum())
        print(f"round {rounds}: {s.n} letters scheduled {delay} ticks ahead at tick {s.now}; rows sent per tick {sent}; "
              f"{ok} delivered", flush=True)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    done = bool((rt.state == a.adds).all())
    t = rt.timers()
    print(f"every counter == {a.adds}: {done}; clock at tick {t['now']}, {t['delivered']} records delivered by "
          f"{rounds} scheduled rounds, {t['live']} pending", flush=True)
    rt.close()
    sys.exit(0 if done and t["live"] == 0 else 1)


if __name__ == "__main__":
    main()
