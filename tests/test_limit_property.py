"""A seeded random driver over a pool with ``concurrencyLimit``: claims,
releases, closes, cancels, the clock and backends that come and go, under
a gradient limiter whose windows and probes are short enough to move
``allowed()`` many times in a run.  After every step, once the loop has
settled, the pool's count of leases in flight is the kit's own, it is
within what was allowed when those leases began, and no claim waits
beside an idle slot while there is room under the limit."""

import random

import pytest

from cueball_amd.testing import advance, settle
from conftest import run_vt
from limit_kit import LimitKit

STEPS = 400
CL = {"window": 40, "minSamples": 2, "probeSamples": 2, "probeLimit": 2,
      "probeSpread": 0, "probeInterval": 300, "initialLimit": 5,
      "maxLimit": 8, "smoothing": 1.0}


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_in_flight_follows_the_handles_and_the_gate_holds(seed):
    async def body(loop):
        rng = random.Random(seed)
        kit = await LimitKit(loop, CL, backends=("b1", "b2"), per=4).up()
        pool = kit.pool
        present = {"b1", "b2"}
        serial = 0
        began = {}          # label -> allowed() when its lease began
        ended = set()

        def live():
            return [l for l in began if l not in ended and
                    kit.boxes[l]["hdl"].get_state() in
                    ("claiming", "claimed")]

        allowed_seen = set()
        moved = 0
        for step in range(STEPS):
            op = rng.choice(("claim", "claim", "claim", "release",
                             "release", "close", "cancel", "advance",
                             "advance", "backend"))
            before = kit.limit()["allowed"]
            if op == "claim":
                serial += 1
                timeout = rng.choice((None, None, 35, 75))
                opts = {} if timeout is None else {"timeout": timeout}
                kit.queue("c%d" % serial, **opts)
            elif op in ("release", "close"):
                held = live()
                if not held:
                    continue
                label = rng.choice(held)
                ended.add(label)
                getattr(kit.boxes[label]["hdl"], op)()
            elif op == "cancel":
                waiting = kit.order()
                if not waiting:
                    continue
                kit.boxes[rng.choice(waiting)]["waiter"].cancel()
            elif op == "advance":
                await advance(loop, rng.choice((0.01, 0.02, 0.04)))
            else:
                if len(present) == 2 and rng.random() < 0.5:
                    gone = rng.choice(sorted(present))
                    present.discard(gone)
                    kit.resolver.remove(gone)
                elif len(present) < 2:
                    back = ({"b1", "b2"} - present).pop()
                    present.add(back)
                    kit.resolver.add(back, {"address": "10.0.0.1",
                                            "port": 80})
            await settle(loop)
            # whatever was served in this step began under `before` or
            # under what allowed() is now
            st = kit.limit()
            for label in kit.served():
                if label not in began:
                    began[label] = max(before, st["allowed"])
            allowed_seen.add(st["allowed"])
            moved += st["allowed"] != before

            held = live()
            assert st["inFlight"] == len(held), (step, op)
            assert st["inFlight"] == pool.p_cl_lim.in_flight
            assert 0 <= st["inFlight"] <= max(
                [began[l] for l in held] or [0]), (step, op)
            idle = sum(1 for fsm in pool.p_idleq
                       if fsm.is_in_state("idle"))
            if st["inFlight"] < st["allowed"]:
                assert not (kit.waiting() > 0 and idle > 0), (step, op)

        # the run went through what it is about
        assert moved >= 6 and len(allowed_seen) >= 3, (moved, allowed_seen)
        assert kit.pool.get_stats()["counters"].get("limit-held", 0) > 0
        assert kit.limit()["probes"] >= 3

        # wind down
        for _ in range(50):
            for label in kit.served():
                began.setdefault(label, 0)
            if not live() and kit.waiting() == 0:
                break
            for label in live():
                ended.add(label)
                kit.boxes[label]["hdl"].release()
            await advance(loop, 0.05)
        assert kit.waiting() == 0
        assert kit.in_flight() == 0 and pool.p_cl_lim.in_flight == 0
        assert not pool.p_cl_open and not pool.p_cl_handed
        await kit.stop()
    run_vt(body)
