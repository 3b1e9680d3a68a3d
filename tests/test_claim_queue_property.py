"""A seeded random driver over a pool with ``claimQueue``: two
connections, ``maxQueued`` 6, three classes, under each order.  The
model is a plain list kept by the rules of the option as they are
documented: link the claim where its class and the order put it, then,
if the list is too long, the last entry loses.  After every step the
pool's waiter queue equals the list, and at the end every callback has
fired exactly once, with the outcome the model predicted."""

import random

import pytest

from cueball_amd.testing import advance, settle
from conftest import run_vt
from claim_queue_kit import QueueKit

MAX_QUEUED = 6
CLASSES = 3
LIFO_AFTER = 50
STEPS = 400

ORDERS = {
    "fifo": {"order": "fifo"},
    "lifo": {"order": "lifo"},
    "adaptive": {"order": "adaptive", "lifoAfter": LIFO_AFTER},
}


class Model:
    def __init__(self, order, idle):
        self.order = order
        self.queue = []         # [label], head first
        self.prio = {}
        self.deadline = {}      # label -> ms, waiters with a timeout
        self.expect = {}        # label -> outcome, None: no callback
        self.holders = []
        self.idle = idle
        self.since = 0.0

    def newest_first(self, now):
        if self.order == "fifo":
            return False
        if self.order == "lifo":
            return True
        return bool(self.queue) and now - self.since >= LIFO_AFTER

    def claim(self, label, prio, timeout, now):
        self.prio[label] = prio
        if self.idle:
            self.idle -= 1
            self.holders.append(label)
            self.expect[label] = "served"
            return
        if not self.queue:
            self.since = now
        ahead = self.newest_first(now)
        at = len(self.queue)
        for i, other in enumerate(self.queue):
            if self.prio[other] > prio or \
                    (ahead and self.prio[other] == prio):
                at = i
                break
        self.queue.insert(at, label)
        if timeout is not None:
            self.deadline[label] = now + timeout
        if len(self.queue) > MAX_QUEUED:
            loser = self.queue.pop()
            self.deadline.pop(loser, None)
            self.expect[loser] = "ClaimQueueFullError", loser != label

    def cancel(self, label):
        self.queue.remove(label)
        self.deadline.pop(label, None)
        self.expect[label] = None

    def expire(self, now):
        for label in [l for l in self.queue
                      if self.deadline.get(l, now + 1) <= now]:
            self.queue.remove(label)
            del self.deadline[label]
            self.expect[label] = "ClaimTimeoutError"

    def release(self, label):
        self.holders.remove(label)
        if self.queue:
            nxt = self.queue.pop(0)
            self.deadline.pop(nxt, None)
            self.holders.append(nxt)
            self.expect[nxt] = "served"
        else:
            self.idle += 1


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_queue_follows_the_model(order, seed):
    async def body(loop):
        rng = random.Random("%s-%d" % (order, seed))
        cq = dict(ORDERS[order], maxQueued=MAX_QUEUED, priorities=CLASSES)
        kit = await QueueKit(loop, cq).up()
        model = Model(order, idle=2)
        serial = 0
        t0 = loop.time()

        def now():
            return (loop.time() - t0) * 1000.0

        for step in range(STEPS):
            op = rng.choice(("claim", "claim", "claim", "cancel",
                             "advance", "release", "release"))
            if op == "claim":
                serial += 1
                label = "c%d" % serial
                prio = rng.randrange(CLASSES)
                # deadlines end in 5 ms, the clock moves in tens: no
                # deadline ever falls on the instant of a step
                timeout = rng.choice((None, None, 25, 65, 105))
                opts = {} if timeout is None else {"timeout": timeout}
                model.claim(label, prio, timeout, now())
                kit.queue(label, prio, **opts)
            elif op == "cancel":
                if not model.queue:
                    continue
                label = rng.choice(model.queue)
                model.cancel(label)
                kit.boxes[label]["waiter"].cancel()
            elif op == "advance":
                await advance(loop, rng.choice((0.01, 0.02, 0.04)))
                model.expire(now())
            else:
                if not model.holders:
                    continue
                label = rng.choice(model.holders)
                model.release(label)
                kit.boxes[label]["hdl"].release()
            await settle(loop)
            assert kit.order() == model.queue, (step, op)
            st = kit.queue_stats()
            assert st["queued"] == [
                sum(1 for l in model.queue if model.prio[l] == p)
                for p in range(CLASSES)]
            assert st["lifo"] == model.newest_first(now())
            assert len(model.queue) <= MAX_QUEUED

        # wind down: serve whatever still waits
        while model.holders:
            label = model.holders[0]
            model.release(label)
            kit.boxes[label]["hdl"].release()
            await settle(loop)
            assert kit.order() == model.queue
        assert model.queue == [] and kit.order() == []

        outcomes = dict(kit.log)
        assert len(outcomes) == len(kit.log)       # nobody called twice
        shed = rejected = 0
        for label, want in model.expect.items():
            box = kit.boxes[label]
            if want is None:
                assert box["fired"] == 0, label
                continue
            assert box["fired"] == 1, label
            if isinstance(want, tuple):
                want, displaced = want
                assert kit.errors[label].displaced is displaced, label
                shed += displaced
                rejected += not displaced
            assert outcomes[label] == want, label
        assert set(model.expect) == set(kit.boxes)
        st = kit.queue_stats()
        assert (st["shed"], st["rejected"]) == (shed, rejected)
        # the run went through what it is about
        assert shed + rejected > 0
        assert "ClaimTimeoutError" in outcomes.values()
        await kit.stop()
    run_vt(body)
