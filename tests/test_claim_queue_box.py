"""The claim queue over real sockets on the deployment box (run with
-m gpu).

One loopback line-echo server that answers after 50 ms behind a pool of
one connection, so that every claim behind the first waits in the
queue.  The placement rules are pinned on the virtual clock in
test_claim_queue_pool.py; this is about the plumbing: the native deque's
new methods under the native feed, the native handle under a Python
ticket, shedding on the real clock, real TCP.  About half a second in
all.
"""

import asyncio

import pytest

from cueball_amd.errors import ClaimQueueFullError

from balance_kit import DelayServer
from retry_kit import run, until

pytestmark = pytest.mark.gpu

DELAY = 0.05
RECOVERY = {"default": {"timeout": 2000, "retries": 2, "delay": 50,
                        "maxDelay": 200}}


def test_native_runtime_in_use():
    """The claim queue must ride on the native deque, handle and slot
    cycle, not replace them."""
    from cueball_amd import _speed
    from cueball_amd import connection_fsm, fsm, pool, queue
    assert fsm.FSM is _speed.FSM
    assert pool._native_pool_claim is _speed.pool_claim
    assert pool._NativeClaimTicket is _speed.ClaimTicket
    assert pool._NativeSlotDispatch is _speed.SlotDispatch
    assert issubclass(connection_fsm.ClaimHandle, _speed.ClaimHandleBase)
    assert connection_fsm._SlotKit is _speed.SlotKit
    assert queue.Queue is _speed.Queue
    for name in ("unshift", "insert_after", "peek_last"):
        assert callable(getattr(queue.Queue, name)), name
        assert name in _speed.Queue.__dict__, name


class Box:
    """The pool, its one connection's server, and labelled claimers:
    each writes its label as a line and releases on the echo."""

    async def start(self, cq):
        from cueball_amd.connection import tcp_constructor
        from cueball_amd.pool import ConnectionPool
        from cueball_amd.resolver import StaticIpResolver

        self.loop = loop = asyncio.get_running_loop()
        self.server = await DelayServer(delay=DELAY, http=False).start()
        resolver = StaticIpResolver({"backends": [
            {"address": "127.0.0.1", "port": self.server.port}]})
        self.pool = ConnectionPool({
            "domain": "queue.box", "constructor": tcp_constructor(loop=loop),
            "resolver": resolver, "recovery": RECOVERY, "spares": 1,
            "maximum": 1, "loop": loop, "claimQueue": cq})
        resolver.start()
        await until(lambda: self.pool.get_stats()["idleConnections"] == 1,
                    "the connection")
        self.wrote = []     # labels in the order their lines went out
        self.done = []      # labels in the order their echoes came back
        self.failed = {}    # label -> error
        self.garbled = []
        return self

    def claim(self, label, **options):
        line = label.encode() + b"\n"

        def cb(err, hdl=None, conn=None):
            if err is not None:
                self.failed[label] = err
                return
            got = []

            def on_data(chunk):
                got.append(chunk)
                if b"".join(got).endswith(b"\n"):
                    conn.remove_listener("data", on_data)
                    if b"".join(got) != line:
                        self.garbled.append((label, b"".join(got)))
                    hdl.release()
                    self.done.append(label)

            conn.on("data", on_data)
            self.wrote.append(label)
            conn.write(line)

        return self.pool.claim(options, cb)

    async def settled(self, claims):
        await until(lambda: len(self.done) + len(self.failed) == claims,
                    "the last echo")
        # the pool hears of the last release a loop turn later
        await until(lambda: self.pool.get_stats()["idleConnections"] == 1,
                    "the last release")
        assert self.garbled == []

    async def stop(self):
        stopped = self.loop.create_future()
        self.pool.on("stateChanged",
                     lambda st: st == "stopped" and stopped.set_result(None))
        self.pool.stop()
        await asyncio.wait_for(stopped, 10.0)
        self.server.stop()


def test_bound_and_classes_over_real_sockets():
    async def body():
        box = await Box().start({"maxQueued": 4, "priorities": 2})
        spec = [("first", 0)] + \
            [("low%d" % n, 1) for n in range(1, 5)] + \
            [("high1", 0), ("high2", 0), ("late", 1)]
        for label, prio in spec:
            box.claim(label, priority=prio)
            await asyncio.sleep(0)
        await box.settled(len(spec))
        counters = dict(box.pool.get_stats()["counters"])
        stats = box.pool.get_queue_stats()
        print("wrote", box.wrote, "failed", sorted(box.failed),
              "counters", counters)
        # the two newest of the first four were displaced, the last
        # claim turned away
        assert sorted(box.failed) == ["late", "low3", "low4"]
        assert all(isinstance(e, ClaimQueueFullError)
                   for e in box.failed.values())
        assert box.failed["low3"].displaced is True
        assert box.failed["low4"].displaced is True
        assert box.failed["late"].displaced is False
        assert box.wrote == ["first", "high1", "high2", "low1", "low2"]
        assert box.done == box.wrote
        assert counters["queue-shed"] == 2
        assert counters["queue-rejected"] == 1
        assert counters["claim"] == len(spec)
        assert counters["max-claim-queue"] == 4
        # four queued at first, then the two that displaced
        assert counters["queued-claim"] == 6
        assert box.server.served == len(box.done) == 5
        assert len(box.done) + len(box.failed) == len(spec)
        assert stats["queued"] == [0, 0]
        assert (stats["rejected"], stats["shed"]) == (1, 2)
        assert box.pool.get_stats()["waiterCount"] == 0
        await box.stop()
    run(body())


def test_newest_first_over_real_sockets():
    async def body():
        box = await Box().start({"order": "lifo"})
        for label in ("first", "w1", "w2", "w3"):
            box.claim(label)
            await asyncio.sleep(0)
        await box.settled(4)
        counters = dict(box.pool.get_stats()["counters"])
        print("wrote", box.wrote, "counters", counters)
        assert box.failed == {}
        assert box.wrote == ["first", "w3", "w2", "w1"]
        assert box.done == box.wrote
        assert counters["queue-lifo"] == 3
        assert box.server.served == 4
        assert box.pool.get_queue_stats()["queued"] == [0]
        await box.stop()
    run(body())
