"""Shared fixtures of the concurrency-limit tests: the processor-sharing
server model (in arithmetic, on the virtual clock and over loopback
TCP), a pool of 16 connections on a DummyResolver, and closed-loop
claimers."""

import asyncio
import heapq

from cueball_amd import utils as mod_utils
from cueball_amd.limit import ConcurrencyLimiter
from cueball_amd.testing import advance, settle

from claim_queue_kit import QueueKit

#: the model server: CAPACITY requests at once take BASE ms each, n of
#: them take ``BASE * max(1, n / CAPACITY)``
CAPACITY = 4
BASE = 50.0
CLAIMERS = 16


def hold_of(active, base=BASE, capacity=CAPACITY):
    return base * max(1.0, active / capacity)


def limiter(cl, maximum=CLAIMERS):
    """A ConcurrencyLimiter from the option as a pool would take it."""
    return ConcurrencyLimiter(mod_utils.assert_concurrency_limit(
        {"maximum": maximum, "concurrencyLimit": cl}))


def closed_loop(lim, windows, claimers=CLAIMERS):
    """Drive `lim` alone with `claimers` closed-loop claimers against
    the model server until `windows` windows have closed: a claimer
    starts a lease whenever ``allowed()`` leaves room, its hold time
    fixed at the start by the leases then in flight.  Returns
    ``floor(limit)`` after each window."""
    now = 0.0
    ends = []
    seq = 0
    active = 0
    floors = []
    while lim.windows < windows:
        while active < min(claimers, lim.allowed()):
            active += 1
            seq += 1
            hold = hold_of(active)
            heapq.heappush(ends, (now + hold, seq, lim.on_start(now), hold))
        now, _, token, hold = heapq.heappop(ends)
        active -= 1
        before = lim.windows
        lim.on_sample(token, hold, now)
        if lim.windows != before:
            floors.append(int(lim.limit // 1))
    return floors


class LimitKit(QueueKit):
    """Four backends, four connections each: ``maximum`` 16, and the
    labelled claims of the claim-queue kit.  ``cl`` is the
    ``concurrencyLimit`` option, None for a pool without it."""

    def __init__(self, loop, cl=None, cq=None, **opts):
        if cl is not None:
            opts["concurrencyLimit"] = cl
        opts.setdefault("backends", ("b1", "b2", "b3", "b4"))
        opts.setdefault("per", 4)
        super().__init__(loop, cq, **opts)
        self.events = []
        self.pool.on("limitChanged",
                     lambda new, old: self.events.append((new, old)))

    async def up_auto(self):
        """up() for a pool that sizes itself: every socket connects as
        it is made, and nothing is said about their order."""
        self.auto = True
        self.resolver_fsm.start()
        for k in self.backends:
            self.resolver.add(k, {"address": "10.0.0.1", "port": 80})
        await advance(self.loop, 0.05)
        return self

    def key(self, label):
        """The backend that served the claim `label`."""
        return self.boxes[label]["conn"].key

    def limit(self):
        return self.pool.get_limit_stats()

    def in_flight(self):
        return self.limit()["inFlight"]

    def idle(self):
        return self.pool.get_stats()["idleConnections"]

    def waiting(self):
        return self.pool.get_stats()["waiterCount"]

    def live_handles(self, boxes):
        """The kit's own count: handles of `boxes` that hold a lease."""
        return sum(1 for b in boxes
                   if b.get("hdl") is not None and
                   b["hdl"].get_state() in ("claiming", "claimed"))

    async def closed_loop(self, seconds, claimers=CLAIMERS, base=BASE):
        """`claimers` closed-loop claimers against the model server for
        `seconds` of virtual time.  Returns ``{"leases": [(end s, hold
        ms)], "peaks": [(s, active)], "served"}``; afterwards every
        lease has ended."""
        loop = self.loop
        t0 = loop.time()
        state = {"active": 0, "stop": False}
        leases = []
        peaks = []

        def claim():
            self.pool.claim({}, cb)

        def cb(err, hdl=None, conn=None):
            assert err is None, err
            state["active"] += 1
            peaks.append((loop.time() - t0, state["active"]))
            hold = hold_of(state["active"], base)

            def done():
                state["active"] -= 1
                leases.append((loop.time() - t0, hold))
                hdl.release()
                if not state["stop"]:
                    claim()

            loop.call_later(hold / 1000.0, done)

        for _ in range(claimers):
            claim()
        await advance(loop, seconds)
        state["stop"] = True
        await advance(loop, 1.0)
        assert state["active"] == 0
        return {"leases": leases, "peaks": peaks,
                "served": sum(1 for t, _ in leases if t <= seconds)}


class ModelServer:
    """The model server over loopback TCP: a line echo that answers
    after ``base * max(1, active / CAPACITY)`` seconds, `active` counting
    the lines being answered, the new one included."""

    def __init__(self, base):
        self.base = base
        self.active = 0
        self.served = 0
        self.peaks = []         # (loop time, active) at every arrival
        self.port = None
        self._server = None
        self._writers = set()

    async def start(self):
        self._server = await asyncio.start_server(
            self._handle, "127.0.0.1", 0)
        self.port = self._server.sockets[0].getsockname()[1]
        return self

    def stop(self):
        self._server.close()
        for w in list(self._writers):
            w.close()

    async def _handle(self, reader, writer):
        loop = asyncio.get_running_loop()
        self._writers.add(writer)
        try:
            while True:
                data = await reader.readline()
                if not data:
                    break
                self.active += 1
                self.peaks.append((loop.time(), self.active))
                try:
                    await asyncio.sleep(
                        self.base * max(1.0, self.active / CAPACITY))
                finally:
                    self.active -= 1
                self.served += 1
                writer.write(data)
                await writer.drain()
        except (asyncio.IncompleteReadError, ConnectionResetError,
                BrokenPipeError):
            pass
        finally:
            self._writers.discard(writer)
            writer.close()
