"""``maxConnectionAge`` and ``recycle()`` on a pool: every connected
socket gets a deadline; idle connections are retired one at a time,
each after the previous one's replacement connected; a claimed
connection is left alone until its lease is released."""

import asyncio
import gc

from cueball_amd.pool import ConnectionPool
from cueball_amd.resolver import ResolverFSM
from cueball_amd.testing import (DummyConnection, DummyResolver, advance,
                                 settle)
from conftest import run_vt

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 0}}
AGE = 60_000


def instance_vars(obj):
    """vars(obj); the native runtime's objects keep their instance dict
    without a ``__dict__`` attribute, so there it is found among the
    object's referents."""
    try:
        return vars(obj)
    except TypeError:
        for ref in gc.get_referents(obj):
            if isinstance(ref, dict) and ref.get("p_uuid") == obj.p_uuid:
                return ref
        raise


async def leap(loop, seconds):
    """Move the virtual clock ahead without visiting every 5 Hz sample
    on the way: each timer that is overdue then fires once."""
    loop._vt_set(loop.time() + seconds)
    await asyncio.sleep(0)
    await settle(loop)


class Kit:
    """A pool on a DummyResolver.  ``conns`` keeps every connection
    ever constructed, in order; ``died`` maps a connection to the
    virtual time of its destroy()."""

    def __init__(self, loop, backends=("b1",), auto=(), **opts):
        self.loop = loop
        self.conns = []
        self.born = {}
        self.died = {}
        self.events = []
        self.resolver = DummyResolver()

        def constructor(backend):
            c = DummyConnection(backend)
            c.key = backend["key"]
            self.conns.append(c)
            orig_connect, orig_destroy = c.connect, c.destroy

            def connect():
                self.born[c] = loop.time()
                orig_connect()

            def destroy():
                self.died.setdefault(c, loop.time())
                orig_destroy()

            c.connect, c.destroy = connect, destroy
            if c.key in auto:
                loop.call_soon(c.connect)
            return c

        base = {"constructor": constructor, "recovery": RECOVERY,
                "loop": loop, "domain": "foobar", "spares": 1,
                "maximum": 1}
        base.update(opts)
        if base.get("maxConnectionAge") is not None:
            base.setdefault("connectionAgeSpread", 0)
        self.resolver_fsm = ResolverFSM(self.resolver, {"loop": loop})
        base["resolver"] = self.resolver_fsm
        self.pool = ConnectionPool(base)
        self.pool.on("connectionRecycled",
                     lambda key, reason: self.events.append((key, reason)))
        self.resolver_fsm.start()
        for k in backends:
            self.resolver.add(k, {"address": "10.0.0.1", "port": 80})

    def dead(self, conns=None):
        return [c for c in (self.conns if conns is None else conns)
                if c.dead]

    async def connect_new(self):
        for c in self.conns:
            if not c.connected and not c.dead:
                c.connect()
        await settle(self.loop)

    async def to(self, t):
        """Advance to the absolute virtual time `t`, exactly."""
        await advance(self.loop, t - self.loop.time())

    def claim(self):
        box = {}

        def cb(err, hdl=None, conn=None):
            box.update(err=err, hdl=hdl, conn=conn)

        self.pool.claim({"timeout": 10_000}, cb)
        return box

    def counter(self, name):
        return self.pool.get_stats()["counters"].get(name, 0)

    async def stop(self):
        self.pool.stop()
        # long enough for a slot that is still connecting to give up
        await advance(self.loop, 30.0)
        assert self.pool.is_in_state("stopped")


def test_idle_connections_are_retired_one_at_a_time():
    async def body(loop):
        kit = Kit(loop, spares=4, maximum=8, maxConnectionAge=AGE)
        pool = kit.pool
        await settle(loop)
        assert len(kit.conns) == 4
        originals = list(kit.conns)
        t0 = loop.time()
        await kit.connect_new()
        idle = [pool.get_stats()["idleConnections"]]
        assert idle == [4]

        await kit.to(t0 + 59.9)
        assert kit.dead() == []
        await kit.to(t0 + 60)
        idle.append(pool.get_stats()["idleConnections"])
        assert len(kit.dead(originals)) == 1
        assert len(kit.conns) == 5 and not kit.conns[4].connected

        # the replacement is still connecting: nothing else goes
        await kit.to(t0 + 61)
        idle.append(pool.get_stats()["idleConnections"])
        assert len(kit.dead(originals)) == 1
        assert len(kit.conns) == 5

        for n in (2, 3, 4):
            await kit.connect_new()
            idle.append(pool.get_stats()["idleConnections"])
            assert len(kit.dead(originals)) == n
            assert len(kit.conns) == 4 + n
        await kit.connect_new()
        idle.append(pool.get_stats()["idleConnections"])

        assert len(kit.conns) == 8
        assert kit.counter("recycled-age") == 4
        assert kit.events == [("b1", "age")] * 4
        assert kit.dead(kit.conns[4:]) == []
        print("idleConnections at each observation:", idle)
        assert min(idle) >= 3
        assert idle[-1] == 4
        await kit.stop()
    run_vt(body)


def test_busy_lease_is_not_disturbed():
    async def body(loop):
        kit = Kit(loop, maxConnectionAge=AGE)
        pool = kit.pool
        await settle(loop)
        t0 = loop.time()
        await kit.connect_new()
        box = kit.claim()
        await settle(loop)
        c0 = kit.conns[0]
        assert box["err"] is None and box["conn"] is c0

        await kit.to(t0 + 61)
        assert not c0.dead and c0.connected
        assert box["conn"] is c0
        assert len(kit.conns) == 1
        ages = pool.get_connection_ages()["connections"]
        assert [a["recycling"] for a in ages] == [True]
        assert kit.counter("recycled-age") == 1   # counted when marked

        box["hdl"].release()
        box2 = kit.claim()
        await settle(loop)
        assert c0.dead
        assert len(kit.conns) == 2
        assert "conn" not in box2      # never handed the retired socket
        await kit.connect_new()
        assert box2["err"] is None
        assert box2["conn"] is kit.conns[1] and box2["conn"] is not c0
        assert kit.counter("recycled-age") == 1
        box2["hdl"].release()
        await kit.stop()
    run_vt(body)


def test_several_busy_leases_are_all_marked():
    async def body(loop):
        kit = Kit(loop, spares=2, maximum=2, maxConnectionAge=AGE)
        pool = kit.pool
        await settle(loop)
        t0 = loop.time()
        await kit.connect_new()
        boxes = [kit.claim(), kit.claim()]
        await settle(loop)
        assert {b["conn"] for b in boxes} == set(kit.conns[:2])

        await kit.to(t0 + 60)
        ages = pool.get_connection_ages()["connections"]
        assert [a["recycling"] for a in ages] == [True, True]
        assert [a["state"] for a in ages] == ["busy", "busy"]
        assert kit.dead() == []
        assert kit.counter("recycled-age") == 2

        # either may come back first; neither waits for the other
        boxes[1]["hdl"].release()
        await settle(loop)
        assert boxes[1]["conn"].dead and not boxes[0]["conn"].dead
        boxes[0]["hdl"].release()
        await settle(loop)
        assert boxes[0]["conn"].dead
        await kit.stop()
    run_vt(body)


def test_reconnect_resets_the_clock():
    async def body(loop):
        kit = Kit(loop, maxConnectionAge=AGE)
        await settle(loop)
        t0 = loop.time()
        await kit.connect_new()

        await kit.to(t0 + 30)
        kit.conns[0].emit("error", RuntimeError("reset by peer"))
        await advance(loop, 0)           # zero backoff delay
        assert len(kit.conns) == 2 and kit.conns[0].dead
        await kit.connect_new()
        c1 = kit.conns[1]
        assert kit.born[c1] == t0 + 30

        await kit.to(t0 + 60)
        assert not c1.dead
        assert kit.counter("recycled-age") == 0
        ages = kit.pool.get_connection_ages()
        assert ages["oldestMs"] == 30_000
        assert ages["connections"][0]["expiresInMs"] == 30_000
        await kit.to(t0 + 89.9)
        assert not c1.dead
        await kit.to(t0 + 90)
        assert c1.dead
        assert kit.died[c1] == t0 + 90
        assert kit.counter("recycled-age") == 1
        await kit.stop()
    run_vt(body)


def test_spread_staggers_the_deadlines():
    async def body(loop):
        kit = Kit(loop, auto=("b1",), spares=8, maximum=16,
                  maxConnectionAge=AGE, connectionAgeSpread=0.5)
        await settle(loop)
        originals = kit.conns[:8]
        assert len(originals) == 8
        assert all(c.connected for c in originals)
        for _ in range(70):
            await advance(loop, 1.0)
        lifetimes = [kit.died[c] - kit.born[c] for c in originals]
        print("lifetimes (s):", sorted(round(x, 2) for x in lifetimes))
        assert min(lifetimes) >= 30
        assert min(lifetimes) <= 60
        assert len(set(lifetimes)) > 1
        # "max" is the maximum: pacing may add loop turns, not seconds
        assert max(lifetimes) <= 60.001
        await kit.stop()
    run_vt(body)


def test_recycle_without_the_age_option():
    async def body(loop):
        kit = Kit(loop, spares=3, maximum=4)
        pool = kit.pool
        await settle(loop)
        await kit.connect_new()
        box = kit.claim()
        await advance(loop, 11.0)        # a periodic rebalance at the latest
        await kit.connect_new()          # the spare that replaces it
        assert len(kit.conns) == 4
        st = pool.get_stats()
        assert st["idleConnections"] == 3 and st["totalConnections"] == 4
        assert not any(k.startswith("p_age_") for k in instance_vars(pool))
        before = list(kit.conns)
        busy = box["conn"]

        assert pool.recycle() == 4
        # idle ones are paced, the busy one only marked
        assert len(kit.dead(before)) == 1 and not busy.dead
        await settle(loop)
        assert len(kit.conns) == 5
        await advance(loop, 1.0)
        assert len(kit.dead(before)) == 1
        for n in (2, 3):
            await kit.connect_new()
            assert len(kit.dead(before)) == n
            assert pool.get_stats()["idleConnections"] >= 2
        await kit.connect_new()
        assert not busy.dead
        assert kit.counter("recycled-manual") == 4
        assert len(kit.conns) == 7

        box["hdl"].release()
        await settle(loop)
        assert busy.dead
        await kit.connect_new()
        assert len(kit.dead(before)) == 4
        assert kit.events == [("b1", "manual")] * 4
        assert kit.counter("recycled-manual") == 4
        assert kit.counter("recycled-age") == 0

        # connections opened after the call are unaffected: a day
        # later none was recycled or replaced (the ordinary shrink
        # towards `spares` may have closed the fourth)
        after = kit.conns[4:]
        assert len(after) == 4
        await advance(loop, 60.0)
        for _ in range(24):
            await leap(loop, 3600.0)
        assert len(kit.dead(after)) <= 1
        assert len(kit.conns) == 8
        assert kit.counter("recycled-manual") == 4
        assert len(kit.events) == 4

        # a second call takes the new ones
        live = 4 - len(kit.dead(after))
        assert pool.recycle() == live
        await kit.stop()
        assert pool.recycle() == 0
    run_vt(body)


def test_recycle_on_a_failed_pool_returns_zero():
    async def body(loop):
        kit = Kit(loop, recovery={"default": {"timeout": 2000,
                                              "retries": 1, "delay": 0}})
        await settle(loop)
        kit.conns[0].emit("error", RuntimeError("refused"))
        await advance(loop, 0.1)
        assert kit.pool.is_in_state("failed")
        assert kit.pool.recycle() == 0
        await kit.stop()
    run_vt(body)


def test_recycling_at_maximum_needs_no_headroom():
    async def body(loop):
        kit = Kit(loop, auto=("b1",), spares=2, maximum=2,
                  maxConnectionAge=AGE)
        pool = kit.pool
        totals = []
        pool.on("connectionRecycled", lambda *a: totals.append(
            pool.get_stats()["totalConnections"]))
        await settle(loop)
        originals = kit.conns[:2]
        for _ in range(130):
            await advance(loop, 0.5)
            totals.append(pool.get_stats()["totalConnections"])
        assert len(kit.dead(originals)) == 2
        assert kit.counter("recycled-age") == 2
        assert max(totals) <= 2
        assert pool.get_stats()["idleConnections"] == 2
        assert len(kit.conns) == 4
        await kit.stop()
    run_vt(body)


def test_stop_cancels_the_age_timer():
    async def body(loop):
        kit = Kit(loop, spares=2, maximum=2, maxConnectionAge=AGE)
        await settle(loop)
        await kit.connect_new()
        assert kit.pool.p_age_timer is not None
        await advance(loop, 10.0)
        await kit.stop()
        n = len(kit.conns)
        await advance(loop, 2 * AGE / 1000.0)
        assert len(kit.conns) == n == 2
        assert kit.counter("recycled-age") == 0
        left = [h for h in loop._scheduled if not h._cancelled]
        assert left == []
    run_vt(body)


def test_dead_backend_does_not_block_recycling():
    async def body(loop):
        # b2 never answers: it is declared dead and keeps a monitor
        kit = Kit(loop, backends=("b1", "b2"), auto=("b1",), spares=2,
                  maximum=4, maxConnectionAge=AGE,
                  recovery={"default": {"timeout": 2000, "retries": 2,
                                        "delay": 0, "maxTimeout": 4000}})
        pool = kit.pool
        for _ in range(30):
            await advance(loop, 1.0)
        assert pool.is_declared_dead("b2")
        assert pool.is_in_state("running")
        monitors = [f for f in pool.p_connections["b2"] if f.csf_monitor]
        assert len(monitors) == 1
        first = [c for c in kit.conns if c.key == "b1"
                 and kit.born.get(c, 1e99) <= loop.time()]
        assert len(first) >= 2 and kit.dead(first) == []
        for _ in range(80):
            await advance(loop, 1.0)
        assert pool.is_declared_dead("b2")
        assert len(kit.dead(first)) == len(first)
        assert kit.counter("recycled-age") >= len(first)
        assert pool.get_stats()["idleConnections"] >= 2
        await kit.stop()
    run_vt(body)


def test_oldest_connection_gauge():
    async def body(loop):
        name = "cueball_pool_oldest_connection_seconds"
        kit = Kit(loop, spares=2, maximum=2, maxConnectionAge=AGE)
        pool = kit.pool
        await settle(loop)
        t0 = loop.time()
        kit.conns[0].connect()
        await kit.to(t0 + 5)
        kit.conns[1].connect()
        await kit.to(t0 + 12)
        pool._lp_tick()
        gauge = pool.p_collector.get_collector(name)
        labels = {"pool": pool.p_uuid.split("-")[0], "domain": "foobar"}
        assert gauge.value(labels) == 12.0
        assert pool.get_connection_ages()["oldestMs"] == 12_000
        assert name in pool.p_collector.collect()
        await kit.stop()

        plain = Kit(loop)
        await settle(loop)
        await plain.connect_new()
        await advance(loop, 0.5)
        assert name not in plain.pool.p_collector.collect()
        await plain.stop()
    run_vt(body)


def test_pool_that_is_not_running_retires_nothing():
    async def body(loop):
        kit = Kit(loop, spares=2, maximum=2, maxConnectionAge=AGE,
                  recovery={"default": {"timeout": 2000, "retries": 1,
                                        "delay": 0}})
        pool = kit.pool
        await settle(loop)
        t0 = loop.time()
        kit.conns[0].connect()
        await settle(loop)
        assert pool.is_in_state("running")
        # the other slot fails: one backend, so the pool fails with it
        kit.conns[1].emit("error", RuntimeError("refused"))
        await advance(loop, 0.1)
        assert pool.is_in_state("failed")
        await kit.to(t0 + 61)
        assert not kit.conns[0].dead
        assert kit.counter("recycled-age") == 0
        await kit.stop()
    run_vt(body)
