"""Pools, sets and agents with ``srvRanking``: connections live on the
lowest reachable SRV priority, spread by weight; the pool fails over
when a whole tier is declared dead and fails back when a monitor
reconnects.  With the option off, rank fields change nothing."""

import asyncio
import logging

import pytest

from cueball_amd.agent import HttpAgent
from cueball_amd.connection_set import ConnectionSet
from cueball_amd.errors import PoolFailedError
from cueball_amd.logutil import CueballLogger
from cueball_amd.pool import ConnectionPool
from cueball_amd.resolver import ResolverFSM
from cueball_amd.testing import (DummyConnection, DummyResolver, advance,
                                 settle)
from conftest import run_vt

# retries=1: the first failed connect declares the backend dead
RECOVERY = {"default": {"timeout": 500, "retries": 1, "delay": 0}}

TWO_PLUS_STANDBY = {
    "p1": {"priority": 0, "weight": 1},
    "p2": {"priority": 0, "weight": 1},
    "s1": {"priority": 10, "weight": 1},
}


class Kit:
    """A pool (or set) on a DummyResolver with tracked connections."""

    def __init__(self, loop, backends, cset=False, **opts):
        self.loop = loop
        self.connections = []
        self.resolver = DummyResolver()
        self.prio_events = []
        self.added = []

        def constructor(backend):
            c = DummyConnection(backend)
            c.backend = backend.get("key")
            self.connections.append(c)
            orig_destroy = c.destroy

            def destroy():
                if c in self.connections:
                    self.connections.remove(c)
                orig_destroy()

            c.destroy = destroy
            return c

        base = {"constructor": constructor, "recovery": RECOVERY,
                "loop": loop}
        base.update(opts)
        if cset:
            base.setdefault("target", 3)
            base.setdefault("maximum", 4)
            base["resolver"] = self.resolver
            self.obj = ConnectionSet(base)

            def on_added(ckey, conn, hdl):
                # a set's consumer owns error handling on its connections
                conn.on("error", lambda err: None)
                self.added.append(conn)

            self.obj.on("added", on_added)
            self.obj.on("removed", lambda ck, conn, hdl: hdl.release())
            self.resolver.start()
        else:
            base.setdefault("spares", 2)
            base.setdefault("maximum", 4)
            base["domain"] = "foobar"
            self.resolver_fsm = ResolverFSM(self.resolver, {"loop": loop})
            base["resolver"] = self.resolver_fsm
            self.obj = ConnectionPool(base)
            self.resolver_fsm.start()
        self.obj.on("priorityChanged",
                    lambda old, new: self.prio_events.append((old, new)))
        for k, b in backends.items():
            self.resolver.add(k, b)

    def counts(self):
        out = {}
        for c in self.connections:
            out[c.backend] = out.get(c.backend, 0) + 1
        return out

    def by_backend(self, key):
        return [c for c in self.connections if c.backend == key]

    async def connect_all(self):
        for c in list(self.connections):
            if not c.connected:
                c.connect()
        await settle(self.loop)

    async def kill(self, key):
        """Fail every connection to `key`, reconnect attempts included,
        as a host going away does, until it is declared dead."""
        for _ in range(4):
            for c in self.by_backend(key):
                c.emit("error", RuntimeError("host down"))
            await advance(self.loop, 0.1)
            if self.obj.is_declared_dead(key):
                return
        raise AssertionError("%s was not declared dead" % key)

    def claim(self):
        box = {}

        def cb(err, hdl=None, conn=None):
            box.update(err=err, hdl=hdl, conn=conn)

        self.obj.claim({"timeout": 1000}, cb)
        return box


def test_option_must_be_bool():
    async def body(loop):
        for bad in (1, "true", 0):
            with pytest.raises(TypeError):
                Kit(loop, {}, srvRanking=bad)
            with pytest.raises(TypeError):
                Kit(loop, {}, cset=True, srvRanking=bad)
    run_vt(body)


def test_pool_fails_over_to_standby_and_back(caplog):
    async def body(loop):
        log = CueballLogger(logging.getLogger("srv-ranking-test"))
        kit = Kit(loop, TWO_PLUS_STANDBY, srvRanking=True, log=log)
        pool = kit.obj
        await settle(loop)
        # all connections on the primaries
        assert kit.counts() == {"p1": 1, "p2": 1}
        await kit.connect_all()
        assert pool.is_in_state("running")
        rk = pool.get_ranking()
        assert rk["enabled"] is True
        assert rk["activePriority"] == 0
        assert [t["priority"] for t in rk["tiers"]] == [0, 10]
        assert rk["tiers"][0] == {
            "priority": 0, "backends": 2, "dead": 0, "connections": 2,
            "weights": {"p1": 1, "p2": 1}}
        assert rk["tiers"][1] == {
            "priority": 10, "backends": 1, "dead": 0, "connections": 0,
            "weights": {"s1": 1}}
        assert kit.prio_events == []

        # one primary dead: the tier stays active, its share moves to
        # the other primary, nothing on the standby
        await kit.kill("p1")
        assert pool.is_declared_dead("p1")
        assert kit.counts() == {"p1": 1, "p2": 2}
        assert kit.prio_events == []
        for c in kit.by_backend("p2"):
            if not c.connected:
                c.connect()
        await settle(loop)

        # both dead: fail over
        await kit.kill("p2")
        assert pool.is_declared_dead("p2")
        assert kit.prio_events == [(0, 10)]
        # one monitor per dead primary plus the spares on the standby
        assert kit.counts() == {"p1": 1, "p2": 1, "s1": 2}
        assert not pool.is_in_state("failed")
        for c in kit.by_backend("s1"):
            c.connect()
        await settle(loop)
        assert pool.is_in_state("running")
        box = kit.claim()
        await settle(loop)
        assert box["err"] is None
        assert box["conn"].backend == "s1"
        box["hdl"].release()
        await settle(loop)
        rk = pool.get_ranking()
        assert rk["activePriority"] == 10
        assert rk["tiers"][0]["dead"] == 2
        assert rk["tiers"][0]["connections"] == 2   # the monitors
        assert rk["tiers"][1]["connections"] == 2

        # a monitor connects: fail back, standby connections drain
        await advance(loop, 1.0)
        mon = [c for c in kit.by_backend("p1") if not c.connected][0]
        mon.connect()
        await advance(loop, 0.1)
        assert kit.prio_events == [(0, 10), (10, 0)]
        assert not pool.is_declared_dead("p1")
        assert kit.counts().get("s1", 0) == 0
        assert kit.counts()["p1"] == 2      # its own slot + p2's share
        assert kit.counts()["p2"] == 1      # still monitored
        assert pool.get_ranking()["activePriority"] == 0
        assert pool.is_in_state("running")
        pool.stop()
        await advance(loop, 1.0)

    with caplog.at_level(logging.INFO, logger="srv-ranking-test"):
        run_vt(body)
    msgs = [r.getMessage() for r in caplog.records]
    # the logger appends its bound fields in brackets
    assert [m.split(" [")[0] for m in msgs if "priority" in m] == [
        "failing over to priority 10", "failing back to priority 0"]


def test_changed_moves_the_spread_without_removing_backends():
    async def body(loop):
        kit = Kit(loop, {"a": {"priority": 0, "weight": 1},
                         "b": {"priority": 0, "weight": 1}},
                  srvRanking=True, spares=4, maximum=4)
        removed = []
        kit.resolver.on("removed", removed.append)
        await settle(loop)
        await kit.connect_all()
        assert kit.counts() == {"a": 2, "b": 2}

        kit.resolver.change("a", weight=3)
        await settle(loop)
        await kit.connect_all()
        assert kit.counts() == {"a": 3, "b": 1}
        assert removed == []
        assert kit.obj.p_backends["a"]["weight"] == 3
        assert kit.obj.get_ranking()["tiers"][0]["weights"] == \
            {"a": 3, "b": 1}
        assert kit.prio_events == []
        kit.obj.stop()
        await advance(loop, 1.0)
    run_vt(body)


def test_changed_is_ignored_with_the_option_off():
    async def body(loop):
        kit = Kit(loop, {"a": {"priority": 0, "weight": 1},
                         "b": {"priority": 0, "weight": 1}},
                  spares=4, maximum=4)
        await settle(loop)
        await kit.connect_all()
        assert kit.counts() == {"a": 2, "b": 2}
        kit.resolver.change("a", weight=3)
        kit.resolver.change("b", priority=10)
        await advance(loop, 0.5)
        assert kit.counts() == {"a": 2, "b": 2}
        assert kit.obj.p_backends["a"]["weight"] == 1
        assert kit.obj.get_ranking() == {"enabled": False}
        kit.obj.stop()
        await advance(loop, 1.0)
    run_vt(body)


def test_option_off_spreads_ranked_backends_evenly():
    async def body(loop):
        kit = Kit(loop, {"p1": {"priority": 0, "weight": 30},
                         "p2": {"priority": 0, "weight": 10},
                         "s1": {"priority": 10, "weight": 1}},
                  spares=3, maximum=6)
        await settle(loop)
        assert kit.counts() == {"p1": 1, "p2": 1, "s1": 1}
        assert kit.prio_events == []
        kit.obj.stop()
        await advance(loop, 1.0)
    run_vt(body)


def test_all_tiers_dead_fails_the_pool():
    async def body(loop):
        kit = Kit(loop, TWO_PLUS_STANDBY, srvRanking=True)
        pool = kit.obj
        await settle(loop)
        await kit.connect_all()
        await kit.kill("p1")
        await kit.kill("p2")
        assert not pool.is_in_state("failed")
        assert kit.counts().get("s1") == 2
        await kit.kill("s1")
        assert pool.is_in_state("failed")
        box = kit.claim()
        await settle(loop)
        assert isinstance(box["err"], PoolFailedError)
        # everything dead: back on the lowest priority present
        assert pool.get_ranking()["activePriority"] == 0
        pool.stop()
        # the monitors are mid-connect: fail them so their slots stop
        for c in list(kit.connections):
            c.emit("error", RuntimeError("host down"))
        await advance(loop, 5.0)
        assert pool.is_in_state("stopped")
    run_vt(body)


def test_cset_leaves_standby_alone_while_a_primary_lives():
    async def body(loop):
        kit = Kit(loop, TWO_PLUS_STANDBY, cset=True, srvRanking=True)
        cset = kit.obj
        await settle(loop)
        # target 3 would take all three backends without ranking
        assert kit.counts() == {"p1": 1, "p2": 1}
        await kit.connect_all()
        assert sorted(c.backend for c in kit.added) == ["p1", "p2"]
        rk = cset.get_ranking()
        assert rk["activePriority"] == 0
        assert rk["tiers"][1]["connections"] == 0

        await kit.kill("p1")
        assert "s1" not in kit.counts()
        assert sorted(c.backend for c in kit.added) == ["p1", "p2"]

        await kit.kill("p2")
        assert kit.prio_events == [(0, 10)]
        assert kit.counts().get("s1") == 1
        kit.by_backend("s1")[0].connect()
        await settle(loop)
        assert [c.backend for c in kit.added][-1] == "s1"
        assert cset.get_ranking()["activePriority"] == 10
        cset.stop()
        await advance(loop, 1.0)
    run_vt(body)


def test_cset_option_off_uses_every_backend():
    async def body(loop):
        kit = Kit(loop, TWO_PLUS_STANDBY, cset=True)
        await settle(loop)
        assert kit.counts() == {"p1": 1, "p2": 1, "s1": 1}
        assert kit.obj.get_ranking() == {"enabled": False}
        kit.obj.stop()
        await advance(loop, 1.0)
    run_vt(body)


def test_agent_passes_the_option_through(monkeypatch):
    from cueball_amd import agent as mod_agent
    configs = []
    real = mod_agent.resolver_for_ip_or_domain

    def spy(args):
        configs.append(args["resolverConfig"])
        return real(args)

    monkeypatch.setattr(mod_agent, "resolver_for_ip_or_domain", spy)

    async def body():
        recovery = {"default": {"timeout": 200, "retries": 1, "delay": 0}}
        with pytest.raises(TypeError):
            HttpAgent({"defaultPort": 1, "recovery": recovery,
                       "spares": 1, "maximum": 1, "srvRanking": "yes"})
        off = HttpAgent({"defaultPort": 1, "recovery": recovery,
                         "spares": 1, "maximum": 1,
                         "initialDomains": ["127.0.0.1"]})
        on = HttpAgent({"defaultPort": 1, "recovery": recovery,
                        "spares": 1, "maximum": 1, "srvRanking": True,
                        "initialDomains": ["127.0.0.1"]})
        try:
            assert off.get_pool("127.0.0.1").get_ranking() == \
                {"enabled": False}
            assert on.get_pool("127.0.0.1").get_ranking()["enabled"]
            # ...and the config of the resolvers the agents build
            assert "srvRanking" not in configs[0]
            assert configs[1]["srvRanking"] is True
        finally:
            for agent in (off, on):
                fut = asyncio.get_running_loop().create_future()
                agent.stop(lambda err, f=fut: f.set_result(err))
                await asyncio.wait_for(fut, 10)

    loop = asyncio.new_event_loop()
    try:
        loop.run_until_complete(body())
    finally:
        loop.close()


def test_active_priority_gauge_follows_failover():
    async def body(loop):
        kit = Kit(loop, TWO_PLUS_STANDBY, srvRanking=True)
        pool = kit.obj
        await settle(loop)
        await kit.connect_all()
        await advance(loop, 0.3)     # one 5 Hz sample
        gauge = pool.p_collector.get_collector(
            "cueball_pool_active_priority")
        labels = {"pool": pool.p_uuid.split("-")[0], "domain": "foobar"}
        assert gauge.value(labels) == 0
        await kit.kill("p1")
        await kit.kill("p2")
        await advance(loop, 0.3)
        assert gauge.value(labels) == 10
        assert "cueball_pool_active_priority" in pool.p_collector.collect()
        pool.stop()
        await advance(loop, 1.0)

        plain = Kit(loop, TWO_PLUS_STANDBY)
        await advance(loop, 0.3)
        assert "cueball_pool_active_priority" not in \
            plain.obj.p_collector.collect()
        plain.obj.stop()
        await advance(loop, 1.0)
    run_vt(body)


def test_pool_hands_the_option_to_its_own_resolver(monkeypatch):
    from cueball_amd import resolver as mod_resolver
    from cueball_amd.testing import dummy_resolver_factory
    seen = []
    factory = dummy_resolver_factory([])

    def spy(options):
        seen.append(options.get("srvRanking"))
        return factory(options)

    monkeypatch.setattr(mod_resolver, "Resolver", spy)

    async def body(loop):
        for flag in (True, False):
            opts = {"domain": "svc.test", "recovery": RECOVERY,
                    "spares": 1, "maximum": 1, "loop": loop,
                    "constructor": lambda b: DummyConnection(b)}
            if flag:
                opts["srvRanking"] = True
            pool = ConnectionPool(opts)
            await settle(loop)
            pool.stop()
            await advance(loop, 1.0)
    run_vt(body)
    assert seen == [True, False]
