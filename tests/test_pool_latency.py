"""Per-pool latency histograms: what is recorded, what is not, and how it
is published.  Runs on the virtual clock with scripted connections; every
duration is a multiple of 1/1024 s, so it is exact in binary and the
sums can be compared with ==.
"""

import pytest

from cueball_amd import metrics
from cueball_amd.errors import ClaimTimeoutError
from cueball_amd.pool import ConnectionPool
from cueball_amd.resolver import ResolverFSM
from cueball_amd.testing import (DummyConnection, DummyResolver, advance,
                                 settle)
from conftest import run_vt

RECOVERY = {"default": {"timeout": 2000, "retries": 1, "delay": 0}}
SNAP_KEYS = {"count", "sumMs", "minMs", "maxMs", "p50", "p90", "p99", "p999"}


class Ctx:
    """One backend, one connection: claims queue behind each other."""

    def __init__(self, loop, **opts):
        self.loop = loop
        self.connections = []
        self.collector = metrics.create_collector()
        self.resolver = DummyResolver()
        self.resolver_fsm = ResolverFSM(self.resolver, {"loop": loop})
        pool_opts = {
            "domain": "lat.test",
            "constructor": lambda b: DummyConnection(b, self.connections),
            "recovery": RECOVERY,
            "spares": 1,
            "maximum": 1,
            "resolver": self.resolver_fsm,
            "collector": self.collector,
            "loop": loop,
        }
        pool_opts.update(opts)
        self.pool = ConnectionPool(pool_opts)
        self.resolver_fsm.start()

    async def up(self, connect_after=0.0):
        self.resolver.add("b1", {})
        await settle(self.loop)
        assert len(self.connections) == 1
        if connect_after:
            await advance(self.loop, connect_after)
        self.connections[0].connect()
        await settle(self.loop)

    def claim(self, opts=None):
        box = {}

        def cb(err, hdl=None, conn=None):
            box["err"] = err
            box["hdl"] = hdl

        box["ret"] = self.pool.claim(opts or {}, cb)
        return box

    def stats(self):
        return self.pool.get_latency_stats()

    async def stop(self):
        self.pool.stop()
        await advance(self.loop, 10.0)   # outlasts a pending connect
        assert self.pool.is_in_state("stopped")


def test_snapshot_shape_and_no_new_stats_keys():
    async def body(loop):
        ctx = Ctx(loop)
        await ctx.up()
        st = ctx.stats()
        assert set(st) == {"claimWait", "claimHold", "connect"}
        for snap in st.values():
            assert set(snap) == SNAP_KEYS
        assert st["claimWait"]["count"] == 0
        assert st["claimWait"]["p99"] is None
        assert set(ctx.pool.get_stats()) == {
            "counters", "totalConnections", "idleConnections",
            "pendingConnections", "waiterCount"}
        await ctx.stop()

    run_vt(body)


def test_connect_time():
    async def body(loop):
        ctx = Ctx(loop)
        await ctx.up(connect_after=0.5)
        c = ctx.stats()["connect"]
        assert c["count"] == 1
        assert c["sumMs"] == 500.0
        assert c["minMs"] == c["maxMs"] == c["p50"] == 500.0
        await ctx.stop()

    run_vt(body)


def test_failed_connect_not_recorded():
    async def body(loop):
        ctx = Ctx(loop)
        ctx.resolver.add("b1", {})
        await settle(loop)
        ctx.connections[0].emit("error", OSError("refused"))
        await settle(loop)
        assert ctx.stats()["connect"]["count"] == 0
        await ctx.stop()

    run_vt(body)


def test_wait_and_hold():
    async def body(loop):
        ctx = Ctx(loop)
        await ctx.up()

        a = ctx.claim()
        await settle(loop)
        assert a["err"] is None and a["hdl"] is not None
        w = ctx.stats()["claimWait"]
        assert w["count"] == 1 and w["sumMs"] == 0.0
        assert ctx.stats()["claimHold"]["count"] == 0   # still held

        b = ctx.claim()
        await settle(loop)
        assert "hdl" not in b                           # queued behind A
        await advance(loop, 0.25)
        a["hdl"].release()
        await settle(loop)
        assert b["err"] is None and b["hdl"] is not None

        st = ctx.stats()
        assert st["claimWait"]["count"] == 2
        assert st["claimWait"]["sumMs"] == 250.0        # 0 + B's 250
        assert st["claimWait"]["maxMs"] == 250.0
        assert st["claimWait"]["minMs"] == 0.0
        assert st["claimHold"]["count"] == 1
        assert st["claimHold"]["sumMs"] == 250.0        # A's lease

        await advance(loop, 0.125)
        b["hdl"].close()
        await settle(loop)
        st = ctx.stats()
        assert st["claimHold"]["count"] == 2
        assert st["claimHold"]["sumMs"] == 375.0
        assert st["claimWait"]["count"] == 2
        # releasing twice is an error and records nothing more
        with pytest.raises(Exception):
            b["hdl"].release()
        assert ctx.stats()["claimHold"]["count"] == 2
        await ctx.stop()

    run_vt(body)


@pytest.mark.parametrize("opts", [
    {},                                     # pool_claim fast path
    {"timeout": 5000},                      # claim_fast with options
    {"errorOnEmpty": True},                 # ticket slow path
], ids=["pool_claim", "claim_fast", "slow_path"])
def test_every_claim_route_records_the_same(opts):
    async def body(loop):
        ctx = Ctx(loop)
        await ctx.up()
        held = ctx.claim()
        await settle(loop)
        box = ctx.claim(dict(opts))
        await settle(loop)
        await advance(loop, 0.0625)
        held["hdl"].release()
        await settle(loop)
        assert box["err"] is None
        await advance(loop, 0.03125)
        box["hdl"].release()
        await settle(loop)
        st = ctx.stats()
        assert st["claimWait"]["count"] == 2
        assert st["claimWait"]["sumMs"] == 62.5
        assert st["claimHold"]["count"] == 2
        assert st["claimHold"]["sumMs"] == 62.5 + 31.25
        await ctx.stop()

    run_vt(body)


def test_not_recorded():
    async def body(loop):
        ctx = Ctx(loop)
        await ctx.up()
        a = ctx.claim()
        await settle(loop)
        base = ctx.stats()
        assert base["claimWait"]["count"] == 1

        # a claim that times out while queued
        t = ctx.claim({"timeout": 125})
        await advance(loop, 0.25)
        assert isinstance(t["err"], ClaimTimeoutError)
        assert ctx.stats()["claimWait"] == base["claimWait"]

        # a claim cancelled while waiting
        c = ctx.claim()
        await settle(loop)
        c["ret"].cancel()
        await settle(loop)
        a["hdl"].release()
        await settle(loop)
        assert "hdl" not in c
        st = ctx.stats()
        assert st["claimWait"] == base["claimWait"]
        assert st["claimHold"]["count"] == 1
        await ctx.stop()

    run_vt(body)


def test_cancelled_while_claiming_not_recorded():
    """A claim cancelled during the slot handshake still passes through
    'claimed' on its way to 'released'; it was never served, so it
    leaves neither a wait nor a hold behind."""
    import math
    from cueball_amd.connection_fsm import ClaimHandle
    from cueball_amd.events import EventEmitter
    from cueball_amd.latency import PoolLatency
    from cueball_amd.logutil import default_logger

    class FakePool:
        def __init__(self, loop):
            self.p_lat = PoolLatency(loop)

    class FakeSlot:
        """stands still in the handshake: claim() neither accepts nor
        rejects"""
        def is_in_state(self, st):
            return st == "idle"

        def get_state(self):
            return "idle"

        def claim(self, handle):
            pass

    async def body(loop):
        pool = FakePool(loop)
        called = []

        def make():
            return ClaimHandle({
                "pool": pool, "claimStack": [], "log": default_logger(),
                "callback": lambda *a: called.append(a),
                "claimTimeout": math.inf, "loop": loop})

        hdl = make()
        hdl.try_(FakeSlot())
        assert hdl.is_in_state("claiming")
        hdl.cancel()
        await advance(loop, 0.125)
        hdl.accept(EventEmitter())
        await settle(loop)
        assert hdl.is_in_state("released")
        assert called == []
        assert pool.p_lat.wait.count == 0
        assert pool.p_lat.hold.count == 0

        # the same walk without the cancel records both
        hdl = make()
        hdl.try_(FakeSlot())
        await advance(loop, 0.125)
        hdl.accept(EventEmitter())
        assert len(called) == 1
        await advance(loop, 0.25)
        hdl.release()
        await settle(loop)
        assert pool.p_lat.wait.snapshot()["sumMs"] == 125.0
        assert pool.p_lat.hold.snapshot()["sumMs"] == 250.0
        assert pool.p_lat.wait.count == pool.p_lat.hold.count == 1

    run_vt(body)


def test_pinger_claims_not_recorded():
    async def body(loop):
        checked = []

        def do_check(hdl, conn):
            checked.append(conn)
            hdl.release()

        ctx = Ctx(loop, checkTimeout=125, checker=do_check)
        await ctx.up()
        await advance(loop, 0.5)
        assert checked, "the health checker never ran"
        st = ctx.stats()
        assert st["claimWait"]["count"] == 0
        assert st["claimHold"]["count"] == 0
        await ctx.stop()

    run_vt(body)


def test_disabled():
    async def body(loop):
        ctx = Ctx(loop, latencyStats=False)
        await ctx.up()
        a = ctx.claim()
        await settle(loop)
        a["hdl"].release()
        await advance(loop, 1.0)
        assert ctx.stats() is None
        text = ctx.collector.collect()
        assert "cueball_pool_connections" in text
        assert "cueball_claim_" not in text
        assert "cueball_connect_seconds" not in text
        await ctx.stop()

    run_vt(body)
    with pytest.raises(TypeError):
        run_vt(lambda loop: _bad_option(loop))


async def _bad_option(loop):
    Ctx(loop, latencyStats="yes")


def _series(text, name):
    out = {}
    for line in text.splitlines():
        if line.startswith(name + "_bucket{"):
            le = line.split('le="')[1].split('"')[0]
            out[le] = int(line.rsplit(" ", 1)[1])
    return out


def test_published_from_the_lpf_tick():
    async def body(loop):
        ctx = Ctx(loop)
        await ctx.up()
        a = ctx.claim()
        b = ctx.claim()
        await settle(loop)
        await advance(loop, 0.03125)          # B waits 31.25 ms
        a["hdl"].release()
        await settle(loop)
        b["hdl"].release()
        await settle(loop)
        # nothing is published from the claim path
        assert "cueball_claim_wait_seconds_bucket{" not in \
            ctx.collector.collect()

        await advance(loop, 0.25)             # past one 5 Hz LPF tick
        text = ctx.collector.collect()
        assert "# TYPE cueball_claim_wait_seconds histogram" in text
        assert "# TYPE cueball_claim_hold_seconds histogram" in text
        assert "# TYPE cueball_connect_seconds histogram" in text
        wait = _series(text, "cueball_claim_wait_seconds")
        n = ctx.stats()["claimWait"]["count"]
        assert n == 2
        assert wait["+Inf"] == n
        # le = 4**k us in seconds, k = 2..13, then +Inf
        assert list(wait) == [repr(4 ** k / 1e6) for k in range(2, 14)] \
            + ["+Inf"]
        # A waited 0 (under every bound); B's 31250 us is < 65536 us
        # but not < 16384 us
        assert wait[repr(16 / 1e6)] == 1
        assert wait[repr(16384 / 1e6)] == 1
        assert wait[repr(65536 / 1e6)] == 2
        vals = list(wait.values())
        assert vals == sorted(vals)
        # same labels as the connection gauge
        lab = 'domain="lat.test",pool="%s"' % ctx.pool.p_uuid.split("-")[0]
        assert "cueball_claim_wait_seconds_count{%s} 2" % lab in text
        assert "cueball_claim_wait_seconds_sum{%s} 0.03125" % lab in text
        await ctx.stop()

    run_vt(body)


def test_half_open_bound_convention():
    """A sample of exactly 16 us is NOT counted under le=16us: a bound
    L counts rounded-us values < L."""
    from cueball_amd.latency import EXPOSITION_BOUNDS_US, LatencyHistogram
    h = LatencyHistogram()
    h.record(0.015)
    h.record(0.016)
    cum = h.cumulative(EXPOSITION_BOUNDS_US)
    assert cum[0] == 1 and cum[1] == 2


def test_foreign_collector_without_histograms():
    class Foreign:
        """counter-only collector, like a minimal artedi stand-in"""
        def __init__(self):
            self._c = metrics.create_collector()

        def counter(self, **kw):
            return self._c.counter(**kw)

    async def body(loop):
        ctx = Ctx(loop, collector=Foreign())
        await ctx.up()
        a = ctx.claim()
        await settle(loop)
        a["hdl"].release()
        await advance(loop, 0.5)     # LPF ticks must not trip
        assert ctx.stats()["claimWait"]["count"] == 1
        await ctx.stop()

    run_vt(body)


def test_agent_latency_stats():
    from cueball_amd.agent import HttpAgent

    async def body(loop):
        agent = HttpAgent({
            "spares": 1, "maximum": 1, "loop": loop,
            "recovery": RECOVERY,
            "initialDomains": ["127.0.0.1"],
        })
        st = agent.get_latency_stats()
        assert set(st) == {"127.0.0.1"}
        assert set(st["127.0.0.1"]) == {"claimWait", "claimHold", "connect"}
        agent.stop()
        await advance(loop, 3.0)

    run_vt(body)
