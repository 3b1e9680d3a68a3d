"""Shared fixtures of the claim-balancing tests: a pool on a
DummyResolver with a fixed number of connections per backend, whose
idle queue starts out in a known order, and a paced workload whose
leases are held for a time that depends on the backend."""

import asyncio
import gc

from cueball_amd.pool import ConnectionPool
from cueball_amd.resolver import ResolverFSM
from cueball_amd.testing import (DummyConnection, DummyResolver, advance,
                                 settle)

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 0}}

#: the instance variables of a pool created without any opt-in feature
PLAIN_POOL_VARS = {
    "_gauge", "_gauge_labels", "_lat_metrics", "p_backends", "p_busy_hwm",
    "p_check_timeout", "p_checker", "p_claim_log", "p_codel",
    "p_collector", "p_connections", "p_constructor", "p_counters",
    "p_dead", "p_demand_hwm", "p_domain", "p_idleq", "p_in_rebalance",
    "p_initq", "p_keys", "p_last_error", "p_last_rebal_clamped",
    "p_last_rebalance", "p_lastrate", "p_lat", "p_log", "p_lp_timer",
    "p_lpf", "p_max", "p_maxrate", "p_noop_census", "p_rate_delay_timer",
    "p_rebal_scheduled", "p_rebal_timer", "p_recovery", "p_resolver",
    "p_resolver_custom", "p_shuffle_timer", "p_spares",
    "p_started_resolver", "p_total_conns", "p_uuid", "p_waiters"}


def instance_vars(obj, marker="p_uuid"):
    """vars(obj); the native runtime's objects keep their instance dict
    without a ``__dict__`` attribute, so there it is found among the
    object's referents."""
    try:
        return vars(obj)
    except TypeError:
        for ref in gc.get_referents(obj):
            if isinstance(ref, dict) and marker in ref:
                return ref
        raise


def idle_keys(pool):
    return [fsm.csf_backend["key"] for fsm in pool.p_idleq]


class DelayServer:
    """A loopback server that answers after ``delay`` seconds and
    counts what it served.  ``http`` True: a keep-alive HTTP/1.1 server
    answering every request with 200 ``ok``; False: a line echo."""

    def __init__(self, delay=0.0, http=True):
        self.delay = delay
        self.http = http
        self.served = 0
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
        self._writers.add(writer)
        try:
            while True:
                if self.http:
                    data = await reader.readuntil(b"\r\n\r\n")
                else:
                    data = await reader.readline()
                if not data:
                    break
                self.served += 1
                if self.delay:
                    await asyncio.sleep(self.delay)
                if self.http:
                    writer.write(b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\n"
                                 b"Connection: keep-alive\r\n\r\nok")
                else:
                    writer.write(data)
                await writer.drain()
        except (asyncio.IncompleteReadError, ConnectionResetError,
                BrokenPipeError):
            pass
        finally:
            self._writers.discard(writer)
            writer.close()


class Kit:
    """``per`` connections to each of ``backends``; ``spares`` and
    ``maximum`` are both their product, so the pool neither grows nor
    shrinks.  ``lb`` is the ``claimBalancing`` option, None for a pool
    without it.  Sockets connect when ``up()`` says so, round-robin
    over the backends, which is then the order of the idle queue:
    b1, b2, b1, b2."""

    def __init__(self, loop, lb=None, backends=("b1", "b2"), per=2, **opts):
        self.loop = loop
        self.backends = tuple(backends)
        self.per = per
        self.conns = []
        self.pending = []
        self.auto = False
        self.resolver = DummyResolver()

        def constructor(backend):
            c = DummyConnection(backend)
            c.key = backend["key"]
            self.conns.append(c)
            if self.auto:
                loop.call_soon(c.connect)
            else:
                self.pending.append(c)
            return c

        n = len(self.backends) * per
        base = {"constructor": constructor, "recovery": RECOVERY,
                "loop": loop, "domain": "foobar", "spares": n, "maximum": n}
        if lb is not None:
            base["claimBalancing"] = lb
        base.update(opts)
        self.resolver_fsm = ResolverFSM(self.resolver, {"loop": loop})
        base["resolver"] = self.resolver_fsm
        self.pool = ConnectionPool(base)

    async def up(self):
        self.resolver_fsm.start()
        for k in self.backends:
            self.resolver.add(k, {"address": "10.0.0.1", "port": 80})
        await settle(self.loop)
        await advance(self.loop, 0.01)
        assert sorted(c.key for c in self.pending) == \
            sorted(self.backends * self.per)
        nth = {}
        order = []
        for c in self.pending:
            nth[c.key] = nth.get(c.key, 0) + 1
            order.append((nth[c.key], c.key, c))
        order.sort(key=lambda t: t[:2])
        self.pending = []
        self.auto = True
        for _, _, c in order:
            c.connect()
            await settle(self.loop)
        assert idle_keys(self.pool) == list(self.backends) * self.per
        return self

    # -- leases ---------------------------------------------------------
    def claim(self, options=None):
        """One claim; the box fills in when it is served."""
        box = {"at": self.loop.time()}

        def cb(err, hdl=None, conn=None):
            box.update(err=err, hdl=hdl, conn=conn,
                       key=None if conn is None else conn.key)

        box["waiter"] = self.pool.claim(options or {}, cb)
        return box

    async def lease(self, hold_ms, options=None, how="release"):
        """Claim, hold for `hold_ms`, end the lease; returns the key."""
        box = self.claim(options)
        await settle(self.loop)
        assert box.get("err", 1) is None, box
        await advance(self.loop, hold_ms / 1000.0)
        if how == "report":
            box["hdl"].report_failure()
        if how == "close":
            box["hdl"].close()
        else:
            box["hdl"].release()
        await settle(self.loop)
        return box["key"]

    async def lease_on(self, key, hold_ms):
        """A lease of `hold_ms` on backend `key`, steered there with
        ``avoidBackends``."""
        others = [k for k in self.backends if k != key]
        got = await self.lease(hold_ms, {"avoidBackends": others})
        assert got == key
        return got

    async def workload(self, claims, pace_ms, hold_ms, until=None):
        """`claims` claims, one every `pace_ms`; a lease on backend k is
        held ``hold_ms[k]`` and released.  Returns ``(keys in claim
        order, mean ms from claim() to release)``.  `until` may stop
        the run early: it is called with each served key."""
        loop = self.loop
        served = []
        spans = []

        def one():
            t0 = loop.time()

            def cb(err, hdl=None, conn=None):
                assert err is None, err
                served.append((conn.key, loop.time()))

                def done():
                    hdl.release()
                    spans.append((loop.time() - t0) * 1000.0)

                loop.call_later(hold_ms[conn.key] / 1000.0, done)

            self.pool.claim({}, cb)

        for _ in range(claims):
            one()
            await advance(loop, pace_ms / 1000.0)
            if until is not None and served and until(served[-1][0]):
                break
        await advance(loop, max(hold_ms.values()) / 1000.0 + 0.01)
        assert len(spans) == len(served)
        self.served_at = [t for _, t in served]
        return [k for k, _ in served], sum(spans) / len(spans)

    # -- observation ----------------------------------------------------
    def stats(self, key=None):
        st = self.pool.get_balancing_stats()
        return st if key is None else st["backends"][key]

    def outstanding(self):
        return {k: v["outstanding"]
                for k, v in self.stats()["backends"].items()}

    def counter(self, name):
        return self.pool.get_stats()["counters"].get(name, 0)

    async def stop(self):
        self.pool.stop()
        await advance(self.loop, 30.0)
        assert self.pool.is_in_state("stopped")
