"""Shared fixtures of the outlier-detection tests: a pool on a
DummyResolver whose connections connect by themselves, with helpers to
take a lease on a chosen backend and to end it in a chosen way."""

import gc

from cueball_amd.pool import ConnectionPool
from cueball_amd.resolver import ResolverFSM
from cueball_amd.testing import (DummyConnection, DummyResolver, advance,
                                 settle)

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 0}}
BASE = 1000
OD = {"consecutiveFailures": 2, "baseEjectionTime": BASE,
      "maxEjectionTime": 5000}


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


class Kit:
    """A pool on a DummyResolver whose connections connect by
    themselves, except to the backends named in ``down``, which refuse.
    ``conns`` keeps every connection ever constructed; ``events`` every
    ejection and reinstatement with its virtual time."""

    def __init__(self, loop, backends=("b1", "b2", "b3"), od=OD, **opts):
        self.loop = loop
        self.conns = []
        self.down = set()
        self.events = []
        self.served = []
        self.pings = []
        self.resolver = DummyResolver()

        def constructor(backend):
            c = DummyConnection(backend)
            c.key = backend["key"]
            self.conns.append(c)
            if c.key in self.down:
                loop.call_soon(c.emit, "error", Exception("refused"))
            else:
                loop.call_soon(c.connect)
            return c

        base = {"constructor": constructor, "recovery": RECOVERY,
                "loop": loop, "domain": "foobar", "spares": 2,
                "maximum": 4}
        if od is not None:
            base["outlierDetection"] = dict(od)
        base.update(opts)
        self.resolver_fsm = ResolverFSM(self.resolver, {"loop": loop})
        base["resolver"] = self.resolver_fsm
        self.pool = ConnectionPool(base)
        self.pool.on("backendEjected", lambda key, info: self.events.append(
            ("ejected", key, dict(info), loop.time())))
        self.pool.on("backendReinstated", lambda key, why:
                     self.events.append(("reinstated", key, why,
                                         loop.time())))
        self.resolver_fsm.start()
        for k in backends:
            if isinstance(k, str):
                k = (k, {})
            self.resolver.add(k[0], dict({"address": "10.0.0.1",
                                          "port": 80}, **k[1]))

    # -- leases ---------------------------------------------------------
    async def claim(self):
        """One claim; the box is empty if nothing served it yet."""
        box = {}

        def cb(err, hdl=None, conn=None):
            assert err is None, err
            box.update(hdl=hdl, conn=conn, key=conn.key,
                       ejected=set(self.ejected()))
            self.served.append(conn.key)
            # the claimer listens for errors, as a real one must
            box["on_error"] = conn.on("error", lambda e: None)

        box["waiter"] = self.pool.claim({"timeout": 10_000}, cb)
        await settle(self.loop)
        if "hdl" not in box:
            await advance(self.loop, 0.01)
        return box

    async def lease_on(self, key):
        """A lease on backend `key`.  Leases that land elsewhere on the
        way are held and then released: other backends may see
        successes, `key` sees nothing."""
        held = []
        try:
            for _ in range(4):
                box = await self.claim()
                assert "hdl" in box, "claim was not served"
                if box["key"] == key:
                    return box
                held.append(box)
            raise AssertionError("no lease on %s" % key)
        finally:
            for box in held:
                await self.end(box, "release")

    async def end(self, box, how):
        """End a lease: release, close, report (report_failure, then
        release), error or sockclose (the socket fails or closes under
        the lease, which is then released)."""
        hdl, conn = box["hdl"], box["conn"]
        if how == "error":
            conn.emit("error", Exception("boom"))
        elif how == "sockclose":
            conn.emit("close")
        elif how == "report":
            hdl.report_failure()
        if how in ("error", "sockclose"):
            await settle(self.loop)
        conn.remove_listener("error", box["on_error"])
        if how == "close":
            hdl.close()
        else:
            hdl.release()
        await settle(self.loop)
        await advance(self.loop, 0.01)

    async def fail_on(self, key, times=1, how="close"):
        for _ in range(times):
            await self.end(await self.lease_on(key), how)

    # -- observation ----------------------------------------------------
    def stats(self, key=None):
        st = self.pool.get_outlier_stats()
        return st if key is None else st["backends"][key]

    def streak(self, key):
        return self.stats(key)["consecutiveFailures"]

    def ejected(self):
        return sorted(k for k, v in self.stats()["backends"].items()
                      if v["ejected"])

    def counter(self, name):
        return self.pool.get_stats()["counters"].get(name, 0)

    def slots(self, key):
        return list(self.pool.p_connections.get(key, ()))

    def live(self, key):
        return [c for c in self.conns if c.key == key and not c.dead]

    def od_timers(self):
        return [h for h in self.loop._scheduled
                if not h._cancelled and "_od_expired" in repr(h)]

    async def to(self, t):
        """Advance to the absolute virtual time `t`, exactly."""
        await advance(self.loop, t - self.loop.time())

    async def stop(self):
        self.pool.stop()
        await advance(self.loop, 30.0)
        assert self.pool.is_in_state("stopped")
