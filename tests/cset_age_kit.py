"""Helpers for the ConnectionSet connection-age tests: a set on a
DummyResolver with a consumer that records the added/removed contract.
Not a test module."""

import asyncio
import gc

from cueball_amd.connection_set import ConnectionSet
from cueball_amd.testing import (DummyConnection, DummyResolver, advance,
                                 settle)

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
            if isinstance(ref, dict) and ref.get("cs_uuid") == obj.cs_uuid:
                return ref
        raise


async def leap(loop, seconds):
    """Move the virtual clock ahead without visiting every timer on the
    way: each timer that is overdue then fires once."""
    loop._vt_set(loop.time() + seconds)
    await asyncio.sleep(0)
    await settle(loop)


class Kit:
    """A set on a DummyResolver.  ``conns`` keeps every connection ever
    constructed, in order.  ``log`` is the consumer's view: "added
    b1.1", "removed b1.1", ... in the order the events arrived.  With
    ``hold`` the consumer keeps the handle on 'removed' (in ``held``)
    instead of releasing it at once.  ``low`` is the smallest number of
    advertised connections seen at any event since the first 'added'."""

    def __init__(self, loop, backends=("b1",), hold=False, **opts):
        self.loop = loop
        self.conns = []
        self.log = []
        self.advertised = {}   # ckey -> (conn, hdl)
        self.held = []         # (ckey, conn, hdl) removed, not released
        self.hold = hold
        self.recycled = []     # (key, reason)
        self.failed = []       # (key, reason)
        self.low = None
        self.resolver = DummyResolver()

        def constructor(backend):
            c = DummyConnection(backend)
            c.key = backend["key"]
            self.conns.append(c)
            return c

        base = {"constructor": constructor, "recovery": RECOVERY,
                "loop": loop, "target": 1, "maximum": 1,
                "resolver": self.resolver}
        base.update(opts)
        if base.get("maxConnectionAge") is not None:
            base.setdefault("connectionAgeSpread", 0)
        self.cset = ConnectionSet(base)
        self.cset.on("added", self._on_added)
        self.cset.on("removed", self._on_removed)
        self.cset.on("connectionRecycled",
                     lambda key, reason: self.recycled.append((key, reason)))
        self.cset.on("connectionRecycleFailed",
                     lambda key, reason: self.failed.append((key, reason)))
        self.resolver.start()
        for k in backends:
            self.resolver.add(k, {})

    def sample(self):
        n = len(self.cset.get_connections())
        if self.low is None or n < self.low:
            self.low = n

    def _on_added(self, ckey, conn, hdl):
        assert ckey not in self.advertised
        self.advertised[ckey] = (conn, hdl)
        self.log.append("added " + ckey)
        self.sample()

    def _on_removed(self, ckey, conn, hdl):
        assert self.advertised.pop(ckey)[0] is conn
        self.log.append("removed " + ckey)
        self.sample()
        if self.hold:
            self.held.append((ckey, conn, hdl))
        else:
            hdl.release()

    def of(self, key, live=True):
        """Connections constructed for backend `key`; with ``live``
        only those not destroyed."""
        return [c for c in self.conns
                if c.key == key and not (live and c.dead)]

    def pending(self):
        return [c for c in self.conns if not c.connected and not c.dead]

    async def connect_new(self):
        for c in self.pending():
            c.connect()
        await settle(self.loop)

    async def to(self, t):
        """Advance to the absolute virtual time `t`, exactly."""
        await advance(self.loop, t - self.loop.time())

    def counter(self, name):
        return self.cset.get_stats()["counters"].get(name, 0)

    def ages(self):
        return self.cset.get_connection_ages()["connections"]

    async def stop(self):
        self.cset.stop()
        # long enough for a slot that is still connecting to give up
        await advance(self.loop, 30.0)
        assert self.cset.is_in_state("stopped")
