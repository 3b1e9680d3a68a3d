"""Shared fixtures of the hedge tests, on top of retry_kit's.

For the driver tests on a VirtualLoop: ``Rig``, one HedgeHost and
HedgedTries on it whose attempts are retry_kit's scripted ``FakeTry``s.
For the tests over real sockets: ``hedge_counters`` and ``held``.
"""

import asyncio

from cueball_amd import utils as mod_utils
from cueball_amd.hedge import COUNTERS, HedgedTry, HedgeHost, HedgePolicy
from retry_kit import HOST, ScriptServer, Tries, timers


def policy_of(**hedge):
    return HedgePolicy(mod_utils.assert_hedge_policy({"hedge": hedge}))


class Rig:
    """One HedgeHost on `loop`, and tries on it whose attempts are
    scripted."""

    def __init__(self, loop, **hedge):
        self.loop = loop
        self.policy = policy_of(**hedge)
        self.host = HedgeHost("svc", self.policy, loop.time)
        self.stopped = False
        self.idle = True
        self.idle_asked = []

    def has_idle(self, avoid):
        self.idle_asked.append(avoid)
        return self.idle

    def start(self, method="GET", avoid=(), policy=None):
        tries = Tries()
        ht = HedgedTry(self.loop, policy or self.policy, self.host, method,
                       tries, avoid, self.has_idle, lambda: self.stopped)
        log = []
        ht.on("response", lambda r: log.append(("response", r)))
        ht.on("error", lambda e: log.append(("error", e)))
        ht.on("abort", lambda: log.append(("abort",)))
        ht.on("hedge", lambda ms: log.append(("hedge", ms)))
        ht.start()
        return ht, tries, log

    def counter(self, name):
        return self.host.counters.get(name, 0)

    def counted(self):
        """The counters that are not 0."""
        return {c: n for c, n in self.host.counters.items() if n}

    def assert_clean(self, *all_tries):
        """After every ending: no scheduled handle, both counts 0, no
        armed try, no listener of the driver's left on any attempt."""
        assert timers(self.loop) == []
        assert self.host.active == 0 and self.host.hedging == 0
        assert not self.host.pending
        for tries in all_tries:
            for t in tries.tries:
                assert t.listeners_left() == 0


def hedge_counters(agent):
    """The agent's hedge counters for ``HOST``; all 0 before the host's
    first request."""
    st = agent.get_hedge_stats().get(HOST)
    if st is None:
        return dict.fromkeys(COUNTERS, 0)
    return st["counters"]


async def held_server():
    """A server that holds every request until the event is set."""
    release = asyncio.Event()
    server = await ScriptServer(default=("hold", release)).start()
    return server, release
