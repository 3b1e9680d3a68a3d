"""Connection age on a ConnectionSet over real sockets on the deployment
box (run with -m gpu).

Two loopback echo servers that count their accepts and remember which
socket carried which payload.  A set with ``target: 2`` and a 300 ms
``maxConnectionAge`` feeds a small multiplexing consumer for about
1.5 s: every payload comes back exactly once, the consumer never has
fewer than two usable connections while the sockets are replaced
underneath it, and the sockets in use at the end are not the ones in
use at the start.
"""

import asyncio

import pytest

pytestmark = pytest.mark.gpu

RUN_SECONDS = 1.5
RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 50,
                        "maxDelay": 200}}


def test_native_runtime_in_use():
    """The set's slots, handles and FSMs are the native ones."""
    from cueball_amd import _speed
    from cueball_amd import connection_fsm, connection_set, fsm
    assert fsm.FSM is _speed.FSM
    assert connection_fsm._SlotKit is _speed.SlotKit
    assert issubclass(connection_fsm.ClaimHandle, _speed.ClaimHandleBase)
    assert issubclass(connection_set.ConnectionSet, _speed.FSM)
    assert issubclass(connection_set.LogicalConnection, _speed.FSM)


class EchoServer:
    """Echoes newline-framed payloads; ``served_by`` maps a payload to
    the (server port, peer port) of the socket it came in on."""

    def __init__(self):
        self.server = None
        self.port = None
        self.writers = set()
        self.accepted = 0
        self.served_by = {}
        self.duplicates = []

    async def _echo(self, reader, writer):
        self.accepted += 1
        peer = (self.port, writer.get_extra_info("peername")[1])
        self.writers.add(writer)
        try:
            while True:
                line = await reader.readline()
                if not line:
                    break
                if line in self.served_by:
                    self.duplicates.append(line)
                self.served_by[line] = peer
                writer.write(line)
                await writer.drain()
        except ConnectionError:
            pass
        finally:
            self.writers.discard(writer)
            writer.close()

    async def start(self):
        self.server = await asyncio.start_server(
            self._echo, "127.0.0.1", 0)
        self.port = self.server.sockets[0].getsockname()[1]

    def kill(self):
        self.server.close()
        for w in list(self.writers):
            w.close()


class Mux:
    """A multiplexing consumer: numbered payloads go round-robin over
    whatever is advertised, several in flight per connection.  On
    'removed' it stops sending on that connection and releases the
    handle once the echoes still in flight are back."""

    def __init__(self, cset):
        self.links = {}        # ckey -> link dict
        self.added = []
        self.removed = []
        self.echoed = {}       # payload -> times echoed
        self.errors = []
        self.turn = 0
        cset.on("added", self.on_added)
        cset.on("removed", self.on_removed)

    def usable(self):
        return [ln for ln in self.links.values() if not ln["draining"]]

    def on_added(self, ckey, conn, hdl):
        link = {"ckey": ckey, "conn": conn, "hdl": hdl, "inflight": 0,
                "draining": False, "buf": b""}

        def lost(*args):
            self.errors.append((ckey, "lost", args))

        link["listeners"] = [
            ("data", conn.on("data", lambda d: self.on_data(link, d))),
            ("error", conn.on("error", lost)),
            ("close", conn.on("close", lost)),
        ]
        self.links[ckey] = link
        self.added.append(ckey)

    def on_removed(self, ckey, conn, hdl):
        self.removed.append(ckey)
        link = self.links[ckey]
        link["draining"] = True
        if link["inflight"] == 0:
            self.finish(link)

    def finish(self, link):
        for ev, listener in link["listeners"]:
            link["conn"].remove_listener(ev, listener)
        del self.links[link["ckey"]]
        link["hdl"].release()

    def on_data(self, link, data):
        lines = (link["buf"] + data).split(b"\n")
        link["buf"] = lines.pop()
        for line in lines:
            payload = line + b"\n"
            self.echoed[payload] = self.echoed.get(payload, 0) + 1
            link["inflight"] -= 1
        if link["draining"] and link["inflight"] == 0:
            self.finish(link)

    def send(self, payload):
        usable = self.usable()
        link = usable[self.turn % len(usable)]
        self.turn += 1
        link["inflight"] += 1
        link["conn"].write(payload)
        return len(usable)


def test_make_before_break_over_real_sockets():
    from cueball_amd.connection import tcp_constructor
    from cueball_amd.connection_set import ConnectionSet
    from cueball_amd.resolver import StaticIpResolver

    async def main():
        loop = asyncio.get_running_loop()
        servers = [EchoServer(), EchoServer()]
        for server in servers:
            await server.start()
        resolver = StaticIpResolver({
            "backends": [{"address": "127.0.0.1", "port": s.port}
                         for s in servers],
            "loop": loop,
        })
        cset = ConnectionSet({
            "domain": "cset.age.box",
            "constructor": tcp_constructor(loop=loop),
            "resolver": resolver,
            "recovery": RECOVERY,
            "target": 2,
            "maximum": 2,
            "maxConnectionAge": 300,
            "connectionAgeSpread": 0.2,
            "loop": loop,
        })
        mux = Mux(cset)
        recycled = []
        cset.on("connectionRecycled",
                lambda key, reason: recycled.append(reason))
        failed = []
        cset.on("connectionRecycleFailed",
                lambda key, reason: failed.append((key, reason)))
        resolver.start()

        async def until(cond, what, seconds=15.0):
            for _ in range(int(seconds / 0.01)):
                if cond():
                    return
                await asyncio.sleep(0.01)
            raise AssertionError("timed out waiting for " + what)

        def counters():
            return cset.get_stats()["counters"]

        def served_by(payload):
            for server in servers:
                if payload in server.served_by:
                    return server.served_by[payload]
            raise AssertionError("no server saw %r" % payload)

        await until(lambda: len(mux.added) >= 2,
                    "both backends to be advertised")

        # 1. multiplexed traffic while the sockets roll over
        payloads = []
        fewest = None
        start = loop.time()
        while loop.time() - start < RUN_SECONDS:
            payload = b"m%07d\n" % len(payloads)
            usable = mux.send(payload)
            payloads.append(payload)
            if fewest is None or usable < fewest:
                fewest = usable
            await asyncio.sleep(0.002)
        await until(lambda: len(mux.echoed) == len(payloads),
                    "the last echoes")
        first = {served_by(p) for p in payloads[:20]}
        last = {served_by(p) for p in payloads[-20:]}
        print("payloads", len(payloads), "fewest usable", fewest,
              "accepts", [s.accepted for s in servers],
              "recycled-age", counters().get("recycled-age"),
              "first sockets", sorted(first), "last sockets", sorted(last))
        assert len(payloads) > 40
        assert mux.errors == []
        assert failed == []
        assert sorted(mux.echoed) == sorted(payloads)
        assert all(n == 1 for n in mux.echoed.values())
        assert sum(len(s.served_by) for s in servers) == len(payloads)
        assert all(s.duplicates == [] for s in servers)
        assert fewest >= 2
        assert all(s.accepted > 1 for s in servers)
        assert first.isdisjoint(last)
        assert counters().get("recycled-age", 0) >= 2
        assert recycled == ["age"] * counters()["recycled-age"]
        # the successor was always 'added' before its predecessor was
        # 'removed'
        for ckey in mux.removed:
            backend, serial = ckey.rsplit(".", 1)
            later = [ck for ck in mux.added
                     if ck.rsplit(".", 1)[0] == backend and
                     int(ck.rsplit(".", 1)[1]) > int(serial)]
            assert later, ckey

        # 2. recycle() on the quiet set: both sockets are replaced
        def quiet():
            ages = cset.get_connection_ages()["connections"]
            return len(ages) == 2 and len(mux.usable()) == 2 and all(
                a["ckey"] is not None and not a["recycling"] for a in ages)

        await until(quiet, "two advertised connections, nothing recycling")
        # no await between the check and the call
        before = sum(s.accepted for s in servers)
        assert cset.recycle() == 2
        await until(
            lambda: counters().get("recycled-manual", 0) == 2
            and sum(s.accepted for s in servers) - before >= 2,
            "two further accepts")
        print("after recycle(): accepts",
              sum(s.accepted for s in servers) - before,
              "recycled-manual", counters()["recycled-manual"])
        assert sum(s.accepted for s in servers) - before >= 2
        assert counters()["recycled-manual"] == 2
        assert mux.errors == []

        cset.stop()
        await until(lambda: cset.is_in_state("stopped"), "the set to stop")
        assert mux.links == {}
        assert len(mux.added) == len(mux.removed)
        for server in servers:
            server.kill()
        await asyncio.sleep(0.05)

    asyncio.run(main())
