"""Connection age over real sockets on the deployment box (run with
-m gpu).

One loopback echo server that counts its accepts and remembers which
peer port sent what.  A pool with a 300 ms ``maxConnectionAge`` serves
back-to-back claims for about 1.5 s: no claim notices the sockets being
replaced underneath it, and the sockets in use at the end are not the
ones in use at the start.
"""

import asyncio

import pytest

pytestmark = pytest.mark.gpu

RUN_SECONDS = 1.5
RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 50,
                        "maxDelay": 200}}


def test_native_runtime_in_use():
    """Recycling must ride on the native claim path, not replace it."""
    from cueball_amd import _speed
    from cueball_amd import fsm, pool
    assert fsm.FSM is _speed.FSM
    assert pool._native_pool_claim is _speed.pool_claim
    assert pool._NativeClaimTicket is _speed.ClaimTicket
    assert pool._NativeSlotDispatch is _speed.SlotDispatch


class EchoServer:
    def __init__(self):
        self.server = None
        self.port = None
        self.writers = set()
        self.accepted = 0
        self.peer_ports = []     # one per accept
        self.served_by = {}      # payload -> peer port

    async def _echo(self, reader, writer):
        self.accepted += 1
        peer = writer.get_extra_info("peername")[1]
        self.peer_ports.append(peer)
        self.writers.add(writer)
        try:
            while True:
                data = await reader.read(1024)
                if not data:
                    break
                self.served_by[data] = peer
                writer.write(data)
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


def test_rolling_replacement_over_real_sockets():
    from cueball_amd.connection import tcp_constructor
    from cueball_amd.pool import ConnectionPool
    from cueball_amd.resolver import StaticIpResolver

    async def main():
        loop = asyncio.get_running_loop()
        server = EchoServer()
        await server.start()
        resolver = StaticIpResolver({
            "backends": [{"address": "127.0.0.1", "port": server.port}],
            "loop": loop,
        })
        pool = ConnectionPool({
            "domain": "age.box",
            "constructor": tcp_constructor(loop=loop),
            "resolver": resolver,
            "recovery": RECOVERY,
            "spares": 2,
            "maximum": 4,
            "maxConnectionAge": 300,
            "connectionAgeSpread": 0.2,
            "loop": loop,
        })
        recycled = []
        pool.on("connectionRecycled",
                lambda key, reason: recycled.append(reason))
        resolver.start()

        async def until(cond, what, seconds=15.0):
            for _ in range(int(seconds / 0.01)):
                if cond():
                    return
                await asyncio.sleep(0.01)
            raise AssertionError("timed out waiting for " + what)

        async def claim_echo(payload):
            """One claim with an echo round trip; any error fails the
            test."""
            hdl, conn = await asyncio.wait_for(
                pool.claim_async({"timeout": 5000}), timeout=10)
            got = loop.create_future()

            def lost(*args):
                if not got.done():
                    got.set_exception(ConnectionError("connection lost"))

            listeners = [
                ("data", conn.on("data", lambda d: (not got.done())
                                 and got.set_result(d))),
                ("error", conn.on("error", lost)),
                ("close", conn.on("close", lost)),
            ]
            try:
                conn.write(payload)
                data = await asyncio.wait_for(got, timeout=5)
            finally:
                for ev, listener in listeners:
                    conn.remove_listener(ev, listener)
            assert data == payload
            hdl.release()

        await until(lambda: pool.get_stats()["idleConnections"] >= 2,
                    "the spares to connect")

        # 1. back-to-back claims while the sockets roll over
        payloads = []
        start = loop.time()
        while loop.time() - start < RUN_SECONDS:
            payload = b"m%d" % len(payloads)
            await claim_echo(payload)
            payloads.append(payload)
        counters = pool.get_stats()["counters"]
        first = {server.served_by[p] for p in payloads[:20]}
        last = {server.served_by[p] for p in payloads[-20:]}
        print("claims", len(payloads), "accepts", server.accepted,
              "recycled-age", counters.get("recycled-age"),
              "first ports", sorted(first), "last ports", sorted(last))
        assert len(payloads) > 40
        assert len(server.served_by) == len(payloads)
        assert server.accepted > 4
        assert first.isdisjoint(last)
        assert counters.get("recycled-age", 0) >= 2
        assert recycled == ["age"] * counters["recycled-age"]
        assert counters.get("claim") == len(payloads)

        # 2. recycle() on the idle pool: both sockets are replaced
        def quiet():
            ages = pool.get_connection_ages()["connections"]
            return len(ages) == 2 and all(
                a["state"] == "idle" and not a["recycling"] for a in ages)

        await until(quiet, "two idle connections and nothing in flight")
        # no await between the check and the call
        before = server.accepted
        assert pool.recycle() == 2
        await until(
            lambda: pool.get_stats()["counters"].get(
                "recycled-manual", 0) == 2
            and server.accepted - before >= 2,
            "two further accepts")
        print("after recycle(): accepts", server.accepted - before,
              "recycled-manual",
              pool.get_stats()["counters"]["recycled-manual"])
        assert server.accepted - before >= 2

        pool.stop()
        await until(lambda: pool.is_in_state("stopped"), "the pool to stop")
        server.kill()
        await asyncio.sleep(0.05)

    asyncio.run(main())
