"""SRV ranking over real sockets on the deployment box (run with -m gpu).

Three loopback echo servers behind a static resolver, two at priority 0
and a standby at priority 10.  Claims stay off the standby while a
primary lives, keep succeeding through it once both primaries are gone,
and return to the primaries when their ports come back.
"""

import asyncio

import pytest

pytestmark = pytest.mark.gpu

N_CLAIMS = 300
# about 2 retries 50 ms apart before a backend is declared dead; the
# monitors of a dead backend then knock every 200 ms at the most
RECOVERY = {"default": {"timeout": 500, "retries": 2, "delay": 50,
                        "maxDelay": 200}}


def test_native_runtime_in_use():
    """Ranking must ride on the native claim path, not replace it."""
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

    async def _echo(self, reader, writer):
        self.accepted += 1
        self.writers.add(writer)
        try:
            while True:
                data = await reader.read(1024)
                if not data:
                    break
                writer.write(data)
                await writer.drain()
        except ConnectionError:
            pass
        finally:
            self.writers.discard(writer)
            writer.close()

    async def start(self):
        self.server = await asyncio.start_server(
            self._echo, "127.0.0.1", self.port or 0)
        self.port = self.server.sockets[0].getsockname()[1]

    def kill(self):
        """Stop listening and drop every open connection."""
        self.server.close()
        for w in list(self.writers):
            w.close()


def test_failover_and_failback_over_real_sockets():
    from cueball_amd.connection import tcp_constructor
    from cueball_amd.pool import ConnectionPool
    from cueball_amd.resolver import StaticIpResolver

    async def main():
        loop = asyncio.get_running_loop()
        primaries = [EchoServer(), EchoServer()]
        standby = EchoServer()
        for s in primaries + [standby]:
            await s.start()

        resolver = StaticIpResolver({
            "backends": [
                {"address": "127.0.0.1", "port": primaries[0].port,
                 "priority": 0, "weight": 1},
                {"address": "127.0.0.1", "port": primaries[1].port,
                 "priority": 0, "weight": 1},
                {"address": "127.0.0.1", "port": standby.port,
                 "priority": 10, "weight": 1}],
            "loop": loop,
        })
        pool = ConnectionPool({
            "domain": "ranking.box",
            "constructor": tcp_constructor(loop=loop),
            "resolver": resolver,
            "recovery": RECOVERY,
            "spares": 2,
            "maximum": 4,
            "srvRanking": True,
            "loop": loop,
        })
        prio_events = []
        pool.on("priorityChanged",
                lambda old, new: prio_events.append((old, new)))
        resolver.start()

        async def until(cond, what, seconds=15.0):
            for _ in range(int(seconds / 0.01)):
                if cond():
                    return
                await asyncio.sleep(0.01)
            raise AssertionError("timed out waiting for " + what)

        async def claim_echo(payload):
            """One claim with an echo round trip; returns the port."""
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
            except (ConnectionError, asyncio.TimeoutError):
                for ev, listener in listeners:
                    conn.remove_listener(ev, listener)
                hdl.close()
                raise
            for ev, listener in listeners:
                conn.remove_listener(ev, listener)
            assert data == payload
            port = conn.backend["port"]
            hdl.release()
            return port

        await until(lambda: pool.get_stats()["idleConnections"] >= 2,
                    "the spares to connect")

        # 1. everything healthy: nothing touches the standby
        ports = {}
        for i in range(N_CLAIMS):
            p = await claim_echo(b"a%d" % i)
            ports[p] = ports.get(p, 0) + 1
        print("healthy: claims per port", ports,
              "standby accepted", standby.accepted)
        assert standby.port not in ports
        assert standby.accepted == 0
        assert sum(ports.values()) == N_CLAIMS
        assert pool.get_ranking()["activePriority"] == 0

        # 2. both primaries go away: claims carry on through the standby
        for s in primaries:
            s.kill()
        failures = 0
        served = 0
        while prio_events != [(0, 10)] or served < 50:
            try:
                p = await claim_echo(b"b%d" % served)
            except (ConnectionError, asyncio.TimeoutError):
                # a connection handed out while its primary was
                # closing; only counted before the failover completes
                assert prio_events == []
                failures += 1
                assert failures < 20
                continue
            if prio_events:
                assert p == standby.port
                served += 1
        rk = pool.get_ranking()
        print("failed over: events", prio_events, "ranking", rk)
        assert not pool.is_in_state("failed")
        assert rk["activePriority"] == 10
        assert rk["tiers"][0]["dead"] == 2
        assert rk["tiers"][1]["connections"] >= 1

        # 3. the primaries return on their old ports: fail back
        for s in primaries:
            await s.start()
        await until(lambda: prio_events == [(0, 10), (10, 0)],
                    "the pool to fail back")
        await until(
            lambda: pool.get_ranking()["tiers"][1]["connections"] == 0
            and pool.get_stats()["idleConnections"] >= 1,
            "the standby connections to drain")
        ports = {}
        for i in range(N_CLAIMS):
            p = await claim_echo(b"c%d" % i)
            ports[p] = ports.get(p, 0) + 1
        print("failed back: claims per port", ports)
        assert standby.port not in ports
        assert pool.get_ranking()["activePriority"] == 0

        pool.stop()
        for s in primaries + [standby]:
            s.kill()
        await asyncio.sleep(0.1)
        return prio_events

    assert asyncio.run(main()) == [(0, 10), (10, 0)]
