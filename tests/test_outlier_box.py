"""Outlier ejection over real sockets on the deployment box (run with
-m gpu).

Two loopback servers behind one pool: one echoes, the other accepts and
then hangs up on the first byte it is sent for as long as a flag is
set.  Sequential claims for about 1.5 s: the bad one is ejected after
exactly three failed claims, every claim handed out while it is away is
served by the good one, it comes back after 400 ms, fails again and is
away for 800 ms, and once the flag is cleared both serve again.
"""

import asyncio

import pytest

pytestmark = pytest.mark.gpu

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 50,
                        "maxDelay": 200}}
DEADLINE = 15.0


def test_native_runtime_in_use():
    """Outlier detection must ride on the native claim path, not
    replace it."""
    from cueball_amd import _speed
    from cueball_amd import connection_fsm, fsm, pool
    assert fsm.FSM is _speed.FSM
    assert pool._native_pool_claim is _speed.pool_claim
    assert pool._NativeClaimTicket is _speed.ClaimTicket
    assert pool._NativeSlotDispatch is _speed.SlotDispatch
    assert issubclass(connection_fsm.ClaimHandle, _speed.ClaimHandleBase)
    assert connection_fsm._SlotKit is _speed.SlotKit


class Server:
    """Echo server; while ``hang_up`` is set it closes a connection on
    the first byte it receives instead."""

    def __init__(self):
        self.server = None
        self.port = None
        self.writers = set()
        self.hang_up = False
        self.hung_up = 0
        self.served_by = {}      # payload -> peer port

    async def _serve(self, reader, writer):
        peer = writer.get_extra_info("peername")[1]
        self.writers.add(writer)
        try:
            while True:
                data = await reader.read(1024)
                if not data:
                    break
                if self.hang_up:
                    self.hung_up += 1
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
            self._serve, "127.0.0.1", 0)
        self.port = self.server.sockets[0].getsockname()[1]

    def kill(self):
        self.server.close()
        for w in list(self.writers):
            w.close()


def test_ejection_and_recovery_over_real_sockets():
    from cueball_amd.connection import tcp_constructor
    from cueball_amd.pool import ConnectionPool
    from cueball_amd.resolver import StaticIpResolver

    async def main():
        loop = asyncio.get_running_loop()
        good, bad = Server(), Server()
        await good.start()
        await bad.start()
        bad.hang_up = True
        resolver = StaticIpResolver({
            "backends": [{"address": "127.0.0.1", "port": good.port},
                         {"address": "127.0.0.1", "port": bad.port}],
            "loop": loop,
        })
        pool = ConnectionPool({
            "domain": "outlier.box",
            "constructor": tcp_constructor(loop=loop),
            "resolver": resolver,
            "recovery": RECOVERY,
            "spares": 2,
            "maximum": 4,
            "outlierDetection": {"consecutiveFailures": 3,
                                 "baseEjectionTime": 400},
            "loop": loop,
        })
        failed = []              # payloads of the claims that failed
        events = []
        pool.on("backendEjected", lambda key, info: events.append(
            ("ejected", key, dict(info), len(failed), loop.time())))
        pool.on("backendReinstated", lambda key, why: events.append(
            ("reinstated", key, why, len(failed), loop.time())))
        resolver.start()

        async def until(cond, what, seconds=DEADLINE):
            for _ in range(int(seconds / 0.005)):
                if cond():
                    return
                await asyncio.sleep(0.005)
            raise AssertionError("timed out waiting for " + what)

        def failures():
            return sum(b["failures"] for b in
                       pool.get_outlier_stats()["backends"].values())

        async def claim_once(payload):
            """One claim and one round trip.  Returns (ok, out): `out`
            says whether a backend was ejected when the claim was
            handed out."""
            hdl, conn = await asyncio.wait_for(
                pool.claim_async({"timeout": 5000}), timeout=10)
            out = pool.get_outlier_stats()["ejected"] > 0
            got = loop.create_future()

            def lost(*args):
                if not got.done():
                    got.set_result(None)

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
            if data is None:
                failed.append(payload)
                hdl.close()
                # sequential: the pool has judged this lease before
                # the next claim goes out
                await until(lambda: failures() == len(failed),
                            "the failure to be counted")
                return False, out
            assert data == payload
            hdl.release()
            return True, out

        await until(lambda: pool.get_stats()["idleConnections"] >= 2,
                    "the spares to connect")
        assert len(pool.get_outlier_stats()["backends"]) == 2

        # 1. claims until the bad server has been out twice
        n = 0
        while_out = []           # payloads of claims handed out meanwhile
        start = loop.time()

        def twice_back():
            return [e[0] for e in events].count("reinstated") >= 2

        while not twice_back():
            assert loop.time() - start < DEADLINE, events
            payload = b"m%d" % n
            n += 1
            ok, out = await claim_once(payload)
            if out:
                assert ok, "a claim failed during an ejection"
                while_out.append(payload)
            if bad.hang_up and \
                    [e[0] for e in events].count("ejected") == 2:
                bad.hang_up = False
        took = loop.time() - start
        print("claims", n, "failed", len(failed), "during ejections",
              len(while_out), "seconds %.2f" % took, "events",
              [(e[0], e[2], e[3]) for e in events])

        assert [e[0] for e in events] == ["ejected", "reinstated",
                                          "ejected", "reinstated"]
        bad_key = events[0][1]
        assert pool.p_backends[bad_key]["port"] == bad.port
        assert all(e[1] == bad_key for e in events)
        # exactly three failed claims each time, and not one otherwise
        assert events[0][2] == {"reason": "consecutive-failures",
                                "durationMs": 400, "ejections": 1}
        assert events[0][3] == 3
        assert events[1][2] == "expired" and events[1][3] == 3
        assert events[2][2] == {"reason": "consecutive-failures",
                                "durationMs": 800, "ejections": 2}
        assert events[2][3] == 6
        assert events[3][2] == "expired"
        assert len(failed) == 6 and bad.hung_up == 6
        assert events[1][4] - events[0][4] == pytest.approx(0.4, abs=0.1)
        assert events[3][4] - events[2][4] == pytest.approx(0.8, abs=0.1)
        # while it was out, the good server answered everything
        assert len(while_out) > 40
        assert all(p in good.served_by for p in while_out)
        assert not any(p in bad.served_by for p in while_out)
        counters = pool.get_stats()["counters"]
        assert counters["backend-ejected"] == 2
        assert counters["backend-reinstated"] == 2
        assert counters.get("ejection-refused", 0) == 0

        # 2. recovery: both serve claims again
        served_bad = len(bad.served_by)
        served_good = len(good.served_by)
        start = loop.time()
        while len(bad.served_by) < served_bad + 3 or \
                len(good.served_by) < served_good + 3:
            assert loop.time() - start < DEADLINE, "no recovery"
            ok, out = await claim_once(b"r%d" % n)
            n += 1
            assert ok and not out
        stats = pool.get_outlier_stats()
        print("after recovery:", stats)
        assert stats["ejected"] == 0
        assert stats["backends"][bad_key]["consecutiveFailures"] == 0
        assert len(failed) == 6

        pool.stop()
        await until(lambda: pool.is_in_state("stopped"), "the pool to stop")
        good.kill()
        bad.kill()
        await until(lambda: not good.writers and not bad.writers,
                    "the servers to close")

    asyncio.run(main())
