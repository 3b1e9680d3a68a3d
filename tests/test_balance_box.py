"""Claim balancing over real sockets on the deployment box (run with
-m gpu).

Two loopback echo servers behind one pool, spares 4: one answers at
once, the other after 30 ms.  200 claims, 10 ms apart; each claimer
writes a line, awaits the echo and releases.  Once without the option,
once with ``{"choices": "all"}``, about 4 s in all.  The arithmetic is
pinned on the virtual clock in test_balance_pool.py; this is about the
plumbing: the native handle and slot cycle under a Python ticket, lease
timing on the real clock, real TCP.
"""

import asyncio

import pytest

from balance_kit import DelayServer
from retry_kit import run, until

pytestmark = pytest.mark.gpu

CLAIMS = 200
PACE = 0.01
DELAY = 0.03
RECOVERY = {"default": {"timeout": 2000, "retries": 2, "delay": 50,
                        "maxDelay": 200}}


def test_native_runtime_in_use():
    """Balancing must ride on the native handle and slot cycle, not
    replace them."""
    from cueball_amd import _speed
    from cueball_amd import connection_fsm, fsm, pool, queue
    assert fsm.FSM is _speed.FSM
    assert pool._native_pool_claim is _speed.pool_claim
    assert pool._NativeClaimTicket is _speed.ClaimTicket
    assert pool._NativeSlotDispatch is _speed.SlotDispatch
    assert issubclass(connection_fsm.ClaimHandle, _speed.ClaimHandleBase)
    assert connection_fsm._SlotKit is _speed.SlotKit
    assert queue.Queue is _speed.Queue


async def one_run(lb):
    from cueball_amd.connection import tcp_constructor
    from cueball_amd.pool import ConnectionPool
    from cueball_amd.resolver import StaticIpResolver

    loop = asyncio.get_running_loop()
    fast = await DelayServer(http=False).start()
    slow = await DelayServer(delay=DELAY, http=False).start()
    resolver = StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": s.port} for s in (fast, slow)]})
    opts = {"domain": "balance.box", "constructor": tcp_constructor(loop=loop),
            "resolver": resolver, "recovery": RECOVERY, "spares": 4,
            "maximum": 4, "loop": loop}
    if lb is not None:
        opts["claimBalancing"] = lb
    pool = ConnectionPool(opts)
    resolver.start()
    await until(lambda: pool.get_stats()["idleConnections"] == 4,
                "the spares to connect")
    assert sorted(len(v) for v in pool.p_connections.values()) == [2, 2]

    done = []
    errors = []

    def claimer(n):
        line = b"line %d\n" % n

        def cb(err, hdl=None, conn=None):
            if err is not None:
                errors.append(err)
                return
            got = []

            def on_data(chunk):
                got.append(chunk)
                if b"".join(got).endswith(b"\n"):
                    conn.remove_listener("data", on_data)
                    if b"".join(got) != line:
                        errors.append((n, b"".join(got)))
                    hdl.release()
                    done.append(n)

            conn.on("data", on_data)
            conn.write(line)

        pool.claim({"timeout": 5000}, cb)

    start = loop.time()
    for n in range(CLAIMS):
        claimer(n)
        await asyncio.sleep(PACE)
    await until(lambda: len(done) + len(errors) == CLAIMS,
                "the last echo")
    took = loop.time() - start
    # the pool hears of the last release a loop turn later
    await asyncio.sleep(0.05)
    assert errors == []
    assert sorted(done) == list(range(CLAIMS))
    assert fast.served + slow.served == CLAIMS
    stats = pool.get_balancing_stats()
    counters = dict(pool.get_stats()["counters"])

    stopped = loop.create_future()
    pool.on("stateChanged",
            lambda st: st == "stopped" and stopped.set_result(None))
    pool.stop()
    await asyncio.wait_for(stopped, 10.0)
    for s in (fast, slow):
        s.stop()
    return slow.served, took, stats, counters


def test_balancing_steers_around_a_delayed_server_over_real_sockets():
    async def body():
        off, off_took, off_stats, _ = await one_run(None)
        on, on_took, on_stats, counters = await one_run({"choices": "all"})
        print("claims", CLAIMS, "delayed server served: off", off, "on", on,
              "seconds off %.2f on %.2f" % (off_took, on_took),
              "counters", counters)
        assert off_stats == {"enabled": False}
        assert on_stats["enabled"] is True
        assert sum(v["leases"] for v in on_stats["backends"].values()) \
            == CLAIMS
        assert sum(v["outstanding"]
                   for v in on_stats["backends"].values()) == 0
        # without a yardstick that shows the problem the comparison
        # below says nothing: fail as inconclusive
        assert off >= 0.20 * CLAIMS, \
            "inconclusive: the plain pool sent the delayed server %d" % off
        assert on <= off / 2.0, (on, off)
        assert counters["balanced-claim"] + \
            counters.get("queued-claim", 0) >= CLAIMS
    run(body())
