"""The concurrency limit over real sockets on the deployment box (run
with -m gpu).

One loopback echo server that behaves like a saturating service: it
answers after ``base * max(1, active / 4)``, base 20 ms.  Sixteen
closed-loop claimers over real TCP for 3 s, once without the option and
once with ``aimd``, about 8 s in all.  The arithmetic is pinned on the
virtual clock in test_limit_estimator.py and test_limit_pool.py; this is
about the plumbing: the native handle and slot cycle under a Python
listener, lease timing on the real clock, real TCP.
"""

import asyncio

import pytest

from limit_kit import CAPACITY, ModelServer
from retry_kit import run, until

pytestmark = pytest.mark.gpu

CLAIMERS = 16
SECONDS = 3.0
BASE = 0.02
RECOVERY = {"default": {"timeout": 2000, "retries": 2, "delay": 50,
                        "maxDelay": 200}}
AIMD = {"algorithm": "aimd", "latencyThreshold": 30, "window": 200,
        "minSamples": 5}


def test_native_runtime_in_use():
    """The limit must ride on the native handle and slot cycle, not
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


async def one_run(cl):
    from cueball_amd.connection import tcp_constructor
    from cueball_amd.pool import ConnectionPool
    from cueball_amd.resolver import StaticIpResolver

    loop = asyncio.get_running_loop()
    server = await ModelServer(BASE).start()
    resolver = StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": server.port}]})
    opts = {"domain": "limit.box", "constructor": tcp_constructor(loop=loop),
            "resolver": resolver, "recovery": RECOVERY, "spares": CLAIMERS,
            "maximum": CLAIMERS, "loop": loop}
    if cl is not None:
        opts["concurrencyLimit"] = cl
    pool = ConnectionPool(opts)
    resolver.start()
    await until(lambda: pool.get_stats()["idleConnections"] == CLAIMERS,
                "the connections")

    state = {"stop": False, "open": 0}
    leases = []             # (end, seconds from the callback to the echo)
    errors = []
    serial = [0]

    def claimer():
        serial[0] += 1
        line = b"line %d\n" % serial[0]

        def cb(err, hdl=None, conn=None):
            if err is not None:
                errors.append(err)
                return
            t0 = loop.time()
            state["open"] += 1
            got = []

            def on_data(chunk):
                got.append(chunk)
                if b"".join(got).endswith(b"\n"):
                    conn.remove_listener("data", on_data)
                    if b"".join(got) != line:
                        errors.append((line, b"".join(got)))
                    leases.append((loop.time(), loop.time() - t0))
                    state["open"] -= 1
                    hdl.release()
                    if not state["stop"]:
                        claimer()

            conn.on("data", on_data)
            conn.write(line)

        pool.claim({"timeout": 5000}, cb)

    start = loop.time()
    for _ in range(CLAIMERS):
        claimer()
    await asyncio.sleep(SECONDS)
    state["stop"] = True
    served = server.served
    await until(lambda: state["open"] == 0 and
                pool.get_stats()["waiterCount"] == 0, "the last echoes")
    # the pool hears of the last release a loop turn later
    await asyncio.sleep(0.05)
    assert errors == []
    half = start + SECONDS / 2
    out = {
        "served": served,
        "meanMs": 1000.0 * sum(s for _, s in leases) / len(leases),
        "lateMeanMs": 1000.0 * (lambda xs: sum(xs) / len(xs))(
            [s for t, s in leases if t > half]),
        "latePeak": max(a for t, a in server.peaks if t > half),
        "stats": pool.get_limit_stats(),
        "counters": dict(pool.get_stats()["counters"]),
    }

    stopped = loop.create_future()
    pool.on("stateChanged",
            lambda st: st == "stopped" and stopped.set_result(None))
    pool.stop()
    await asyncio.wait_for(stopped, 10.0)
    server.stop()
    return out


def test_the_limit_finds_the_knee_of_a_saturating_server_over_real_tcp():
    async def body():
        off = await one_run(None)
        on = await one_run(AIMD)
        print("claimers", CLAIMERS, "seconds", SECONDS, "base ms",
              BASE * 1000.0, "capacity", CAPACITY)
        for name, res in (("off", off), ("on", on)):
            print(name, "served", res["served"],
                  "mean ms %.1f" % res["meanMs"],
                  "late mean ms %.1f" % res["lateMeanMs"],
                  "late peak", res["latePeak"], res["stats"],
                  res["counters"])
        assert off["stats"] == {"enabled": False}
        assert on["stats"]["enabled"] is True
        assert on["stats"]["inFlight"] == 0
        assert on["stats"]["windows"] >= 5
        # without a yardstick that shows the problem the comparison
        # below says nothing: fail as inconclusive
        assert off["meanMs"] >= 3 * BASE * 1000.0, \
            "inconclusive: the plain pool's leases took %.1f ms" \
            % off["meanMs"]
        # at 8 the model's latency is 2 x base, over the threshold: the
        # limit cannot stay there
        assert on["latePeak"] <= 8
        assert on["meanMs"] <= off["meanMs"] / 1.5
        # a limit that collapsed to 2 or less would show here
        assert on["served"] >= 0.6 * off["served"]
    run(body())
