"""Latency histograms on the deployment box (run with -m gpu).

Host code like the rest of the framework (tests/test_gpu_box.py), but it
has to hold where the library is deployed: the native histogram is the
one in use, and over real sockets the pool's own wait times stay inside
externally measured ones.
"""

import asyncio
import time

import pytest

pytestmark = pytest.mark.gpu

N_CLAIMS = 2000
CONCURRENCY = 4


def test_native_histogram_in_use():
    """No silent pure-Python fallback for the per-claim recorder."""
    from cueball_amd import _speed
    import cueball_amd.latency as latency
    assert latency.LatencyHistogram is _speed.LatencyHistogram
    import asyncio as aio
    loop = aio.new_event_loop()
    try:
        kit = latency.PoolLatency(loop)
        assert type(kit) is _speed.PoolLatency
        assert type(kit.wait) is _speed.LatencyHistogram
        assert kit.direct == 1      # stock loop clock: read in C
    finally:
        loop.close()


def test_wait_times_lie_inside_external_ones():
    """2000 claims through claim({}, cb) (the pool_claim fast path), 4 in
    flight, 2 echo backends.  Each is timed externally with
    time.monotonic() from just before claim() until inside the callback.
    The pool's interval (handle construction -> just before the
    callback) lies inside that one, and rounding to whole microseconds
    adds at most 0.5 us per sample, so

        claimWait.sumMs <= external_sum_ms + 2000 * 0.0005
    """
    from cueball_amd.connection import tcp_constructor
    from cueball_amd.pool import ConnectionPool
    from cueball_amd.resolver import StaticIpResolver

    async def main():
        loop = asyncio.get_running_loop()

        async def echo(reader, writer):
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
                writer.close()

        servers = [await asyncio.start_server(echo, "127.0.0.1", 0)
                   for _ in range(2)]
        resolver = StaticIpResolver({
            "backends": [
                {"address": "127.0.0.1",
                 "port": s.sockets[0].getsockname()[1]} for s in servers],
            "loop": loop,
        })
        pool = ConnectionPool({
            "domain": "latency.box",
            "constructor": tcp_constructor(loop=loop),
            "resolver": resolver,
            "recovery": {"default": {"timeout": 2000, "retries": 3,
                                     "delay": 100, "maxDelay": 1000}},
            "spares": 2,
            "maximum": 4,
            "loop": loop,
        })
        resolver.start()
        # let both spares connect first, without claiming
        for _ in range(1500):
            if pool.get_stats()["idleConnections"] >= 2:
                break
            await asyncio.sleep(0.01)
        assert pool.get_stats()["idleConnections"] >= 2

        done = loop.create_future()
        state = {"issued": 0, "finished": 0, "ext_ms": 0.0}
        mono = time.monotonic

        def issue():
            state["issued"] += 1

            def cb(err, hdl=None, conn=None):
                state["ext_ms"] += (mono() - t0) * 1000.0
                assert err is None, err
                hdl.release()
                state["finished"] += 1
                if state["issued"] < N_CLAIMS:
                    issue()
                elif state["finished"] == N_CLAIMS and not done.done():
                    done.set_result(None)

            t0 = mono()
            pool.claim({}, cb)

        for _ in range(CONCURRENCY):
            issue()
        await asyncio.wait_for(done, timeout=60)
        stats = pool.get_latency_stats()

        pool.stop()
        for s in servers:
            s.close()
        await asyncio.sleep(0.1)
        return stats, state["ext_ms"]

    stats, ext_ms = asyncio.run(main())
    wait, hold = stats["claimWait"], stats["claimHold"]
    print("claimWait n=%d sum=%.3f ms; external sum=%.3f ms; p50=%s p99=%s"
          % (wait["count"], wait["sumMs"], ext_ms, wait["p50"],
             wait["p99"]))
    assert wait["count"] == hold["count"] == N_CLAIMS
    assert stats["connect"]["count"] >= 2
    assert wait["sumMs"] <= ext_ms + N_CLAIMS * 0.0005
