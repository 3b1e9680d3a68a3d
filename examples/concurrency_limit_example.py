"""The concurrency limit: how many leases to carry at once, measured
instead of guessed.

Runs self-contained on one loopback echo server that behaves like a
service with a knee: up to four requests at once take 20 ms each, `n`
of them take ``20 * n / 4`` ms.  Sixteen callers, each sending its next
request as soon as the last one is answered, for four seconds, behind a
pool with ``maximum`` 16.  Three pools:

- without ``concurrencyLimit``: all sixteen connections are kept busy,
  every request takes 80 ms, and the server answers no more requests per
  second than it would at four;
- ``{"algorithm": "aimd", "latencyThreshold": 30}``: the limit backs off
  while a window's mean lease time is over 30 ms and creeps up while it
  is not; the requests beyond it wait in the pool's queue, the ones in
  flight take about 30 ms;
- ``True``, the gradient controller with its defaults but a shorter
  window: it measures the unloaded latency itself in a short probe, aims
  at one and a half times that, and needs no threshold.

The throughput is the same in all three: the server was saturated
anyway.  What changes is where the requests wait, and how long the ones
that the server has seen take.
"""

import asyncio
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cueball_amd
from cueball_amd.connection import tcp_constructor

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 100}}
BASE, CAPACITY, CALLERS, RUN_FOR = 0.02, 4, 16, 4.0


async def run(limit):
    loop = asyncio.get_running_loop()
    active = [0]

    async def handler(reader, writer):
        try:
            while data := await reader.readline():
                active[0] += 1
                try:
                    await asyncio.sleep(BASE * max(1, active[0] / CAPACITY))
                finally:
                    active[0] -= 1
                writer.write(data)
                await writer.drain()
        except ConnectionError:
            pass
        writer.close()

    server = await asyncio.start_server(handler, "127.0.0.1", 0)
    port = server.sockets[0].getsockname()[1]
    resolver = cueball_amd.StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": port}]})
    options = {
        "domain": "limit.local",
        "resolver": resolver,
        "constructor": tcp_constructor(),
        "spares": CALLERS,
        "maximum": CALLERS,
        "recovery": RECOVERY,
    }
    if limit is not None:
        options["concurrencyLimit"] = limit
    pool = cueball_amd.ConnectionPool(options)
    changes = []
    pool.on("limitChanged", lambda new, old: changes.append((new, old)))
    resolver.start()
    while pool.get_stats()["idleConnections"] < CALLERS:
        await asyncio.sleep(0.01)

    leases = []
    stop = [False]
    pending = [0]

    def call():
        pending[0] += 1
        asked = loop.time()

        def cb(err, hdl=None, conn=None):
            if err is not None:
                pending[0] -= 1
                return
            got = loop.time()

            def on_data(chunk):
                conn.remove_listener("data", on_data)
                leases.append((got - asked, loop.time() - got))
                hdl.release()
                pending[0] -= 1
                if not stop[0]:
                    call()

            conn.on("data", on_data)
            conn.write(b"ping\n")

        pool.claim({"timeout": 5000}, cb)

    for _ in range(CALLERS):
        call()
    await asyncio.sleep(RUN_FOR)
    stop[0] = True
    while pending[0] > 0:
        await asyncio.sleep(0.01)
    await asyncio.sleep(0.05)
    late = leases[len(leases) // 2:]
    stats = pool.get_limit_stats()

    stopped = loop.create_future()
    pool.on("stateChanged",
            lambda st: st == "stopped" and stopped.set_result(None))
    pool.stop()
    await stopped
    server.close()
    return {
        "requests": len(leases),
        "waitMs": 1000 * sum(w for w, _ in late) / len(late),
        "leaseMs": 1000 * sum(h for _, h in late) / len(late),
        "stats": stats,
        "changes": changes,
    }


async def main():
    cases = (
        ("no limit", None),
        ("aimd, threshold 30 ms",
         {"algorithm": "aimd", "latencyThreshold": 30, "window": 200,
          "minSamples": 5}),
        ("gradient", {"window": 200, "minSamples": 5}),
    )
    for name, limit in cases:
        res = await run(limit)
        print("%-22s %4d requests; second half: %5.1f ms in the pool's "
              "queue, %5.1f ms at the server"
              % (name, res["requests"], res["waitMs"], res["leaseMs"]))
        st = res["stats"]
        if st["enabled"]:
            print("%-22s limit %.1f after %d windows (%d up, %d down), "
                  "baseline %s ms, limitChanged %d times"
                  % ("", st["limit"], st["windows"], st["raised"],
                     st["lowered"],
                     "-" if st["baselineMs"] is None
                     else "%.1f" % st["baselineMs"], len(res["changes"])))


if __name__ == "__main__":
    asyncio.run(main())
