"""Claim balancing: a pool that steers claims away from a backend which
is merely slow.

Runs self-contained on two loopback echo servers, two connections each.
One answers at once; the other takes 40 ms for the first 1.5 seconds
and answers at once after that.  The same paced requests go through a
pool without ``claimBalancing`` and through one with it.  The plain pool
sends the slow server about two requests in five; the balanced one
tries it once, keeps away while its estimate says 40 ms, and comes back
once the estimate has aged (``decayTime`` 500 ms here, so after about
500 * ln(40 ms / fast) ms) and the server proves fast again.
"""

import asyncio
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cueball_amd
from cueball_amd.connection import tcp_constructor

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 100}}
SLOW, SLOW_FOR, RUN_FOR, PACE = 0.04, 1.5, 4.0, 0.01


async def run(balancing):
    loop = asyncio.get_running_loop()
    t0 = loop.time()
    served = [0, 0]

    def make_handler(i):
        async def handler(reader, writer):
            try:
                while data := await reader.read(4096):
                    served[i] += 1
                    if i == 1 and loop.time() - t0 < SLOW_FOR:
                        await asyncio.sleep(SLOW)
                    writer.write(data)
                    await writer.drain()
            except ConnectionError:
                pass
            writer.close()
        return handler

    servers = [await asyncio.start_server(make_handler(i), "127.0.0.1", 0)
               for i in range(2)]
    ports = [s.sockets[0].getsockname()[1] for s in servers]
    resolver = cueball_amd.StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": p} for p in ports]})
    options = {
        "domain": "balancing.local",
        "resolver": resolver,
        "constructor": tcp_constructor(),
        "spares": 4,
        "maximum": 4,
        "recovery": RECOVERY,
    }
    if balancing is not None:
        options["claimBalancing"] = balancing
    pool = cueball_amd.ConnectionPool(options)
    resolver.start()
    while pool.get_stats()["idleConnections"] < 4:
        await asyncio.sleep(0.01)
    t0 = loop.time()

    took = []

    async def one_request(i):
        start = loop.time()
        handle, conn = await pool.claim_async({"timeout": 2000})
        answer = loop.create_future()
        listener = conn.on("data", lambda d: answer.done() or
                           answer.set_result(d))
        conn.write(b"request %d" % i)
        await answer
        conn.remove_listener("data", listener)
        handle.release()
        took.append(loop.time() - start)

    tasks = []
    i = 0
    while loop.time() - t0 < RUN_FOR:
        tasks.append(loop.create_task(one_request(i)))
        i += 1
        await asyncio.sleep(PACE)
    await asyncio.gather(*tasks)
    await asyncio.sleep(0.05)

    print("claimBalancing %r" % (balancing,))
    print("  %d requests, mean %.1f ms; fast server %d, slow server %d"
          % (len(took), sum(took) / len(took) * 1000.0, served[0],
             served[1]))
    stats = pool.get_balancing_stats()
    for key, rec in stats.get("backends", {}).items():
        print("  port %d: %r" % (pool.p_backends[key]["port"], rec))
    counters = pool.get_stats()["counters"]
    print("  %r" % {k: counters.get(k, 0) for k in (
        "claim", "balanced-claim", "balanced-reordered", "queued-claim")})

    pool.stop()
    for s in servers:
        s.close()
    await asyncio.sleep(0.2)
    return served[1]


async def main():
    plain = await run(None)
    balanced = await run({"choices": "all", "decayTime": 500})
    print("the slow server was sent %d requests by the plain pool and %d "
          "by the balanced one" % (plain, balanced))


if __name__ == "__main__":
    asyncio.run(main())
