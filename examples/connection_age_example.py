"""Bounded connection age: a pool that replaces its sockets every second.

Runs self-contained on a loopback echo server.  The pool keeps four
connections with ``maxConnectionAge`` 1000 ms and the default 20 %
spread, serves a claim every 50 ms for three seconds and prints
``get_connection_ages()`` and the recycle counters on the way, then
replaces everything once more by hand with ``recycle()``.
"""

import asyncio
import os
import pprint
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cueball_amd
from cueball_amd.connection import tcp_constructor

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 100}}


def show(pool, title):
    ages = pool.get_connection_ages()
    print("%s: oldest %s ms of at most %s" % (
        title, ages["oldestMs"] and round(ages["oldestMs"]), ages["maxAgeMs"]))
    pprint.pprint([
        {k: (round(v) if isinstance(v, float) else v) for k, v in c.items()}
        for c in ages["connections"]])
    counters = pool.get_stats()["counters"]
    print("recycled-age %d, recycled-manual %d" % (
        counters.get("recycled-age", 0), counters.get("recycled-manual", 0)))


async def main():
    accepted = []

    async def echo(reader, writer):
        accepted.append(writer.get_extra_info("peername")[1])
        try:
            while data := await reader.read(4096):
                writer.write(data)
                await writer.drain()
        except ConnectionError:
            pass
        writer.close()

    server = await asyncio.start_server(echo, "127.0.0.1", 0)
    port = server.sockets[0].getsockname()[1]

    resolver = cueball_amd.StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": port}]})
    pool = cueball_amd.ConnectionPool({
        "domain": "aging.local",
        "resolver": resolver,
        "constructor": tcp_constructor(),
        "spares": 4,
        "maximum": 8,
        "recovery": RECOVERY,
        "maxConnectionAge": 1000,
    })
    pool.on("connectionRecycled", lambda key, reason: print(
        "connectionRecycled: backend %s, reason %s" % (key, reason)))
    resolver.start()

    while pool.get_stats()["idleConnections"] < 4:
        await asyncio.sleep(0.01)
    show(pool, "just connected")

    for i in range(60):
        handle, conn = await pool.claim_async()
        conn.write(b"ping %d" % i)
        handle.release()
        await asyncio.sleep(0.05)
        if i % 20 == 19:
            show(pool, "after %d claims" % (i + 1))
    print("the server has accepted %d connections for a pool of 4"
          % len(accepted))

    print("recycle() marked %d connections" % pool.recycle())
    while pool.get_stats()["counters"].get("recycled-manual", 0) < 4:
        await asyncio.sleep(0.01)
    show(pool, "after recycle()")

    pool.stop()
    server.close()
    await asyncio.sleep(0.2)


if __name__ == "__main__":
    asyncio.run(main())
