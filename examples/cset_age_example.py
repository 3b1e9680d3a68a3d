"""Bounded connection age on a ConnectionSet: make-before-break.

Runs self-contained on a loopback echo server.  A set with ``target: 1``
on one static backend replaces its only connection every second, and the
consumer is never without one: it logs ``added b.2`` *before*
``removed b.1``, sends on whatever is advertised, and releases a removed
connection once its echoes are back.  At the end everything is replaced
once more by hand with ``recycle()``.
"""

import asyncio
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cueball_amd
from cueball_amd.connection import tcp_constructor

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 100}}


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
    cset = cueball_amd.ConnectionSet({
        "resolver": resolver,
        "constructor": tcp_constructor(),
        "target": 1,
        "maximum": 1,
        "recovery": RECOVERY,
        "maxConnectionAge": 1000,
        "connectionAgeSpread": 0,
    })

    live = {}         # ckey -> [conn, handle, echoes still in flight]
    leaving = set()   # 'removed', waiting for its echoes

    def short(ckey):
        return "b." + ckey.rsplit(".", 1)[1]

    def let_go(ckey):
        conn, hdl, _ = live.pop(ckey)
        leaving.discard(ckey)
        conn.remove_listener("data", on_data[ckey])
        hdl.release()

    on_data = {}

    def on_added(ckey, conn, hdl):
        print("added %s    (advertised now: %d)" % (short(ckey),
                                                    len(live) + 1))
        live[ckey] = [conn, hdl, 0]

        def data(chunk):
            live[ckey][2] -= chunk.count(b"\n")
            if ckey in leaving and live[ckey][2] == 0:
                let_go(ckey)

        on_data[ckey] = conn.on("data", data)

    def on_removed(ckey, conn, hdl):
        print("removed %s  (still advertised: %d)" % (
            short(ckey), len(live) - len(leaving) - 1))
        leaving.add(ckey)
        if live[ckey][2] == 0:
            let_go(ckey)

    cset.on("added", on_added)
    cset.on("removed", on_removed)
    cset.on("connectionRecycled", lambda key, reason: print(
        "connectionRecycled: reason %s" % reason))
    resolver.start()

    while not live:
        await asyncio.sleep(0.01)

    fewest = None
    for i in range(150):
        usable = [ck for ck in live if ck not in leaving]
        fewest = len(usable) if fewest is None else min(fewest, len(usable))
        live[usable[-1]][2] += 1
        live[usable[-1]][0].write(b"ping %d\n" % i)
        await asyncio.sleep(0.02)
    print("150 payloads sent, never fewer than %d usable connection(s); "
          "the server has accepted %d" % (fewest, len(accepted)))

    ages = cset.get_connection_ages()
    print("oldest %d ms of at most %d" % (ages["oldestMs"],
                                          ages["maxAgeMs"]))
    print("recycle() marked %d connection(s)" % cset.recycle())
    while cset.get_stats()["counters"].get("recycled-manual", 0) < 1:
        await asyncio.sleep(0.01)
    print("counters:", {k: v for k, v in
                        cset.get_stats()["counters"].items()
                        if k.startswith("recycle")})

    cset.stop()
    while not cset.is_in_state("stopped"):
        await asyncio.sleep(0.01)
    server.close()


if __name__ == "__main__":
    asyncio.run(main())
