"""SRV ranking: two primaries (priority 0) and a standby (priority 10).

Runs self-contained on local echo servers behind a StaticIpResolver,
whose backends may carry the priority and weight a DNS resolver with
``srvRanking`` would take from SRV records.  Prints ``get_ranking()``
while the primaries are healthy, kills them, and prints it again once
the pool has failed over to the standby.
"""

import asyncio
import os
import pprint
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cueball_amd
from cueball_amd.connection import tcp_constructor

RECOVERY = {"default": {"timeout": 500, "retries": 2, "delay": 50,
                        "maxDelay": 200}}


async def main():
    writers = {}

    def echo_for(name):
        async def echo(reader, writer):
            writers.setdefault(name, []).append(writer)
            try:
                while data := await reader.read(4096):
                    writer.write(data)
                    await writer.drain()
            except ConnectionError:
                pass
            writer.close()
        return echo

    names = ["primary-a", "primary-b", "standby"]
    servers = {n: await asyncio.start_server(echo_for(n), "127.0.0.1", 0)
               for n in names}
    port = {n: s.sockets[0].getsockname()[1] for n, s in servers.items()}

    resolver = cueball_amd.StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": port["primary-a"],
         "priority": 0, "weight": 3},
        {"address": "127.0.0.1", "port": port["primary-b"],
         "priority": 0, "weight": 1},
        {"address": "127.0.0.1", "port": port["standby"],
         "priority": 10, "weight": 1},
    ]})
    pool = cueball_amd.ConnectionPool({
        "domain": "ranked.local",
        "resolver": resolver,
        "constructor": tcp_constructor(),
        "spares": 4,
        "maximum": 8,
        "recovery": RECOVERY,
        "srvRanking": True,
    })
    failed_over = asyncio.get_running_loop().create_future()
    pool.on("priorityChanged", lambda old, new: (
        print("priorityChanged: %d -> %d" % (old, new)),
        failed_over.done() or failed_over.set_result(None)))
    resolver.start()

    while pool.get_stats()["idleConnections"] < 4:
        await asyncio.sleep(0.01)
    print("healthy (3:1 over the primaries, nothing on the standby):")
    pprint.pprint(pool.get_ranking())

    for n in ("primary-a", "primary-b"):
        servers[n].close()
        for w in writers.get(n, ()):
            w.close()
    await asyncio.wait_for(failed_over, timeout=10)
    # wait for the standby connections, and for the primaries' slots
    # that were caught mid-reconnect to wind down to the two monitors
    while pool.get_stats()["idleConnections"] < 4 or \
            pool.get_ranking()["tiers"][0]["connections"] > 2:
        await asyncio.sleep(0.01)
    print("primaries down (one monitor each, the load on the standby):")
    pprint.pprint(pool.get_ranking())

    handle, conn = await pool.claim_async()
    print("claim served by port %d (standby is %d)"
          % (conn.backend["port"], port["standby"]))
    handle.release()

    pool.stop()
    servers["standby"].close()
    await asyncio.sleep(0.2)


if __name__ == "__main__":
    asyncio.run(main())
