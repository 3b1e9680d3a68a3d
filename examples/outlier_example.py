"""Outlier ejection: a pool that stops using a backend which accepts
connections but fails the requests sent to it.

Runs self-contained on three loopback servers.  Two echo; the third
hangs up on the first byte for the first 1.2 seconds and behaves after
that.  The pool ejects it after three failed leases in a row, for
400 ms and then for 800 ms, serves every claim from the other two in the
meantime, and takes it back for good once it has recovered.
"""

import asyncio
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cueball_amd
from cueball_amd.connection import tcp_constructor

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 100}}


async def main():
    loop = asyncio.get_running_loop()
    t0 = loop.time()
    state = {"broken": True}

    def stamp():
        return "%5.2f s" % (loop.time() - t0)

    def make_handler(flaky):
        async def handler(reader, writer):
            try:
                while data := await reader.read(4096):
                    if flaky and state["broken"]:
                        break
                    writer.write(data)
                    await writer.drain()
            except ConnectionError:
                pass
            writer.close()
        return handler

    servers = [await asyncio.start_server(make_handler(i == 2),
                                          "127.0.0.1", 0) for i in range(3)]
    ports = [s.sockets[0].getsockname()[1] for s in servers]
    print("echo servers on ports %d and %d, flaky server on port %d"
          % tuple(ports))

    resolver = cueball_amd.StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": p} for p in ports]})
    pool = cueball_amd.ConnectionPool({
        "domain": "outlier.local",
        "resolver": resolver,
        "constructor": tcp_constructor(),
        "spares": 3,
        "maximum": 6,
        "recovery": RECOVERY,
        "outlierDetection": {"consecutiveFailures": 3,
                             "baseEjectionTime": 400,
                             "maxEjectionTime": 5000},
    })

    def port_of(key):
        return pool.p_backends[key]["port"]

    pool.on("backendEjected", lambda key, info: print(
        "%s  backendEjected: port %d, %r" % (stamp(), port_of(key), info)))
    pool.on("backendReinstated", lambda key, reason: print(
        "%s  backendReinstated: port %d, reason %s"
        % (stamp(), port_of(key), reason)))
    resolver.start()
    while pool.get_stats()["idleConnections"] < 3:
        await asyncio.sleep(0.01)

    async def one_request(i):
        """Claim, send, wait for the echo; close the lease if the
        connection dies instead."""
        handle, conn = await pool.claim_async({"timeout": 2000})
        answer = loop.create_future()

        def done(value):
            if not answer.done():
                answer.set_result(value)

        listeners = [("data", conn.on("data", done)),
                     ("error", conn.on("error", lambda e: done(None))),
                     ("close", conn.on("close", lambda: done(None)))]
        conn.write(b"request %d" % i)
        data = await answer
        for event, listener in listeners:
            conn.remove_listener(event, listener)
        if data is None:
            handle.close()          # counts against the backend
            return False
        handle.release()            # counts for it
        return True

    ok = failed = i = 0
    while loop.time() - t0 < 2.5:
        if state["broken"] and loop.time() - t0 > 1.2:
            state["broken"] = False
            print("%s  the flaky server recovers" % stamp())
        if await one_request(i):
            ok += 1
        else:
            failed += 1
            print("%s  request %d failed" % (stamp(), i))
        i += 1
        await asyncio.sleep(0.005)

    print("%d requests answered, %d failed" % (ok, failed))
    stats = pool.get_outlier_stats()
    print("ejected now: %d" % stats["ejected"])
    for key, rec in stats["backends"].items():
        print("port %d: %r" % (port_of(key), rec))
    counters = pool.get_stats()["counters"]
    print({k: counters.get(k, 0) for k in (
        "backend-ejected", "backend-reinstated", "ejection-refused")})

    pool.stop()
    for s in servers:
        s.close()
    await asyncio.sleep(0.2)


if __name__ == "__main__":
    asyncio.run(main())
