"""Request hedging: an agent that sends a slow request a second time,
to another backend, and takes the first answer.

Runs self-contained on two loopback HTTP servers.  Both answer, but one
of them takes 200 ms over every request once it has been told to
stall.  First, sixty GETs against two healthy
servers fill the latency window of the adaptive policy: no hedge is
sent while there is no estimate, and none is needed afterwards.  Then
one server starts to stall.  Without hedging every request that meets
it would take 200 ms; with it, such a request is sent again after about
the p95 of recent response times and answered by the other server.  A
POST is not hedged unless the call says it may be.
"""

import asyncio
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cueball_amd

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 20}}
HOST = "hedge.local"
STALL = 0.2


async def main():
    loop = asyncio.get_running_loop()
    served = {"steady": 0, "moody": 0}
    state = {"stalling": False}

    def make_handler(name):
        async def handler(reader, writer):
            try:
                while data := await reader.read(4096):
                    served[name] += data.count(b"\r\n\r\n")
                    if name == "moody" and state["stalling"]:
                        await asyncio.sleep(STALL)
                    writer.write(b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\n"
                                 b"Connection: keep-alive\r\n\r\nok")
                    await writer.drain()
            except ConnectionError:
                pass
            writer.close()
        return handler

    servers = [await asyncio.start_server(make_handler(name), "127.0.0.1", 0)
               for name in ("steady", "moody")]
    ports = [s.sockets[0].getsockname()[1] for s in servers]
    print("steady server on port %d, moody server on port %d" % tuple(ports))

    resolver = cueball_amd.StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": p} for p in ports]})
    agent = cueball_amd.HttpAgent({
        "spares": 2,
        "maximum": 4,
        "recovery": RECOVERY,
        "hedge": {
            # adaptive: the p95 of the last 2 to 4 s, between 5 and 100 ms
            "percentile": 95,
            "window": 2000,
            "minSamples": 20,
            "minDelay": 5,
            "maxDelay": 100,
        },
    })
    agent.create_pool(HOST, {"resolver": resolver})
    resolver.start()
    pool = agent.get_pool(HOST)
    while pool.get_stats()["idleConnections"] < 2:
        await asyncio.sleep(0.01)

    def get(path, method="GET", **kw):
        """One request; resolves to (request, response or error, ms)."""
        fut = loop.create_future()
        t0 = loop.time()
        req = agent.request(
            HOST, method, path, None, None,
            lambda err, resp: fut.set_result(
                (req, err or resp, (loop.time() - t0) * 1000.0)), **kw)
        return fut

    print("sixty GETs against two healthy servers:")
    slowest = 0.0
    for i in range(60):
        req, res, ms = await get("/warm/%d" % i)
        slowest = max(slowest, ms)
        await asyncio.sleep(0.005)
    stats = agent.get_hedge_stats()[HOST]
    print("  slowest %.1f ms; hedges sent: %d, not sent for want of samples: "
          "%d; the delay is now %.1f ms"
          % (slowest, stats["counters"]["hedge-sent"],
             stats["counters"]["hedge-skipped-samples"], stats["delayMs"]))

    print("the moody server starts to take %d ms; twenty GETs:"
          % (STALL * 1000))
    state["stalling"] = True
    for i in range(20):
        req, res, ms = await get("/slow/%d" % i)
        print("  GET /slow/%d -> %s in %5.1f ms%s" % (
            i, res.status_code, ms,
            ", answered by the %s" % req.winner if req.hedged else ""))
        await asyncio.sleep(0.05)       # let the pool reconnect

    print("a POST waits for the server it was sent to:")
    for i in range(10):
        req, res, ms = await get("/post/%d" % i, "POST")
        if ms > STALL * 500:
            print("  POST /post/%d -> %s in %.1f ms, not hedged"
                  % (i, res.status_code, ms))
            break
    print("unless the call says it is safe to send twice:")
    for i in range(10):
        req, res, ms = await get("/idem/%d" % i, "POST",
                                 hedge={"methods": ["POST"]})
        if req.hedged:
            print("  POST /idem/%d -> %s in %.1f ms, answered by the %s"
                  % (i, res.status_code, ms, req.winner))
            break
        await asyncio.sleep(0.05)

    print("hedge stats:", agent.get_hedge_stats()[HOST])
    print("requests seen by the servers:", served)
    print([line for line in agent.collector.collect().splitlines()
           if line.startswith("cueball_agent_hedge")])

    done = loop.create_future()
    agent.stop(lambda err: done.set_result(None))
    await done
    for s in servers:
        s.close()
    await asyncio.sleep(0.3)


if __name__ == "__main__":
    asyncio.run(main())
