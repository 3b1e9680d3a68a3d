"""Request retries: an agent that sends a failed request to another
backend, and a retry budget that keeps a burst of failures from turning
into a burst of retries.

Runs self-contained on two loopback HTTP servers.  One answers; the
other resets every request it is sent.  First, ten GETs one after the
other: each that meets the bad server is retried, on the good one, and
succeeds.  A POST is not retried unless the call says it may be.  Then
a brownout: both servers reset, and forty GETs go out at once.  With a
budget of 20 % only a few of them may retry; the rest end with their
own errors at once, the counter ``retry-budget-exhausted`` says how
many, and the service is spared forty more requests it could not have
answered.
"""

import asyncio
import os
import socket
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cueball_amd
from cueball_amd.http_client import HttpParseError

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 20}}
HOST = "retry.local"


async def main():
    loop = asyncio.get_running_loop()
    # a reset under a request is also raised into the loop by the claim
    # handle (the socket has no error listener of ours); keep it quiet
    loop.set_exception_handler(lambda loop, ctx: None)
    served = {"good": 0, "bad": 0}
    state = {"brownout": False}

    def make_handler(name):
        async def handler(reader, writer):
            try:
                while data := await reader.read(4096):
                    served[name] += data.count(b"\r\n\r\n")
                    if name == "bad" or state["brownout"]:
                        writer.get_extra_info("socket").setsockopt(
                            socket.SOL_SOCKET, socket.SO_LINGER,
                            struct.pack("ii", 1, 0))
                        break
                    writer.write(b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\n"
                                 b"Connection: keep-alive\r\n\r\nok")
                    await writer.drain()
            except ConnectionError:
                pass
            writer.close()
        return handler

    servers = [await asyncio.start_server(make_handler(name), "127.0.0.1", 0)
               for name in ("good", "bad")]
    ports = [s.sockets[0].getsockname()[1] for s in servers]
    print("good server on port %d, resetting server on port %d"
          % tuple(ports))

    resolver = cueball_amd.StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": p} for p in ports]})
    agent = cueball_amd.HttpAgent({
        "spares": 2,
        "maximum": 4,
        "recovery": RECOVERY,
        "retry": {
            "maxRetries": 2,
            "delay": 5,
            "perTryTimeout": 1000,
            "budget": {"percent": 20, "minConcurrency": 1},
        },
    })
    agent.create_pool(HOST, {"resolver": resolver})
    resolver.start()
    pool = agent.get_pool(HOST)
    while pool.get_stats()["idleConnections"] < 2:
        await asyncio.sleep(0.01)

    def get(path, method="GET", **kw):
        """One request; resolves to (request, response or error)."""
        fut = loop.create_future()
        req = agent.request(
            HOST, method, path, None, None,
            lambda err, resp: fut.set_result((req, err or resp)), **kw)
        req.on("retry", lambda n, reason, ms: print(
            "  %s %s: retry %d after a %s, in %.1f ms"
            % (method, path, n, reason, ms)))
        return fut

    print("ten GETs, one after the other:")
    for i in range(10):
        req, res = await get("/seq/%d" % i)
        print("  GET /seq/%d -> %s in %d %s" % (
            i, res.status_code, req.attempts,
            "try" if req.attempts == 1 else "tries"))
        await asyncio.sleep(0.05)      # let the pool reconnect

    print("a POST, until it meets the bad server:")
    for i in range(10):
        req, res = await get("/post/%d" % i, "POST")
        if isinstance(res, (OSError, HttpParseError)):
            print("  POST /post/%d -> %s: %s, %d try, not retried"
                  % (i, type(res).__name__, res, req.attempts))
            break
        await asyncio.sleep(0.05)
    print("and one that says it is safe to repeat:")
    for i in range(10):
        req, res = await get("/idem/%d" % i, "POST",
                             retry={"methods": ["POST"]})
        if req.attempts > 1:
            print("  POST /idem/%d -> %s in %d tries"
                  % (i, res.status_code, req.attempts))
            break
        await asyncio.sleep(0.05)

    before = agent.get_retry_stats()[HOST]["counters"]
    print("a brownout, forty GETs at once, budget 20 %:")
    state["brownout"] = True
    sent = sum(served.values())
    results = await asyncio.gather(*[get("/burst/%d" % i)
                                     for i in range(40)])
    state["brownout"] = False
    ok = sum(1 for _, res in results if not isinstance(res, Exception))
    retried = sum(1 for req, _ in results if req.attempts > 1)
    print("  %d answered, %d failed; %d were retried, the servers saw "
          "%d requests" % (ok, len(results) - ok, retried,
                           sum(served.values()) - sent))
    stats = agent.get_retry_stats()[HOST]
    print("  retries denied by the budget: %d"
          % (stats["counters"]["retry-budget-exhausted"]
             - before["retry-budget-exhausted"]))
    print("retry stats:", stats)
    print("requests seen by the servers:", served)
    print([line for line in agent.collector.collect().splitlines()
           if line.startswith("cueball_agent_")])

    done = loop.create_future()
    agent.stop(lambda err: done.set_result(None))
    await done
    for s in servers:
        s.close()
    await asyncio.sleep(0.2)


if __name__ == "__main__":
    asyncio.run(main())
