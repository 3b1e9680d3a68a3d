"""The claim queue: a bound, priority classes and newest-first service
for the claims that have to wait.

Runs self-contained on one loopback echo server that takes 20 ms per
request, behind a pool of two connections: an overloaded backend.  For
one second background requests arrive every 4 ms, two and a half times
what the backend can do, and an interactive request every 50 ms; a
request is worth nothing to its caller after 300 ms.  Three pools:

- without ``claimQueue``: everybody stands in one line that only grows,
  and before long every request is served too late to matter, the
  interactive ones included;
- ``{"maxQueued": 8, "priorities": 2}``, interactive requests in class
  0: the line is bounded, so what is served is served in time, the
  excess is told so at once (ClaimQueueFullError), and the interactive
  requests go first;
- the same with ``"order": "adaptive"``: once the line has stood for
  ``lifoAfter`` ms the newest claim of a class is served first, so the
  backend's time goes to callers that are still waiting.
"""

import asyncio
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cueball_amd
from cueball_amd.connection import tcp_constructor

RECOVERY = {"default": {"timeout": 2000, "retries": 3, "delay": 100}}
SERVICE, RUN_FOR, USEFUL = 0.02, 1.0, 0.3
BACKGROUND_EVERY, INTERACTIVE_EVERY = 0.004, 0.05


async def run(claim_queue):
    loop = asyncio.get_running_loop()

    async def handler(reader, writer):
        try:
            while data := await reader.read(4096):
                await asyncio.sleep(SERVICE)
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
        "domain": "queue.local",
        "resolver": resolver,
        "constructor": tcp_constructor(),
        "spares": 2,
        "maximum": 2,
        "recovery": RECOVERY,
    }
    if claim_queue is not None:
        options["claimQueue"] = claim_queue
    pool = cueball_amd.ConnectionPool(options)
    resolver.start()
    while pool.get_stats()["idleConnections"] < 2:
        await asyncio.sleep(0.01)

    # kind -> [in time, too late, turned away]
    tally = {"interactive": [0, 0, 0], "background": [0, 0, 0]}

    async def one_request(kind):
        start = loop.time()
        claim_options = {}
        if claim_queue is not None and kind == "background":
            claim_options["priority"] = 1
        try:
            handle, conn = await pool.claim_async(claim_options)
        except cueball_amd.ClaimQueueFullError:
            tally[kind][2] += 1
            return
        answer = loop.create_future()
        listener = conn.on("data", lambda d: answer.done() or
                           answer.set_result(d))
        conn.write(b"request")
        await answer
        conn.remove_listener("data", listener)
        handle.release()
        late = loop.time() - start > USEFUL
        tally[kind][1 if late else 0] += 1

    tasks = []
    t0 = loop.time()
    next_interactive = 0.0
    while loop.time() - t0 < RUN_FOR:
        tasks.append(loop.create_task(one_request("background")))
        if loop.time() - t0 >= next_interactive:
            next_interactive += INTERACTIVE_EVERY
            tasks.append(loop.create_task(one_request("interactive")))
        await asyncio.sleep(BACKGROUND_EVERY)
    await asyncio.gather(*tasks)
    await asyncio.sleep(0.05)

    print("claimQueue %r" % (claim_queue,))
    for kind, (good, late, refused) in tally.items():
        print("  %-11s %3d in time, %3d too late, %3d turned away"
              % (kind, good, late, refused))
    counters = pool.get_stats()["counters"]
    print("  %r" % {k: counters.get(k, 0) for k in (
        "claim", "queued-claim", "max-claim-queue", "queue-rejected",
        "queue-shed", "queue-lifo")})
    print("  drained in %.2f s; %r" % (loop.time() - t0,
                                        pool.get_queue_stats()))

    pool.stop()
    server.close()
    await asyncio.sleep(0.2)
    return tally


async def main():
    plain = await run(None)
    bounded = await run({"maxQueued": 8, "priorities": 2})
    await run({"maxQueued": 8, "priorities": 2, "order": "adaptive",
               "lifoAfter": 100})
    print("interactive requests served in time: %d without the option, "
          "%d with it" % (plain["interactive"][0],
                          bounded["interactive"][0]))


if __name__ == "__main__":
    asyncio.run(main())
