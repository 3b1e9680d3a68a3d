"""Key affinity: the same key goes to the same backend.

Runs self-contained on three loopback servers that stand for a sharded
cache: each answers ``hit`` for a key it has seen before and ``miss``
otherwise.  240 requests over 11 tenants, one after the other, through
two pools with two connections per server:

- without ``claimAffinity``: round-robin over the idle connections, so
  every server has to learn every tenant;
- with ``claimAffinity: {}`` and the tenant as the claim's
  ``affinityKey``: every tenant has its server, and only the first
  request of each is a miss.

Then one server is stopped: its tenants move to their second choice,
everybody else stays where they were.
"""

import asyncio
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cueball_amd
from cueball_amd.connection import tcp_constructor

RECOVERY = {"default": {"timeout": 2000, "retries": 2, "delay": 50,
                        "maxDelay": 200}}
TENANTS = ["tenant-%d" % i for i in range(11)]
REQUESTS = 240


class CacheServer:
    def __init__(self):
        self.seen = set()
        self.writers = set()

    async def start(self):
        self.server = await asyncio.start_server(
            self.handle, "127.0.0.1", 0)
        self.port = self.server.sockets[0].getsockname()[1]
        return self

    async def handle(self, reader, writer):
        self.writers.add(writer)
        try:
            while line := await reader.readline():
                writer.write(b"hit\n" if line in self.seen else b"miss\n")
                self.seen.add(line)
                await writer.drain()
        except ConnectionError:
            pass
        self.writers.discard(writer)
        writer.close()

    def stop(self):
        self.server.close()
        for w in list(self.writers):
            w.close()


async def lookup(pool, tenant, keyed):
    """One request for `tenant`; (answer, backend key)."""
    options = {"timeout": 5000}
    if keyed:
        options["affinityKey"] = tenant
    handle, conn = await pool.claim_async(options)
    got = asyncio.get_running_loop().create_future()
    listener = conn.on(
        "data", lambda d: (not got.done()) and got.set_result(d))
    conn.write(tenant.encode() + b"\n")
    answer = (await got).strip().decode()
    conn.remove_listener("data", listener)
    backend = handle.get_backend()["key"]
    handle.release()
    await asyncio.sleep(0)
    return answer, backend


async def drive(pool, keyed):
    hits = 0
    where = {}
    for n in range(REQUESTS):
        tenant = TENANTS[n % len(TENANTS)]
        answer, backend = await lookup(pool, tenant, keyed)
        hits += answer == "hit"
        where.setdefault(tenant, set()).add(backend)
    return hits, where


async def run(affinity):
    servers = [await CacheServer().start() for _ in range(3)]
    resolver = cueball_amd.StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": s.port} for s in servers]})
    options = {
        "domain": "cache.local",
        "resolver": resolver,
        "constructor": tcp_constructor(),
        "spares": 6,
        "maximum": 6,
        "recovery": RECOVERY,
    }
    if affinity is not None:
        options["claimAffinity"] = affinity
    pool = cueball_amd.ConnectionPool(options)
    resolver.start()
    while pool.get_stats()["idleConnections"] < 6:
        await asyncio.sleep(0.01)

    keyed = affinity is not None
    hits, where = await drive(pool, keyed)
    print("  %d of %d requests were cache hits; a tenant was served by "
          "%.1f servers on average"
          % (hits, REQUESTS,
             sum(len(v) for v in where.values()) / len(where)))

    if keyed:
        st = pool.get_affinity_stats()
        print("  hits %(hits)d, spilled busy %(spilledBusy)d, spilled load "
              "%(spilledLoad)d, queued %(queued)d" % st)
        # stop the server that is first choice of the most tenants
        firsts = [pool.get_affinity_order(t)[0] for t in TENANTS]
        gone = max(sorted(set(firsts)), key=firsts.count)
        port = pool.p_backends[gone]["port"]
        [s for s in servers if s.port == port][0].stop()
        while any(fsm.is_in_state("idle") or fsm.is_in_state("busy")
                  for fsm in pool.p_connections.get(gone, ())) or \
                pool.get_stats()["idleConnections"] < 4:
            await asyncio.sleep(0.01)
        _, after = await drive(pool, keyed)
        moved = [t for t in TENANTS if after[t] != where[t]]
        print("  one server stopped: %d tenants moved, all of them its own "
              "(%s), each to its second choice (%s)"
              % (len(moved),
                 all(pool.get_affinity_order(t)[0] == gone for t in moved),
                 all(after[t] == {pool.get_affinity_order(t)[1]}
                     for t in moved)))

    stopped = asyncio.get_running_loop().create_future()
    pool.on("stateChanged",
            lambda st: st == "stopped" and stopped.set_result(None))
    pool.stop()
    await asyncio.wait_for(stopped, 10)
    for s in servers:
        s.stop()


async def main():
    print("without claimAffinity:")
    await run(None)
    print("with claimAffinity:")
    await run({})


if __name__ == "__main__":
    asyncio.run(main())
