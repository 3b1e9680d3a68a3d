"""Key affinity over real sockets on the deployment box (run with
-m gpu).

Three loopback line-echo servers behind one pool, spares 6: 120 claims
over 12 keys, each writing a line, awaiting the echo and releasing;
then one server is stopped and the same claims run again.  The
arithmetic is pinned on the virtual clock in test_affinity_pool.py;
this is about the plumbing: the native hash and rank, the native handle
and slot cycle under a Python ticket, real TCP, a backend that dies.
"""

import asyncio

import pytest

from cueball_amd.affinity import order as affinity_order

from balance_kit import DelayServer
from retry_kit import run, until

pytestmark = pytest.mark.gpu

KEYS = [b"tenant-%d" % i for i in range(12)]
CLAIMS = 120
RECOVERY = {"default": {"timeout": 2000, "retries": 2, "delay": 50,
                        "maxDelay": 200}}


def test_native_runtime_in_use():
    """Affinity must ride on the native handle and slot cycle, not
    replace them, and hash on the native core."""
    from cueball_amd import _speed
    from cueball_amd import affinity, connection_fsm, fsm, pool, queue
    assert fsm.FSM is _speed.FSM
    assert pool._native_pool_claim is _speed.pool_claim
    assert pool._NativeClaimTicket is _speed.ClaimTicket
    assert pool._NativeSlotDispatch is _speed.SlotDispatch
    assert issubclass(connection_fsm.ClaimHandle, _speed.ClaimHandleBase)
    assert connection_fsm._SlotKit is _speed.SlotKit
    assert queue.Queue is _speed.Queue
    assert affinity.fnv1a64 is _speed.affinity_hash
    assert affinity.rank is _speed.affinity_rank
    assert affinity.fnv1a64 is not affinity.PurePythonFnv1a64


async def claims(pool, errors):
    """CLAIMS sequential keyed claims; {key: set of backend keys that
    served it}."""
    loop = asyncio.get_running_loop()
    served = {}
    for n in range(CLAIMS):
        key = KEYS[n % len(KEYS)]
        line = b"line %d\n" % n
        done = loop.create_future()

        def cb(err, hdl=None, conn=None, key=key, line=line, done=done):
            if err is not None:
                errors.append(err)
                done.set_result(None)
                return
            got = []

            def on_data(chunk):
                got.append(chunk)
                if b"".join(got).endswith(b"\n"):
                    conn.remove_listener("data", on_data)
                    if b"".join(got) != line:
                        errors.append((line, b"".join(got)))
                    served.setdefault(key, set()).add(
                        hdl.get_backend()["key"])
                    hdl.release()
                    done.set_result(None)

            conn.on("data", on_data)
            conn.write(line)

        pool.claim({"timeout": 5000, "affinityKey": key}, cb)
        await asyncio.wait_for(done, 10.0)
        # the pool hears of the release a loop turn later
        await asyncio.sleep(0)
    return served


def test_keys_stick_to_their_server_and_fail_over_over_real_sockets():
    async def body():
        from cueball_amd.connection import tcp_constructor
        from cueball_amd.pool import ConnectionPool
        from cueball_amd.resolver import StaticIpResolver

        loop = asyncio.get_running_loop()
        servers = [await DelayServer(http=False).start() for _ in range(3)]
        resolver = StaticIpResolver({"backends": [
            {"address": "127.0.0.1", "port": s.port} for s in servers]})
        pool = ConnectionPool({
            "domain": "affinity.box", "constructor": tcp_constructor(loop=loop),
            "resolver": resolver, "recovery": RECOVERY, "spares": 6,
            "maximum": 6, "loop": loop, "claimAffinity": {}})
        resolver.start()
        await until(lambda: pool.get_stats()["idleConnections"] == 6,
                    "the spares to connect")
        assert sorted(len(v) for v in pool.p_connections.values()) == \
            [2, 2, 2]
        by_port = {s.port: s for s in servers}
        server_of = {k: by_port[b["port"]]
                     for k, b in pool.p_backends.items()}
        order = {key: pool.get_affinity_order(key) for key in KEYS}
        assert order == {key: affinity_order(key, list(server_of))
                         for key in KEYS}

        # 1. every key on its first choice
        errors = []
        served = await claims(pool, errors)
        assert errors == []
        for key in KEYS:
            assert served[key] == {order[key][0]}, key
        counters = dict(pool.get_stats()["counters"])
        assert counters["affinity-hit"] == CLAIMS
        assert counters["affinity-claim"] == CLAIMS
        assert sum(s.served for s in servers) == CLAIMS
        per = CLAIMS // len(KEYS)
        for k, s in server_of.items():
            assert s.served == per * sum(
                1 for key in KEYS if order[key][0] == k)

        # 2. the first choice of the most keys goes away
        firsts = [order[key][0] for key in KEYS]
        gone = max(sorted(set(firsts)), key=firsts.count)
        orphans = [key for key in KEYS if order[key][0] == gone]
        assert len(orphans) >= 2, \
            "inconclusive: %d keys on the stopped server" % len(orphans)
        server_of[gone].stop()
        await until(lambda: not any(
            fsm.is_in_state("idle") or fsm.is_in_state("busy")
            for fsm in pool.p_connections.get(gone, ())),
            "the stopped server's connections to go")
        await until(lambda: pool.get_stats()["idleConnections"] >= 4,
                    "the other servers' connections to be idle")

        errors = []
        before = {k: s.served for k, s in server_of.items()}
        served = await claims(pool, errors)
        assert errors == []
        # DNS still lists the server: the orders have not changed
        assert {key: pool.get_affinity_order(key) for key in KEYS} == order
        for key in KEYS:
            if key in orphans:
                assert served[key] == {order[key][1]}, key
            else:
                assert served[key] == {order[key][0]}, key
        counters = dict(pool.get_stats()["counters"])
        print("stopped", gone, "orphans", len(orphans), "counters", counters)
        assert counters["affinity-hit"] == \
            2 * CLAIMS - per * len(orphans)
        assert counters["affinity-spill-busy"] == per * len(orphans)
        assert counters["affinity-claim"] == 2 * CLAIMS
        assert counters.get("affinity-spill-load", 0) == 0
        assert counters.get("affinity-queued", 0) == 0
        assert server_of[gone].served == before[gone]
        assert sum(s.served for s in servers) == 2 * CLAIMS
        st = pool.get_affinity_stats()
        assert st["claims"] == 2 * CLAIMS
        assert st["backends"][gone]["firstChoice"] == 2 * per * len(orphans)
        assert st["backends"][gone]["placed"] == per * len(orphans)

        stopped = loop.create_future()
        pool.on("stateChanged",
                lambda st: st == "stopped" and stopped.set_result(None))
        pool.stop()
        await asyncio.wait_for(stopped, 10.0)
        for s in servers:
            s.stop()
    run(body())
