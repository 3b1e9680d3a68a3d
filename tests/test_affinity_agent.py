"""``claimAffinity`` on an agent, against three real localhost HTTP
servers: requests with an ``affinityKey=`` reach the server the key's
order names, and a retried one fails over to the key's second choice."""

import pytest

from cueball_amd.affinity import order as affinity_order

from balance_kit import DelayServer
from retry_kit import (HOST, ScriptServer, finish, key_of, make_agent,
                       request, run, served_by, until)

KEYS = ["user:%d" % i for i in range(6)]
REQUESTS = 30


async def three_idle(pool):
    await until(lambda: len({fsm.get_backend()["key"]
                             for fsm in pool.p_idleq
                             if fsm.is_in_state("idle")}) == 3,
                "a connection to every server")


def test_every_key_reaches_the_server_its_order_names():
    async def body():
        servers = [await DelayServer().start() for _ in range(3)]
        agent, pool = await make_agent(servers, None, spares=3, maximum=6,
                                       claimAffinity={})
        await three_idle(pool)
        by_key = {key_of(pool, s): s for s in servers}
        seen = {}
        for n in range(REQUESTS):
            key = KEYS[n % len(KEYS)]
            before = {k: s.served for k, s in by_key.items()}
            # str and bytes are one key
            resp = await request(agent, "/%d" % n,
                                 affinityKey=key if n % 2 else key.encode())
            assert not isinstance(resp, Exception), (n, resp)
            assert resp.status_code == 200 and resp.body == b"ok"
            got = [k for k, s in by_key.items() if s.served > before[k]]
            assert len(got) == 1
            seen.setdefault(key, set()).add(got[0])
        for key in KEYS:
            assert seen[key] == {pool.get_affinity_order(key)[0]}, key
            assert pool.get_affinity_order(key) == \
                affinity_order(key, list(by_key))
        assert sum(s.served for s in servers) == REQUESTS

        st = agent.get_affinity_stats(HOST)
        assert st["enabled"] is True and st["loadFactor"] == 1.25
        assert st["claims"] == REQUESTS
        assert st["hits"] + st["spilledBusy"] + st["spilledLoad"] + \
            st["queued"] == st["claims"]
        assert st["hits"] == REQUESTS
        assert sum(v["placed"] for v in st["backends"].values()) == REQUESTS
        assert sum(v["firstChoice"]
                   for v in st["backends"].values()) == REQUESTS
        for k, s in by_key.items():
            assert st["backends"][k]["placed"] == s.served
        # a request without a key is none of affinity's business
        resp = await request(agent, "/plain")
        assert resp.status_code == 200
        assert agent.get_affinity_stats(HOST)["claims"] == REQUESTS
        await finish(agent, *servers)
    run(body())


def test_affinity_key_needs_the_option_and_a_key_type():
    async def body():
        server = await DelayServer().start()
        plain, _ = await make_agent([server], None)
        assert plain.get_affinity_stats(HOST) == {"enabled": False}
        with pytest.raises(ValueError):
            plain.request(HOST, "GET", "/", affinityKey="user:1")
        with pytest.raises(ValueError):
            await plain.request_async(HOST, "GET", "/", affinityKey=b"u")
        with pytest.raises(TypeError):
            plain.request(HOST, "GET", "/", affinityKey=7)
        assert server.served == 0
        assert plain.get_pool(HOST).get_stats()["counters"].get(
            "claim", 0) == 0
        await finish(plain, server)

        server = await DelayServer().start()
        on, _ = await make_agent([server], None, claimAffinity={})
        for bad in (7, 1.5, ["user:1"], bytearray(b"u")):
            with pytest.raises(TypeError):
                on.request(HOST, "GET", "/", affinityKey=bad)
        assert server.served == 0
        await finish(on, server)
    run(body())


def test_a_retried_keyed_get_ends_on_the_second_choice():
    async def body():
        servers = [await ScriptServer().start() for _ in range(3)]
        agent, pool = await make_agent(
            servers, {"maxRetries": 2, "delay": 1, "maxDelay": 2},
            spares=3, maximum=6, claimAffinity={})
        await three_idle(pool)
        by_key = {key_of(pool, s): s for s in servers}
        order = pool.get_affinity_order("user:42")
        first, second = by_key[order[0]], by_key[order[1]]
        first.default = "reset"
        resp = await request(agent, "/failover", affinityKey="user:42")
        assert not isinstance(resp, Exception), resp
        assert resp.status_code == 200
        assert served_by("/failover", *servers) in (
            [first.port, second.port], [second.port, first.port])
        assert first.resets == 1 and second.paths == ["/failover"]
        assert by_key[order[2]].paths == []
        st = agent.get_affinity_stats(HOST)
        # both tries were keyed claims, and each got the first backend
        # of the order that it did not avoid
        assert st["claims"] == 2 and st["hits"] == 2
        assert st["backends"][order[0]]["placed"] == 1
        assert st["backends"][order[1]]["placed"] == 1
        await finish(agent, *servers)
    run(body())
