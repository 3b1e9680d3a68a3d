"""``concurrencyLimit`` on an agent, against real localhost HTTP servers:
the option reaches the per-host pools, a hedge is not sent into a
service at its limit, and a request the limit holds still honours the
retry option's ``totalTimeout``."""

import asyncio

import pytest

from cueball_amd.errors import RequestTimeoutError

from hedge_kit import hedge_counters, held_server
from retry_kit import (HOST, ScriptServer, finish, make_agent, request,
                       run, until)


def fixed(n):
    """A limit that stays where it is put."""
    return {"algorithm": "aimd", "latencyThreshold": 1e9,
            "initialLimit": n, "maxLimit": n}


def test_the_option_reaches_the_pools_and_the_stats_come_back():
    async def body():
        a = await ScriptServer().start()
        agent, pool = await make_agent(
            [a], None, concurrencyLimit={"probeSpread": 0, "maxLimit": 3})
        assert pool.p_cl["maxLimit"] == 3
        assert pool.p_cl["algorithm"] == "gradient"
        st = agent.get_limit_stats(HOST)
        assert st == pool.get_limit_stats()
        assert st["enabled"] is True and st["limit"] == 3.0
        assert st["probing"] is True
        for n in range(12):
            resp = await request(agent, "/%d" % n)
            assert resp.status_code == 200
        await asyncio.sleep(0.02)
        st = agent.get_limit_stats(HOST)
        assert st["samples"] == 12 and st["inFlight"] == 0
        assert st["probing"] is False and st["baselineMs"] > 0
        # every pool has a limit of its own
        b = await ScriptServer().start()
        from cueball_amd.resolver import StaticIpResolver
        res = StaticIpResolver({"backends": [
            {"address": "127.0.0.1", "port": b.port}]})
        agent.create_pool("svc.other", {"resolver": res})
        res.start()
        assert agent.get_limit_stats("svc.other")["samples"] == 0
        assert agent.get_pool("svc.other").p_cl_lim is not pool.p_cl_lim
        await finish(agent, a, b)

        plain, _ = await make_agent([await ScriptServer().start()], None)
        assert plain.get_limit_stats(HOST) == {"enabled": False}
        await finish(plain)
        with pytest.raises(ValueError):
            await make_agent([], None, concurrencyLimit={"bogus": 1})
        with pytest.raises(ValueError):
            # over the agent's maximum of 4
            await make_agent([], None, concurrencyLimit={"maxLimit": 5})
    run(body())


@pytest.mark.parametrize("limit,hedges", [(1, 0), (4, 1)])
def test_a_hedged_get_is_not_hedged_at_the_limit(limit, hedges):
    """Two servers that hold every request: the hedge delay runs out
    with an idle connection to the other server either way, and only a
    pool below its limit lets the hedge go."""
    async def body():
        one, release = await held_server()
        two = await ScriptServer(default=("hold", release)).start()
        agent, pool = await make_agent(
            [one, two], None, hedge={"delay": 20},
            concurrencyLimit=fixed(limit))
        task = asyncio.ensure_future(request(agent, "/held"))
        await until(lambda: len(one.paths) + len(two.paths) >= 1,
                    "the request to arrive")
        await asyncio.sleep(0.1)
        counters = hedge_counters(agent)
        assert counters["hedge-sent"] == hedges
        assert counters["hedge-skipped-no-idle"] == 1 - hedges
        assert len(one.paths) + len(two.paths) == 1 + hedges
        assert pool.get_stats()["idleConnections"] >= 1 or hedges
        assert agent.get_limit_stats(HOST)["inFlight"] == 1 + hedges
        release.set()
        resp = await task
        assert resp.status_code == 200
        await finish(agent, one, two)
    run(body())


def test_a_request_the_limit_holds_still_honours_total_timeout():
    async def body():
        server, release = await held_server()
        agent, pool = await make_agent(
            [server], {"delay": 1, "totalTimeout": 150},
            concurrencyLimit=fixed(1))
        # the holder is a plain request: no deadline of its own
        first = asyncio.ensure_future(request(agent, "/first", retry=False))
        await until(lambda: server.paths == ["/first"],
                    "the first request to arrive")
        loop = asyncio.get_running_loop()
        t0 = loop.time()
        res = await request(agent, "/second")
        took = loop.time() - t0
        assert isinstance(res, RequestTimeoutError) and res.kind == "total"
        assert 0.14 <= took < 1.0
        # it never left: an idle connection was there, the limit held it
        assert server.paths == ["/first"]
        counters = pool.get_stats()["counters"]
        assert counters["limit-held"] >= 1
        assert pool.get_stats()["waiterCount"] == 0
        release.set()
        resp = await first
        assert resp.status_code == 200
        await asyncio.sleep(0.02)
        assert agent.get_limit_stats(HOST)["inFlight"] == 0
        await finish(agent, server)
    run(body())
