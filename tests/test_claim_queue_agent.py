"""``claimQueue`` and ``priority=`` on an agent, against loopback HTTP
servers that answer after a delay: one connection per pool, so that
every request behind the first has to wait for it."""

import asyncio

from cueball_amd.errors import ClaimQueueFullError
from cueball_amd.utils import RETRY_REASONS

from balance_kit import DelayServer
from retry_kit import (HOST, finish, make_agent, quiet, request, run,
                       until)

DELAY = 0.05


def spy_claims(pool):
    """Record the options of every claim the pool is asked for."""
    seen = []
    real = pool.claim

    def claim(options=None, cb=None):
        seen.append(dict(options) if isinstance(options, dict) else options)
        return real(options, cb)

    pool.claim = claim
    return seen


def waiting(pool):
    return [hdl.ch_priority for hdl in pool.p_waiters]


async def one_connection(cq, retry=None, **opts):
    server = await DelayServer(delay=DELAY).start()
    agent, pool = await make_agent([server], retry, spares=1, maximum=1,
                                   claimQueue=cq, **opts)
    return server, agent, pool, spy_claims(pool)


def test_priority_reaches_the_pool():
    async def body():
        server, agent, pool, claims = await one_connection(
            {"priorities": 3, "defaultPriority": 1})
        done = []

        def go(path, **kw):
            async def one():
                resp = await request(agent, path, **kw)
                done.append((path, getattr(resp, "status_code", resp)))
            return asyncio.ensure_future(one())

        tasks = [go("/first")]
        await until(lambda: pool.get_stats()["idleConnections"] == 0,
                    "the first request to claim")
        tasks += [go("/low", priority=2), go("/plain"),
                  go("/high", priority=0), go("/mid", priority=1)]
        await until(lambda: len(waiting(pool)) == 4, "the claims to queue")
        assert waiting(pool) == [0, 1, 1, 2]
        assert agent.get_queue_stats(HOST)["queued"] == [1, 2, 1]
        assert [c.get("priority") for c in claims] == [None, 2, None, 0, 1]
        await asyncio.gather(*tasks)
        assert done == [("/first", 200), ("/high", 200), ("/plain", 200),
                        ("/mid", 200), ("/low", 200)]
        assert server.served == 5
        await finish(agent, server)
    run(body())


def test_a_full_queue_fails_the_request():
    async def body():
        server, agent, pool, claims = await one_connection(
            {"maxQueued": 1, "priorities": 2, "defaultPriority": 1})
        first = asyncio.ensure_future(request(agent, "/first"))
        await until(lambda: pool.get_stats()["idleConnections"] == 0,
                    "the first request to claim")
        second = asyncio.ensure_future(request(agent, "/second"))
        await until(lambda: waiting(pool) == [1], "the second to queue")
        third = await request(agent, "/third")
        assert isinstance(third, ClaimQueueFullError)
        assert third.displaced is False and third.pool is pool
        # a more urgent request takes the place of the one that waits
        urgent = asyncio.ensure_future(
            request(agent, "/urgent", priority=0))
        got = await second
        assert isinstance(got, ClaimQueueFullError) and got.displaced is True
        assert waiting(pool) == [0]
        assert (await first).status_code == 200
        assert (await urgent).status_code == 200
        st = agent.get_queue_stats(HOST)
        assert (st["rejected"], st["shed"]) == (1, 1)
        assert server.served == 2
        assert len(claims) == 4
        await finish(agent, server)
    run(body())


def test_under_retry_a_full_queue_costs_one_attempt_and_no_budget():
    async def body():
        retry = {"maxRetries": 3, "retryOn": list(RETRY_REASONS),
                 "delay": 1, "maxDelay": 2}
        server, agent, pool, claims = await one_connection(
            {"maxQueued": 1}, retry)
        first = asyncio.ensure_future(request(agent, "/first"))
        await until(lambda: pool.get_stats()["idleConnections"] == 0,
                    "the first request to claim")
        second = asyncio.ensure_future(request(agent, "/second"))
        await until(lambda: len(waiting(pool)) == 1, "the second to queue")
        before = len(claims)
        third = await request(agent, "/third", priority=0)
        assert isinstance(third, ClaimQueueFullError)
        assert third.displaced is False
        # one try, one claim: the pool said it is overloaded
        assert len(claims) == before + 1
        assert claims[-1].get("priority") == 0
        assert (await first).status_code == 200
        assert (await second).status_code == 200
        stats = agent.get_retry_stats()[HOST]
        assert stats["retrying"] == 0 and stats["active"] == 0
        assert not any(stats["counters"].values()), stats
        assert len(claims) == 3 and server.served == 2
        await finish(agent, server)
    run(body())


def test_under_hedge_the_keyword_reaches_the_second_attempt():
    async def body():
        servers = [await DelayServer(delay=0.1).start() for _ in range(2)]
        agent, pool = await make_agent(
            servers, None, spares=2, maximum=2, hedge={"delay": 20},
            claimQueue={"priorities": 2})
        claims = spy_claims(pool)
        resp = await request(agent, "/hedged", priority=1)
        assert resp.status_code == 200
        assert agent.get_hedge_stats()[HOST]["counters"]["hedge-sent"] == 1
        assert len(claims) == 2
        assert [c.get("priority") for c in claims] == [1, 1]
        assert claims[1].get("avoidBackends")
        # without the keyword no attempt names a class
        await until(lambda: pool.get_stats()["idleConnections"] == 2,
                    "the attempt that lost to be replaced")
        resp = await request(agent, "/plain")
        assert resp.status_code == 200
        assert len(claims) > 2
        assert [c.get("priority") for c in claims[2:]] == \
            [None] * (len(claims) - 2)
        # the keyword alone, with the driver switched off for the call
        await until(lambda: pool.get_stats()["idleConnections"] >= 1,
                    "an idle connection")
        resp = await request(agent, "/direct", priority=1, hedge=False)
        assert resp.status_code == 200
        assert claims[-1].get("priority") == 1
        assert "avoidBackends" not in claims[-1]
        await until(lambda: quiet(pool), "the pool to settle")
        await finish(agent, *servers)
    run(body())
