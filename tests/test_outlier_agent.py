"""``outlierDetection`` on an agent's pools, against real localhost
servers: what an agent does on purpose (closing after a non-keep-alive
response, closing on abort) is not held against a backend; socket
errors under a request and failing pings are."""

import asyncio
import socket
import struct

from cueball_amd.agent import HttpAgent
from cueball_amd.http_client import HttpParseError, HttpRequest
from cueball_amd.resolver import StaticIpResolver
from cueball_amd.testing import MockHttpServer

RECOVERY = {"default": {"timeout": 2000, "retries": 2, "delay": 50,
                        "maxDelay": 200}}
DEADLINE = 10.0


def run(coro):
    loop = asyncio.new_event_loop()
    # a reset under a request with no error listener of the user's is
    # re-raised into the loop by design; keep the log quiet about it
    loop.set_exception_handler(lambda loop, ctx: None)
    try:
        return loop.run_until_complete(coro)
    finally:
        loop.close()


async def until(cond, what, deadline=DEADLINE):
    """Poll `cond` every few ms; no wait here is open-ended."""
    loop = asyncio.get_running_loop()
    end = loop.time() + deadline
    while not cond():
        assert loop.time() < end, "timed out waiting for " + what
        await asyncio.sleep(0.005)


async def stop_agent(agent):
    fut = asyncio.get_running_loop().create_future()
    agent.stop(lambda err: fut.set_result(err))
    await asyncio.wait_for(fut, DEADLINE)


class ResetServer:
    """Accepts, and while ``bad`` is set answers the first byte of a
    request with a TCP reset; otherwise answers 200 like a keep-alive
    HTTP server."""

    def __init__(self):
        self.bad = True
        self.resets = 0
        self.served = 0
        self.port = None
        self._server = None

    async def start(self):
        self._server = await asyncio.start_server(
            self._handle, "127.0.0.1", 0)
        self.port = self._server.sockets[0].getsockname()[1]

    def stop(self):
        self._server.close()

    async def _handle(self, reader, writer):
        try:
            while True:
                data = await reader.read(4096)
                if not data:
                    break
                if self.bad:
                    self.resets += 1
                    sock = writer.get_extra_info("socket")
                    sock.setsockopt(socket.SOL_SOCKET, socket.SO_LINGER,
                                    struct.pack("ii", 1, 0))
                    break
                self.served += 1
                writer.write(b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\n"
                             b"Connection: keep-alive\r\n\r\nok")
                await writer.drain()
        except (ConnectionResetError, BrokenPipeError):
            pass
        finally:
            writer.close()


def only_backend(agent, host):
    st = agent.get_outlier_stats()[host]["backends"]
    assert len(st) == 1
    return list(st.values())[0]


async def request(agent, host, path):
    """One request; the response, or the error it failed with."""
    try:
        return await asyncio.wait_for(
            agent.request_async(host, "GET", path), DEADLINE)
    except (OSError, HttpParseError) as e:
        return e


def quiet(pool):
    st = pool.get_stats()
    return st["waiterCount"] == 0 and \
        st["idleConnections"] + st["pendingConnections"] == \
        st["totalConnections"]


def test_what_an_agent_does_on_purpose_is_neutral():
    async def body():
        srv = MockHttpServer()
        await srv.start()
        agent = HttpAgent({
            "defaultPort": srv.port, "recovery": RECOVERY,
            "spares": 1, "maximum": 2,
            "outlierDetection": {"consecutiveFailures": 2,
                                 "baseEjectionTime": 300}})
        host = "127.0.0.1"
        resp = await request(agent, host, "/warm")
        assert resp.status_code == 200
        pool = agent.get_pool(host)
        await until(lambda: only_backend(agent, host)["successes"] == 1,
                    "the first success")

        # non-keep-alive responses: the lease is released after the
        # socket closed
        for _ in range(3):
            resp = await request(agent, host, "/close")
            assert resp.status_code == 200 and resp.body == b"bye"
            await until(lambda: quiet(pool), "the lease to end")

        # an abort with the socket in hand: the lease is closed
        # (an upload that never ends, so that no response can come
        # first)
        for _ in range(3):
            req = HttpRequest("POST", "/upload", host=host, streaming=True)
            req.on("error", lambda e: None)
            agent.add_request(req, host)
            req.write(b"some")
            await until(lambda: req.conn is not None, "a socket")
            req.abort()
            await until(lambda: quiet(pool), "the lease to end")

        rec = only_backend(agent, host)
        assert rec["failures"] == 0 and rec["consecutiveFailures"] == 0
        assert rec["successes"] == 1
        assert pool.get_stats()["counters"].get("ejection-refused", 0) == 0
        await stop_agent(agent)
        srv.stop()
    run(body())


def test_a_socket_error_under_a_request_counts():
    async def body():
        srv = ResetServer()
        await srv.start()
        agent = HttpAgent({
            "defaultPort": srv.port, "recovery": RECOVERY,
            "spares": 1, "maximum": 2,
            "outlierDetection": {"consecutiveFailures": 2,
                                 "baseEjectionTime": 300}})
        host = "127.0.0.1"
        for n in (1, 2):
            res = await request(agent, host, "/x")
            assert isinstance(res, Exception)
            await until(lambda: only_backend(agent, host)["failures"] == n,
                        "failure %d" % n)
        assert only_backend(agent, host)["consecutiveFailures"] == 2
        # the only backend there is: never ejected
        pool = agent.get_pool(host)
        assert pool.get_stats()["counters"]["ejection-refused"] == 1
        assert agent.get_outlier_stats()[host]["ejected"] == 0
        srv.bad = False
        res = await request(agent, host, "/x")
        assert res.status_code == 200
        await until(
            lambda: only_backend(agent, host)["consecutiveFailures"] == 0,
            "the streak to reset")
        await stop_agent(agent)
        srv.stop()
    run(body())


def test_a_failing_ping_counts():
    async def body():
        srv = MockHttpServer()
        await srv.start()
        agent = HttpAgent({
            "defaultPort": srv.port, "recovery": RECOVERY,
            "spares": 1, "maximum": 2,
            "ping": "/err500", "pingInterval": 40,
            "outlierDetection": {"consecutiveFailures": 2,
                                 "baseEjectionTime": 300}})
        host = "127.0.0.1"
        resp = await request(agent, host, "/warm")
        assert resp.status_code == 200
        await until(lambda: only_backend(agent, host)["failures"] >= 2,
                    "two failed pings")
        rec = only_backend(agent, host)
        assert rec["consecutiveFailures"] >= 2
        await stop_agent(agent)
        srv.stop()
    run(body())


def test_an_answering_ping_does_not_reset_the_streak():
    async def body():
        srv = ResetServer()
        await srv.start()
        # ResetServer answers any request with 200 once it is good
        agent = HttpAgent({
            "defaultPort": srv.port, "recovery": RECOVERY,
            "spares": 1, "maximum": 2,
            "ping": "/health", "pingInterval": 40,
            "outlierDetection": {"consecutiveFailures": 5,
                                 "baseEjectionTime": 300}})
        host = "127.0.0.1"
        res = await request(agent, host, "/x")
        assert isinstance(res, Exception)
        await until(lambda: only_backend(agent, host)["failures"] == 1,
                    "the failure")
        srv.bad = False
        served = srv.served
        await until(lambda: srv.served >= served + 3, "three pings")
        rec = only_backend(agent, host)
        assert rec["consecutiveFailures"] == 1 and rec["successes"] == 0
        await stop_agent(agent)
        srv.stop()
    run(body())


def test_a_host_pool_ejects_and_reinstates():
    async def body():
        good = MockHttpServer()
        bad = ResetServer()
        await good.start()
        await bad.start()
        res = StaticIpResolver({"backends": [
            {"address": "127.0.0.1", "port": good.port},
            {"address": "127.0.0.1", "port": bad.port}]})
        agent = HttpAgent({
            "recovery": RECOVERY, "spares": 2, "maximum": 4,
            "outlierDetection": {"consecutiveFailures": 2,
                                 "baseEjectionTime": 300}})
        agent.create_pool("foobar", {"resolver": res})
        res.start()
        pool = agent.get_pool("foobar")
        events = []
        pool.on("backendEjected",
                lambda key, info: events.append(("ejected", key, info)))
        pool.on("backendReinstated",
                lambda key, why: events.append(("reinstated", key, why)))

        loop = asyncio.get_running_loop()
        end = loop.time() + DEADLINE
        while not events:
            assert loop.time() < end, "no ejection"
            await request(agent, "foobar", "/x")
        bad_key = events[0][1]
        assert pool.p_backends[bad_key]["port"] == bad.port
        assert events[0][2] == {"reason": "consecutive-failures",
                                "durationMs": 300, "ejections": 1}
        assert bad.resets == 2
        stats = agent.get_outlier_stats()["foobar"]
        assert stats["ejected"] == 1
        assert stats["backends"][bad_key]["ejected"] is True

        # while it is out every request is answered, by the good server
        n = 0
        while len(events) == 1:
            assert loop.time() < end, "no reinstatement"
            out = pool.get_outlier_stats()["ejected"] == 1
            resp = await request(agent, "foobar", "/y")
            if out and len(events) == 1:
                assert resp.status_code == 200
                n += 1
        assert n > 0 and bad.resets == 2
        assert events[1] == ("reinstated", bad_key, "expired")

        # by hand, through the agent
        assert agent.eject_backend("foobar", bad_key, 60_000) is True
        assert agent.get_outlier_stats()["foobar"]["ejected"] == 1
        assert agent.reinstate_backend("foobar", bad_key) is True
        assert events[-1] == ("reinstated", bad_key, "manual")
        assert agent.get_outlier_stats()["foobar"]["ejected"] == 0
        await stop_agent(agent)
        good.stop()
        bad.stop()
    run(body())
