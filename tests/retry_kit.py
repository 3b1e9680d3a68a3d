"""Shared fixtures of the retry tests.

For the tests over real sockets: ``ScriptServer``, a small keep-alive
HTTP server whose every answer is scripted, per connection or per
request (reset, hang, a status, hold until released), and which records
which path it served; ``make_agent`` puts a set of them behind one
StaticIpResolver.  For the driver tests on a VirtualLoop: ``FakeTry``
and ``Tries``, the scripted stand-ins for "start one try".
"""

import asyncio
import collections
import socket
import struct

from cueball_amd.agent import HttpAgent
from cueball_amd.events import EventEmitter
from cueball_amd.http_client import HttpParseError
from cueball_amd.resolver import StaticIpResolver

RECOVERY = {"default": {"timeout": 2000, "retries": 2, "delay": 50,
                        "maxDelay": 200}}
DEADLINE = 10.0
HOST = "svc.retry"

REASONS = {200: b"OK", 404: b"Not Found", 500: b"Internal Server Error",
           502: b"Bad Gateway", 503: b"Service Unavailable",
           504: b"Gateway Timeout"}


def run(coro):
    loop = asyncio.new_event_loop()
    # a reset under a request is re-raised into the loop by the claim
    # handle when the socket has no error listener of the user's, by
    # design; keep the log quiet about it
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


async def stop_servers(*servers):
    """Stop the servers and wait until their connections are gone."""
    for s in servers:
        s.stop()
    await until(lambda: not any(s._writers for s in servers),
                "the servers' connections to close")


async def finish(agent, *servers):
    await stop_agent(agent)
    await stop_servers(*servers)


class ScriptServer:
    """Keep-alive HTTP/1.1 server with scripted answers.

    The action for a request is, in this order: the action its
    connection was given from ``conn_script`` when it was accepted (if
    that was not None), the next entry of ``script``, ``default``.  An
    action is one of

    - ``"ok"``: 200 with body ``ok``;
    - ``("status", code)``: that status, body ``code``, keep-alive;
    - ``"reset"``: a TCP reset instead of an answer;
    - ``"hang"``: no answer at all, until the peer hangs up;
    - ``("hold", event)``: 200 once the asyncio.Event is set.

    ``paths`` lists the path of every request received, ``actions`` the
    action each was given; ``conn_count`` counts accepted connections.
    """

    def __init__(self, default="ok"):
        self.default = default
        self.script = collections.deque()
        self.conn_script = collections.deque()
        self.paths = []
        self.actions = []
        self.methods = []
        self.conn_count = 0
        self.resets = 0
        self.hangs = 0
        self.hung_now = 0
        self.port = None
        self._server = None
        self._writers = set()

    async def start(self):
        self._server = await asyncio.start_server(
            self._handle, "127.0.0.1", 0)
        self.port = self._server.sockets[0].getsockname()[1]
        return self

    def stop(self):
        self._server.close()
        for w in list(self._writers):
            w.close()

    def count(self, action):
        return self.actions.count(action)

    async def _read_request(self, reader):
        head = b""
        while b"\r\n\r\n" not in head:
            data = await reader.read(4096)
            if not data:
                return None
            head += data
        head, _, rest = head.partition(b"\r\n\r\n")
        lines = head.decode("latin-1").split("\r\n")
        method, path = lines[0].split()[:2]
        clen = 0
        for line in lines[1:]:
            name, _, value = line.partition(":")
            if name.strip().lower() == "content-length":
                clen = int(value)
        while len(rest) < clen:
            data = await reader.read(4096)
            if not data:
                return None
            rest += data
        return method, path

    async def _handle(self, reader, writer):
        self.conn_count += 1
        self._writers.add(writer)
        conn_action = self.conn_script.popleft() if self.conn_script \
            else None
        try:
            while True:
                req = await self._read_request(reader)
                if req is None:
                    break
                method, path = req
                action = conn_action
                if action is None:
                    action = self.script.popleft() if self.script \
                        else self.default
                self.methods.append(method)
                self.paths.append(path)
                self.actions.append(action)
                if action == "reset":
                    self.resets += 1
                    sock = writer.get_extra_info("socket")
                    sock.setsockopt(socket.SOL_SOCKET, socket.SO_LINGER,
                                    struct.pack("ii", 1, 0))
                    break
                if action == "hang":
                    self.hangs += 1
                    self.hung_now += 1
                    try:
                        # until the client gives up on us
                        await asyncio.wait_for(reader.read(1), DEADLINE)
                    finally:
                        self.hung_now -= 1
                    break
                code = 200
                if isinstance(action, tuple) and action[0] == "hold":
                    await asyncio.wait_for(action[1].wait(), DEADLINE)
                elif isinstance(action, tuple) and action[0] == "status":
                    code = action[1]
                body = b"ok" if code == 200 else str(code).encode()
                if method == "HEAD":
                    body = b""
                writer.write(b"HTTP/1.1 %d %s\r\nContent-Length: %d\r\n"
                             b"Connection: keep-alive\r\n\r\n%s"
                             % (code, REASONS.get(code, b"Status"),
                                len(body), body))
                await writer.drain()
        except (ConnectionResetError, BrokenPipeError, asyncio.TimeoutError):
            pass
        finally:
            self._writers.discard(writer)
            writer.close()


def served_by(path, *servers):
    """The ports of the servers that received `path`, in the order
    given, once per request."""
    return [s.port for s in servers for p in s.paths if p == path]


async def make_agent(servers, retry, **opts):
    """An HttpAgent with a pool ``HOST`` over `servers`, spares 2,
    maximum 4, waited for until one connection per server is idle."""
    res = StaticIpResolver({"backends": [
        {"address": "127.0.0.1", "port": s.port} for s in servers]})
    base = {"recovery": RECOVERY, "spares": 2, "maximum": 4}
    if retry is not None:
        base["retry"] = retry
    base.update(opts)
    agent = HttpAgent(base)
    agent.create_pool(HOST, {"resolver": res})
    res.start()
    pool = agent.get_pool(HOST)
    await until(lambda: pool.get_stats()["idleConnections"] >=
                min(2, len(servers)), "the spares to connect")
    return agent, pool


def key_of(pool, server):
    """The pool's backend key for `server`."""
    for k, b in pool.p_backends.items():
        if b["port"] == server.port:
            return k
    raise AssertionError("no backend on port %d" % server.port)


async def request(agent, path, method="GET", body=None, **kw):
    """One request; the response, or the error it failed with."""
    from cueball_amd.errors import CueballError
    try:
        return await asyncio.wait_for(
            agent.request_async(HOST, method, path, None, body, **kw),
            DEADLINE)
    except (OSError, HttpParseError, CueballError) as e:
        return e


def quiet(pool):
    st = pool.get_stats()
    return st["waiterCount"] == 0 and \
        st["idleConnections"] + st["pendingConnections"] == \
        st["totalConnections"]


def idle_keys(pool):
    """Backend keys of the idle queue, head first."""
    return [fsm.get_backend()["key"] for fsm in pool.p_idleq]


# -- the driver on a VirtualLoop -------------------------------------------

class FakeResponse(EventEmitter):
    def __init__(self, status, complete=True):
        super().__init__()
        self.status_code = status
        self.complete = complete

    def finish(self):
        self.complete = True
        self.emit("end")


class FakeHandle:
    """What the driver touches of a claim handle."""

    def __init__(self, state="claimed"):
        self.state = state
        self.reported = []

    def is_in_state(self, st):
        return self.state == st

    def report_failure(self, err=None):
        assert self.state == "claimed"
        self.reported.append(err)


class FakeTry(EventEmitter):
    """One scripted try: the test decides when it is claimed, answers
    or fails."""

    def __init__(self, avoid):
        super().__init__()
        self.avoid = avoid
        self.try_backend = None
        self.try_handle = None
        self.aborted = False

    def claimed(self, key):
        self.try_backend = key
        self.try_handle = FakeHandle()
        return self

    def abort(self):
        self.aborted = True
        self.emit("abort")

    def respond(self, status, complete=True):
        resp = FakeResponse(status, complete)
        self.emit("response", resp)
        return resp

    def fail(self, err):
        self.emit("error", err)

    def listeners_left(self):
        return sum(self.listener_count(e)
                   for e in ("response", "error", "abort"))


class Tries:
    """The injected "start one try": keeps every try it started."""

    def __init__(self):
        self.tries = []
        self.raises = None

    def __call__(self, avoid):
        if self.raises is not None:
            raise self.raises
        t = FakeTry(avoid)
        self.tries.append(t)
        return t

    @property
    def last(self):
        return self.tries[-1]


def timers(loop):
    """The loop's scheduled handles that are still live."""
    return [h for h in loop._scheduled if not h._cancelled]
