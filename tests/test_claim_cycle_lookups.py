"""The claim cycle after per-claim lookups were cut from it: the leak
detector's cache and the claimed state's one registration show a claimer
what the pure-Python runtime shows, and so do the handle's entry table and
the loops' flush batches, which were worked on and left as they were.

Pools here have 1 or 2 backends on the virtual clock.  Scenarios return
plain data; they run on the runtime this process selected and once more,
all together, in a child process on the pure-Python runtime, and the
results are compared.  What is about the native core's own objects is
native only.
"""

import asyncio
import gc
import json
import logging
import math
import os
import re
import subprocess
import sys
import weakref

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from cueball_amd import fsm as mod_fsm  # noqa: E402
from cueball_amd import pool as mod_pool  # noqa: E402
from cueball_amd.connection_fsm import ClaimHandle  # noqa: E402
from cueball_amd.events import PurePythonEventEmitter  # noqa: E402
from cueball_amd.latency import PoolLatency  # noqa: E402
from cueball_amd.logutil import default_logger  # noqa: E402
from cueball_amd.pool import ConnectionPool  # noqa: E402
from cueball_amd.resolver import ResolverFSM  # noqa: E402
from cueball_amd.testing import (DummyConnection, DummyResolver,  # noqa: E402
                                 VirtualLoop, advance, settle)

RECOVERY = {"default": {"timeout": 500, "retries": 1, "delay": 0}}
LEAK_EVENTS = ("close", "error", "readable", "data")

native_only = pytest.mark.skipif(
    not mod_fsm.NATIVE, reason="about the native core's own objects")


def cycle_state(emitter=None):
    from cueball_amd import _speed
    if emitter is None:
        return _speed._debug_cycle_state()
    return _speed._debug_cycle_state(emitter)


def run_vt(body):
    loop = VirtualLoop()
    try:
        return loop.run_until_complete(body(loop))
    finally:
        loop.close()


class Kit:
    """A pool of `n` backends, one connected connection each."""

    def __init__(self, loop, n=1, conn_cls=DummyConnection):
        self.loop = loop
        self.n = n
        self.conns = []
        self.keep = []
        self.resolver = DummyResolver()
        self.rfsm = ResolverFSM(self.resolver, {"loop": loop})

        def constructor(backend):
            c = conn_cls(backend)
            self.conns.append(c)
            return c

        self.pool = ConnectionPool({
            "domain": "lookups.test", "constructor": constructor,
            "recovery": RECOVERY, "spares": n, "maximum": n,
            "resolver": self.rfsm, "loop": loop})
        self.rfsm.start()

    async def up(self):
        for i in range(self.n):
            self.resolver.add("b%d" % (i + 1), {})
        await settle(self.loop)
        for c in list(self.conns):
            c.connect()
        await settle(self.loop)
        assert self.pool.get_stats()["idleConnections"] == self.n
        return self

    def slot(self, key="b1"):
        (slot,) = self.pool.p_connections[key]
        return slot

    async def claim(self, options=None):
        box = {}

        def cb(err, hdl=None, conn=None):
            box.update(err=err, hdl=hdl, conn=conn)

        box["ret"] = self.pool.claim(options or {}, cb)
        await settle(self.loop)
        return box

    async def cycle(self, during=None):
        """One claim and release; `during(conn)` runs while claimed."""
        box = await self.claim()
        assert box["err"] is None
        if during is not None:
            during(box["conn"])
        box["hdl"].release()
        await settle(self.loop)
        return box

    async def cycles(self, n, each=None):
        """n claim/release cycles, each claim made in the callback of
        the one before."""
        pool = self.pool
        left = {"n": n}
        done = self.loop.create_future()

        def cb(err, hdl=None, conn=None):
            assert err is None
            hdl.release()
            if each is not None:
                each()
            left["n"] -= 1
            if left["n"] > 0:
                pool.claim({}, cb)
            else:
                done.set_result(None)

        self.keep.append(cb)
        pool.claim({}, cb)
        while not done.done():
            await settle(self.loop)
        await settle(self.loop)

    async def stop(self):
        self.pool.stop()
        await settle(self.loop)
        if not self.pool.is_in_state("stopped"):
            await advance(self.loop, 10.0)
        assert self.pool.is_in_state("stopped")


class FakePool:
    """no FSM, no queues: only what a bare handle asks of its pool"""

    def __init__(self, loop):
        self.p_lat = PoolLatency(loop)
        self.counted = []

    def _incr_counter(self, name):
        self.counted.append(name)


class StandingSlot:
    """stands still in the handshake: claim() neither accepts nor
    rejects"""

    def is_in_state(self, st):
        return st == "idle"

    def get_state(self):
        return "idle"

    def claim(self, handle):
        pass


def bare_handle(pool, loop, called=None):
    return ClaimHandle({
        "pool": pool, "claimStack": [], "log": default_logger(),
        "callback": (lambda *a: called.append(a)) if called is not None
        else (lambda *a: None),
        "claimTimeout": math.inf, "loop": loop})


def _noop(*a):
    pass


def _internal(*a):
    pass


_internal._cueball_internal = True


class _ListHandler(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


#: The two runtimes word the leak warning differently, and always did:
#: the native core puts the numbers into the text, the pure-Python handle
#: passes them as log fields.  Both are read back as [event, before,
#: after], which is what the two must agree on.
_LEAK_RE = re.compile(
    r"leaked event handlers"
    r"(?: \(event=(\w+) before=(\d+) after=(\d+)\)"
    r"| \[.*\bevent=(\w+), count_before_claim=(\d+), "
    r"count_after_release=(\d+))")


class logged:
    """the warnings of the "cueball" logger while the block runs"""

    def __enter__(self):
        self.handler = _ListHandler()
        logging.getLogger("cueball").addHandler(self.handler)
        return self

    def __exit__(self, *exc):
        logging.getLogger("cueball").removeHandler(self.handler)

    def leaks(self):
        out = []
        for m in self.handler.messages:
            if "leaked" not in m:
                continue
            g = _LEAK_RE.search(m)
            assert g is not None, m
            ev, before, after = [x for x in g.groups() if x is not None]
            out.append([ev, int(before), int(after)])
        return out

    def others(self):
        return [m.split(" [")[0] for m in self.handler.messages
                if "leaked" not in m]


# -- leak detector --------------------------------------------------------------

async def _leak_run(loop, during, between=None, before=None):
    """Five claims of one connection: nothing, `during`, nothing twice
    with `between` run on the idle connection in between, `during`
    again.  Returns the leak warnings."""
    with logged() as log:
        kit = await Kit(loop).up()
        conn = kit.conns[0]
        if before is not None:
            before(conn)
        await kit.cycle()
        await kit.cycle(during)
        await kit.cycle()
        if between is not None:
            between(conn)
        await kit.cycle()
        await kit.cycle(during)
        await kit.stop()
    return log.leaks()


def _sc_on(ev):
    async def sc(loop):
        return await _leak_run(loop, lambda conn: conn.on(ev, _noop))
    return sc


def _sc_once(ev):
    async def sc(loop):
        return await _leak_run(loop, lambda conn: conn.once(ev, _noop))
    return sc


def _with_data_list(conn):
    # a "data" list that both runtimes keep: it holds a listener the
    # detector does not count
    conn.on("data", _internal)


async def sc_events_append(loop):
    return await _leak_run(
        loop, lambda conn: conn._events["data"].append(_noop),
        before=_with_data_list)


async def sc_events_replace_same_length(loop):
    def during(conn):
        # one uncounted listener goes, one counted comes: the length of
        # the list is what it was
        ls = list(conn._events["data"])
        ls[0] = lambda *a: None
        conn._events["data"] = ls

    def between(conn):
        conn._events["data"] = [_internal]
    return await _leak_run(loop, during, between, before=_with_data_list)


async def sc_events_replace_other_length(loop):
    def during(conn):
        conn._events["data"] = list(conn._events["data"]) + [_noop]
    return await _leak_run(loop, during, before=_with_data_list)


async def sc_events_key_added(loop):
    def during(conn):
        assert "readable" not in conn._events
        conn._events["readable"] = [_noop]

    def between(conn):
        del conn._events["readable"]
    return await _leak_run(loop, during, between)


async def sc_events_key_deleted(loop):
    """A counted listener's list deleted on the idle connection: the next
    claim's "before" is 0 again, so putting one back is a leak."""
    def before(conn):
        conn.on("data", _noop)

    def during(conn):
        if "data" not in conn._events:
            conn._events["data"] = [_noop]

    def between(conn):
        del conn._events["data"]

    with logged() as log:
        kit = await Kit(loop).up()
        conn = kit.conns[0]
        before(conn)
        await kit.cycle()
        await kit.cycle(during)         # the list is there: nothing
        between(conn)
        await kit.cycle(during)         # 0 -> 1
        await kit.cycle()
        await kit.stop()
    return log.leaks()


async def sc_added_and_removed(loop):
    def during(conn):
        for ev in LEAK_EVENTS:
            ls = conn.on(ev, _noop)
            conn.remove_listener(ev, ls)
            w = conn.once(ev, _noop)
            conn.remove_listener(ev, w)
    return await _leak_run(loop, during)


async def sc_two_claims_nothing_changed(loop):
    with logged() as log:
        kit = await Kit(loop).up()
        kit.conns[0].on("data", _noop)          # while idle: not a leak
        await kit.cycle()
        await kit.cycle()
        await kit.stop()
    return log.leaks()


#: what the detector counts on an idle connection of a pool: the socket
#: manager's own `close` listener (its `error` listener is marked as the
#: library's)
BASE = {"close": 1, "error": 0, "readable": 0, "data": 0}

LEAK_SCENARIOS = {}
for _ev in LEAK_EVENTS:
    _want = [[_ev, BASE[_ev], BASE[_ev] + 1],
             [_ev, BASE[_ev] + 1, BASE[_ev] + 2]]
    LEAK_SCENARIOS["on_" + _ev] = (_sc_on(_ev), _want)
    LEAK_SCENARIOS["once_" + _ev] = (_sc_once(_ev), _want)
LEAK_SCENARIOS.update({
    "events_append": (sc_events_append, [["data", 0, 1], ["data", 1, 2]]),
    "events_replace_same_length": (sc_events_replace_same_length,
                                   [["data", 0, 1], ["data", 0, 1]]),
    "events_replace_other_length": (sc_events_replace_other_length,
                                    [["data", 0, 1], ["data", 1, 2]]),
    "events_key_added": (sc_events_key_added,
                         [["readable", 0, 1], ["readable", 0, 1]]),
    "events_key_deleted": (sc_events_key_deleted, [["data", 0, 1]]),
    "added_and_removed": (sc_added_and_removed, []),
    "two_claims_nothing_changed": (sc_two_claims_nothing_changed, []),
})


# -- the claimed state's registration -------------------------------------------

def _marks(listeners):
    return [bool(getattr(cb, "_cueball_internal", False)) for cb in listeners]


async def sc_error_listener_on_a_kit_slot(loop):
    kit = await Kit(loop).up()
    conn = kit.conns[0]
    # the socket manager listens too, before and after: counted from there
    idle = conn.listeners("error")
    n = len(idle)
    out = {"idle": conn.listener_count("error") - n}
    box = await kit.claim()
    mine = [cb for cb in conn.listeners("error") if cb not in idle]
    out["claimed"] = [conn.listener_count("error") - n, _marks(mine)]
    box["hdl"].release()
    await settle(loop)
    out["released"] = conn.listener_count("error") - n
    box = await kit.claim()
    out["claimed_again"] = conn.listener_count("error") - n
    box["hdl"].close()
    await settle(loop)
    out["closed"] = [len([cb for cb in conn.listeners("error")
                          if cb in mine]), box["hdl"].get_state()]
    await kit.stop()
    return out


async def sc_error_listener_without_a_kit(loop):
    fake = FakePool(loop)
    conn = DummyConnection({})
    out = []
    for leave in ("release", "close"):
        h = bare_handle(fake, loop)
        h.try_(StandingSlot())
        out.append(conn.listener_count("error"))
        h.accept(conn)
        out.append([conn.listener_count("error"),
                    _marks(conn.listeners("error"))])
        getattr(h, leave)()
        out.append([conn.listener_count("error"), h.get_state()])
        await settle(loop)
    return out


class CountingConnection(DummyConnection):
    removed = None

    def remove_listener(self, event, listener):
        if self.removed is None:
            self.removed = []
        self.removed.append(event)
        return super().remove_listener(event, listener)


async def sc_remove_listener_overridden(loop):
    kit = await Kit(loop, conn_cls=CountingConnection).up()
    conn = kit.conns[0]
    conn.removed = []
    n = conn.listener_count("error")
    out = []
    for _ in range(3):
        box = await kit.claim()
        out.append([conn.removed.count("error"),
                    conn.listener_count("error") - n])
        box["hdl"].release()
        await settle(loop)
    out.append([conn.removed.count("error"),
                conn.listener_count("error") - n])
    await kit.stop()
    return out


async def sc_error_while_claimed(loop):
    """`error` on a claimed connection of a bare handle (no slot reacts):
    with a listener of the user's it is logged and counted, without one
    it is raised at the emitter."""
    out = {}
    with logged() as log:
        fake = FakePool(loop)
        conn = DummyConnection({})
        h = bare_handle(fake, loop)
        h.try_(StandingSlot())
        h.accept(conn)
        seen = []
        user = conn.on("error", lambda e: seen.append(str(e)))
        conn.emit("error", RuntimeError("with"))
        out["with"] = [seen, fake.counted, h.get_state()]
        conn.remove_listener("error", user)
        try:
            conn.emit("error", RuntimeError("without"))
            out["without"] = None
        except Exception as e:
            out["without"] = [type(e).__name__, str(e)]
        out["state"] = h.get_state()
        out["listeners"] = conn.listener_count("error")
        h.release()
        await settle(loop)
        out["after"] = conn.listener_count("error")
        # released: nobody listens any more
        out["emit_after"] = conn.emit("error", RuntimeError("late"))
    # the pure-Python handle goes on to name the claim callback
    out["log"] = [m[:len("connection emitted error while claimed")]
                  for m in log.others()]
    return out


async def sc_leave_from_the_callback(loop):
    out = []
    for leave in ("release", "close"):
        kit = await Kit(loop).up()
        conn = kit.conns[0]
        idle = conn.listeners("error")
        box = {}

        def cb(err, hdl=None, conn_=None):
            box["mine"] = [x for x in conn_.listeners("error")
                           if x not in idle]
            getattr(hdl, leave)()
            # the handle leaves `claimed` when its entry returns
            box["state"] = hdl.get_state()
            box["hdl"] = hdl

        kit.pool.claim({}, cb)
        await settle(loop)
        left = [x for x in conn.listeners("error") if x in box["mine"]]
        out.append([leave, len(box["mine"]), box["state"], len(left),
                    box["hdl"].get_state_history()])
        await kit.stop()
    return out


# -- entry table ------------------------------------------------------------------

async def sc_subclass_overrides_released(loop):
    ran = []

    class MyHandle(ClaimHandle):
        def state_released(self, S):
            ran.append(self.get_state())
            super().state_released(S)

    saved = mod_pool.ClaimHandle
    mod_pool.ClaimHandle = MyHandle
    try:
        kit = await Kit(loop).up()
        idle = kit.conns[0].listener_count("error")
        # with options the call goes through the Python claim(), which
        # builds the handle from the class the module names
        box = await kit.claim({"timeout": 1000})
        out = {"cls": type(box["hdl"]).__name__}
        box["hdl"].release()
        await settle(loop)
        out["ran"] = ran
        out["history"] = box["hdl"].get_state_history()
        out["errors"] = kit.conns[0].listener_count("error") - idle
        await kit.stop()
        return out
    finally:
        mod_pool.ClaimHandle = saved


_MISSING = object()


async def sc_class_entry_assigned(loop):
    """ClaimHandle.state_claimed assigned after 10 claims, and put back.
    (The pure-Python runtime resolves a class's entries once and keeps
    them, so this is about the native core.)"""
    kit = await Kit(loop).up()
    idle = kit.conns[0].listener_count("error")
    await kit.cycles(10)
    ran = []
    saved = ClaimHandle.__dict__.get("state_claimed", _MISSING)
    orig = ClaimHandle.state_claimed

    def mine(self, S):
        ran.append([self.get_state(), S is not None])
        orig(self, S)

    out = {}
    ClaimHandle.state_claimed = mine
    try:
        box = await kit.claim()
        out["ran"] = list(ran)
        out["claimed"] = [box["err"] is None, box["hdl"].get_state(),
                          kit.conns[0].listener_count("error") - idle]
        box["hdl"].release()
        await settle(loop)
        out["released"] = [box["hdl"].get_state(),
                           kit.conns[0].listener_count("error") - idle]
    finally:
        if saved is _MISSING:
            del ClaimHandle.state_claimed
        else:
            ClaimHandle.state_claimed = saved
    await kit.cycles(3)
    out["ran_after"] = len(ran)
    out["claims"] = kit.pool.p_counters["claim"]
    await kit.stop()
    return out


# -- flush batch ------------------------------------------------------------------

def sc_two_loops_alternately():
    """Claims on loop A, then B, then A again, made while neither loop
    runs; each handle's events arrive while its own loop runs."""
    a, b = VirtualLoop(), VirtualLoop()
    try:
        kits = {"a": a.run_until_complete(Kit(a, n=2).up()),
                "b": b.run_until_complete(Kit(b, n=2).up())}
        seen = []

        def claim(name, tag):
            kit = kits[name]

            def cb(err, hdl=None, conn=None):
                hdl.release()

            hdl = kit.pool.claim({}, cb)
            hdl.on("stateChanged", lambda st: seen.append(
                [tag, st, asyncio.get_running_loop() is kit.loop]))

        claim("a", "a1")
        claim("b", "b1")
        claim("a", "a2")
        a.run_until_complete(settle(a))
        mid = len(seen)
        b.run_until_complete(settle(b))
        claim("b", "b2")
        claim("a", "a3")
        b.run_until_complete(settle(b))
        a.run_until_complete(settle(a))
        out = {"mid": sorted(set(t for t, _, _ in seen[:mid])),
               "right_loop": all(ok for _, _, ok in seen),
               "last": {t: [st for tt, st, _ in seen if tt == t][-1]
                        for t in ("a1", "a2", "a3", "b1", "b2")}}
        for name, loop in (("a", a), ("b", b)):
            loop.run_until_complete(kits[name].stop())
        return out
    finally:
        a.close()
        b.close()


async def sc_flush_that_raises(loop):
    """A stateChanged listener that raises ends that flush; the next
    claim's events are delivered as ever."""
    errors = []
    loop.set_exception_handler(
        lambda lp, ctx: errors.append(type(ctx.get("exception")).__name__))
    kit = await Kit(loop).up()

    def bad(st):
        raise KeyError("listener")

    # a handle of no slot, so that only the flush is cut short
    h = bare_handle(FakePool(loop), loop)
    h.on("stateChanged", bad)
    h.cancel()
    await settle(loop)
    out = {"errors": errors[:], "state": h.get_state()}
    seen = []
    box = await kit.claim()
    box["hdl"].on("stateChanged", seen.append)
    box["hdl"].release()
    await settle(loop)
    out["seen"] = seen
    out["errors_after"] = len(errors)
    out["idle"] = kit.pool.get_stats()["idleConnections"]
    await kit.stop()
    return out


SCENARIOS = {
    "error_listener_on_a_kit_slot": sc_error_listener_on_a_kit_slot,
    "error_listener_without_a_kit": sc_error_listener_without_a_kit,
    "remove_listener_overridden": sc_remove_listener_overridden,
    "error_while_claimed": sc_error_while_claimed,
    "leave_from_the_callback": sc_leave_from_the_callback,
    "subclass_overrides_released": sc_subclass_overrides_released,
    "flush_that_raises": sc_flush_that_raises,
}
for _name, (_fn, _) in LEAK_SCENARIOS.items():
    SCENARIOS["leak_" + _name] = _fn


def _run_all():
    res = {name: run_vt(fn) for name, fn in SCENARIOS.items()}
    res["two_loops_alternately"] = sc_two_loops_alternately()
    return res


@pytest.fixture(scope="module")
def here():
    return json.loads(json.dumps(_run_all()))


@pytest.fixture(scope="module")
def pure():
    """Every scenario on the pure-Python runtime, in one child process."""
    env = dict(os.environ, CUEBALL_PURE="1")
    out = subprocess.run(
        [sys.executable, os.path.abspath(__file__), "--scenarios"],
        env=env, stdout=subprocess.PIPE, check=True, timeout=120)
    res = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert res.pop("native") is False
    return res


@pytest.mark.parametrize(
    "name", sorted(SCENARIOS) + ["two_loops_alternately"])
def test_same_on_both_runtimes(name, here, pure):
    assert here[name] == pure[name]


@pytest.mark.parametrize("name", sorted(LEAK_SCENARIOS))
def test_leak_detector(name, here):
    assert here["leak_" + name] == LEAK_SCENARIOS[name][1]


@native_only
def test_a_connection_that_is_no_native_emitter_counts_nothing():
    async def body(loop):
        with logged() as log:
            fake = FakePool(loop)
            conn = PurePythonEventEmitter()
            h = bare_handle(fake, loop)
            h.try_(StandingSlot())
            h.accept(conn)
            assert conn.listener_count("error") == 1
            conn.on("data", _noop)
            conn.on("close", _noop)
            h.release()
            await settle(loop)
            assert h.is_in_state("released")
            assert conn.listener_count("error") == 0
            assert cycle_state(conn)["leak_cache"] is None
        assert log.leaks() == []
    run_vt(body)


@native_only
def test_the_leak_cache_survives_claims_that_change_nothing():
    async def body(loop):
        kit = await Kit(loop).up()
        conn = kit.conns[0]
        conn.on("data", _noop)
        assert cycle_state(conn)["leak_cache"] is None
        await kit.cycle()
        assert cycle_state(conn)["leak_cache"] == (1, 0, 0, 1)
        lists = dict(conn._events)
        refs = {k: sys.getrefcount(v) for k, v in lists.items()}
        await kit.cycle()
        await kit.cycles(5)
        assert cycle_state(conn)["leak_cache"] == (1, 0, 0, 1)
        # the same lists, referenced as often as before
        assert all(conn._events[k] is v for k, v in lists.items())
        assert {k: sys.getrefcount(v) for k, v in lists.items()} == refs
        # a listener through the emitter invalidates it, the next claim
        # fills it again
        ls = conn.on("close", _noop)
        assert cycle_state(conn)["leak_cache"] is None
        await kit.cycle()
        assert cycle_state(conn)["leak_cache"] == (2, 0, 0, 1)
        conn.remove_listener("close", ls)
        # behind the emitter's back the accessor cannot know: the next
        # claim finds out (test_leak_detector), and counts afresh
        conn._events["readable"] = [_noop]
        await kit.cycle()
        assert cycle_state(conn)["leak_cache"] == (1, 0, 1, 1)
        await kit.stop()
    run_vt(body)


@native_only
def test_the_cached_lists_are_the_collectors_business():
    """A connection in a cycle through one of its listener lists is
    freed although the cache refers to the list."""
    async def body(loop):
        fake = FakePool(loop)
        conn = DummyConnection({})
        conn.on("data", lambda *a, c=conn: c)       # conn -> list -> conn
        h = bare_handle(fake, loop)
        h.try_(StandingSlot())
        h.accept(conn)
        h.release()
        await settle(loop)
        assert cycle_state(conn)["leak_cache"] == (0, 0, 0, 1)
        gone = weakref.ref(conn)
        del conn, h
        gc.collect()
        assert gone() is None
    run_vt(body)


def test_error_listener_while_claimed_and_not_after(here):
    k = here["error_listener_on_a_kit_slot"]
    assert k == {"idle": 0, "claimed": [1, [True]], "released": 0,
                 "claimed_again": 1, "closed": [0, "closed"]}
    b = here["error_listener_without_a_kit"]
    assert b == [0, [1, [True]], [0, "released"],
                 0, [1, [True]], [0, "closed"]]
    assert here["remove_listener_overridden"] == [
        [0, 1], [1, 1], [2, 1], [3, 0]]
    assert here["leave_from_the_callback"] == [
        ["release", 1, "claimed", 0,
         ["waiting", "claiming", "claimed", "released"]],
        ["close", 1, "claimed", 0,
         ["waiting", "claiming", "claimed", "closed"]]]


def test_error_emitted_while_claimed(here):
    e = here["error_while_claimed"]
    assert e["with"] == [["with"], ["error-while-claimed"], "claimed"]
    assert e["without"] == ["RuntimeError", "without"]
    assert e["state"] == "claimed" and e["listeners"] == 1
    assert e["after"] == 0 and e["emit_after"] is False
    assert e["log"] == ["connection emitted error while claimed"]


@native_only
def test_the_kit_registers_its_one_callback_every_time():
    async def body(loop):
        kit = await Kit(loop).up()
        conn = kit.conns[0]
        box = await kit.claim()
        (first,) = [cb for cb in conn.listeners("error")
                    if type(cb).__name__ == "_SlotKitCb"]
        box["hdl"].release()
        await settle(loop)
        refs = sys.getrefcount(first)
        box = await kit.claim()
        assert [cb for cb in conn.listeners("error") if cb is first]
        second = conn.listeners("error")[-1]
        assert second is first
        del second
        # the list and the handle refer to it while claimed
        assert sys.getrefcount(first) == refs + 2
        box["hdl"].release()
        await settle(loop)
        assert sys.getrefcount(first) == refs
        await kit.stop()
    run_vt(body)


def test_entry_overridden_in_a_subclass(here):
    s = here["subclass_overrides_released"]
    assert s == {"cls": "MyHandle", "ran": ["released"], "errors": 0,
                 "history": ["waiting", "claiming", "claimed", "released"]}


@native_only
def test_entry_assigned_on_the_class_and_put_back():
    c = run_vt(sc_class_entry_assigned)
    assert c["ran"] == [["claimed", True]]
    assert c["claimed"] == [True, "claimed", 1]
    assert c["released"] == ["released", 0]
    assert c["ran_after"] == 1 and c["claims"] == 14


@native_only
def test_an_entry_set_on_one_instance_is_that_instances_only():
    async def body(loop):
        kit = await Kit(loop).up()
        await kit.cycles(3)
        idle = kit.conns[0].listener_count("error")
        ran = []
        box = await kit.claim()
        hdl = box["hdl"]

        def mine(S):
            ran.append(hdl.get_state())
            type(hdl).state_released(hdl, S)

        hdl.state_released = mine
        hdl.release()
        await settle(loop)
        assert ran == ["released"] and hdl.is_in_state("released")
        assert kit.conns[0].listener_count("error") == idle
        await kit.cycles(3)
        assert ran == ["released"]
        await kit.stop()
    run_vt(body)


def test_two_loops_used_alternately(here):
    t = here["two_loops_alternately"]
    assert t["right_loop"] is True
    # while only loop A ran, only A's handles heard anything
    assert t["mid"] == ["a1", "a2"]
    assert t["last"] == {k: "released"
                         for k in ("a1", "a2", "a3", "b1", "b2")}


def test_after_a_flush_that_raises_the_next_claim_flushes(here):
    f = here["flush_that_raises"]
    assert f["errors"] == ["KeyError"] and f["state"] == "cancelled"
    assert f["seen"] == ["released"]
    assert f["errors_after"] == 1 and f["idle"] == 1


# -- handles -----------------------------------------------------------------------

@native_only
def test_a_handle_the_user_keeps_is_not_handed_out_again():
    async def body(loop):
        kit = await Kit(loop).up()
        box = await kit.cycle()
        kept = box["hdl"]
        history = kept.get_state_history()
        later = []
        for _ in range(6):
            later.append((await kit.cycle())["hdl"])
            assert later[-1] is not kept
        assert len(set(map(id, later + [kept]))) == 7
        assert kept.is_in_state("released")
        assert kept.get_state_history() == history
        assert kept.ch_connection is kit.conns[0]
        await kit.stop()
    run_vt(body)


@native_only
def test_a_weak_reference_to_a_released_handle_dies():
    async def body(loop):
        kit = await Kit(loop).up()
        box = await kit.cycle()
        ref = weakref.ref(box["hdl"])
        box.clear()                 # or handle, callback and box are a cycle
        del box
        # the slot remembers the last handle it served, no other
        await kit.cycles(2)
        assert ref() is None
        await kit.stop()
    run_vt(body)


# -- resource hygiene ---------------------------------------------------------------

@native_only
def test_5000_cycles_leave_nothing_behind():
    states = [sys.intern(s) for s in [
        "idle", "busy", "waiting", "claiming", "claimed", "released",
        "stateChanged", "error"]]

    async def body(loop):
        kit = await Kit(loop, n=2).up()
        pool = kit.pool
        for c in kit.conns:
            c.on("data", _noop)
        await kit.cycles(200)                       # warm every lazy path
        box = await kit.claim()
        (kit_cb,) = [cb for cb in box["conn"].listeners("error")
                     if type(cb).__name__ == "_SlotKitCb"]
        box["hdl"].release()
        await settle(loop)
        box.clear()                 # or handle, callback and box are a cycle
        del box
        lists = [ls for c in kit.conns for ls in c._events.values()]
        watched = [None, True] + states + lists + [kit_cb]
        gc.collect()
        gc.disable()
        try:
            objs0 = len(gc.get_objects())
            refs0 = [sys.getrefcount(o) for o in watched]
            await kit.cycles(5000)
            refs1 = [sys.getrefcount(o) for o in watched]
            objs1 = len(gc.get_objects())
            unreachable = gc.collect()
        finally:
            gc.enable()
        assert unreachable == 0
        assert abs(objs1 - objs0) <= 20, (objs0, objs1)
        drift = [b - a for a, b in zip(refs0, refs1)]
        k = 2 + len(states)
        assert all(abs(d) <= 20 for d in drift[:k]), drift
        # the listener lists and the kit's callback: exactly as before
        assert drift[k:] == [0] * (len(lists) + 1), drift
        assert pool.get_stats()["counters"]["claim"] == 5201
        await kit.stop()
    run_vt(body)


if __name__ == "__main__":
    if sys.argv[1:] == ["--scenarios"]:
        res = _run_all()
        res["native"] = mod_fsm.NATIVE
        print(json.dumps(res))
