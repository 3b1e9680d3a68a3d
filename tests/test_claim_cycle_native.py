"""The claim/release cycle after its interpreter round-trips were cut:
what a claimer, a listener and the leak detector observe is what it was.

Every pool here has 1 backend, spares 1 and maximum 1, on the virtual
clock, so successive claims get the same connection.  The scenarios run
on whichever runtime the process selected; the leak-detector ones are
also replayed in a child process on the pure-Python runtime and the two
logs compared.
"""

import asyncio
import gc
import json
import logging
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from cueball_amd import events as mod_events  # noqa: E402
from cueball_amd import fsm as mod_fsm  # noqa: E402
from cueball_amd import utils as mod_utils  # noqa: E402
from cueball_amd.errors import CueballError  # noqa: E402
from cueball_amd.events import EventEmitter  # noqa: E402
from cueball_amd.fsm import FSM  # noqa: E402
from cueball_amd.pool import ConnectionPool  # noqa: E402
from cueball_amd.resolver import ResolverFSM  # noqa: E402
from cueball_amd.testing import (DummyConnection, DummyResolver,  # noqa: E402
                                 VirtualLoop, advance, settle)

RECOVERY = {"default": {"timeout": 500, "retries": 1, "delay": 0}}


def run_vt(body):
    loop = VirtualLoop()
    try:
        return loop.run_until_complete(body(loop))
    finally:
        loop.close()


class Kit:
    """A 1/1/1 pool whose one connection is connected."""

    def __init__(self, loop):
        self.loop = loop
        self.conns = []
        self.resolver = DummyResolver()
        self.rfsm = ResolverFSM(self.resolver, {"loop": loop})

        def constructor(backend):
            c = DummyConnection(backend)
            self.conns.append(c)
            return c

        self.pool = ConnectionPool({
            "domain": "cycle.test", "constructor": constructor,
            "recovery": RECOVERY, "spares": 1, "maximum": 1,
            "resolver": self.rfsm, "loop": loop})
        self.rfsm.start()

    async def up(self):
        self.resolver.add("b1", {})
        await settle(self.loop)
        for c in list(self.conns):
            c.connect()
        await settle(self.loop)
        assert self.pool.get_stats()["idleConnections"] == 1
        return self

    def slot(self):
        (slot,) = self.pool.p_connections["b1"]
        return slot

    async def claim(self):
        box = {}

        def cb(err, hdl=None, conn=None):
            box.update(err=err, hdl=hdl, conn=conn)

        box["ret"] = self.pool.claim({}, cb)
        await settle(self.loop)
        return box

    async def cycle(self, during=None, disable_check=False):
        """One claim and release; `during(conn)` runs while claimed."""
        box = await self.claim()
        assert box["err"] is None
        assert box["conn"] is self.conns[0]
        if during is not None:
            during(box["conn"])
        if disable_check:
            box["hdl"].disable_release_leak_check()
        box["hdl"].release()
        await settle(self.loop)
        return box

    async def stop(self):
        self.pool.stop()
        await settle(self.loop)
        if not self.pool.is_in_state("stopped"):
            # a replacement connection that never connected: let its
            # timers run out
            await advance(self.loop, 10.0)
        assert self.pool.is_in_state("stopped")


class _ListHandler(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


#: the two runtimes word the warning differently, and did before: the
#: native core puts the numbers into the text, the pure-Python handle
#: passes them as log fields.  Both are read back as [event, before,
#: after].
_LEAK_RE = re.compile(
    r"leaked event handlers"
    r"(?: \(event=(\w+) before=(\d+) after=(\d+)\)"
    r"| \[.*\bevent=(\w+), count_before_claim=(\d+), "
    r"count_after_release=(\d+))")


def _leak_log(scenario, raw=False):
    """Run one scenario coroutine function on a fresh kit and return the
    leak warnings it logged as [event, before, after] lists (or, with
    `raw`, their text with the log fields stripped)."""
    handler = _ListHandler()
    logger = logging.getLogger("cueball")
    logger.addHandler(handler)
    try:
        async def body(loop):
            kit = await Kit(loop).up()
            await scenario(kit)
            await kit.stop()
        run_vt(body)
    finally:
        logger.removeHandler(handler)
    msgs = [m for m in handler.messages if "leaked" in m]
    if raw:
        return [m.split(" [")[0] for m in msgs]
    out = []
    for m in msgs:
        g = _LEAK_RE.search(m)
        assert g is not None, m
        ev, before, after = [x for x in g.groups() if x is not None]
        out.append([ev, int(before), int(after)])
    return out


def _noop(*a):
    pass


# -- the leak-detector scenarios: at least 4 claims of one connection ----

async def leak_nothing_added(kit):
    for _ in range(5):
        await kit.cycle()


async def leak_added_and_left(kit):
    await kit.cycle()
    await kit.cycle(lambda conn: conn.on("data", _noop))
    for _ in range(3):
        await kit.cycle()


async def leak_added_and_removed(kit):
    def during(conn):
        ls = conn.on("data", _noop)
        conn.remove_listener("data", ls)
    for _ in range(5):
        await kit.cycle(during)


async def leak_swapped(kit):
    fns = [lambda *a: None for _ in range(6)]
    kit.conns[0].on("data", fns[0])        # while idle: not a leak
    state = {"i": 0}

    def during(conn):
        i = state["i"]
        conn.remove_listener("data", fns[i])
        conn.on("data", fns[i + 1])
        state["i"] = i + 1
    for _ in range(5):
        await kit.cycle(during)
    assert kit.conns[0].listeners("data") == [fns[5]]


async def leak_added_while_idle(kit):
    await kit.cycle()
    await kit.cycle()
    kit.conns[0].on("data", _noop)          # between claims
    await kit.cycle()
    kit.conns[0].on("close", _noop)
    await kit.cycle()
    await kit.cycle()


async def leak_internal_marker(kit):
    def internal(*a):
        pass
    internal._cueball_internal = True

    await kit.cycle()
    await kit.cycle(lambda conn: conn.on("data", internal))
    for _ in range(3):
        await kit.cycle()


async def leak_check_disabled(kit):
    await kit.cycle()
    # left behind with the check off: nothing said
    await kit.cycle(lambda conn: conn.on("data", _noop), disable_check=True)
    await kit.cycle()
    # the next leak is still seen, on top of the one that stayed
    await kit.cycle(lambda conn: conn.on("data", lambda *a: None))
    await kit.cycle()


LEAK_SCENARIOS = {
    "nothing_added": (leak_nothing_added, []),
    "added_and_left": (leak_added_and_left, [["data", 0, 1]]),
    "added_and_removed": (leak_added_and_removed, []),
    "swapped": (leak_swapped, []),
    "added_while_idle": (leak_added_while_idle, []),
    "internal_marker": (leak_internal_marker, []),
    "check_disabled": (leak_check_disabled, [["data", 1, 2]]),
}


@pytest.mark.parametrize("name", sorted(LEAK_SCENARIOS))
def test_leak_detector(name):
    scenario, expected = LEAK_SCENARIOS[name]
    assert _leak_log(scenario) == expected


@pytest.mark.skipif(not mod_fsm.NATIVE, reason="the native core's wording")
def test_leak_warning_text_of_the_native_core():
    assert _leak_log(leak_added_and_left, raw=True) == [
        "connection claimer looks like it leaked event handlers "
        "(event=data before=0 after=1)"]


def _all_leak_logs():
    return {name: _leak_log(fn) for name, (fn, _) in LEAK_SCENARIOS.items()}


def test_leak_detector_same_log_on_both_runtimes():
    """The pure-Python runtime, in a child process of its own, logs what
    this process logs, scenario by scenario."""
    env = dict(os.environ, CUEBALL_PURE="1")
    out = subprocess.run(
        [sys.executable, os.path.abspath(__file__), "--leak-logs"],
        env=env, stdout=subprocess.PIPE, check=True, timeout=120)
    pure = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert pure.pop("native") is False
    assert pure == _all_leak_logs()


# -- scoped registration and listener order --------------------------------

class _Hopper(FSM):
    """a -> b -> a ...; state a listens on `other` through its scope."""

    def __init__(self, other, loop):
        self.other = other
        self.seen = []
        super().__init__("a", loop=loop)

    def state_a(self, S):
        S.on(self.other, "evt", self.seen.append)

    def state_b(self, S):
        pass


def test_scoped_listener_removed_leaves_no_event_name():
    async def body(loop):
        other = EventEmitter()
        hop = _Hopper(other, loop)
        assert other.event_names() == ["evt"]
        assert other.listener_count("evt") == 1
        hop.goto_state("b")
        assert other.event_names() == []
        assert other.listener_count("evt") == 0
        assert other.listeners("evt") == []
        assert other.emit("evt", 1) is False
        hop.goto_state("a")
        assert other.event_names() == ["evt"]
        assert other.emit("evt", 2) is True
        assert hop.seen == [2]
        # more registrations than a scope holds inline
        many = [EventEmitter() for _ in range(7)]

        class Wide(FSM):
            def state_on(self, S):
                for m in many:
                    S.on(m, "x", _noop)

            def state_off(self, S):
                pass

        wide = Wide("on", loop=loop)
        assert [m.listener_count("x") for m in many] == [1] * 7
        wide.goto_state("off")
        assert [m.listener_count("x") for m in many] == [0] * 7
        assert [m.event_names() for m in many] == [[]] * 7
        await settle(loop)
    run_vt(body)


def test_double_registration_removed_once_keeps_same_survivor():
    def f(*a):
        pass

    def g(*a):
        pass

    got = []
    for cls in (EventEmitter, mod_events.PurePythonEventEmitter):
        em = cls()
        em.on("x", f)
        em.on("x", g)
        em.on("x", f)
        em.remove_listener("x", f)
        got.append(em.listeners("x"))
        em.remove_listener("x", f)
        em.remove_listener("x", g)
        assert em.listeners("x") == [] and em.event_names() == []
        assert em.listener_count("x") == 0
    assert got[0] == got[1] == [g, f]


def test_listener_order_across_busy_idle_cycles():
    async def body(loop):
        kit = await Kit(loop).up()
        slot = kit.slot()
        seen = []

        def first(st):
            # the pool's own dispatcher was registered before us: by now
            # an idle slot is back on the idle queue
            seen.append(("first", st, slot.p_idleq_node is not None))

        def second(st):
            seen.append(("second", st))

        slot.on("stateChanged", first)
        slot.on("stateChanged", second)
        before = slot.listeners("stateChanged")
        assert before[-2:] == [first, second] and len(before) == 3
        for _ in range(3):
            await kit.cycle()
            assert slot.listeners("stateChanged") == before
        assert seen == [("first", "busy", False), ("second", "busy"),
                        ("first", "idle", True), ("second", "idle")] * 3
        assert slot.event_names() == ["stateChanged", "unwanted"] or \
            sorted(slot.event_names()) == ["stateChanged", "unwanted"]
        await kit.stop()
    run_vt(body)


# -- fields that C keeps, written and read from Python ----------------------

def test_csf_wanted_written_from_python_is_seen():
    async def body(loop):
        kit = await Kit(loop).up()
        slot = kit.slot()
        assert slot.csf_wanted is True and slot.csf_handle is None
        box = await kit.claim()
        assert slot.csf_handle is box["hdl"]
        assert slot.is_in_state("busy")
        slot.csf_wanted = 0            # any falsy value
        box["hdl"].release()
        await settle(loop)
        # an unwanted slot does not go back to idle on release
        assert slot.get_state() in ("stopping", "stopped")
        assert slot.csf_prev_handle is None or \
            slot.csf_prev_handle is box["hdl"]
        await kit.stop()

        kit = await Kit(loop).up()
        slot = kit.slot()
        await kit.cycle()
        assert slot.is_in_state("idle")
        slot.set_unwanted()
        assert slot.csf_wanted is False
        await settle(loop)
        assert slot.get_state() in ("stopping", "stopped")
        await kit.stop()
    run_vt(body)


def test_demand_marks_and_waiter_node_after_a_queued_claim():
    async def body(loop):
        kit = await Kit(loop).up()
        pool = kit.pool
        first = await kit.claim()
        assert first["err"] is None
        second = await kit.claim()          # queues: the pool is 1/1/1
        assert "err" not in second
        h2 = second["ret"]
        assert len(pool.p_waiters) == 1
        assert h2.ch_waiter_node is not None and h2.ch_waiter_node.linked
        # what _note_demand computes for 1 connection, none spare, one
        # waiter: busy 1, demand 1 + 1
        assert pool.p_total_conns == 1
        assert pool.p_busy_hwm == 1
        assert pool.p_demand_hwm == 2
        marks = (pool.p_total_conns, pool.p_busy_hwm, pool.p_demand_hwm)
        pool._note_demand()
        assert (pool.p_total_conns, pool.p_busy_hwm,
                pool.p_demand_hwm) == marks
        # python writes are what the next reading starts from
        pool.p_busy_hwm = 0
        pool.p_demand_hwm = 0
        third = await kit.claim()
        assert (pool.p_busy_hwm, pool.p_demand_hwm) == (1, 3)
        third["ret"].cancel()

        h2.cancel()
        assert len(pool.p_waiters) == 0
        assert h2.ch_waiter_node is None
        assert h2.is_in_state("cancelled")
        first["hdl"].release()
        await settle(loop)
        assert "err" not in second
        await kit.stop()
    run_vt(body)


# -- stack traces switched after import -------------------------------------

def test_stack_traces_toggle_after_import():
    async def body(loop):
        kit = await Kit(loop).up()

        def my_releaser(hdl):
            hdl.release()

        async def my_claimer():
            return await kit.claim()

        placeholder = mod_utils.maybe_capture_stack_trace()
        assert not mod_utils.stack_traces_enabled()
        box = await my_claimer()
        assert box["hdl"].ch_claim_stack == placeholder
        my_releaser(box["hdl"])
        assert box["hdl"].ch_release_stack == placeholder
        await settle(loop)

        mod_utils.enable_stack_traces()
        try:
            box = await my_claimer()
            stack = box["hdl"].ch_claim_stack
            assert stack != placeholder
            assert any("my_claimer" in fr for fr in stack)
            assert all(isinstance(fr, str) for fr in stack)
            my_releaser(box["hdl"])
            assert any("my_releaser" in fr
                       for fr in box["hdl"].ch_release_stack)
            with pytest.raises(CueballError) as ei:
                box["hdl"].release()
            assert "released by my_releaser" in str(ei.value)
            await settle(loop)
        finally:
            mod_utils.disable_stack_traces()

        box = await my_claimer()
        assert box["hdl"].ch_claim_stack == placeholder
        my_releaser(box["hdl"])
        assert box["hdl"].ch_release_stack == placeholder
        with pytest.raises(CueballError) as ei:
            box["hdl"].release()
        assert "stack traces disabled" in str(ei.value)
        await settle(loop)
        await kit.stop()
    run_vt(body)


# -- state history ----------------------------------------------------------

def test_state_history_after_3_and_20_transitions():
    async def body(loop):
        hop = _Hopper(EventEmitter(), loop)      # transition 1: a
        assert hop.get_state_history() == ["a"]
        hop.goto_state("b")
        hop.goto_state("a")
        assert hop.get_state_history() == ["a", "b", "a"]
        h = hop.get_state_history()
        h.append("x")                            # a copy, not the record
        assert hop.get_state_history() == ["a", "b", "a"]
        for i in range(17):                      # 20 in all, ends on b
            hop.goto_state("b" if i % 2 == 0 else "a")
        assert hop.get_state() == "b"
        assert hop.get_state_history() == ["a", "b"] * 4
        hop.goto_state("a")
        assert hop.get_state_history() == ["b", "a"] * 4
        # stateChanged still delivers every state, in order
        seen = []
        hop.on("stateChanged", seen.append)
        await settle(loop)
        assert seen == (["a", "b"] * 11)[:21]
    run_vt(body)


def test_state_changed_reaches_listener_added_before_the_flush():
    async def body(loop):
        hop = _Hopper(EventEmitter(), loop)
        hop.goto_state("b")
        seen = []
        hop.on("stateChanged", seen.append)      # after the transitions
        await settle(loop)
        assert seen == ["a", "b"]
        # a listener that causes more transitions than the inline queue
        # holds, while the flush is running
        burst = []

        def on_change(st):
            burst.append(st)
            if len(burst) == 1:
                for i in range(9):
                    hop.goto_state("a" if i % 2 == 0 else "b")

        hop.remove_listener("stateChanged", seen.append)
        hop.on("stateChanged", on_change)
        hop.goto_state("b") if hop.get_state() == "a" else None
        hop.goto_state("a")
        await settle(loop)
        assert burst[0] == "a"
        assert burst[1:] == ["a", "b", "a", "b", "a", "b", "a", "b", "a"]
    run_vt(body)


# -- resource hygiene -------------------------------------------------------

def test_5000_cycles_leave_nothing_behind():
    states = ["idle", "busy", "waiting", "claiming", "claimed", "released",
              "stateChanged", "connected"]
    states = [sys.intern(s) for s in states]

    async def body(loop):
        kit = await Kit(loop).up()
        pool = kit.pool
        left = {"n": 0}
        done = loop.create_future()

        def cb(err, hdl=None, conn=None):
            assert err is None
            hdl.release()
            left["n"] -= 1
            if left["n"] > 0:
                pool.claim({}, cb)
            else:
                done.set_result(None)

        async def burst(n):
            nonlocal done
            done = loop.create_future()
            left["n"] = n
            pool.claim({}, cb)
            while not done.done():
                await asyncio.sleep(0)
            await settle(loop)

        await burst(200)                        # warm every lazy path
        gc.collect()
        gc.disable()
        try:
            objs0 = len(gc.get_objects())
            refs0 = [sys.getrefcount(o) for o in [None, True] + states]
            await burst(5000)
            refs1 = [sys.getrefcount(o) for o in [None, True] + states]
            objs1 = len(gc.get_objects())
            unreachable = gc.collect()
        finally:
            gc.enable()
        assert unreachable == 0
        assert abs(objs1 - objs0) <= 20, (objs0, objs1)
        drift = [b - a for a, b in zip(refs0, refs1)]
        assert all(abs(d) <= 20 for d in drift), drift
        assert pool.get_stats()["counters"]["claim"] >= 5200
        await kit.stop()
    run_vt(body)


if __name__ == "__main__":
    if sys.argv[1:] == ["--leak-logs"]:
        logs = _all_leak_logs()
        logs["native"] = mod_fsm.NATIVE
        print(json.dumps(logs))
