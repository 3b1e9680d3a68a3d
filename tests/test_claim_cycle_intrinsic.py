"""The claim cycle with the library's own listeners as intrinsic hooks of
the native core: what a claimer and a listener observe is what the
pure-Python runtime shows them.

Every pool here has 1 backend (the exhausted-pool scenario: 1 connection
and 2 claimers) on the virtual clock.  The scenarios return plain data;
they run on the runtime this process selected and are replayed once, all
together, in a child process on the pure-Python runtime, and the results
are compared.
"""

import asyncio
import gc
import inspect
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from cueball_amd import fsm as mod_fsm  # noqa: E402
from cueball_amd.errors import (ClaimTimeoutError,  # noqa: E402
                                PoolFailedError, PoolStoppingError)
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
    """A pool of one backend whose one connection is connected."""

    def __init__(self, loop, **options):
        self.loop = loop
        self.conns = []
        self.resolver = DummyResolver()
        self.rfsm = ResolverFSM(self.resolver, {"loop": loop})

        def constructor(backend):
            c = DummyConnection(backend)
            self.conns.append(c)
            return c

        opts = {"domain": "hooks.test", "constructor": constructor,
                "recovery": RECOVERY, "spares": 1, "maximum": 1,
                "resolver": self.rfsm, "loop": loop}
        opts.update(options)
        self.pool = ConnectionPool(opts)
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

    def claim_box(self):
        """A recording claim callback, as box["cb"]."""
        box = {}

        def cb(err, hdl=None, conn=None):
            box.update(err=err, hdl=hdl, conn=conn)

        box["cb"] = cb
        return box

    async def claim(self):
        box = self.claim_box()
        box["ret"] = self.pool.claim({}, box["cb"])
        await settle(self.loop)
        return box

    async def stop(self):
        self.pool.stop()
        await settle(self.loop)
        if not self.pool.is_in_state("stopped"):
            await advance(self.loop, 10.0)
        assert self.pool.is_in_state("stopped")


def _tail(fsm, n):
    return fsm.get_state_history()[-n:]


# -- 1, 2: the order of events on the handle --------------------------------

async def _event_order(loop, remove_a):
    kit = await Kit(loop).up()
    slot = kit.slot()
    rec = []

    def mk(name):
        def listener(st):
            rec.append([name, st, slot.get_state()])
        return listener

    a, b, c = mk("A"), mk("B"), mk("C")
    box = {}

    def cb(err, hdl=None, conn=None):
        assert err is None
        box["hdl"] = hdl
        hdl.on("stateChanged", b)           # inside the claim callback

    hdl = kit.pool.claim({}, cb)
    hdl.on("stateChanged", a)               # right after claim() returns
    await settle(loop)
    assert box["hdl"] is hdl
    hdl.on("stateChanged", c)               # after the callback returned
    if remove_a:
        hdl.remove_listener("stateChanged", a)
    hdl.release()
    await settle(loop)
    await kit.stop()
    return rec


async def sc_event_order(loop):
    return await _event_order(loop, False)


async def sc_event_order_a_removed(loop):
    return await _event_order(loop, True)


async def sc_once_listener(loop):
    kit = await Kit(loop).up()
    slot = kit.slot()
    rec = []
    box = await kit.claim()
    hdl = box["hdl"]
    hdl.once("stateChanged",
             lambda st: rec.append(["once", st, slot.get_state()]))
    hdl.on("stateChanged",
           lambda st: rec.append(["on", st, slot.get_state()]))
    hdl.release()
    await settle(loop)
    rec.append(len(hdl.listeners("stateChanged")))
    await kit.stop()
    return rec


# -- 3: cold exits from the fast lane, one cycle each -----------------------

async def _smgr_dies(loop, how, busy):
    kit = await Kit(loop).up()
    slot = kit.slot()
    conn = kit.conns[0]
    out = {}
    if busy:
        box = await kit.claim()
        # a claimed connection without an 'error' listener raises
        conn.on("error", lambda e: None)
    if how == "error":
        conn.emit("error", RuntimeError("boom"))
    else:
        conn.emit("close")
    await settle(loop)
    out["slot_then"] = _tail(slot, 4)
    if busy:
        out["handle_then"] = _tail(box["hdl"], 4)
        box["hdl"].release()
        await settle(loop)
        out["handle"] = _tail(box["hdl"], 4)
    out["slot"] = _tail(slot, 5)
    await kit.stop()
    return out


async def sc_smgr_error_idle(loop):
    return await _smgr_dies(loop, "error", False)


async def sc_smgr_closed_idle(loop):
    return await _smgr_dies(loop, "closed", False)


async def sc_smgr_error_busy(loop):
    return await _smgr_dies(loop, "error", True)


async def sc_smgr_closed_busy(loop):
    return await _smgr_dies(loop, "closed", True)


async def sc_unwanted_idle(loop):
    kit = await Kit(loop).up()
    slot = kit.slot()
    box = await kit.claim()
    box["hdl"].release()
    await settle(loop)
    names = sorted(slot.event_names())
    slot.set_unwanted()
    await settle(loop)
    out = {"names": names, "slot": _tail(slot, 4),
           "seen_unwanted": kit.conns[0].seen_unwanted}
    await kit.stop()
    return out


async def sc_handle_close(loop):
    kit = await Kit(loop).up()
    slot = kit.slot()
    box = await kit.claim()
    box["hdl"].close()
    await settle(loop)
    out = {"handle": _tail(box["hdl"], 4), "slot": _tail(slot, 4)}
    await kit.stop()
    return out


async def sc_cancel_while_waiting(loop):
    kit = await Kit(loop).up()
    pool = kit.pool
    first = await kit.claim()
    second = await kit.claim()              # 2 claimers, 1 connection
    h2 = second["ret"]
    out = {"queued": len(pool.p_waiters),
           "linked": h2.ch_waiter_node is not None and
           h2.ch_waiter_node.linked}
    h2.cancel()
    out["after"] = len(pool.p_waiters)
    out["node_gone"] = h2.ch_waiter_node is None
    await settle(loop)
    first["hdl"].release()
    await settle(loop)
    out["called"] = "err" in second
    out["h2"] = _tail(h2, 3)
    out["h1"] = _tail(first["hdl"], 4)
    out["slot"] = _tail(kit.slot(), 3)
    await kit.stop()
    return out


async def sc_claim_timeout(loop):
    kit = await Kit(loop).up()
    pool = kit.pool
    first = await kit.claim()
    box = kit.claim_box()
    h2 = pool.claim({"timeout": 100}, box["cb"])
    await settle(loop)
    out = {"queued": len(pool.p_waiters)}
    await advance(loop, 0.2)
    out["err"] = type(box.get("err")).__name__
    out["after"] = len(pool.p_waiters)
    out["h2"] = _tail(h2, 3)
    first["hdl"].release()
    await settle(loop)
    out["slot"] = _tail(kit.slot(), 3)
    await kit.stop()
    return out


async def sc_lost_race_at_busy(loop):
    """The claim's flush is queued before the socket manager's: the
    ticket still finds the slot idle, and the busy entry finds the
    socket manager no longer connected."""
    kit = await Kit(loop).up()
    slot = kit.slot()
    box = kit.claim_box()
    hdl = kit.pool.claim({}, box["cb"])
    kit.conns[0].emit("close")
    await settle(loop)
    out = {"called": "err" in box, "handle": _tail(hdl, 4),
           "slot": _tail(slot, 4), "slot_handle": slot.csf_handle is None}
    hdl.cancel()
    await settle(loop)
    out["handle_end"] = _tail(hdl, 2)
    await kit.stop()
    return out


# -- 4: a handler for a state the slot has left in the same cascade ---------

async def sc_stale_slot_hook(loop):
    """A listener that ran before the slot's own reaction to `released`
    has already moved the slot on: the slot's reaction is obsolete."""
    kit = await Kit(loop).up()
    slot = kit.slot()
    hdl = kit.pool.claim({}, lambda *a: None)

    def mover(st):
        if st == "released":
            slot.goto_state("stopping")

    hdl.on("stateChanged", mover)           # before the slot goes busy
    await settle(loop)
    hdl.release()
    await settle(loop)
    out = {"slot": _tail(slot, 4), "handle": _tail(hdl, 2)}
    await kit.stop()
    return out


async def sc_stale_smgr_hook(loop):
    """A listener on the socket manager, there since before the slot went
    idle, makes the slot unwanted when the socket closes: the slot is
    gone from idle when its own reaction to `closed` is due."""
    kit = await Kit(loop).up()
    slot = kit.slot()

    def on_smgr(st):
        if st == "closed":
            slot.set_unwanted()

    slot.get_socket_mgr().on("stateChanged", on_smgr)
    box = await kit.claim()
    box["hdl"].release()
    await settle(loop)
    kit.conns[0].emit("close")
    await settle(loop)
    out = {"slot": _tail(slot, 4)}
    await kit.stop()
    return out


# -- 5: the tracer ----------------------------------------------------------

async def sc_tracer_mid_run(loop):
    kit = await Kit(loop).up()
    box = await kit.claim()
    box["hdl"].release()
    await settle(loop)
    seen = []
    mod_fsm.set_transition_tracer(
        lambda fsm, st: seen.append([type(fsm).__name__, st]))
    try:
        box = await kit.claim()
        box["hdl"].release()
        await settle(loop)
    finally:
        mod_fsm.set_transition_tracer(None)
    await kit.stop()
    return seen


# -- 6: claim call shapes ---------------------------------------------------

async def sc_claim_shapes(loop):
    out = {}
    kit = await Kit(loop).up()
    pool = kit.pool

    async def one(name, call):
        box = kit.claim_box()
        ret = call(box["cb"])
        sync = "err" in box                 # never from inside claim()
        await settle(loop)
        out[name] = {"sync": sync, "err": type(box.get("err")).__name__,
                     "same": box.get("hdl") is ret,
                     "conn": box.get("conn") is kit.conns[0]}
        if box.get("hdl") is not None:
            box["hdl"].release()
            await settle(loop)

    await one("cb", lambda cb: pool.claim(cb))
    await one("dict_cb", lambda cb: pool.claim({}, cb))
    await one("none_cb", lambda cb: pool.claim(None, cb))
    await one("keywords", lambda cb: pool.claim(options={}, cb=cb))
    await one("cb_keyword", lambda cb: pool.claim({}, cb=cb))
    await one("timeout", lambda cb: pool.claim({"timeout": 1000}, cb))
    await one("avoid", lambda cb: pool.claim({"avoidBackends": ["b1"]}, cb))
    await one("bound", lambda cb: ConnectionPool.claim(pool, {}, cb))
    try:
        pool.claim({})
    except TypeError as e:
        out["no_cb"] = str(e)
    out["claims"] = pool.get_stats()["counters"]["claim"]

    pool.stop()                             # stopping, then stopped
    box = kit.claim_box()
    stub = pool.claim({}, box["cb"])
    out["stopping_sync"] = "err" in box
    await settle(loop)
    out["stopping"] = [type(box["err"]).__name__, type(stub).__name__]
    out["claims_after"] = pool.get_stats()["counters"]["claim"]
    await kit.stop()

    kit = await Kit(loop, targetClaimDelay=100).up()
    box = kit.claim_box()
    ret = kit.pool.claim({}, box["cb"])
    await settle(loop)
    out["codel"] = [box["err"] is None, box["hdl"] is ret,
                    ret.ch_claim_timeout < float("inf")]
    box["hdl"].release()
    await settle(loop)
    await kit.stop()

    kit = Kit(loop)                         # its connection never connects
    kit.resolver.add("b1", {})
    await advance(loop, 10.0)
    out["failed_state"] = kit.pool.get_state()
    box = kit.claim_box()
    kit.pool.claim({}, box["cb"])
    await settle(loop)
    out["failed"] = type(box.get("err")).__name__
    kit.pool.stop()
    await advance(loop, 10.0)
    return out


SCENARIOS = {
    "event_order": sc_event_order,
    "event_order_a_removed": sc_event_order_a_removed,
    "once_listener": sc_once_listener,
    "smgr_error_idle": sc_smgr_error_idle,
    "smgr_closed_idle": sc_smgr_closed_idle,
    "smgr_error_busy": sc_smgr_error_busy,
    "smgr_closed_busy": sc_smgr_closed_busy,
    "unwanted_idle": sc_unwanted_idle,
    "handle_close": sc_handle_close,
    "cancel_while_waiting": sc_cancel_while_waiting,
    "claim_timeout": sc_claim_timeout,
    "lost_race_at_busy": sc_lost_race_at_busy,
    "stale_slot_hook": sc_stale_slot_hook,
    "stale_smgr_hook": sc_stale_smgr_hook,
    "tracer_mid_run": sc_tracer_mid_run,
    "claim_shapes": sc_claim_shapes,
}


def _run_all():
    return {name: run_vt(fn) for name, fn in SCENARIOS.items()}


@pytest.fixture(scope="module")
def here():
    return _run_all()


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


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_same_on_both_runtimes(name, here, pure):
    assert json.loads(json.dumps(here[name])) == pure[name]


def test_event_order_on_the_handle(here):
    rec = here["event_order"]
    by = {n: [(st, sl) for who, st, sl in rec if who == n] for n in "ABC"}
    # A was there before the flush: it hears of every state
    assert [st for st, _ in by["A"]] == ["waiting", "claiming", "claimed",
                                         "released"]
    # B came during the emission of `waiting`, C after `claimed`
    assert [st for st, _ in by["B"]] == ["claiming", "claimed", "released"]
    assert [st for st, _ in by["C"]] == ["released"]
    # the slot reacts to `released` after A and before B and C
    assert by["A"][-1] == ("released", "busy")
    assert by["B"][-1] == ("released", "idle")
    assert by["C"][-1] == ("released", "idle")
    # and in that order
    assert [who for who, st, _ in rec if st == "released"] == ["A", "B", "C"]


def test_removing_a_listener_keeps_the_slots_place(here):
    rec = here["event_order_a_removed"]
    rel = [(who, sl) for who, st, sl in rec if st == "released"]
    assert rel == [("B", "idle"), ("C", "idle")]
    # with no listener before it the slot still reacted
    rec = here["once_listener"]
    assert rec == [["once", "released", "idle"], ["on", "released", "idle"],
                   1]


@pytest.mark.skipif(not mod_fsm.NATIVE,
                    reason="the pure handle lists its ticket")
def test_listeners_of_a_handle_are_the_users():
    async def body(loop):
        kit = await Kit(loop).up()
        box = kit.claim_box()
        hdl = kit.pool.claim({}, box["cb"])
        # the one visible difference from the pure runtime
        # (docs/internals.md): the library's own listeners are not listed
        assert hdl.listeners("stateChanged") == []
        assert hdl.event_names() == []
        assert hdl.listener_count("stateChanged") == 0
        await settle(loop)
        assert box["hdl"] is hdl and kit.slot().is_in_state("busy")
        assert hdl.listeners("stateChanged") == []
        assert hdl.event_names() == []

        def f(st):
            pass

        def g(st):
            pass

        hdl.on("stateChanged", f)
        w = hdl.once("stateChanged", g)
        assert hdl.listeners("stateChanged") == [f, w]
        assert hdl.event_names() == ["stateChanged"]
        hdl.remove_listener("stateChanged", f)
        assert hdl.listeners("stateChanged") == [w]
        hdl.release()
        await settle(loop)
        assert hdl.listeners("stateChanged") == []
        assert kit.slot().is_in_state("idle")
        # the slot's own listeners: the dispatcher, and `unwanted`
        assert len(kit.slot().listeners("stateChanged")) == 1
        assert sorted(kit.slot().event_names()) == ["stateChanged",
                                                    "unwanted"]
        await kit.stop()
    run_vt(body)


def _follows(hist, a, b):
    """state b was entered right after state a"""
    return any(x == a and y == b for x, y in zip(hist, hist[1:]))


def test_cold_exits(here):
    assert _follows(here["smgr_error_idle"]["slot"], "idle", "retrying")
    assert _follows(here["smgr_closed_idle"]["slot"], "idle", "connecting")
    # while busy the slot only notes what it saw; it moves on release
    assert here["smgr_error_busy"]["slot_then"][-1] == "busy"
    assert _follows(here["smgr_error_busy"]["slot"], "busy", "retrying")
    assert here["smgr_closed_busy"]["slot_then"][-1] == "busy"
    assert _follows(here["smgr_closed_busy"]["slot"], "busy", "connecting")
    assert here["unwanted_idle"]["names"] == ["stateChanged", "unwanted"]
    assert here["unwanted_idle"]["slot"][-3:] == ["idle", "stopping",
                                                  "stopped"]
    assert here["handle_close"]["handle"][-1] == "closed"
    assert _follows(here["handle_close"]["slot"], "busy", "killing")
    c = here["cancel_while_waiting"]
    assert (c["queued"], c["linked"], c["after"], c["node_gone"]) == \
        (1, True, 0, True)
    assert c["called"] is False and c["h2"][-1] == "cancelled"
    t = here["claim_timeout"]
    assert (t["queued"], t["after"], t["err"]) == \
        (1, 0, ClaimTimeoutError.__name__)
    assert t["h2"][-1] == "failed" and t["slot"][-1] == "idle"
    # the slot saw no event of the socket manager's yet: it treats the
    # rejected claim as released, and learns of the close back in idle
    r = here["lost_race_at_busy"]
    assert r["called"] is False and r["slot_handle"] is True
    assert r["handle"][-3:] == ["waiting", "claiming", "waiting"]
    assert r["slot"][-3:] == ["busy", "idle", "connecting"]
    assert r["handle_end"][-1] == "cancelled"


def test_stale_handler_does_nothing(here):
    assert here["stale_slot_hook"]["slot"][-3:] == ["busy", "stopping",
                                                    "stopped"]
    assert here["stale_slot_hook"]["handle"][-1] == "released"
    assert here["stale_smgr_hook"]["slot"][-2:] == ["idle", "stopped"]


def test_tracer_set_mid_run_sees_the_six_transitions(here):
    assert [st for _, st in here["tracer_mid_run"]] == [
        "waiting", "claiming", "busy", "claimed", "released", "idle"]


def test_claim_call_shapes(here):
    s = here["claim_shapes"]
    ok = {"sync": False, "err": "NoneType", "same": True, "conn": True}
    for name in ("cb", "dict_cb", "none_cb", "keywords", "cb_keyword",
                 "timeout", "avoid", "bound"):
        assert s[name] == ok, name
    assert "callback" in s["no_cb"]
    assert s["claims"] == 8 and s["claims_after"] == 9
    assert s["stopping_sync"] is False
    assert s["stopping"] == [PoolStoppingError.__name__, "_CancelStub"]
    assert s["codel"] == [True, True, True]
    assert s["failed_state"] == "failed"
    assert s["failed"] == PoolFailedError.__name__
    assert inspect.getdoc(ConnectionPool.claim)
    assert "avoidBackends" in inspect.getdoc(ConnectionPool.claim)


# -- 7: resource hygiene ----------------------------------------------------

def test_5000_cycles_with_and_without_listeners_leave_nothing_behind():
    """test_5000_cycles_leave_nothing_behind with a listener on every
    tenth handle: the handles without one never get an event dict, the
    others go through the listener list."""
    states = [sys.intern(s) for s in [
        "idle", "busy", "waiting", "claiming", "claimed", "released",
        "stateChanged", "connected"]]

    async def body(loop):
        kit = await Kit(loop).up()
        pool = kit.pool
        left = {"n": 0, "heard": 0}
        done = loop.create_future()

        def listener(st):
            left["heard"] += 1

        def cb(err, hdl=None, conn=None):
            assert err is None
            if left["n"] % 10 == 0:
                hdl.on("stateChanged", listener)
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
            left["heard"] = 0
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
        # each of the 500 listeners came during the emission of
        # `waiting` and heard `claiming`, `claimed` and `released`
        assert left["heard"] == 1500
        assert pool.get_stats()["counters"]["claim"] >= 5200
        await kit.stop()
    run_vt(body)


if __name__ == "__main__":
    if sys.argv[1:] == ["--scenarios"]:
        res = _run_all()
        res["native"] = mod_fsm.NATIVE
        print(json.dumps(res))
