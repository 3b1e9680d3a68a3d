"""The pool's native claim context and the smaller claim handle: what a
claimer observes is what the pure-Python runtime shows.

The native core reads the attributes that ``ConnectionPool.__init__``
binds once (queues, counters, latency recorder, claim log, dead map,
whether there is a CoDel) from a per-pool context object instead of the
instance dict, and the handle refers to that context instead of copying
from it.  Pools here have 1 or 2 backends on the virtual clock.  The
scenarios return plain data; they run on the runtime this process
selected and once more, all together, in a child process on the
pure-Python runtime, and the results are compared.
"""

import gc
import json
import math
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from cueball_amd import fsm as mod_fsm  # noqa: E402
from cueball_amd import pool as mod_pool  # noqa: E402
from cueball_amd.connection_fsm import (ClaimHandle,  # noqa: E402
                                        ConnectionSlotFSM)
from cueball_amd.events import EventEmitter  # noqa: E402
from cueball_amd.fsm import FSM, FSMError  # noqa: E402
from cueball_amd.latency import PoolLatency  # noqa: E402
from cueball_amd.logutil import default_logger  # noqa: E402
from cueball_amd.pool import ConnectionPool  # noqa: E402
from cueball_amd.resolver import ResolverFSM  # noqa: E402
from cueball_amd.testing import (DummyConnection, DummyResolver,  # noqa: E402
                                 VirtualLoop, advance, settle)

RECOVERY = {"default": {"timeout": 500, "retries": 1, "delay": 0}}

native_only = pytest.mark.skipif(
    not mod_fsm.NATIVE, reason="about the native core's own objects")


def run_vt(body):
    loop = VirtualLoop()
    try:
        return loop.run_until_complete(body(loop))
    finally:
        loop.close()


class Kit:
    """A pool of `n` backends, one connected connection each."""

    def __init__(self, loop, n=1, **options):
        self.loop = loop
        self.n = n
        self.conns = []
        self.keep = []
        self.resolver = DummyResolver()
        self.rfsm = ResolverFSM(self.resolver, {"loop": loop})

        def constructor(backend):
            c = DummyConnection(backend)
            self.conns.append(c)
            return c

        opts = {"domain": "ctx.test", "constructor": constructor,
                "recovery": RECOVERY, "spares": n, "maximum": n,
                "resolver": self.rfsm, "loop": loop}
        opts.update(options)
        self.pool = ConnectionPool(opts)
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

    async def claim(self):
        box = {}

        def cb(err, hdl=None, conn=None):
            box.update(err=err, hdl=hdl, conn=conn)

        box["ret"] = self.pool.claim({}, cb)
        await settle(self.loop)
        return box

    async def cycles(self, n):
        """n claim/release cycles, each claim made in the callback of
        the one before."""
        pool = self.pool
        left = {"n": n}
        done = self.loop.create_future()

        def cb(err, hdl=None, conn=None):
            assert err is None
            hdl.release()
            left["n"] -= 1
            if left["n"] > 0:
                pool.claim({}, cb)
            else:
                done.set_result(None)

        # cb refers to itself: kept, so that this cycle of the test's own
        # is not garbage while a test counts
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


def _tail(fsm, n):
    return fsm.get_state_history()[-n:]


def instance_vars(pool):
    """vars(pool); the native runtime's objects keep their instance dict
    without a ``__dict__`` attribute, so there it is found among the
    object's referents."""
    try:
        return vars(pool)
    except TypeError:
        for ref in gc.get_referents(pool):
            if isinstance(ref, dict) and "p_idleq" in ref:
                return ref
        raise


class FakePool:
    """no FSM, no queues: only what a bare handle asks of its pool"""

    def __init__(self, loop):
        self.p_lat = PoolLatency(loop)


class StandingSlot:
    """stands still in the handshake: claim() neither accepts nor
    rejects"""

    def __init__(self):
        self.asked = []

    def is_in_state(self, st):
        self.asked.append(st)
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


# -- counters: 1 connection, 3 claimers, 30 claims --------------------------

async def sc_counters_queueing(loop):
    """Three claimers share the one connection; a claimer that is served
    releases, and claims again once the next in line has been served."""
    kit = await Kit(loop).up()
    pool = kit.pool
    served = []

    def cb(err, hdl=None, conn=None):
        assert err is None
        served.append(hdl)

    issued = 0
    for _ in range(3):
        pool.claim({}, cb)
        issued += 1
    await settle(loop)
    depth = [len(pool.p_waiters)]
    done = 0
    while done < 30:
        assert len(served) == done + 1          # one is served at a time
        served[done].release()
        done += 1
        await settle(loop)
        if issued < 30:
            pool.claim({}, cb)
            issued += 1
            await settle(loop)
        depth.append(len(pool.p_waiters))
    out = {
        "claim": pool.p_counters["claim"],
        "queued": pool.p_counters["queued-claim"],
        "maxq": pool.p_counters["max-claim-queue"],
        "busy_hwm": pool.p_busy_hwm,
        "demand_hwm": pool.p_demand_hwm,
        "stats": pool.get_stats(),
        "depth": depth,
    }
    await kit.stop()
    return out


# -- what a handle shows ------------------------------------------------------

async def sc_handle_attributes(loop):
    kit = await Kit(loop).up()
    box = await kit.claim()
    hdl = box["hdl"]
    out = {
        "log": hdl.ch_log is kit.pool.p_claim_log,
        "pool": hdl.ch_pool is kit.pool,
        "slot": hdl.ch_slot is kit.slot(),
        "conn": hdl.ch_connection is kit.conns[0]
        and box["conn"] is kit.conns[0],
        "ret": box["ret"] is hdl,
        "flags": [int(hdl.ch_cancelled), int(hdl.ch_pinger),
                  int(hdl.ch_throw_error),
                  int(hdl.ch_do_release_leak_check)],
    }
    hdl.disable_release_leak_check()
    out["flags_after"] = int(hdl.ch_do_release_leak_check)
    hdl.release()
    await settle(loop)
    out["log_after"] = hdl.ch_log is kit.pool.p_claim_log
    await kit.stop()

    # a bare handle on a pool that is no FSM: its own log, and the
    # pool's recorder
    fake = FakePool(loop)
    called = []
    bare = bare_handle(fake, loop, called)
    out["bare_log"] = bare.ch_log is not None and \
        bare.ch_log is not kit.pool.p_claim_log
    out["bare_pool"] = bare.ch_pool is fake
    bare.try_(StandingSlot())
    await advance(loop, 0.125)
    bare.accept(EventEmitter())
    out["bare_called"] = len(called)
    await advance(loop, 0.25)
    bare.release()
    await settle(loop)
    out["bare_wait"] = [fake.p_lat.wait.count,
                        round(fake.p_lat.wait.sum_ms)]
    out["bare_hold"] = [fake.p_lat.hold.count,
                        round(fake.p_lat.hold.sum_ms)]
    out["bare_state"] = bare.get_state()
    return out


# -- a handle that outlives its pool; p_backends rebound ---------------------

async def sc_release_after_stop(loop):
    kit = await Kit(loop).up()
    box = await kit.claim()
    hdl, slot, pool = box["hdl"], kit.slot(), kit.pool
    pool.stop()
    await settle(loop)
    out = {"pool_then": pool.get_state(), "slot_then": slot.get_state(),
           "handle_then": hdl.get_state()}
    hdl.release()
    await settle(loop)
    if not pool.is_in_state("stopped"):
        await advance(loop, 10.0)
    out["pool"] = _tail(pool, 3)
    out["slot"] = _tail(slot, 4)
    out["handle"] = _tail(hdl, 2)
    out["backends"] = pool.p_backends
    return out


async def sc_backends_rebound(loop):
    """What state_stopped does to the pool's maps, done while a handle
    is out: the slot that goes idle afterwards is no backend's any
    more."""
    kit = await Kit(loop).up()
    box = await kit.claim()
    slot = kit.slot()
    kit.pool.p_keys = []
    kit.pool.p_connections = {}
    kit.pool.p_backends = {}
    box["hdl"].release()
    await settle(loop)
    await advance(loop, 1.0)
    out = {"slot": _tail(slot, 5), "handle": _tail(box["hdl"], 2),
           "idle": len(kit.pool.p_idleq)}
    await kit.stop()
    return out


async def sc_pool_vars(loop):
    fresh = Kit(loop)
    out = {"fresh_ctx": getattr(fresh.pool, "_claim_ctx", None) is None}
    names0 = set(instance_vars(fresh.pool))
    kit = await Kit(loop).up()
    await kit.cycles(10)
    out["same_vars"] = set(instance_vars(kit.pool)) == names0
    out["claims"] = kit.pool.p_counters["claim"]
    await kit.stop()
    await fresh.stop()
    return out


# -- transitions ---------------------------------------------------------------

def _refused(hdl, to):
    before = hdl.get_state()
    try:
        hdl.goto_state(to)
    except FSMError as e:
        return [before, to, str(e), hdl.get_state()]
    return [before, to, None, hdl.get_state()]


async def sc_invalid_transitions(loop):
    fake = FakePool(loop)
    out = []
    h = bare_handle(fake, loop)
    out.append(_refused(h, "released"))             # waiting
    h.try_(StandingSlot())
    out.append(_refused(h, "released"))             # claiming
    h.accept(EventEmitter())
    out.append(_refused(h, "waiting"))              # claimed
    h.release()
    out.append(_refused(h, "waiting"))              # released
    h = bare_handle(fake, loop)
    h.try_(StandingSlot())
    h.accept(EventEmitter())
    h.close()
    out.append(_refused(h, "claimed"))              # closed
    h = bare_handle(fake, loop)
    h.cancel()
    out.append(_refused(h, "waiting"))              # cancelled
    h = bare_handle(fake, loop)
    h.fail(RuntimeError("no"))
    out.append(_refused(h, "claiming"))             # failed
    await settle(loop)
    return out


class ListFSM(FSM):
    """valid_transitions given as a list of strings built at run time:
    equal to the state names, not the same objects"""

    def __init__(self, loop):
        super().__init__("one", loop=loop)

    def state_one(self, S):
        S.valid_transitions(["".join(["t", "w", "o"])])

    def state_two(self, S):
        S.valid_transitions(["-".join(["thr", "ee"]).replace("-", "")])

    def state_three(self, S):
        S.valid_transitions([])


async def sc_list_valid(loop):
    f = ListFSM(loop)
    out = []
    try:
        f.goto_state("three")
    except FSMError as e:
        out.append(str(e))
    f.goto_state("".join(["tw", "o"]))
    f.goto_state("three")
    out.append(f.get_state_history())
    await settle(loop)
    return out


# -- subclasses ----------------------------------------------------------------

async def sc_subclasses(loop):
    class MyHandle(ClaimHandle):
        pass

    class MySlot(ConnectionSlotFSM):
        pass

    saved = (mod_pool.ClaimHandle, mod_pool.ConnectionSlotFSM)
    mod_pool.ClaimHandle, mod_pool.ConnectionSlotFSM = MyHandle, MySlot
    try:
        kit = await Kit(loop).up()
        slot = kit.slot()
        out = {"slot_cls": type(slot).__name__}
        box = {}

        def cb(err, hdl=None, conn=None):
            box.update(err=err, hdl=hdl, conn=conn)

        # with options the call goes through the Python claim(), which
        # builds the handle from the class the module names
        ret = kit.pool.claim({"timeout": 1000}, cb)
        await settle(loop)
        hdl = box["hdl"]
        out["handle_cls"] = type(hdl).__name__
        out["ret"] = ret is hdl
        out["conn"] = box["conn"] is kit.conns[0]
        out["slot_busy"] = slot.get_state()
        out["log"] = hdl.ch_log is kit.pool.p_claim_log
        hdl.release()
        await settle(loop)
        out["handle"] = _tail(hdl, 4)
        out["slot"] = _tail(slot, 3)
        # and a second claimer queued behind the first
        a = await kit.claim()
        b = await kit.claim()
        out["queued"] = [a["hdl"].get_state(), b["ret"].get_state(),
                         len(kit.pool.p_waiters)]
        a["hdl"].release()
        await settle(loop)
        out["fed"] = [b["hdl"] is b["ret"], b["ret"].get_state()]
        b["hdl"].release()
        await settle(loop)
        await kit.stop()
        return out
    finally:
        mod_pool.ClaimHandle, mod_pool.ConnectionSlotFSM = saved


async def sc_try_on_slots(loop):
    out = {}
    fake = FakePool(loop)
    slot = StandingSlot()
    h = bare_handle(fake, loop)
    h.try_(slot)
    out["asked"] = slot.asked
    out["state"] = h.get_state()

    kit = await Kit(loop).up()
    box = await kit.claim()                         # the slot is busy now
    h2 = bare_handle(kit.pool, loop)
    try:
        h2.try_(kit.slot())
        out["busy_slot"] = None
    except FSMError as e:
        out["busy_slot"] = "idle slot" in str(e)
    out["h2"] = h2.get_state()
    h2.cancel()
    box["hdl"].release()
    await settle(loop)
    await kit.stop()
    return out


SCENARIOS = {
    "counters_queueing": sc_counters_queueing,
    "handle_attributes": sc_handle_attributes,
    "release_after_stop": sc_release_after_stop,
    "backends_rebound": sc_backends_rebound,
    "pool_vars": sc_pool_vars,
    "invalid_transitions": sc_invalid_transitions,
    "list_valid": sc_list_valid,
    "subclasses": sc_subclasses,
    "try_on_slots": sc_try_on_slots,
}


def _run_all():
    return {name: run_vt(fn) for name, fn in SCENARIOS.items()}


def _plain(res):
    """What both runtimes must agree on: the texts of the refused
    transitions name the valid states as the runtime holds them (a tuple
    here, a list there), so only their from/to/outcome are compared."""
    res = json.loads(json.dumps(res))
    res["invalid_transitions"] = [
        [a, b, text is not None, c]
        for a, b, text, c in res["invalid_transitions"]]
    return res


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
    assert _plain(here)[name] == _plain(pure)[name]


@native_only
def test_handle_fits_the_small_object_allocator():
    # 512 bytes less the 16 of the collector's header
    assert ClaimHandle.__basicsize__ <= 496


def test_counters_of_a_queueing_run(here):
    c = here["counters_queueing"]
    assert c["claim"] == 30
    # one connection and three claimers: every claim but the first finds
    # it busy and queues, behind at most one other
    assert c["queued"] == 29 and c["maxq"] == 2
    assert c["depth"] == [2] * 28 + [1, 0, 0]
    assert c["busy_hwm"] <= 1 and c["demand_hwm"] <= 3
    assert c["stats"]["counters"]["claim"] == 30
    assert c["stats"]["counters"]["queued-claim"] == 29


def test_handle_attributes(here):
    a = here["handle_attributes"]
    for name in ("log", "pool", "slot", "conn", "ret", "log_after",
                 "bare_log", "bare_pool"):
        assert a[name] is True, name
    assert a["flags"] == [0, 0, 1, 1] and a["flags_after"] == 0
    # the bare handle waited 125 ms and held for 250, on its own pool's
    # recorder
    assert a["bare_called"] == 1 and a["bare_state"] == "released"
    assert a["bare_wait"] == [1, 125] and a["bare_hold"] == [1, 250]


def test_release_after_the_pool_was_told_to_stop(here):
    r = here["release_after_stop"]
    assert r["handle_then"] == "claimed" and r["slot_then"] == "busy"
    assert r["handle"] == ["claimed", "released"]
    assert r["slot"][-1] == "stopped" and r["pool"][-1] == "stopped"
    assert r["backends"] == {}
    b = here["backends_rebound"]
    # not parked on the idle queue: told it is unwanted, and it stops
    assert b["handle"] == ["claimed", "released"] and b["idle"] == 0
    assert b["slot"][-3:] == ["idle", "stopping", "stopped"]


def test_a_pool_that_never_claimed(here):
    v = here["pool_vars"]
    assert v == {"fresh_ctx": True, "same_vars": True, "claims": 10}


@native_only
def test_the_context_hangs_off_the_pool_not_its_dict():
    async def body(loop):
        kit = await Kit(loop).up()
        pool = kit.pool
        await kit.cycles(3)
        ctx = pool._claim_ctx
        assert ctx is not None and all(v is not ctx for v in instance_vars(pool).values())
        assert type(ctx).__name__ == "_PoolCtx"
        # one per pool, for every handle of it
        box = await kit.claim()
        assert pool._claim_ctx is ctx
        n = sys.getrefcount(ctx)
        box2 = await kit.claim()                    # queued: a second handle
        assert sys.getrefcount(ctx) == n + 1
        box["hdl"].release()
        await settle(loop)
        box2["hdl"].release()
        await settle(loop)
        # the boxes are in a cycle with their handles (the callback);
        # the slot remembers the last handle it served, no other
        del box, box2
        gc.collect()
        assert sys.getrefcount(ctx) == n - 1
        # it does not keep the pool
        assert pool not in gc.get_referents(ctx)
        assert ctx in gc.get_referents(pool)
        await kit.stop()
    run_vt(body)


def test_invalid_transitions_out_of_every_handle_state(here):
    rows = here["invalid_transitions"]
    assert [(a, b, c) for a, b, _, c in rows] == [
        ("waiting", "released", "waiting"),
        ("claiming", "released", "claiming"),
        ("claimed", "waiting", "claimed"),
        ("released", "waiting", "released"),
        ("closed", "claimed", "closed"),
        ("cancelled", "waiting", "cancelled"),
        ("failed", "claiming", "failed")]
    if not mod_fsm.NATIVE:
        assert all(text for _, _, text, _ in rows)
        return
    valid = {"waiting": ("claiming", "cancelled", "failed"),
             "claiming": ("claimed", "waiting", "cancelled"),
             "claimed": ("released", "closed")}
    for a, b, text, _ in rows:
        assert text == "ClaimHandle: invalid transition %r -> %r " \
            "(valid: %r)" % (a, b, valid.get(a, ())), a


def test_valid_transitions_as_a_list_of_equal_strings(here):
    text, hist = here["list_valid"]
    assert text == "ListFSM: invalid transition 'one' -> 'three' " \
        "(valid: ['two'])"
    assert hist == ["one", "two", "three"]


def test_user_subclasses_walk_the_cycle(here):
    s = here["subclasses"]
    assert s["handle_cls"] == "MyHandle" and s["slot_cls"] == "MySlot"
    assert s["ret"] and s["conn"] and s["log"]
    assert s["slot_busy"] == "busy"
    assert s["handle"] == ["waiting", "claiming", "claimed", "released"]
    assert s["slot"] == ["idle", "busy", "idle"]
    assert s["queued"] == ["claimed", "waiting", 1]
    assert s["fed"] == [True, "claimed"]


def test_try_on_a_foreign_slot_and_on_a_busy_native_one(here):
    t = here["try_on_slots"]
    assert t["asked"] == ["idle"] and t["state"] == "claiming"
    assert t["busy_slot"] is True and t["h2"] == "waiting"


@native_only
def test_a_non_handle_in_the_waiter_queue_is_skipped():
    async def body(loop):
        kit = await Kit(loop).up()
        a = await kit.claim()
        kit.pool.p_waiters.push(object())           # ahead of the claimer
        b = await kit.claim()
        assert len(kit.pool.p_waiters) == 2
        a["hdl"].release()
        await settle(loop)
        assert b["hdl"] is b["ret"] and b["hdl"].is_in_state("claimed")
        assert len(kit.pool.p_waiters) == 0
        b["hdl"].release()
        await settle(loop)
        await kit.stop()
    run_vt(body)


# -- resource hygiene ---------------------------------------------------------

@native_only
def test_a_handle_that_outlives_its_pool_leaves_no_garbage():
    """Claim, tell the pool to stop, drop everything but the handle:
    release() works on what the handle keeps alive, the pool stops, and
    with the collector off nothing of that is left unreachable.  A
    stopped pool that is dropped is cyclic, as it always was; the
    context is part of that and goes with it."""
    import weakref

    async def body(loop):
        kit = await Kit(loop).up()
        box = await kit.claim()
        hdl = box["hdl"]
        box.clear()                 # or handle, callback and box are a cycle
        ctx = kit.pool._claim_ctx
        kit.pool.stop()
        await settle(loop)
        del box, kit
        gc.collect()
        gc.disable()
        try:
            assert hdl.ch_log is hdl.ch_pool.p_claim_log
            hdl.release()
            await settle(loop)
            await advance(loop, 10.0)
            assert hdl.is_in_state("released")
            assert hdl.ch_pool.is_in_state("stopped")
            assert hdl.ch_pool._claim_ctx is ctx
            assert gc.collect() == 0
        finally:
            gc.enable()
        # the collector sees through the context: what it holds ...
        pool = hdl.ch_pool
        held = gc.get_referents(ctx)
        for obj in (pool.p_counters, pool.p_dead, pool.p_claim_log,
                    pool.p_idleq, pool.p_waiters, pool.p_initq):
            assert any(obj is h for h in held)
        assert not any(pool is h for h in held)
        # ... and that pool, context and handle are freed together
        gone = weakref.ref(pool)
        del pool, held, ctx, hdl
        gc.collect()
        assert gone() is None
    run_vt(body)


@native_only
def test_5000_cycles_leave_nothing_behind():
    states = [sys.intern(s) for s in [
        "idle", "busy", "waiting", "claiming", "claimed", "released",
        "stateChanged", "connected"]]

    async def body(loop):
        kit = await Kit(loop).up()
        pool = kit.pool
        await kit.cycles(200)                       # warm every lazy path
        ctx = pool._claim_ctx
        watched = [None, True, ctx, pool.p_counters, pool.p_claim_log,
                   pool.p_idleq, pool.p_waiters] + states
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
        assert all(abs(d) <= 20 for d in drift[:2]), drift
        # the context and what it holds: exactly as before
        assert drift[2:7] == [0, 0, 0, 0, 0], drift
        assert all(abs(d) <= 20 for d in drift[7:]), drift
        assert pool._claim_ctx is ctx
        assert pool.get_stats()["counters"]["claim"] == 5200
        await kit.stop()
    run_vt(body)


if __name__ == "__main__":
    if sys.argv[1:] == ["--scenarios"]:
        res = _run_all()
        res["native"] = mod_fsm.NATIVE
        print(json.dumps(res))
