"""ConnectionSet fuzzing with connection age in use: the added/removed
contract under churn, with ``recycle()`` and leaps of the clock past a
lifetime thrown in.  Make-before-break relaxes the set's singleton
invariant to "at most two advertised connections per backend, on at
most one backend at a time", and adds one of its own: a connection that
is 'removed' because it was recycled has a successor advertised at that
very moment."""

from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from cueball_amd.connection_set import ConnectionSet
from cueball_amd.testing import (DummyConnection, DummyResolver,
                                 VirtualLoop, advance)
from cset_age_kit import leap

RECOVERY = {"default": {"timeout": 500, "retries": 2, "delay": 0}}
AGE = 2_000
MAXIMUM = 4

CSET_ACTIONS = st.lists(
    st.tuples(
        st.sampled_from([
            "add_backend", "remove_backend", "connect", "conn_error",
            "conn_close", "set_target", "close_handle", "tick",
            "big_tick", "recycle", "leap",
        ]),
        st.integers(min_value=0, max_value=7),
    ),
    min_size=5,
    max_size=50,
)


@settings(max_examples=120, deadline=None,
          suppress_health_check=[HealthCheck.too_slow])
@given(actions=CSET_ACTIONS)
def test_cset_with_age_survives_random_interleavings(actions):
    loop = VirtualLoop()
    try:
        loop.run_until_complete(_cset_age_scenario(loop, actions))
    finally:
        loop.close()


def _split(ckey):
    backend, serial = ckey.rsplit(".", 1)
    return backend, int(serial)


async def _cset_age_scenario(loop, actions):
    conns = []
    resolver = DummyResolver()

    def ctor(backend):
        c = DummyConnection(backend)
        c.key = backend.get("key")
        conns.append(c)
        orig = c.destroy

        def destroy():
            if c in conns:
                conns.remove(c)
            orig()

        c.destroy = destroy
        return c

    cset = ConnectionSet({
        "constructor": ctor,
        "recovery": RECOVERY,
        "target": 2,
        "maximum": MAXIMUM,
        "resolver": resolver,
        "maxConnectionAge": AGE,
        "connectionAgeSpread": 0.5,
        "loop": loop,
    })

    advertised = {}   # ckey -> (conn, hdl)
    all_added = []
    all_removed = []
    # predecessors named by a 'connectionRecycled' while their
    # successor was advertised too: each must be 'removed' next
    due_removed = set()

    def check_advertised():
        per_backend = {}
        for ck in advertised:
            bk = _split(ck)[0]
            per_backend[bk] = per_backend.get(bk, 0) + 1
        assert all(v <= 2 for v in per_backend.values()), per_backend
        assert sum(1 for v in per_backend.values() if v == 2) <= 1, \
            per_backend

    def on_added(ckey, conn, hdl):
        assert ckey not in advertised, "double-advertise of %s" % ckey
        assert ckey not in all_added, "ckey reuse: %s" % ckey
        advertised[ckey] = (conn, hdl)
        all_added.append(ckey)
        check_advertised()

    def on_removed(ckey, conn, hdl):
        assert ckey in advertised, "removed before added: %s" % ckey
        advertised.pop(ckey)
        all_removed.append(ckey)
        if ckey in due_removed:
            # removed because it was recycled: the successor is up
            due_removed.discard(ckey)
            backend, serial = _split(ckey)
            assert any(_split(ck)[0] == backend and
                       _split(ck)[1] > serial for ck in advertised), \
                (ckey, sorted(advertised))
        hdl.release()

    def on_recycled(key, reason):
        assert reason in ("age", "manual")
        assert not due_removed
        serials = sorted(_split(ck)[1] for ck in advertised
                         if _split(ck)[0] == key)
        if len(serials) == 2:
            due_removed.add("%s.%d" % (key, serials[0]))

    cset.on("added", on_added)
    cset.on("removed", on_removed)
    cset.on("connectionRecycled", on_recycled)
    resolver.start()

    backends = set()
    next_backend = [0]

    # Start from a set that has something to recycle: two backends, up
    # and advertised.  A random walk from nothing seldom gets that far
    # before it ends.
    for _ in range(2):
        k = "c%d" % next_backend[0]
        next_backend[0] += 1
        backends.add(k)
        resolver.add(k, {})
    await advance(loop, 0.05)
    for c in list(conns):
        c.connect()
    await advance(loop, 0.05)
    assert len(advertised) == 2

    for kind, seed in actions:
        if kind == "add_backend":
            k = "c%d" % next_backend[0]
            next_backend[0] += 1
            backends.add(k)
            resolver.add(k, {})
        elif kind == "remove_backend":
            if backends:
                k = sorted(backends)[seed % len(backends)]
                backends.discard(k)
                resolver.remove(k)
        elif kind == "connect":
            live = [c for c in conns if not c.connected and not c.dead]
            if live:
                live[seed % len(live)].connect()
        elif kind == "conn_error":
            live = [c for c in conns if not c.dead]
            if live:
                c = live[seed % len(live)]
                c.once("error", lambda e: None)
                c.emit("error", RuntimeError("prop"))
        elif kind == "conn_close":
            live = [c for c in conns if not c.dead]
            if live:
                live[seed % len(live)].emit("close")
        elif kind == "set_target":
            cset.set_target(1 + seed % 4)
        elif kind == "close_handle":
            if advertised:
                ck = sorted(advertised)[seed % len(advertised)]
                conn, hdl = advertised.pop(ck)
                hdl.close()
        elif kind == "recycle":
            n = cset.recycle()
            assert 0 <= n <= len(advertised)
        elif kind == "leap":
            await leap(loop, AGE / 1000.0 + 0.001)
        elif kind == "tick":
            await advance(loop, 0.05)
        elif kind == "big_tick":
            await advance(loop, 0.7)

        # invariants
        assert len(all_added) == len(set(all_added)), "ckey reuse"
        assert not due_removed, "recycled, but never removed"
        check_advertised()
        repl = cset.cs_age_repl
        slots = len(cset.cs_fsm) + (0 if repl is None else 1)
        current_slots = sum(1 for k in cset.cs_fsm
                            if k in cset.cs_backends) + \
            (0 if repl is None else 1)
        assert current_slots <= MAXIMUM + 2
        assert cset.get_stats()["totalConnections"] == slots
        if repl is not None:
            assert cset.cs_fsm.get(repl["key"]) is repl["old"]
            assert repl["new"] not in cset.cs_fsm.values()

    cset.stop()
    await advance(loop, 8.0)
    assert cset.is_in_state("stopped"), {
        k: (f.get_state(), f.csf_smgr.get_state(), f.csf_wanted,
            f.csf_monitor)
        for k, f in cset.cs_fsm.items()}
    # everything advertised was eventually removed
    assert not advertised
    assert cset.cs_age_repl is None and not cset.cs_age_retired
    # no LogicalConnection is left behind
    assert not cset.cs_lconns, {
        ck: lc.get_state() for ck, lc in cset.cs_lconns.items()}
    assert not conns
