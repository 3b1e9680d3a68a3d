"""Resolvers with ``srvRanking``: SRV priority and weight are carried
to the emitted backends, rank edits surface as 'changed', and nothing
moves when the option is off."""

import asyncio

import pytest

from cueball_amd.cli import main as cbresolve_main
from cueball_amd.dns_client import NoNameError
from cueball_amd.dns_wire import DnsMessage
from cueball_amd.resolver import (DNSResolver, DNSResolverFSM,
                                  StaticIpResolver, srv_key)
from cueball_amd.testing import MockDnsServer, advance, settle
from conftest import run_vt

# no spread: TTL sleeps last exactly the TTL, so each advance(SRV_TTL)
# below spans exactly one SRV refresh
RECOVERY = {"default": {"timeout": 1000, "retries": 3, "delay": 100,
                        "delaySpread": 0.0}}
INT_NO_V6 = {
    "lo0": [{"address": "::1", "family": "IPv6"}],
    "foo0": [{"address": "1.2.3.4", "family": "IPv4"}],
}
SRV_NAME = "_svc._tcp.shop.test"
SRV_TTL = 10
TODAYS_KEYS = {"name", "port", "address"}


class ZoneClient:
    """Scripted DNS client answering from an editable zone:
    ``zone[(name, rtype)] = [(target, port, priority, weight), ...]``
    for SRV and ``[address, ...]`` for A.  Unknown names are NXDOMAIN,
    known names without records of the type are NODATA."""

    def __init__(self):
        self.zone = {}
        self.history = []

    def set_srv(self, *records):
        self.zone[(SRV_NAME, "SRV")] = list(records)

    def count(self, rtype, name=None):
        return len([h for h in self.history if h[1] == rtype and
                    (name is None or h[0] == name)])

    def lookup(self, opts, cb, loop=None):
        name, rtype = opts["domain"], opts["type"]
        self.history.append((name, rtype))
        recs = self.zone.get((name, rtype))
        if recs is None and not any(k[0] == name for k in self.zone):
            loop.call_soon(lambda: cb(NoNameError(name), None))
            return
        msg = DnsMessage()
        for rec in recs or ():
            if rtype == "SRV":
                target, port, prio, weight = rec
                msg.answers.append({
                    "type": "SRV", "name": name, "ttl": SRV_TTL,
                    "priority": prio, "weight": weight, "port": port,
                    "target": target})
            else:
                msg.answers.append({"type": rtype, "name": name,
                                    "ttl": 3600, "target": rec})
        loop.call_soon(lambda: cb(None, msg))


def make(loop, nsc, domain="shop.test", **opts):
    DNSResolverFSM._nic_cache = INT_NO_V6
    DNSResolverFSM._nic_cache_updated = loop.time() * 1000.0
    ropts = {"domain": domain, "service": "_svc._tcp", "defaultPort": 80,
             "resolvers": ["1.1.1.1"], "recovery": RECOVERY,
             "_nsclient": nsc, "loop": loop}
    ropts.update(opts)
    return DNSResolver(ropts)


def collect(res):
    ev = []
    res.on("added", lambda k, b: ev.append(("added", k, dict(b))))
    res.on("removed", lambda k: ev.append(("removed", k)))
    res.on("changed", lambda k, b: ev.append(("changed", k, dict(b))))
    # the wrapper consumes 'updated'; the inner machine emits it
    res.r_fsm.on("updated", lambda *a: ev.append(("updated",)))
    return ev


def two_backend_zone():
    nsc = ZoneClient()
    nsc.set_srv(("b1.shop.test", 8080, 0, 30), ("b2.shop.test", 8080, 10, 5))
    nsc.zone[("b1.shop.test", "A")] = ["10.0.0.1"]
    nsc.zone[("b2.shop.test", "A")] = ["10.0.0.2"]
    return nsc


def by_name(backends):
    return {b["name"]: b for b in backends}


def test_option_must_be_bool():
    async def body(loop):
        for bad in (1, "yes", 0):
            with pytest.raises(TypeError):
                make(loop, ZoneClient(), srvRanking=bad)
    run_vt(body)


def test_option_off_emits_todays_dicts_and_never_changed():
    async def body(loop):
        nsc = two_backend_zone()
        res = make(loop, nsc)
        ev = collect(res)
        inner_ev = []
        res.r_fsm.on("changed", lambda *a: inner_ev.append(a))
        res.start()
        await advance(loop, 1.0)
        added = [e for e in ev if e[0] == "added"]
        assert len(added) == 2
        for _, k, b in added:
            assert set(b) == TODAYS_KEYS
        for b in res.list().values():
            assert set(b) - {"key"} == TODAYS_KEYS
        # weights and priorities differ on the next refresh
        nsc.set_srv(("b1.shop.test", 8080, 5, 1),
                    ("b2.shop.test", 8080, 0, 99))
        n_srv = nsc.count("SRV")
        await advance(loop, SRV_TTL)
        assert nsc.count("SRV") > n_srv
        assert [e for e in ev if e[0] in ("changed", "removed")] == []
        assert len([e for e in ev if e[0] == "added"]) == 2
        assert inner_ev == []
        assert "backend-changed" not in res.r_fsm.r_counters
        res.stop()
        await settle(loop)
    run_vt(body)


def test_option_on_carries_priority_and_weight():
    async def body(loop):
        res = make(loop, two_backend_zone(), srvRanking=True)
        ev = collect(res)
        res.start()
        await advance(loop, 1.0)
        got = by_name(e[2] for e in ev if e[0] == "added")
        assert (got["b1.shop.test"]["priority"],
                got["b1.shop.test"]["weight"]) == (0, 30)
        assert (got["b2.shop.test"]["priority"],
                got["b2.shop.test"]["weight"]) == (10, 5)
        for b in got.values():
            assert set(b) == TODAYS_KEYS | {"priority", "weight"}
            assert type(b["priority"]) is int and type(b["weight"]) is int
        listed = by_name(res.list().values())
        assert listed["b2.shop.test"]["priority"] == 10
        assert listed["b2.shop.test"]["weight"] == 5
        # rank is not part of a backend's identity
        for k, b in res.list().items():
            assert k == srv_key({"name": b["name"], "port": b["port"],
                                 "address": b["address"]})
        res.stop()
        await settle(loop)
    run_vt(body)


def test_plain_name_fallback_ranks_zero():
    async def body(loop):
        # no SRV records at all: NXDOMAIN on the SRV name
        nsc = ZoneClient()
        nsc.zone[("plain.test", "A")] = ["10.0.0.9"]
        res = make(loop, nsc, domain="plain.test", srvRanking=True)
        ev = collect(res)
        res.start()
        await advance(loop, 1.0)
        added = [e[2] for e in ev if e[0] == "added"]
        assert len(added) == 1
        assert added[0]["port"] == 80
        assert (added[0]["priority"], added[0]["weight"]) == (0, 0)
        res.stop()
        await settle(loop)
    run_vt(body)


def test_srv_error_fallback_ranks_zero():
    async def body(loop):
        class TimingOutSrv(ZoneClient):
            def lookup(self, opts, cb, loop=None):
                if opts["type"] == "SRV":
                    from cueball_amd.dns_client import TimeoutError_
                    self.history.append((opts["domain"], "SRV"))
                    loop.call_later(
                        opts["timeout"] / 1000.0,
                        lambda: cb(TimeoutError_(opts["domain"]), None))
                    return
                super().lookup(opts, cb, loop)

        nsc = TimingOutSrv()
        nsc.zone[("plain.test", "A")] = ["10.0.0.9"]
        res = make(loop, nsc, domain="plain.test", srvRanking=True)
        ev = collect(res)
        res.start()
        await advance(loop, 30.0)
        added = [e[2] for e in ev if e[0] == "added"]
        assert len(added) == 1
        assert (added[0]["priority"], added[0]["weight"]) == (0, 0)
        res.stop()
        await settle(loop)
    run_vt(body)


def test_duplicate_records_keep_best_rank():
    async def body(loop):
        nsc = ZoneClient()
        # four records, one backend: lowest priority wins, and among the
        # records at that priority the highest weight
        nsc.set_srv(("b1.shop.test", 8080, 10, 99),
                    ("b1.shop.test", 8080, 5, 3),
                    ("b1.shop.test", 8080, 5, 7),
                    ("b1.shop.test", 8080, 5, 4))
        nsc.zone[("b1.shop.test", "A")] = ["10.0.0.1"]
        res = make(loop, nsc, srvRanking=True)
        ev = collect(res)
        res.start()
        await advance(loop, 1.0)
        added = [e[2] for e in ev if e[0] == "added"]
        assert len(added) == 1
        assert (added[0]["priority"], added[0]["weight"]) == (5, 7)
        res.stop()
        await settle(loop)
    run_vt(body)


def test_weight_edit_emits_one_changed_and_keeps_address_cache():
    async def body(loop):
        nsc = two_backend_zone()
        res = make(loop, nsc, srvRanking=True)
        ev = collect(res)
        res.start()
        await advance(loop, 1.0)
        keys = {e[2]["name"]: e[1] for e in ev if e[0] == "added"}
        del ev[:]
        a_before = nsc.count("A")
        srv_before = nsc.count("SRV")

        nsc.set_srv(("b1.shop.test", 8080, 0, 30),
                    ("b2.shop.test", 8080, 10, 50))   # b2: weight 5 -> 50
        await advance(loop, SRV_TTL)
        assert nsc.count("SRV") == srv_before + 1
        # the cached A result of both targets was carried over
        assert nsc.count("A") == a_before
        assert [e[0] for e in ev] == ["changed", "updated"]
        _, k, b = ev[0]
        assert k == keys["b2.shop.test"]
        assert (b["priority"], b["weight"]) == (10, 50)
        assert b["address"] == "10.0.0.2"
        assert res.r_fsm.r_counters["backend-changed"] == 1
        assert by_name(res.list().values())["b2.shop.test"]["weight"] == 50

        # an unchanged refresh emits nothing but 'updated'
        del ev[:]
        await advance(loop, SRV_TTL)
        assert nsc.count("SRV") == srv_before + 2
        assert [e[0] for e in ev] == ["updated"]

        # a priority edit alongside an add and a remove: order is
        # removed, added, changed, updated
        del ev[:]
        nsc.set_srv(("b2.shop.test", 8080, 0, 50),
                    ("b3.shop.test", 8080, 0, 1))
        nsc.zone[("b3.shop.test", "A")] = ["10.0.0.3"]
        await advance(loop, SRV_TTL)
        assert [e[0] for e in ev] == ["removed", "added", "changed",
                                      "updated"]
        assert ev[0][1] == keys["b1.shop.test"]
        assert ev[2][1] == keys["b2.shop.test"]
        assert ev[2][2]["priority"] == 0
        res.stop()
        await settle(loop)
    run_vt(body)


def test_bootstrap_resolvers_ignore_ranking():
    async def body(loop):
        DNSResolverFSM._nic_cache = INT_NO_V6
        DNSResolverFSM._nic_cache_updated = loop.time() * 1000.0
        boot = DNSResolverFSM({
            "domain": "ns.test", "recovery": RECOVERY, "loop": loop,
            "_nsclient": ZoneClient(), "_isBootstrap": True,
            "srvRanking": True})
        assert boot.r_srv_ranking is False
    run_vt(body)


def test_static_resolver_rank_fields():
    async def body(loop):
        res = StaticIpResolver({"loop": loop, "backends": [
            {"address": "10.0.0.1", "port": 80, "priority": 0,
             "weight": 65535},
            {"address": "10.0.0.2", "port": 80, "priority": 10},
            {"address": "10.0.0.3", "port": 80},
        ]})
        ev = collect(res)
        res.start()
        await settle(loop)
        got = {e[2]["address"]: e[2] for e in ev if e[0] == "added"}
        assert got["10.0.0.1"] == {
            "name": "10.0.0.1:80", "address": "10.0.0.1", "port": 80,
            "priority": 0, "weight": 65535}
        assert got["10.0.0.2"] == {
            "name": "10.0.0.2:80", "address": "10.0.0.2", "port": 80,
            "priority": 10}
        # nothing given: exactly today's output
        assert got["10.0.0.3"] == {
            "name": "10.0.0.3:80", "address": "10.0.0.3", "port": 80}
        assert res.list()[srv_key(got["10.0.0.1"])]["weight"] == 65535
        res.stop()
        await settle(loop)
    run_vt(body)


@pytest.mark.parametrize("field", ["priority", "weight"])
def test_static_resolver_rank_validation(field):
    def mk(val):
        return StaticIpResolver({"backends": [
            {"address": "10.0.0.1", "port": 80, field: val}],
            "loop": asyncio.new_event_loop()})

    for bad in (-1, 65536):
        with pytest.raises(ValueError):
            mk(bad)
    for bad in ("1", 1.5, True):
        with pytest.raises(TypeError):
            mk(bad)


def test_wrapper_forwards_changed():
    async def body(loop):
        res = make(loop, two_backend_zone(), srvRanking=True)
        outer, inner = [], []
        res.on("changed", lambda k, b: outer.append((k, b)))
        res.r_fsm.on("changed", lambda k, b: inner.append((k, b)))
        res.r_fsm.emit("changed", "k1", {"weight": 3})
        assert outer == inner == [("k1", {"weight": 3})]
    run_vt(body)


def test_mock_dns_server_round_trip_over_udp():
    """Non-default priority and weight through dns_wire, the real
    DnsClient and the resolver, over UDP on loopback."""
    async def body():
        loop = asyncio.get_running_loop()
        srv = MockDnsServer()
        await srv.start()
        srv.add_srv("_svc._tcp.shop.test", "b1.shop.test", 8080,
                    priority=7, weight=300)
        srv.add_srv("_svc._tcp.shop.test", "b2.shop.test", 8081)
        srv.add_a("b1.shop.test", "127.0.0.21")
        srv.add_a("b2.shop.test", "127.0.0.22")
        DNSResolverFSM._nic_cache = INT_NO_V6
        DNSResolverFSM._nic_cache_updated = loop.time() * 1000.0
        res = DNSResolver({
            "domain": "shop.test", "service": "_svc._tcp",
            "resolvers": [srv.resolver_address], "recovery": RECOVERY,
            "srvRanking": True, "loop": loop})
        done = loop.create_future()
        res.on("stateChanged", lambda st: st in ("running", "failed")
               and not done.done() and done.set_result(st))
        res.start()
        try:
            assert await asyncio.wait_for(done, 10) == "running"
            got = by_name(res.list().values())
        finally:
            res.stop()
            srv.stop()
            await asyncio.sleep(0)
        return got

    loop = asyncio.new_event_loop()
    try:
        got = loop.run_until_complete(body())
    finally:
        loop.close()
    assert (got["b1.shop.test"]["priority"],
            got["b1.shop.test"]["weight"]) == (7, 300)
    # add_srv defaults are the constants it always used
    assert (got["b2.shop.test"]["priority"],
            got["b2.shop.test"]["weight"]) == (0, 10)


def test_cbresolve_rank_columns(capsys):
    assert cbresolve_main(["-S", "10.0.0.1:80"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert len(plain) == 1
    assert plain[0].split()[:2] == ["10.0.0.1", "80"]
    assert len(plain[0].split()) == 3

    assert cbresolve_main(["-w", "-S", "10.0.0.1:80"]) == 0
    ranked = capsys.readouterr().out.splitlines()
    assert len(ranked) == 1
    cols = ranked[0].split()
    # address port priority weight key
    assert cols[:4] == ["10.0.0.1", "80", "0", "0"]
    assert cols[4] == plain[0].split()[2]

    assert cbresolve_main(["--srv-ranking", "-S", "10.0.0.1:80"]) == 0
    assert capsys.readouterr().out.splitlines() == ranked


def test_cbresolve_rank_columns_from_dns():
    """bin/cbresolve -w prints the SRV record's priority and weight."""
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    async def body():
        srv = MockDnsServer()
        await srv.start()
        srv.add_srv("_web._tcp.shop.test", "s1.shop.test", 8443,
                    priority=20, weight=65535)
        srv.add_a("s1.shop.test", "10.9.8.7")
        try:
            outs = []
            for flags in (["-w"], []):
                proc = await asyncio.create_subprocess_exec(
                    sys.executable, os.path.join(root, "bin", "cbresolve"),
                    *flags, "-r", srv.resolver_address, "-s", "_web._tcp",
                    "-t", "5s", "shop.test",
                    stdout=asyncio.subprocess.PIPE,
                    stderr=asyncio.subprocess.PIPE, cwd=root)
                out, err = await asyncio.wait_for(proc.communicate(), 60)
                assert proc.returncode == 0, (out, err)
                outs.append(out.decode().split())
            return outs
        finally:
            srv.stop()

    loop = asyncio.new_event_loop()
    try:
        ranked, plain = loop.run_until_complete(body())
    finally:
        loop.close()
    assert ranked[:4] == ["10.9.8.7", "8443", "20", "65535"]
    assert plain[:2] == ["10.9.8.7", "8443"] and len(plain) == 3
    assert ranked[4] == plain[2]
