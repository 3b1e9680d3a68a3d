#!/usr/bin/env python3
"""What does ``claimBalancing`` cost the claim path, on and off?

**On against off, same build** (the default).  bench.py measures pools
with default options and is not to be told otherwise, so this runs the
same thing next to it: the headline scenario's claim/release loop (8
loopback echo backends, spares 8, maximum 16, 16 concurrent claimers,
20000 claims per step; the driver and the backends are bench.py's own),
without the option (``off``), with ``claimBalancing: {}`` (``two``: two
random choices) and with ``{"choices": "all"}`` (``all``), each run in a
fresh child process, the order rotated every round.  Prints one line per
run and a markdown summary.

    python tools/balance_overhead.py --rounds 8 --steps 20 --warmup 2
    python tools/balance_overhead.py --cprofile profiles/balance_cprofile.txt

**The walk** (``--walk``).  The headline loop keeps every connection
busy, so a claim seldom finds more than one idle slot to choose from.
This is the other end: a pool of fake connections on 8 backends with N
of them idle, one claim at a time (claim, release from the callback,
claim again), so that every claim walks N idle slots; N = 8, 32, 128,
each mode in a fresh process.

    python tools/balance_overhead.py --walk

**Off against another tree** (``--against DIR``): the unchanged
``bench.py --config C`` of this tree and of the tree in DIR, the option
off in both; see retry_overhead.py.

    python tools/balance_overhead.py --against ../parent --config headline
    python tools/balance_overhead.py --against ../parent --config agent
"""

import argparse
import asyncio
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402
import retry_overhead  # noqa: E402
from cueball_amd.connection import tcp_constructor  # noqa: E402
from cueball_amd.pool import ConnectionPool  # noqa: E402
from cueball_amd.resolver import StaticIpResolver  # noqa: E402

SPARES, MAXIMUM, CONCURRENCY, CLAIMS_PER_STEP = 8, 16, 16, 20000
MODES = {"off": None, "two": {}, "all": {"choices": "all"}}


async def one_run(mode, steps, warmup, profile=None):
    loop = asyncio.get_running_loop()
    backends = await bench.start_backends(8)
    resolver = StaticIpResolver({
        "backends": [{"address": "127.0.0.1", "port": p}
                     for (_, p) in backends],
        "loop": loop})
    opts = {
        "domain": "bench.local",
        "constructor": tcp_constructor(loop=loop),
        "resolver": resolver,
        "recovery": {"default": {"timeout": 2000, "retries": 3,
                                 "delay": 100, "maxDelay": 2000}},
        "spares": SPARES, "maximum": MAXIMUM, "loop": loop,
    }
    if MODES[mode] is not None:
        opts["claimBalancing"] = dict(MODES[mode])
    pool = ConnectionPool(opts)
    resolver.start()
    await bench.wait_for_idle(pool, SPARES)

    lat = []
    driver = bench.ClaimDriver(pool, loop, CONCURRENCY, lat)
    for _ in range(warmup):
        await driver.run_step(CLAIMS_PER_STEP)
    lat.clear()
    if profile is not None:
        profile.enable()
    t0 = time.perf_counter()
    for _ in range(steps):
        await driver.run_step(CLAIMS_PER_STEP)
    t1 = time.perf_counter()
    if profile is not None:
        profile.disable()
    ops = steps * CLAIMS_PER_STEP
    stats = pool.get_balancing_stats()
    counters = pool.get_stats()["counters"]
    out = {
        "mode": mode,
        "claims_per_s": round(ops / (t1 - t0), 1),
        "us_per_claim": round((t1 - t0) / ops * 1e6, 3),
        "lat_p50_ms": round(statistics.median(lat) * 1000, 4),
        "lat_p99_ms": round(statistics.quantiles(lat, n=100)[98] * 1000, 4),
        "failed": len(driver.failed),
        # proof of which path the run took: claims the balancer placed,
        # claims that queued, leases it timed
        "balanced": counters.get("balanced-claim", 0),
        "reordered": counters.get("balanced-reordered", 0),
        "queued": counters.get("queued-claim", 0),
        "leases": sum(b["leases"] for b in
                      stats.get("backends", {}).values()),
    }
    pool.stop()
    for srv, _ in backends:
        srv.close()
    await asyncio.sleep(0.1)
    return out


async def walk_run(mode, idle, claims):
    """Serial claim/release on a pool with `idle` idle fake connections."""
    from cueball_amd.resolver import ResolverFSM
    from cueball_amd.testing import DummyConnection, DummyResolver
    loop = asyncio.get_running_loop()
    resolver = DummyResolver()
    rfsm = ResolverFSM(resolver, {"loop": loop})

    def constructor(backend):
        c = DummyConnection(backend)
        loop.call_soon(c.connect)
        return c

    opts = {"domain": "walk.local", "constructor": constructor,
            "resolver": rfsm, "spares": idle, "maximum": idle, "loop": loop,
            "recovery": {"default": {"timeout": 2000, "retries": 3,
                                     "delay": 100, "maxDelay": 2000}}}
    if MODES[mode] is not None:
        opts["claimBalancing"] = dict(MODES[mode])
    pool = ConnectionPool(opts)
    rfsm.start()
    for i in range(8):
        resolver.add("b%d" % i, {"address": "10.0.0.%d" % i, "port": 80})
    await bench.wait_for_idle(pool, idle)

    async def serial(n):
        done = loop.create_future()
        left = [n]

        def cb(err, hdl=None, conn=None):
            assert err is None, err
            hdl.release()
            left[0] -= 1
            if left[0]:
                pool.claim({}, cb)
            else:
                done.set_result(None)

        pool.claim({}, cb)
        await done

    await serial(claims // 10)
    t0 = time.perf_counter()
    await serial(claims)
    t1 = time.perf_counter()
    counters = pool.get_stats()["counters"]
    out = {"mode": mode, "idle": idle,
           "us_per_claim": round((t1 - t0) / claims * 1e6, 3),
           "balanced": counters.get("balanced-claim", 0),
           "queued": counters.get("queued-claim", 0)}
    pool.stop()
    await asyncio.sleep(0.1)
    return out


def walk(claims):
    sizes = (8, 32, 128)
    table = {}
    for idle in sizes:
        for mode in MODES:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", mode,
                   "--walk-idle", str(idle), "--walk-claims", str(claims)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, check=True,
                                 timeout=300)
            got = json.loads(res.stdout.decode().strip().splitlines()[-1])
            print(json.dumps(got), flush=True)
            table[(idle, mode)] = got["us_per_claim"]
    lines = ["", "us per serial claim/release, %d claims:" % claims, "",
             "| idle connections | %s |" % " | ".join(MODES),
             "|---|%s" % ("---|" * len(MODES))]
    for idle in sizes:
        lines.append("| %d | %s |" % (idle, " | ".join(
            "%.3f" % table[(idle, m)] for m in MODES)))
    print("\n".join(lines))


def child(mode, steps, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", mode,
           "--steps", str(steps), "--warmup", str(warmup)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, check=True,
                         timeout=300)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def summary(rows):
    modes = list(MODES)
    lines = ["| round | order | %s |" % " | ".join(modes),
             "|---|---|%s" % ("---|" * len(modes))]
    for i, (order, got) in enumerate(rows, 1):
        lines.append("| %d | %s | %s |" % (i, order, " | ".join(
            "%.1f" % got[m]["claims_per_s"] for m in modes)))
    lines += ["", "| | %s |" % " | ".join(modes),
              "|---|%s" % ("---|" * len(modes))]
    cols = {m: [got[m] for _, got in rows] for m in modes}

    def row(title, fn):
        lines.append("| %s | %s |" % (
            title, " | ".join(fn(cols[m]) for m in modes)))

    def med(c, field):
        return statistics.median(x[field] for x in c)

    off = med(cols["off"], "claims_per_s")
    row("median claims/s", lambda c: "%.1f" % med(c, "claims_per_s"))
    row("min .. max", lambda c: "%.1f .. %.1f" % (
        min(x["claims_per_s"] for x in c),
        max(x["claims_per_s"] for x in c)))
    row("ratio to off", lambda c: "%.3f" % (med(c, "claims_per_s") / off))
    row("median us per claim", lambda c: "%.3f" % med(c, "us_per_claim"))
    row("median claim latency p50, ms",
        lambda c: "%.4f" % med(c, "lat_p50_ms"))
    row("median claim latency p99, ms",
        lambda c: "%.4f" % med(c, "lat_p99_ms"))
    row("claims queued, median", lambda c: "%d" % med(c, "queued"))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one", choices=tuple(MODES),
                    help="a single run in this process; prints one JSON "
                         "line")
    ap.add_argument("--cprofile", metavar="FILE",
                    help="profile the timed steps of one run into FILE")
    ap.add_argument("--cprofile-mode", default="all",
                    choices=("two", "all"),
                    help="the mode --cprofile runs")
    ap.add_argument("--walk", action="store_true",
                    help="serial claims on pools with 8, 32 and 128 idle "
                         "fake connections")
    ap.add_argument("--walk-idle", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--walk-claims", type=int, default=50000)
    ap.add_argument("--against", metavar="DIR",
                    help="compare bench.py of this tree with the tree in "
                         "DIR, the option off in both")
    ap.add_argument("--config", default="headline",
                    choices=("headline", "agent"),
                    help="the bench.py scenario of --against")
    args = ap.parse_args()

    if args.one and args.walk_idle:
        print(json.dumps(asyncio.run(
            walk_run(args.one, args.walk_idle, args.walk_claims))))
        return
    if args.one:
        print(json.dumps(asyncio.run(
            one_run(args.one, args.steps, args.warmup))))
        return
    if args.walk:
        walk(args.walk_claims)
        return
    if args.against:
        retry_overhead.against(args.against, args.config, args.rounds,
                               args.steps, args.warmup)
        return
    if args.cprofile:
        import cProfile
        import io
        import pstats
        prof = cProfile.Profile()
        mode = args.cprofile_mode
        res = asyncio.run(one_run(mode, args.steps, args.warmup, prof))
        buf = io.StringIO()
        buf.write("claimBalancing %r, %d steps of %d claims under "
                  "cProfile: %s\n\n" % (MODES[mode], args.steps,
                                        CLAIMS_PER_STEP, json.dumps(res)))
        # file names only: where the tree lives is nobody's business
        pstats.Stats(prof, stream=buf).strip_dirs().sort_stats(
            "tottime").print_stats(30)
        with open(args.cprofile, "w") as f:
            f.write(buf.getvalue())
        print(buf.getvalue())
        return

    modes = list(MODES)
    rows = []
    for rnd in range(args.rounds):
        order = modes[rnd % len(modes):] + modes[:rnd % len(modes)]
        if rnd % 2:
            order.reverse()
        got = {}
        for mode in order:
            got[mode] = child(mode, args.steps, args.warmup)
            print(json.dumps(got[mode]), flush=True)
        rows.append((" ".join(order), got))
    print()
    print(summary(rows))


if __name__ == "__main__":
    main()
