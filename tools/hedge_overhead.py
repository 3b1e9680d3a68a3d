#!/usr/bin/env python3
"""What does the ``hedge`` option cost a request, on and off?

The method and the scenario are those of ``tools/retry_overhead.py``,
whose comparison code this reuses.

**On against off, same build** (the default).  The agent scenario of
bench.py (8 loopback HTTP backends, spares 8, maximum 32, steps of 1000
concurrent GETs), once without the option and once with ``hedge: {}``
against these healthy backends, each run in a fresh child process,
order reversed every round.  No hedge is ever sent: with 1000 requests
in flight on 32 connections the adaptive delay sits at its ceiling
and a request that reaches it has no connection yet, so what is
measured is the driver, its timer and its histogram sample.  Prints one
line per run and a markdown summary.

    python tools/hedge_overhead.py --rounds 8 --steps 20 --warmup 2
    python tools/hedge_overhead.py --cprofile profiles/hedge_cprofile.txt

**Off against another tree** (``--against DIR``): the unchanged
``bench.py --config C`` of this tree and of the tree in DIR, the option
off in both; see retry_overhead.py.

    python tools/hedge_overhead.py --against ../parent --config headline
    python tools/hedge_overhead.py --against ../parent --config agent
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
from cueball_amd.agent import HttpAgent  # noqa: E402
from cueball_amd.testing import DummyResolver  # noqa: E402

BACKENDS, SPARES, MAXIMUM, CONCURRENCY = (
    retry_overhead.BACKENDS, retry_overhead.SPARES, retry_overhead.MAXIMUM,
    retry_overhead.CONCURRENCY)
HOST = retry_overhead.HOST


async def one_run(mode, steps, warmup, profile=None):
    loop = asyncio.get_running_loop()
    servers = []
    for _ in range(BACKENDS):
        srv = await loop.create_server(bench._FastHttpProtocol,
                                       "127.0.0.1", 0)
        servers.append((srv, srv.sockets[0].getsockname()[1]))
    resolver = DummyResolver()
    opts = {
        "defaultPort": servers[0][1],
        "recovery": {"default": {"timeout": 2000, "retries": 3,
                                 "delay": 100, "maxDelay": 2000}},
        "spares": SPARES, "maximum": MAXIMUM, "loop": loop,
    }
    if mode == "on":
        opts["hedge"] = {}
    agent = HttpAgent(opts)
    agent.create_pool(HOST, {"resolver": resolver})
    resolver.start()
    for i, (_, port) in enumerate(servers):
        resolver.add("b%d" % i, {"address": "127.0.0.1", "port": port,
                                 "name": "b%d" % i})
    pool = agent.get_pool(HOST)
    deadline = time.monotonic() + 15
    while pool.get_stats()["idleConnections"] < SPARES and \
            time.monotonic() < deadline:
        await asyncio.sleep(0.01)

    lat = []

    async def one_get(i):
        t0 = loop.time()
        resp = await agent.request_async(HOST, "GET", "/%d" % i)
        lat.append(loop.time() - t0)
        assert resp.status_code == 200

    async def step():
        await asyncio.gather(*[one_get(i) for i in range(CONCURRENCY)])

    for _ in range(warmup):
        await step()
    lat.clear()
    if profile is not None:
        profile.enable()
    t0 = time.perf_counter()
    for _ in range(steps):
        await step()
    t1 = time.perf_counter()
    if profile is not None:
        profile.disable()
    stats = agent.get_hedge_stats().get(HOST)
    counters = {} if stats is None else stats["counters"]
    out = {
        "mode": mode,
        "requests_per_s": round(steps * CONCURRENCY / (t1 - t0), 1),
        "lat_p50_ms": round(statistics.median(lat) * 1000, 4),
        "lat_p99_ms": round(statistics.quantiles(lat, n=100)[98] * 1000, 4),
        # proof that the on-run went through the driver, that its
        # timers were armed, and that no hedge was sent
        "driven": stats is not None,
        "delay_ms": None if stats is None else stats["delayMs"],
        "samples": 0 if stats is None else stats["samples"],
        "hedges": counters.get("hedge-sent", 0),
        "skipped": {k[len("hedge-skipped-"):]: v
                    for k, v in counters.items()
                    if k.startswith("hedge-skipped-") and v},
        "left_active": 0 if stats is None else stats["active"],
    }
    fut = loop.create_future()
    agent.stop(lambda e: fut.set_result(None))
    await fut
    for srv, _ in servers:
        srv.close()
    await asyncio.sleep(0.1)
    return out


def child(mode, steps, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", mode,
           "--steps", str(steps), "--warmup", str(warmup)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, check=True,
                         timeout=300)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one", choices=("off", "on"),
                    help="a single run in this process; prints one JSON "
                         "line")
    ap.add_argument("--cprofile", metavar="FILE",
                    help="profile the timed steps of one on-run into FILE")
    ap.add_argument("--against", metavar="DIR",
                    help="compare bench.py of this tree with the tree in "
                         "DIR, the option off in both")
    ap.add_argument("--config", default="headline",
                    choices=("headline", "agent"),
                    help="the bench.py scenario of --against")
    args = ap.parse_args()

    if args.one:
        print(json.dumps(asyncio.run(
            one_run(args.one, args.steps, args.warmup))))
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
        res = asyncio.run(one_run("on", args.steps, args.warmup, prof))
        buf = io.StringIO()
        buf.write("hedge: {} on, %d steps of %d GETs under cProfile: "
                  "%s\n\n" % (args.steps, CONCURRENCY, json.dumps(res)))
        # file names only: where the tree lives is nobody's business
        pstats.Stats(prof, stream=buf).strip_dirs().sort_stats(
            "tottime").print_stats(45)
        with open(args.cprofile, "w") as f:
            f.write(buf.getvalue())
        print(buf.getvalue())
        return

    rows = []
    for rnd in range(1, args.rounds + 1):
        order = ("off", "on") if rnd % 2 else ("on", "off")
        got = {}
        for mode in order:
            got[mode] = child(mode, args.steps, args.warmup)
            print(json.dumps(got[mode]), flush=True)
        rows.append((" ".join(order), got["off"], got["on"]))
    print()
    print(retry_overhead.summary(rows))


if __name__ == "__main__":
    main()
