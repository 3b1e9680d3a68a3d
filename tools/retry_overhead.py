#!/usr/bin/env python3
"""What does the ``retry`` option cost a request, on and off?

Two questions, two modes.

**On against off, same build** (the default).  bench.py measures agents
with default options and is not to be told otherwise, so this runs the
same thing next to it: the agent scenario (8 loopback HTTP backends,
spares 8, maximum 32, steps of 1000 concurrent GETs; the backends are
bench.py's own), once without the option and once with ``retry: {}``
against these healthy backends, each run in a fresh child process,
order reversed every round.  Prints one line per run and a markdown
summary.

    python tools/retry_overhead.py --rounds 6 --steps 20 --warmup 2
    python tools/retry_overhead.py --cprofile profiles/retry_cprofile.txt

**Off against another tree** (``--against DIR``).  Runs the unchanged
``bench.py --config C`` of this tree and of the tree in DIR (say a
checkout of the parent commit with its own build of the native core) in
fresh processes, the option off in both: per round the other tree
twice and this tree once, order reversed every round, so that the
other tree's spread against itself is measured in the same session.

    python tools/retry_overhead.py --against ../parent --config headline
    python tools/retry_overhead.py --against ../parent --config agent
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

import bench  # noqa: E402
from cueball_amd.agent import HttpAgent  # noqa: E402
from cueball_amd.testing import DummyResolver  # noqa: E402

BACKENDS, SPARES, MAXIMUM, CONCURRENCY = 8, 8, 32, 1000
HOST = "svc.bench"


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
        opts["retry"] = {}
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
    stats = agent.get_retry_stats().get(HOST)
    out = {
        "mode": mode,
        "requests_per_s": round(steps * CONCURRENCY / (t1 - t0), 1),
        "lat_p50_ms": round(statistics.median(lat) * 1000, 4),
        "lat_p99_ms": round(statistics.quantiles(lat, n=100)[98] * 1000, 4),
        # proof that the on-run went through the driver, and that
        # nothing was retried
        "driven": stats is not None,
        "retries": 0 if stats is None else sum(
            v for k, v in stats["counters"].items()
            if k.startswith("retry-")),
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


def med(values):
    return statistics.median(values)


def summary(rows):
    lines = ["| round | order | off | on |", "|---|---|---|---|"]
    for i, (order, off, on) in enumerate(rows, 1):
        lines.append("| %d | %s | %.1f | %.1f |" % (
            i, order, off["requests_per_s"], on["requests_per_s"]))
    lines += ["", "| | off | on |", "|---|---|---|"]
    cols = [[r[1] for r in rows], [r[2] for r in rows]]

    def row(title, fn):
        lines.append("| %s | %s | %s |" % (title, fn(cols[0]), fn(cols[1])))

    row("median requests/s", lambda c: "%.1f" % med(
        [x["requests_per_s"] for x in c]))
    row("min .. max", lambda c: "%.1f .. %.1f" % (
        min(x["requests_per_s"] for x in c),
        max(x["requests_per_s"] for x in c)))
    row("median request latency p50, ms", lambda c: "%.4f" % med(
        [x["lat_p50_ms"] for x in c]))
    row("median request latency p99, ms", lambda c: "%.4f" % med(
        [x["lat_p99_ms"] for x in c]))
    off = med([x["requests_per_s"] for x in cols[0]])
    on = med([x["requests_per_s"] for x in cols[1]])
    lines += ["", "on / off, median requests/s: %.3f" % (on / off)]
    return "\n".join(lines)


def bench_child(tree, config, steps, warmup):
    """One ``bench.py --config`` run of `tree` in a fresh process."""
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1",
           "--steps", str(steps), "--warmup", str(warmup),
           "--config", config]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, check=True,
                         timeout=600, cwd=tree)
    out = json.loads(res.stdout.decode().strip().splitlines()[-1])
    return {"value": out["value"],
            "p50": out["config"]["claim_latency_p50_ms"],
            "p99": out["config"]["claim_latency_p99_ms"]}


def against(other, config, rounds, steps, warmup):
    """Rounds of (other, this, other), order reversed every round."""
    other = os.path.abspath(other)
    rows = []
    for rnd in range(1, rounds + 1):
        order = ("P1", "B", "P2") if rnd % 2 else ("P2", "B", "P1")
        got = {}
        for which in order:
            tree = ROOT if which == "B" else other
            got[which] = bench_child(tree, config, steps, warmup)
            print(json.dumps(dict(got[which], tree=which, round=rnd,
                                  config=config)), flush=True)
        rows.append((" ".join(order), got))
    lines = ["", "`bench.py --config %s --steps %d --warmup %d`; P1 and P2 "
             "are the two runs of the other tree, B is this tree."
             % (config, steps, warmup), "",
             "| round | order | P1 | B | P2 |", "|---|---|---|---|---|"]
    for i, (order, got) in enumerate(rows, 1):
        lines.append("| %d | %s | %.1f | %.1f | %.1f |" % (
            i, order, got["P1"]["value"], got["B"]["value"],
            got["P2"]["value"]))
    parent = [g[w]["value"] for _, g in rows for w in ("P1", "P2")]
    branch = [g["B"]["value"] for _, g in rows]
    lo, hi, bmed = min(parent), max(parent), med(branch)
    lines += [
        "", "| | other tree (P1 and P2) | this tree |", "|---|---|---|",
        "| runs | %d | %d |" % (len(parent), len(branch)),
        "| median | %.1f | %.1f |" % (med(parent), bmed),
        "| min .. max | %.1f .. %.1f | %.1f .. %.1f |" % (
            lo, hi, min(branch), max(branch)),
        "| median latency p50, ms | %.4f | %.4f |" % (
            med([g[w]["p50"] for _, g in rows for w in ("P1", "P2")]),
            med([g["B"]["p50"] for _, g in rows])),
        "", "Criterion: this tree's median inside the other tree's own "
        "min .. max: %.1f <= %.1f <= %.1f: **%s** (this tree's median is "
        "%+.1f %% against the other's)." % (
            lo, bmed, hi, "met" if lo <= bmed <= hi else "not met",
            (bmed / med(parent) - 1.0) * 100.0)]
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=6)
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
                    choices=("headline", "static1", "codel", "agent"),
                    help="the bench.py scenario of --against")
    args = ap.parse_args()

    if args.one:
        print(json.dumps(asyncio.run(
            one_run(args.one, args.steps, args.warmup))))
        return
    if args.against:
        against(args.against, args.config, args.rounds, args.steps,
                args.warmup)
        return
    if args.cprofile:
        import cProfile
        import io
        import pstats
        prof = cProfile.Profile()
        res = asyncio.run(one_run("on", args.steps, args.warmup, prof))
        buf = io.StringIO()
        buf.write("retry: {} on, %d steps of %d GETs under cProfile: "
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
    print(summary(rows))


if __name__ == "__main__":
    main()
