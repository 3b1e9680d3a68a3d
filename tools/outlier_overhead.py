#!/usr/bin/env python3
"""What does ``outlierDetection`` cost the claim path when it is on?

bench.py measures pools with default options and is not to be told
otherwise, so this runs the same thing next to it: the headline
scenario's claim/release loop (8 loopback echo backends, spares 8,
maximum 16, 16 concurrent claimers, 20000 claims per step; the driver
and the backends are bench.py's own), once with the option off and once
with it on, each run in a fresh child process, order reversed every
round.  Prints one line per run and a markdown summary.

    python tools/outlier_overhead.py --rounds 6 --steps 20 --warmup 2
    python tools/outlier_overhead.py --cprofile profiles/outlier_cprofile.txt
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
from cueball_amd.connection import tcp_constructor  # noqa: E402
from cueball_amd.pool import ConnectionPool  # noqa: E402
from cueball_amd.resolver import StaticIpResolver  # noqa: E402

SPARES, MAXIMUM, CONCURRENCY, CLAIMS_PER_STEP = 8, 16, 16, 20000


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
    if mode == "on":
        opts["outlierDetection"] = {}
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
    stats = pool.get_outlier_stats()
    out = {
        "mode": mode,
        "claims_per_s": round(ops / (t1 - t0), 1),
        "lat_p50_ms": round(statistics.median(lat) * 1000, 4),
        "lat_p99_ms": round(statistics.quantiles(lat, n=100)[98] * 1000, 4),
        "failed": len(driver.failed),
        # proof that the on-run watched its leases
        "successes": sum(b["successes"]
                         for b in stats["backends"].values()),
    }
    pool.stop()
    for srv, _ in backends:
        srv.close()
    await asyncio.sleep(0.1)
    return out


def child(mode, steps, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", mode,
           "--steps", str(steps), "--warmup", str(warmup)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, check=True,
                         timeout=300)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def summary(rows):
    lines = ["| round | order | off | on |", "|---|---|---|---|"]
    for i, (order, off, on) in enumerate(rows, 1):
        lines.append("| %d | %s | %.1f | %.1f |" % (
            i, order, off["claims_per_s"], on["claims_per_s"]))
    lines += ["", "| | off | on |", "|---|---|---|"]
    cols = [[r[1] for r in rows], [r[2] for r in rows]]

    def row(title, fn):
        lines.append("| %s | %s | %s |" % (title, fn(cols[0]), fn(cols[1])))

    row("median claims/s", lambda c: "%.1f" % statistics.median(
        x["claims_per_s"] for x in c))
    row("min .. max", lambda c: "%.1f .. %.1f" % (
        min(x["claims_per_s"] for x in c),
        max(x["claims_per_s"] for x in c)))
    row("median claim latency p50, ms", lambda c: "%.4f" % statistics.median(
        x["lat_p50_ms"] for x in c))
    row("median claim latency p99, ms", lambda c: "%.4f" % statistics.median(
        x["lat_p99_ms"] for x in c))
    return "\n".join(lines)


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
    args = ap.parse_args()

    if args.one:
        print(json.dumps(asyncio.run(
            one_run(args.one, args.steps, args.warmup))))
        return
    if args.cprofile:
        import cProfile
        import io
        import pstats
        prof = cProfile.Profile()
        res = asyncio.run(one_run("on", args.steps, args.warmup, prof))
        buf = io.StringIO()
        buf.write("outlierDetection on, %d steps of %d claims under "
                  "cProfile: %s\n\n" % (args.steps, CLAIMS_PER_STEP,
                                        json.dumps(res)))
        pstats.Stats(prof, stream=buf).sort_stats("tottime").print_stats(30)
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
