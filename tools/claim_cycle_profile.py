#!/usr/bin/env python3
"""Where does a claim/release cycle of the headline benchmark spend?

Two measurements next to ``bench.py --config headline`` (8 backends,
spares 8, maximum 16, 16 concurrent claimers), both with bench.py's own
``ClaimDriver``:

**--cprofile**: the timed steps under cProfile, top functions by own
time, file names only (the format of profiles/claimpath_cprofile_r2.txt).
What it shows of the native core is one line per C entry point; its use
is to see which Python functions the core still calls back into.

**--floor**: the same driver against a stub pool that does no pool
work: ``claim()`` only queues the callback, one ``call_soon`` per loop
turn fires every queued callback with a stub handle whose ``release()``
does nothing.  What is left is the benchmark's own callback, the clock
reads and the event loop: the floor no change to the library can get
under.  Printed next to the real pool's cost in the same process, both
as CPU microseconds per claim.

``--tree DIR`` measures the tree in DIR (say a checkout of the parent
commit with its own build of the native core) instead of this one.

    python tools/claim_cycle_profile.py --floor
    python tools/claim_cycle_profile.py --cprofile --tree ../parent
"""

import argparse
import asyncio
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPARES, MAXIMUM, CONCURRENCY, CLAIMS_PER_STEP = 8, 16, 16, 20000


class _StubHandle:
    __slots__ = ()

    def release(self):
        pass


class StubPool:
    """claim() queues the callback; one call_soon per loop turn fires
    all that are queued."""

    def __init__(self, loop):
        self.loop = loop
        self.queue = []
        self.scheduled = False
        self.handle = _StubHandle()

    def claim(self, options, cb):
        self.queue.append(cb)
        if not self.scheduled:
            self.scheduled = True
            self.loop.call_soon(self._fire)

    def _fire(self):
        self.scheduled = False
        queue, self.queue = self.queue, []
        hdl = self.handle
        for cb in queue:
            cb(None, hdl, None)


async def timed_steps(bench, pool, steps, warmup, profile=None):
    loop = asyncio.get_running_loop()
    lat = []
    driver = bench.ClaimDriver(pool, loop, CONCURRENCY, lat)
    driver.record_lat = True
    for _ in range(warmup):
        await driver.run_step(CLAIMS_PER_STEP)
    lat.clear()
    if profile is not None:
        profile.enable()
    c0, w0 = time.process_time(), time.perf_counter()
    for _ in range(steps):
        await driver.run_step(CLAIMS_PER_STEP)
    c1, w1 = time.process_time(), time.perf_counter()
    if profile is not None:
        profile.disable()
    n = steps * CLAIMS_PER_STEP
    return {"claims": n,
            "cpu_us_per_claim": round((c1 - c0) / n * 1e6, 3),
            "wall_us_per_claim": round((w1 - w0) / n * 1e6, 3),
            "claims_per_s": round(n / (w1 - w0), 1)}


async def run(bench, args, profile=None):
    loop = asyncio.get_running_loop()
    out = {}
    if args.floor:
        out["stub_pool"] = await timed_steps(
            bench, StubPool(loop), args.steps, args.warmup)
    backends = await bench.start_backends(8)
    pool = bench.make_pool(backends, spares=SPARES, maximum=MAXIMUM,
                           loop=loop)
    await bench.wait_for_idle(pool, 8)
    out["real_pool"] = await timed_steps(bench, pool, args.steps,
                                         args.warmup, profile)
    pool.stop()
    for srv, _ in backends:
        srv.close()
    await asyncio.sleep(0.1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=ROOT,
                    help="the tree to measure (default: this one)")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--floor", action="store_true")
    ap.add_argument("--cprofile", action="store_true")
    ap.add_argument("--top", type=int, default=25)
    args = ap.parse_args()

    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import bench
    assert os.path.dirname(os.path.abspath(bench.__file__)) == tree

    profile = None
    if args.cprofile:
        import cProfile
        profile = cProfile.Profile()
    out = asyncio.run(run(bench, args, profile))
    print(json.dumps(out))
    if profile is not None:
        import pstats
        buf = io.StringIO()
        pstats.Stats(profile, stream=buf).strip_dirs().sort_stats(
            "tottime").print_stats(args.top)
        print(buf.getvalue())


if __name__ == "__main__":
    main()
