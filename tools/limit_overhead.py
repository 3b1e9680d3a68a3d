#!/usr/bin/env python3
"""What does a pool with ``concurrencyLimit`` pay per claim?

bench.py measures pools with default options and is not to be told
otherwise, so this runs bench.py itself with one thing changed: every
pool it makes gets ``concurrencyLimit: {"algorithm": "aimd",
"latencyThreshold": 1e9}`` (or the JSON given with
``--concurrency-limit``): a limit that stays at the pool's ``maximum``
and never holds a claim, so that what is measured is the bookkeeping
(a Python ticket and a Python slot listener per lease in place of the
native ones, a start and a sample per lease), not a throttle.  All other
arguments are bench.py's own, and the result line it prints is
bench.py's:

    python tools/limit_overhead.py --gpus 1 --steps 10 --warmup 2
    python tools/limit_overhead.py --concurrency-limit '{}' --steps 10

The option-off side of the comparison is the unchanged ``python bench.py``
with the same arguments, on this tree and on the parent's;
``profiles/limit_overhead.md`` has the numbers and the order of the
runs.  The figure is recorded, not asserted.
"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

_ConnectionPool = bench.ConnectionPool


def main() -> None:
    limit = {"algorithm": "aimd", "latencyThreshold": 1e9}
    if "--concurrency-limit" in sys.argv:
        at = sys.argv.index("--concurrency-limit")
        limit = json.loads(sys.argv[at + 1])
        del sys.argv[at:at + 2]

    def opted_in(options):
        options["concurrencyLimit"] = dict(limit)
        pool = _ConnectionPool(options)
        assert pool.get_limit_stats()["enabled"]
        return pool

    # bench.make_pool looks the class up in its module at call time
    bench.ConnectionPool = opted_in
    bench.main()


if __name__ == "__main__":
    main()
