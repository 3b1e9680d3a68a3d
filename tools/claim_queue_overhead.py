#!/usr/bin/env python3
"""What does a pool with ``claimQueue`` pay per claim?

bench.py measures pools with default options and is not to be told
otherwise, so this runs bench.py itself with one thing changed: every
pool it makes gets ``claimQueue: {"maxQueued": 64}`` (or the JSON given
with ``--claim-queue``).  All other arguments are bench.py's own, and
the result line it prints is bench.py's:

    python tools/claim_queue_overhead.py --gpus 1 --steps 20 --warmup 2
    python tools/claim_queue_overhead.py --claim-queue \\
        '{"maxQueued": 64, "priorities": 2}' --steps 20 --warmup 2

The option-off side of the comparison is the unchanged ``python bench.py``
with the same arguments, on this tree and on the parent's;
``profiles/claim_queue_overhead.md`` has the numbers and the order of
the runs.
"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

_ConnectionPool = bench.ConnectionPool


def main() -> None:
    claim_queue = {"maxQueued": 64}
    if "--claim-queue" in sys.argv:
        at = sys.argv.index("--claim-queue")
        claim_queue = json.loads(sys.argv[at + 1])
        del sys.argv[at:at + 2]

    def opted_in(options):
        options["claimQueue"] = dict(claim_queue)
        pool = _ConnectionPool(options)
        assert pool.get_queue_stats()["enabled"]
        return pool

    # bench.make_pool looks the class up in its module at call time
    bench.ConnectionPool = opted_in
    bench.main()


if __name__ == "__main__":
    main()
