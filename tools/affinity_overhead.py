#!/usr/bin/env python3
"""What does a claim with ``affinityKey`` cost?

A pool of fake connections on 8 backends, two idle connections each,
``claimAffinity: {}``; one claim at a time (claim, release from the
callback, claim again), in four ways, each in a fresh child process, the
order rotated every round:

- ``plain``: ``claim({}, cb)``, the runtime's own fast path;
- ``avoid``: ``avoidBackends`` naming one backend.  The path existed
  before key affinity and uses the same Python-ticket mechanism: the fair
  comparison;
- ``key``: ``affinityKey``, a 16-byte key out of 64, on the hash and
  rank the runtime has loaded (the native ones, where the native core
  is built);
- ``key-pure``: the same with ``cueball_amd.affinity``'s Python hash
  and rank put in place of the native ones, everything else unchanged.

    python tools/affinity_overhead.py --rounds 5 --claims 50000

Prints one JSON line per run and a markdown summary.  The option-off
side, a pool without ``claimAffinity`` against the parent commit, is
the unchanged ``python bench.py`` on both trees;
``profiles/claim_affinity_overhead.md`` has the numbers.
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

MODES = ("plain", "avoid", "key", "key-pure")
BACKENDS, PER = 8, 2
KEYS = [b"tenant-%09d" % i for i in range(64)]


async def one_run(mode, claims):
    from cueball_amd import affinity
    from cueball_amd.pool import ConnectionPool
    from cueball_amd.resolver import ResolverFSM
    from cueball_amd.testing import DummyConnection, DummyResolver
    if mode == "key-pure":
        affinity.fnv1a64 = affinity.PurePythonFnv1a64
        affinity.rank = affinity.PurePythonRank
    loop = asyncio.get_running_loop()
    resolver = DummyResolver()
    rfsm = ResolverFSM(resolver, {"loop": loop})

    def constructor(backend):
        c = DummyConnection(backend)
        loop.call_soon(c.connect)
        return c

    idle = BACKENDS * PER
    pool = ConnectionPool({
        "domain": "affinity.local", "constructor": constructor,
        "resolver": rfsm, "spares": idle, "maximum": idle, "loop": loop,
        "claimAffinity": {},
        "recovery": {"default": {"timeout": 2000, "retries": 3,
                                 "delay": 100, "maxDelay": 2000}}})
    rfsm.start()
    for i in range(BACKENDS):
        resolver.add("b%d" % i, {"address": "10.0.0.%d" % i, "port": 80})
    while pool.get_stats()["idleConnections"] < idle:
        await asyncio.sleep(0.01)

    if mode == "plain":
        options = [{}]
    elif mode == "avoid":
        options = [{"avoidBackends": ["b%d" % (i % BACKENDS)]}
                   for i in range(len(KEYS))]
    else:
        options = [{"affinityKey": k} for k in KEYS]
    assert len(KEYS[0]) == 16

    async def serial(n):
        done = loop.create_future()
        left = [n]

        def cb(err, hdl=None, conn=None):
            assert err is None, err
            hdl.release()
            left[0] -= 1
            if left[0]:
                pool.claim(options[left[0] % len(options)], cb)
            else:
                done.set_result(None)

        pool.claim(options[0], cb)
        await done

    await serial(claims // 10)
    t0 = time.perf_counter()
    await serial(claims)
    t1 = time.perf_counter()
    counters = pool.get_stats()["counters"]
    out = {"mode": mode,
           "native_hash": affinity.fnv1a64 is not affinity.PurePythonFnv1a64,
           "claims_per_s": round(claims / (t1 - t0), 1),
           "us_per_claim": round((t1 - t0) / claims * 1e6, 3),
           # proof of which path the run took
           "keyed": counters.get("affinity-claim", 0),
           "hits": counters.get("affinity-hit", 0),
           "queued": counters.get("queued-claim", 0)}
    pool.stop()
    await asyncio.sleep(0.1)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--claims", type=int, default=50000)
    ap.add_argument("--one", choices=MODES)
    args = ap.parse_args()
    if args.one:
        print(json.dumps(asyncio.run(one_run(args.one, args.claims))))
        return
    runs = {m: [] for m in MODES}
    for rnd in range(args.rounds):
        k = rnd % len(MODES)
        for mode in MODES[k:] + MODES[:k]:
            res = subprocess.run(
                [sys.executable, os.path.abspath(__file__), "--one", mode,
                 "--claims", str(args.claims)],
                stdout=subprocess.PIPE, check=True, timeout=300)
            got = json.loads(res.stdout.decode().strip().splitlines()[-1])
            print(json.dumps(got), flush=True)
            runs[mode].append(got)
    print("\n| mode | median claims/s | min .. max | median us per claim |")
    print("|---|---|---|---|")
    for mode in MODES:
        cps = [r["claims_per_s"] for r in runs[mode]]
        print("| %s | %.1f | %.1f .. %.1f | %.3f |" % (
            mode, statistics.median(cps), min(cps), max(cps),
            statistics.median(r["us_per_claim"] for r in runs[mode])))


if __name__ == "__main__":
    main()
