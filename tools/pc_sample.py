#!/usr/bin/env python3
"""Which functions of the native core does a claim/release cycle spend in?

A per-function profile of the uninstrumented build on a host without
``perf``.  The C source beside this file (pc_sample.c) is compiled with
the system compiler into a temporary directory and loaded with ctypes;
its SIGALRM handler samples the program counter of the timed loop of
bench.py's own ``ClaimDriver``, with the arguments of ``bench.py
--config C``.  A sample inside ``_speed`` is charged to its function
("self"); one outside it that has a return address into ``_speed`` among
the top stack words is charged to that function as "called": the
interpreter, libc and the vdso, called shallowly from the core (the
benchmark's own callback runs inside the ``claimed`` entry and is in
there).  Function names come from ``nm``; inlined functions count for
the function they were inlined into.

The "self" column is exact.  The "called" column is a guess: the first
stack word that points into the core's code can be a return address that
an earlier, deeper call left behind in a slot the current frames never
wrote.  A function that makes a short call out just before a long one is
made from the same depth (``emitter_leak_counts`` before the claim
callback) is charged with the long one.  Read "called" as "in or below
the core", and its split by function with that in mind.

    python tools/pc_sample.py --config headline
    python tools/pc_sample.py --config static1 --tree ../parent --top 40

It samples the host CPU only.
"""

import argparse
import asyncio
import bisect
import collections
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

#: bench.py's arguments per scenario: backends, spares, maximum, claimers
CONFIGS = {
    "headline": (8, 8, 16, 16),
    "static1": (1, 1, 2, 1),
}
CLAIMS_PER_STEP = 20000


def build_sampler(tmpdir):
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        raise SystemExit("pc_sample: no C compiler (cc, gcc or $CC)")
    lib = os.path.join(tmpdir, "pc_sample.so")
    subprocess.check_call([cc, "-O2", "-shared", "-fPIC", "-o", lib,
                           os.path.join(HERE, "pc_sample.c"), "-lpthread"])
    dll = ctypes.CDLL(lib)
    dll.pcs_start.argtypes = [ctypes.c_int, ctypes.c_uint64,
                              ctypes.c_uint64, ctypes.c_long]
    dll.pcs_start.restype = ctypes.c_int
    dll.pcs_stop.restype = ctypes.c_long
    dll.pcs_missed.restype = ctypes.c_long
    dll.pcs_pcs.restype = ctypes.POINTER(ctypes.c_uint64)
    dll.pcs_vias.restype = ctypes.POINTER(ctypes.c_uint64)
    return dll


def mapped_range(path):
    """(load base, lowest, highest address of the executable mappings) of
    the object `path` in this process.  Its data is left out: a stack
    word that points at one of its type objects is no return address."""
    real = os.path.realpath(path)
    lo = hi = base = None
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split()
            if len(parts) < 6 or os.path.realpath(parts[5]) != real:
                continue
            a, b = (int(x, 16) for x in parts[0].split("-"))
            if int(parts[2], 16) == 0 and base is None:
                base = a
            if "x" not in parts[1]:
                continue
            lo = a if lo is None else min(lo, a)
            hi = b if hi is None else max(hi, b)
    if lo is None:
        raise SystemExit("pc_sample: %s is not mapped" % path)
    return (lo if base is None else base), lo, hi


def text_symbols(path):
    """Sorted [(address, name)] of the functions of `path`."""
    out = subprocess.run(["nm", "-C", "--defined-only", path],
                         stdout=subprocess.PIPE, check=True)
    syms = []
    for line in out.stdout.decode(errors="replace").splitlines():
        parts = line.split(None, 2)
        if len(parts) == 3 and parts[1] in "tTwW":
            name = parts[2].replace("(anonymous namespace)::", "")
            syms.append((int(parts[0], 16), name.split("(")[0]))
    syms.sort()
    return syms


def symbol_of(syms, addrs, off):
    i = bisect.bisect_right(addrs, off) - 1
    return syms[i][1] if i >= 0 else "?"


async def sampled_steps(bench, dll, rng, cfg, steps, warmup, hz):
    n_backends, spares, maximum, claimers = cfg
    loop = asyncio.get_running_loop()
    backends = await bench.start_backends(n_backends)
    pool = bench.make_pool(backends, spares=spares, maximum=maximum,
                           loop=loop)
    await bench.wait_for_idle(pool, min(spares, n_backends))
    lat = []
    driver = bench.ClaimDriver(pool, loop, claimers, lat)
    for _ in range(warmup):
        await driver.run_step(CLAIMS_PER_STEP)
    lat.clear()
    cap = hz * 600              # ten minutes' worth
    if dll.pcs_start(hz, rng[1], rng[2], cap) != 0:
        raise SystemExit("pc_sample: could not start the timer")
    try:
        for _ in range(steps):
            await driver.run_step(CLAIMS_PER_STEP)
    finally:
        n = dll.pcs_stop()
    pool.stop()
    for srv, _ in backends:
        srv.close()
    await asyncio.sleep(0.1)
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="headline", choices=sorted(CONFIGS))
    ap.add_argument("--tree", default=ROOT,
                    help="the tree to sample (default: this one)")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hz", type=int, default=4000)
    ap.add_argument("--top", type=int, default=30)
    ap.add_argument("--json", action="store_true",
                    help="one JSON line instead of the table")
    args = ap.parse_args()

    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import bench
    assert os.path.dirname(os.path.abspath(bench.__file__)) == tree
    from cueball_amd import fsm as mod_fsm
    if not mod_fsm.NATIVE:
        raise SystemExit("pc_sample: the native core is not in use")
    from cueball_amd import _speed
    rng = mapped_range(_speed.__file__)
    syms = text_symbols(_speed.__file__)
    addrs = [a for a, _ in syms]

    with tempfile.TemporaryDirectory(prefix="pc_sample.") as tmp:
        dll = build_sampler(tmp)
        n = asyncio.run(sampled_steps(bench, dll, rng, CONFIGS[args.config],
                                      args.steps, args.warmup, args.hz))
        pcs, vias = dll.pcs_pcs(), dll.pcs_vias()
        self_, called = collections.Counter(), collections.Counter()
        elsewhere = 0
        base, lo, hi = rng
        for i in range(n):
            pc, via = pcs[i], vias[i]
            if lo <= pc < hi:
                self_[symbol_of(syms, addrs, pc - base)] += 1
            elif via:
                called[symbol_of(syms, addrs, via - base)] += 1
            else:
                elsewhere += 1
        missed = dll.pcs_missed()
        dll.pcs_free()

    if n == 0:
        raise SystemExit("pc_sample: no samples")
    in_self, in_called = sum(self_.values()), sum(called.values())
    if args.json:
        print(json.dumps({
            "config": args.config, "samples": n, "missed": missed,
            "self": in_self, "called": in_called, "elsewhere": elsewhere,
            "functions": {k: [self_[k], called[k]]
                          for k in set(self_) | set(called)}}))
        return
    pct = lambda x: 100.0 * x / n
    print("%s: %d samples at %d Hz over %d steps of %d claims "
          "(%d ticks not taken)" % (args.config, n, args.hz, args.steps,
                                    CLAIMS_PER_STEP, missed))
    print("_speed self %.1f %%, called from _speed %.1f %%, elsewhere "
          "%.1f %%" % (pct(in_self), pct(in_called), pct(elsewhere)))
    print()
    print("| function | self % | called % | both % |")
    print("|---|---|---|---|")
    names = sorted(set(self_) | set(called),
                   key=lambda k: -(self_[k] + called[k]))
    for k in names[:args.top]:
        print("| `%s` | %.1f | %.1f | %.1f |" % (
            k, pct(self_[k]), pct(called[k]), pct(self_[k] + called[k])))


if __name__ == "__main__":
    main()
