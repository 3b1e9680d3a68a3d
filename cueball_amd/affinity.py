"""Key affinity for claims: the arithmetic, and nothing else.

A pool created with ``claimAffinity`` asks this module in which order
the backends are to be tried for a claim that carries an
``affinityKey``.  The order is rendezvous hashing (highest random
weight): every backend gets a score that depends on the key and on the
backend alone, and the backends are tried by descending score.  Removing
a backend moves only the keys that had it first, each to its former
second choice; adding it again moves them back.

The hash is part of the public contract (docs/api.md, "Key affinity"):
clients in different processes, on either runtime and on any version
must agree on it, so it is spelled out here in full and never borrows
from Python's salted ``hash()``.

- ``fnv1a64``: FNV-1a over 64 bits, offset ``0xcbf29ce484222325``,
  prime ``0x100000001b3``.
- ``mix64``: the splitmix64 finaliser.
- ``backend_hash(key) = mix64(fnv1a64(key as UTF-8))``.
- ``score(affinity key, backend) = mix64(fnv1a64(affinity key) ^
  backend_hash(backend))``.

The queue walk, the load census and the bookkeeping live in
``cueball_amd.pool``.
"""

from __future__ import annotations

import os as _os
from fractions import Fraction
from typing import Any, Callable, Iterable, List, Optional, Sequence, Tuple

__all__ = ["fnv1a64", "mix64", "backend_hash", "score", "rank", "order",
           "load_cap", "key_bytes", "DEFAULT_LOAD_FACTOR"]

_MASK = 0xFFFFFFFFFFFFFFFF
_FNV_OFFSET = 0xcbf29ce484222325
_FNV_PRIME = 0x100000001b3

#: the bound of "consistent hashing with bounded loads" as that
#: literature states it: no backend carries more than 1.25 times the mean
DEFAULT_LOAD_FACTOR = 1.25


def fnv1a64(data: bytes) -> int:
    """FNV-1a, 64 bits."""
    h = _FNV_OFFSET
    for b in data:
        h = ((h ^ b) * _FNV_PRIME) & _MASK
    return h


def mix64(z: int) -> int:
    """The splitmix64 finaliser, modulo 2^64."""
    z &= _MASK
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & _MASK
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & _MASK
    z ^= z >> 31
    return z


def rank(key: bytes, backend_hashes: Sequence[int]) -> Tuple[int, ...]:
    """The indices of `backend_hashes` (``backend_hash`` values) by
    descending score for the affinity key `key`, best first.  Equal
    scores keep their input order: hand the hashes in backend-key order
    and a tie goes to the smaller key."""
    kh = fnv1a64(key)
    scores = [mix64(kh ^ h) for h in backend_hashes]
    return tuple(sorted(range(len(scores)), key=lambda i: -scores[i]))


PurePythonFnv1a64 = fnv1a64
PurePythonRank = rank

# Native core: when the C++ extension is built, its hash and rank
# replace the two above, which is what a keyed claim pays for per try
# (CUEBALL_PURE=1 forces the Python ones; the suite compares both).
if not _os.environ.get("CUEBALL_PURE"):
    try:
        from ._speed import affinity_hash as fnv1a64  # type: ignore # noqa
        from ._speed import affinity_rank as rank  # type: ignore # noqa
    except ImportError:
        pass


def key_bytes(affinity_key: Any) -> bytes:
    """An affinity key as the hash reads it: ``bytes`` as they are, a
    ``str`` UTF-8 encoded; the empty key is a key like any other."""
    if isinstance(affinity_key, bytes):
        return affinity_key
    if isinstance(affinity_key, str):
        return affinity_key.encode("utf-8")
    raise TypeError("affinityKey must be bytes or str, not %s"
                    % type(affinity_key).__name__)


def _backend_hash(key: str, fnv: Callable[[bytes], int]) -> int:
    return mix64(fnv(key.encode("utf-8")))


def backend_hash(key: str) -> int:
    """What a backend key contributes to every score: computed once
    per backend, when the resolver adds it."""
    return _backend_hash(key, fnv1a64)


def score(affinity_key: Any, backend: str) -> int:
    return mix64(fnv1a64(key_bytes(affinity_key)) ^ backend_hash(backend))


def _order(affinity_key: Any, backend_keys: Iterable[str],
           fnv: Callable[[bytes], int], rank_: Callable) -> List[str]:
    data = key_bytes(affinity_key)
    keys = sorted(backend_keys)
    idx = rank_(data, tuple(_backend_hash(k, fnv) for k in keys))
    return [keys[i] for i in idx]


def order(affinity_key: Any, backend_keys: Iterable[str]) -> List[str]:
    """`backend_keys` by descending ``score`` for `affinity_key`, the
    backend to prefer first; a tie goes to the lexicographically smaller
    backend key.  The order of `backend_keys` itself does not matter."""
    return _order(affinity_key, backend_keys, fnv1a64, rank)


def PurePythonOrder(affinity_key: Any,
                    backend_keys: Iterable[str]) -> List[str]:
    """``order`` on the Python hash and rank, whatever is loaded."""
    return _order(affinity_key, backend_keys, PurePythonFnv1a64,
                  PurePythonRank)


def load_fraction(load_factor: Any) -> Tuple[int, int]:
    """`load_factor` as the exact ratio its shortest decimal spelling
    names (1.1 is 11/10, not the binary double next to it), so that
    ``load_cap`` is integer arithmetic and no ceiling hangs on float
    fuzz."""
    if isinstance(load_factor, int):
        return load_factor, 1
    f = Fraction(repr(float(load_factor)))
    return f.numerator, f.denominator


def cap_of(num: int, den: int, total_in_use: int, backends: int) -> int:
    """``load_cap`` for a factor that ``load_fraction`` has split."""
    return -((-num * (total_in_use + 1)) // (den * backends))


def load_cap(load_factor: Any, total_in_use: int,
             backends_with_connections: int) -> int:
    """``ceil(load_factor * (total_in_use + 1) / m)``: how many of its
    connections a backend may have in use before a keyed claim passes
    it over, with `m` backends holding connections and the claim itself
    counted in.  The bound of "consistent hashing with bounded loads"."""
    num, den = load_fraction(load_factor)
    return cap_of(num, den, total_in_use, backends_with_connections)
