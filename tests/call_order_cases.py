"""Inputs for the order of the pair table (hla-la_amd/csrc/call_order_core.h), deterministic from seeds: (name, LL, Mism_avg) with the sizes placed at the constants
of the device path -- the tile size T, the heap cap H, the threads of a level's workgroup and the elements of one step of its scans, which the library reports
(pkg.call_order_params()).  tests/test_call_order_model.py holds the host model against std::sort + std::reverse on them, tests/test_gpu_call_order.py the device."""
import functools

import numpy as np

from conftest import load_package

P = load_package()
PARAMS = P.call_order_params()
T, H, BLOCK, CHUNK = PARAMS["tile"], PARAMS["max_heap"], PARAMS["block"], PARAMS["chunk"]
E_ARG, E_CAPACITY = -1, -4
LARGEST = 70001
LOCUS_DUP = {120: ((5, 17), (40, 3), (41, 3), (119, 0)), 200: ((5, 17), (40, 3), (41, 3), (199, 0))}


def sizes():
    s = {1, 2, 16, 17, 18, 33, T - 1, T, T + 1, 2 * T + 3}
    for c in (BLOCK, CHUNK, H):
        s |= {c - 1, c, c + 1}
    s |= {CHUNK + 2, 2 * CHUNK + 1, 2 * CHUNK + 2}          # a level's walk covers n - 1 places: one step exactly, two steps exactly, and one place more
    return sorted(s)


def drawn(n, distinct, seed):
    rng = np.random.default_rng(seed)
    return -0.37 * rng.integers(0, distinct, n), 0.5 * rng.integers(0, min(distinct, 7), n)


def organ_pipe(n):
    i = np.arange(n)
    return np.where(i < n // 2, i, n - i).astype(np.float64), (i % 3).astype(np.float64)


def lopsided(n, seed):
    """the three smallest keys at places 1, n / 2 and n - 1: the median of three is the third smallest element, and a child of at most 16 comes out of a grid level"""
    rng = np.random.default_rng(seed)
    ll = rng.integers(10, 60, n).astype(np.float64); ma = rng.integers(0, 3, n).astype(np.float64)
    ll[[1, n // 2, n - 1]] = [1.0, 2.0, 3.0]
    return ll, ma


@functools.lru_cache(maxsize=None)
def locus_table(C):
    from test_call import table
    return table(C, np.random.default_rng(100 + C), LOCUS_DUP[C])


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for n in sizes():
        for d in (1, 3, 50):
            out.append((f"drawn-{n}-{d}", *drawn(n, d, 1000 * d + n)))
    for n in (T + 1, LARGEST):
        i = np.arange(n, dtype=np.float64)
        out.append((f"ascending-{n}", i, np.ones(n)))
        out.append((f"descending-{n}", -i, np.arange(n) % 2 * 1.0))
        out.append((f"zeros-{n}", np.where(np.arange(n) & 1, -0.0, 0.0), np.where(np.arange(n) & 2, 0.0, -0.0)))
    for n in (T + 1, 3 * T):
        out.append((f"lopsided-{n}", *lopsided(n, n)))
    out.append(("organ-16384", *organ_pipe(16384)))
    for C in (120, 200):
        ll, ma, _ = locus_table(C)
        out.append((f"locus-C{C}", ll, ma))
    assert max(len(c[1]) for c in out) == LARGEST
    return out


def tie_families():
    """the cases in which pairs tie in both keys beyond the sizes that the library sorts by insertion alone"""
    return [c for c in cases() if len(c[1]) > 16 and (c[0].startswith(("drawn-", "zeros-", "locus-", "lopsided-")))]


REFUSED_N = 20000                 # organ-pipe: a range beyond H is met with no depth left
REFUSED_C = 200                   # ... and the same family as the table of a locus (nP = 20 100)


def stable_order(ll, ma):
    """a stable sort by the same keys, reversed: what a device sort that is not the library's would give"""
    return np.lexsort((-np.asarray(ma), np.asarray(ll)))[::-1].astype(np.int32)


@functools.lru_cache(maxsize=None)
def references():
    """std::sort + std::reverse of every case, computed once"""
    return {name: P.host_pair_order_reference(ll, ma) for name, ll, ma in cases()}
