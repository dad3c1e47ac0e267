"""Inputs of the tests of the pairing stage's overflow class (k_pair_overflow, csrc/kernel_pair_overflow.hip): pairs beyond the three capacities of the pairing
kernels -- more than 64 kept chains on a mate, more than 1024 combinations, several combinations with a chain of more than 512 columns.  Built from the helpers
of tests/pair_edge_cases.py, in its family format; tests/test_pair_overflow_reference.py holds the oracle, tests/test_gpu_pair_overflow.py the kernels against
tests/pair_reference.py without capacities.  Plain numpy; every family is built once per process."""
import functools

import numpy as np

import pair_edge_cases as pe
from tools import synth

OVER_COUNTS = [(2, 2), (129, 1), (1, 129), (128, 2), (130, 3), (65, 65), (65, 16)]


def beyond(kept):
    """Pairs that a capacity alone keeps from the pairing kernels, by their kept counts (chains of up to 512 columns)."""
    return pe._refused(kept)


@functools.lru_cache(maxsize=None)
def over_counts():
    """Kept chains per mate around the words of the shared-by-chain-k mask (64 / 65, 128 / 129 / 130), one mate over the limit with few combinations
    (129 x 1, 1 x 129), 4225 and 1040 combinations; (2, 2) is an ordinary pair beside them.  Every second pair holds its records in reverse order."""
    w = pe.base_world()
    reads = pe._base_reads(w, len(OVER_COUNTS), seed=31)
    out, kept = [], []
    for p, (n1, n2) in enumerate(OVER_COUNTS):
        for m, n in enumerate((n1, n2)):
            out.append(pe.with_variants(reads[2 * p + m], n, reverse=bool(p % 2))); kept.append(n)
    return dict(name="over-counts", world=w, batch=pe.assemble(out, 200.0, 35.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=384,
                beyond=beyond(kept), n_comb=[a * b for a, b in OVER_COUNTS], floors=dict(multi=7, not_first=5))


OVER_BEST = [({64}, 2), ({129}, 3), ({64, 129}, 1)]          # positions of the good chains among the 130 of mate 1; kept chains of mate 2


@functools.lru_cache(maxsize=None)
def over_best():
    """300-base reads, 130 kept chains on mate 1: the selected chain in the second and in the third mask word, at the last list position, and tied at the top
    (the first of the two wins)."""
    w = pe.base_world()
    reads = pe._base_reads(w, len(OVER_BEST), seed=37, read_len=300, ins_mean=150.0)
    out, kept = [], []
    for p, (good, n2) in enumerate(OVER_BEST):
        out += [pe.with_good_at(reads[2 * p], 130, good), pe.with_variants(reads[2 * p + 1], n2)]; kept += [130, n2]
    return dict(name="over-best", world=w, batch=pe.assemble(out, 150.0, 35.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=512,
                beyond=[0, 1, 2], best1=[min(g) for g, _ in OVER_BEST], floors=dict(multi=3, not_first=3))


OVER_COLUMN_LENGTHS = (520, 600)


@functools.lru_cache(maxsize=None)
def over_columns():
    """max_columns = 1024.  Reads of 520 and 600 bases with 2 x 3 kept chains: chains of 521 and 601 columns with six combinations.  The two registers of so long
    a read lie too many nats apart for the exact model to decide most Phred bytes (floors: undecided columns are counted, not capped); what binds the kernels
    on this family is equality with the oracle."""
    w = pe.base_world()
    out, kept = [], []
    for p, L in enumerate(OVER_COLUMN_LENGTHS):
        reads = pe._base_reads(w, 1, seed=50 + p, read_len=L, ins_mean=150.0, haps=[0])
        out += [pe.with_variants(reads[0], 2), pe.with_variants(reads[1], 3)]; kept += [2, 3]
    return dict(name="over-columns", world=w, batch=pe.assemble(out, 150.0, 35.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=1024,
                beyond=[0, 1], lengths=list(OVER_COLUMN_LENGTHS), undecided_uncapped=True, floors=dict(multi=2))


@functools.lru_cache(maxsize=None)
def over_fan():
    """pe.fan()'s recipe with 65 kept chains on the mate of pair 0 that runs back through the fan: a pair beyond the capacities that also owns DP calls of the
    side stream's classes, so that a fused alignment lists it for the overflow class in its second pairing pass."""
    w = synth.make_fan_world()
    q = pe.low_quals(150, 7)
    out, kept = [], []
    for p, (s, n1, n2) in enumerate([(614, 65, 2), (614, 3, 3), (50, 12, 11), (680, 2, 2)]):
        a = pe._direct_pair(w, 310 - p, s, 150, 180 + 5 * p, q)
        m1 = dict(a[0], recs=[pe.placed(a[0]["recs"][0], 150, i % 2, 8 + i // 2) for i in range(n1 - 1)] + [pe.far(a[0]["recs"][0], 150)])
        out += [m1, pe.with_variants(a[1], n2, q1_tenths=7)]; kept += [n1, n2]
    return dict(name="over-fan", world=w, batch=pe.assemble(out, 200.0, 35.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=384, deferred=[0, 1],
                beyond=[0], floors=dict(multi=4))


OVER_FIXTURE = [(65, 1), (1, 65), (65, 16), (41, 25)]


@functools.lru_cache(maxsize=None)
def over_fixture():
    """The family of tests/golden/ref_pair_overflow.npz (what the reference's own processBAM makes of it is committed there): 65 kept chains on either mate, 1040
    and 1025 combinations, every second pair in reverse order, on the world of 1600 levels that pe.limits() uses."""
    w = pe._world(11, 1600, 1, 3, n_largegap=0)
    reads = pe._base_reads(w, len(OVER_FIXTURE), seed=38, ins_mean=120.0)
    out, kept = [], []
    for p, (n1, n2) in enumerate(OVER_FIXTURE):
        out += [pe.with_variants(reads[2 * p], n1, reverse=bool(p % 2)), pe.with_variants(reads[2 * p + 1], n2, reverse=bool(p % 2))]; kept += [n1, n2]
    return dict(name="over-fixture", world=w, batch=pe.assemble(out, 120.0, 35.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=384,
                beyond=[0, 1, 2, 3], n_comb=[a * b for a, b in OVER_FIXTURE], floors=dict(multi=4, not_first=2))


def check_floors(s, f, label):
    """pe.check_floors; a family with undecided_uncapped states its undecided share instead of capping it at 1 %."""
    if not f.get("undecided_uncapped"):
        return pe.check_floors(s, f["floors"], label)
    print("%s: %s" % (label, {k: (float("%.3g" % v) if isinstance(v, float) else v) for k, v in s.items()}))
    print("%s: %d of %d columns undecided by the exact model" % (label, s["undecided"] + s["whole"], s["columns"]))
    for k, v in f["floors"].items():
        assert s[k] >= v, (label, k, s[k], v)


NEW_FAMILIES = {"over-counts": over_counts, "over-best": over_best, "over-columns": over_columns, "over-fan": over_fan, "over-fixture": over_fixture}
