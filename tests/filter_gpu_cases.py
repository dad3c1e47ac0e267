"""Cases for the typer's filter stage off the host (hlala_filter_positions_gpu and its host model, hlala_host_filter_model): exon-position dicts in the layout
Batch.exon_positions() returns, each with the parameters it runs under.  Shared by tests/test_filter_gpu_model.py (model == hlala_filter_positions == oracle) and
tests/test_gpu_filter_positions.py (device == hlala_filter_positions); everything is deterministic and built once per process."""
import functools

import numpy as np

from conftest import load_package
from test_filters import hand_case, synth_positions

P = load_package()
MAX_BUCKET = 4096
DT = dict(read_pair=np.int32, read_weighted_ok=np.float64, read_fraction_ok=np.float64, read_distance=np.int32, read_cols_nongap=np.int32, pos_off=np.int32, pos_exon=np.int32,
          pos_level=np.int32, pos_mate=np.uint8, pos_mapq=np.uint8, pos_novel_gap=np.int32, geno_off=np.int32, geno_chars=np.uint8, qual_chars=np.uint8, read_reverse=np.uint8)


def locus(reads):
    """reads: (w1, w2, rev1, rev2, [(exon position, quality byte, mate, allele bytes), ...]) -> the dict of Batch.exon_positions(), read_reverse included.  The arrays
    the filters never read (qual_chars, pos_level, read_fraction_ok, ...) are there and hold values no filter could make sense of."""
    e = {k: [] for k in DT}
    e["pos_off"].append(0); e["geno_off"].append(0)
    for r, (w1, w2, r1, r2, pos) in enumerate(reads):
        e["read_pair"].append(r); e["read_weighted_ok"] += [w1, w2]; e["read_fraction_ok"] += [-7.0, -7.0]; e["read_distance"].append(-3); e["read_cols_nongap"] += [-1, -1]
        e["read_reverse"] += [r1, r2]
        for x, q, mate, al in pos:
            al = al.encode("latin-1") if isinstance(al, str) else bytes(al)
            e["pos_exon"].append(x); e["pos_level"].append(-5); e["pos_mate"].append(mate); e["pos_mapq"].append(q); e["pos_novel_gap"].append(-9)
            e["geno_chars"] += list(al); e["qual_chars"] += [255] * len(al); e["geno_off"].append(len(e["geno_chars"]))
        e["pos_off"].append(len(e["pos_exon"]))
    e = {k: np.array(v, DT[k]) for k, v in e.items()}
    e.update(n_reads=len(reads), n_pos=len(e["pos_exon"]), n_chars=len(e["geno_chars"]))
    return e


Q_OK = ord("I")


def single_bucket(n, seed=0, weights=None, alleles=None):
    """n reads with one position each at exon position 0.  weights: per read (both mates); default: mostly 1.0 (ties) with a few lower values."""
    rng = np.random.default_rng(1000 + seed + n)
    reads = []
    for r in range(n):
        w = float(weights[r]) if weights is not None else (1.0 if rng.random() < 0.7 else 1.0 - int(rng.integers(1, 4)) / 128.0)
        al = alleles[r] if alleles is not None else ("ACGT"[int(rng.integers(0, 2))] if rng.random() < 0.9 else ("G", "AT", "_")[int(rng.integers(0, 3))])
        reads.append((w, w, int(rng.random() < 0.5), 0, [(0, Q_OK, 1, al)]))
    return locus(reads)


def adversary_bucket(n):
    """a bucket whose weights drive std::sort into its heap sort: McIlroy's adversary (bam_fill_wide_cases.adversary) scaled into [0, 1], exactly"""
    import bam_fill_wide_cases as W
    return single_bucket(n, weights=W.adversary(n).astype(np.float64) / 8192.0)


def strand_world(seed, n_reads, n_exon):
    rng = np.random.default_rng(seed)
    e = synth_positions(rng, n_reads, n_exon)
    e["read_reverse"] = (rng.random(2 * n_reads) < 0.07).astype(np.uint8)
    e["read_mapq"] = np.ones(2 * n_reads)
    return e


@functools.lru_cache(maxsize=None)
def worlds():
    """the worlds of tests/test_filters.py with their parameter sets, then the switches and first20_n values around the insertion-sort limit: [(name, e, params)]"""
    d = P.default_filter_params
    out = [("hand", hand_case(), None)]
    for seed, n_reads, n_exon in ((1, 60, 200), (2, 900, 300), (3, 4000, 546), (4, 2500, 120)):
        e = synth_positions(np.random.default_rng(seed), n_reads, n_exon)
        for k, prm in enumerate((None, d(high_coverage_filter=1, high_coverage_min_coverage=1, high_coverage_min_freq=0.15), d(first20_limit_per_read=0), d(min_per_position_mapq=0.2))):
            out.append((f"seed{seed}-set{k}", e, prm))
        if seed == 2:
            for ff in (0, 2):
                out.append((f"seed2-filter_first20={ff}", e, d(filter_first20=ff)))
            for n20 in (0, 1, 16, 17, 20):
                out.append((f"seed2-first20_n={n20}", e, d(first20_n=n20)))
    for seed, n_reads, n_exon in ((11, 1500, 150), (12, 4000, 300)):
        e = strand_world(seed, n_reads, n_exon)
        for cov, fr in ((100, 0.1), (30, 0.05), (10, 0.2)):
            out.append((f"seed{seed}-strand{cov}", e, d(long_read_strand_filter=1, strand_min_allele_coverage=cov, strand_min_freq=fr)))
    return out


# Buckets that tell the library's tie order from a stable one: n entries of weight 1.0 (all tied at the top) but the last, every entry allele 'A' but the ones at
# `minor`, which carry 'C'.  'C' is kicked where none of its entries is among the first 20.  A stable descending sort takes entries 0..19; std::sort + std::reverse
# leave another 20 in front.  Chosen on the reference machine's libstdc++ so that hlala_filter_positions itself differs from the stable order on them; the test counts
# how many still do and asks for 8.
TIE_BUCKETS = [(22, (11,)), (25, (20,)), (28, (14,)), (32, (16,)), (33, (17, 18)), (35, (31, 32)), (37, (19,)), (39, (37,)), (42, (11,)), (45, (1,)), (48, (2, 3)), (52, (13,)),
               (57, (5, 6, 7)), (60, (20, 21)), (63, (16,)), (64, (31,)), (64, (1, 2, 3))]


def tie_bucket(n, minor):
    return single_bucket(n, weights=[1.0] * (n - 1) + [0.5], alleles=["C" if i in minor else "A" for i in range(n)])


@functools.lru_cache(maxsize=None)
def genotype_locus():
    """one locus whose buckets hold what allele identity and the strand order can trip over; every read has a position in several buckets"""
    rng = np.random.default_rng(77)
    ins = bytes(rng.integers(65, 70, 300).astype(np.uint8))
    long_a, long_b = ins, ins[:-1] + b"Z"                                      # two 300-byte insertions that differ in the last byte
    pools = [
        ["A", "C", "G", "T"],                                                  # 0: length 1
        ["AC", "AG", "ACG", "ACT", "ACGT", "ACGA", "ACGTA", "ACGTC"],          # 1: lengths 2-5 that differ only in the last byte
        ["A", "AC", "ACG", "ACGT", "ACGTA"],                                   # 2: each a proper prefix of the next
        ["_", "A", "_", "AT"],                                                 # 3: the gap allele
        [long_a, long_b, b"A", ins[:299]],                                     # 4: 300-byte insertions, and their common prefix
        [b"\x7f", b"\x80", b"\xff", b"A\x80", b"A\x7f", b"A"],                 # 5: bytes >= 0x80: the strand order is unsigned
        [bytes([65 + (i % 26), 65 + (i // 26)]) for i in range(300)],          # 6: 300 distinct alleles in one bucket
        [b"", b"A", b""],                                                      # 7: an empty genotype is an allele like any other
    ]
    reads = []
    for r in range(700):
        w = 1.0 if rng.random() < 0.6 else 1.0 - int(rng.integers(1, 6)) / 64.0
        pos = []
        for x, pool in enumerate(pools):
            if x == 6:
                al = pool[r % 300] if r < 600 else pool[int(rng.integers(0, 300))]
            else:
                al = pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.5 else pool[0]
            pos.append((x, Q_OK if rng.random() < 0.95 else ord("#"), 1 + int(rng.random() < 0.4), al))
            if rng.random() < 0.02:
                pos.append((x, Q_OK, 2, pool[-1]))                             # a read with two entries in one bucket
        reads.append((w, 1.0, int(rng.random() < 0.3), int(rng.random() < 0.6), pos))
    return locus(reads)


def genotype_cases():
    d = P.default_filter_params
    e = genotype_locus()
    return [("genotypes-default", e, None),
            ("genotypes-strand", e, d(long_read_strand_filter=1, strand_min_allele_coverage=3, strand_min_freq=0.3)),
            ("genotypes-strand-hc", e, d(long_read_strand_filter=1, strand_min_allele_coverage=1, strand_min_freq=0.45, high_coverage_filter=1, high_coverage_min_coverage=10, high_coverage_min_freq=0.02)),
            ("genotypes-first20-off", e, d(filter_first20=0, long_read_strand_filter=1, strand_min_allele_coverage=2, strand_min_freq=0.2))]


E_ARG, E_CAPACITY = -1, -4


def refusals():
    """[(name, e, params, code)]: what the host refuses, refused alike; what only the new path can see, refused with HLALA_E_ARG; a bucket beyond the capacity"""
    d = P.default_filter_params
    base = single_bucket(30, seed=5)

    def with_(**kw):
        e = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        for k, (i, v) in kw.items():
            e[k][i] = v
        return e
    no_rev = {k: v for k, v in base.items() if k != "read_reverse"}
    return [("bucket-4097", single_bucket(MAX_BUCKET + 1, seed=9), None, E_CAPACITY),
            ("nan-weight", with_(read_weighted_ok=(7, np.nan)), None, E_ARG),
            ("quality-byte-0", with_(pos_mapq=(3, 0)), None, E_ARG),
            ("quality-byte-20", with_(pos_mapq=(29, 20)), None, E_ARG),
            ("negative-exon", with_(pos_exon=(11, -1)), None, E_ARG),
            ("pos_off-descends", with_(pos_off=(10, 12)), None, E_ARG),
            ("geno_off-descends", with_(geno_off=(10, 10 ** 5)), None, E_ARG),
            ("pos_off-end", with_(pos_off=(30, 29)), None, E_ARG),
            ("geno_off-end", with_(geno_off=(30, 10 ** 6)), None, E_ARG),
            ("strand-without-read_reverse", no_rev, d(long_read_strand_filter=1), E_ARG)]


HOST_REFUSES = {"quality-byte-0", "quality-byte-20", "negative-exon", "strand-without-read_reverse"}      # hlala_filter_positions answers HLALA_E_ARG to these itself


def empty_cases():
    """n_reads == 0; reads without positions; a locus where no position passes the mapq test (also under a limit that then ignores every read)"""
    d = P.default_filter_params
    none = locus([])
    no_pos = locus([(1.0, 1.0, 0, 0, []) for _ in range(5)])
    low = locus([(1.0, 0.9, 0, 1, [(x, ord("#"), 1, "A") for x in range(r % 3, 3 + r % 3)]) for r in range(40)])
    return [("no-reads", none, None), ("no-positions", no_pos, None), ("no-positions-limit=-1", no_pos, d(first20_limit_per_read=-1)), ("none-passes", low, None),
            ("none-passes-limit=-1", low, d(first20_limit_per_read=-1))]


def host_only_cases():
    """parameter values the reference never runs with and the oracle does not take: the host's loops decide, and the new path follows them"""
    d = P.default_filter_params
    e = synth_positions(np.random.default_rng(2), 900, 300)
    return [("seed2-first20_n=-3", e, d(first20_n=-3)), ("seed2-limit=-1", e, d(first20_limit_per_read=-1)), ("seed2-first20_n=5000", e, d(first20_n=5000)),
            ("seed2-min_prop=1.5", e, d(first20_min_prop=1.5, first20_limit_per_read=40))]


@functools.lru_cache(maxsize=None)
def thin_locus():
    """3000 buckets of one entry"""
    return locus([(1.0 - (r % 7) / 100.0, 1.0, r & 1, 0, [(50 * r + k, Q_OK, 1, "ACGT"[(r + k) % 4]) for k in range(50)]) for r in range(60)])


def check_equal(got, want, what):
    """(pos_use, read_ignored, stats[, counts]) against (pos_use, read_ignored, stats): bytes and all twelve counters"""
    assert np.array_equal(got[0], want[0]), f"{what}: pos_use differs at {np.flatnonzero(got[0] != want[0])[:8]}"
    assert np.array_equal(got[1], want[1]), f"{what}: read_ignored differs at {np.flatnonzero(got[1] != want[1])[:8]}"
    assert len(want[2]) == 12 and got[2] == want[2], f"{what}: counters {got[2]} != {want[2]}"
