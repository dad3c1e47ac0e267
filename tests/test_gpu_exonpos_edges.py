"""The exon-position kernels (csrc/kernel_exonpos.hip: k_exon_positions<0>, k_exon_positions<1>, k_unit_stats) on the families of tests/exonpos_edge_cases.py:
mates that share a hundred levels (the whole two-pointer merge), every kind of column run, locus descriptions on every edge of a mate, every threshold met
with equality and missed by the least amount, batch sizes around the block of 128 threads, refused units, single reads.

Per family there is one Context and the batch is aligned once.  Every call of Batch.exon_positions is held
  * against the exact model (tests/exonpos_reference.py) fed with the library's OWN Batch.pairs(): integers and characters exactly, read_weighted_ok and
    read_fraction_ok bit for bit (and within the model's derived bounds of their exact rational values), read_mapq and read_reverse exactly (the model copies
    them from the same pairs) -- this holds whatever the aligner chose;
  * against the oracle's exon_positions of the oracle's own alignments, as tests/test_exon_positions.py does (read_mapq: rtol 1e-9, atol 1e-15: device exp()).
The census floors of the family hold on the library's own pairs; Batch.unit_stats equals the model's; a call with cap_pos one below the need answers
HLALA_E_CAPACITY with the needed sizes and the call with exactly the need equals the first result; a second call gives identical arrays.
Largest |binary64 - exact| / bound ratios of the OK fractions are printed (pytest -s).  tests/test_exonpos_reference.py::test_the_suite_bites shows which
family notices which kind of broken kernel."""
import ctypes as C

import numpy as np
import pytest

import exonpos_edge_cases as ee
import exonpos_reference as er
import oracle_binding as ob
from test_exonpos_reference import aligned, check_locus_expectation, check_size_outcomes, oracle_positions, pcorrect

pytestmark = pytest.mark.gpu


class Run:
    """A family on the GPU: the context, the aligned batch, its pairs, the model over them."""

    def __init__(self, pkg, oracle, f):
        self.pkg, self.f = pkg, f
        b = self.b = f["batch"]
        self.ctx = pkg.Context(f["world"]["graph"], f["world"]["contigs"], insert_mean=b.get("insert_mean", 200.0), insert_sd=b.get("insert_sd", 35.0), rng_seed=5,
                               long_read_mode=f["long_read_mode"], max_columns=f["max_columns"])
        self.gb = self.ctx.batch_unpaired(b) if f["unpaired"] else self.ctx.batch(b)
        self.gb.align()
        self.pairs = self.gb.pairs()
        # pCorrect as the library's tables hold it; the same data as the oracle's
        table = np.zeros(256); q = np.arange(256, dtype=np.uint8)
        self.ctx._check(self.ctx.lib.hlala_kat_phred(self.ctx.h, 256, None, None, q.ctypes.data_as(pkg.c_u8p), table.ctypes.data_as(pkg.c_f64p)), "hlala_kat_phred")
        assert np.array_equal(table, pcorrect())
        self.M = er.Model(self.pairs, b, f["max_columns"], table, f["unpaired"])
        self.ob, self.opairs, self.oM = aligned(oracle, f)          # the oracle's batch lacks the units it cannot be given (the family's last ones)
        self.ratio = 0.0

    def library(self, L):
        return self.gb.exon_positions(L["level_min"], L["level_to_exon"], L["insert_mean"], L["insert_sd"], **er.locus_args(L))

    def check(self, L, label, oracle_locus=None):
        f = self.f; label = "%s: %s" % (f["name"], label)
        g = self.library(L)
        er.compare(g, self.M.exon_positions(L), label + " (model on the library's pairs)", mapq_exact=True)
        Lo = oracle_locus or L
        if Lo["pair_mask"] is not None:
            Lo = dict(Lo, pair_mask=Lo["pair_mask"][:self.ob["n_pairs"]])
        er.compare(g, oracle_positions(self.opairs, self.ob, f, Lo), label + " (oracle)", reverse=False)
        assert (np.diff(g["read_pair"]) > 0).all() and g["pos_off"][0] == 0 and g["pos_off"][-1] == g["n_pos"] and g["geno_off"][0] == 0 and g["geno_off"][-1] == g["n_chars"], label
        assert (np.diff(g["pos_off"]) > 0).all() and (np.diff(g["geno_off"]) > 0).all(), label
        return g

    def rows(self):
        n = self.b["n_pairs"]
        return [r for u in range(n) if self.pairs["pair_status"][u] == 0 for r in ([u] if self.f["unpaired"] else [2 * u, 2 * u + 1])]

    def unit_stats(self):
        er.compare_stats(self.gb.unit_stats(), self.M.unit_stats(), self.f["name"] + ": unit_stats")

    def capacity(self, L, first):
        """cap_pos one below the need: HLALA_E_CAPACITY and the need in n_reads / n_pos / n_chars; exactly the need: the first result again."""
        pkg, ctx = self.pkg, self.ctx
        need = (first["n_reads"], first["n_pos"], first["n_chars"])
        assert need[1] > 0
        D, keep = pkg.make_locus_desc(L["level_min"], L["level_to_exon"], L["insert_mean"], L["insert_sd"], **er.locus_args(L))
        o, d = pkg.alloc_exon_positions_out(need[0], need[1] - 1, need[2])
        rc = ctx.lib.hlala_exon_positions(ctx.h, self.gb.b, C.byref(D), C.byref(o))
        assert rc == pkg.E_CAPACITY and (o.n_reads, o.n_pos, o.n_chars) == need, (rc, o.n_reads, o.n_pos, o.n_chars, need)
        o, d = pkg.alloc_exon_positions_out(*need)
        ctx._check(ctx.lib.hlala_exon_positions(ctx.h, self.gb.b, C.byref(D), C.byref(o)), "hlala_exon_positions")
        identical(pkg.trim_exon_positions(o, d), first, self.f["name"] + ": exactly the needed capacity")

    def done(self, floors_locus=None, census=None):
        f = self.f
        if census is None and floors_locus is not None:
            census = ee.census(self.pairs, self.b, f["max_columns"], floors_locus, f["unpaired"])
        if census is not None:
            ee.check_floors(census, f["floors"], f["name"] + " (library)")
        print("%s: largest |binary64 - exact| / bound of the OK fractions: %.3g" % (f["name"], self.M.fp_ratio(self.rows())))
        self.gb.close(); self.ctx.close()


def identical(a, b, label):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)
        else:
            assert a[k] == b[k], (label, k)


@pytest.mark.parametrize("name", list(ee.FIXED))
def test_family(pkg, oracle, name):
    """overlap: the merge of lines 178-189 (take = 0 / 1 / 2 / 3, worstQ of line 66, both cursors advancing); columns: pos_next's fold of insertion columns
    (line 51), the strip rule (lines 60-61, 94-97), both novel-gap sweeps (lines 43, 57); refused: line 111 and k_unit_stats' line 209;
    unpaired_columns / unpaired_long: the single-read branch, lines 115-150, and chains of thousands of columns."""
    f = ee.FIXED[name](); R = Run(pkg, oracle, f)
    n = f["batch"]["n_pairs"]
    first = None
    for label, L in f["loci"]:
        g = R.check(L, label)
        first = first or (L, g)
    L, g = first
    R.unit_stats()
    R.capacity(L, g)
    identical(R.library(L), g, name + ": the same call again")
    R.unit_stats()
    if name == "refused":
        bad = sorted(f["refused"])
        assert [u for u in range(n) if R.pairs["pair_status"][u] != 0] == bad and bad
        us = R.gb.unit_stats()
        assert not set(g["read_pair"].tolist()) & set(bad) and g["n_pairs_ok"] + g["n_pairs_broken"] == n - len(bad) and g["n_reads"] == n - len(bad)
        for u in bad:
            assert us["valid"][u] == 0 and all(not v.reshape(n, -1)[u].any() for v in us.values())
    if f["unpaired"]:
        assert (g["pos_mate"] == 1).all() and (g["read_distance"] == -1).all() and (g["read_weighted_ok"][1::2] == -1).all() and (g["read_fraction_ok"][1::2] == -1).all()
        assert (g["read_cols_nongap"][1::2] == 0).all() and (g["read_mapq"][1::2] == -1).all() and not g["read_reverse"][1::2].any()
        for (label, Lg, r, kept), (_, Lo, _, _) in zip(ee.column_count_cases(R.M), ee.column_count_cases(R.oM)):          # line 126: n >= min_alignment_columns
            x = R.check(Lg, label, oracle_locus=Lo)
            assert (r in x["read_pair"]) == kept and x["n_pairs_ok"] + x["n_pairs_broken"] == n, label
    R.done(floors_locus=L if f["floors"] else None)


def test_loci(pkg, oracle):
    """Locus descriptions read off the library's own alignment: the overlap test of lines 168-172 with a locus ending on / one level before a mate's first
    level and starting on / one level after its last (use[0] != use[1]: read_cols_nongap 0 for the unused mate, line 194), holes in level_to_exon
    (line 54), a hole right after a level with folded insertion columns, a pair that passes the test without a position (cnt stays 0, line 190), and a locus
    far from every read: zero-size outputs, pos_off == [0]."""
    f = ee.loci(); R = Run(pkg, oracle, f)
    n = f["batch"]["n_pairs"]
    p, up, descs = ee.loci_of(R.pairs, f["max_columns"], n)
    po, upo, descs_o = ee.loci_of(R.opairs, f["max_columns"], n)
    assert (p, up) == (po, upo)
    total = dict.fromkeys(ee.CENSUS_KEYS, 0)
    for (label, L, exp), (_, Lo, _) in zip(descs, descs_o):
        g = R.check(L, label, oracle_locus=Lo)
        check_locus_expectation(g, p, up, exp, label)
        for k, v in ee.census(R.pairs, R.b, f["max_columns"], L).items():
            total[k] += v
    R.unit_stats()
    R.done(census=total)


def test_thresholds(pkg, oracle):
    """The pair test of lines 162-164 met with equality and missed by the least amount: |dist - mean| == 5 sd, mate_mapq[2p] == min_mapq (mate 1 alone is
    tested), min(w) == min_weighted_ok, strands_valid == 0.  The thresholds are read off the library's own pairs (the oracle's call gets the oracle's)."""
    f = ee.thresholds(); R = Run(pkg, oracle, f)
    n = f["batch"]["n_pairs"]
    for (label, L, p, kept), (_, Lo, po, _) in zip(ee.threshold_cases(R.M), ee.threshold_cases(R.oM)):
        assert p == po, label
        g = R.check(L, label, oracle_locus=Lo)
        assert (p in g["read_pair"]) == kept, (label, p)
        assert g["n_pairs_ok"] + g["n_pairs_broken"] == n, label
    R.unit_stats()
    R.done(floors_locus=ee.whole(-100.0, 20.0))


@pytest.mark.parametrize("n", ee.SIZES)
def test_sizes(pkg, oracle, n):
    """n_pairs on both sides of the 128-thread block (line 108) and of the scan over n_pairs + 1 triples, under no mask, all ones, all zero (nothing
    counted: line 110 comes before the pair test), the last pair alone and pairs 127 / 128 alone: the accepted pairs land in ascending order with
    contiguous pos_off / geno_off."""
    f = ee.sizes(n); R = Run(pkg, oracle, f)
    out = {}
    for label, mask in ee.size_masks(n):
        out[label] = R.check(ee.whole(-100.0, 20.0, pair_mask=mask), label)
    check_size_outcomes(out, n)
    L = ee.whole(-100.0, 20.0)
    R.unit_stats()
    R.capacity(L, out["no mask"])
    identical(R.library(L), out["no mask"], "sizes %d: the same call again" % n)
    R.done(floors_locus=L)
