"""The typer pinned to the REFERENCE's own HLATyper.cpp (CPU; oracle/_ref/libhlala_ref.so built from a checkout of the reference by oracle/ref/Makefile).

Per family of tests/ref_typer.py the oracle aligns the sample (pinned by test_reference_pin_pipeline.py), then
  * the includeInHLA decision is HLATyper::intervalOverlapsWithGenes on the first and last level of every alignment;
  * the oracle's exon_positions of every locus is compared field by field with the reference's oneReadAlignment_2_exonPositions_paired,
    alignmentWeightedOKFraction, alignmentFractionOK and removeDoublePositionsFromRead (ref_typer_exon_positions): integers and characters exactly, doubles
    exactly;
  * the product's CPU chain (oracle filter_positions -> exon_loglik -> pair_loglik -> call_locus, k-mer presence, the host writer) writes the files of hla/
    for the reference's 17 loci in its order, HLATyper::HLATypeInference writes them from the same alignments (one OpenMP thread: with more, the order of
    its pair table and with it every tie depends on thread timing), and every file is compared BYTE FOR BYTE.  Both sides are host libm summing in the same
    order and printing through the same stream rules; the one normalisation is the sign of a printed NaN (tests/test_typer_files.py).
The p column of R1_columnIncompatibilities is pinned up to the formula of the chi-squared stand-in (oracle/ref/standin/boost/math/distributions/chi_squared.hpp).

Floors are asserted on the reference's own files so that no family passes vacuously.  The module skips, with the reason, only where test_reference_pin.py
skips: neither oracle/_ref/libhlala_ref.so nor the reference sources exist."""
import ctypes as C

import numpy as np
import pytest

import exonpos_edge_cases as ee
import exonpos_reference as er
import oracle_binding as ob
import ref_binding as rb
import ref_typer as rt


@pytest.fixture(scope="module")
def ref():
    ok, why = rb.available()
    if not ok:
        pytest.skip(why)
    return rb


class OracleBackend:
    """the per-locus chain of the product on the CPU: every step is the oracle's"""

    def __init__(self, pkg, case, pairs, include):
        self.pkg, self.case, self.pairs, self.include = pkg, case, pairs, np.asarray(include, np.uint8)
        self.b = case["batch"]; self.per = 2 if case["paired"] else 1; self.n = int(self.b["n_pairs"])
        self._kmers = None; self.filter_stats = []

    def _reverse(self, e):
        rev = np.asarray(self.b["chain_reverse"], np.uint8)[np.asarray(self.pairs["best_chain"])]
        out = np.zeros(2 * e["n_reads"], np.uint8)
        if self.case["paired"]:
            out[:] = rev.reshape(-1, 2)[e["read_pair"]].reshape(-1)
        else:
            out[0::2] = rev[:self.n][e["read_pair"]]
        return out

    def exon_positions(self, L, mask=True, insert=None):
        b = self.b; ins = insert or ((b["insert_mean"], b["insert_sd"]) if self.case["paired"] else (0.0, 0.0))
        e = ob.exon_positions(self.pairs, b, self.case["stride"], L.level_min, L.level_to_exon, ins[0], ins[1], pair_mask=self.include if mask else None,
                              unpaired=not self.case["paired"])
        e["read_reverse"] = self._reverse(e)
        return e

    def filter(self, e, prm):
        use, ign, st = ob.filter_positions(e, prm)
        self.filter_stats.append(st)
        return use

    def type(self, xin):
        LL, M = ob.exon_loglik(xin, 1 if self.case["long_mode"] else 0)
        pl = ob.pair_loglik(LL, M)
        return pl[0], pl[1], pl[2], ob.call_locus(*pl)

    def kmers(self, queries):
        if self._kmers is None:
            self._kmers = rt.kmer_index(self.b, np.nonzero(self.include)[0], self.per)
        return np.asarray([1 if rt.canonical(q) in self._kmers else 0 for q in queries], np.uint8)

    def unit_stats(self):
        """hlala_unit_alignment_stats on the CPU: strands, distance, fraction OK and columns from the columns of the selected alignments; the weighted-OK
        fractions are the oracle's (its exon_positions over a "locus" of all levels returns them for every pair with valid strands; the others print none)."""
        n, per, st, pr = self.n, self.per, self.case["stride"], self.pairs
        us = dict(valid=(np.asarray(pr["pair_status"])[:n] == 0).astype(np.uint8), strands_valid=np.zeros(n, np.uint8), distance=np.zeros(n, np.int32), fraction_ok=np.zeros(2 * n),
                  weighted_ok=np.zeros(2 * n), n_columns=np.zeros(2 * n, np.int32), mate_mapq=np.zeros(2 * n))
        fl = rt.first_last_levels(pr, per * n, st)
        for u in range(n):
            for m in range(per):
                r = per * u + m; k = int(pr["n_cols"][r]); g = pr["col_gchar"][r * st:r * st + k]; s = pr["col_schar"][r * st:r * st + k]
                both = (g == ord("_")) & (s == ord("_"))
                us["fraction_ok"][2 * u + m] = ((g == s) & ~both).sum() / (~both).sum(); us["n_columns"][2 * u + m] = k; us["mate_mapq"][2 * u + m] = pr["mate_mapq"][r]
            if per == 2:
                a, z = fl[2 * u], fl[2 * u + 1]
                us["distance"][u] = z[0] - a[1] - 1 if a[0] < z[0] else a[0] - z[1] - 1
                us["strands_valid"][u] = pr["strands_valid"][u]
        nl = int(self.case["world"]["graph"]["n_levels"])

        class Whole:
            level_min = 0; level_to_exon = np.arange(nl, dtype=np.int32)
        e = self.exon_positions(Whole, mask=False, insert=(0.0, 1e12))
        for i, u in enumerate(e["read_pair"]):
            us["weighted_ok"][2 * u] = e["read_weighted_ok"][2 * i]
            if per == 2:
                us["weighted_ok"][2 * u + 1] = e["read_weighted_ok"][2 * i + 1]
        return us


def compare_exon_positions(eo, er, label):
    """oracle against reference (tests/ref_typer.py: reference_run), every field"""
    assert eo["n_reads"] == er["n_reads"] and eo["n_pos"] == er["n_pos"] and eo["n_chars"] == er["n_chars"], (label, eo["n_reads"], er["n_reads"], eo["n_pos"], er["n_pos"])
    assert (eo["n_pairs_ok"], eo["n_pairs_broken"]) == (er["n_pairs_ok"], er["n_pairs_broken"]), label
    for k in ("read_pair", "pos_off", "pos_exon", "pos_level", "pos_mate", "pos_novel_gap", "geno_off", "geno_chars", "qual_chars", "read_distance"):
        assert np.array_equal(eo[k], er[k]), (label, k)
    for k in ("read_weighted_ok", "read_fraction_ok"):                      # doubles: exactly equal
        assert np.array_equal(eo[k], er[k]), (label, k, np.abs(eo[k] - er[k]).max())
    # mapQ_position is PhredToPCorrect of the character the alignment carries; the oracle keeps the character
    if eo["n_pos"]:
        p = np.zeros(eo["n_pos"]); q = np.ascontiguousarray(eo["pos_mapq"], np.uint8)
        ob.lib().orc_phred(int(eo["n_pos"]), None, None, q.ctypes.data_as(ob.P.c_u8p), p.ctypes.data_as(ob.P.c_f64p))
        assert np.array_equal(p, er["pos_mapq_p"]) and np.array_equal(p, rt.PHRED_TO_P_CORRECT[q]), (label, "pos_mapq")
    # per-mate fields a position of the entry witnesses (the reference keeps them per position only)
    seen = er["read_cols_nongap"] != -1
    assert seen.reshape(-1, 2).any(1).all(), label
    assert np.array_equal(eo["read_cols_nongap"][seen], er["read_cols_nongap"][seen]), (label, "read_cols_nongap")
    assert np.array_equal(eo["read_mapq"][seen], er["read_mapq"][seen]), (label, "read_mapq")
    assert np.array_equal(eo["read_reverse"][seen], er["read_reverse"][seen]) and (er["read_reverse"][~seen] == 255).all(), (label, "read_reverse")


@pytest.mark.parametrize("family", list(rt.FAMILIES))
def test_family_matches_the_reference(pkg, oracle, ref, tmp_path, family):
    case = rt.build_case(family); w = case["world"]; b = case["batch"]; st = case["stride"]
    n = int(b["n_pairs"]); per = 2 if case["paired"] else 1
    gdir = tmp_path / "graph"; rt.write_graph_dir(gdir, case)
    lib = C.CDLL(pkg.LIB_PATH)
    o = oracle(w["graph"], w["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=5, long_read_mode=1 if case["long_mode"] else 0, max_columns=st)
    pairs = (o.align_batch(b) if case["paired"] else o.align_long_reads(b))["pairs"]
    assert (np.asarray(pairs["pair_status"])[:n] == 0).all()
    # ---- the loci as the product reads them from the graph directory
    T = pkg.Typer(lib, gdir); genes = T.genes()
    gf = np.asarray([g[1] for g in genes], np.int32); gl = np.asarray([g[2] for g in genes], np.int32)
    assert sorted(g[0] for g in genes) == sorted(("HLA-" if l in rt.TWO_EXONS else "") + l for l in rt.LOCI)
    loci = {}
    for locus in rt.LOCI:
        L = T.locus(locus); loci[locus] = (L.level_min, L.level_to_exon); L.free()
    T.close()
    R = rt.reference_run(ref, case, gdir, pairs, tmp_path, loci)
    # ---- includeInHLA
    n_cov = int(w["graph"]["n_levels"]) - 1
    if case["paired"]:
        _, inc = ob.postprocess_pairs(pairs, n, st, gf, gl, n_cov)
    else:               # the oracle's postprocess takes pairs; for single reads the interval test is stated here
        fl = rt.first_last_levels(pairs, n, st)
        inc = ((fl[:, :1] <= gl[None, :]) & (fl[:, 1:] >= gf[None, :])).any(1).astype(np.uint8)
    assert np.array_equal(inc, R["include"])
    assert 0 < inc.sum() < n                                                      # floor: pairs included > 0 and < all
    # ---- exon positions, per locus and field
    be = OracleBackend(pkg, case, pairs, inc)

    class Desc:
        pass
    n_entries = 0; counts = dict.fromkeys(ee.CENSUS_KEYS, 0)
    ins = (b["insert_mean"], b["insert_sd"]) if case["paired"] else (0.0, 0.0)
    walk = er.Model(pairs, b, st, rt.PHRED_TO_P_CORRECT, unpaired=not case["paired"])
    for locus in rt.LOCI:
        D = Desc(); D.level_min, D.level_to_exon = loci[locus]
        eo = be.exon_positions(D)
        compare_exon_positions(eo, R["exon"][locus], (family, locus))
        n_entries += eo["n_reads"]
        # what the exon-position stage meets in this family (tests/exonpos_edge_cases.py: census; the counts are recorded in DESIGN.md)
        for k, v in ee.census(pairs, b, st, er.make_locus(D.level_min, D.level_to_exon, ins[0], ins[1], pair_mask=inc), unpaired=not case["paired"], model=walk).items():
            counts[k] += v
    print("census of %s over its %d loci: %s" % (family, len(rt.LOCI), {k: v for k, v in counts.items() if v}))
    assert n_entries > 20
    # ---- the files
    out_p = tmp_path / "product"
    res, _ = rt.write_product_files(pkg, lib, case, gdir, out_p, be, inc)
    got = rt.read_files(out_p); want = R["files"]                                 # no locus and no file may be missing on either side
    bad = [fn for fn in want if rt.normalise(fn, got[fn]) != rt.normalise(fn, want[fn])]
    assert not bad, "\n".join("%s: %s" % (fn, rt.first_difference(got[fn], want[fn])) for fn in bad[:6])
    check_floors(family, want, res, be.filter_stats)
    # ---- the committed fixture is what the reference writes today
    fx = rt.load_fixture(family)
    assert fx["sha"] == ref.sources_hash(pipeline=True), "tests/golden/ref_typer_%s.npz was written from other reference sources: python tests/golden/make_ref_golden_typer.py" % family
    assert fx["digest_full"] == rt.rows_digest(R["rows"]) and np.array_equal(fx["include"], R["include"])
    assert fx["files"] == want
    for locus in rt.LOCI:
        for k in rt.EXON_KEYS:
            assert np.array_equal(fx["exon"][locus][k], R["exon"][locus][k]), (locus, k)


def check_floors(family, want, res, filter_stats):
    """on the REFERENCE's files"""
    F = rt.FAMILIES[family]
    piled = {l: rt.pileup_stats(want["R1_pileup_%s.txt" % l]) for l in rt.LOCI}
    for l in F.get("typed", F["cover"]):
        assert piled[l][0] > 0, (family, l)                                       # piled positions per locus with reads
    if family != "long":                                                          # (a long read covers most of the short graph of that family)
        assert any(piled[l][0] == 0 for l in rt.LOCI), family                     # a locus with zero reads
    bg = rt.bestguess_rows(want["R1_bestguess.txt"])
    assert len(bg) == 2 * len(rt.LOCI)
    if family == "het":
        assert any(int(r[10]) > 0 for r in bg), "no NColumns_UnaccountedAllele > 0"
        assert res["A"]["n_clusters"] % 4 != 0
        called = {r[0]: set() for r in bg}
        for r in bg:
            called[r[0]].add(r[2])
        for l in ("A", "B", "DQA1"):
            assert len(called[l]) == 2, (l, called[l])                            # heterozygous calls
    if family == "wide":
        assert res["C"]["n_clusters"] > 256 and len(set(np.asarray(res["C"]["pair_ll"]).tolist())) >= 6
    if family == "ties":
        assert max(rt.pp_top_ties(want["R1_PP_%s_pairs.txt" % l]) for l in F["cover"]) >= 3
        assert rt.pp_tied_ll_other_mismatches(want["R1_PP_DRB1_pairs.txt"]) >= 2  # equal LL, different Mismatches_avg: the second sort key decides
        pl, ma = np.asarray(res["DRB1"]["pair_ll"]), np.asarray(res["DRB1"]["mis_avg"])
        assert max(len(set(ma[pl == v].tolist())) for v in set(pl.tolist())) >= 3  # ... and equal to the bit, not only in the printed digits
    if family == "indels":
        assert sum(piled[l][1] for l in rt.LOCI) > 0 and sum(piled[l][2] for l in rt.LOCI) > 0
    if family == "long":
        summ = want["summaryStatistics.txt"].decode()
        total = int(summ.split("(unpaired) alignments:")[1].split()[0]); long_enough = int(summ.split("Alignments with length >= 1000:")[1].split()[0])
        assert 0 < long_enough < total                                            # reads rejected for length
        assert sum(st["strand_removed_alleles"] for st in filter_stats) > 0 and sum(st["strand_alleles_enough_coverage"] for st in filter_stats) > sum(st["strand_removed_alleles"] for st in filter_stats)
        assert sum(st["high_coverage_removed_alleles"] for st in filter_stats) > 0
        assert any(int(r[10]) > 0 for r in bg), "no NColumns_UnaccountedAllele > 0"
        assert sum(int(np.sum(r["e"]["pos_novel_gap"] >= 2)) for r in res.values()) > 0
    if family == "filters":
        assert sum(st["removed_alleles"] for st in filter_stats) > 0 and sum(st["reads_kicked_out"] for st in filter_stats) > 0
        assert sum(rt.first20_cut_ties(r["e"]) for r in res.values()) > 0         # equal weighted-OK values across the cut of the first 20: std::sort on ties decides
