"""The typer on the device against the REFERENCE's own HLATyper.cpp, from fixtures alone.

tests/golden/ref_typer_<family>.npz hold what hla::HLATyper (built from a checkout of the reference, oracle/ref/) makes of the sample families of
tests/ref_typer.py: its include decision, its exon positions per locus and the files HLATypeInference writes, byte for byte (written by
tests/golden/make_ref_golden_typer.py; tests/test_reference_pin_typer.py checks on the CPU that they are what the reference writes).  Nothing here reads
the reference or its library.

Per family the world, the sample and the graph directory are rebuilt from the seeds, the sample is aligned on the device and the alignments are held against
the digest of what the reference was fed (a mismatch there is a failure of the ALIGNMENT, reported as such).  Then set_gene_intervals / postprocess,
exon_positions, the host filters, exon_loglik, pair_loglik, call_locus -- and the same through type_locus --, kmer_presence, the writer and the summary:
  exon_positions  exactly the reference's arrays, except the posteriors (device exp) at the rtol = 1e-9, atol = 1e-15 of tests/test_typer_chain.py;
  the files       byte for byte where no field descends from a device exp / log; LL and P of R1_PP_*, Q1 of the best-guess files and the mapping
                  qualities of the pile-up as numbers, with the margins and the order rules of tests/ref_typer.py (compare_pairs_file);
  the call        the two Allele strings per locus exactly."""
import ctypes as C

import numpy as np
import pytest

import ref_typer as rt

pytestmark = pytest.mark.gpu


class DeviceBackend:
    """the per-locus chain of the product on the device"""

    def __init__(self, pkg, lib, case, ctx, gb, include):
        self.pkg, self.lib, self.case, self.ctx, self.gb, self.include = pkg, lib, case, ctx, gb, include
        self.b = case["batch"]

    def exon_positions(self, L):
        ins = (self.b["insert_mean"], self.b["insert_sd"]) if self.case["paired"] else (0.0, 0.0)
        return self.gb.exon_positions(L.level_min, L.level_to_exon, ins[0], ins[1], pair_mask=self.include)

    def filter(self, e, prm):
        return self.pkg.filter_positions(self.lib, e, prm)[0]

    def type(self, xin):
        LL, M = self.ctx.exon_loglik(xin)
        pl = self.ctx.pair_loglik(LL, M)
        call = self.ctx.call_locus(*pl)
        t = self.ctx.type_locus(xin)                     # the three steps in one call: every output bit for bit what the three calls return
        assert np.array_equal(t["LL"], LL) and np.array_equal(t["mism"], M)
        for a, b in zip((t["pairLL"], t["misAvg"], t["misMin"]), pl):
            assert np.array_equal(a, b)
        for k in ("order", "p_normalized", "cluster_marginal"):
            assert np.array_equal(t[k], call[k]), k
        for k in ("first_cluster", "second_cluster", "first_marginal", "second_p", "ll_max", "max_pair", "n_sort_ties"):
            assert t[k] == call[k], k
        return pl[0], pl[1], pl[2], call

    def kmers(self, queries):
        return self.ctx.kmer_presence(self.gb, queries, 31, self.include) if len(queries) else np.zeros(0, np.uint8)

    def unit_stats(self):
        return self.gb.unit_stats()


@pytest.mark.parametrize("family", list(rt.FAMILIES))
def test_device_typer_matches_reference_fixture(pkg, tmp_path, family):
    fx = rt.load_fixture(family)
    case = rt.build_case(family); w = case["world"]; b = case["batch"]
    assert rt.family_params(family) == fx["params"], "tests/golden/ref_typer_%s.npz was written for other parameters of the family" % family
    gdir = tmp_path / "graph"; rt.write_graph_dir(gdir, case)
    lib = C.CDLL(pkg.LIB_PATH)
    ctx = pkg.Context(w["graph"], w["contigs"], insert_mean=b["insert_mean"] or 200.0, insert_sd=b["insert_sd"] or 35.0, rng_seed=5, long_read_mode=1 if case["long_mode"] else 0,
                      max_columns=case["stride"])
    gb = ctx.batch(b) if case["paired"] else ctx.batch_unpaired(b)
    gb.align()
    assert gb.stats().n_errors == 0
    pairs = gb.pairs()
    T = pkg.Typer(lib, gdir); genes = T.genes(); T.close()
    ctx.set_gene_intervals([g[1] for g in genes], [g[2] for g in genes])
    include = gb.postprocess()
    # ---- the alignments are the ones the reference was fed
    assert np.array_equal(include, fx["include"]), "ALIGNMENT (or includeInHLA) differs from what the reference was fed"
    units = np.nonzero(include)[0]
    rows = rt.typer_rows(case, pairs, units)
    assert rt.rows_digest(rows, exact_only=True) == fx["digest_exact"], "ALIGNMENT differs from what the reference was fed (columns, strands or per-position qualities)"
    assert np.allclose(rows["row_mapq"], fx["row_mapq"], rtol=1e-9, atol=1e-15), "ALIGNMENT: mapping qualities differ from what the reference was fed"
    if case["paired"]:
        assert np.allclose(rows["unit_mapq"], fx["unit_mapq"], rtol=1e-9, atol=1e-15), "ALIGNMENT: pair mapping qualities differ from what the reference was fed"
    # ---- the chain and the files
    be = DeviceBackend(pkg, lib, case, ctx, gb, include)
    out = tmp_path / "product"
    res, _ = rt.write_product_files(pkg, lib, case, gdir, out, be, include)
    for locus in rt.LOCI:
        eg, er = res[locus]["e"], fx["exon"][locus]
        for k in rt.EXON_COUNTS:
            assert eg[k] == er[k], (locus, k, eg[k], er[k])
        for k in ("read_pair", "pos_off", "pos_exon", "pos_level", "pos_mate", "pos_novel_gap", "geno_off", "geno_chars", "qual_chars", "read_distance", "read_weighted_ok", "read_fraction_ok"):
            assert np.array_equal(eg[k], er[k]), (locus, k)
        seen = er["read_cols_nongap"] != -1                     # per-mate fields the reference keeps per position only: -1 where no position witnesses them
        assert np.array_equal(eg["read_cols_nongap"][seen], er["read_cols_nongap"][seen]) and np.array_equal(eg["read_reverse"][seen], er["read_reverse"][seen]), locus
        assert np.allclose(eg["read_mapq"][seen], er["read_mapq"][seen], rtol=1e-9, atol=1e-15), locus              # posteriors: device exp()
        assert np.array_equal(rt.PHRED_TO_P_CORRECT[eg["pos_mapq"]], er["pos_mapq_p"]), (locus, "pos_mapq")        # mapQ_position of the character the device keeps
    got = rt.read_files(out); want = fx["files"]
    bad = rt.compare_device_files(got, want)
    assert not bad, "\n".join(bad[:8])
    # ---- the call, with no escape
    gr, wr = rt.bestguess_rows(got["R1_bestguess.txt"]), rt.bestguess_rows(want["R1_bestguess.txt"])
    assert [(r[0], r[1], r[2]) for r in gr] == [(r[0], r[1], r[2]) for r in wr]
