"""Shared by the typer pin (tests/test_reference_pin_typer.py), its fixtures (tests/golden/make_ref_golden_typer.py) and the GPU test over them
(tests/test_gpu_reference_pin_typer.py): the sample families, the graph directory with gene segments for the reference's 17 loci, the per-locus chain of
the product (exon positions -> filters -> likelihoods -> all pairs -> call -> k-mers -> result files) over a backend (oracle on the CPU, kernels on the GPU),
and the comparison rules for the files.  Needs numpy and the package only; nothing here reads the reference."""
import hashlib
import io
import json
import lzma
import math
import os
import zipfile

import numpy as np

from tools import synth
import ref_pipeline as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_FILE = os.path.join(ROOT, "tests", "golden", "hla_nom_g.txt")
# loci_for_HLAtyping in the reference's order (hla/HLATyper.cpp:42) and the loci with two exons in fill_loci_2_exons (:2812-2846)
LOCI = ["A", "B", "C", "DQA1", "DQB1", "DRB1", "DPA1", "DPB1", "DRA", "DRB3", "DRB4", "E", "F", "G", "H", "K", "V"]
TWO_EXONS = {"A", "B", "C", "E", "F", "G", "H", "K", "V"}
FILES_PER_LOCUS = ("R1_pileup_%s.txt", "R1_readIDs_%s.txt", "R1_PP_%s_pairs.txt", "R1_columnIncompatibilities_%s.txt")
FILES_ONCE = ("summaryStatistics.txt", "histogram_matchesPerRead.txt", "R1_bestguess.txt", "R1_bestguess_G.txt", "R1_parameters.txt")
NUC = np.frombuffer(b"ACGT", np.uint8)
# Utilities::PhredToPCorrect per character (Utilities.cpp:357-377; host libm, the arithmetic of tests/test_typer_files.py), for characters from '!' on
PHRED_TO_P_CORRECT = np.asarray([-1.0 if q < 33 else 1 - math.exp(math.log(10.0) * ((q - 33) / -10.0)) for q in range(256)])

# ------------------------------------------------------------------ families
# exon: columns per exon of a locus (default `exon`); allele_n: allele rows per locus (default `alleles`); cover: share of the generated pairs over a locus that
# is kept (a locus not named gets no reads at all; a pair with mates over several loci is kept with the smallest of their shares), pad_p: the share kept outside the genes.
FAMILIES = {
    # heterozygous at A, B and DQA1 with coverage >= 40 there; A has a cluster count that is no multiple of 4 (k_pair_loglik tiles 4 x 256).  DRB1 is 8 columns wide under coverage >= 100, and at A, B, DQA1 and DRB1 one allele of the sample is not in the graph:
    # in short-read mode the reference counts unaccounted alleles only at positions the high-coverage stage has seen (>= highCoverage_minCoverage = 100 reads,
    # hla/HLATyper.cpp:1806-1822), so DRB1 is where NColumns_UnaccountedAllele becomes positive.
    "het": dict(world=dict(seed=101, n_mut=5, n_largegap=1, mut_density=0.03, gap_frac=0.1), batch=dict(seed=102, n_pairs=4000, read_len=100, ins_mean=40.0, ins_sd=12.0),
                haps=(1, 3), exon=6, exons={"A": 38, "B": 36, "DQA1": 40, "C": 30, "DRB1": 8}, alleles=3, allele_n={"A": 34, "B": 14, "DQA1": 9, "C": 12, "DRB1": 7},
                cover={"A": 0.36, "B": 0.36, "DQA1": 0.36, "DRB1": 1.0, "C": 0.04, "E": 0.05}, pad_p=0.03, select_seed=103, novel=("A", "B", "DQA1", "DRB1"), force_het=("A", "B", "DQA1", "DRB1")),
    # homozygous, low coverage, and no read over exon 3 of A, where a share of its alleles carry their only difference: clusters identical on the covered
    # columns, exactly equal pair likelihoods at the top.  DRB1 carries three DISTANT alleles: the sample's allele with substitutions in columns 8-14 and 17-23
    # of its exon, and in 0, 1 or 2 of the columns 15-16 between them.  A read that reaches one of the middle columns has crossed seven substituted ones, each
    # costing about -8 in the log-likelihood, and Utilities::logAvg (Utilities.cpp:1368-1379) of the sample's allele and such an allele is exactly log(0.5) + a
    # once b - a < -36.7 (1 + exp(b - a) rounds to 1): pairs of the sample's allele with the three have log-likelihoods equal to the bit and different
    # Mismatches_avg, which is where the second key of the pair sort decides
    "ties": dict(world=dict(seed=111, n_mut=4, n_largegap=0, mut_density=0.02, gap_frac=0.0), batch=dict(seed=112, n_pairs=1000, read_len=100, ins_mean=120.0, ins_sd=20.0),
                 haps=(2,), exon=6, exons={"A": 50, "B": 44, "DQB1": 40, "DRB1": 32}, alleles=2, allele_n={"A": 26, "B": 18, "DQB1": 11, "DRB1": 9}, dup_frac=0.0, mut_per_allele=1,
                 cover={"A": 0.8, "B": 0.5, "DQB1": 0.5, "DRB1": 0.8}, pad_p=0.03, select_seed=113, blind={"A": 1}, distant={"DRB1": 3}),
    # the same with reads over C alone, which has more than 256 clusters (k_pair_loglik tiles 4 x 256): every allele differs from the others in the uncovered
    # exon, half of them also in one of six (column, base) choices of the covered one, so that the table holds a few dozen distinct values in an order the cluster
    # numbering does not follow.  A family of its own with short allele names because the all-pairs file of such a locus fills a fixture: its 33 thousand lines
    # come in the order std::sort leaves tied keys in, which does not compress
    "wide": dict(world=dict(seed=151, n_mut=4, n_largegap=0, mut_density=0.02, gap_frac=0.0), batch=dict(seed=152, n_pairs=3000, read_len=60, ins_mean=30.0, ins_sd=10.0, clip_max=10, indel_read_frac=0.0),
                 haps=(2,), exon=6, exons={"C": 60}, alleles=2, allele_n={"C": 290}, dup_frac=0.0, short_names=("C",),
                 cover={"C": 1.0}, pad_p=0.01, select_seed=153, blind={"C": 1}, wide=("C",)),
    # alleles with '_' columns and '*' stretches, reads with insertions and deletions, mates that overlap (removeDoublePositionsFromRead)
    "indels": dict(world=dict(seed=121, n_mut=5, n_largegap=1, mut_density=0.04, gap_frac=0.5), batch=dict(seed=122, n_pairs=900, read_len=100, ins_mean=-50.0, ins_sd=15.0, indel_read_frac=0.6),
                   haps=(1, 2), exon=6, exons={"A": 46, "C": 40, "DRB1": 44}, alleles=3, allele_n={"A": 22, "C": 13, "DRB1": 10}, gap_alleles=True,
                   cover={"A": 1.0, "C": 1.0, "DRB1": 0.3, "G": 0.3}, pad_p=0.2, select_seed=123),
    # a third allele in a twentieth of the reads over covered columns: kick-outs of the first-20 filter, ignored reads, std::sort on tied weighted-OK values
    "filters": dict(world=dict(seed=131, n_mut=5, n_largegap=0, mut_density=0.05, gap_frac=0.05), batch=dict(seed=132, n_pairs=1500, read_len=100, ins_mean=120.0, ins_sd=20.0, qual_lo=20),
                    haps=(1,) * 19 + (2,) * 19 + (4,) * 2, exon=6, exons={"A": 50, "B": 46}, alleles=3, allele_n={"A": 18, "B": 12},
                    cover={"A": 1.0, "B": 1.0, "DPB1": 0.5}, pad_p=0.1, select_seed=133),
    # unpaired reads with long-read error rates, longReadsMode set: insertionP / deletionP 0.075, the high-coverage filter from coverage 1 at frequency 0.15, the
    # strand filter (a tenth of the reads are on the reverse strand, so that alleles seen >= 100 times have a rarer-strand share around the threshold 0.1),
    # positions inside novel gaps of two or more columns, reads with fewer than 1000 alignment columns.  The graph is short and the exons tiny because nearly every
    # read covers every locus: the pile-up files decide the size of the fixture.
    "long": dict(world=dict(seed=141, n_mut=3, n_largegap=0, mut_density=0.02, gap_frac=0.2), long=dict(seed=142, n_reads=165, len_lo=930, len_hi=1330, sub=0.03, ins=0.025, dele=0.025, clip_max=20),
                 haps=(1, 2), exon=2, exons={"A": 14, "DQA1": 9}, alleles=3, allele_n={"A": 11, "DQA1": 6}, layout=(260, 14), n_short=20, p_reverse=0.10, strand_seed=143, novel=("A",), force_het=("A",),
                 cover={l: 1.0 for l in LOCI}, typed=("A", "B")),
}


def g_file_names():
    """allele names per locus from the G-group file: the first name of every line, so that neighbouring names fall into different groups."""
    out = {}
    with open(G_FILE) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            loc, names, _ = line.rstrip("\n").split(";")
            out.setdefault(loc[:-1], []).append(loc + names.split("/")[0])
    return out


def concat_unpaired(a, b):
    """two unpaired batches as one"""
    n = dict(a); n["n_pairs"] = a["n_pairs"] + b["n_pairs"]; n["n_chains"] = a["n_chains"] + b["n_chains"]
    for k, last in (("read_off", len(a["read_bases"])), ("chain_off", a["n_chains"]), ("cigar_off", len(a["cigar"]))):
        n[k] = np.concatenate([a[k], np.asarray(b[k][1:]) + last]).astype(np.int32)
    n["read_primary"] = np.concatenate([a["read_primary"], np.asarray(b["read_primary"]) + a["n_chains"]]).astype(np.int32)
    for k in ("read_bases", "read_quals", "chain_contig", "chain_pos", "chain_offset", "chain_as", "chain_reverse", "cigar"):
        n[k] = np.concatenate([a[k], b[k]]).astype(np.asarray(a[k]).dtype)
    return n


def build_case(family):
    """World, sample and gene layout of a family, from its seeds alone."""
    F = FAMILIES[family]
    # ---- layout: padding, then per locus [intron][exon 2][intron][exon 3][intron], levels of a make_world graph
    end_pad, pad = F.get("layout", (420, 260))
    pos = end_pad; genes = {}; segs = []
    def seg(kind, a, b, locus=None, exon=None):
        if b > a:
            segs.append(dict(kind=kind, a=a, b=b, locus=locus, exon=exon))
    seg("pad", 0, pos)
    for li, locus in enumerate(LOCI):
        n = F.get("exons", {}).get(locus, F["exon"] + li % 3)
        g0 = pos; ex = []
        seg("intron", pos, pos + 12, locus, 1); pos += 12
        for k in range(2 if locus in TWO_EXONS else 1):
            ln = n + 3 * k
            seg("exon", pos, pos + ln, locus, 2 + k); ex.append((pos, pos + ln)); pos += ln
            seg("intron", pos, pos + 18, locus, 2 + k); pos += 18
        genes[locus] = dict(first=g0, last=pos - 1, exons=ex)
        seg("pad", pos, pos + pad); pos += pad
    seg("pad", pos, pos + end_pad); pos += end_pad
    G = pos
    wk = dict(F["world"]); H = synth.make_haplotypes(np.random.default_rng(wk.pop("seed")), G, **wk); nh = H.shape[0]
    for locus in F.get("force_het", ()):           # the two haplotypes of the sample differ in two columns in the middle of the locus' first exon
        h1, h2 = F["haps"][:2]; a, b = genes[locus]["exons"][0]; c = (a + b) // 2
        H[h1, c - 2] = ord("A"); H[h2, c - 2] = ord("C"); H[h1, c + 1] = ord("G"); H[h2, c + 1] = ord("T")
    w = dict(H=H, graph=synth.build_graph(H, 1), contigs=synth.make_contigs(H), G=G)
    # ---- allele rows: the haplotypes, then copies with substitutions (and, gap_alleles, '_' columns and '*' ends), then exact copies
    rng = np.random.default_rng(F["world"]["seed"] + 7)
    pool = g_file_names(); alleles = {}
    for locus in LOCI:
        gi = genes[locus]; n = max(F.get("allele_n", {}).get(locus, F["alleles"]), nh if locus in F["cover"] else 1)
        blind = gi["exons"][F["blind"][locus]] if locus in F.get("blind", {}) else None
        cols = np.concatenate([np.arange(a, b) for a, b in gi["exons"]])
        names = [] if locus in F.get("short_names", ()) else (pool.get(locus) or [])[:n]
        names += ["%s*%02d:%02d" % (locus, 90 + i // 90, 1 + i % 90) for i in range(n - len(names))]
        rows = []
        for i in range(n):
            if i < nh:
                r = H[i, gi["first"]:gi["last"] + 1].copy()
            elif n - i <= F.get("distant", {}).get(locus, 0):
                a = gi["exons"][0][0] - gi["first"]; r = rows[F["haps"][0]].copy()
                for c in list(range(8, 15)) + list(range(17, 24)) + list(range(15, 15 + (n - 1 - i))):
                    r[a + c] = NUC[(int(np.nonzero(NUC == r[a + c])[0][0]) + 1) % 4]
            elif locus in F.get("wide", ()):
                r = rows[0].copy()
                for c in rng.choice(np.arange(*blind), 2, replace=False):
                    r[c - gi["first"]] = NUC[rng.integers(0, 4)]
                if i % 2:
                    a, b = gi["exons"][0]; v = int(rng.integers(0, 6))
                    r[a + 5 + 9 * (v // 3) - gi["first"]] = NUC[(int(np.nonzero(NUC == rows[0][a + 5 + 9 * (v // 3) - gi["first"]])[0][0]) + 1 + v % 3) % 4]
            elif rng.random() < F.get("dup_frac", 0.15):
                r = rows[int(rng.integers(0, len(rows)))].copy()
            else:
                r = rows[int(rng.integers(0, min(len(rows), nh)))].copy()
                for c in rng.choice(np.arange(*blind) if blind and i % 2 else cols, F.get("mut_per_allele", int(rng.integers(1, 3))), replace=False):
                    r[c - gi["first"]] = NUC[rng.integers(0, 4)]
                if F.get("gap_alleles") and rng.random() < 0.4:
                    r[int(rng.choice(cols)) - gi["first"]] = ord("_")
                if F.get("gap_alleles") and rng.random() < 0.3:
                    a, b = gi["exons"][-1]; r[b - 4 - gi["first"]:b - gi["first"]] = ord("*")
            rows.append(r)
        if locus in F.get("novel", ()):         # the sample carries an allele the graph does not know: at the first exon column where its two haplotypes differ, no row keeps the base of the second
            h1, h2 = F["haps"][:2]
            c = [c for c in cols if H[h1, c] != H[h2, c] and H[h1, c] != ord("_") and H[h2, c] != ord("_")][0] - gi["first"]
            for r in rows:
                if r[c] == H[h2, c + gi["first"]]:
                    r[c] = H[h1, c + gi["first"]]
        alleles[locus] = (names, np.stack(rows))
    # ---- sample
    if "long" in F:
        kw = dict(F["long"]); n = kw.pop("n_reads")
        b = synth.make_long_batch(w, n, haps=F["haps"], **kw)
        kw.update(seed=kw["seed"] + 50, len_lo=60, len_hi=110); n += F["n_short"]
        b = concat_unpaired(b, synth.make_long_batch(w, F["n_short"], haps=F["haps"], **kw))      # short reads: some lie outside every gene, all are too short to be typed
        b["chain_reverse"] = (np.random.default_rng(F["strand_seed"]).random(b["n_chains"]) < F["p_reverse"]).astype(np.uint8)   # bases are in alignment orientation: the strand is a flag
        b["insert_mean"], b["insert_sd"] = 0.0, 0.0
        return dict(family=family, world=w, batch=b, genes=genes, segs=segs, alleles=alleles, G=G, paired=False, long_mode="ont2d",
                    names1=["%s%04d" % (family, i) for i in range(n)], names2=None, stride=2048)
    kw = dict(F["batch"]); n_pairs = kw.pop("n_pairs"); seed = kw.pop("seed")
    b = synth.make_batch(w, n_pairs, seed=seed, haps=F["haps"], **kw)
    rl = int(kw["read_len"]); t0 = np.asarray(b["truth_level0"]).reshape(-1, 2)
    srng = np.random.default_rng(F["select_seed"]); keep = []
    for p in range(n_pairs):
        over = [l for l in LOCI if any(t0[p, m] - 10 <= genes[l]["last"] and t0[p, m] + rl + 10 >= genes[l]["first"] for m in range(2))]
        u = srng.random()
        if not over:
            k = u < F["pad_p"]
        else:
            k = u < min(F["cover"].get(l, 0.0) for l in over)
        for l, x in F.get("blind", {}).items():                # no mate may lie over the blind exon
            a, z = genes[l]["exons"][x]
            k = k and not any(t0[p, m] - 5 <= z and t0[p, m] + rl + 5 >= a for m in range(2))
        if k:
            keep.append(p)
    sb = rp.subset_units(b, keep)
    sb["insert_mean"], sb["insert_sd"] = b["insert_mean"], b["insert_sd"]
    for k in ("read_off", "chain_off", "cigar_off"):
        sb[k] = np.asarray(sb[k], np.int32)
    n = len(keep)
    return dict(family=family, world=w, batch=sb, genes=genes, segs=segs, alleles=alleles, G=G, paired=True, long_mode="",
                names1=["%s%04d/1" % (family, i) for i in range(n)], names2=["%s%04d/2" % (family, i) for i in range(n)], stride=384)


def write_graph_dir(root, case):
    """<root>/PRG with segments.txt, padding segments, gene segments `<n>_gene_<locus>_<m>_(exon|intron)_<N>.txt` for all 17 loci and a graph.txt (the typer only asks
    whether it is readable).  Class-I genes are named HLA-<locus>, the others by the locus alone: find_file_for_exon accepts both."""
    prg = os.path.join(str(root), "PRG"); os.makedirs(prg)
    H = case["world"]["H"]; names = []
    for k, s in enumerate(case["segs"], 1):
        cols = "IndividualID " + " ".join("L%d" % x for x in range(s["a"], s["b"]))
        if s["kind"] == "pad":
            fn = "%d_pad_%d.txt" % (k, k); lines = [cols, "ref " + " ".join(chr(c) for c in H[0, s["a"]:s["b"]])]
        else:
            gene = ("HLA-" if s["locus"] in TWO_EXONS else "") + s["locus"]
            fn = "%d_gene_%s_%d_%s_%d.txt" % (k, gene, k, s["kind"], s["exon"])
            an, rows = case["alleles"][s["locus"]]; g0 = case["genes"][s["locus"]]["first"]
            lines = [cols] + [nm + " " + " ".join(chr(c) for c in r[s["a"] - g0:s["b"] - g0]) for nm, r in zip(an, rows)]
        with open(os.path.join(prg, fn), "w") as f:
            f.write("\n".join(lines) + "\n")
        names.append(fn)
    with open(os.path.join(prg, "segments.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    with open(os.path.join(prg, "graph.txt"), "w") as f:
        f.write("see segments.txt\n")


# ------------------------------------------------------------------ alignments as rows

def first_last_levels(pairs, n_rows, stride):
    """alignment_firstLevel / alignment_lastLevel per row (-1: no level)"""
    fl = np.full((n_rows, 2), -1, np.int32)
    for r in range(n_rows):
        lv = pairs["col_level"][r * stride:r * stride + int(pairs["n_cols"][r])]; lv = lv[lv != -1]
        if len(lv):
            fl[r] = (lv[0], lv[-1])
    return fl


def typer_rows(case, pairs, units):
    """The selected alignments of the given units in the layout ref_typer_reads takes (rows = mates of the units, in order) and the digest over them."""
    b = case["batch"]; per = 2 if case["paired"] else 1; st = case["stride"]
    rows = [per * u + m for u in units for m in range(per)]
    nc = np.asarray(pairs["n_cols"], np.int32)[rows]
    col_off = np.concatenate([[0], np.cumsum(nc)]).astype(np.int32)
    take = np.concatenate([np.arange(r * st, r * st + int(pairs["n_cols"][r])) for r in rows]) if rows else np.zeros(0, np.int64)
    ro = np.asarray(b["read_off"], np.int64)
    rlen = np.asarray([ro[r + 1] - ro[r] for r in rows], np.int64)
    bases = np.concatenate([b["read_bases"][ro[r]:ro[r + 1]] for r in rows]); quals = np.concatenate([b["read_quals"][ro[r]:ro[r + 1]] for r in rows])
    best = np.asarray(pairs["best_chain"]).reshape(-1)[rows]
    nm = [(case["names1"], case["names2"])[m][u] if case["paired"] else case["names1"][u] for u in units for m in range(per)]
    d = dict(n_units=len(units), paired=int(case["paired"]),
             seeds=dict(n_reads=len(rows), read_off=np.concatenate([[0], np.cumsum(rlen)]).astype(np.int32), read_bases=bases.astype(np.uint8), read_quals=quals.astype(np.uint8),
                        n_chains=len(rows), chain_read=np.arange(len(rows), dtype=np.int32), chain_seq_begin=np.zeros(len(rows), np.int32), chain_seq_end=(rlen - 1).astype(np.int32),
                        chain_reverse=np.asarray(b["chain_reverse"], np.uint8)[best], col_off=col_off, col_level=pairs["col_level"][take].astype(np.int32),
                        col_edge=pairs["col_edge"][take].astype(np.int32), col_gchar=pairs["col_gchar"][take].astype(np.uint8), col_schar=pairs["col_schar"][take].astype(np.uint8)),
             col_mapq=pairs["col_mapq"][take].astype(np.uint8), row_mapq=np.asarray(pairs["mate_mapq"], np.float64)[rows],
             unit_mapq=np.asarray(pairs["pair_mapq"], np.float64)[list(units)], primary_reverse=np.asarray(b["chain_reverse"], np.uint8)[np.asarray(b["read_primary"])[rows]],
             names=nm)
    return d


def rows_digest(rows, exact_only=False):
    """SHA-256 over the alignment columns (and, unless exact_only, the mapping qualities) the reference was fed."""
    h = hashlib.sha256()
    s = rows["seeds"]
    for k in ("read_off", "read_bases", "read_quals", "chain_reverse", "col_off", "col_level", "col_edge", "col_gchar", "col_schar"):
        h.update(k.encode()); h.update(np.ascontiguousarray(s[k]).tobytes())
    h.update(np.ascontiguousarray(rows["col_mapq"]).tobytes()); h.update(np.ascontiguousarray(rows["primary_reverse"]).tobytes())
    if not exact_only:
        h.update(np.ascontiguousarray(rows["row_mapq"]).tobytes()); h.update(np.ascontiguousarray(rows["unit_mapq"]).tobytes())
    h.update("\n".join(rows["names"]).encode())
    return h.hexdigest()


# ------------------------------------------------------------------ the product's chain over a backend

def filter_params(pkg, long_mode):
    """The settings HLATypeInference runs with (hla/HLATyper.cpp:67-79; long reads :938-947, and the first-20 filter is skipped, :1509)."""
    if long_mode:
        return pkg.default_filter_params(filter_first20=0, high_coverage_filter=1, high_coverage_min_coverage=1, high_coverage_min_freq=0.15, long_read_strand_filter=1)
    return pkg.default_filter_params()


def canonical(kmer):
    rc = kmer[::-1].translate(str.maketrans("ACGT", "TGCA"))
    return min(kmer, rc)


def kmer_index(batch, units, per, k=31):
    """canonical k-mers of the reads of the given units (the index of hla/HLATyper.cpp:999-1027; orientation does not matter to a canonical k-mer)"""
    idx = set(); ro = batch["read_off"]
    for u in units:
        for m in range(per):
            r = per * u + m; s = bytes(batch["read_bases"][ro[r]:ro[r + 1]]).decode()
            for i in range(len(s) - k + 1):
                idx.add(canonical(s[i:i + k]))
    return idx


def write_product_files(pkg, lib, case, graph_dir, out, backend, include):
    """The reference's 17 loci in its order through `backend` (exon_positions(L) -> e, filter(e, prm) -> use, type(xin) -> (pair_ll, mis_avg, mis_min, call),
    kmers(queries) -> present, unit_stats() -> dict) and the host writer.  Returns per locus (e, use, pair_ll, mis_avg, mis_min, call, L info)."""
    T = pkg.Typer(lib, graph_dir); T.load_g_groups(G_FILE)
    b = case["batch"]; long_mode = bool(case["long_mode"]); prm = filter_params(pkg, long_mode)
    us = backend.unit_stats()
    ins = (float(b["insert_mean"]), float(b["insert_sd"])) if case["paired"] else (0.0, 0.0)
    pkg.typer_begin_output(lib, out)
    pkg.typer_write_summary(lib, out, us, unpaired=not case["paired"], unit_mask=include, insert_mean=ins[0], insert_sd=ins[1])
    res = {}
    for locus in LOCI:
        L = T.locus(locus)
        e = backend.exon_positions(L)
        use = backend.filter(e, prm)
        xin = pkg.exon_in_from_positions(e, use, L.cluster_seq, L.n_clusters, L.n_columns)
        pair_ll, mis_avg, mis_min, call = backend.type(xin)
        kc = []
        for c in (call["first_cluster"], call["second_cluster"]):
            q, total = L.cluster_kmers(c, 31)
            kc.append(-1.0 if total == 0 else float(np.asarray(backend.kmers(q)).sum()) / total)
        co = pkg.CallOut(call["first_cluster"], call["second_cluster"], call["first_marginal"], call["second_p"], call["ll_max"], call["max_pair"], call["n_sort_ties"])
        rep = L.write_files(out, e, case["names1"], case["names2"] if case["paired"] else None, pair_ll, mis_avg, mis_min, call["order"], call["p_normalized"], co,
                            kmers_covered=kc, params=prm, long_read_mode=long_mode, unit_stats=us, unit_mask=include, insert_mean=ins[0], insert_sd=ins[1])
        res[locus] = dict(e=e, use=use, pair_ll=pair_ll, mis_avg=mis_avg, mis_min=mis_min, call=call, n_clusters=L.n_clusters, n_columns=L.n_columns,
                          level_min=L.level_min, level_to_exon=L.level_to_exon, report=rep)
        L.free()
    pkg.typer_end_output(lib, out, LOCI, very_conservative=True)
    genes = T.genes(); T.close()
    return res, genes


def read_files(out):
    """every result file of a directory as bytes, by name; all 9 kinds for all 17 loci must be there"""
    want = list(FILES_ONCE) + [p % l for l in LOCI for p in FILES_PER_LOCUS]
    have = sorted(os.listdir(str(out)))
    assert have == sorted(want), (sorted(set(want) - set(have)), sorted(set(have) - set(want)))
    d = {}
    for fn in want:
        with open(os.path.join(str(out), fn), "rb") as f:
            d[fn] = f.read()
    return d


def normalise(fn, data):
    """the one normalisation of tests/test_typer_files.py: the sign of a printed NaN (0/0 * 100 in summaryStatistics.txt) is a detail of the C library"""
    return data.replace(b"(nan%)", b"(-nan%)") if fn == "summaryStatistics.txt" else data


def first_difference(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return "line %d:\n  got  %r\n  want %r" % (i + 1, x[:300], y[:300])
    return "line counts %d / %d" % (len(la), len(lb))


# ------------------------------------------------------------------ what the reference's files say about a family (floors)

def pp_top_ties(data):
    """size of the group of exactly equal (LL text and P text) lines at the top of an R1_PP file"""
    rows = [l.split("\t") for l in data.decode().splitlines()[1:]]
    n = 0
    while n < len(rows) and rows[n][1:3] == rows[0][1:3]:
        n += 1
    return n


def pileup_stats(data):
    """(piled positions, positions with an insertion: a genotype longer than one character, positions with a deletion: genotype "_")"""
    n = ins = dele = 0
    for line in data.decode().splitlines():
        f = line.split("\t")
        if len(f) < 4 or f[2] == "0":
            continue
        for ent in f[3].split("], "):
            gt = ent.split(" (")[0]
            n += 1; ins += len(gt) > 1; dele += gt == "_"
    return n, ins, dele


def pp_tied_ll_other_mismatches(data):
    """number of neighbouring lines of an R1_PP file with identical LL text and different Mismatches_avg: the second key of the pair sort decided there"""
    rows = [l.split("\t") for l in data.decode().splitlines()[1:]]
    return sum(1 for a, b in zip(rows, rows[1:]) if a[2] == b[2] and a[3] != b[3])


def first20_cut_ties(e):
    """positions (exon columns) of an exon-positions dict with at least 20 alleles whose 20th and 21st largest read-pair weighted-OK value are equal: which
    of the tied reads make the "first 20" is then decided by std::sort on tied keys (hla/HLATyper.cpp:1520-1565)"""
    per = {}
    for r in range(e["n_reads"]):
        w = (e["read_weighted_ok"][2 * r] + e["read_weighted_ok"][2 * r + 1]) / 2.0
        for j in range(e["pos_off"][r], e["pos_off"][r + 1]):
            if PHRED_TO_P_CORRECT[e["pos_mapq"][j]] >= 0.7:
                per.setdefault(int(e["pos_exon"][j]), []).append(w)
    return sum(1 for v in per.values() if len(v) > 20 and sorted(v, reverse=True)[19] == sorted(v, reverse=True)[20])


def bestguess_rows(data):
    return [l.split("\t") for l in data.decode().splitlines()[1:]]


# ------------------------------------------------------------------ the reference's side (the binding is handed in: this module does not load it)

EXON_KEYS = ("read_pair", "read_weighted_ok", "read_fraction_ok", "read_distance", "read_cols_nongap", "pos_off", "pos_exon", "pos_level", "pos_mate", "pos_novel_gap",
             "geno_off", "geno_chars", "qual_chars", "read_reverse", "read_mapq", "pos_mapq_p")
EXON_COUNTS = ("n_reads", "n_pos", "n_chars", "n_pairs_ok", "n_pairs_broken")


def reference_run(rb, case, graph_dir, pairs, work_dir, loci):
    """What the reference makes of the alignments `pairs` of a case: the include decision (intervalOverlapsWithGenes on the first and last level of every
    alignment), per locus of `loci` ({name: (level_min, level_to_exon)}) its exon positions with read_pair mapped back to the units of the batch, and the
    files HLATypeInference writes from the included units."""
    w, b, st = case["world"], case["batch"], case["stride"]; n = int(b["n_pairs"]); per = 2 if case["paired"] else 1
    R = rb.Reference(w["graph"], rng_seed=5, long_read_mode=1 if case["long_mode"] else 0, max_columns=st)
    RT = rb.ReferenceTyper(R, graph_dir)
    fl = first_last_levels(pairs, per * n, st)
    assert (fl[:, 0] >= 0).all()
    include = RT.include(fl[:, 0], fl[:, 1]).reshape(n, per).any(1)                # processBAM.cpp:2114-2133 / :2298-2312 / :2428-2448
    units = np.nonzero(include)[0]
    rows = typer_rows(case, pairs, units)
    ins = (float(b["insert_mean"]), float(b["insert_sd"])) if case["paired"] else (0.0, 0.0)
    exon = {}
    for locus, (level_min, l2e) in loci.items():
        e = RT.exon_positions(rows, level_min, l2e, ins[0], ins[1])
        e["read_pair"] = units[e["read_pair"]].astype(np.int32)
        exon[locus] = e
    gd = os.path.join(str(work_dir), "cwd"); os.makedirs(gd)
    with open(G_FILE, "rb") as f, open(os.path.join(gd, "hla_nom_g.txt"), "wb") as o:
        o.write(f.read())
    out = os.path.join(str(work_dir), "reference")
    RT2 = rb.ReferenceTyper(R, graph_dir)                                          # HLATypeInference changes members in long-read mode: a typer of its own
    RT2.infer(rows, ins[0], ins[1], out, case["long_mode"], gd)
    files = read_files(out)
    RT.close(); RT2.close(); R.close()
    return dict(include=include.astype(np.uint8), units=units, rows=rows, exon=exon, files=files)


# ------------------------------------------------------------------ fixtures tests/golden/ref_typer_<family>.npz

def fixture_path(family):
    return os.path.join(ROOT, "tests", "golden", "ref_typer_%s.npz" % family)


def family_params(family):
    return json.dumps(FAMILIES[family], sort_keys=True, default=list)


def pack_fixture(family, ref, sources_sha256):
    """arrays of a fixture: the family's parameters, the include decision, digests of the alignments the reference was fed (`exact`: columns, strands, reads,
    per-position qualities, names; `full`: plus the mapping qualities) and the mapping qualities themselves, the reference's exon positions per locus, its
    files (one LZMA stream over their concatenation: the pile-up and all-pairs files are megabytes of text) and the hash of the reference's sources."""
    d = {"meta__family": np.asarray(family), "meta__params": np.asarray(family_params(family)), "meta__ref_sources_sha256": np.asarray(sources_sha256),
         "in__include": ref["include"], "in__digest_exact": np.asarray(rows_digest(ref["rows"], exact_only=True)), "in__digest_full": np.asarray(rows_digest(ref["rows"])),
         "in__row_mapq": ref["rows"]["row_mapq"], "in__unit_mapq": ref["rows"]["unit_mapq"]}
    inner = {}
    for locus, e in ref["exon"].items():
        for k in EXON_KEYS:
            inner["%s__%s" % (locus, k)] = e[k]
        inner["%s__counts" % locus] = np.asarray([e[k] for k in EXON_COUNTS], np.int32)
    buf = io.BytesIO(); save_fixture(buf, inner, zipfile.ZIP_STORED)          # the per-read arrays repeat from locus to locus: one LZMA stream over all of them
    d["exon__xz"] = np.frombuffer(lzma.compress(buf.getvalue(), format=lzma.FORMAT_XZ, preset=9 | lzma.PRESET_EXTREME), np.uint8)
    names = sorted(ref["files"])
    d["files__names"] = np.asarray(names); d["files__sizes"] = np.asarray([len(ref["files"][n]) for n in names], np.int64)
    d["files__xz"] = np.frombuffer(lzma.compress(b"".join(ref["files"][n] for n in names), format=lzma.FORMAT_XZ, preset=9 | lzma.PRESET_EXTREME), np.uint8)
    return d


def save_fixture(path, arrays, compression=zipfile.ZIP_DEFLATED):
    """an .npz whose bytes depend on the arrays alone (numpy stamps the members with the time of day)"""
    with zipfile.ZipFile(path, "w", compression) as z:
        for k in sorted(arrays):
            buf = io.BytesIO(); np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)); zi.compress_type = compression; zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def load_fixture(family):
    z = np.load(fixture_path(family))
    names = [str(x) for x in z["files__names"]]; sizes = z["files__sizes"]; blob = lzma.decompress(z["files__xz"].tobytes()); off = np.concatenate([[0], np.cumsum(sizes)])
    exon = {}; zi = np.load(io.BytesIO(lzma.decompress(z["exon__xz"].tobytes())))
    for locus in LOCI:
        e = {k: zi["%s__%s" % (locus, k)] for k in EXON_KEYS}
        e.update(zip(EXON_COUNTS, (int(x) for x in zi["%s__counts" % locus])))
        exon[locus] = e
    return dict(params=str(z["meta__params"]), sha=str(z["meta__ref_sources_sha256"]), include=z["in__include"], digest_exact=str(z["in__digest_exact"]), digest_full=str(z["in__digest_full"]),
                row_mapq=z["in__row_mapq"], unit_mapq=z["in__unit_mapq"], exon=exon, files={n: blob[off[i]:off[i + 1]] for i, n in enumerate(names)})


# ------------------------------------------------------------------ files whose numbers come from a device exp / log

def half_ulp6(text):
    """half a unit of the sixth significant digit of a number printed with the default stream precision"""
    v = abs(float(text))
    if v == 0 or not np.isfinite(v):
        return 0.0
    return 0.5 * 10.0 ** (np.floor(np.log10(v)) - 5)


def close_printed(got, want, rel):
    """Two numbers printed with 6 significant digits, computed from values that agree to `rel` relative: they differ by at most `rel` of their size plus half
    a unit of the sixth digit on either side (each print rounds once)."""
    g, w = float(got), float(want)
    if np.isnan(g) or np.isnan(w):
        return np.isnan(g) and np.isnan(w)
    return abs(g - w) <= rel * max(abs(g), abs(w)) + half_ulp6(got) + half_ulp6(want)


REL = 1e-9          # the project's parity of the device's all-pairs log-likelihoods and posteriors with the host (tests/test_typer.py, tests/test_typer_chain.py)


def compare_pairs_file(got, want):
    """R1_PP_<locus>_pairs.txt of the device chain against the reference's.  ClusterID and Mismatches_avg are compared as text; LL and P descend from the
    device's exp / log and are compared as numbers.  The margin is not free: the device's pairLL agrees with the host's to REL relative, so a printed LL may
    differ by REL * |LL| plus half a unit of the sixth printed digit on either side; P = exp(LL - LLmax) / sum(P) then carries REL * (|LL| + |LLmax|) relative,
    plus the same rounding of the print.
    Order: the file is sorted by LL.  Wherever neighbouring reference LLs differ by more than the margin the order must be the reference's; inside a run of
    LLs equal within the margin the SET of lines is compared.  Inside a group the reference prints as exactly equal (identical LL and P text) the order must
    still be the reference's: that is the tie rule of the sort."""
    G = [l.split("\t") for l in got.decode().splitlines()]; W = [l.split("\t") for l in want.decode().splitlines()]
    assert G[0] == W[0] and len(G) == len(W), "header or line count"
    G, W = G[1:], W[1:]; n = len(W)
    if n == 0:
        return
    llmax = abs(float(W[0][2]))

    def same(g, w):
        return g[0] == w[0] and g[3] == w[3] and close_printed(g[2], w[2], REL) and close_printed(g[1], w[1], REL * (abs(float(w[2])) + llmax))
    i = 0
    while i < n:
        j = i + 1
        while j < n and abs(float(W[j][2]) - float(W[j - 1][2])) <= REL * max(abs(float(W[j][2])), abs(float(W[j - 1][2]))) + half_ulp6(W[j][2]) + half_ulp6(W[j - 1][2]):
            j += 1
        by_id = {g[0]: g for g in G[i:j]}
        assert len(by_id) == j - i and set(by_id) == {w[0] for w in W[i:j]}, "lines %d..%d: other cluster pairs than the reference's" % (i + 2, j + 1)
        for w in W[i:j]:
            assert same(by_id[w[0]], w), "line of %s: got %r, want %r" % (w[0], by_id[w[0]], w)
        i = j
    i = 0
    while i < n:
        j = i + 1
        while j < n and W[j][1:3] == W[i][1:3]:
            j += 1
        assert [g[0] for g in G[i:j]] == [w[0] for w in W[i:j]], "lines %d..%d: the reference prints them as exactly equal, in another order" % (i + 2, j + 1)
        i = j


def compare_bestguess_file(got, want, pp_files):
    """R1_bestguess.txt / R1_bestguess_G.txt: every field as text -- the two Allele strings with no escape -- except Q1, a posterior: the first row's is a sum
    of P over the pairs of a cluster, the second row's one P; both within REL * (|LLmin| + |LLmax|) of the locus' table (compare_pairs_file) plus the print."""
    G = [l.split("\t") for l in got.decode().splitlines()]; W = [l.split("\t") for l in want.decode().splitlines()]
    assert G[0] == W[0] and len(G) == len(W), "header or line count"
    for g, w in zip(G[1:], W[1:]):
        lls = [abs(float(l.split("\t")[2])) for l in pp_files["R1_PP_%s_pairs.txt" % w[0]].decode().splitlines()[1:]]
        assert len(g) == len(w) and g[:3] == w[:3] and g[4:] == w[4:], (g, w)
        assert close_printed(g[3], w[3], REL * (max(lls) + min(lls))), (g, w)


def compare_pileup_file(got, want):
    """R1_pileup_<locus>.txt: an entry reads `genotype (qualities) [pairsDistance d | alignmentLength n | mapQ_position | mapQ mapQ_genomic | weighted-OK x 2 | IDs]`.
    mapQ and mapQ_genomic are the read's posterior (device exp, REL relative: tests/test_gpu_align.py); everything else is compared as text."""
    G = got.decode().splitlines(); W = want.decode().splitlines()
    assert len(G) == len(W), "line count"
    for ln, (g, w) in enumerate(zip(G, W)):
        if g == w:
            continue
        pg, pw = g.split(" | "), w.split(" | ")
        assert len(pg) == len(pw), "line %d" % (ln + 1)
        for i, (a, b) in enumerate(zip(pg, pw)):
            if i % 5 == 3:
                ta, tb = a.split(" "), b.split(" ")
                assert len(ta) == len(tb) == 2 and all(close_printed(x, y, REL) for x, y in zip(ta, tb)), "line %d: mapQ %r / %r" % (ln + 1, a, b)
            else:
                assert a == b, "line %d: %r / %r" % (ln + 1, a[:200], b[:200])


def compare_device_files(got, want):
    """the files of a device run against the reference's; returns the list of disagreements (file: what)"""
    bad = []
    for fn in want:
        try:
            if fn.startswith("R1_PP_"):
                compare_pairs_file(got[fn], want[fn])
            elif fn.startswith("R1_bestguess"):
                compare_bestguess_file(got[fn], want[fn], want)
            elif fn.startswith("R1_pileup_"):
                compare_pileup_file(got[fn], want[fn])
            else:
                assert normalise(fn, got[fn]) == normalise(fn, want[fn]), first_difference(got[fn], want[fn])
        except AssertionError as e:
            bad.append("%s: %s" % (fn, e))
    return bad
