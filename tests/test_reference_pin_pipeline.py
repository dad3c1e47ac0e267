"""CPU: the oracle's projection, pairing and mapping qualities against the reference's own processBAM.cpp, built locally (oracle/ref/).

tests/test_reference_pin.py pins the extension DP and the scoring; its seed chains come from the oracle's own projection, and everything after scoring
was checked against the oracle's reading only.  Here the static members of mapper::processBAM face the oracle on the same world families (full pipeline, fan,
tie-heavy, band, Graph M, reads of 76 and 250 bases) plus a batch with hard-clipped records, a batch with reference2level_offset != 0, a set of corner
CIGARs and a batch of long single reads:

  projection  transformBAMreadToInternalAlignment, PRGContigBAMAlignment::checkAlignmentConcordanceWithSequence and PRGContigAlignment2Seed(paranoid = true)
              (cleanInitialAlignment, restrictInitialAlignmentToNoGapAreas, the edge choice of the rethreading) in the order of alignment2Chain
              (processBAM.cpp:3050-3126): for EVERY kept chain status, n_cols, seq_begin, seq_end, removed_cols and the level / edge / graph character /
              sequence character rows are equal, none left out.
  pairing     the kept chains extended and scored by the reference (the code test_reference_pin.py pins), the pairing loop of alignOneReadPair
              (:3408-3506: alignedReadPair_strandsValid, alignedReadPair_pairsDistancesUnderlyingSequences, Utilities::findVectorMax), the selection
              (:3538-3548) and assignMappingQualities: best_chain, n_combinations, strands_valid, n_cols, every column row and col_mapq exact for EVERY pair;
              pair_ll within rtol 1e-12, pair_mapq / mate_mapq within rtol 1e-9 and atol 1e-15 (the bars of tests/test_gpu_align.py); the number of doubles
              that differ at all is printed.
  unpaired    Utilities::findVectorMax + assignMappingQualities_unpaired on the oracle's long-read chains and log-likelihoods, the same rules
              (col_fromseed is not compared there: the driver's input type does not carry it).

What the pin rests on besides the reference's text:
  * the insert-size density is pinned UP TO ITS FORMULA: boost::math::pdf(normal, x) is a stand-in, exp(-(x-m)^2 / (2 sd^2)) / (sd sqrt(2 pi)) in double
    precision (oracle/ref/standin/boost/math/distributions/normal.hpp); Boost is not part of the build;
  * BamAlignment::AlignedBases is built by the driver with BamTools' documented BuildCharData rule (oracle/ref/ref_driver.cpp);
  * inGraphGapStretch comes from a scan inside processBAM's constructor (:91-149), which cannot be called: it is an input, and a NumPy statement of the rule
    (ref_pipeline.gap_stretch_rule) is what the pin rests on: test_gap_stretch_rule and every batch here hold the oracle's vector against it, and
    tests/test_gpu_reference_pin_pipeline.py holds the library's hlala_graph_get_gap_stretch against it on every fixture graph;
  * the keep mask (which records survive the strand / identical-coordinate pre-filter of alignOneReadPair, :3200-3240, a non-static member) is the oracle's
    and an input here, as the oracle's seeds were an input to test_reference_pin.py.
Left unpinned: that pre-filter, sortChainsInSeeds, the padding of alignOneLongRead (extendToFullSequenceLength), BamTools' decoding of records.

Corner records (ref_pipeline.CORNER_KINDS / GAP_KINDS): '=' / 'X' for 'M', 'P' operations, leading and trailing 'H', leading 'S', a leading 'I' after 'S', 'I'
directly after 'D', 'D' directly after 'I', insertions of several bases, both strands, seeds that run into a gap stretch from either side or lie wholly inside
one.  Kinds on which the reference itself fails are no expected answer and are NOT part of the compared set (test_dropped_corner_kinds shows that it fails):
  skip_N      'N' in the CIGAR: transformBAMreadToInternalAlignment throws ("should only be the case for RNASeq data", processBAM.cpp:5168);
  pad         a 'P' operation of non-zero length: the reference drops 'P' from its CIGAR walk (:4817) but BamTools writes '*' into AlignedBases for it, so the
              walk's cross-check of the base after the pad against AlignedBases fails (:5018-5035; the reference first prints the record through BamTools'
              GetEndPosition, which the stand-in does not define: the call fails there).  The oracle and the product accept such a record; what they do
              with it is not compared.  'P' of length zero (pad_empty) goes through and is compared;
  all_I       only insertions: transformBAMreadToInternalAlignment returns false (:5271-5287; status REFUSED), which alignment2Chain does not survive;
              the oracle refuses the batch ("alignment consists of insertions only").
A record that starts with 'I' (I_lead_noS) or ends its aligned part with 'I' (I_trail) is accepted by the reference and is part of the compared set.

Floors (FLOORS below): about half of the counts the reference's outputs give on these deterministic inputs; the counts are printed.
The module skips, with the reason, only where test_reference_pin.py skips: neither oracle/_ref/libhlala_ref.so nor the reference sources exist."""
import time

import numpy as np
import pytest

import ref_binding as rb
import ref_pipeline as rp
from oracle_binding import OracleError
from tools import synth
from util import seeds_from_chains

RS = 777
T0 = time.time()


@pytest.fixture(scope="module")
def ref():
    ok, why = rb.available()
    if not ok:
        pytest.skip(why)
    return rb.Reference


def clean_changed(stage0, stage1, rows):
    """Chains on which cleanInitialAlignment changed something: it only ever removes columns, so its output is shorter than the gap-filled alignment
    (the columns from the first to the last defined level plus one column per skipped level, processBAM.cpp:2538-2577)."""
    st = stage0["_stride"]; n = 0
    for c in rows:
        lv = stage0["col_level"][c * st:c * st + int(stage0["n_cols"][c])]
        d = np.nonzero(lv != -1)[0]
        inner = lv[d[0]:d[-1] + 1]
        filled = int((inner == -1).sum()) + int(inner[-1] - inner[0] + 1)
        n += int(stage1["n_cols"][c] != filled)
    return n


def pin(oracle, ref, w, b, label, tot, max_columns=384, pairs=True):
    """One batch: the oracle's stage A and pairs against the reference; adds the counts to `tot`."""
    kw = dict(insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=RS, max_columns=max_columns)
    o = oracle(w["graph"], w["contigs"], **kw)
    exp = o.align_batch(b) if pairs else o.align_batch(b, stop_after_projection=True)
    gap = rb.gap_stretch_rule(w["graph"])
    assert np.array_equal(gap, o.graph_gap_stretch()), label
    status = exp["seeds"]["status"][:b["n_chains"]]
    assert np.all(status >= 0), label
    keep = (status == 0).astype(np.uint8)
    rows = np.nonzero(keep)[0]
    t0 = time.time()
    r = ref(w["graph"], rng_seed=RS, max_columns=max_columns)
    got, stages = r.project_chains(w["contigs"], b, keep, gap, stages=True)
    assert np.all(got["status"][rows] == rb.PROJ_OK) and np.all(got["status"][keep == 0] == rb.PROJ_NOT_KEPT), label
    bad = rp.projection_diffs(exp["seeds"], got, rows)
    assert not bad, "%s: the projection of %d of %d kept chains differs from the reference, first: %s" % (label, len(bad), len(rows), list(bad.items())[:3])
    hard = sum(any(op == "H" for _, op in rp.cigar_of(b, c)) for c in rows)
    c = dict(chains=len(rows), reverse=int(np.asarray(b["chain_reverse"])[rows].sum()), hardclipped=hard, removed=int((got["removed_cols"][rows] > 0).sum()),
             cleaned=clean_changed(stages[0], stages[1], rows), offset=int((np.asarray(b["chain_offset"])[rows] != 0).sum()))
    if pairs:
        n = b["n_pairs"]
        seeds = seeds_from_chains(b, got)                      # the reference's own seed chains go on
        assert np.array_equal(seeds["_keep"], rows)
        pg, ext, pen = r.pair_chains(w["contigs"], seeds, rows, n, b["insert_mean"], b["insert_sd"])
        bad, differ = rp.pair_diffs(exp["pairs"], pg, n)
        assert not bad, "%s: %d of %d pairs differ from the reference, first: %s" % (label, len(bad), n, list(bad.items())[:3])
        first = np.array([rows[np.searchsorted(rows, b["chain_off"][rd])] for rd in range(2 * n)])          # the first kept chain of every read
        c.update(pairs=n, doubles_differ=differ, multi=int((pg["n_combinations"][:n] > 1).sum()), invalid_strands=int((pg["strands_valid"][:n] == 0).sum()),
                 penalty=int(pen.sum()), not_first=int(np.any((pg["best_chain"][:2 * n] != first).reshape(n, 2), axis=1).sum()), mapq_lt1=int((pg["pair_mapq"][:n] < 1).sum()))
    tot["ref_seconds"] = tot.get("ref_seconds", 0.0) + time.time() - t0
    print("%s: %s" % (label, c))
    for k, v in c.items():
        tot[k] = tot.get(k, 0) + v
    r.close(); o.close()
    return got, exp


def check_floors(tot, family):
    print("family %s: %s (module clock %.0f s)" % (family, {k: (round(v, 1) if isinstance(v, float) else v) for k, v in tot.items()}, time.time() - T0))
    for k, v in FLOORS[family].items():
        assert tot[k] >= v, "family %s: %s = %d, expected at least %d" % (family, k, tot[k], v)


# ------------------------------------------------------------------ the gap-stretch input

def test_gap_stretch_rule(oracle):
    """inGraphGapStretch (processBAM.cpp:91-149: runs of at least three consecutive levels that each have an outgoing '_' edge): the oracle's vector equals the
    NumPy statement of the rule that the projection pin uses as its input.  By hand first: runs of 2, 3 and 4 levels, and a run that reaches the last level.  The
    library's vector (hlala_graph_get_gap_stretch needs a context, so a device) is held against the same statement on every fixture graph by
    tests/test_gpu_reference_pin_pipeline.py."""
    from test_oracle_kat import _linear_graph
    g = _linear_graph("ACGTACGTACGTACGTACGTACGT", extra_edges=[(2, "_"), (3, "_"), (6, "_"), (7, "_"), (8, "_"), (11, "_"), (12, "_"), (13, "_"), (14, "_"), (21, "_"), (22, "_")])
    want = np.zeros(g["n_levels"] - 1, np.uint8); want[6:9] = 1; want[11:15] = 1
    assert np.array_equal(rb.gap_stretch_rule(g), want)
    assert np.array_equal(oracle(g, None).graph_gap_stretch(), want)
    g = _linear_graph("ACGTACGTAC", extra_edges=[(7, "_"), (8, "_"), (9, "_")])
    want = np.zeros(10, np.uint8); want[7:10] = 1
    assert np.array_equal(rb.gap_stretch_rule(g), want) and np.array_equal(oracle(g, None).graph_gap_stretch(), want)
    n = runs_of_two = 0
    for w in (synth.make_world(seed=2, G=8000, k=0), synth.make_world(seed=51, G=6000, k=0, extra_identical=3, n_largegap=2), synth.make_fan_world(),
              synth.make_world_m(seed=9, n_levels=30_000, n_windows=2, alleles=(200, 800))):
        want = rb.gap_stretch_rule(w["graph"])
        assert np.array_equal(oracle(w["graph"], None).graph_gap_stretch(), want)
        runs_of_two += int(rb.gap_stretch_rule(w["graph"], min_len=2).sum() - want.sum())
        n += int(want.sum())
    assert n > 1000 and runs_of_two > 0          # the worlds have runs of exactly two levels: a minimum of 2 instead of 3 would show


# ------------------------------------------------------------------ the worlds of the GPU suite

def test_full_pipeline_worlds(oracle, ref):
    tot = {}
    for seed, G, k, n_pairs in [(1, 5000, 1, 150), (2, 8000, 0, 80), (3, 8000, 3, 150), (4, 3000, 10, 100), (5, 30000, 2, 150)]:
        w = synth.make_world(seed=seed, G=G, k=k)
        pin(oracle, ref, w, synth.make_batch(w, n_pairs, seed=seed + 10), "seed %d G %d k %d" % (seed, G, k), tot)
    check_floors(tot, "full pipeline")


def test_fan_world(oracle, ref):
    tot = {}
    w = synth.make_fan_world()
    pin(oracle, ref, w, synth.make_batch(w, 60, seed=23, max_secondary=3), "fan", tot)
    check_floors(tot, "fan")


def test_tie_heavy_worlds(oracle, ref):
    """Identical haplotypes and a secondary for every read (p_secondary = 1): many combinations per pair, equal log-likelihoods, the first maximum decides."""
    tot = {}
    for k, seed in [(0, 51), (2, 52)]:
        w = synth.make_world(seed=seed, G=6000, k=k, extra_identical=3, n_largegap=2)
        b = synth.make_batch(w, 60, seed=seed + 1, p_secondary=1.0, max_secondary=6, p_random_secondary=0.0, clip_max=45)
        pin(oracle, ref, w, b, "ties k %d" % k, tot)
    check_floors(tot, "tie-heavy")


def test_band_worlds(oracle, ref):
    from test_gpu_align import BAND_WORLDS
    tot = {}
    for name, wk, bk in BAND_WORLDS:
        w = synth.make_world(**wk)
        pin(oracle, ref, w, synth.make_batch(w, 60, **bk), "band: " + name, tot)
    check_floors(tot, "band")


def test_reads_of_76_and_250_bases(oracle, ref):
    tot = {}
    w = synth.make_world(seed=61, G=7000, k=1)
    wm = synth.make_world_m(seed=9, n_levels=30_000, n_windows=2, alleles=(200, 800))
    for L in (76, 250):
        b = synth.make_batch(w, 50, seed=62 + L, read_len=L, ins_mean=float(L + 80), ins_sd=30.0, clip_max=L // 3, indel_read_frac=0.0 if L < 100 else 0.2)
        pin(oracle, ref, w, b, "reads of %d" % L, tot, max_columns=512)
        b = synth.make_batch_m(wm, 30, seed=70 + L, read_len=L, jump_mean=float(L + 200), clip_max=L // 3, frac_gene=0.5)
        pin(oracle, ref, wm, b, "Graph M, reads of %d" % L, tot, max_columns=512)
    check_floors(tot, "read lengths")


def test_graph_m_worlds(oracle, ref):
    tot = {}
    for seed, alleles, n_pairs in [(7, (400, 1500), 40), (8, (1500, 3000), 20)]:
        w = synth.make_world_m(seed=seed, n_levels=30_000, n_windows=2, alleles=alleles)
        pin(oracle, ref, w, synth.make_batch_m(w, n_pairs, seed=21, frac_gene=1.0), "Graph M seed %d" % seed, tot)
    check_floors(tot, "Graph M")


def test_hardclipped_records_and_interval_offsets(oracle, ref):
    """Non-primary records with 'H' in place of 'S' (as BWA writes supplementary alignments; synth.make_batch's hardclip_frac draws the decision but writes no 'H'),
    and records of an interval that starts 7 bases into its contig's coordinates (chain_offset != 0)."""
    tot = {}
    w = synth.make_world(seed=3, G=8000, k=3)
    b, n_hard = rp.hardclip_nonprimary(synth.make_batch(w, 120, seed=13, p_secondary=1.0, hardclip_frac=0.5), 0.5, seed=5)
    assert n_hard > 50
    pin(oracle, ref, w, b, "hard clips", tot)
    w7, b = rp.with_interval_offset(w, synth.make_batch(w, 120, seed=14), k=7)
    pin(oracle, ref, w7, b, "chain_offset 7", tot)
    check_floors(tot, "clips and offsets")


def test_pairing_corners(oracle, ref):
    """What the generated batches hardly hold: pairs whose best combination is not the first one (the records of every read in reverse order), pairs with both mates
    on one strand (strands not valid: the insert-size term is the penalty) and an insert-size distribution so narrow that the density of most distances underflows
    to zero (distance_P <= 0, processBAM.cpp:3447: the penalty again)."""
    tot = {}
    w = synth.make_world(seed=52, G=6000, k=2, extra_identical=3, n_largegap=2)
    b = synth.make_batch(w, 80, seed=54, p_secondary=1.0, max_secondary=6, p_random_secondary=0.3, clip_max=45)
    pin(oracle, ref, w, rp.same_strand_pairs(rp.reversed_chain_order(b), every=4), "reverse order, same-strand pairs", tot)
    b = dict(synth.make_batch(w, 40, seed=55, p_secondary=0.5), insert_sd=0.5)
    pin(oracle, ref, w, b, "insert sd 0.5", tot)
    check_floors(tot, "pairing corners")


# ------------------------------------------------------------------ corner records

# What the reference does with the kinds that are not compared (see the module docstring): "fails" = an assert or an exception inside the reference.
DROPPED = {"skip_N": "fails", "pad": "fails", "all_I": "refused"}
COMPARED = [k for k in rp.CORNER_KINDS if k not in DROPPED] + list(rp.GAP_KINDS)


def _corner_world():
    w = synth.make_world(seed=51, G=6000, k=0, extra_identical=3, n_largegap=2)
    base = synth.make_batch(w, 12 * len(COMPARED), seed=91, p_secondary=0.0, indel_read_frac=0.0)
    return w, base


def test_corner_records(oracle, ref):
    tot = {}
    w, base = _corner_world()
    b, kinds = rp.corner_batch(w, base, COMPARED, rb.gap_stretch_rule(w["graph"]))
    got, exp = pin(oracle, ref, w, b, "corner records", tot)
    rows = np.asarray(b["chain_off"])[0:2 * b["n_pairs"]:2]
    per_kind = {k: dict(n=0, reverse=0, removed=0) for k in COMPARED}
    for p, k in enumerate(kinds):
        c = int(rows[p])
        assert got["status"][c] == rb.PROJ_OK, k
        per_kind[k]["n"] += 1; per_kind[k]["reverse"] += int(b["chain_reverse"][c]); per_kind[k]["removed"] += int(got["removed_cols"][c] > 0)
    print("corner kinds: %s" % per_kind)
    for k, v in per_kind.items():
        assert v["n"] == 12 and 0 < v["reverse"] < 12, (k, v)          # every kind on both strands
    assert per_kind["gap_from_left"]["removed"] > 0 and per_kind["gap_from_right"]["removed"] > 0
    check_floors(tot, "corner")


def test_dropped_corner_kinds(oracle, ref):
    """The kinds that are not part of the compared set: the reference fails on them (or refuses the record), which is no expected answer; what the oracle and the product
    do with a record the reference fails on is not compared.  A record the reference refuses (only insertions) is refused by the oracle too."""
    w, base = _corner_world()
    gap = rb.gap_stretch_rule(w["graph"])
    refused = 0
    for kind, what in DROPPED.items():
        for p in (0, 1, 2, 3):
            b, _ = rp.corner_batch(w, rp.subset_units(base, [p]), [kind], gap)
            keep = np.ones(b["n_chains"], np.uint8)
            r = ref(w["graph"], rng_seed=RS)
            if what == "fails":
                with pytest.raises(rb.ReferenceError_) as e:
                    r.project_chains(w["contigs"], b, keep, gap)
                if p == 0:
                    print("%s: %s" % (kind, str(e.value)[:200]))
            else:
                got = r.project_chains(w["contigs"], b, keep, gap)
                assert got["status"][0] == rb.PROJ_REFUSED and got["status"][1] == rb.PROJ_OK
                refused += 1
                with pytest.raises(OracleError, match="insertions only"):
                    oracle(w["graph"], w["contigs"], rng_seed=RS).align_batch(b, stop_after_projection=True)
            r.close()
    print("projections the reference refused: %d" % refused)
    assert refused >= FLOORS["dropped"]["refused"]


# ------------------------------------------------------------------ unpaired mapping qualities

def test_unpaired_mapping_qualities(oracle, ref):
    """assignMappingQualities_unpaired (processBAM.cpp:3900-4059) and the first-maximum choice of alignOneLongRead (:3770) on the oracle's long-read chains: paired
    batches read as single reads (several records per read; once with the records of every read in reverse order, so that the best one is rarely the first) and
    long reads with a second alignment."""
    tot = dict(reads=0, multi=0, mapq_lt1=0, not_first=0, doubles_differ=0)
    cases = []
    w = synth.make_world(seed=52, G=6000, k=2, extra_identical=3, n_largegap=2)
    cases.append((w, synth.as_unpaired(synth.make_batch(w, 60, seed=53, p_secondary=1.0, max_secondary=6, p_random_secondary=0.0, clip_max=45)), 0, 384))
    cases.append((w, rp.reversed_chain_order(synth.as_unpaired(synth.make_batch(w, 40, seed=56, p_secondary=1.0, max_secondary=6, p_random_secondary=0.3, clip_max=45))), 0, 384))
    w = synth.make_world(seed=3, G=8000, k=3)
    cases.append((w, synth.make_long_batch(w, 40, seed=5, len_lo=300, len_hi=900, p_second=0.7), 1, 2048))
    for w, b, long_mode, stride in cases:
        n = b["n_pairs"]
        o = oracle(w["graph"], w["contigs"], rng_seed=RS, long_read_mode=long_mode, max_columns=stride)
        exp = o.align_long_reads(b)
        assert np.all(exp["pairs"]["pair_status"][:n] == 0)
        chains = rp.finished_chains(b, exp["ext"], n)
        r = ref(w["graph"], rng_seed=RS, long_read_mode=long_mode, max_columns=stride)
        got = r.mapq_unpaired(chains, exp["ext"]["ll"][chains["_keep"]], n)
        got["best_chain"][:n] = chains["_keep"][got["best_chain"][:n]]
        bad, differ = rp.pair_diffs(exp["pairs"], got, n, per_unit=1, cols=("col_level", "col_edge", "col_gchar", "col_schar", "col_mapq"))
        assert not bad, "%d of %d reads differ from the reference, first: %s" % (len(bad), n, list(bad.items())[:3])
        first = np.array([chains["_keep"][np.searchsorted(chains["_keep"], b["chain_off"][rd])] for rd in range(n)])
        c = dict(reads=n, multi=int((got["n_combinations"][:n] > 1).sum()), mapq_lt1=int((got["pair_mapq"][:n] < 1).sum()), not_first=int((got["best_chain"][:n] != first).sum()),
                 doubles_differ=differ)
        print("unpaired (long_read_mode %d): %s" % (long_mode, c))
        for k, v in c.items():
            tot[k] += v
        r.close(); o.close()
    check_floors(tot, "unpaired")


# ------------------------------------------------------------------ the committed fixtures

def test_oracle_matches_the_committed_pipeline_fixtures(oracle):
    """tests/golden/ref_proj_*.npz, ref_pair_*.npz and ref_unpaired_*.npz (written by the reference, see make_ref_golden_pipeline.py) against the oracle: needs no
    reference, so the pin holds wherever the suite runs."""
    import golden_pipeline as gp
    for name in gp.PROJ_FIXTURES:
        f = gp.load(name)
        o = oracle(f["graph"], f["contigs"], rng_seed=int(f["meta"]["rng_seed"]), max_columns=int(f["meta"]["max_columns"]))
        got = o.align_batch(f["batch"], stop_after_projection=True)["seeds"]
        assert np.array_equal((got["status"][:f["batch"]["n_chains"]] == 0).astype(np.uint8), f["keep"]), name
        gp.check_projection(got, f, name)
    for name in gp.PAIR_FIXTURES:
        f = gp.load(name)
        o = oracle(f["graph"], f["contigs"], insert_mean=float(f["meta"]["insert_mean"]), insert_sd=float(f["meta"]["insert_sd"]), rng_seed=int(f["meta"]["rng_seed"]),
                   max_columns=int(f["meta"]["max_columns"]))
        got = o.align_batch(f["batch"])
        assert np.array_equal((got["seeds"]["status"][:f["batch"]["n_chains"]] == 0).astype(np.uint8), f["keep"]), name
        gp.check_pairs(got["pairs"], f, name)
    for name in gp.UNPAIRED_FIXTURES:
        f = gp.load(name)
        o = oracle(f["graph"], f["contigs"], rng_seed=int(f["meta"]["rng_seed"]), long_read_mode=int(f["meta"]["long_read_mode"]), max_columns=int(f["meta"]["max_columns"]))
        gp.check_pairs(o.align_long_reads(f["batch"])["pairs"], f, name, per_unit=1)


def test_committed_pipeline_fixtures_are_what_the_reference_writes(ref):
    """The reference built here, run on the fixtures' inputs, writes the fixtures' outputs again; the new fixtures carry the hash over the enlarged source list, and
    the hash the older ref_*.npz carry still is the one over the aligner's sources alone."""
    import golden_pipeline as gp
    from test_gpu_reference_pin import FIXTURES, load
    for name in gp.PROJ_FIXTURES + gp.PAIR_FIXTURES + gp.UNPAIRED_FIXTURES:
        f = gp.load(name)
        again = gp.reference_outputs(f, name)
        for k, v in f["exp"].items():
            assert np.array_equal(again[k], v), (name, k)
        if f["meta"]["ref_sources_sha256"] != rb.sources_hash(pipeline=True):
            print("%s was written by reference sources %s, this reference is %s: same outputs" % (name, f["meta"]["ref_sources_sha256"], rb.sources_hash(pipeline=True)))
    old = {str(load(name)["meta"]["ref_sources_sha256"]) for name in FIXTURES}
    new = {str(gp.load(name)["meta"]["ref_sources_sha256"]) for name in gp.PROJ_FIXTURES + gp.PAIR_FIXTURES + gp.UNPAIRED_FIXTURES}
    assert len(old) == 1 and len(new) == 1 and old != new
    if old == {rb.sources_hash()}:
        assert new == {rb.sources_hash(pipeline=True)}


# Floors: about half of what the reference's outputs give on the inputs above (printed by every test).  A count that is only one or two in a family has no floor
# there: best combinations that are not the first one are the business of "pairing corners" and "unpaired", which hold dozens.
FLOORS = {
    "full pipeline": dict(chains=940, reverse=470, removed=710, pairs=315, multi=185, mapq_lt1=37),
    "fan": dict(chains=70, reverse=34, removed=15, pairs=30, multi=8),
    "tie-heavy": dict(chains=228, reverse=115, removed=185, pairs=60, multi=52, mapq_lt1=21),
    "band": dict(chains=490, reverse=245, removed=340, pairs=180, multi=83, mapq_lt1=16),
    "read lengths": dict(chains=220, reverse=110, removed=110, pairs=80, multi=40, mapq_lt1=8),
    "Graph M": dict(chains=86, reverse=43, removed=11, pairs=30, multi=19),
    "clips and offsets": dict(chains=420, hardclipped=62, offset=174, removed=355, pairs=120, multi=90, mapq_lt1=27),
    "pairing corners": dict(pairs=60, multi=47, invalid_strands=10, penalty=23, not_first=35, mapq_lt1=9),
    "corner": dict(chains=192, reverse=96, hardclipped=18, removed=150, cleaned=6, pairs=96, invalid_strands=12, penalty=20),
    "dropped": dict(refused=2),
    "unpaired": dict(reads=120, multi=88, mapq_lt1=17, not_first=29),
}
