"""The exact model of the exon-position stage (tests/exonpos_reference.py) against the oracle, on every family and locus of tests/exonpos_edge_cases.py and
on hand-written columns that no aligner may ever produce.  CPU only: this is the evidence that the model is right before a GPU is involved
(tests/test_gpu_exonpos_edges.py then holds the kernels against the model).  The census floors are asserted here on the oracle's alignments.

Every field of oracle_binding.exon_positions is compared: integers and characters exactly, read_weighted_ok / read_fraction_ok bit for bit and within the
bounds derived in tests/exonpos_reference.py of their exact rational values, read_mapq exactly (both sides copy the oracle's own posterior here).
The last test breaks the model four ways and checks that some family notices each: what the model sees, the GPU comparison against the model sees."""
import ctypes as C

import numpy as np
import pytest

import exonpos_edge_cases as ee
import exonpos_reference as er
import oracle_binding as ob
import pair_edge_cases as pe

_ALIGNED = {}


def pcorrect():
    """PhredToPCorrect of every byte, from the project's own table (data, not re-derived)."""
    out = np.zeros(256); q = np.arange(256, dtype=np.uint8)
    ob.lib().orc_phred(256, None, None, q.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def aligned(oracle, f):
    """(batch as the oracle was given it, the oracle's pairs, the model over them); once per process and family."""
    if f["name"] not in _ALIGNED:
        if f.get("oracle_fails"):
            b, x = pe.oracle_answers(oracle, f)
        else:
            b = f["batch"]
            o = oracle(f["world"]["graph"], f["world"]["contigs"], insert_mean=b.get("insert_mean", 200.0), insert_sd=b.get("insert_sd", 35.0), rng_seed=5,
                       long_read_mode=f["long_read_mode"], max_columns=f["max_columns"])
            x = o.align_long_reads(b) if f["unpaired"] else o.align_batch(b)
            o.close()
        _ALIGNED[f["name"]] = (b, x["pairs"], er.Model(x["pairs"], b, f["max_columns"], pcorrect(), f["unpaired"]))
    return _ALIGNED[f["name"]]


def oracle_positions(pairs, b, f, L):
    return ob.exon_positions(pairs, b, f["max_columns"], L["level_min"], L["level_to_exon"], L["insert_mean"], L["insert_sd"], unpaired=f["unpaired"], **er.locus_args(L))


def check(oracle, f, L, label):
    b, pairs, M = aligned(oracle, f)
    m = M.exon_positions(L); e = oracle_positions(pairs, b, f, L)
    er.compare(e, m, "%s: %s" % (f["name"], label), mapq_exact=True, reverse=False)
    assert np.array_equal(np.diff(m["read_pair"]) > 0, np.ones(max(0, m["n_reads"] - 1), bool)), (label, "read_pair ascending")
    return m


def fp(oracle, f):
    b, pairs, M = aligned(oracle, f)
    rows = [r for u in range(b["n_pairs"]) if pairs["pair_status"][u] == 0 for r in ([u] if f["unpaired"] else [2 * u, 2 * u + 1])]
    print("%s: largest |binary64 - exact| / bound of the OK fractions: %.3g" % (f["name"], M.fp_ratio(rows)))


@pytest.mark.parametrize("name", ["overlap", "columns", "unpaired_columns", "unpaired_long"])
def test_model_matches_oracle(oracle, name):
    f = ee.FIXED[name]()
    b, pairs, M = aligned(oracle, f)
    assert (pairs["pair_status"][:b["n_pairs"]] == 0).all()
    total = 0
    for label, L in f["loci"]:
        total += check(oracle, f, L, label)["n_pos"]
    assert total > 1000
    ee.check_floors(ee.census(pairs, b, f["max_columns"], f["loci"][0][1], f["unpaired"]), f["floors"], name + " (oracle)")
    fp(oracle, f)
    if f["unpaired"]:
        m = check(oracle, f, f["loci"][0][1], "second slots")
        assert (m["pos_mate"] == 1).all() and (m["read_distance"] == -1).all() and (m["read_weighted_ok"][1::2] == -1).all() and (m["read_fraction_ok"][1::2] == -1).all()
        assert (m["read_cols_nongap"][1::2] == 0).all() and (m["read_mapq"][1::2] == -1).all()
        for label, L, r, kept in ee.column_count_cases(M):
            m = check(oracle, f, L, label)
            assert (r in m["read_pair"]) == kept and m["n_pairs_ok"] + m["n_pairs_broken"] == b["n_pairs"], label


def test_loci(oracle):
    f = ee.loci(); b, pairs, M = aligned(oracle, f)
    p, up, descs = ee.loci_of(pairs, f["max_columns"], b["n_pairs"])
    total = dict.fromkeys(ee.CENSUS_KEYS, 0)
    for label, L, exp in descs:
        m = check(oracle, f, L, label)
        check_locus_expectation(m, p, up, exp, label)
        for k, v in ee.census(pairs, b, f["max_columns"], L).items():
            total[k] += v
    ee.check_floors(total, f["floors"], "loci (oracle)")


def check_locus_expectation(m, p, up, exp, label):
    assert (p in m["read_pair"]) == exp["present"], label
    assert m["n_pairs_ok"] > 0, label
    if exp["present"]:
        i = m["read_pair"].tolist().index(p); used = m["read_cols_nongap"][2 * i:2 * i + 2] > 0
        assert (bool(used[up]), bool(used[1 - up])) == exp["use"], (label, used, exp["use"])          # read_cols_nongap is 0 for the mate that is not used
    if "n_reads" in exp:
        assert m["n_reads"] == exp["n_reads"] and m["pos_off"].tolist() == [0] and m["geno_off"].tolist() == [0], label


def test_thresholds(oracle):
    f = ee.thresholds(); b, pairs, M = aligned(oracle, f)
    for label, L, p, kept in ee.threshold_cases(M):
        m = check(oracle, f, L, label)
        assert (p in m["read_pair"]) == kept, (label, p)
        assert m["n_pairs_ok"] + m["n_pairs_broken"] == b["n_pairs"]
    ee.check_floors(ee.census(pairs, b, f["max_columns"], ee.whole(-100.0, 20.0)), f["floors"], "thresholds (oracle)")


@pytest.mark.parametrize("n", ee.SIZES)
def test_sizes(oracle, n):
    f = ee.sizes(n); b, pairs, M = aligned(oracle, f)
    out = {}
    for label, mask in ee.size_masks(n):
        out[label] = check(oracle, f, ee.whole(-100.0, 20.0, pair_mask=mask), label)
    check_size_outcomes(out, n)
    ee.check_floors(ee.census(pairs, b, f["max_columns"], ee.whole(-100.0, 20.0)), f["floors"], f["name"] + " (oracle)")


def check_size_outcomes(out, n):
    for k in er.KEYS_COUNT:
        assert out["all ones"][k] == out["no mask"][k], k
    for k in er.KEYS_INT:
        assert np.array_equal(out["all ones"][k], out["no mask"][k]), k
    z = out["all zero"]
    assert z["n_reads"] == 0 and z["n_pairs_ok"] == 0 and z["n_pairs_broken"] == 0
    for label, m in out.items():
        if label.startswith("pair ") or label == "the last pair":
            p = n - 1 if label == "the last pair" else int(label.split()[1])
            assert m["n_pairs_ok"] + m["n_pairs_broken"] == 1 and m["read_pair"].tolist() == [p][:m["n_reads"]], label
        assert m["pos_off"][0] == 0 and m["pos_off"][-1] == m["n_pos"] and (np.diff(m["pos_off"]) > 0).all(), label
        assert m["geno_off"][0] == 0 and m["geno_off"][-1] == m["n_chars"] and (np.diff(m["geno_off"]) > 0).all(), label


def test_refused_units(oracle):
    """The oracle cannot be given the pair the library refuses; a unit with pair_status != 0 is made by hand from one it aligned."""
    f = ee.refused(); b, pairs, M = aligned(oracle, f)
    assert b["n_pairs"] == 2
    L = f["loci"][0][1]
    full = check(oracle, f, L, "both pairs")
    assert full["n_reads"] == 2
    x = dict(pairs, pair_status=np.array([0, -1], np.int32))
    M2 = er.Model(x, b, f["max_columns"], pcorrect())
    m = M2.exon_positions(L); e = oracle_positions(x, b, f, L)
    er.compare(e, m, "refused", mapq_exact=True, reverse=False)
    assert m["read_pair"].tolist() == [0] and m["n_pairs_ok"] + m["n_pairs_broken"] == 1
    us = M2.unit_stats()
    assert us["valid"].tolist() == [1, 0] and all(not us[k].reshape(2, -1)[1].any() for k in us)


def test_unit_stats_of_the_model(oracle):
    """The per-unit statistics against the plain facts of the oracle's pairs and against the oracle's own OK fractions (its exon positions of the whole graph
    under a test that every pair with valid strands passes)."""
    f = ee.overlap(); b, pairs, M = aligned(oracle, f)
    n = b["n_pairs"]; us = M.unit_stats()
    assert us["valid"].all() and np.array_equal(us["strands_valid"], pairs["strands_valid"][:n]) and np.array_equal(us["n_columns"], pairs["n_cols"][:2 * n])
    assert np.array_equal(us["mate_mapq"], pairs["mate_mapq"][:2 * n])
    e = oracle_positions(pairs, b, f, ee.whole(0.0, 1e12))
    u = e["read_pair"]; both = np.stack([2 * u, 2 * u + 1], 1).reshape(-1)
    assert e["n_reads"] == int(pairs["strands_valid"][:n].sum()) > 100
    assert np.array_equal(us["weighted_ok"][both], e["read_weighted_ok"]) and np.array_equal(us["fraction_ok"][both], e["read_fraction_ok"]) and np.array_equal(us["distance"][u], e["read_distance"])
    f = ee.unpaired_columns(); b, pairs, M = aligned(oracle, f)
    n = b["n_pairs"]; us = M.unit_stats()
    e = oracle_positions(pairs, b, f, ee.whole(0.0, 0.0, min_alignment_columns=0))
    assert e["n_reads"] == n and np.array_equal(us["weighted_ok"], e["read_weighted_ok"]) and np.array_equal(us["fraction_ok"], e["read_fraction_ok"])
    assert (us["distance"] == -1).all() and not us["strands_valid"].any() and (us["mate_mapq"][1::2] == -1).all() and not us["n_columns"][1::2].any()


# (levels, graph characters, read characters, mapping-quality characters, qualities of the read's bases)
HAND = {
    "only insertion columns": [([-1, -1, -1], "___", "ACG", "JJJ", "123"), ([30, 31], "AA", "AA", "JJ", "45")],
    # '_' on both sides inside a run of single gaps (levels 11 .. 13) and at the end of one (level 16): neither sweep counts it, neither resets on it
    "a column with '_' on both sides": [([10, 11, 12, 13, 14, 15, 16, 17], "AC_GTA_C", "A___TA_C", "JJJJJJJJ", "1234"), ([14, 15, 16, 17, 18], "TA_CG", "TA_CG", "KKKKK", "5678")],
    "inserted bases run to the last column": [([20, 21, 22, -1, -1], "ACG__", "ACGTT", "JJJJJ", "12345"), ([22, 23], "GA", "GA", "KK", "11")],
    "a lone '_' then inserted bases to the last column": [([20, 21, 22, -1, -1], "ACG__", "AC_TT", "JJJJJ", "1234"), ([22, 23], "GA", "GA", "KK", "21")],
    "first == -1 on mate 2": [([20, 21, 22], "ACG", "ACG", "JJJ", "123"), ([-1, -1], "__", "TT", "KK", "45")],
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_written_columns(oracle, name):
    pr, batch, stride = ee.fake_pairs(HAND[name])
    M = er.Model(pr, batch, stride, pcorrect())
    for a, z in ((0, 40), (11, 22), (22, 22)):
        for sd in (1e6, 0.0):
            L = er.make_locus(a, np.arange(z - a + 1), 0.0, sd)
            m = M.exon_positions(L)
            e = ob.exon_positions(pr, batch, stride, a, L["level_to_exon"], 0.0, sd)
            er.compare(e, m, (name, a, z, sd), mapq_exact=True, reverse=False)
    m = M.exon_positions(er.make_locus(0, np.arange(41), 0.0, 1e6))
    geno = [bytes(m["geno_chars"][m["geno_off"][i]:m["geno_off"][i + 1]]).decode() for i in range(m["n_pos"])]
    if name == "only insertion columns":
        assert m["pos_level"].tolist() == [30, 31] and m["pos_mate"].tolist() == [2, 2] and m["read_cols_nongap"].tolist() == [0, 2] and m["read_distance"].tolist() == [30]
    if name == "a column with '_' on both sides":
        # mate 1: forward sweep 0 1 1 2 0 0 0 0, backward 0 2 1 1 0 0 0 0; mate 2 wins levels 14 ('5' > '2'), 15 ('6' > '3') and 17 ('7' > '4'); level 16 is '_' on both: mate 1
        assert m["pos_level"].tolist() == list(range(10, 19)) and m["pos_novel_gap"].tolist() == [0, 2, 1, 2, 0, 0, 0, 0, 0]
        assert geno == list("A___TA_CG") and m["pos_mate"].tolist() == [1, 1, 1, 1, 2, 2, 1, 2, 2]
    if name == "inserted bases run to the last column":
        assert geno == ["A", "C", "GTT", "A"] and m["pos_mate"].tolist() == [1, 1, 1, 2] and m["pos_novel_gap"].tolist() == [0, 0, 0, 0]          # the worst of "345" beats '1'; the novel gap is that of the position's own column
    if name == "a lone '_' then inserted bases to the last column":
        assert geno == ["A", "C", "TT", "A"] and bytes(m["qual_chars"]).decode() == "12341" and m["pos_novel_gap"].tolist() == [0, 0, 3, 0]          # "_TT" -> "TT"; worst '3' beats '2'
    if name == "first == -1 on mate 2":
        assert m["pos_mate"].tolist() == [1, 1, 1] and m["read_cols_nongap"].tolist() == [3, 0] and m["read_distance"].tolist() == [20]


def test_oracle_intervals_overlap_clause_by_clause():
    """Utilities::intervalsOverlap: the oracle's against the model's on every arrangement of two intervals within eight levels."""
    for x1 in range(8):
        for x2 in range(x1, 8):
            for y1 in range(8):
                for y2 in range(y1, 8):
                    assert bool(ob.lib().orc_intervals_overlap(x1, x2, y1, y2)) == er.intervals_overlap(x1, x2, y1, y2) == (x1 <= y2 and y1 <= x2)


def _differs(a, b):
    return any(a[k] != b[k] for k in er.KEYS_COUNT) or any(not np.array_equal(a[k], b[k]) for k in er.KEYS_INT)


def test_the_suite_bites(oracle):
    """The model broken as a kernel could be, against the unbroken model on the families' own pairs: wherever the two differ, the GPU comparison of
    tests/test_gpu_exonpos_edges.py (library == unbroken model, every field) fails for a kernel broken that way.  No faulty kernel needs to run."""
    caught = {}
    # the tie rule: >= for > in the choice between the mates
    for name in ("overlap", "columns"):
        f = ee.FIXED[name](); b, pairs, M = aligned(oracle, f); L = f["loci"][0][1]
        if _differs(M.exon_positions(L), M.exon_positions(L, tie_to_later=True)):
            caught.setdefault("tie rule", []).append(name)
    # the strip rule: the leading '_' is kept
    for name in ("columns", "unpaired_columns"):
        f = ee.FIXED[name](); b, pairs, M = aligned(oracle, f); L = f["loci"][0][1]
        if _differs(M.exon_positions(L), er.Model(pairs, b, f["max_columns"], pcorrect(), f["unpaired"], strip=False).exon_positions(L)):
            caught.setdefault("strip rule", []).append(name)
    # one comparison of the overlap test left out (a clause left out whole changes nothing: each is implied by the others on intervals)
    f = ee.loci(); b, pairs, M = aligned(oracle, f)
    p, up, descs = ee.loci_of(pairs, f["max_columns"], b["n_pairs"])
    for drop in range(8):
        if any(_differs(M.exon_positions(L), M.exon_positions(L, drop=drop)) for _, L, _ in descs):
            caught.setdefault("overlap test, comparison %d" % drop, []).append("loci")
    # < for <= in the insert test
    f = ee.thresholds(); b, pairs, M = aligned(oracle, f)
    for label, L, p, kept in ee.threshold_cases(M):
        if label.startswith("insert") and _differs(M.exon_positions(L), M.exon_positions(L, strict_insert=True)):
            caught.setdefault("insert test", []).append("thresholds: " + label)
    print("caught: %s" % caught)
    assert {"tie rule", "strip rule", "insert test"} <= set(caught) and all("overlap test, comparison %d" % d in caught for d in range(8)), caught
    assert caught["tie rule"] == ["overlap", "columns"] and caught["strip rule"] == ["columns", "unpaired_columns"]
    assert {"thresholds: insert mean -40, sd 8", "thresholds: insert mean +40, sd 8"} <= set(caught["insert test"])
