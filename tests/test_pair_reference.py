"""CPU: tests/pair_reference.py -- stage C restated in exact arithmetic -- against the oracle, on the batches of tests/pair_edge_cases.py.

Per family: the records the filters keep are the table the family was built for; the oracle's pair outputs equal the reference's where they are integers (the
first maximum among the combination log likelihoods, which both form by the same three double operations: pair_ll is compared for equality), lie within
the bounds derived in tests/pair_reference.py where they are doubles, and its Phred bytes equal the exact ones wherever the bound decides them.  The floors
of every family (pairs with several combinations, with a posterior below 1, with a best combination that is not the first, distinct bytes in one row, no
more than 1 % undecided columns) are asserted: without them the comparison would say little.  The largest error / bound ratios are printed (pytest -s).

Where the reference build exists (oracle/_ref/), the families go through pin() of tests/test_reference_pin_pipeline.py as well: the oracle's answers at 64
chains and 1024 combinations then are the reference's own.

The oracle has no capacities: pairs the library refuses (tests/test_gpu_pair_edges.py) are compared here like any other."""
import numpy as np
import pytest

import pair_edge_cases as pe
import pair_reference as pr

FAMILIES = {
    "counts": pe.counts, "maxima": pe.maxima, "maxima-reversed": lambda: pe.maxima(True), "records": pe.records, "draws": lambda: pe.draws(17), "columns": pe.columns,
    "gaps": pe.gaps, "insert-ends": pe.insert_ends, "levels-16": lambda: pe.sequence_levels(16), "levels-17": lambda: pe.sequence_levels(17),
    "levels-33": lambda: pe.sequence_levels(33), "levels-16+1": lambda: pe.sequence_levels("16+1"), "unpaired": pe.unpaired, "fan": pe.fan, "limits": pe.limits,
    **{"draws-%d" % n: (lambda n=n: pe.draws(n)) for n in pe.DRAW_SIZES if n != 17},
}


def _units(f, b, exp, capacities=False):
    return pr.batch_units(b, exp["ext"], f["world"]["contigs"], b["insert_mean"], b["insert_sd"], unpaired=bool(f.get("unpaired")), capacities=capacities)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_oracle_meets_the_exact_reference(oracle, name):
    f = FAMILIES[name]()
    per = 1 if f.get("unpaired") else 2
    b, exp = pe.oracle_answers(oracle, f)
    if f["kept"] is not None:
        assert np.array_equal(pe.kept_counts(b, exp["seeds"]["status"], per), f["kept"][:per * b["n_pairs"]]), "the filters keep other records than the family was built for"
    assert np.all(exp["pairs"]["pair_status"][:b["n_pairs"]] == 0)
    units = _units(f, b, exp)
    s = pe.check_units(units, exp["pairs"], name, per)
    pe.check_floors(s, f["floors"], name)
    if "best" in f:
        assert [u["best"] for u in units] == f["best"]
    assert len(pe.refused_by_capacity(_units(f, b, exp, capacities=True))) == len([u for u in f["refused"] if u not in f["oracle_fails"]])


def test_families_reach_the_sizes_they_are_for(oracle):
    """Floors that are not counts of pairs: the combination counts at every edge, selected chains of 192 and of 193 columns with several combinations, look-ups
    on both sides of both ends of the insert-size table, three anchoring levels with 16 sequences and one with 17."""
    f = pe.counts(); b, exp = pe.oracle_answers(oracle, f)
    assert {1, 2, 63, 64, 65, 126, 128, 129, 1023, 1024, 1025, 1056, 4096} <= set(exp["pairs"]["n_combinations"][:b["n_pairs"]].tolist())
    f = pe.columns(); b, exp = pe.oracle_answers(oracle, f); P = exp["pairs"]
    multi = np.repeat(P["n_combinations"][:b["n_pairs"]] > 1, 2)
    assert {192, 193, 480, 481} <= set(P["n_cols"][:2 * b["n_pairs"]][multi].tolist())
    f = pe.insert_ends(); b, exp = pe.oracle_answers(oracle, f)
    seen = {d for u in _units(f, b, exp) for ds in u["dist"] for d in ds}
    assert set(range(pe.INSERT_DMIN - 3, pe.INSERT_DMAX + 4)) <= seen and min(seen) < 0
    counts = {k: pe.level_counts(pe.level_world(k)[0], _units(pe.sequence_levels(k), *pe.oracle_answers(oracle, pe.sequence_levels(k)))) for k in pe.LEVEL_WORLDS}
    assert max(max(c) for c in counts[16]) == 16 and len(counts[16]) > 1 and max(max(c) for c in counts[17]) == 17 and max(max(c) for c in counts[33]) == 33
    assert {(16, 16, 16, 17), (16, 16, 17, 16), (16, 17, 16, 16), (17, 16, 16, 17)} <= counts["16+1"]
    # "16+1": where the seventeenth sequence is anchored at both ends, its distance alone is next to the mean (all others: twelve more)
    f = pe.sequence_levels("16+1"); b, exp = pe.oracle_answers(oracle, f)
    near = [min(abs(d - 100) for ds in u["dist"] for d in ds) for u in _units(f, b, exp)]
    assert sum(x <= 2 for x in near) >= 8 and sum(x >= 10 for x in near) >= 4


def test_insert_size_doubles_against_sixty_digits():
    """The double evaluation of the log density (what the combination log likelihoods are made of) against its value at 60 digits, at every distance of the
    insert-ends family: within insert_ll_bound where the density is a positive double, the penalty where it is not."""
    m, sd = pe.INSERT_MEAN, pe.INSERT_SD
    worst = 0.0; penalties = 0
    for d in range(pe.INSERT_DMIN - 3, pe.INSERT_DMAX + 4):
        x = pr.insert_ll_exact(m, sd, d)
        if x is None:
            assert pr.insert_ll(m, sd, d) == pr.insert_penalty(m, sd); penalties += 1
            continue
        err = abs(float(pr.MP.mpf(pr.insert_ll(m, sd, d)) - x)); bound = pr.insert_ll_bound(m, sd, d)
        assert err <= bound, (d, err, bound)
        worst = max(worst, err / bound)
    print("insert-size log density: largest error / bound %.3g, distances at the penalty %d" % (worst, penalties))
    assert penalties >= 2 * (5 + 3) and abs(float(pr.MP.mpf(pr.insert_penalty(m, sd)) - pr.insert_ll_exact(m, sd, m + 8 * sd))) <= pr.insert_ll_bound(m, sd, m + 8 * sd)


def test_phred_bytes_of_the_exact_reference():
    """pr.phred_exact against Utilities::PCorrectToPhred by hand: 0 -> 255 (1e-100), 1 -> 33, 0.1 -> 43, thresholds at half Phred units."""
    M = pr.MP.mpf
    assert pr.phred_exact(M(0)) == 255 and pr.phred_exact(M(1)) == 33 and pr.phred_exact(M("0.1")) == 43 and pr.phred_exact(M("1e-30")) == 255
    t = M(10) ** (M("-10.5") / 10)          # -10 log10 = 10.5: rounds up to 11 at the threshold, 10 just above it
    assert pr.phred_exact(t * (1 - M(2) ** -60)) == 44 and pr.phred_exact(t * (1 + M(2) ** -60)) == 43
    assert pr.phred_range(M(1), 0.0) == (255, pr.phred_exact(M(pr.U)), 255)
    # a confidence of exactly 1 evaluated in doubles: 1, or 1 - k 2^-53 (k = 1, 2, 3, 4: -10 log10 = 159.5, 156.5, 154.8, 153.5)
    assert pr.whole_bytes(0.0) == {255, 193} and pr.whole_bytes(3 * pr.U) == {255, 193, 190, 188, 187}
    big = pr.whole_bytes(5000 * pr.U)
    assert {255, 193, 190, 188, 187, 186, 185, 184, 183} <= big and 191 not in big and 194 not in big and min(big) == pr.phred_exact(M(5001) * pr.U) and big >= set(range(min(big), 184))


@pytest.mark.parametrize("name", [k for k in FAMILIES if k != "unpaired"])          # (the unpaired path of the reference takes other inputs: tests/test_reference_pin_pipeline.py)
def test_families_through_the_reference_pin(oracle, name):
    """The reference's own processBAM on the families (pin() of tests/test_reference_pin_pipeline.py): projection and pairing of the oracle equal the reference's."""
    import ref_binding as rb
    import test_reference_pin_pipeline as tp
    ok, why = rb.available()
    if not ok:
        pytest.skip(why)
    f = FAMILIES[name]()
    tot = {}
    tp.pin(oracle, rb.Reference, f["world"], f["batch"], name, tot, max_columns=f["max_columns"])
    assert tot["pairs"] == f["batch"]["n_pairs"] and tot["multi"] >= f["floors"].get("multi", 1)


def test_limits_family_is_the_committed_fixture():
    """tests/golden/ref_pair_limits.npz holds the batch of pair_edge_cases.limits(): what tests/test_gpu_reference_pin_pipeline.py compares with the reference's
    answers is the family tests/test_gpu_pair_edges.py runs."""
    import golden_pipeline as gp
    f = gp.load("ref_pair_limits.npz"); b = pe.limits()["batch"]
    for k in gp.BATCH_KEYS:
        assert np.array_equal(np.asarray(f["batch"][k]), np.asarray(b[k])), k
    assert int(f["exp"]["n_combinations"].max()) == 1024 and float(f["meta"]["insert_mean"]) == b["insert_mean"]
