"""CPU: the oracle against tests/pair_reference.py WITHOUT capacities on the families of tests/pair_overflow_cases.py -- the pairs the overflow class of the
pairing stage is for.  As tests/test_pair_reference.py does for its families: the records the filters keep are the table the family was built for, integers and
pair_ll equal, doubles within the derived bounds, Phred bytes equal where the bound decides them, the family's floors hold.  With the library's capacities the
model refuses exactly the pairs each family is for."""
import os

import numpy as np
import pytest

import pair_edge_cases as pe
import pair_overflow_cases as po
import pair_reference as pr


def _units(f, b, exp, capacities):
    return pr.batch_units(b, exp["ext"], f["world"]["contigs"], b["insert_mean"], b["insert_sd"], capacities=capacities)


@pytest.mark.parametrize("name", list(po.NEW_FAMILIES))
def test_oracle_meets_the_exact_reference_beyond_the_capacities(oracle, name):
    f = po.NEW_FAMILIES[name]()
    b, exp = pe.oracle_answers(oracle, f)
    n = b["n_pairs"]
    assert np.array_equal(pe.kept_counts(b, exp["seeds"]["status"]), f["kept"]), "the filters keep other records than the family was built for"
    assert np.all(exp["pairs"]["pair_status"][:n] == 0)
    units = _units(f, b, exp, False)
    s = pe.check_units(units, exp["pairs"], name)
    po.check_floors(s, f, name)
    if "n_comb" in f:
        assert exp["pairs"]["n_combinations"][:n].tolist() == f["n_comb"]
    if "best1" in f:
        assert [u["best1"] for u in units] == f["best1"]
    if "lengths" in f:          # one column more than bases: the variants' own one-base indels
        assert [int(exp["pairs"]["n_cols"][2 * p:2 * p + 2].max()) for p in range(n)] == [L + 1 for L in f["lengths"]]
    # with the library's capacities: refused are exactly the pairs the family is for
    assert pe.refused_by_capacity(_units(f, b, exp, True)) == f["beyond"]


def test_fixture_family_is_the_committed_fixture():
    """tests/golden/ref_pair_overflow.npz holds the batch of pair_overflow_cases.over_fixture(): what tests/test_gpu_pair_overflow.py compares with the reference's
    answers is the family it also runs against the oracle and the exact model."""
    import golden_pipeline as gp
    f = gp.load("ref_pair_overflow.npz"); fam = po.over_fixture(); b = fam["batch"]
    for k in gp.BATCH_KEYS:
        assert np.array_equal(np.asarray(f["batch"][k]), np.asarray(b[k])), k
    assert f["exp"]["n_combinations"].tolist() == fam["n_comb"] and float(f["meta"]["insert_mean"]) == b["insert_mean"] and int(f["meta"]["max_columns"]) == fam["max_columns"]
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pair_overflow.npz")) <= 47851
