"""hlala_filter_positions_gpu (kernel_filter.hip) against hlala_filter_positions, the host function that calls the library's std::sort: pos_use, read_ignored and all
twelve counters exactly, on the case lists of tests/test_filter_gpu_model.py (which holds the host model against the same function) and at the sizes where the
bucket kernels change their path: the insertion-sort limit, the wavefront, the capacity."""
import ctypes as C

import numpy as np
import pytest

import filter_gpu_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    from tools import synth
    w = synth.make_world(seed=11, G=4000, k=1)
    c = pkg.Context(w["graph"], w["contigs"], insert_mean=200.0, insert_sd=35.0, rng_seed=5, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    return lambda e, prm=None: pkg.filter_positions(lib, e, prm)


def run(pkg, ctx, host, name, e, prm=None):
    got = pkg.filter_positions_gpu(ctx, e, prm)
    F.check_equal(got, host(e, prm), name)
    return got[3]


@pytest.mark.parametrize("k", range(len(F.worlds())), ids=[w[0] for w in F.worlds()])
def test_worlds(pkg, ctx, host, k):
    run(pkg, ctx, host, *F.worlds()[k])


@pytest.mark.parametrize("k", range(4), ids=[c[0] for c in F.genotype_cases()])
def test_genotypes(pkg, ctx, host, k):
    name, e, prm = F.genotype_cases()[k]
    counts = run(pkg, ctx, host, name, e, prm)
    assert counts == pkg.host_filter_model(e, prm)[3]


@pytest.mark.parametrize("k", range(4), ids=[c[0] for c in F.host_only_cases()])
def test_parameter_edges(pkg, ctx, host, k):
    run(pkg, ctx, host, *F.host_only_cases()[k])


def test_tie_buckets(pkg, ctx, host):
    differ = 0
    for n, minor in F.TIE_BUCKETS:
        e = F.tie_bucket(n, minor)
        run(pkg, ctx, host, f"tie bucket {n} {minor}", e)
        differ += not np.array_equal(pkg.host_filter_model(e, tie_rule=1)[0], host(e)[0])
    assert differ >= 8, differ                                  # a stable order would not have passed


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 19, 20, 21, 63, 64, 65, 128, 129, 4095, 4096])
def test_single_bucket(pkg, ctx, host, n):
    counts = run(pkg, ctx, host, f"single bucket {n}", F.single_bucket(n))
    assert counts["largest_bucket"] == n and counts["buckets"] == (n > 0) and counts["buckets_sorted"] == (n >= 20)


@pytest.mark.parametrize("n", [64, 1000, 4096])
def test_adversary(pkg, ctx, host, n):
    e = F.adversary_bucket(n)
    counts = run(pkg, ctx, host, f"adversary {n}", e)
    assert counts["heap_sorts"] >= 1 and counts["heap_sorts"] == pkg.host_filter_model(e)[3]["heap_sorts"]


def test_refusals_leave_nothing_and_the_context_usable(pkg, ctx, host):
    for name, e, prm, code in F.refusals():
        rc, text, use, ign, st, counts = pkg.filter_positions_gpu(ctx, e, prm, raw=True)
        assert rc == code, (name, rc, text)
        assert (use == 0xAA).all() and (ign == 0xAA).all(), name
        if code == F.E_CAPACITY:
            assert text.startswith("not available:") and "4097" in text, text
        run(pkg, ctx, host, "after " + name, F.single_bucket(40, seed=3))


@pytest.mark.parametrize("k", range(5), ids=[c[0] for c in F.empty_cases()])
def test_empty_loci(pkg, ctx, host, k):
    name, e, prm = F.empty_cases()[k]
    assert run(pkg, ctx, host, name, e, prm)["buckets"] == 0


def test_3000_buckets_of_one_entry(pkg, ctx, host):
    counts = run(pkg, ctx, host, "thin locus", F.thin_locus())
    assert counts["buckets"] == 3000 and counts["largest_bucket"] == 1 and counts["buckets_sorted"] == 0
    assert run(pkg, ctx, host, "thin locus, first20_n = 1", F.thin_locus(), pkg.default_filter_params(first20_n=1))["buckets_sorted"] == 3000


def test_back_to_back_on_one_context(pkg, ctx, host):
    a = next(w for w in F.worlds() if w[0] == "seed2-set0"); b = F.genotype_cases()[1]
    for name, e, prm in (a, b, a, a, b):
        run(pkg, ctx, host, name, e, prm)


def test_bytes_moved(pkg, ctx, host):
    """only what the rule reads goes up: qual_chars, pos_level, read_fraction_ok and the other arrays of the struct do not"""
    e = F.genotype_locus()
    nr, np_, nch = e["n_reads"], e["n_pos"], e["n_chars"]
    base = e["pos_off"].nbytes + e["pos_exon"].nbytes + e["pos_mapq"].nbytes + e["pos_mate"].nbytes + e["geno_off"].nbytes + e["geno_chars"].nbytes + e["read_weighted_ok"].nbytes
    assert base == 4 * (nr + 1) + 4 * np_ + np_ + np_ + 4 * (np_ + 1) + nch + 16 * nr
    c = run(pkg, ctx, host, "genotypes", e)
    assert c["bytes_up"] == base and c["bytes_down"] == np_ + nr
    c = run(pkg, ctx, host, "genotypes, strand", e, pkg.default_filter_params(long_read_strand_filter=1))
    assert c["bytes_up"] == base + e["read_reverse"].nbytes
    # the arrays that stay behind may even be absent
    thin = {k: v for k, v in e.items() if k not in ("qual_chars", "pos_level", "read_fraction_ok", "read_pair", "read_distance", "read_cols_nongap", "pos_novel_gap")}
    F.check_equal(pkg.filter_positions_gpu(ctx, thin), host(e), "without the arrays the rule does not read")
