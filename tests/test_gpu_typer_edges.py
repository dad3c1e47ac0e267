"""The typer kernels at their tile edges, numeric extremes and limits, against the high-precision restatement of tests/typer_reference.py
(which tests/test_typer_reference.py holds against the oracle on the same inputs, without a GPU):

  k_pair_loglik     C and R around the 4 x 256 cluster tile and the 512-read tile; equal operands, zeros, operands beyond the range of exp
  k_exon_loglik     reads without (used) positions, quality bytes outside 33 .. 73, long genotypes on '_', C around a block; 70 000 reads
  kmer_scan_read    reads of one to seventeen tiles, k-mers planted at the tile edges, N at a tile edge, k = 1 .. 31, the 4096-query capacity
  k_call_*          tables whose spread exceeds the range of exp, all-equal tables, just more pairs than one pass of the grid covers

Tolerances are derived in tests/typer_reference.py; every test prints the largest error / bound ratio it saw (pytest -s)."""
import numpy as np
import pytest

import oracle_binding as ob
import typer_edge_cases as ec
import typer_reference as tr
from tools import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    return synth.make_world(seed=1, G=300, k=1)


@pytest.fixture(scope="module")
def ctx(pkg, world):
    return pkg.Context(world["graph"], world["contigs"])


@pytest.fixture(scope="module")
def ctx_long(pkg, world):
    return pkg.Context(world["graph"], world["contigs"], long_read_mode=1)


def assert_type_locus_equals_the_three_calls(ctx, loc):
    LL, mism = ctx.exon_loglik(loc)
    pl, ma, mn = ctx.pair_loglik(LL, mism)
    call = ctx.call_locus(pl, ma, mn)
    for want_table in (True, False):
        got = ctx.type_locus(loc, want_reads_table=want_table)
        if want_table:
            assert np.array_equal(got["LL"], LL) and np.array_equal(got["mism"], mism)
        assert np.array_equal(got["pairLL"], pl) and np.array_equal(got["misAvg"], ma) and np.array_equal(got["misMin"], mn)
        for k in ("order", "p_normalized", "cluster_marginal"):
            assert np.array_equal(got[k], call[k]), k
        for k in ("first_cluster", "second_cluster", "first_marginal", "second_p", "ll_max", "max_pair", "n_sort_ties"):
            assert got[k] == call[k], k
    return call


# ------------------------------------------------------------------------------------------------ all pairs
@pytest.mark.parametrize("C,R", ec.PAIR_SHAPES)
def test_pair_loglik_at_tile_edges(ctx, C, R):
    """mismatch sums exactly, |pairLL - ref| <= 2^-52 (R + 8) sum(|t| + 2) for every pair, the best pair found"""
    LL, mism = ec.pair_case(C, R)
    ec.check_pairs(ctx.pair_loglik(LL, mism), C, R)


@pytest.mark.parametrize("C,R", ec.TYPE_LOCUS_SHAPES)
def test_type_locus_at_tile_edges(ctx, C, R):
    assert_type_locus_equals_the_three_calls(ctx, synth.make_locus(seed=C + R, n_clusters=C, n_reads=R, exon_length=60, read_cover=12))


# ------------------------------------------------------------------------------------------------ per-read scoring
@pytest.mark.parametrize("long_mode", [0, 1])
@pytest.mark.parametrize("C", ec.EXON_CLUSTERS)
def test_exon_loglik_edges(ctx, ctx_long, oracle, C, long_mode):
    """bit-identical to the oracle, mismatch counts exact, |LL - ref| <= 2^-52 (n_pos + 4) sum(|term| + 1)"""
    loc = ec.exon_case(C)
    LL, mism = (ctx_long if long_mode else ctx).exon_loglik(loc)
    eLL, em = ob.exon_loglik(loc, long_mode)
    assert np.array_equal(mism, em) and np.array_equal(LL, eLL)                       # table-driven, reference order: bit-identical to the oracle
    ec.check_exon((LL, mism), C, long_mode)


def test_seventy_thousand_reads(ctx, oracle):
    """More reads at one locus than the second dimension of a grid is documented to hold (65 535): hlala_exon_loglik and hlala_type_locus have to take them.
    The MI355X runtime accepts the launch as it is; this test is the guard of that."""
    loc = ec.many_reads_case()
    assert loc["n_reads"] == 70000
    LL, mism = ctx.exon_loglik(loc)
    eLL, em = ob.exon_loglik(loc)
    assert np.array_equal(mism, em) and np.array_equal(LL, eLL)
    ec.check_exon((LL, mism), "many", 0)
    got = ctx.pair_loglik(LL, mism)
    ec.check_many_reads_pairs(got, LL, mism)
    call = assert_type_locus_equals_the_three_calls(ctx, loc)
    e = ob.call_locus(*ob.pair_loglik(eLL, em))
    for k in ("first_cluster", "second_cluster", "max_pair", "n_sort_ties"):
        assert call[k] == e[k], k
    assert np.array_equal(call["order"], e["order"]) and np.allclose(call["p_normalized"], e["p_normalized"], rtol=1e-9, atol=1e-300)


# ------------------------------------------------------------------------------------------------ k-mers
@pytest.fixture(scope="module")
def kmer_world():
    return synth.make_world(seed=3, G=8000, k=1)


@pytest.fixture(scope="module")
def kmer_ctx(pkg, kmer_world):
    return pkg.Context(kmer_world["graph"], kmer_world["contigs"], long_read_mode=1)


@pytest.mark.parametrize("k", ec.KMER_KS)
def test_kmers_across_tiles(kmer_ctx, kmer_world, k):
    """Every read alone (a mask of one read), through hlala_kmer_presence and through hlala_kmer_keep_reads / hlala_kmer_presence_kept, then all reads at once:
    the answers of the index of the read(s), exactly."""
    ctx = kmer_ctx
    cases = ec.kmer_reads(k); reads = [s for s, _, _ in cases]
    gb = ctx.batch_unpaired(ec.reads_batch(kmer_world, reads, synth))
    ctx.kmer_forget_reads()
    for i, (s, q, note) in enumerate(cases):
        idx = tr.kmer_index([s], k)
        want = np.array([tr.kmer_answer(idx, x) for x in q], np.uint8)
        mask = np.zeros(len(reads), np.uint8); mask[i] = 1
        assert np.array_equal(ctx.kmer_presence(gb, q, k, mask), want), (k, note, "presence")
        assert ctx.kmer_keep_reads(gb, mask) == 1
        assert np.array_equal(ctx.kmer_presence_kept(q, k), want), (k, note, "kept")
        ctx.kmer_forget_reads()
    allq = sorted({x for _, q, _ in cases for x in q})
    for mask in (None, (np.arange(len(reads)) % 3 == 0).astype(np.uint8)):
        idx = tr.kmer_index([s for i, s in enumerate(reads) if mask is None or mask[i]], k)
        want = np.array([tr.kmer_answer(idx, x) for x in allq], np.uint8)
        assert np.array_equal(ctx.kmer_presence(gb, allq, k, mask), want), (k, "all reads")
        assert ctx.kmer_keep_reads(gb, mask) == (len(reads) if mask is None else int(mask.sum()))
        assert np.array_equal(ctx.kmer_presence_kept(allq, k), want), (k, "all reads kept")
        ctx.kmer_forget_reads()


@pytest.mark.parametrize("k", [12, 31])
def test_kmer_query_capacity(pkg, kmer_ctx, kmer_world, k):
    """4096 distinct questions fill the table held in LDS; repeats and reverse complements of them do not count; one more distinct question is refused."""
    ctx = kmer_ctx
    reads = [s for s, _, _ in ec.kmer_reads(k)]
    gb = ctx.batch_unpaired(ec.reads_batch(kmer_world, reads, synth))
    q, extra = ec.kmer_capacity_queries(reads, k, np.random.default_rng(5))
    assert len({tr.canonical(x) for x in q}) == 4096 and len(q) == 4096 + 120
    idx = tr.kmer_index(reads, k)
    want = np.array([tr.kmer_answer(idx, x) for x in q], np.uint8)
    assert 200 < want.sum() < 1000
    assert np.array_equal(ctx.kmer_presence(gb, q, k), want)
    ctx.kmer_forget_reads(); ctx.kmer_keep_reads(gb)
    assert np.array_equal(ctx.kmer_presence_kept(q, k), want)
    with pytest.raises(pkg.HlalaError, match="4096"):
        ctx.kmer_presence(gb, q + [extra], k)
    with pytest.raises(pkg.HlalaError, match="4096"):
        ctx.kmer_presence_kept(q + [extra], k)
    ctx.kmer_forget_reads()
    for bad_k in (0, 32):
        with pytest.raises(pkg.HlalaError):
            ctx.kmer_presence(gb, ["A" * bad_k], bad_k)


# ------------------------------------------------------------------------------------------------ the call
@pytest.mark.parametrize("profile", ec.CALL_PROFILES)
@pytest.mark.parametrize("C", ec.CALL_CLUSTERS)
def test_posteriors_at_numeric_extremes(ctx, oracle, C, profile):
    """|P_i - ref_i| <= ref_i 2^-52 (|LL_i - max| + 1100 + nP / 262144) + 5e-324, the marginals to the same relative bound; the integer outputs are the oracle's"""
    table = ec.call_case(C, profile)
    ec.check_call(ctx.call_locus(*table), C, profile, oracle_call=ob.call_locus(*table))


def test_posteriors_with_the_dominant_pair_early(ctx, oracle):
    """262 450 pairs, one of them 40 ahead and anywhere in the table: the terms of e^-40 behind it have to survive in the normalising sum.  The reference's
    serial sum loses them (the oracle's posteriors miss this tolerance by a few per cent, which is why the CPU test does not run this table); the kernel's
    per-thread and tree sums must not.  Posteriors and marginals against the high-precision reference, the integer outputs against the oracle."""
    table = ec.call_case(724, "ahead40early")
    assert int(np.argmax(table[0])) < len(table[0]) - 1024
    ec.check_call(ctx.call_locus(*table), 724, "ahead40early", oracle_call=ob.call_locus(*table))
