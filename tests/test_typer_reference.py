"""The high-precision restatement of the typer (tests/typer_reference.py) against the CPU oracle, on the inputs of the GPU edge tests
(tests/test_gpu_typer_edges.py) and with their tolerances: an error of the restatement, or a tolerance the double-precision formulas
themselves do not meet, shows here, on a machine without a GPU.  Every test prints the largest error / bound ratio it saw (pytest -s)."""
import math

import numpy as np
import pytest

import oracle_binding as ob
import typer_edge_cases as ec
import typer_reference as tr

LD = np.longdouble


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_reference_by_hand():
    la = lambda a, b: math.log((math.exp(a) + math.exp(b)) / 2)
    LL = np.array([[-1.0, -2.0], [-3.0, -2.0]]); mism = np.array([[0, 2], [1, 2]])
    for engine in ("mpmath", "longdouble"):
        ref, (avg2, mn), mag = tr.pair_loglik_ref(LL, mism, engine)
        assert np.allclose(ref.astype(np.float64), [-3.0, la(-1, -3) + la(-2, -2), -5.0], rtol=1e-15, atol=0)
        assert avg2.tolist() == [4, 5, 6] and mn.tolist() == [2, 2, 3]
        assert np.allclose(mag, [3 + 4, abs(la(-1, -3)) + 2 + 4, 5 + 4], rtol=1e-15)
    # operands beyond the range of exp: the smaller one vanishes, two equal ones average to themselves
    ref, _, _ = tr.pair_loglik_ref(np.array([[-1e300], [-1.0]]), np.zeros((2, 1), int), "mpmath")
    assert float(ref[0]) == -1e300 and float(ref[1]) == pytest.approx(-1 - math.log(2), rel=1e-15) and float(ref[2]) == -1.0
    P, marg, worst = tr.call_ref(np.log([1.0, 4.0, 2.0, 1.0, 2.0, 0.5]))
    assert np.allclose(P.astype(np.float64), np.array([1, 4, 2, 1, 2, 0.5]) / 10.5, rtol=1e-15)
    assert np.allclose(marg.astype(np.float64), np.array([7, 7, 4.5]) / 10.5, rtol=1e-15)                  # a pair (c, c) counts once
    assert worst.tolist() == pytest.approx([math.log(4.0), math.log(4.0), math.log(8.0)])
    assert tr.kmer_index(["ACGTN", "TTT"], 2) == {"AC", "CG", "AA"} and tr.kmer_index(["ACG"], 4) == set()
    assert tr.kmer_answer({"AC"}, "GT") == 1 and tr.kmer_answer({"AC"}, "GN") == 0


def test_exon_reference_by_hand():
    seq = np.frombuffer(b"ACG_" + b"ATG_", np.uint8)
    loc = dict(n_clusters=2, exon_length=4, cluster_seq=seq, n_reads=2, pos_off=np.array([0, 4, 5], np.int32), pos_exon=np.array([0, 1, 2, 3, 1], np.int32),
               pos_g0=np.frombuffer(b"AC_TC", np.uint8), pos_glen=np.array([1, 1, 1, 2, 1], np.int32), pos_qual=np.array([73, 255, 0, 33, 32], np.uint8),
               pos_use=np.array([1, 1, 1, 1, 1], np.uint8))
    for long_mode, r in ((0, 0.001), (1, 0.075)):
        LL, mism, mag, n_used = tr.exon_loglik_ref(loc, long_mode)
        lmm, ldel, lins = math.log(1 - 2 * r), math.log(r), math.log(r) + math.log(0.25)
        hit, miss, hit0, miss0 = math.log(0.999), math.log((1 - 0.999) / 3), math.log(0.001), math.log((1 - 0.001) / 3)
        want = [[(lmm + hit) + (lmm + hit) + ldel + 2 * lins, lmm + hit0], [(lmm + hit) + (lmm + miss) + ldel + 2 * lins, lmm + miss0]]
        assert np.allclose(LL.astype(np.float64), want, rtol=1e-14, atol=0)
        assert mism.tolist() == [[1, 0], [2, 1]] and n_used.tolist() == [4, 1]
        assert mag[0, 1] == pytest.approx(abs(lmm + hit0) + 1)


@pytest.mark.parametrize("C,R", [(3, 513), (5, 1025), (4, 1)])
def test_reference_engines_agree(C, R):
    """the longdouble path (used where mpmath would take minutes) against the formula as written in mpmath: far inside the tolerance asserted with either"""
    LL, mism = ec.pair_case(C, R)
    a, _, mag = tr.pair_loglik_ref(LL, mism, "mpmath"); b, _, mag2 = tr.pair_loglik_ref(LL, mism, "longdouble")
    assert np.all(np.abs(a - b) <= tr.pair_bound(R, mag) / 1000) and np.allclose(mag, mag2, rtol=1e-12)
    LLc = ec.call_case(23, "spread5000")[0]
    Pa, ma, wa = tr.call_ref(LLc, "mpmath"); Pb, mb, wb = tr.call_ref(LLc, "longdouble")
    assert np.all(np.abs(Pa - Pb) <= Pa * LD(2.0 ** -52)) and np.all(np.abs(ma - mb) <= ma * LD(2.0 ** -52)) and np.array_equal(wa, wb)


# ------------------------------------------------------------------------------------------------ the oracle inside the tolerances
@pytest.mark.parametrize("C,R", ec.PAIR_SHAPES)
def test_oracle_pair_loglik_within_bound(oracle, C, R):
    LL, mism = ec.pair_case(C, R)
    ec.check_pairs(ob.pair_loglik(LL, mism), C, R)


@pytest.mark.parametrize("long_mode", [0, 1])
@pytest.mark.parametrize("C", ec.EXON_CLUSTERS)
def test_oracle_exon_loglik_within_bound(oracle, C, long_mode):
    loc = ec.exon_case(C)
    n = np.diff(loc["pos_off"]); used = np.add.reduceat(np.append(loc["pos_use"], 0).astype(int), loc["pos_off"][:-1]) * (n > 0)
    assert (n == 0).sum() >= 3 and ((n > 0) & (used == 0)).any() and n[-1] == 0                                  # reads without positions, all positions filtered
    assert set(loc["pos_qual"][loc["pos_use"] == 1]) == set(ec.QUAL_BYTES)
    ec.check_exon(ob.exon_loglik(loc, long_mode), C, long_mode)


def test_oracle_many_reads_within_bound(oracle):
    loc = ec.many_reads_case()
    LL, mism = ob.exon_loglik(loc)
    ec.check_exon((LL, mism), "many", 0)
    ec.check_many_reads_pairs(ob.pair_loglik(LL, mism), LL, mism)


@pytest.mark.parametrize("profile", ec.CALL_PROFILES)
@pytest.mark.parametrize("C", ec.CALL_CLUSTERS)
def test_oracle_call_within_bound(oracle, C, profile):
    ec.check_call(ob.call_locus(*ec.call_case(C, profile)), C, profile)


# ------------------------------------------------------------------------------------------------ the k-mer questions are what they claim to be
@pytest.mark.parametrize("k", ec.KMER_KS)
def test_kmer_questions(k):
    cases = ec.kmer_reads(k)
    lens = {len(s) for s, _, _ in cases}
    assert lens == set(ec.kmer_lengths(k)) and all(any((L - 256 * j) in (k - 1, k, k + 1) for j in range(3)) for L in lens if L < 600)
    planted = 0
    for s, q, note in cases:
        idx = tr.kmer_index([s], k)
        ans = [tr.kmer_answer(idx, x) for x in q]
        if "plant@" in note or "palindrome" in note:
            assert ans[0] == 1 and (ans[1] == 1 or "palindrome" in note); planted += 1
        if "N@" in note:
            n_cover = len([o for o in range(max(0, 255 - k + 1), 257) if o + k <= len(s)])
            assert not any(ans[:n_cover]) and all(ans[n_cover:n_cover + 1])                                    # covering an N: absent; the neighbours: present
        if "shorter" in note:
            assert not any(ans)
    assert planted >= 30
    reads = [s for s, _, _ in cases]
    if k >= 12:
        q, extra = ec.kmer_capacity_queries(reads, k, np.random.default_rng(5))
        canon = {tr.canonical(x) for x in q}
        assert len(q) == 4096 + 120 and len(canon) == 4096 and tr.canonical(extra) not in canon
        idx = tr.kmer_index(reads, k)
        assert 200 < sum(tr.kmer_answer(idx, x) for x in q) < 1000
