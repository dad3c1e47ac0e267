"""The typer's arithmetic, restated in high precision (test infrastructure; uses neither the oracle nor the library).

The oracle evaluates the same double-precision formulas as the kernels, so a comparison with it cannot tell how far both are from the
number they stand for.  Here every quantity is computed with mpmath at 60 digits, or -- where that takes more than a few seconds -- in
numpy.longdouble (64-bit mantissa) with an exact sum of the terms (math.fsum over the double halves of every term).  Results come back
as numpy.longdouble: its 2^-64 relative rounding is a four-thousandth of the smallest tolerance used against them.

    pair_loglik_ref(LL, mism)            all cluster pairs: sum over reads of log((exp a + exp b) / 2), mismatch sums, sum of (|t| + 2)
    call_ref(pairLL)                     posteriors exp(LL - max) / sum and per-cluster marginals
    exon_loglik_ref(locus, long_mode)    per (cluster, read) log-likelihoods, mismatch counts, sum of (|term| + 1), positions used
    kmer_index(reads, k)                 set of canonical k-mers over ACGT

and the tolerances the tests derive from them (pair_bound, exon_bound, posterior_bound, marginal_bound)."""
import math

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 60
LD = np.longdouble
EPS = 2.0 ** -52
MPMATH_TERMS = 20000            # more pair terms than this: the longdouble path (mpmath: ~40 us per term)


def tri(c1, c2, C):
    """Index of the pair (c1 <= c2) in the c1-major table of all pairs."""
    return c1 * C - c1 * (c1 - 1) // 2 + (c2 - c1)


def _ld(x):
    """mpf -> longdouble: the mantissa through two doubles (exact to 2^-106, then rounded once), scaled by the exponent, which may lie outside the range of a double."""
    if x == 0:
        return LD(0)
    man, ex = MP.frexp(x)
    hi = float(man)
    return np.ldexp(LD(hi) + LD(float(man - MP.mpf(hi))), int(ex))


def _exact_sum_ld(t):
    """Sum of a 1-d longdouble array: every element is split into two doubles (exact: 64 = 53 + 11 bits), math.fsum adds them without error,
    a second pass recovers what the first result's rounding to double dropped."""
    hi = t.astype(np.float64); lo = (t - hi.astype(LD)).astype(np.float64)
    parts = hi.tolist() + lo.tolist()
    s1 = math.fsum(parts)
    return LD(s1) + LD(math.fsum(parts + [-s1]))


# ------------------------------------------------------------------------------------------------ all pairs
def pair_loglik_ref(LL, mism, engine=None):
    """(ref, (avg2, mn), mag): per pair (c1 <= c2) in table order
         ref   sum_r log((exp(a_r) + exp(b_r)) / 2)                       numpy.longdouble
         avg2  sum_r (m1 + m2)  -- twice the sum of the averages --  and  mn  sum_r min(m1, m2)        Python integers (object arrays)
         mag   sum_r (|t_r| + 2) over the pair's terms t_r                 float
    engine: "mpmath" (the formula as written, 60 digits), "longdouble" (max + log1p(exp(-|a - b|)) - log 2 per term, exact sum) or None: by size."""
    LL = np.asarray(LL, np.float64); mism = np.asarray(mism)
    C, R = LL.shape; nP = C * (C + 1) // 2
    if engine is None:
        engine = "mpmath" if nP * R <= MPMATH_TERMS else "longdouble"
    ref = np.zeros(nP, LD); mag = np.zeros(nP, np.float64)
    avg2 = np.zeros(nP, object); mn = np.zeros(nP, object)
    M = mism.astype(np.int64)
    for c1 in range(C):
        i0 = tri(c1, c1, C); n = C - c1
        avg2[i0:i0 + n] = [int(x) for x in (M[c1] + M[c1:]).sum(axis=1)]
        mn[i0:i0 + n] = [int(x) for x in np.minimum(M[c1], M[c1:]).sum(axis=1)]
    if engine == "mpmath":
        E = [[MP.exp(MP.mpf(float(v))) for v in row] for row in LL]
        for c1 in range(C):
            for c2 in range(c1, C):
                s = MP.mpf(0); m = MP.mpf(0)
                for r in range(R):
                    t = MP.log((E[c1][r] + E[c2][r]) / 2)
                    s += t; m += abs(t) + 2
                ref[tri(c1, c2, C)] = _ld(s); mag[tri(c1, c2, C)] = float(m)
        return ref, (avg2, mn), mag
    assert engine == "longdouble"
    A = LL.astype(LD); ln2 = LD(float(MP.log(2))) + LD(float(MP.log(2) - MP.mpf(float(MP.log(2)))))
    for c1 in range(C):
        a = A[c1][None, :]; b = A[c1:]
        T = np.maximum(a, b) + (np.log1p(np.exp(-np.abs(a - b))) - ln2)
        i0 = tri(c1, c1, C)
        for j in range(C - c1):
            ref[i0 + j] = _exact_sum_ld(T[j])
        mag[i0:i0 + C - c1] = (np.abs(T).sum(axis=1) + 2 * R).astype(np.float64)
    return ref, (avg2, mn), mag


def pair_bound(R, mag):
    """|pairLL - ref| <= 2^-52 (R + 8) sum(|t| + 2): R serial additions of at most half an ulp of a partial sum <= sum |t| each; every term from one
    exp, one log and three additions of at most about an ulp each (the documented FP64 bound of exp and log) on magnitudes <= |t| + 2."""
    return EPS * (R + 8) * np.asarray(mag, np.float64)


# ------------------------------------------------------------------------------------------------ the call
def call_ref(pairLL, engine=None):
    """(P, marginal, worst): P_i = exp(LL_i - max) / sum_j exp(LL_j - max); marginal_c = sum of P over the pairs that contain c ((c, c) once);
    worst_c = the largest |LL_i - max| among the pairs of c whose P_i is at least 2^-64 of marginal_c (smaller ones cannot move the marginal at
    the precision asserted).  numpy.longdouble, numpy.longdouble, float."""
    LLd = np.asarray(pairLL, np.float64)
    nP = len(LLd); C = int((math.isqrt(8 * nP + 1) - 1) // 2); assert C * (C + 1) // 2 == nP
    if engine is None:
        engine = "mpmath" if nP <= 400 else "longdouble"
    mx = float(LLd.max())
    if engine == "mpmath":
        e = [MP.exp(MP.mpf(float(v)) - MP.mpf(mx)) for v in LLd]
        s = MP.fsum(e)
        Pm = [x / s for x in e]
        P = np.array([_ld(x) for x in Pm], LD)
    else:
        # longdouble: LL - max is exact or rounded to 2^-64 relative, exp and the divide to an ulp; the terms are non-negative, so the pairwise sum
        # of numpy keeps 2^-64 log2(n) relative.  exp(-5000) = 1e-2172 is an ordinary longdouble
        e = np.exp(LLd.astype(LD) - LD(mx))
        P = e / np.sum(e)
        Pm = None
    marg = np.zeros(C, LD); worst = np.zeros(C, np.float64)
    dist = np.abs(LLd - mx)
    for c in range(C):
        idx = np.array([tri(min(c, x), max(c, x), C) for x in range(C)])
        marg[c] = _ld(MP.fsum([Pm[i] for i in idx])) if Pm is not None else np.sum(P[idx])
        carry = P[idx] >= marg[c] * LD(2.0 ** -64)
        worst[c] = float(dist[idx][carry].max()) if carry.any() else 0.0
    return P, marg, worst


def posterior_bound(P_ref, pairLL):
    """|P_i - ref_i| <= ref_i 2^-52 (|LL_i - max| + 1100 + nP / 262144) + 5e-324: the rounding of the argument of exp weighs |LL_i - max| ulps, exp and the
    divide two, the normalising sum (non-negative terms, depth <= 1024 + 8 + per-thread count) the rest; one denormal step absolute."""
    LLd = np.asarray(pairLL, np.float64); nP = len(LLd)
    return P_ref * LD(EPS) * (np.abs(LLd - LLd.max()) + 1100 + nP / 262144).astype(LD) + LD(5e-324)


def marginal_bound(marg_ref, worst, nP, C):
    """The same relative bound with the worst |LL - max| among the pairs of the cluster that carry weight; every one of the C posteriors summed brings its
    own denormal step of absolute slack."""
    return marg_ref * LD(EPS) * (worst + 1100 + nP / 262144).astype(LD) + LD(C) * LD(5e-324)


# ------------------------------------------------------------------------------------------------ per-read scoring
def _phred_p_correct(q):
    """Utilities::PhredToPCorrect with a quality byte below 33 read as 33: 1 - 10^(-(q - 33) / 10), exactly."""
    q = max(int(q), 33)
    return 1 - MP.power(10, MP.mpf(-(q - 33)) / 10)


def exon_loglik_ref(locus, long_read_mode=0):
    """(LL, mism, mag, n_used): per (cluster, read) the sum over the read's used positions of the position's log-likelihood, the mismatch count,
    sum(|term| + 1) over those positions and (per read) how many there are.  The rules are those of k_exon_loglik / typer_tables (hla/HLATyper.cpp:2067-2277):

      exon '_' : read "_" alone costs nothing, anything else (1 + l_diff) (log pIns + log 1/4)
      exon base: read '_' first: log pDel; else log(1 - pIns - pDel) + log pCorrect (same base) or log((1 - pCorrect) / 3); plus l_diff (log pIns + log 1/4)
      pCorrect : > 0.999 -> 0.999, == 0 -> 0.001; quality bytes below 33 read as 33; pIns = pDel = 0.001, or 0.075 in long-read mode
      mismatch : the read's genotype is neither "_" nor the exon character alone

    The constants 0.999, 0.001, 0.075 and 1/3 are the doubles the program text names, taken exactly.  (An uncapped pCorrect strictly inside (0, 0.999) would be
    formed by the program as 1 - pWrong in double, which costs 1 - pCorrect up to 2^-53 / pWrong relative: the tolerance of exon_bound does not cover that, and
    the tests keep to quality bytes whose pCorrect is one of the two constants.)"""
    C, Pn, R = int(locus["n_clusters"]), int(locus["exon_length"]), int(locus["n_reads"])
    seq = np.asarray(locus["cluster_seq"], np.uint8).reshape(C, Pn)
    off = np.asarray(locus["pos_off"]); pe = np.asarray(locus["pos_exon"]); g0 = np.asarray(locus["pos_g0"]); gl = np.asarray(locus["pos_glen"])
    pq = np.asarray(locus["pos_qual"]); use = np.asarray(locus["pos_use"])
    p_indel = MP.mpf(0.075 if long_read_mode else 0.001)
    l_ins = MP.log(p_indel) + MP.log(MP.mpf(0.25)); l_del = MP.log(p_indel); l_mm = MP.log(1 - p_indel - p_indel)
    cache = {}

    def term(e, g, glen, q):
        key = (e == 95, g == 95, e == g, int(glen), int(q))
        if key not in cache:
            l_diff = int(glen) - 1
            if e == 95:
                t = MP.mpf(0) if (glen == 1 and g == 95) else l_ins * (1 + l_diff)
            else:
                if g == 95:
                    t = l_del
                else:
                    pc = _phred_p_correct(q)
                    if pc > MP.mpf(0.999): pc = MP.mpf(0.999)
                    if pc == 0: pc = MP.mpf(0.001)
                    t = l_mm + (MP.log(pc) if e == g else MP.log((1 - pc) * MP.mpf(1.0 / 3.0)))
                t = t + l_ins * l_diff
            cache[key] = (t, abs(t) + 1)
        return cache[key]

    LLm = [[MP.mpf(0)] * R for _ in range(C)]; magm = [[MP.mpf(0)] * R for _ in range(C)]
    mism = np.zeros((C, R), np.int64); n_used = np.zeros(R, np.int64)
    for r in range(R):
        for i in range(int(off[r]), int(off[r + 1])):
            if not use[i]:
                continue
            n_used[r] += 1
            col = seq[:, pe[i]]; g = int(g0[i]); glen = int(gl[i])
            for c in range(C):
                e = int(col[c])
                t, m = term(e, g, glen, pq[i])
                LLm[c][r] += t; magm[c][r] += m
                if not (glen == 1 and g == 95) and not (glen == 1 and g == e):
                    mism[c, r] += 1
    LL = np.array([[_ld(x) for x in row] for row in LLm], LD).reshape(C, R)
    mag = np.array([[float(x) for x in row] for row in magm], np.float64).reshape(C, R)
    return LL, mism, mag, n_used


def exon_bound(n_used, mag):
    """|LL - ref| <= 2^-52 (n_pos + 4) sum(|term| + 1): n_pos serial additions, a term of at most three table entries (a libm log each) and two additions;
    the + 1 per position covers what the rounding of a probability near 1 costs its logarithm in absolute terms."""
    return EPS * (np.asarray(n_used, np.float64)[None, :] + 4) * np.asarray(mag, np.float64)


# ------------------------------------------------------------------------------------------------ k-mers
_RC = str.maketrans("ACGT", "TGCA")


def canonical(kmer):
    """The lexicographically smaller of a k-mer and its reverse complement (kMer_canonical_representation, hla/HLATyper.cpp:4237-4256)."""
    rc = kmer[::-1].translate(_RC)
    return min(kmer, rc)


def kmer_index(reads, k):
    """Canonical forms of all k-mers over ACGT of the reads (strings); a k-mer with any other character is in no index."""
    index = set()
    acgt = set("ACGT")
    for s in reads:
        bad = [0 if ch in acgt else 1 for ch in s]
        run = 0                                   # length of the ACGT-only stretch that ends at position i
        for i in range(len(s)):
            run = 0 if bad[i] else run + 1
            if run >= k:
                index.add(canonical(s[i - k + 1:i + 1]))
    return index


def kmer_answer(index, query):
    return 1 if (set(query) <= set("ACGT") and canonical(query) in index) else 0
