"""Inputs of the typer edge tests and the checks both sides have to pass on them: tests/test_typer_reference.py holds the oracle, tests/test_gpu_typer_edges.py
the kernels against tests/typer_reference.py.  Plain numpy: neither the oracle nor the library is used here.  Every input is a function of its arguments
alone, built once per process and read-only; so is its high-precision reference."""
import functools
import itertools

import numpy as np

import typer_reference as tr

# ------------------------------------------------------------------------------------------------ all pairs
# k_pair_loglik tiles the clusters by 4 rows x 256 columns and the reads by 512: every C and R next to those edges.  The large C only with R = 1 and 513
PAIR_SHAPES = [(C, R) for C in (1, 3, 4, 5) for R in (1, 511, 512, 513, 1025)] + [(C, R) for C in (255, 256, 257, 259) for R in (1, 513)]
TYPE_LOCUS_SHAPES = [(5, 513), (257, 1), (259, 513)]
BIG = (1 << 20)


@functools.lru_cache(maxsize=None)
def pair_case(C, R):
    """(LL [C, R], mism [C, R]): ordinary values in (-31, -1) with the extremes mixed in so that, the diagonal apart, no pair's tolerance is emptied by them.

    R > 1: every row carries max(1, R // 100) entries each of 0.0, -745 and -1e4 at reads of its own choice, and one entry of -1e300 at read (2 c + 1) % R --
           a different read for every row, so -1e300 meets itself only in the pair (c, c) and an ordinary operand in every other pair of the row.
    R = 1: the one entry of row c is -1e300 (c = 1 only), -1e4 (c % 4 == 2), -745 (c % 4 == 3) or ordinary.
    C = 1: the single pair is the row against itself: -745 and 0.0 only.
    C >= 2: row 0 is all zeros: the pair (0, 0) sums to exactly 0 and is the best pair, by a margin the tests assert.
    C >= 3: the last row is a copy of row (C - 1) // 2 (a == b exactly in that pair) except where that row holds -1e300, where the copy is ordinary."""
    rng = np.random.default_rng(1000 * C + R)
    LL = -rng.random((C, R)) * 30 - 1
    n_each = max(1, R // 100)
    for c in range(C):
        if R == 1:
            if C > 1: LL[c, 0] = -1e300 if c == 1 else (-1e4 if c % 4 == 2 else (-745.0 if c % 4 == 3 else LL[c, 0]))
            else: LL[c, 0] = -745.0
            continue
        own = (2 * c + 1) % R
        at = [r for r in rng.permutation(R) if r != own][:3 * n_each]
        for j, v in enumerate((0.0, -745.0, -1e4) if C > 1 else (0.0, -745.0, -745.0)):
            LL[c, at[j * n_each:(j + 1) * n_each]] = v
        if C > 1: LL[c, own] = -1e300
    mism = rng.choice(np.array([0, 0, 1, 2, 3, BIG - 1, BIG, BIG + 1], np.int32), (C, R)).astype(np.int32)
    if C >= 2:
        LL[0] = 0.0; mism[0, ::2] = 0
    if C >= 3:
        src = (C - 1) // 2
        fresh = -rng.random(R) * 30 - 1
        LL[C - 1] = np.where(LL[src] < -1e299, fresh, LL[src]); mism[C - 1] = mism[src]
    assert C > R or len({(2 * c + 1) % R for c in range(C)}) == C or R == 1
    LL.setflags(write=False); mism.setflags(write=False)
    return LL, mism


@functools.lru_cache(maxsize=None)
def pair_ref(C, R):
    """The high-precision side of pair_case(C, R), computed once per process: (ref, (avg2, mn), mag, bound)."""
    LL, mism = pair_case(C, R)
    ref, mis, mag = tr.pair_loglik_ref(LL, mism)
    return ref, mis, mag, tr.pair_bound(R, mag)


# ------------------------------------------------------------------------------------------------ per-read scoring
EXON_CLUSTERS = (1, 255, 256, 257)
QUAL_BYTES = (0, 32, 33, 73, 74, 255)           # below 33 (read as 33), 33 (pCorrect 0 -> 0.001), 73 / 74 / 255 (capped at 0.999)


def _locus(C, P, seq, reads):
    """reads: list of lists of (exon column, g0, glen, quality byte, use)"""
    off = [0]; flat = []
    for r in reads:
        flat += r; off.append(len(flat))
    col = lambda i, dt: np.asarray([p[i] for p in flat], dt)
    d = dict(n_clusters=C, exon_length=P, cluster_seq=np.ascontiguousarray(seq.reshape(-1), np.uint8), n_reads=len(reads), pos_off=np.asarray(off, np.int32),
             pos_exon=col(0, np.int32), pos_g0=col(1, np.uint8), pos_glen=col(2, np.int32), pos_qual=col(3, np.uint8), pos_use=col(4, np.uint8))
    for v in d.values():
        if isinstance(v, np.ndarray): v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def exon_case(C):
    """A hand-made locus of 12 exon columns: cluster c has '_' in column j where (7 c + 3 j) % 5 == 0 and "ACGT"[(c + j) % 4] elsewhere.  Every combination of
    (column, first genotype character in "_ACGT", genotype length in 1 / 2 / 5) occurs once as a used position, the quality bytes of QUAL_BYTES cycling with a
    stride coprime to the rest; the positions are dealt into reads of 1, 2, 3, 7, 1, 2, ... positions with filtered positions (pos_use == 0) in between, after
    a read without positions and a read whose positions are all filtered, and before two more reads without positions."""
    P = 12
    c = np.arange(C)[:, None]; j = np.arange(P)[None, :]
    seq = np.frombuffer(b"ACGT", np.uint8)[(c + j) % 4].copy(); seq[(7 * c + 3 * j) % 5 == 0] = ord("_")
    combos = [(col, g0, glen) for col, g0, glen in itertools.product(range(P), b"_ACGT", (1, 2, 5))]
    pos = [(col, g0, glen, QUAL_BYTES[(5 * i + i // 6) % 6], 1) for i, (col, g0, glen) in enumerate(combos)]
    reads = [[], [(3, ord("A"), 1, 73, 0), (0, ord("_"), 2, 33, 0), (5, ord("C"), 5, 0, 0)]]
    sizes = itertools.cycle((1, 2, 3, 7)); i = 0
    while i < len(pos):
        n = next(sizes); r = pos[i:i + n]; i += n
        if len(reads) % 3 == 0:                                  # filtered positions at the start, inside and at the end of a read
            f = (r[0][0], r[0][1], r[0][2], r[0][3], 0)
            r = [f] + r[:1] + [f] + r[1:] + [f]
        reads.append(r)
    reads += [[], []]
    return _locus(C, P, seq, reads)


@functools.lru_cache(maxsize=None)
def many_reads_case():
    """C = 3, R = 70 000 reads of one to three positions over 8 exon columns (a twentieth of the reads: every position filtered): the read count of deep
    targeted data at one locus, more than the 65 535 a grid's second dimension is documented to hold."""
    C, P, R = 3, 8, 70000
    rng = np.random.default_rng(70000)
    seq = np.frombuffer(b"ACGT_", np.uint8)[rng.integers(0, 5, (C, P))]
    n = rng.integers(1, 4, R); off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32); N = int(off[-1])
    use = (rng.random(N) < 0.9).astype(np.uint8)
    dead = np.flatnonzero(rng.random(R) < 0.05)
    for r in dead: use[off[r]:off[r + 1]] = 0
    d = dict(n_clusters=C, exon_length=P, cluster_seq=np.ascontiguousarray(seq.reshape(-1), np.uint8), n_reads=R, pos_off=off, pos_exon=rng.integers(0, P, N).astype(np.int32),
             pos_g0=np.frombuffer(b"_ACGT", np.uint8)[rng.integers(0, 5, N)], pos_glen=rng.choice(np.array([1, 1, 1, 2, 5], np.int32), N).astype(np.int32),
             pos_qual=np.asarray(QUAL_BYTES, np.uint8)[rng.integers(0, 6, N)], pos_use=use)
    for v in d.values():
        if isinstance(v, np.ndarray): v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def exon_ref(key, long_read_mode):
    """tr.exon_loglik_ref of exon_case(key) (key: a cluster count) or of many_reads_case() (key: "many"), once per process, with the bound."""
    loc = many_reads_case() if key == "many" else exon_case(key)
    LL, mism, mag, n_used = tr.exon_loglik_ref(loc, long_read_mode)
    return LL, mism, mag, n_used, tr.exon_bound(n_used, mag)


# ------------------------------------------------------------------------------------------------ the call
CALL_CLUSTERS = (1, 2, 23, 724)                 # 724 clusters = 262 450 pairs: just above the 262 144 elements one pass of k_call_p's grid covers
CALL_PROFILES = ("spread5000", "equal", "ahead40", "copies")


def call_dups(C):
    return {1: (), 2: ((1, 0),), 23: ((5, 17), (22, 0), (11, 10), (12, 10)), 724: ((5, 17), (723, 0), (300, 299), (301, 299))}[C]


@functools.lru_cache(maxsize=None)
def call_case(C, profile):
    """(pairLL, misAvg, misMin) of C clusters:
       spread5000  LL uniform over a range of 5000: most posteriors underflow to 0 or to denormals
       equal       every LL the same (and every mismatch sum: the whole table is one run of ties)
       ahead40     one pair 40 ahead of all the others, which lie within 2 of each other
       ahead40early  the same with the dominant pair anywhere in the large table too: for the kernels only (see below), not in CALL_PROFILES
       copies      the table of per-read rows in which clusters copy other clusters (call_dups): exact ties in LL and mismatches"""
    rng = np.random.default_rng(7000 + 10 * C + (CALL_PROFILES + ("ahead40early",)).index(profile))
    nP = C * (C + 1) // 2
    MA = rng.integers(0, 8, nP) / 2.0; MM = np.floor(MA)
    if profile == "spread5000":
        LL = -rng.random(nP) * 5000 - 3
    elif profile == "equal":
        LL = np.full(nP, -1234.5); MA = np.full(nP, 2.5); MM = np.full(nP, 2.0)
    elif profile in ("ahead40", "ahead40early"):
        # (the reference's normalising sum, which the oracle follows, runs serially over the table: once it holds the 1 of the dominant pair, every later term of
        #  e^-40 lies below half an ulp of it and is lost -- 4e-13 relative over 262 450 pairs, outside a tolerance derived for the kernel's fixed-depth tree.  In the
        #  large table the dominant pair is therefore the last one, where either order of summation is accurate; in the small ones it sits anywhere.  The kernels are
        #  also run on "ahead40early", where it sits anywhere in the large table as well: the oracle's posteriors miss the tolerance there by design of the reference)
        LL = -rng.random(nP) * 2 - 100; LL[int(rng.integers(0, nP)) if (nP <= 1024 or profile == "ahead40early") else nP - 1] = LL.max() + 40
    else:
        R = 40
        ll = -rng.random((C, R)) * 30 - 1; mm = rng.integers(0, 4, (C, R))
        for a, b in call_dups(C):
            ll[a] = ll[b]; mm[a] = mm[b]
        LL = np.zeros(nP); MA = np.zeros(nP); MM = np.zeros(nP)
        for c1 in range(C):
            i0 = tr.tri(c1, c1, C); n = C - c1
            hi = np.maximum(ll[c1], ll[c1:]); lo = np.minimum(ll[c1], ll[c1:])
            LL[i0:i0 + n] = np.sum(np.log(0.5) + hi + np.log1p(np.exp(lo - hi)), axis=1)
            MA[i0:i0 + n] = np.sum((mm[c1] + mm[c1:]) / 2.0, axis=1); MM[i0:i0 + n] = np.sum(np.minimum(mm[c1], mm[c1:]), axis=1)
    for v in (LL, MA, MM): v.setflags(write=False)
    return LL, MA, MM


@functools.lru_cache(maxsize=None)
def call_reference(C, profile):
    """tr.call_ref of call_case(C, profile), once per process, with the two bounds: (P, marg, bound_P, bound_marg)."""
    LL, _, _ = call_case(C, profile)
    P, marg, worst = tr.call_ref(LL)
    return P, marg, tr.posterior_bound(P, LL), tr.marginal_bound(marg, worst, len(LL), C)


# ------------------------------------------------------------------------------------------------ k-mers
KMER_KS = (1, 2, 12, 30, 31)
KMER_TILE = 256
LONG_READ = 4133                                 # 16 tiles and a ragged seventeenth
_RC = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s[::-1].translate(_RC)


def kmer_lengths(k):
    """k-1, k, k+1 (a length of 0 cannot be a read: one tile further, 256 + k - 1, stands in for it), the lengths around one and two full tiles, one long read."""
    L = [k - 1 if k > 1 else KMER_TILE + k - 1, k, k + 1, 255 + k, 256 + k - 1, 256 + k, 257 + k, 512 + k - 1, 512 + k, LONG_READ]
    return sorted(set(L))


def _background(rng, L, k, letter=None):
    """k >= 12: random ACGT (a planted k-mer is then unique, which kmer_reads asserts); k <= 2: one letter, so that the planted one is the only other k-mer"""
    if k <= 2:
        return (letter or "A") * L
    return "".join(rng.choice(list("ACGT"), L))


def _plant(k, palindrome=False):
    """k = 1: C against a background of A; k = 2: CG (its own reverse complement); else a fixed pattern no random background holds (asserted), or for an even k
    on request a k-mer that is its own reverse complement"""
    if k == 1: return "C"
    if k == 2: return "CG"
    if palindrome:
        h = ("CCGTGACCTTGAGCA" * 3)[:k // 2]
        return h + revcomp(h)
    return ("CCCCGGGGTTCATCAGTCCGGACGTTTAAGC" * 2)[:k]


@functools.lru_cache(maxsize=None)
def kmer_reads(k):
    """[(read, queries, note)]: one read per (length, planted offset) with a k-mer planted at offset 0, 255, 256, 257, 511, 512 or len-k -- asked forward and
    reverse-complemented, with the k-mers that start around the tile edges and some that are absent --; per length >= 258 one read with N at offsets 255 and 256,
    asked for the k-mers that cover them with the N read as A (what its low two bits are: absent), and for their neighbours; for an even k a planted k-mer that is
    its own reverse complement.  The answers come from typer_reference.kmer_index of the read alone."""
    rng = np.random.default_rng(900 + k)
    out = []
    absent = ["G" * k, "T" * k] if k > 2 else []

    def edge_queries(s):
        q = []
        for o in (0, 1, 254, 255, 256, 257, 258, 510, 511, 512, 513, len(s) - k - 1, len(s) - k, len(s) - k + 1):
            if 0 <= o and o + k <= len(s): q.append(s[o:o + k])
        return q

    for L in kmer_lengths(k):
        for o in sorted({0, 255, 256, 257, 511, 512, L - k}):
            if o < 0 or o + k > L: continue
            bg = _background(rng, L, k); p = _plant(k)
            assert tr.canonical(p) not in tr.kmer_index([bg], k)
            s = bg[:o] + p + bg[o + k:]
            out.append((s, [p, revcomp(p)] + edge_queries(s) + absent, "L%d plant@%d" % (L, o)))
        if L < k:
            out.append((_background(rng, L, k), [_plant(k)] + absent, "L%d shorter than k" % L))
        if L >= 258:
            bg = _background(rng, L, k, "C")
            s = bg[:255] + "NN" + bg[257:]
            asA = s.replace("N", "A")
            cover = [asA[o:o + k] for o in range(max(0, 255 - k + 1), 257) if o + k <= L]
            near = [s[o:o + k] for o in (255 - k, 257) if 0 <= o and o + k <= L]
            assert near and all("N" not in x for x in near)
            out.append((s, cover + near + absent, "L%d N@255,256" % L))
        if k % 2 == 0 and L >= 255 + k:
            bg = _background(rng, L, k); p = _plant(k, True); assert p == revcomp(p)
            assert tr.canonical(p) not in tr.kmer_index([bg], k)
            s = bg[:255] + p + bg[255 + k:]
            out.append((s, [p] + edge_queries(s) + absent, "L%d palindrome@255" % L))
    return tuple(out)


def kmer_capacity_queries(reads, k, rng, n_distinct=4096):
    """`n_distinct` queries with pairwise different canonical forms, some hundred of them k-mers of the reads, then 60 repeats and 60 reverse complements of
    earlier ones on top (which add no distinct k-mer).  Returns (queries, one more query whose canonical form is new)."""
    seen = set(); q = []

    def add(x):
        c = tr.canonical(x)
        if c in seen or "N" in x: return
        seen.add(c); q.append(x)
    long_reads = [s for s in reads if len(s) >= 600 + k]
    for s in long_reads[:3]:
        for o in range(0, 600, 5): add(s[o:o + k])
    while len(q) < n_distinct + 1:
        add("".join(rng.choice(list("ACGT"), k)))
    extra = q.pop()
    return q + q[:60] + [revcomp(x) for x in q[100:160]], extra


def reads_batch(world, reads, synth):
    """An unpaired batch of reads of exactly the given lengths, made read by read by synth.make_long_batch (error-free: one alignment of len(read) matched
    bases each) and joined; the bases are then overwritten with the given content."""
    from ref_typer import concat_unpaired
    b = None
    for i, s in enumerate(reads):
        one = synth.make_long_batch(world, 1, seed=i, len_lo=len(s), len_hi=len(s), sub=0.0, ins=0.0, dele=0.0, clip_max=0)
        assert int(one["read_off"][1]) == len(s), "the contigs of the world are shorter than the read"
        b = one if b is None else concat_unpaired(b, one)
    b["read_bases"] = np.frombuffer("".join(reads).encode(), np.uint8).copy()
    assert len(b["read_bases"]) == int(b["read_off"][-1])
    return b


# ------------------------------------------------------------------------------------------------ what both the oracle and the kernels have to satisfy
LD = np.longdouble


def ratio(got, ref, bound):
    """largest |got - ref| / bound (0 / 0 counts as 0)"""
    err = np.abs(np.asarray(got, np.float64).astype(LD) - ref); b = np.asarray(bound).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, LD(0), err / b)
    return float(np.max(q)) if q.size else 0.0


def check_pairs(got, C, R):
    """what both the oracle and the kernel have to satisfy on pair_case(C, R); returns the largest error / bound"""
    pl, ma, mn = got
    ref, (avg2, mnr), mag, bound = pair_ref(C, R)
    assert [int(2 * x) for x in ma] == list(avg2) and all(float(2 * x).is_integer() for x in ma), "misAvg"
    assert [int(x) for x in mn] == list(mnr) and all(float(x).is_integer() for x in mn), "misMin"
    # no tolerance is empty: -1e300 on both sides at one read swamps a pair's bound, which may happen in a row's pair with itself only; every other bound
    # is below 1e-6, against terms of 1 to 31 per read
    LL, _ = pair_case(C, R)
    huge = LL < -1e299
    swamped = np.array([bool((huge[c1] & huge[c2]).any()) for c1 in range(C) for c2 in range(c1, C)])
    diagonal = np.array([c1 == c2 for c1 in range(C) for c2 in range(c1, C)])
    assert not (swamped & ~diagonal).any() and (bound[~swamped] < 1e-6).all() and (C == 1) <= (not swamped.any())
    q = ratio(pl, ref, bound); qs = ratio(np.asarray(pl)[~swamped], ref[~swamped], bound[~swamped])
    print("pair_loglik C=%d R=%d: largest |pairLL - ref| / bound = %.3g (%d of %d pairs with a bound below 1e-6)" % (C, R, qs, int((~swamped).sum()), len(ref)))
    assert q <= 1.0
    if len(ref) > 1:
        best = int(np.argmax(ref)); others = np.arange(len(ref)) != best
        second = int(np.argmax(np.where(others, ref, -np.inf)))
        assert ref[best] - ref[second] > 2 * max(bound[best], bound[second])                                    # the inputs decide the best pair beyond the tolerance ...
        assert np.all(ref[best] - ref[others] > (bound[best] + bound[others]).astype(LD))
        assert int(np.argmax(pl)) == best                                                                       # ... so it has to be found
    return q


def check_exon(got, key, long_mode):
    LL, mism = got
    ref, mref, mag, n_used, bound = exon_ref(key, long_mode)
    assert np.array_equal(mism, mref), "mismatch counts"
    q = ratio(LL, ref, bound)
    print("exon_loglik %s long=%d: largest |LL - ref| / bound = %.3g" % (key, long_mode, q))
    assert q <= 1.0 and np.all(np.isfinite(LL))
    return q


def check_many_reads_pairs(got, LL, mism):
    """the all-pairs sums over 70 000 reads of the many-reads locus, from the per-read table LL (the oracle's and the kernel's are bit-identical)"""
    ref, (avg2, mnr), mag = tr.pair_loglik_ref(LL, mism, "longdouble")
    pl, ma, mn = got
    assert [int(2 * x) for x in ma] == list(avg2) and [int(x) for x in mn] == list(mnr)
    q = ratio(pl, ref, tr.pair_bound(LL.shape[1], mag))
    print("pair_loglik C=3 R=70000: largest |pairLL - ref| / bound = %.3g" % q)
    assert q <= 1.0
    return q


def check_call(got, C, profile, oracle_call=None):
    LL, MA, MM = call_case(C, profile)
    P, marg, bP, bM = call_reference(C, profile)
    qP = ratio(got["p_normalized"], P, bP); qM = ratio(got["cluster_marginal"], marg, bM)
    print("call C=%d %s: largest |P - ref| / bound = %.3g, marginals %.3g" % (C, profile, qP, qM))
    assert qP <= 1.0 and qM <= 1.0
    assert got["ll_max"] == LL.max() and got["max_pair"] == int(np.argmax(LL))
    if profile == "equal":                                       # P = 1 / nP (to the bound, above); the same additions for every cluster
        assert np.all(got["cluster_marginal"] == got["cluster_marginal"][0]) and got["n_sort_ties"] == len(LL) - 1
    if profile == "copies":
        for a, b in call_dups(C):
            assert got["cluster_marginal"][a] == got["cluster_marginal"][b]
        assert (got["n_sort_ties"] > 0) == (C > 1)
    if profile == "spread5000" and C >= 23:
        assert (np.asarray(got["p_normalized"]) == 0).any() and (P.astype(np.float64) < 2.3e-308).sum() > len(LL) // 2       # the underflow is in the table
    if oracle_call is not None:
        for k in ("first_cluster", "second_cluster", "max_pair", "n_sort_ties"):
            assert got[k] == oracle_call[k], k
        assert np.array_equal(got["order"], oracle_call["order"])
    return qP, qM
