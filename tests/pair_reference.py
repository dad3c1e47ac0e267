"""Stage C -- the pairing loop and the mapping qualities -- restated plainly (test infrastructure; uses neither the oracle nor the library).

What is restated, by the reference's lines:
    mapper/processBAM.cpp:3408-3550              the pairing loop of alignOneReadPair: combination log likelihoods, first maximum, selection
    mapper/processBAM.cpp:4062-4312              assignMappingQualities: posteriors, mate posteriors, per-column confidences, Phred bytes
    mapper/processBAM.cpp:3900-4059              assignMappingQualities_unpaired: the same with one list
    mapper/aligner/alignerBase.cpp:213-244       alignedReadPair_strandsValid
    mapper/aligner/alignerBase.cpp:290-329       alignedReadPair_pairsDistancesUnderlyingSequences
    mapper/reads/verboseSeedChain.h:206-280      the last / first two defined levels and their anchors, the first level found per sequence winning
    Utilities.cpp:178-203, 309-323, 987-999      PCorrectToPhred, findVectorMax, normalize_vector

Input: the extended chains of a batch (status, log likelihood, strand, columns: level, graph character, read character) and the contigs' level tables.
Output per pair: the kept lists, the combination log likelihoods, the first maximum, and -- in exact arithmetic -- the posteriors, the mate posteriors, the
per-column confidences of the selected chains and their Phred bytes.

Where double precision is part of the statement, and where it is not.  A combination's log likelihood is three double-precision operations on given doubles,
(ll1 + ll2) + llIS, where llIS is log(pdf(d)) of the normal density written out in doubles, exp(-(d-m)^2 / (2 sd^2)) / (sd sqrt(2 pi)), or the penalty
log(pdf(m + 8 sd)) where the density is not positive.  These are evaluated here as written, with Python floats and the math module (IEEE doubles, the host's
libm): the maximum is chosen among these doubles, so a tie is a tie of doubles and no tolerance applies to the choice.  insert_ll_exact() gives the same
quantity at 60 digits and insert_ll_bound() what the doubles may differ from it.  Everything after the combination log likelihoods -- exp, the normalising
sum, the quotients, the sums over rows, columns and sharing chains -- is computed with mpmath at 60 digits from those doubles.

Bounds for a double-precision evaluation in the reference's order (u = 2^-53, eps = 2^-52, n = nComb, D_i = |LL_i - max|):
    e_i = exp(fl(LL_i - max))   the difference is rounded once (relative u, so the argument moves by u D_i), exp to one ulp (2u): relative u (D_i + 2)
    S = sum e_i, left to right  n - 1 additions of non-negative terms: relative (n - 1) u on top of the terms' own errors, whose weighted mean is at most
                                2u + u sum(e_i D_i) / S <= 2u + 0.37 n u (x e^-x <= 0.37, S >= 1)
    P_i = e_i / S               one more rounding: relative u (D_i + 2) + u (1.37 n + 1) + u  <=  eps (n + 4 + D_i)                    [posterior_bound]
    Q = sum of P_i over a set   (a mate's row or column of the table; the combinations whose chain shares a column with the selected chain), left to right, at most
                                n terms: absolute  sum_set P_i eps (n + 4 + D_i)  +  eps n Q                                            [returned per Q as its bound]
    Phred byte                  1 - Q cancels near 1, so the absolute bound on Q is the bound on pWrong = 1 - Q (the subtraction itself: u); -10 log10(pWrong) + 33
                                and its rounding are four roundings of values below 288: 288 * 4u in Phred units, a relative 2^-44 of pWrong.  The byte is a
                                non-increasing step function of pWrong: the computed byte must lie between the exact bytes of pWrong + delta and pWrong - delta
                                (at pWrong <= 0 the byte is that of 1e-100, 255).  Where both are equal the byte is decided and must be equal; else any byte in
                                between passes and the column counts as undecided.
                                A column that every chain of its mate's list shares has Q = 1 exactly, pWrong = 0: a double sum of all posteriors gives 1
                                (byte 255) or 1 - k 2^-53 with an integer k of at most delta / 2^-53, whose byte is that of k 2^-53 (193, 190, 188, 187, ...):
                                whole_bytes() lists what such a column may hold, and nothing else passes.  Every column of a mate with ONE kept chain is such a
                                column, whatever the input; in a mate with several kept chains they count towards the cap on the undecided share like the
                                undecided columns with Q < 1.

capacity_refusal() states the library's contract (include/hlala_gpu.h), which the reference program does not have: at most 64 kept alignments per mate, at most
1024 combinations, at most 512 columns per chain where there are several combinations."""
import math

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 60
EPS = 2.0 ** -52
U = 2.0 ** -53
CHAIN_OK = 0
MAX_CHAINS, MAX_COMB, MAX_COLS = 64, 1024, 512


# ------------------------------------------------------------------------------------------------ insert size
def normal_pdf(mean, sd, x):
    """The density as the reference build evaluates it, in doubles, operation by operation."""
    e = x - mean
    e *= -e
    e /= 2 * sd * sd
    try:
        r = math.exp(e)
    except OverflowError:          # (never: e <= 0)
        r = math.inf
    return r / (sd * math.sqrt(2 * 3.141592653589793238462643383279502884))


def insert_penalty(mean, sd):
    """max_insertsize_penalty_log, processBAM.cpp:2342-2346"""
    return math.log(normal_pdf(mean, sd, mean + 8 * sd))


def insert_ll(mean, sd, d):
    """processBAM.cpp:3446-3465"""
    p = normal_pdf(mean, sd, float(d))
    return insert_penalty(mean, sd) if p <= 0 else math.log(p)


def insert_ll_exact(mean, sd, d):
    """log of the density at 60 digits, or None where the density is below half of the smallest double (the penalty applies)."""
    m, s = MP.mpf(mean), MP.mpf(sd)
    lg = -((MP.mpf(d) - m) ** 2) / (2 * s * s) - MP.log(s * MP.sqrt(2 * MP.pi))
    return None if lg < MP.log(MP.mpf(2) ** -1075) else lg


def insert_ll_bound(mean, sd, d):
    """What the double evaluation may differ from insert_ll_exact: the exponent's three roundings move it by 3u |exponent|, exp, the quotient and the log add
    4u relative / absolute, the result's own rounding u |log|; a subnormal density carries an absolute 2^-1074, which the log divides by the density."""
    lg = insert_ll_exact(mean, sd, d)
    ex = float((MP.mpf(d) - MP.mpf(mean)) ** 2 / (2 * MP.mpf(sd) ** 2))
    sub = float(MP.mpf(2) ** -1074 / MP.exp(lg))
    return U * (3 * ex + 4 + abs(float(lg))) + 2 * sub


# ------------------------------------------------------------------------------------------------ level tables
def level_tables(contigs):
    """graphLevel_2_underlyingSequencePositions (processBAM.cpp:4441-4456): level -> {sequence id: position along that sequence}."""
    off = np.asarray(contigs["contig_off"]); lvl = np.asarray(contigs["contig_level"]); ids = np.asarray(contigs["contig_seqid"])
    t = {}
    for h in range(int(contigs["n_contigs"])):
        for pos, lv in enumerate(lvl[off[h]:off[h + 1]].tolist()):
            t.setdefault(lv, {})[int(ids[h])] = pos
    return t


def _anchors(levels, tables):
    """alignment_end / begin_originalSequenceAnchors: the levels in scan order, the first position found for a sequence wins."""
    a = {}
    for lv in levels:
        for sid, pos in sorted(tables.get(lv, {}).items()):
            if sid not in a:
                a[sid] = pos
    return a


class Chain:
    """One extended chain: what the pairing reads of it."""

    def __init__(self, ext, c, reverse):
        st = ext["_stride"]; n = int(ext["n_cols"][c])
        self.index = c; self.ll = float(ext["ll"][c]); self.reverse = bool(reverse); self.n = n
        self.levels = ext["col_level"][c * st:c * st + n].tolist()
        self.g = ext["col_gchar"][c * st:c * st + n].tolist(); self.s = ext["col_schar"][c * st:c * st + n].tolist()
        d = [lv for lv in self.levels if lv != -1]
        self.first = d[0] if d else -1; self.last = d[-1] if d else -1                  # alignment_firstLevel / _lastLevel
        self.first2 = d[:2]; self.last2 = d[::-1][:2]                                   # alignment_firstLevels(2) / alignment_lastLevels(2): scan order

    def keys(self, mate):
        """positionID of every column (processBAM.cpp:4130-4189): graph character, level, mate, strand, index of the read base (-1 for a gap in the read)."""
        n_bases = sum(1 for x in self.s if x != 95)
        out, i = [], -1
        for g, lv, s in zip(self.g, self.levels, self.s):
            if s == 95:
                idx = -1
            else:
                i += 1
                idx = n_bases - i - 1 if self.reverse else i
            out.append((g, lv, mate, self.reverse, idx))
        return out


def strands_valid(a, b):
    """alignerBase.cpp:213-244"""
    if a.first != -1 and b.first != -1 and a.reverse != b.reverse:
        return a.first < b.first if not a.reverse else a.last > b.last
    return False


def distances(a, b, tables):
    """alignerBase.cpp:290-329: the set of distances over the sequences that both ends are anchored on."""
    up, down = (a, b) if a.first < b.first else (b, a)
    end, begin = _anchors(up.last2, tables), _anchors(down.first2, tables)
    return sorted({begin[sid] - end[sid] - 1 for sid in end if sid in begin})


# ------------------------------------------------------------------------------------------------ Phred
def phred_exact(p_wrong):
    """Utilities::PCorrectToPhred on pWrong (an mpf): round(min(-10 log10 pWrong, 222) + 33), pWrong = 0 read as 1e-100."""
    if p_wrong <= 0:
        return 255
    ph = -10 * MP.log10(p_wrong)
    if ph + 33 > 255:
        return 255
    return int(MP.floor(ph + 33 + MP.mpf(1) / 2))


def phred_range(q, bound):
    """(exact byte, lowest and highest byte a double evaluation within `bound` of q may give) for a confidence q (mpf, already capped at 1)."""
    w = 1 - q
    delta = MP.mpf(bound) + U + abs(w) * MP.mpf(2) ** -44
    return phred_exact(w), phred_exact(w + delta), phred_exact(w - delta)


_WHOLE = {}


def whole_bytes(bound):
    """The bytes a double evaluation within `bound` may give a confidence that is exactly 1: 255 (the sum came out as 1, or above and was capped) and the bytes
    of pWrong = k 2^-53 for k = 1 .. ceil((bound + u) / 2^-53) -- below 1 the doubles are 2^-53 apart and the subtraction from 1 is exact."""
    K = int(math.ceil((bound + U) / U))
    if K not in _WHOLE:
        small = {phred_exact(MP.mpf(k) * U) for k in range(1, min(K, 64) + 1)}
        _WHOLE[K] = {255} | small | (set(range(phred_exact(MP.mpf(K) * U), phred_exact(MP.mpf(64) * U) + 1)) if K > 64 else set())
    return _WHOLE[K]


# ------------------------------------------------------------------------------------------------ one unit
def capacity_refusal(lists, statuses):
    """The library's contract: a flagged record (status < 0), an empty list, more than 64 kept chains on a mate, more than 1024 combinations, or several
    combinations with a chain of more than 512 columns."""
    if any(s < 0 for s in statuses) or any(len(l) < 1 or len(l) > MAX_CHAINS for l in lists):
        return True
    n = 1
    for l in lists:
        n *= len(l)
    return n > MAX_COMB or (n > 1 and max(c.n for l in lists for c in l) > MAX_COLS)


def posterior_bound(n, d):
    return EPS * (n + 4 + d)


def pair_unit(lists, tables, mean, sd, want_columns=True):
    """One pair (two lists) or one single read (one list).  Returns a dict:
         n1, n2, n_comb; LL [n_comb] doubles, row-major (i1, i2); is_ll [n_comb] insert-size terms, dist [n_comb] the distances looked up, anchor_levels [n_comb] the (up to) four levels they
         were read from (None: strands not valid); best (index of the first
         maximum), best1, best2; pair_ll; strands_valid; P [n_comb] posteriors (mpf); mapq; mate [(value mpf, bound)] per list;
         cols [per list: list of (Q mpf capped at 1, bound, exact byte, lowest byte, highest byte) per column of the selected chain]."""
    paired = len(lists) == 2
    A = lists[0]; B = lists[1] if paired else [None]
    n1, n2 = len(A), len(B); n = n1 * n2
    LL, is_ll, dist, anchor_levels = [], [], [], []
    for a in A:
        for b in B:
            anchor_levels.append(None)
            if not paired:
                LL.append(a.ll); is_ll.append(0.0); dist.append([]); continue
            combined = a.ll + b.ll                                                      # :3414
            pen = insert_penalty(mean, sd); t = pen; ds = []
            if strands_valid(a, b):                                                     # :3425-3473
                ds = distances(a, b, tables)
                up, down = (a, b) if a.first < b.first else (b, a)
                anchor_levels[-1] = tuple(up.last2 + down.first2)
                if ds:
                    t = max(insert_ll(mean, sd, d) for d in ds)
            combined += t                                                               # :3497
            LL.append(combined); is_ll.append(t); dist.append(ds)
    best = 0
    for i in range(1, n):                                                               # findVectorMax: the first maximum
        if LL[i] > LL[best]:
            best = i
    best1, best2 = best // n2, best % n2
    r = dict(n1=n1, n2=n2, n_comb=n, LL=LL, is_ll=is_ll, dist=dist, anchor_levels=anchor_levels, best=best, best1=best1, best2=best2, pair_ll=LL[best],
             best_chain=[A[best1].index] + ([B[best2].index] if paired else []), strands_valid=bool(paired and strands_valid(A[best1], B[best2])))
    one = MP.mpf(1)
    if n == 1:                                                                          # :4302-4311
        r.update(P=[one], mapq=one, mate=[(one, 0.0)] * len(lists), D=[0.0],
                 cols=[[(one, 0.0, 255, 255, 255)] * l[bi].n for l, bi in zip(lists, (best1, best2))])
        return r
    mx = MP.mpf(LL[best])
    D = [float(mx - MP.mpf(v)) for v in LL]
    e = [MP.exp(MP.mpf(v) - mx) for v in LL]                                            # :4071-4085
    S = MP.fsum(e)
    P = [x / S for x in e]
    w = [p * posterior_bound(n, d) for p, d in zip(P, D)]                                # each posterior's absolute bound
    r.update(P=P, D=D, mapq=P[best])

    def total(idx):
        q = MP.fsum(P[i] for i in idx)
        return q, float(MP.fsum(w[i] for i in idx) + EPS * n * q)
    rows = [[i1 * n2 + i2 for i2 in range(n2)] for i1 in range(n1)]
    colsI = [[i1 * n2 + i2 for i1 in range(n1)] for i2 in range(n2)]
    r["mate"] = [(lambda t: (min(t[0], one), t[1]))(total(rows[best1]))] + ([(lambda t: (min(t[0], one), t[1]))(total(colsI[best2]))] if paired else [])
    if not paired:
        r["mate"] = [(P[best], float(w[best]))]                                         # forReturn.mapQ = mapQ, :3922
    r["cols"] = []
    if want_columns:
        for m, (lst, sel, groups) in enumerate(zip(lists, (best1, best2), (rows, colsI))):
            per = [total(g) for g in groups]                                            # what chain k of this mate contributes to a column it shares
            sets = [set(c.keys(m)) for c in lst]
            cache, out = {}, []
            for key in lst[sel].keys(m):
                share = tuple(k for k in range(len(lst)) if key in sets[k])
                if share not in cache:
                    q = MP.fsum(per[k][0] for k in share); bd = sum(per[k][1] for k in share) + EPS * n * float(q)
                    q = one if len(share) == len(lst) else min(q, one)                  # (every chain shares the column: the sum of all posteriors); :4267
                    cache[share] = (q, bd) + phred_range(q, bd)
                out.append(cache[share])
            r["cols"].append(out)
    return r


def batch_units(batch, ext, contigs, mean, sd, unpaired=False, want_columns=True, capacities=True):
    """Every unit of a batch: None where capacity_refusal() holds (capacities = False: only where a record is flagged or a list is empty -- the reference
    program has no other limit), else pair_unit().  ext: the extended chains (hlala_chains_out layout, stage 1)."""
    tables = level_tables(contigs) if not unpaired else {}
    per = 1 if unpaired else 2
    co = np.asarray(batch["chain_off"]); rev = np.asarray(batch["chain_reverse"]); st = np.asarray(ext["status"])
    out = []
    for u in range(int(batch["n_pairs"])):
        lists, statuses = [], []
        for m in range(per):
            r = per * u + m
            cs = range(int(co[r]), int(co[r + 1]))
            statuses += [int(st[c]) for c in cs]
            lists.append([Chain(ext, c, rev[c]) for c in cs if st[c] == CHAIN_OK])
        no = capacity_refusal(lists, statuses) if capacities else (any(s < 0 for s in statuses) or any(len(l) < 1 for l in lists))
        out.append(None if no else pair_unit(lists, tables, mean, sd, want_columns))
    return out
