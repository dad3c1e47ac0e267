"""The exact model of the exon-position stage (csrc/kernel_exonpos.hip: k_exon_positions<0/1>, k_unit_stats), restated from the reference's text in plain
loops over alignment columns.  Plain Python and numpy: neither the oracle nor the library is used here.

  mate_positions          oneReadAlignment_2_exonPositions_paired / _unpaired   hla/HLATyper.cpp:3192-3565, :3568-3930
  weighted_ok             alignmentWeightedOKFraction                           :3933-4018
  fraction_ok             alignmentFractionOK                                   :3082-3101
  remove_double           removeDoublePositionsFromRead                         :4020-4083
  Model.exon_positions    the pair test :1404-1410, the read test :1476, the per-locus loop :1385-1494
  Model.unit_stats        the per-unit statistics                               :1043-1097
  intervals_overlap       Utilities::intervalsOverlap                           Utilities.cpp:168-176
  distance                alignedReadPair_pairsDistanceInGraphLevels            mapper/aligner/alignerBase.cpp:246-283

The merge is written as the reference writes it: both mates' lists are built in full, thrown together, grouped by graph level, and one alternative per level
is kept (the first one with the strictly best worst-quality).  Nothing here knows of cursors, passes or slots.

Inputs: a `pairs` dict in the layout of Batch.pairs() / Oracle.align_batch()["pairs"] (per mate row r: n_cols[r] and the columns col_level, col_gchar,
col_schar, col_mapq at [r * stride, r * stride + n_cols[r]); unpaired batches have one row per read), the batch (read_off, read_bases, read_quals and, for
read_reverse, chain_reverse), the stride, and a locus: dict(level_min, level_to_exon, insert_mean, insert_sd, min_mapq, min_weighted_ok, pair_mask,
min_alignment_columns).  pCorrect is DATA: the table of 256 doubles that the project itself builds (orc_phred on the CPU side, hlala_kat_phred on the GPU
side); it is not re-derived here.

Agreement.  Integers and characters: exact.  read_weighted_ok and read_fraction_ok: the model performs the same IEEE-754 binary64 operations in the same
(column) order as the reference -- additions of 1.0 or pCorrect, one division, one subtraction; no product, so nothing a compiler could contract -- and the
values must be bit-identical.  Both are also computed with fractions.Fraction, and the binary64 value must lie within the following bound of the exact one.

  weighted_ok = 1 - S / L, S = sum of k terms t_i in [0, 1] (k = columns that add a mismatch), L = read length, u = 2^-53, gamma_n = n u / (1 - n u).
    Recursive summation of non-negative terms: fl(S) = S (1 + theta_k), |theta_k| <= gamma_k (at most k roundings; Higham, Accuracy and Stability, 4.2).
    The division adds one rounding: q^ = (S / L)(1 + theta_{k+1}).  The subtraction adds one: w^ = (1 - q^)(1 + delta), |delta| <= u.  With q = S / L, w = 1 - q:
        |w^ - w| <= |q^ - q| + u |1 - q^| <= gamma_{k+1} q + u (|w| + gamma_{k+1} q) = u |w| + (1 + u) gamma_{k+1} q          =: weighted_bound(k, q, w)
  fraction_ok = ok / checked, two exact integers and one division: |f^ - f| <= u |f|                                              =: fraction_bound(f)

(The bounds are evaluated in exact rational arithmetic.  Most terms are the integer 1.0, whose partial sums are exact, so the observed error is far smaller.)
read_mapq holds posteriors that the device computes with its own exp(): rtol 1e-9, atol 1e-15, as tests/test_exon_positions.py has it."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
GAP = ord("_")
KEYS_INT = ("read_pair", "read_distance", "read_cols_nongap", "pos_off", "pos_exon", "pos_level", "pos_mate", "pos_mapq", "pos_novel_gap", "geno_off", "geno_chars", "qual_chars")
KEYS_COUNT = ("n_reads", "n_pos", "n_chars", "n_pairs_ok", "n_pairs_broken")
STATS_INT = ("valid", "strands_valid", "distance", "n_columns")


def gamma(n):
    return n * U / (1 - n * U)


def weighted_bound(k, q, w):
    return U * abs(w) + (1 + U) * gamma(k + 1) * q


def fraction_bound(f):
    return U * abs(f)


def make_locus(level_min, level_to_exon, insert_mean, insert_sd, min_mapq=0.0, min_weighted_ok=0.0, pair_mask=None, min_alignment_columns=1000):
    return dict(level_min=int(level_min), level_to_exon=np.asarray(level_to_exon, np.int32), insert_mean=float(insert_mean), insert_sd=float(insert_sd),
                min_mapq=float(min_mapq), min_weighted_ok=float(min_weighted_ok), pair_mask=None if pair_mask is None else np.asarray(pair_mask, np.uint8),
                min_alignment_columns=int(min_alignment_columns))


def locus_args(L):
    """The locus as the arguments of oracle_binding.exon_positions / Batch.exon_positions after (level_min, level_to_exon, insert_mean, insert_sd)."""
    return dict(min_mapq=L["min_mapq"], min_weighted_ok=L["min_weighted_ok"], pair_mask=L["pair_mask"], min_alignment_columns=L["min_alignment_columns"])


def intervals_overlap(x1, x2, y1, y2, drop=None):
    """Utilities::intervalsOverlap.  (`drop`: leave one comparison of the eight out -- a broken variant, for the checks that the suite bites.)"""
    t = [x1 >= y1, x1 <= y2, x2 >= y1, x2 <= y2, y1 >= x1, y1 <= x2, y2 >= x1, y2 <= x2]
    if drop is not None:
        t[drop] = True
    return (t[0] and t[1]) or (t[2] and t[3]) or (t[4] and t[5]) or (t[6] and t[7])


def first_level(lv):
    for x in lv:
        if x != -1:
            return int(x)
    return -1


def last_level(lv):
    for x in reversed(lv):
        if x != -1:
            return int(x)
    return -1


def distance(lv1, lv2):
    if first_level(lv1) < first_level(lv2):
        return first_level(lv2) - last_level(lv1) - 1
    return first_level(lv1) - last_level(lv2) - 1


def fraction_ok(g, s):
    """(binary64 value, exact value or None where no column was checked: 0 / 0 is a NaN in the reference)."""
    ok = checked = 0
    for gc, sc in zip(g, s):
        if gc == GAP and sc == GAP:
            continue
        checked += 1
        if gc == sc:
            ok += 1
    if checked == 0:
        return float("nan"), None
    return float(ok) / float(checked), Fraction(ok, checked)


def weighted_ok(g, s, quals, read_len, pcorrect):
    """(binary64 value, exact value, number of terms added)."""
    idx = -1; wm = 0.0; exact = Fraction(0); k = 0
    for gc, sc in zip(g, s):
        if sc != GAP:
            idx += 1
            if gc == GAP:
                wm += 1.0; exact += 1; k += 1
            elif sc != gc:
                pc = float(pcorrect[quals[idx]])
                wm += pc; exact += Fraction(pc); k += 1
        elif gc != GAP:
            wm += 1.0; exact += 1; k += 1
    return 1.0 - (wm / float(read_len)), 1 - exact / read_len, k


def mate_positions(lv, g, s, mq, quals, mate, strip=True):
    """Every position of one alignment, in or out of any exon (the first loop of oneReadAlignment_2_exonPositions_*): a position per column with a level;
    a column without one appends its base to the position before it, and where that position was a lone '_' the '_' is dropped.
    (`strip` False: the '_' stays -- a broken variant, for the checks that the suite bites.)"""
    n = len(lv)
    novel = [0] * n
    run = 0
    for c in range(n):
        if g[c] != GAP and s[c] != GAP:
            run = 0
        elif not (g[c] == GAP and s[c] == GAP):
            run += 1
        novel[c] = max(novel[c], run)
    run = 0
    for c in range(n - 1, -1, -1):
        if g[c] != GAP and s[c] != GAP:
            run = 0
        elif not (g[c] == GAP and s[c] == GAP):
            run += 1
        novel[c] = max(novel[c], run)
    out = []; idx = -1
    for c in range(n):
        if lv[c] == -1:
            idx += 1
            if out:
                p = out[-1]
                p["genotype"].append(int(s[c])); p["qualities"].append(int(quals[idx])); p["n_ins"] += 1
                if len(p["genotype"]) != len(p["qualities"]):
                    assert len(p["genotype"]) == len(p["qualities"]) + 1 and p["genotype"][0] == GAP
                    if strip:
                        p["genotype"] = p["genotype"][1:]; p["strip"] = True
                    else:
                        p["qualities"].insert(0, 0)
        else:
            p = dict(level=int(lv[c]), mate=mate, mapq=int(mq[c]), novel_gap=novel[c], n_ins=0, strip=False)
            if s[c] != GAP:
                idx += 1
                p["genotype"] = [int(s[c])]; p["qualities"] = [int(quals[idx])]
            else:
                p["genotype"] = [GAP]; p["qualities"] = []
            out.append(p)
    return out


def worst_quality(p):
    """getBestExonPosition's Q: 0 for the genotype "_", else the smallest quality character."""
    return 0 if p["genotype"] == [GAP] else min(p["qualities"])


def remove_double(positions, tie_to_later=False):
    """(`tie_to_later`: >= for > -- a broken variant, for the checks that the suite bites.)"""
    per_level = {}
    for p in positions:
        per_level.setdefault(p["level"], []).append(p)
    out = []
    for level in sorted(per_level):
        best = None; best_q = None
        for i, alt in enumerate(per_level[level]):
            q = worst_quality(alt)
            if i == 0 or (q >= best_q if tie_to_later else q > best_q):
                best, best_q = alt, q
        out.append(best)
    return out


class Model:
    """The per-mate work is done once per alignment (it does not depend on the locus); exon_positions() then runs the per-locus loop."""

    def __init__(self, pairs, batch, stride, pcorrect, unpaired=False, strip=True):
        self.pairs, self.batch, self.stride, self.unpaired = pairs, batch, int(stride), unpaired
        self.n = int(batch["n_pairs"]); self.per = 1 if unpaired else 2
        self.pcorrect = np.asarray(pcorrect, np.float64); assert self.pcorrect.shape == (256,)
        self.strip = strip
        self._mate = {}

    def mate(self, r):
        """Everything about the alignment in row r that no locus changes."""
        if r not in self._mate:
            P, B, st = self.pairs, self.batch, self.stride
            n = int(P["n_cols"][r]); sl = slice(r * st, r * st + n)
            lv = [int(x) for x in P["col_level"][sl]]; g = [int(x) for x in P["col_gchar"][sl]]; s = [int(x) for x in P["col_schar"][sl]]; mq = P["col_mapq"][sl]
            quals = np.asarray(B["read_quals"])[int(B["read_off"][r]):int(B["read_off"][r + 1])]
            w, w_exact, k = weighted_ok(g, s, quals, len(quals), self.pcorrect)
            f, f_exact = fraction_ok(g, s)
            self._mate[r] = dict(n=n, lv=lv, first=first_level(lv), last=last_level(lv), w=w, w_exact=w_exact, w_terms=k, f=f, f_exact=f_exact,
                                 cols_nongap=sum(1 for x in s if x != GAP), positions=mate_positions(lv, g, s, mq, quals, 1 + (r % 2 if self.per == 2 else 0), self.strip),
                                 starts_with_insertion=bool(n and lv[0] == -1), ends_with_insertion=bool(n and lv[-1] == -1))
        return self._mate[r]

    def fp_ratio(self, rows):
        """Largest |binary64 - exact| / bound over the weighted and the plain OK fractions of the given rows; asserts the bounds."""
        worst = 0.0
        for r in rows:
            m = self.mate(r)
            b = weighted_bound(m["w_terms"], 1 - m["w_exact"], m["w_exact"]); e = abs(Fraction(m["w"]) - m["w_exact"])
            assert e <= b, ("weighted_ok", r, float(e), float(b))
            if b:
                worst = max(worst, float(e / b))
            if m["f_exact"] is not None:
                b = fraction_bound(m["f_exact"]); e = abs(Fraction(m["f"]) - m["f_exact"])
                assert e <= b, ("fraction_ok", r, float(e), float(b))
                if b:
                    worst = max(worst, float(e / b))
        return worst

    def in_exon(self, m, L, drop=None):
        """The second loop of oneReadAlignment_2_exonPositions_*: (used, the positions on exon levels with their exon position)."""
        lmin = L["level_min"]; l2e = L["level_to_exon"]; lmax = lmin + len(l2e) - 1
        assert m["first"] <= m["last"]
        if not intervals_overlap(m["first"], m["last"], lmin, lmax, drop):
            return False, []
        out = []
        for p in m["positions"]:
            if lmin <= p["level"] <= lmax and l2e[p["level"] - lmin] >= 0:
                out.append(dict(p, exon=int(l2e[p["level"] - lmin])))
        return True, out

    def pair_test(self, u, L, strict_insert=False):
        """:1404-1410 (pairs), :1476 (single reads).  (`strict_insert`: < for <= -- a broken variant.)"""
        P = self.pairs
        if self.unpaired:
            return bool(P["mate_mapq"][u] >= L["min_mapq"]) and self.mate(u)["n"] >= L["min_alignment_columns"]
        a, b = self.mate(2 * u), self.mate(2 * u + 1)
        d = abs(float(distance(a["lv"], b["lv"])) - L["insert_mean"])
        return bool(P["strands_valid"][u]) and (d < 5 * L["insert_sd"] if strict_insert else d <= 5 * L["insert_sd"]) and bool(P["mate_mapq"][2 * u] >= L["min_mapq"]) \
            and a["w"] >= L["min_weighted_ok"] and b["w"] >= L["min_weighted_ok"]

    def accepted(self, L, **broken):
        """(unit, [used per mate], [in-exon positions per mate]) of every unit that passes the test, and the two counters."""
        out = []; ok = bad = 0
        for u in range(self.n):
            if L["pair_mask"] is not None and not L["pair_mask"][u]:
                continue
            if self.pairs["pair_status"][u] != 0:
                continue
            if not self.pair_test(u, L, broken.get("strict_insert", False)):
                bad += 1
                continue
            ok += 1
            rows = [u] if self.unpaired else [2 * u, 2 * u + 1]
            ul = [self.in_exon(self.mate(r), L, broken.get("drop")) for r in rows]
            out.append((u, [x[0] for x in ul], [x[1] for x in ul]))
        return out, ok, bad

    def exon_positions(self, L, **broken):
        """The dict of oracle_binding.exon_positions / Batch.exon_positions (read_reverse only where the pairs dict names the selected chains)."""
        P, B = self.pairs, self.batch
        acc, ok, bad = self.accepted(L, **broken)
        d = {k: [] for k in KEYS_INT + ("read_weighted_ok", "read_fraction_ok", "read_mapq", "read_reverse")}
        d["pos_off"].append(0); d["geno_off"].append(0)
        for u, used, lists in acc:
            if self.unpaired:
                final = lists[0]
            else:
                final = remove_double(lists[0] + lists[1], broken.get("tie_to_later", False)) if lists[0] or lists[1] else []
            if not final:
                continue
            rows = [u] if self.unpaired else [2 * u, 2 * u + 1]
            m = [self.mate(r) for r in rows]
            d["read_pair"].append(u)
            d["read_distance"].append(-1 if self.unpaired else distance(m[0]["lv"], m[1]["lv"]))
            for i in range(2):
                have = i < len(m)
                d["read_weighted_ok"].append(m[i]["w"] if have else -1.0); d["read_fraction_ok"].append(m[i]["f"] if have else -1.0)
                d["read_cols_nongap"].append(m[i]["cols_nongap"] if have and used[i] else 0)
                d["read_mapq"].append(float(P["mate_mapq"][rows[i]]) if have else -1.0)
                if "best_chain" in P and "chain_reverse" in B:
                    d["read_reverse"].append(int(B["chain_reverse"][int(P["best_chain"][rows[i]])]) if have else 0)
            for p in final:
                d["pos_exon"].append(p["exon"]); d["pos_level"].append(p["level"]); d["pos_mate"].append(p["mate"]); d["pos_mapq"].append(p["mapq"])
                d["pos_novel_gap"].append(p["novel_gap"])
                d["geno_chars"] += p["genotype"]; d["qual_chars"] += p["qualities"] if p["qualities"] else [0]
                d["geno_off"].append(len(d["geno_chars"]))
            d["pos_off"].append(len(d["pos_exon"]))
        dt = dict(read_weighted_ok=np.float64, read_fraction_ok=np.float64, read_mapq=np.float64, pos_mate=np.uint8, pos_mapq=np.uint8, geno_chars=np.uint8,
                  qual_chars=np.uint8, read_reverse=np.uint8)
        out = {k: np.asarray(v, dt.get(k, np.int32)) for k, v in d.items()}
        if not ("best_chain" in P and "chain_reverse" in B):
            del out["read_reverse"]
        assert len(out["geno_chars"]) == len(out["qual_chars"])
        out.update(n_reads=len(out["read_pair"]), n_pos=len(out["pos_exon"]), n_chars=len(out["geno_chars"]), n_pairs_ok=ok, n_pairs_broken=bad)
        return out

    def unit_stats(self):
        """The arrays of hlala_unit_alignment_stats: what :1043-1097 reads off every unit; all zero (valid = 0) for a unit without a selected alignment."""
        n, P = self.n, self.pairs
        d = dict(valid=np.zeros(n, np.uint8), strands_valid=np.zeros(n, np.uint8), distance=np.zeros(n, np.int32), fraction_ok=np.zeros(2 * n), weighted_ok=np.zeros(2 * n),
                 n_columns=np.zeros(2 * n, np.int32), mate_mapq=np.zeros(2 * n))
        for u in range(n):
            if P["pair_status"][u] != 0:
                continue
            rows = [u] if self.unpaired else [2 * u, 2 * u + 1]
            for i, r in enumerate(rows):
                m = self.mate(r)
                d["fraction_ok"][2 * u + i] = m["f"]; d["weighted_ok"][2 * u + i] = m["w"]; d["n_columns"][2 * u + i] = m["n"]; d["mate_mapq"][2 * u + i] = P["mate_mapq"][r]
            if self.unpaired:
                d["fraction_ok"][2 * u + 1] = -1; d["weighted_ok"][2 * u + 1] = -1; d["mate_mapq"][2 * u + 1] = -1; d["distance"][u] = -1
            else:
                d["strands_valid"][u] = P["strands_valid"][u]
                d["distance"][u] = distance(self.mate(rows[0])["lv"], self.mate(rows[1])["lv"])
            d["valid"][u] = 1
        return d


def exon_positions(pairs, batch, stride, locus, pcorrect, unpaired=False):
    return Model(pairs, batch, stride, pcorrect, unpaired).exon_positions(locus)


def unit_stats(pairs, batch, stride, pcorrect, unpaired=False):
    return Model(pairs, batch, stride, pcorrect, unpaired).unit_stats()


def compare(got, exp, label, mapq_exact=False, reverse=True):
    """`got` (the library's or the oracle's dict) against `exp` (the model's, or the oracle's) under the agreement rules of this module."""
    for k in KEYS_COUNT:
        assert got[k] == exp[k], (label, k, got[k], exp[k])
    for k in KEYS_INT:
        assert np.array_equal(got[k], exp[k]), (label, k)
    assert np.array_equal(got["read_weighted_ok"], exp["read_weighted_ok"]), (label, "read_weighted_ok")
    assert np.array_equal(got["read_fraction_ok"], exp["read_fraction_ok"], equal_nan=True), (label, "read_fraction_ok")
    if mapq_exact:
        assert np.array_equal(got["read_mapq"], exp["read_mapq"]), (label, "read_mapq")
    else:
        assert np.allclose(got["read_mapq"], exp["read_mapq"], rtol=1e-9, atol=1e-15), (label, "read_mapq")
    if reverse and "read_reverse" in exp and "read_reverse" in got:
        assert np.array_equal(got["read_reverse"], exp["read_reverse"]), (label, "read_reverse")


def compare_stats(got, exp, label, mapq_exact=True):
    for k in STATS_INT:
        assert np.array_equal(got[k], exp[k]), (label, k)
    for k in ("fraction_ok", "weighted_ok"):
        assert np.array_equal(got[k], exp[k], equal_nan=True), (label, k)
    if mapq_exact:
        assert np.array_equal(got["mate_mapq"], exp["mate_mapq"]), (label, "mate_mapq")
    else:
        assert np.allclose(got["mate_mapq"], exp["mate_mapq"], rtol=1e-9, atol=1e-15), (label, "mate_mapq")
