"""Inputs of the pairing edge tests (stage C: k_pair_chains, k_pair_multi<., false>, k_pair_multi<., true>, pair_insert_ll, pair_positions) and the checks both
sides have to pass on them: tests/test_pair_reference.py holds the oracle, tests/test_gpu_pair_edges.py the kernels, against tests/pair_reference.py.
Plain numpy: neither the oracle nor the library is used here.  Every family is a function of its arguments alone, built once per process.

A family is a dict: world, batch, kept (expected kept records per read: [2 n_pairs], or [n_reads] for the unpaired family), refused (pairs the library refuses:
more than 64 kept records on a mate, more than 1024 combinations, a flagged record), oracle_fails (pairs that the oracle cannot be given: it raises on them),
max_columns, floors.

How the record counts are made.  The duplicate-coordinate filter of alignOneReadPair (processBAM.cpp:3200-3240) keys a record on the levels of its first and last
reference base, so the same read on another haplotype at the same levels is dropped; a record that soft-clips k more bases at its left end (position + k) has a
key of its own and is kept.  Left alone, such records extend back to one and the same alignment (equal likelihoods, every column shared); variant k therefore
carries the CIGAR  kS (x-k)M 1D sM 1I (L-x-s-1)M  with x = 10 + 2k and s = 1 + k % 5, which moves s bases one level to the right.  Every second record is
moreover placed one level to the right as a whole (its "register"), so that no column of the selected chain is shared by every chain of its list, and the
quality bytes are a mix of Phred 1 (a mismatch scores above a match) and Phred 2, which keeps the two registers within some ten nats: a per-column confidence
then stays away from 1 by far more than its rounding error and its Phred byte is decided (tests/pair_reference.py).  The reads are chosen clear of gap stretches
and level skips, where the projection cuts seeds back and the extension puts all variants on the same columns again.  Columns of a mate with ONE kept chain
cannot be helped: their confidence is the sum of all posteriors, exactly 1, and they are counted apart ("whole_one_chain"); in a mate with several kept
chains such columns count as undecided."""
import functools

import numpy as np

import ref_pipeline as rp
from tools import synth

PAIR_CHAINS, PAIR_COMB, PAIR_COMB_LDS, PAIR_COLS = 64, 1024, 128, 512          # csrc/kernel_pair.hip
Q1_TENTHS = 6


# ------------------------------------------------------------------------------------------------ batches as lists of reads
def explode(b, per_unit=2):
    """The reads of batch `b`: dicts of bases, quals, records (contig, pos, offset, AS, rev, cig) and the index of the primary record."""
    ro, co = np.asarray(b["read_off"], np.int64), np.asarray(b["chain_off"], np.int64)
    reads = []
    for r in range(per_unit * b["n_pairs"]):
        recs = [dict(contig=int(b["chain_contig"][c]), pos=int(b["chain_pos"][c]), offset=int(b["chain_offset"][c]), AS=int(b["chain_as"][c]),
                     rev=int(b["chain_reverse"][c]), cig=rp.cigar_of(b, c)) for c in range(co[r], co[r + 1])]
        reads.append(dict(bases=np.asarray(b["read_bases"])[ro[r]:ro[r + 1]].copy(), quals=np.asarray(b["read_quals"])[ro[r]:ro[r + 1]].copy(), recs=recs,
                          primary=int(b["read_primary"][r]) - int(co[r])))
    return reads


def assemble(reads, insert_mean, insert_sd, per_unit=2):
    """Inverse of explode: the hlala_batch_in layout.  The AS values of a read are rewritten to fall by one per record (the layout asks for descending order;
    equal keys are decided by the order then: the later record is the duplicate)."""
    recs = [x for rd in reads for x in rd["recs"]]
    AS = [200 - i for rd in reads for i in range(len(rd["recs"]))]
    enc = [[(l << 4) | rp.OP[o] for l, o in x["cig"] if l > 0] for x in recs]
    co = np.concatenate([[0], np.cumsum([len(rd["recs"]) for rd in reads])])
    b = dict(n_pairs=len(reads) // per_unit, n_chains=len(recs),
             read_off=np.concatenate([[0], np.cumsum([len(rd["bases"]) for rd in reads])]).astype(np.int32),
             read_bases=np.concatenate([rd["bases"] for rd in reads]).astype(np.uint8), read_quals=np.concatenate([rd["quals"] for rd in reads]).astype(np.uint8),
             chain_off=co.astype(np.int32), read_primary=np.asarray([co[i] + rd["primary"] for i, rd in enumerate(reads)], np.int32),
             chain_contig=np.asarray([x["contig"] for x in recs], np.int32), chain_pos=np.asarray([x["pos"] for x in recs], np.int32),
             chain_offset=np.asarray([x["offset"] for x in recs], np.int32), chain_as=np.asarray(AS, np.int32),
             chain_reverse=np.asarray([x["rev"] for x in recs], np.uint8),
             cigar_off=np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int32), cigar=np.asarray([v for e in enc for v in e], np.uint32),
             insert_mean=float(insert_mean), insert_sd=float(insert_sd))
    return b


def placed(rec, L, reg, k, local=True):
    """Record `rec` ([L M], no clips) in register `reg` (the whole read moved that many levels to the right) with k more bases soft-clipped at the left end;
    local: s = 1 + k % 5 bases after x = 10 + 2k moved one more level to the right (1D sM 1I).  The filter's key -- the levels of the first and the last
    reference base -- is (first + reg + k, last + reg): records with different (reg, k) are all kept.  Without `local` the records of one register extend back
    to one and the same alignment: equal log likelihoods, every column shared."""
    assert [o for _, o in rec["cig"]] == ["M"] and rec["cig"][0][0] == L
    x, s = 10 + 2 * k, 1 + k % 5
    assert L - x - s - 1 >= 1
    cig = [(k, "S"), (x - k, "M"), (1, "D"), (s, "M"), (1, "I"), (L - x - s - 1, "M")] if local else [(k, "S"), (L - k, "M")]
    return dict(rec, pos=rec["pos"] + reg + k, cig=cig)


def variant(rec, i, L):
    """Kept record number i of a read: register i % 2, clip i // 2, locally shifted."""
    return placed(rec, L, i % 2, i // 2)


def with_good_at(rd, n, good):
    """n kept records: at the list positions `good` records without indels in register 0 (clips 0, 1, ...: equal chains, some fourteen nats above every other),
    elsewhere records of register 1, two of every four locally shifted (the others are equal chains again, some fourteen nats below)."""
    L = len(rd["bases"]); g = 0; recs = []
    for i in range(n):
        if i in good:
            recs.append(placed(rd["recs"][0], L, 0, g, local=False)); g += 1
        else:
            recs.append(placed(rd["recs"][0], L, 1, i, local=i % 4 >= 2))
    return dict(rd, recs=recs, primary=min(good), quals=low_quals(L))


def low_quals(L, q1_tenths=Q1_TENTHS):
    """Quality bytes '"' (Phred 1: a mismatch scores 0.25 nats above a match) and '#' (Phred 2: 0.56 below) mixed so that a read moved by one level scores within
    some ten nats of the read in place."""
    return np.where((np.arange(L) * 7) % 10 < q1_tenths, 34, 35).astype(np.uint8)


FAR = 40


def far(rec, L, sign=1):
    """The record forty positions to the right, without indels: it shares no column with any variant in place (no read base on the same level), costs about what
    a register costs, and its distance to the other mate is forty more or less -- about a standard deviation.  Where the projection cuts seeds back and the
    extension puts the variants in place on the same columns again, this record keeps its own."""
    return dict(rec, pos=rec["pos"] + sign * FAR, cig=[(L, "M")])


def with_variants(rd, n, reverse=False, q1_tenths=Q1_TENTHS, with_far=0):
    """Read `rd` (one record) with n kept records: the variants 0 .. n-1 (with_far = 1 or -1: n - 1 of them and far() to that side as the last), in reverse order if asked (the best
    record then usually is not the first one)."""
    L = len(rd["bases"])
    recs = [variant(rd["recs"][0], i, L) for i in range(n - int(bool(with_far)))] + ([far(rd["recs"][0], L, with_far)] if with_far else [])
    if reverse:
        recs = recs[::-1]
    return dict(rd, recs=recs, primary=(n - 1 if reverse else 0), quals=low_quals(L, q1_tenths))


def wrong_strand(rec):
    return dict(rec, rev=1 - rec["rev"])


def interleaved(rd, n_records, n_kept, seed):
    """Read with n_records records of which n_kept survive the filters, spread evenly from the first to the last record (one kept record: the last one, so that
    the list is filled from the second block of 64 alone); the others alternately a record on the other strand than the primary's (skipped,
    processBAM.cpp:3216) and an exact copy of an earlier kept record (a duplicate, :3234).  The primary is the first kept record."""
    L = len(rd["bases"])
    at = sorted({int(round(i * (n_records - 1) / (n_kept - 1))) for i in range(n_kept)}) if n_kept > 1 else [n_records - 1]
    assert len(at) == n_kept
    recs, k = [], 0
    for i in range(n_records):
        if k < n_kept and i == at[k]:
            recs.append(variant(rd["recs"][0], k, L)); k += 1
        elif i % 2 or k == 0:
            recs.append(wrong_strand(variant(rd["recs"][0], (i * 7 + seed) % 60, L)))
        else:
            recs.append(dict(recs[at[(i + seed) % k]]))
    return dict(rd, recs=recs, primary=at[0], quals=low_quals(L))


def base_world():
    """Five haplotypes with substitutions and single-level gaps, no long gap (gap stretches -- three gap levels in a row -- are rare)."""
    return _world(11, 6000, 1, 3, n_largegap=0)


@functools.lru_cache(maxsize=None)
def _world(seed, G, k, n_mut, **kw):
    return synth.make_world(seed=seed, G=G, k=k, n_mut=n_mut, **kw)


def _base_reads(w, n_pairs, seed, margin=40, skips=0, candidates=None, **kw):
    """The reads of n_pairs pairs with one record per read, [L M] (no clips, no indels, no secondaries), that lie clear of everything that makes the projection
    rewrite a record: within `margin` levels of either end of both mates the contig visits every level, and no level is in a gap stretch (where
    restrictInitialAlignmentToNoGapAreas cuts a seed back and the extension puts every variant of the read on the same columns again).  skips = 1: a read
    crosses at most one single level that its haplotype lacks, and at least one mate of every pair does, in its body (from base 60 on: behind the variants' own indels)."""
    b = synth.make_batch(w, candidates or 8 * n_pairs + 8, seed=seed, **dict(dict(p_secondary=0.0, indel_read_frac=0.0, p_no_clip=1.0), **kw))
    C = w["contigs"]; off = np.asarray(C["contig_off"]); lvl = np.asarray(C["contig_level"])
    gap = np.concatenate([rp.gap_stretch_rule(w["graph"]), [0]])
    reads = explode(b); keep = []
    for p in range(b["n_pairs"]):
        ok = True; crossed = 0
        for rd in reads[2 * p:2 * p + 2]:
            x = rd["recs"][0]; h = x["contig"]; a, z = x["pos"] - margin, x["pos"] + len(rd["bases"]) + margin
            if a < 0 or off[h] + z > off[h + 1]:
                ok = False; break
            lv = lvl[off[h] + a:off[h] + z]; d = np.diff(lv)
            at = np.nonzero(d != 1)[0] - margin          # where the contig skips a level, as an offset into the read
            crossed += len(at)
            ok = ok and len(at) <= skips and bool(np.all(d[d != 1] == 2)) and bool(np.all((at >= 60) & (at < len(rd["bases"]) - 10))) and not gap[lv[0]:lv[-1] + 1].any()
        if ok and crossed >= skips:
            keep.append(p)
    assert len(keep) >= n_pairs, (len(keep), n_pairs)
    return [reads[2 * p + m] for p in keep[:n_pairs] for m in range(2)]


def _refused(kept):
    k = np.asarray(kept).reshape(-1, 2)
    return [p for p in range(len(k)) if k[p].max() > PAIR_CHAINS or int(k[p, 0]) * int(k[p, 1]) > PAIR_COMB]


# ------------------------------------------------------------------------------------------------ the families
COUNTS = [(1, 1), (1, 2), (2, 1), (63, 1), (64, 1), (1, 64), (65, 1), (1, 65), (64, 2), (8, 8), (8, 16), (16, 8), (43, 3), (64, 16), (16, 64),
          (32, 32), (41, 25), (33, 32), (64, 64),
          (33, 31), (13, 5), (63, 2)]          # 1023, 65 and 126 combinations (127 is prime: no pair of lists of at most 64 has it)


# the pairs the library refuses come last: the batch without them numbers its chains alike, so the same random draws go into every extension
COUNTS_ORDERED = sorted(COUNTS, key=lambda c: max(c) > PAIR_CHAINS or c[0] * c[1] > PAIR_COMB)


@functools.lru_cache(maxsize=None)
def counts():
    """Kept chains per mate at 1, 2, 63, 64 and 65 (refused); combinations at 64, 65, 126, 128, 129 (43 x 3: the first that does not fit the LDS table), 1023, 1024,
    1025 (41 x 25), 1056 and 4096 (all three refused).  Every second pair holds its records in reverse order."""
    w = base_world()
    reads = _base_reads(w, len(COUNTS), seed=31)
    out, kept = [], []
    for p, (n1, n2) in enumerate(COUNTS_ORDERED):
        for m, n in enumerate((n1, n2)):
            out.append(with_variants(reads[2 * p + m], n, reverse=bool(p % 2))); kept.append(n)
    return dict(name="counts", world=w, batch=assemble(out, 200.0, 35.0), kept=np.asarray(kept), refused=_refused(kept), oracle_fails=[], max_columns=384,
                floors=dict(multi=15, mapq_lt1=15, not_first=7, distinct_mapq=10))


# ------------------------------------------------------------------------------------------------ the checks
def without(f, units):
    """The family's batch without the given units (which must be its last ones: the chains of the others keep their numbers)."""
    n = f["batch"]["n_pairs"]
    assert sorted(units) == list(range(n - len(units), n))
    return rp.subset_units(f["batch"], range(n - len(units)), per_unit=1 if f.get("unpaired") else 2) if units else f["batch"]


_ORACLE = {}


def oracle_answers(oracle_cls, f, rng_seed=5):
    """What the oracle (the class is handed in) makes of the family's batch without the units it cannot be given; once per process."""
    if f["name"] not in _ORACLE:
        b = dict(without(f, f["oracle_fails"]), insert_mean=f["batch"]["insert_mean"], insert_sd=f["batch"]["insert_sd"])
        o = oracle_cls(f["world"]["graph"], f["world"]["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=rng_seed, max_columns=f["max_columns"])
        _ORACLE[f["name"]] = (b, o.align_long_reads(b) if f.get("unpaired") else o.align_batch(b))
        o.close()
    return _ORACLE[f["name"]]



def kept_counts(batch, status, per_unit=2):
    co = np.asarray(batch["chain_off"])
    return np.array([int((status[co[r]:co[r + 1]] == 0).sum()) for r in range(per_unit * batch["n_pairs"])])


def check_units(units, got, label, per_unit=2, refused=()):
    """The outputs `got` (hlala_pairs_out layout) of every unit against tests/pair_reference.py's `units`: integers equal, doubles within the derived bounds,
    Phred bytes equal where decided and inside their range where not (undecided: confidence below 1; whole: confidence 1 at sixty digits, as of a column that
    every chain of the list shares, which may hold the bytes of pr.whole_bytes() only; whole_one_chain: those of a mate with one kept chain, where no input can
    avoid them -- see tests/pair_reference.py).  Units in `refused` (and units the reference has no answer for) must carry exactly
    pair_status -1, best_chain -1, n_combinations 0.  Returns the statistics: largest error / bound ratios, columns, undecided columns, distinct bytes."""
    import pair_reference as pr
    st = got["_stride"]
    s = dict(units=0, multi=0, mapq_ratio=0.0, mate_ratio=0.0, ll_differ=0, columns=0, undecided=0, whole=0, whole_one_chain=0, mapq_lt1=0, not_first=0, distinct_mapq=0, refused=0, invalid_strands=0, gap_columns=0, inserted_columns=0)
    for u, ref in enumerate(units):
        rows = range(per_unit * u, per_unit * u + per_unit)
        if ref is None or u in refused:
            assert got["pair_status"][u] == -1 and got["n_combinations"][u] == 0 and all(got["best_chain"][r] == -1 and got["n_cols"][r] == 0 for r in rows), (label, u, "refusal")
            s["refused"] += 1
            continue
        assert got["pair_status"][u] == 0, (label, u, "pair_status", int(got["pair_status"][u]))
        assert got["n_combinations"][u] == ref["n_comb"], (label, u, "n_combinations")
        assert [int(got["best_chain"][r]) for r in rows] == ref["best_chain"], (label, u, "best_chain", ref["best"])
        if per_unit == 2:
            assert bool(got["strands_valid"][u]) == ref["strands_valid"], (label, u, "strands_valid")
        assert got["pair_ll"][u] == ref["pair_ll"], (label, u, "pair_ll", float(got["pair_ll"][u]), ref["pair_ll"])
        s["units"] += 1; s["multi"] += int(ref["n_comb"] > 1); s["not_first"] += int(ref["best"] != 0); s["invalid_strands"] += int(per_unit == 2 and not ref["strands_valid"])
        n = ref["n_comb"]
        q = pr.MP.mpf(float(got["pair_mapq"][u]))
        bound = float(ref["mapq"]) * pr.posterior_bound(n, 0.0)
        err = float(abs(q - ref["mapq"]))
        assert err <= bound, (label, u, "pair_mapq", err, bound)
        if n > 1:
            s["mapq_ratio"] = max(s["mapq_ratio"], err / bound)
        s["mapq_lt1"] += int(got["pair_mapq"][u] < 1)
        for m, r in enumerate(rows):
            v, bd = ref["mate"][m]
            err = float(abs(pr.MP.mpf(float(got["mate_mapq"][r])) - v))
            assert err <= bd, (label, u, "mate_mapq", m, err, bd)
            if n > 1:
                s["mate_ratio"] = max(s["mate_ratio"], err / bd)
            cols = ref["cols"][m]
            assert got["n_cols"][r] == len(cols), (label, u, "n_cols", m)
            mq = got["col_mapq"][r * st:r * st + len(cols)]
            if n > 1:
                s["gap_columns"] += int(((got["col_gchar"][r * st:r * st + len(cols)] == 95) & (got["col_schar"][r * st:r * st + len(cols)] == 95)).sum())
                s["inserted_columns"] += int((got["col_level"][r * st:r * st + len(cols)] == -1).sum())
            s["distinct_mapq"] = max(s["distinct_mapq"], len(set(mq.tolist())))
            one_chain = (ref["n1"], ref["n2"])[m] == 1
            for j, (q, bd, exact, lo, hi) in enumerate(cols):
                s["columns"] += 1
                if lo == hi:
                    assert mq[j] == exact, (label, u, "col_mapq", m, j, int(mq[j]), exact)
                elif q == 1:
                    s["whole_one_chain" if one_chain else "whole"] += 1
                    assert int(mq[j]) in pr.whole_bytes(bd), (label, u, "col_mapq of a column with confidence 1", m, j, int(mq[j]))
                    continue
                else:
                    s["undecided"] += 1
                    assert lo <= mq[j] <= hi, (label, u, "col_mapq undecided", m, j, int(mq[j]), lo, hi)
    return s


def check_floors(s, floors, label):
    """What a family has to hold for the comparison to mean something: the family's own floors; in every family with several combinations at least one pair with a
    posterior below 1 and one whose best combination is not the first; and no more than 1 % of the columns undecided -- the columns with confidence 1 in mates
    with several kept chains count as undecided here, only those of one-chain mates (which the families must have) do not."""
    print("%s: %s" % (label, {k: (float("%.3g" % v) if isinstance(v, float) else v) for k, v in s.items()}))
    assert s["undecided"] + s["whole"] <= 0.01 * max(1, s["columns"] - s["whole_one_chain"]), (label, "undecided columns", s["undecided"], s["whole"], s["columns"])
    if s["multi"]:
        floors = dict(dict(mapq_lt1=1, not_first=1), **floors)
    for k, v in floors.items():
        assert s[k] >= v, (label, k, s[k], v)


# (n1, n2, positions of the good chains in list 1, in list 2): the first maximum is combination min(good1) * n2 + min(good2)
MAXIMA = [(2, 64, (1,), (0,)), (3, 64, (2,), (0,)), (32, 32, (31,), (31,)), (5, 7, (4,), (6,)), (1, 64, (0,), (63,)), (64, 1, (63,), (0,)), (2, 64, (0,), (63,)),
          (3, 40, (0, 2), (5,)), (3, 59, (1, 2), (11,)), (4, 33, (1, 3), (2, 32)), (9, 15, (8,), (1, 14))]


@functools.lru_cache(maxsize=None)
def maxima(reverse=False):
    """Where the maximum is: the last combination, combinations 63, 64, 128 and 1023, and maxima attained by equal log likelihoods in different strides of 64
    (3 x 40: combinations 5 and 85; 3 x 59: 70 and 129, the later one in the lower lane; 4 x 33: 35, 65, 101 and 131).  reverse: every read's records in
    reverse order."""
    w = base_world()
    reads = _base_reads(w, len(MAXIMA), seed=32)
    out, kept, best = [], [], []
    for p, (n1, n2, g1, g2) in enumerate(MAXIMA):
        out += [with_good_at(reads[2 * p], n1, g1), with_good_at(reads[2 * p + 1], n2, g2)]; kept += [n1, n2]
        best.append((n1 - 1 - max(g1)) * n2 + (n2 - 1 - max(g2)) if reverse else min(g1) * n2 + min(g2))
    b = assemble(out, 200.0, 35.0)
    return dict(name="maxima reversed" if reverse else "maxima", world=w, batch=rp.reversed_chain_order(b) if reverse else b, kept=np.asarray(kept), refused=[],
                oracle_fails=[], max_columns=384, best=best, floors=dict(not_first=sum(x != 0 for x in best), mapq_lt1=len(MAXIMA)))


# (records, kept) of mate 1 and of mate 2
RECORDS = [((65, 1), (3, 3)), ((70, 2), (5, 5)), ((128, 63), (2, 2)), ((130, 64), (16, 16)), ((4, 4), (130, 64)), ((1, 1), (70, 63)), ((65, 64), (65, 1)), ((128, 2), (128, 2)),
           ((2, 2), (2, 2))]
ERROR_PAIR = 7          # its first mate gets a 66th record ... see records()
SINGLE_BASE = [(74, "S"), (1, "M"), (75, "S")]          # one aligned base: assert(startInRaw < stopInRaw), processBAM.cpp:5252; flagged HLALA_CHAIN_ERR_INPUT


@functools.lru_cache(maxsize=None)
def records(with_error=False):
    """Mates with more than 64 records of which at most 64 are kept, kept ones in both blocks of 64 records.  with_error: one more pair (a copy of pair 0's
    content) whose first mate has 66 records, the 66th with a single aligned base: the library flags the record and refuses the pair, the oracle raises."""
    w = base_world()
    spec = RECORDS + ([((66, 1), (3, 3))] if with_error else [])
    reads = _base_reads(w, len(spec), seed=33)
    out, kept = [], []
    for p, mates in enumerate(spec):
        for m, (nr, nk) in enumerate(mates):
            rd = reads[2 * p + m]
            if nr == nk:
                rd = with_variants(rd, nk, reverse=bool(p % 2))
            elif nr == 66:
                rd = interleaved(rd, 65, 1, seed=p)
                rd["recs"].append(dict(rd["recs"][64], cig=SINGLE_BASE))
            else:
                rd = interleaved(rd, nr, nk, seed=p + m)
            out.append(rd); kept.append(nk)
    return dict(name="records" + (" with an error record" if with_error else ""), world=w, batch=assemble(out, 200.0, 35.0), kept=np.asarray(kept),
                refused=[len(RECORDS)] if with_error else [], oracle_fails=[len(RECORDS)] if with_error else [], max_columns=384, floors=dict(not_first=3, mapq_lt1=5, multi=8))


# class of pair p of the 17: 0 = up to 128 combinations (k_pair_multi<., false>), 1 = more (k_pair_multi<., true>), None = one combination (k_pair_chains)
DRAW_CLASSES = [0, 1, None, 0, 1, 0, 1, 0, 1, 0, 1, None, None, None, None, None, None]
DRAW_SIZES = (1, 2, 7, 8, 9, 17)


@functools.lru_cache(maxsize=None)
def draws(n_pairs=17):
    """Batch sizes around the draws of eight pairs (k_pair_chains) and of four list entries (k_pair_multi): the first n_pairs of 17 pairs, whose lists hold
    1, 1, 3, 4, 4 and 5 (class 0) and 0, 1, 3, 3, 4 and 5 (class 1) entries at n_pairs = 1, 2, 7, 8, 9, 17."""
    w = base_world()
    reads = _base_reads(w, 17, seed=34)
    out, kept = [], []
    for p, c in enumerate(DRAW_CLASSES[:n_pairs]):
        n1, n2 = {None: (1, 1), 0: (2 + p % 3, 3), 1: (13, 10 + p % 2)}[c]
        out += [with_variants(reads[2 * p], n1, reverse=not p % 2), with_variants(reads[2 * p + 1], n2)]; kept += [n1, n2]          # (pair 0 in reverse order: the batch of one pair has a best combination that is not the first)
    return dict(name="draws of %d" % n_pairs, world=w, batch=assemble(out, 200.0, 35.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=384,
                floors=dict(multi=sum(c is not None for c in DRAW_CLASSES[:n_pairs]), mapq_lt1=sum(c is not None for c in DRAW_CLASSES[:n_pairs])))


def expected_classes(kept, n_cols_max, refused=()):
    """(pairs of class 0, pairs of class 1) as k_pair_chains lists them: several combinations; class 0 = at most 128 of them and no chain over 192 columns."""
    k = np.asarray(kept).reshape(-1, 2)
    c0 = c1 = 0
    for p in range(len(k)):
        n = int(k[p, 0]) * int(k[p, 1])
        if p in refused or n <= 1:
            continue
        if n <= PAIR_COMB_LDS and n_cols_max[p] <= 192:
            c0 += 1
        else:
            c1 += 1
    return c0, c1


def _direct_pair(w, h, s, L, d, quals):
    """A pair read off contig h: mate 1 forward at position s, mate 2 reverse, d bases between them (the inner distance on that contig); one record each."""
    C = w["contigs"]; off = int(C["contig_off"][h]); seq = np.asarray(C["contig_seq"])
    t = s + L + d
    assert s >= 0 and t >= 0 and off + max(s, t) + L + 2 <= int(C["contig_off"][h + 1])
    mk = lambda pos, rev: dict(bases=seq[off + pos:off + pos + L].copy(), quals=quals.copy(), primary=0,
                               recs=[dict(contig=h, pos=pos, offset=0, AS=L, rev=rev, cig=[(L, "M")])])
    return [mk(s, 0), mk(t, 1)]


def two_registers(rd):
    """The read with two kept records: in place and one level to the right, no indels."""
    L = len(rd["bases"])
    return dict(rd, recs=[placed(rd["recs"][0], L, 0, 0, local=False), placed(rd["recs"][0], L, 1, 0, local=False)])


INSERT_MEAN, INSERT_SD = 100.0, 3.0
INSERT_DMIN, INSERT_DMAX = -22, 222          # floor(mean - 40 sd) - 2, ceil(mean + 40 sd) + 2: the ends of the library's table of log densities


@functools.lru_cache(maxsize=None)
def insert_ends():
    """insert_mean = 100, insert_sd = 3: the table of log densities spans -22 .. 222.  At every inner distance d from -25 to 225 one pair with one combination
    and one with two (mate 2 in place and one level to the right: distances d and d + 1); negative distances are overlapping mates.  Then six pairs with both
    mates on one strand, six with the reverse mate upstream (strands not valid) and six whose mates are in the wrong order for their strands.
    Reads of 100 bases off haplotype 0, which visits every level."""
    w = base_world(); L = 100
    q = low_quals(L, 7)
    out, kept, dist = [], [], []
    for d in range(INSERT_DMIN - 3, INSERT_DMAX + 4):
        s = 300 + 17 * (d - INSERT_DMIN)
        a = _direct_pair(w, 0, s, L, d, q); out += a; kept += [1, 1]; dist.append([d])
        a = _direct_pair(w, 0, s + 9, L, d, q); out += [a[0], two_registers(a[1])]; kept += [1, 2]; dist.append([d, d + 1])
    for i in range(18):
        a = _direct_pair(w, 0, 400 + 40 * i, L, 95 + i % 6, q)
        if i % 3 == 0:
            a[1]["recs"][0]["rev"] = 0                                                   # both forward
        elif i % 3 == 1:
            a[0]["recs"][0]["rev"] = 1; a[1]["recs"][0]["rev"] = 1                       # both reverse
        else:
            a[0]["recs"][0]["rev"] = 1; a[1]["recs"][0]["rev"] = 0                       # the reverse mate upstream: first levels in the wrong order
        out += [two_registers(a[0]), a[1]]; kept += [2, 1]; dist.append(None)
    return dict(name="insert ends", world=w, batch=assemble(out, INSERT_MEAN, INSERT_SD), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=384, dist=dist,
                floors=dict(multi=251, mapq_lt1=200, not_first=60, invalid_strands=18))


COLUMN_LENGTHS = (190, 191, 192, 193, 194)


@functools.lru_cache(maxsize=None)
def columns():
    """max_columns = 512.  Reads of 190 .. 194 bases without clips or indels, two kept records on mate 1 (in place and one level to the right: chains of exactly
    as many columns as the read has bases) and three on mate 2 (with one-base indels: one column more): selected chains of 192 columns (three per lane)
    and of 193 (eight per lane) with six combinations.  Then reads of 480 bases with 2 x 3 and 13 x 10 combinations (ordinals and relative levels near
    511).  (Chains beyond the cap of 512: too_long().)"""
    w = base_world()
    out, kept, lengths = [], [], []
    for i, L in enumerate(COLUMN_LENGTHS + (480, 480)):
        reads = _base_reads(w, 2, seed=40 + i, read_len=L, ins_mean=150.0, haps=[0])
        for p in range(2):
            big = L == 480 and p == 1
            a = with_variants(reads[2 * p], 13, reverse=True, q1_tenths=7) if big else dict(two_registers(reads[2 * p]), quals=low_quals(L, 7))
            b = with_variants(reads[2 * p + 1], 10 if big else 3, reverse=bool(p), q1_tenths=7)
            out += [a, b]; kept += [len(a["recs"]), len(b["recs"])]; lengths.append(L)
    return dict(name="columns", world=w, batch=assemble(out, 150.0, 35.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=512, lengths=lengths,
                floors=dict(multi=14, mapq_lt1=14, not_first=4, distinct_mapq=3))


@functools.lru_cache(maxsize=None)
def too_long():
    """Two ordinary pairs and one of 520-base reads (two kept records on mate 1) under max_columns = 512: the library flags the records of the long
    reads (HLALA_CHAIN_ERR_COLUMNS) and refuses the pair; not an input the oracle is given."""
    w = base_world()
    out, kept = [], []
    for p, L in enumerate((150, 150, 520)):
        reads = _base_reads(w, 1, seed=50 + p, read_len=L, ins_mean=150.0, haps=[0])
        out += [dict(two_registers(reads[0]), quals=low_quals(L)), with_variants(reads[1], 3)]; kept += [2, 3]
    return dict(name="too long", world=w, batch=assemble(out, 150.0, 35.0), kept=np.asarray(kept), refused=[2], oracle_fails=[2], max_columns=512, floors=dict())


@functools.lru_cache(maxsize=None)
def gaps():
    """Chains with every kind of column in the selected and in the compared chains: level -1 columns (the base every variant inserts), '_' in the read (the level
    every variant deletes) and '_' in graph and read alike (a level the read's haplotype lacks: at least one mate of every pair crosses one, no mate two, in a k = 0 world whose
    haplotypes lose a level about every 150).  Two to seven kept records per mate, every second pair in reverse order.  The one gap column of a read is shared
    by its whole list (gap columns are matched by level alone): one column in 151 with confidence 1, under the cap."""
    w = _world(11, 6000, 0, 3, n_largegap=0)
    reads = _base_reads(w, 12, seed=57, skips=1, candidates=400, haps=[1, 2, 3])
    out, kept = [], []
    for p in range(12):
        n1, n2 = 2 + p % 6, 2 + (p // 2) % 5
        out += [with_variants(reads[2 * p], n1, reverse=bool(p % 2), q1_tenths=7), with_variants(reads[2 * p + 1], n2, q1_tenths=7)]; kept += [n1, n2]
    return dict(name="gaps", world=w, batch=assemble(out, 200.0, 35.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=384,
                floors=dict(multi=12, mapq_lt1=10, not_first=5, distinct_mapq=3, gap_columns=12, inserted_columns=12))


LEVEL_WORLDS = (16, 17, 33, "16+1")


@functools.lru_cache(maxsize=None)
def level_world(kind):
    """Worlds with 16, 17 and 33 sequences per level (pair_insert_ll: the quarter-wave form takes levels of up to 16, the bisecting form the others), the
    haplotypes with single-level gaps so that the four anchoring levels of a pair hold different counts; "16+1": 17 haplotypes of which the last one is absent
    from chosen levels, so that three anchoring levels hold 16 sequences and the fourth 17 (see sequence_levels), and has lost twelve levels between the mates
    of chosen pairs: its distance alone is the mean there."""
    n = 17 if kind == "16+1" else kind
    rng = np.random.default_rng(600 + n)
    H = synth.make_haplotypes(rng, 6000, n_mut=3, n_largegap=0, extra_identical=n - 4)
    plan = []
    if kind == "16+1":
        H[16] = H[0]                                       # the scaffold, absent only where the plan says
        for i in range(8):
            s = 400 + 600 * i; L = 100; d = 112
            e, b = s + L - 1, s + L + d                    # last level of mate 1, first level of mate 2 (haplotype 0: level = position)
            H[:16, e - 1:e + 1] = H[0, e - 1:e + 1]; H[:16, b:b + 2] = H[0, b:b + 2]          # the sixteen others visit all four levels
            H[16, e + 10:e + 34:2] = ord("_")              # twelve single levels lost between the mates (no three in a row: no gap stretch)
            absent = [lv for j, lv in enumerate((e, e - 1, b, b + 1)) if j != i % 4] if i < 4 else ([e, e - 1] if i % 2 else [b + 1])
            for lv in absent:
                H[16, lv] = ord("_")
            plan.append((s, L, d))
    w = dict(H=H, graph=synth.build_graph(H, 1), contigs=synth.make_contigs(H), G=6000)
    return w, plan


@functools.lru_cache(maxsize=None)
def sequence_levels(kind):
    """Pairs read off haplotype 0 with one combination and with 2 x 2, inner distances around the mean (100, sd 10), in level_world(kind).  "16+1": the
    planned pairs, at distance 112 on haplotype 0 and 100 on haplotype 17 alone."""
    w, plan = level_world(kind)
    q = low_quals(100, 7)
    out, kept = [], []
    if not plan:
        plan = [(300 + 230 * i, 100, 85 + 3 * i) for i in range(12)]
    for s, L, d in plan:
        a = _direct_pair(w, 0, s, L, d, q); out += a; kept += [1, 1]
        a = _direct_pair(w, 0, s + 1, L, d, q); out += [two_registers(a[0]), two_registers(a[1])]; kept += [2, 2]
    return dict(name="sequences per level %s" % kind, world=w, batch=assemble(out, 100.0, 10.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=384,
                floors=dict(multi=len(plan), mapq_lt1=len(plan), not_first=2))


def level_counts(w, units):
    """The set of (numbers of sequences on the anchoring levels: last, second last of the upstream chain, first, second of the downstream one) over all combinations."""
    n = np.bincount(np.asarray(w["contigs"]["contig_level"]), minlength=int(w["graph"]["n_levels"]))
    return {tuple(int(n[lv]) for lv in al) for u in units if u for al in u["anchor_levels"] if al}


UNPAIRED = [(1, 1), (2, 2), (63, 63), (64, 64), (70, 2), (128, 63), (130, 64), (65, 1), (3, 3), (65, 65), (130, 66)]          # (records, kept) per read


@functools.lru_cache(maxsize=None)
def unpaired():
    """hlala_batch_create_unpaired: single reads with 1, 2, 63, 64 and 65 (refused) kept alignments, and with more than 64 records of which at most 64 are kept."""
    w = base_world()
    reads = _base_reads(w, len(UNPAIRED), seed=35)[::2]
    out = []
    for r, (nr, nk) in enumerate(UNPAIRED):
        out.append(with_variants(reads[r], nk, reverse=bool(r % 2)) if nr == nk else interleaved(reads[r], nr, nk, seed=r))
    kept = [nk for _, nk in UNPAIRED]
    return dict(name="unpaired", world=w, batch=assemble(out, 200.0, 35.0, per_unit=1), kept=np.asarray(kept), refused=[r for r, k in enumerate(kept) if k > PAIR_CHAINS],
                oracle_fails=[], max_columns=384, unpaired=True, floors=dict(multi=7, mapq_lt1=7, not_first=2, distinct_mapq=3))          # (of the reads the library takes -- two more have 65 and 66 kept records; reads 1 and 3 hold their records in reverse order)


@functools.lru_cache(maxsize=None)
def fan():
    """synth.make_fan_world: 320 haplotypes on nodes of their own between levels 600 and 612.  Mate 1 of pairs 0 and 1 starts two levels behind the fan with
    8 to 13 bases soft-clipped, so that its extension runs back through the fan (a frontier of hundreds of nodes: the DP classes of the side stream, whose
    pairs hlala_align_batch defers to its second pairing pass): 12 x 11 = 132 combinations (general class) and 3 x 3; pairs 2 and 3 lie far from the fan."""
    w = synth.make_fan_world()
    q = low_quals(150, 7)
    out, kept = [], []
    for p, (s, n1, n2) in enumerate([(614, 12, 11), (614, 3, 3), (50, 12, 11), (680, 2, 2)]):
        a = _direct_pair(w, 310 - p, s, 150, 180 + 5 * p, q)
        m1 = dict(a[0], recs=[placed(a[0]["recs"][0], 150, i % 2, 8 + i // 2) for i in range(n1 - 1)] + [far(a[0]["recs"][0], 150)])          # (far: the extension through the fan is the same for every variant in place)
        out += [m1, with_variants(a[1], n2, q1_tenths=7)]; kept += [n1, n2]
    return dict(name="fan", world=w, batch=assemble(out, 200.0, 35.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=384, deferred=[0, 1],
                floors=dict(multi=4, mapq_lt1=4, not_first=2))


def refused_by_capacity(units):
    """The units for which tests/pair_reference.py (with the library's capacities) has no answer."""
    return [u for u, x in enumerate(units) if x is None]


LIMITS = [(64, 16), (16, 64), (64, 1), (1, 64), (64, 2), (43, 3), (33, 31), (63, 2), (1, 1), (2, 3)]


@functools.lru_cache(maxsize=None)
def limits():
    """The family of tests/golden/ref_pair_limits.npz (what the reference's own processBAM makes of it is committed there): 64 kept chains on either mate, 128,
    129, 1023 and 1024 combinations, every second pair in reverse order, on a world of 1600 levels.  No pair that the library refuses."""
    w = _world(11, 1600, 1, 3, n_largegap=0)
    reads = _base_reads(w, len(LIMITS), seed=36, ins_mean=120.0)
    out, kept = [], []
    for p, (n1, n2) in enumerate(LIMITS):
        out += [with_variants(reads[2 * p], n1, reverse=bool(p % 2)), with_variants(reads[2 * p + 1], n2, reverse=bool(p % 2))]; kept += [n1, n2]
    return dict(name="limits", world=w, batch=assemble(out, 120.0, 35.0), kept=np.asarray(kept), refused=[], oracle_fails=[], max_columns=384,
                floors=dict(multi=9, mapq_lt1=9, not_first=5, distinct_mapq=10))
