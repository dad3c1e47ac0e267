"""Inputs of the exon-position edge tests (csrc/kernel_exonpos.hip: k_exon_positions<0/1>, k_unit_stats), a census of what they contain, and the helpers the
exon-position tests share (locus, fake_pairs).  tests/test_exonpos_reference.py holds the oracle against tests/exonpos_reference.py on them,
tests/test_gpu_exonpos_edges.py the kernels.  Plain numpy: neither the oracle nor the library is used here; every family is built once per process.

A family is a dict: name, world, batch, max_columns, unpaired, long_read_mode, floors (census key -> least count, asserted on the oracle's alignments and
on the library's own; each at most half of what the oracle's alignments held when the family was written) and, where the locus descriptions do not depend
on the alignment, loci.  Families whose loci are read off the alignment (loci, thresholds) have a function for that, which both sides call with their own pairs.

The batches: synth.make_batch with inner distance -100 +- 20 between reads of 150 bases (the mates share about a hundred levels), one pure-M record per
read, no clips.  Every second pair has one and the same quality on every base of both mates, so that its shared levels are exact worst-quality ties."""
import functools

import numpy as np

import exonpos_reference as er
import pair_edge_cases as pe
from tools import synth

G = 5000
GAP = er.GAP
CONST_Q = 33 + 30


# ------------------------------------------------------------------------------------------------ shared helpers
def locus(G, a, exons):
    """level_min = a; `exons` = list of (start offset, length) inside the locus; exon positions run through consecutively."""
    width = max(s + n for s, n in exons)
    l2e = np.full(width, -1, np.int32); k = 0
    for s, n in exons:
        l2e[s:s + n] = np.arange(k, k + n); k += n
    assert a + width < G
    return a, l2e


def fake_pairs(mates, stride=24, per_unit=2):
    """mates = list of (levels, gchars, schars, mapq chars) per mate; reads are the non-gap sequence characters with quality chars given per base."""
    n = len(mates) // per_unit
    pr = dict(pair_status=np.zeros(n, np.int32), n_cols=np.zeros(2 * n, np.int32), col_level=np.zeros(2 * n * stride, np.int32),
              col_gchar=np.zeros(2 * n * stride, np.uint8), col_schar=np.zeros(2 * n * stride, np.uint8), col_mapq=np.zeros(2 * n * stride, np.uint8),
              mate_mapq=np.ones(2 * n), strands_valid=np.ones(n, np.uint8))
    off = [0]; bases = []; quals = []
    for r, (lv, g, s, mq, q) in enumerate(mates):
        m = len(lv); pr["n_cols"][r] = m
        pr["col_level"][r * stride: r * stride + m] = lv
        pr["col_gchar"][r * stride: r * stride + m] = np.frombuffer(g.encode(), np.uint8)
        pr["col_schar"][r * stride: r * stride + m] = np.frombuffer(s.encode(), np.uint8)
        pr["col_mapq"][r * stride: r * stride + m] = np.frombuffer(mq.encode(), np.uint8)
        rb = s.replace("_", ""); assert len(q) == len(rb)
        bases.append(np.frombuffer(rb.encode(), np.uint8)); quals.append(np.frombuffer(q.encode(), np.uint8)); off.append(off[-1] + len(rb))
    batch = dict(n_pairs=n, read_off=np.array(off, np.int32), read_bases=np.concatenate(bases), read_quals=np.concatenate(quals))
    return pr, batch, stride


def whole(insert_mean, insert_sd, **kw):
    """The locus that is the whole graph, every level an exon position."""
    return er.make_locus(0, np.arange(G, dtype=np.int32), insert_mean, insert_sd, **kw)


# ------------------------------------------------------------------------------------------------ the census
CENSUS_KEYS = ("pairs_shared", "shared_levels", "shared_equal", "shared_m1_better", "shared_m2_better", "shared_gap_m1", "shared_gap_m2", "shared_gap_both",
               "pos_from_mate2", "strip_single", "strip_multi", "starts_with_insertion", "ends_with_insertion", "nins_ge2", "novel_gap_ge2", "strip_loses",
               "strip_wins", "use_differs", "ok_without_position")


def census(pairs, batch, stride, L, unpaired=False, model=None):
    """What the selected alignments in `pairs` hold for locus L, counted over the units that pass the locus's test, on exon levels only:
    pairs_shared / shared_levels: pairs whose mates share a level, and such levels; shared_equal / _m1_better / _m2_better: by the worst qualities of the two
    alternatives; shared_gap_m1 / _m2 / _both: shared levels where that mate's alternative is the lone '_'; pos_from_mate2: positions kept from mate 2;
    strip_single / strip_multi: positions whose leading '_' was dropped for one / several inserted bases; starts_ / ends_with_insertion: used alignments whose
    first / last column has no level; nins_ge2: positions with two or more inserted bases; novel_gap_ge2; strip_loses / strip_wins: shared levels where a
    stripped alternative is dropped / kept; use_differs: accepted pairs of which one mate alone overlaps the locus; ok_without_position: units that pass
    the test and yield no read.  (The column walk is tests/exonpos_reference.py's: the model is held against the oracle field by field on the same inputs;
    `model`: a Model over the same pairs, to walk them once for many loci.)"""
    M = model or er.Model(pairs, batch, stride, np.zeros(256), unpaired)
    c = dict.fromkeys(CENSUS_KEYS, 0)
    acc, _, _ = M.accepted(L)
    for u, used, lists in acc:
        rows = [u] if unpaired else [2 * u, 2 * u + 1]
        for i, r in enumerate(rows):
            if used[i]:
                c["starts_with_insertion"] += M.mate(r)["starts_with_insertion"]; c["ends_with_insertion"] += M.mate(r)["ends_with_insertion"]
        c["use_differs"] += int(len(used) == 2 and used[0] != used[1])
        c["ok_without_position"] += int(not any(lists))
        kept = lists[0] if unpaired else er.remove_double(lists[0] + lists[1])
        for p in kept:
            c["pos_from_mate2"] += p["mate"] == 2; c["nins_ge2"] += p["n_ins"] >= 2; c["novel_gap_ge2"] += p["novel_gap"] >= 2
            c["strip_single"] += p["strip"] and p["n_ins"] == 1; c["strip_multi"] += p["strip"] and p["n_ins"] > 1
        if unpaired:
            continue
        by1 = {p["level"]: p for p in lists[0]}
        shared = [(by1[p["level"]], p) for p in lists[1] if p["level"] in by1]
        c["pairs_shared"] += bool(shared); c["shared_levels"] += len(shared)
        for a, b in shared:
            qa, qb = er.worst_quality(a), er.worst_quality(b)
            ga, gb = a["genotype"] == [GAP], b["genotype"] == [GAP]
            if ga and gb:
                c["shared_gap_both"] += 1
            elif ga:
                c["shared_gap_m1"] += 1
            elif gb:
                c["shared_gap_m2"] += 1
            elif qa == qb:
                c["shared_equal"] += 1
            elif qa > qb:
                c["shared_m1_better"] += 1
            else:
                c["shared_m2_better"] += 1
            for mine, other, wins in ((a, b, qa >= qb), (b, a, qb > qa)):
                if mine["strip"]:
                    c["strip_wins" if wins else "strip_loses"] += 1
    return {k: int(v) for k, v in c.items()}


def check_floors(c, floors, label):
    print("%s: %s" % (label, {k: v for k, v in c.items() if v}))
    for k, v in floors.items():
        assert v > 0 and c[k] >= v, (label, k, c[k], v)


# ------------------------------------------------------------------------------------------------ batches
@functools.lru_cache(maxsize=None)
def world():
    return synth.make_world(seed=1, G=G, k=1)


@functools.lru_cache(maxsize=None)
def _reads(n_pairs, seed=11):
    """The reads of the overlapping batch; every second pair with one quality on all its bases."""
    b = synth.make_batch(world(), n_pairs, seed=seed, ins_mean=-100, ins_sd=20, p_secondary=0, indel_read_frac=0, clip_max=0)
    reads = pe.explode(b)
    for p in range(0, n_pairs, 2):
        for rd in reads[2 * p:2 * p + 2]:
            rd["quals"][:] = CONST_Q
    for rd in reads:
        assert len(rd["recs"]) == 1 and rd["recs"][0]["cig"] == [(150, "M")]
    return reads


def _family(name, batch, floors, **kw):
    return dict(dict(name=name, world=world(), batch=batch, max_columns=384, unpaired=False, long_read_mode=0, floors=floors), **kw)


def _upstream(reads, p):
    return 0 if reads[2 * p]["recs"][0]["pos"] <= reads[2 * p + 1]["recs"][0]["pos"] else 1


OVERLAP_LOCI = [("whole", whole(-100.0, 20.0)),
                ("three exons, a third masked", er.make_locus(*locus(G, 1200, [(0, 270), (400, 276), (900, 120)]), -100.0, 20.0, min_weighted_ok=0.9,
                                                              pair_mask=(np.arange(130) % 3 != 0).astype(np.uint8)))]


@functools.lru_cache(maxsize=None)
def overlap():
    """130 pairs whose mates share about a hundred levels: the whole of removeDoublePositionsFromRead.  Every fourth pair lacks two bases of the shared
    levels in its upstream mate, every fourth in its downstream mate (a lone '_' against a base); levels that the haplotype lacks are '_' in both."""
    reads = list(_reads(130))
    for p in range(130):
        if p % 2:
            r = 2 * p + (_upstream(reads, p) if p % 4 == 1 else 1 - _upstream(reads, p))
            reads[r] = _deleted(reads[r], 100 if p % 4 == 1 else 40, 2)
    return _family("overlap", pe.assemble(reads, -100.0, 20.0), loci=OVERLAP_LOCI,
                   floors=dict(pairs_shared=60, shared_equal=3000, shared_m1_better=1200, shared_m2_better=1200, shared_gap_m1=30, shared_gap_m2=25, shared_gap_both=50,
                               pos_from_mate2=4500))


def _recigar(rd, cig):
    assert sum(l for l, o in cig if o in "MIS") == len(rd["bases"])
    return dict(rd, recs=[dict(rd["recs"][0], cig=cig)])


def _deleted(rd, at, n):
    """The read without the n bases from offset `at` on (its last n bases stand in for the ones that would follow), its record with nD there."""
    L = len(rd["bases"])
    sel = np.concatenate([np.arange(at), np.arange(at + n, L), np.arange(L - n, L)])
    return dict(_recigar(rd, [(at, "M"), (n, "D"), (L - at, "M")]), bases=rd["bases"][sel], quals=rd["quals"][sel])


# variant of pair p = p % 8: (CIGAR of the upstream mate, of the downstream mate); None = left as it is.  The mates share reference offsets 50 .. 149 of the
# upstream and 0 .. 99 of the downstream mate (inner distance -100), so an indel at offset 100 upstream / 40 downstream lies in the overlap.
D1I1 = [(40, "M"), (1, "D"), (1, "I"), (109, "M")]          # a deletion then one inserted base: "_" + base, the '_' dropped
D2I3 = [(40, "M"), (2, "D"), (3, "I"), (107, "M")]          # a deletion of two then three inserted bases
LEAD = [(2, "I"), (148, "M")]                               # a leading insertion
TRAIL = [(148, "M"), (2, "I")]                              # a trailing insertion
I3 = [(60, "M"), (3, "I"), (87, "M")]                       # three inserted bases after a matched base
D3 = [(60, "M"), (3, "D"), (90, "M")]                       # a deletion run of three
D1I1_UP = [(100, "M"), (1, "D"), (1, "I"), (49, "M")]       # the strip position of the upstream mate inside the overlap
D2I3_UP = [(110, "M"), (2, "D"), (3, "I"), (37, "M")]
VARIANTS = [(D1I1, D1I1), (D2I3, D2I3), (LEAD, LEAD), (TRAIL, TRAIL), (I3, D3), (D3, I3), (D1I1_UP, D1I1), (D2I3_UP, LEAD)]


@functools.lru_cache(maxsize=None)
def _column_reads(n_pairs=130):
    reads = list(_reads(n_pairs)); out = []
    for p in range(n_pairs):
        up = _upstream(reads, p); v = VARIANTS[p % len(VARIANTS)]
        for m in range(2):
            cig = v[0] if m == up else v[1]
            rd = reads[2 * p + m]
            out.append(rd if cig is None else _recigar(rd, cig))
    return out


COLUMN_FLOORS = dict(strip_single=15, strip_multi=6, starts_with_insertion=4, ends_with_insertion=8, nins_ge2=25, novel_gap_ge2=80, strip_loses=15, strip_wins=12)


@functools.lru_cache(maxsize=None)
def columns():
    """The overlapping pairs with their CIGARs rewritten: every kind of column run, also inside the overlap of the two mates."""
    return _family("columns", pe.assemble(_column_reads(), -100.0, 20.0), loci=[("whole", whole(-100.0, 20.0)), OVERLAP_LOCI[1]], floors=dict(COLUMN_FLOORS))


FAR = (4500, 4700)          # no read of the `loci` family comes near these levels


@functools.lru_cache(maxsize=None)
def loci():
    """The pairs of `columns` that end before level 4300: one alignment, many locus descriptions (loci_of)."""
    w = world(); C = w["contigs"]; off = np.asarray(C["contig_off"]); lvl = np.asarray(C["contig_level"])
    reads = _column_reads(); keep = []
    for p in range(len(reads) // 2):
        ends = [int(lvl[min(off[x["contig"]] + x["pos"] + 160, off[x["contig"] + 1] - 1)]) for rd in reads[2 * p:2 * p + 2] for x in rd["recs"]]
        if max(ends) < 4300:
            keep += [2 * p, 2 * p + 1]
    return _family("loci", pe.assemble([reads[r] for r in keep], -100.0, 20.0), floors=dict(use_differs=15, ok_without_position=500, strip_single=10, pairs_shared=40))          # (summed over the loci of loci_of)


def _first_last(pairs, stride, r):
    lv = pairs["col_level"][r * stride:r * stride + int(pairs["n_cols"][r])]
    return er.first_level(lv), er.last_level(lv)


def chosen_pair(pairs, stride, n_pairs):
    """The first pair with status 0 whose mates overlap by at least 60 levels, one of them holding a level with inserted bases inside the overlap,
    well inside the graph: (pair, (first, last) of the upstream mate, of the downstream mate, that level)."""
    for p in range(n_pairs):
        if pairs["pair_status"][p] != 0:
            continue
        a, b = _first_last(pairs, stride, 2 * p), _first_last(pairs, stride, 2 * p + 1)
        U, D = (a, b) if a[0] <= b[0] else (b, a)
        if not (U[0] >= 200 and D[1] < 4200 and U[0] + 30 < D[0] and D[0] + 60 <= U[1] and U[1] + 30 < D[1]):
            continue
        for r in (2 * p, 2 * p + 1):
            lv = pairs["col_level"][r * stride:r * stride + int(pairs["n_cols"][r])]
            for c in range(1, len(lv)):
                if lv[c] == -1 and lv[c - 1] != -1 and D[0] + 5 < lv[c - 1] < U[1] - 5:
                    return p, U, D, int(lv[c - 1])
    raise AssertionError("no pair with overlapping mates and an insertion inside the overlap")


def loci_of(pairs, stride, n_pairs, insert_mean=-100.0, insert_sd=20.0):
    """The locus descriptions of the `loci` family, read off the alignment: (the chosen pair, the number -- 0 or 1 -- of its upstream mate, [(name, locus,
    expectation)]), expectation = dict of use (whether the upstream, the downstream mate of the chosen pair overlaps the locus) / present (whether the
    chosen pair yields a read) / n_reads."""
    p, U, D, ins = chosen_pair(pairs, stride, n_pairs)
    up = 0 if _first_last(pairs, stride, 2 * p) == U else 1
    mk = lambda a, z, l2e=None, **kw: er.make_locus(a, np.arange(z - a + 1) if l2e is None else l2e, insert_mean, insert_sd, **kw)
    out = [("one level", mk(D[0] + 5, D[0] + 5), dict(use=(True, True), present=True)),
           ("ends on the downstream mate's first level", mk(D[0] - 20, D[0]), dict(use=(True, True), present=True)),             # x1 in [y1, y2] and y2 in [x1, x2]
           ("ends one level before it", mk(D[0] - 20, D[0] - 1), dict(use=(True, False), present=True)),
           ("starts on the upstream mate's last level", mk(U[1], U[1] + 20), dict(use=(True, True), present=True)),              # x2 in [y1, y2] and y1 in [x1, x2]
           ("starts one level after it", mk(U[1] + 1, U[1] + 20), dict(use=(False, True), present=True)),
           ("strictly inside both mates", mk(D[0] + 10, D[0] + 20), dict(use=(True, True), present=True)),                      # y1, y2 in [x1, x2] only
           ("both mates strictly inside", mk(U[0] - 50, D[1] + 50), dict(use=(True, True), present=True)),                      # x1, x2 in [y1, y2] only
           ("ends on the upstream mate's first level", mk(U[0] - 20, U[0]), dict(use=(True, False), present=True)),
           ("starts on the downstream mate's last level", mk(D[1], D[1] + 20), dict(use=(False, True), present=True))]
    a = U[0] - 50; width = D[1] + 50 - a + 1
    ex = [(0, U[0] + 20 - a), (U[0] + 21 - a, 30), (U[0] + 101 - a, width - (U[0] + 101 - a))]          # holes of width 1 and of width 50
    out.append(("holes of width 1 and 50", mk(a, None, locus(G, a, ex)[1]), dict(use=(True, True), present=True)))
    ex = [(0, ins - a + 1), (ins - a + 6, width - (ins - a + 6))]                                        # a hole right after the level with inserted bases
    out.append(("a hole after a level with inserted bases", mk(a, None, locus(G, a, ex)[1]), dict(use=(True, True), present=True)))
    l2e = np.full(width, -1, np.int32); l2e[:40] = np.arange(40); l2e[-40:] = np.arange(40, 80)          # exon levels only outside the pair
    out.append(("overlapped, no exon level", mk(a, None, l2e), dict(use=(True, True), present=False)))
    out.append(("far from every read", mk(FAR[0], FAR[1]), dict(use=(False, False), present=False, n_reads=0)))
    return p, up, out


@functools.lru_cache(maxsize=None)
def thresholds():
    """Overlapping pairs with secondary records (mapping qualities below 1 and different between the mates); the last pair's second mate is put on the other
    strand (strands_valid = 0)."""
    b = synth.make_batch(world(), 130, seed=12, ins_mean=-100, ins_sd=20, indel_read_frac=0, clip_max=0)
    reads = pe.explode(b)
    reads[-1] = dict(reads[-1], recs=[pe.wrong_strand(x) for x in reads[-1]["recs"]])
    return _family("thresholds", pe.assemble(reads, -100.0, 20.0), floors=dict(pairs_shared=50, shared_m1_better=1000, shared_m2_better=1000))


def threshold_cases(M):
    """From the model M of the aligned `thresholds` batch: [(name, locus, pair, kept)] -- the pair's outcome under the locus.  Thresholds are met with
    equality (kept) and missed by the least amount (broken): everything here is exact in binary64."""
    P = M.pairs; n = M.n
    ok = [p for p in range(n) if P["pair_status"][p] == 0 and P["strands_valid"][p]]
    out = []
    p = ok[0]; d = er.distance(M.mate(2 * p)["lv"], M.mate(2 * p + 1)["lv"])
    for mean, kept in ((d - 40, True), (d + 40, True), (d - 41, False), (d + 41, False)):
        out.append(("insert mean %+d, sd 8" % (mean - d), whole(float(mean), 8.0), p, kept))
    q = [p for p in ok if 0 < P["mate_mapq"][2 * p] < 1]
    assert q, "no pair with a mapping quality below 1"
    p = q[0]; v = float(P["mate_mapq"][2 * p])
    out.append(("min_mapq met", whole(-100.0, 1000.0, min_mapq=v), p, True))
    out.append(("min_mapq missed", whole(-100.0, 1000.0, min_mapq=float(np.nextafter(v, 2.0))), p, False))
    q = [p for p in ok if P["mate_mapq"][2 * p + 1] < P["mate_mapq"][2 * p]]
    assert q, "no pair whose second mate has the lower mapping quality"
    p = q[0]
    out.append(("min_mapq between the mates' (mate 1 alone is tested)", whole(-100.0, 1000.0, min_mapq=float(P["mate_mapq"][2 * p])), p, True))
    p = ok[1]; v = min(M.mate(2 * p)["w"], M.mate(2 * p + 1)["w"])
    out.append(("min_weighted_ok met", whole(-100.0, 1000.0, min_weighted_ok=v), p, True))
    out.append(("min_weighted_ok missed", whole(-100.0, 1000.0, min_weighted_ok=float(np.nextafter(v, 2.0))), p, False))
    assert P["pair_status"][n - 1] == 0 and not P["strands_valid"][n - 1], "the pair on one strand"
    out.append(("strands not valid", whole(-100.0, 1000.0), n - 1, False))
    return out


SIZES = (1, 2, 127, 128, 129, 257)


@functools.lru_cache(maxsize=None)
def sizes(n):
    """The first n of 257 overlapping pairs: batch sizes around the block of 128 threads and the scan over n_pairs + 1 elements."""
    return _family("sizes %d" % n, pe.assemble(list(_reads(257, seed=13)[:2 * n]), -100.0, 20.0), floors=dict(pairs_shared=max(1, n // 2)))


def size_masks(n):
    """[(name, mask or None)]: none, all ones, all zero, the last pair alone, pair 127 / 128 alone where there is one."""
    one = lambda p: (np.arange(n) == p).astype(np.uint8)
    return [("no mask", None), ("all ones", np.ones(n, np.uint8)), ("all zero", np.zeros(n, np.uint8)), ("the last pair", one(n - 1))] + \
           [("pair %d" % p, one(p)) for p in (127, 128) if p < n]


@functools.lru_cache(maxsize=None)
def refused():
    """pair_edge_cases.too_long(): two ordinary pairs and one whose reads exceed max_columns (pair_status -1; not an input the oracle is given)."""
    f = pe.too_long()
    Gw = int(f["world"]["graph"]["n_levels"]) - 1
    return dict(f, name="refused", unpaired=False, long_read_mode=0, floors={}, loci=[("whole", er.make_locus(0, np.arange(Gw), 150.0, 35.0))])


@functools.lru_cache(maxsize=None)
def unpaired_columns():
    """The reads of `columns` as single reads."""
    return _family("unpaired columns", synth.as_unpaired(columns()["batch"]), unpaired=True, long_read_mode=1, floors=dict(strip_single=20, strip_multi=15, starts_with_insertion=60),
                   loci=[("whole, 100 columns", whole(0.0, 0.0, min_alignment_columns=100)), ("whole, 1000 columns", whole(0.0, 0.0)),
                         ("three exons, a third masked", er.make_locus(*locus(G, 1200, [(0, 270), (400, 276), (900, 120)]), 0.0, 0.0, min_alignment_columns=100,
                                                                       pair_mask=(np.arange(260) % 3 != 0).astype(np.uint8)))])


@functools.lru_cache(maxsize=None)
def unpaired_long():
    """Eight reads of 2 000 to 3 000 bases with error-rich CIGARs (max_columns = 4096)."""
    b = synth.make_long_batch(world(), 8, seed=21, len_lo=2000, len_hi=3000)
    return _family("unpaired long", b, unpaired=True, long_read_mode=1, max_columns=4096, floors=dict(starts_with_insertion=4, nins_ge2=150, novel_gap_ge2=50),
                   loci=[("whole", whole(0.0, 0.0)), ("three exons", er.make_locus(*locus(G, 1200, [(0, 270), (400, 276), (900, 120)]), 0.0, 0.0))])


def column_count_cases(M):
    """min_alignment_columns met with equality and missed by one, for the first aligned read of an unpaired model: [(name, locus, read, kept)]."""
    r = [u for u in range(M.n) if M.pairs["pair_status"][u] == 0][0]; n = M.mate(r)["n"]
    return [("min_alignment_columns met", whole(0.0, 0.0, min_alignment_columns=n), r, True), ("min_alignment_columns missed", whole(0.0, 0.0, min_alignment_columns=n + 1), r, False)]


FIXED = dict(overlap=overlap, columns=columns, refused=refused, unpaired_columns=unpaired_columns, unpaired_long=unpaired_long)
