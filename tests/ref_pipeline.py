"""Shared by the pipeline pin (tests/test_reference_pin_pipeline.py), its fixtures (tests/golden/make_ref_golden_pipeline.py) and the GPU test over them
(tests/test_gpu_reference_pin_pipeline.py): batch surgery (corner CIGARs, hard clips, interval offsets, sub-batches) and the comparison rules.
Needs numpy only."""
import numpy as np

OPS = "MIDNSHP=X"
OP = {c: i for i, c in enumerate(OPS)}
BATCH_CHAIN_KEYS = ("chain_contig", "chain_pos", "chain_offset", "chain_as", "chain_reverse")
PAIR_EXACT = ("best_chain", "n_combinations", "strands_valid", "n_cols")
PAIR_COLS = ("col_level", "col_edge", "col_gchar", "col_schar", "col_fromseed", "col_mapq")
PROJ_INT = ("status", "n_cols", "seq_begin", "seq_end", "removed_cols")
PROJ_COLS = ("col_level", "col_edge", "col_gchar", "col_schar", "col_fromseed")


# ------------------------------------------------------------------ batches as lists of records

def cigar_of(b, c):
    return [(int(x) >> 4, OPS[int(x) & 15]) for x in b["cigar"][b["cigar_off"][c]:b["cigar_off"][c + 1]]]


def with_cigars(b, cigars, **chain_arrays):
    """Copy of batch `b` with the CIGAR of chain c replaced by cigars[c] (a list of (length, op)) and per-chain arrays replaced."""
    n = dict(b)
    enc = [[(l << 4) | OP[o] for l, o in cg if l > 0] for cg in cigars]
    n["cigar_off"] = np.concatenate([[0], np.cumsum([len(x) for x in enc])]).astype(np.int64)
    n["cigar"] = np.asarray([x for cg in enc for x in cg], np.uint32)
    for k, v in chain_arrays.items():
        n[k] = np.asarray(v, np.asarray(b[k]).dtype)
    return n


def subset_units(b, units, per_unit=2):
    """The batch of the given pairs (per_unit = 2) or single reads (per_unit = 1) of `b`, chains renumbered from 0."""
    ro, co = np.asarray(b["read_off"], np.int64), np.asarray(b["chain_off"], np.int64)
    reads = [per_unit * u + m for u in units for m in range(per_unit)]
    chains = [c for r in reads for c in range(co[r], co[r + 1])]
    cmap = {c: i for i, c in enumerate(chains)}
    n = with_cigars(b, [cigar_of(b, c) for c in chains], **{k: np.asarray(b[k])[chains] for k in BATCH_CHAIN_KEYS})
    n["n_pairs"] = len(units); n["n_chains"] = len(chains)
    n["read_off"] = np.concatenate([[0], np.cumsum([ro[r + 1] - ro[r] for r in reads])]).astype(np.int64)
    n["read_bases"] = np.concatenate([np.asarray(b["read_bases"])[ro[r]:ro[r + 1]] for r in reads]).astype(np.uint8)
    n["read_quals"] = np.concatenate([np.asarray(b["read_quals"])[ro[r]:ro[r + 1]] for r in reads]).astype(np.uint8)
    n["chain_off"] = np.concatenate([[0], np.cumsum([co[r + 1] - co[r] for r in reads])]).astype(np.int64)
    n["read_primary"] = np.asarray([cmap[int(b["read_primary"][r])] for r in reads], np.int32)
    n.pop("truth_level0", None)
    return n


def hardclip_nonprimary(b, frac, seed):
    """BWA writes supplementary records with hard clips: the soft clips of a share `frac` of the non-primary records become hard clips (the read of the batch
    is the primary's, complete).  Returns (batch, number of records changed)."""
    rng = np.random.default_rng(seed)
    prim = set(int(x) for x in b["read_primary"])
    cigs, n = [], 0
    for c in range(b["n_chains"]):
        cg = cigar_of(b, c)
        if c not in prim and rng.random() < frac and any(o == "S" for _, o in cg):
            cg = [(l, "H" if o == "S" else o) for l, o in cg]; n += 1
        cigs.append(cg)
    return with_cigars(b, cigs), n


def with_interval_offset(world, b, k):
    """The world and the batch as an interval that starts k bases into its contigs' coordinates: every contig gets k bases in front (its level table, which is read
    at Position - reference2level_offset while the bases are read at Position -- processBAM.cpp:4979, 5295 --, keeps its length by repeating its last entry k
    times), every record's Position and reference2level_offset grow by k.  Returns (world, batch)."""
    C = world["contigs"]; off = np.asarray(C["contig_off"]); n = C["n_contigs"]
    seq = np.concatenate([np.concatenate([np.full(k, ord("N"), np.uint8), C["contig_seq"][off[h]:off[h + 1]]]) for h in range(n)])
    lvl = np.concatenate([np.concatenate([C["contig_level"][off[h]:off[h + 1]], np.full(k, C["contig_level"][off[h + 1] - 1], np.int32)]) for h in range(n)])
    w = dict(world); w["contigs"] = dict(C, contig_off=(off + k * np.arange(n + 1)).astype(np.int64), contig_seq=seq.astype(np.uint8), contig_level=lvl.astype(np.int32))
    nb = dict(b); nb["chain_pos"] = (np.asarray(b["chain_pos"]) + k).astype(np.int32); nb["chain_offset"] = (np.asarray(b["chain_offset"]) + k).astype(np.int32)
    return w, nb


def reversed_chain_order(b):
    """The records of every read in reverse order (their AS values stay sorted in descending order, as the batch layout asks): the best record of a read then
    usually is its last one, so that a selection which only ever returns the first combination shows."""
    co = np.asarray(b["chain_off"], np.int64)
    n_reads = len(co) - 1
    perm = np.concatenate([np.arange(co[r + 1] - 1, co[r] - 1, -1) for r in range(n_reads)])
    inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
    AS = np.asarray(b["chain_as"])
    n = with_cigars(b, [cigar_of(b, int(c)) for c in perm], **{k: np.asarray(b[k])[perm] for k in BATCH_CHAIN_KEYS})
    n["chain_as"] = np.concatenate([np.sort(AS[co[r]:co[r + 1]])[::-1] for r in range(n_reads)]).astype(np.int32)
    n["read_primary"] = inv[np.asarray(b["read_primary"])].astype(np.int32)
    return n


def same_strand_pairs(b, every):
    """Every `every`-th pair with the strand flag of all records of mate 2 flipped: both mates on one strand, alignedReadPair_strandsValid says no and the
    insert-size term is the penalty (the flag only says in which orientation the batch holds the read: nothing else changes)."""
    rev = np.asarray(b["chain_reverse"]).copy(); co = np.asarray(b["chain_off"], np.int64)
    for p in range(0, b["n_pairs"], every):
        rev[co[2 * p + 1]:co[2 * p + 2]] ^= 1
    n = dict(b); n["chain_reverse"] = rev
    return n


# ------------------------------------------------------------------ corner records

# kind -> rewrite of the record [aS, mM, cS] of mate 1 of a pair; (cigar, position shift)
def _split(m):
    return m // 3


CORNER_KINDS = {
    "eqx":        lambda a, m, c: ([(a, "S"), (_split(m), "="), (1, "X"), (m - _split(m) - 1, "="), (c, "S")], 0),
    "pad":        lambda a, m, c: ([(a, "S"), (_split(m), "M"), (2, "P"), (m - _split(m), "M"), (c, "S")], 0),
    "pad_empty":  lambda a, m, c: ([(a, "S"), (_split(m), "M"), (0, "P"), (m - _split(m), "M"), (c, "S")], 0),
    "skip_N":     lambda a, m, c: ([(a, "S"), (_split(m), "M"), (5, "N"), (m - _split(m), "M"), (c, "S")], 0),
    "H_lead":     lambda a, m, c: ([(a, "H"), (m, "M"), (c, "S")], 0),
    "H_trail":    lambda a, m, c: ([(a, "S"), (m, "M"), (c, "H")], 0),
    "H_both":     lambda a, m, c: ([(a, "H"), (m, "M"), (c, "H")], 0),
    "S_lead":     lambda a, m, c: ([(a, "S"), (m, "M"), (c, "S")], 0),
    "I_lead":     lambda a, m, c: ([(a, "S"), (2, "I"), (m - 2, "M"), (c, "S")], 2),
    "I_lead_noS": lambda a, m, c: ([(a + 3, "I"), (m - 3, "M"), (c, "S")], a + 3),
    "I_after_D":  lambda a, m, c: ([(a, "S"), (_split(m), "M"), (2, "D"), (3, "I"), (m - _split(m) - 3, "M"), (c, "S")], 0),
    "D_after_I":  lambda a, m, c: ([(a, "S"), (_split(m), "M"), (3, "I"), (2, "D"), (m - _split(m) - 3, "M"), (c, "S")], 0),
    "multi_I":    lambda a, m, c: ([(a, "S"), (_split(m), "M"), (4, "I"), (m - _split(m) - 4, "M"), (c, "S")], 0),
    "I_trail":    lambda a, m, c: ([(a, "S"), (m - 2, "M"), (2, "I"), (c, "S")], 0),
    "all_I":      lambda a, m, c: ([(a, "S"), (m, "I"), (c, "S")], 0),
}
GAP_KINDS = ("gap_from_left", "gap_from_right", "gap_inside", "I_at_level_skip")


def corner_batch(world, base, kinds, gap_stretch, seed=1):
    """Batch `base` (one record per read, CIGAR [aS, mM, cS], no indels) with mate 1 of pair p rewritten into kind kinds[p % len(kinds)]; mate 2 stays.
    The GAP_KINDS place mate 1 anew: a perfect read from a contig that has bases inside a gap stretch (`gap_stretch`: inGraphGapStretch), running into the stretch
    from the left, from the right, or lying wholly inside it; I_at_level_skip puts an insertion of n bases where the contig skips n graph levels, the case
    cleanInitialAlignment exists for (inserted bases next to as many skipped levels).  Returns (batch, kind of every pair)."""
    rng = np.random.default_rng(seed)
    C = world["contigs"]; off = np.asarray(C["contig_off"]); lvl = np.asarray(C["contig_level"]); seq = np.asarray(C["contig_seq"])
    d = np.diff(np.concatenate([[0], np.asarray(gap_stretch, np.int8), [0]]))
    stretches = [(int(s), int(e)) for s, e in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0])]          # [s, e)
    b = dict(base)
    bases = np.asarray(b["read_bases"]).copy(); pos = np.asarray(b["chain_pos"]).copy(); contig = np.asarray(b["chain_contig"]).copy()
    ro = np.asarray(b["read_off"], np.int64)
    cigs = [cigar_of(b, c) for c in range(b["n_chains"])]
    kind_of = []
    for p in range(b["n_pairs"]):
        kind = kinds[p % len(kinds)]
        r = 2 * p; c = int(b["chain_off"][r])
        assert b["chain_off"][r + 1] == c + 1, "corner_batch needs one record per read"
        L = int(ro[r + 1] - ro[r])
        cg = cigs[c]
        a = sum(l for l, o in cg[:1] if o == "S"); cc = sum(l for l, o in cg[-1:] if o == "S")
        assert [o for _, o in cg if o != "S"] == ["M"], "corner_batch needs [aS, mM, cS] records"
        if kind == "I_at_level_skip":
            placed = False
            for h in rng.permutation(C["n_contigs"]):
                h = int(h); l = lvl[off[h]:off[h + 1]]
                skip = np.diff(l) - 1
                cand = np.nonzero((skip >= 1) & (skip <= 6))[0]
                cand = cand[(cand > 80) & (cand < len(l) - L)]
                if len(cand) == 0:
                    continue
                q = int(cand[rng.integers(0, len(cand))]); n_ins = int(skip[q]); m1 = 50; rest = L - 20 - m1 - n_ins
                bases[ro[r]:ro[r + 1]] = np.concatenate([seq[off[h] + q - m1 - 9: off[h] + q + 1], np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_ins)],
                                                         seq[off[h] + q + 1: off[h] + q + 1 + rest + 10]])
                pos[c] = q - m1 + 1; contig[c] = h; cigs[c] = [(10, "S"), (m1, "M"), (n_ins, "I"), (rest, "M"), (10, "S")]
                placed = True
                break
            assert placed, "no contig that skips 1 to 6 levels"
        elif kind in GAP_KINDS:
            placed = False
            for t in rng.permutation(len(stretches)):
                s, e = stretches[int(t)]
                for h in rng.permutation(C["n_contigs"]):
                    h = int(h); l = lvl[off[h]:off[h + 1]]
                    inside = np.nonzero((l >= s) & (l < e))[0]
                    if kind == "gap_inside":
                        if len(inside) < 16:
                            continue
                        m = min(len(inside) - 4, L - 20); a2 = (L - m) // 2; p0 = int(inside[2])
                    else:
                        if len(inside) < 3:
                            continue
                        m = L - 20; a2 = 10
                        p0 = int(inside[0]) - (m - min(40, len(inside))) if kind == "gap_from_left" else int(inside[-1]) - min(40, len(inside)) + 1
                    if p0 - a2 < 0 or p0 + m + (L - a2 - m) >= len(l):
                        continue
                    bases[ro[r]:ro[r + 1]] = seq[off[h] + p0 - a2: off[h] + p0 - a2 + L]
                    pos[c] = p0; contig[c] = h; cigs[c] = [(a2, "S"), (m, "M"), (L - a2 - m, "S")]
                    placed = True
                    break
                if placed:
                    break
            assert placed, "no contig with bases in a gap stretch for " + kind
        else:
            a = max(a, 4); cc = max(cc, 4)
            cg2, shift = CORNER_KINDS[kind](a, L - a - cc, cc)
            pos[c] = pos[c] + (a - sum(l for l, o in cg[:1] if o == "S")) + shift
            cigs[c] = cg2
        kind_of.append(kind)
    n = with_cigars(b, cigs, chain_pos=pos, chain_contig=contig)
    n["read_bases"] = bases
    return n, kind_of


def gap_stretch_rule(graph, min_len=3):
    """inGraphGapStretch by the rule of processBAM.cpp:91-149, stated on arrays: level l (of the n_levels - 1 levels that have outgoing edges) is in a
    stretch when it belongs to a run of at least `min_len` consecutive levels that each have an outgoing '_' edge."""
    L = int(graph["n_levels"])
    has = np.zeros(L - 1, bool)
    lv = np.asarray(graph["node_level"])[np.asarray(graph["edge_from"])[np.asarray(graph["edge_label"]) == ord("_")]]
    has[lv] = True
    d = np.diff(np.concatenate([[0], has.astype(np.int8), [0]]))
    out = np.zeros(L - 1, np.uint8)
    for a, b in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]):          # run [a, b)
        if b - a >= min_len:
            out[a:b] = 1
    return out


def finished_chains(b, ext, n_reads):
    """The oracle's finished long-read chains (status 0) in the hlala_seeds_in layout, grouped by read."""
    st = ext["_stride"]
    co = np.asarray(b["chain_off"])
    chain_read = np.repeat(np.arange(n_reads), np.diff(co[:n_reads + 1]))
    keep = np.nonzero(ext["status"][:b["n_chains"]] == 0)[0]
    cols = lambda k: np.concatenate([ext[k][c * st:c * st + int(ext["n_cols"][c])] for c in keep])
    return dict(n_reads=n_reads, read_off=np.asarray(b["read_off"], np.int32), read_bases=b["read_bases"], read_quals=b["read_quals"], n_chains=len(keep),
                chain_read=chain_read[keep].astype(np.int32), chain_seq_begin=ext["seq_begin"][keep], chain_seq_end=ext["seq_end"][keep],
                chain_reverse=np.asarray(b["chain_reverse"])[keep], col_off=np.concatenate([[0], np.cumsum(ext["n_cols"][keep])]).astype(np.int32),
                col_level=cols("col_level"), col_edge=cols("col_edge"), col_gchar=cols("col_gchar"), col_schar=cols("col_schar"), _keep=keep.astype(np.int32))


# ------------------------------------------------------------------ comparisons (every unit, none left out)

def projection_diffs(got, exp, rows, got_rows=None):
    """Per chain of `rows`, the names of the stage-A outputs in which `got` (row got_rows[i]) differs from `exp` (row rows[i])."""
    sg, se = got["_stride"], exp["_stride"]
    got_rows = rows if got_rows is None else got_rows
    bad = {}
    for cg, ce in zip(got_rows, rows):
        cg, ce = int(cg), int(ce)
        b = [k for k in PROJ_INT if got[k][cg] != exp[k][ce]]
        if exp["status"][ce] == 0:
            n = int(exp["n_cols"][ce])
            b += [k for k in PROJ_COLS if not np.array_equal(got[k][cg * sg:cg * sg + n], exp[k][ce * se:ce * se + n])]
        if b:
            bad[ce] = b
    return bad


def pair_diffs(got, exp, n_units, per_unit=2, cols=PAIR_COLS):
    """Per unit, the names of the exact outputs in which `got` differs from `exp`; the doubles within the bars of tests/test_gpu_align.py (pair_ll rtol 1e-12;
    pair_mapq / mate_mapq rtol 1e-9, atol 1e-15).  Returns (bad, number of doubles that differ at all)."""
    sg, se = got["_stride"], exp["_stride"]
    bad = {}
    differ = 0
    for u in range(n_units):
        b = []
        rows = range(per_unit * u, per_unit * u + per_unit)
        for k in PAIR_EXACT:
            idx = [u] if k in ("n_combinations", "strands_valid") else list(rows)
            if any(got[k][i] != exp[k][i] for i in idx):
                b.append(k)
        for r in rows:
            n = int(exp["n_cols"][r])
            b += [k for k in cols if not np.array_equal(got[k][r * sg:r * sg + n], exp[k][r * se:r * se + n])]
        if not np.isclose(got["pair_ll"][u], exp["pair_ll"][u], rtol=1e-12, atol=0):
            b.append("pair_ll")
        if not np.isclose(got["pair_mapq"][u], exp["pair_mapq"][u], rtol=1e-9, atol=1e-15):
            b.append("pair_mapq")
        if not np.allclose(got["mate_mapq"][list(rows)], exp["mate_mapq"][list(rows)], rtol=1e-9, atol=1e-15):
            b.append("mate_mapq")
        differ += int(got["pair_ll"][u] != exp["pair_ll"][u]) + int(got["pair_mapq"][u] != exp["pair_mapq"][u]) + int(np.sum(got["mate_mapq"][list(rows)] != exp["mate_mapq"][list(rows)]))
        if b:
            bad[u] = sorted(set(b))
    return bad, differ


def pack_rows(d, n_rows, keys):
    """Strided column arrays `keys` of `d` packed row after row (n_cols gives the offsets): the layout of the fixtures."""
    st = d["_stride"]
    mask = (np.arange(st)[None, :] < d["n_cols"][:n_rows, None]).reshape(-1)
    return {k: d[k][:n_rows * st][mask] for k in keys}


def unpack_rows(packed, n_cols, stride, keys):
    """Inverse of pack_rows."""
    n = len(n_cols)
    mask = (np.arange(stride)[None, :] < np.asarray(n_cols)[:, None]).reshape(-1)
    out = {"_stride": stride, "n_cols": np.asarray(n_cols)}
    for k in keys:
        a = np.zeros(n * stride, packed[k].dtype); a[mask] = packed[k]; out[k] = a
    return out
