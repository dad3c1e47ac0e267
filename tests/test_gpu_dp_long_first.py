"""Long DP calls first (batch.h: dpl_list, retry_entry): the order in which the persistent DP kernels draw their calls never shows in a result.

A call is LONG when the read bases it can consume (start_seq of a left extension, seqLen - start_seq of a right one) reach the context's threshold
(HLALA_DP_LONG_BASES, read once by hlala_create: 0 = no call is long, the order of the lists as it was before there was a threshold).  The jump-free and the general
dense list of a direction hold their long calls in front of the short ones, a retry row of tiers 1..6 is filled with long calls from the front and with short ones from
the back.  Every output -- columns, dp_iters, dp_score, likelihoods, chosen chains, the call / iteration / cell counters, the calls entering each class -- is per
item: contexts with the threshold at 0, 1 (every call long), the default and 4096 (no call long: the DP takes reads of at most 1024 bases) return identical arrays,
which equal the oracle's.
"""
import numpy as np
import pytest

from tools import synth
from util import compare_chains, seeds_from_chains

pytestmark = pytest.mark.gpu

DEFAULT_T = 48                                   # hlala_api.hip: dp_long_bases
THRESHOLDS = ("0", "1", None, "4096")            # None: the default
EDGE_BASES = (0, 1, 2, DEFAULT_T - 1, DEFAULT_T, DEFAULT_T + 1)      # T - 1, T, T + 1 for T = 1 and for the default
PAIR_INT = ("pair_status", "best_chain", "n_combinations", "strands_valid", "n_cols", "col_level", "col_edge", "col_gchar", "col_schar", "col_fromseed", "col_mapq")
GAP = ord("_")


def make_ctx(pkg, monkeypatch, threshold, w, **kw):
    if threshold is None:
        monkeypatch.delenv("HLALA_DP_LONG_BASES", raising=False)
    else:
        monkeypatch.setenv("HLALA_DP_LONG_BASES", threshold)
    return pkg.Context(w["graph"], w["contigs"], **kw)


def assert_same_arrays(got, ref, label):
    assert set(got) == set(ref), label
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(got[k], v, equal_nan=True) if v.dtype.kind == "f" else np.array_equal(got[k], v), (label, k)


def assert_same_chains(got, ref, label):
    """Every array of hlala_batch_get_chains, as far as the library defines it: the status and the DP outputs (dp_iters, dp_score, ...: reset for every chain) whole,
    the other per-chain values for the chains whose status is 0, the column arrays over each such chain's n_cols columns.  (Behind them a row holds what its memory
    held before -- the rows of a batch are not cleared --, which differs between two contexts however their calls are ordered.)"""
    assert set(got) == set(ref), label
    status = ref["status"]; n = len(status); stride = ref["_stride"]
    ok = status == 0
    assert np.array_equal(got["status"], status), label
    assert np.array_equal(got["n_cols"][ok], ref["n_cols"][ok]), label
    inside = ((np.arange(stride)[None, :] < ref["n_cols"][:, None]) & ok[:, None]).ravel()
    for k, v in ref.items():
        if not isinstance(v, np.ndarray):
            assert got[k] == v, (label, k)
            continue
        g = got[k]
        assert g.shape == v.shape and g.dtype == v.dtype, (label, k)
        if v.size == n * stride:
            g, v = g[inside], v[inside]
        elif v.size == n:
            g, v = g[ok], v[ok]
        else:
            assert v.size == 2 * n and k.startswith("dp_"), (label, k)
        assert np.array_equal(g, v, equal_nan=True) if v.dtype.kind == "f" else np.array_equal(g, v), (label, k)


def assert_pairs_match_oracle(got, ep):
    for k in PAIR_INT:
        assert np.array_equal(got[k], ep[k]), k
    assert np.allclose(got["pair_ll"], ep["pair_ll"], rtol=1e-12, atol=0)
    assert np.allclose(got["pair_mapq"], ep["pair_mapq"], rtol=1e-9, atol=1e-15)
    assert np.allclose(got["mate_mapq"], ep["mate_mapq"], rtol=1e-9, atol=1e-15)


def counters(st):
    return (int(st.n_dp_calls), int(st.n_dp_iterations), int(st.n_dp_cells), int(st.n_errors), tuple(int(x) for x in st.n_dp_class), int(st.n_dp_jump_free),
            int(st.n_chains_retried), int(st.n_dp_retried_large))


def bases_left(gb):
    """(left, right): read bases left of the DP calls the batch's last extension listed (hlala_debug_dp_items: item, rOff, seqLen, start_seq, ...)."""
    items, _ = gb.dp_items()
    nc = items.shape[0] // 2
    l, r = items[:nc], items[nc:]
    return l[l[:, 0] >= 0, 3], (r[:, 2] - r[:, 3])[r[:, 0] >= 0]


def trim_seeds(seeds):
    """Seed chains cut back at both ends so that the read bases left of them are the values of EDGE_BASES, chain c taking EDGE_BASES[c % 6] on the left and
    EDGE_BASES[(c // 6) % 6] on the right: a chain starts and ends on a column that holds a read base and a graph character on a real edge.  An end that cannot be
    put there (the seed starts behind the target) stays where it is."""
    off = seeds["col_off"]; n = seeds["n_chains"]
    sb, se = seeds["chain_seq_begin"].copy(), seeds["chain_seq_end"].copy()
    cols = {k: [] for k in ("col_level", "col_edge", "col_gchar", "col_schar")}
    new_off = [0]
    for c in range(n):
        a, b = int(off[c]), int(off[c + 1])
        s = seeds["col_schar"][a:b]; g = seeds["col_gchar"][a:b]; e = seeds["col_edge"][a:b]
        r = int(seeds["chain_read"][c]); seq_len = int(seeds["read_off"][r + 1] - seeds["read_off"][r])
        has_base = s != GAP
        assert int(has_base.sum()) == int(se[c]) - int(sb[c]) + 1
        before = np.concatenate(([0], np.cumsum(has_base)[:-1])) + int(sb[c])          # read position of a column's base
        anchor = has_base & (g != GAP) & (e >= 0)
        i, j = 0, b - a - 1
        t_l, t_r = EDGE_BASES[c % 6], EDGE_BASES[(c // 6) % 6]
        ci = np.flatnonzero(anchor & (before == t_l))
        cj = np.flatnonzero(anchor & (before == seq_len - 1 - t_r))
        if len(ci) and len(cj) and cj[-1] - ci[0] >= 8:
            i, j = int(ci[0]), int(cj[-1])
        elif len(ci) and j - ci[0] >= 8:
            i = int(ci[0])
        elif len(cj) and cj[-1] >= 8:
            j = int(cj[-1])
        if anchor[i] and anchor[j]:
            sb[c] = before[i]; se[c] = before[j]
        else:
            i, j = 0, b - a - 1
        for k in cols:
            cols[k].append(seeds[k][a + i:a + j + 1])
        new_off.append(new_off[-1] + j + 1 - i)
    out = dict(seeds)
    out.update(chain_seq_begin=sb.astype(np.int32), chain_seq_end=se.astype(np.int32), col_off=np.asarray(new_off, np.int32))
    for k, v in cols.items():
        out[k] = np.concatenate(v).astype(seeds[k].dtype)
    return out


def test_calls_at_the_threshold_in_both_directions(pkg, oracle, monkeypatch):
    """Seed chains trimmed so that 0, 1, 2, 47, 48 and 49 read bases are left of them, on either side: calls just below, at and just above the threshold of 1 and the
    default one, left and right.  Stage B of the four contexts: identical arrays, equal to the oracle's."""
    w = synth.make_world(seed=7, G=6000, k=1)
    b = synth.make_batch(w, 300, seed=17, p_no_clip=0.5)
    kw = dict(insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=777)
    o = oracle(w["graph"], w["contigs"], **kw)
    seeds = trim_seeds(seeds_from_chains(b, o.align_batch(b, stop_after_projection=True)["seeds"]))
    exp = o.extend_seeds(seeds)
    ref = None
    for t in THRESHOLDS:
        ctx = make_ctx(pkg, monkeypatch, t, w, **kw)
        gb = ctx.batch_from_seeds(seeds); gb.extend()
        got, st = gb.chains(1), gb.stats()
        if ref is None:
            left, right = bases_left(gb)
            for v in EDGE_BASES[1:]:          # (no bases left: no call)
                assert (left == v).sum() >= 3 and (right == v).sum() >= 3, (v, int((left == v).sum()), int((right == v).sum()))
            compare_chains(got, exp, seeds["n_chains"], label="trimmed seeds")
            assert (st.n_dp_calls, st.n_dp_iterations, st.n_dp_cells, st.n_errors) == (exp["_stats"][0], exp["_stats"][1], exp["_stats"][2], 0)
            ref = (got, counters(st))
        else:
            assert_same_chains(got, ref[0], t)
            assert counters(st) == ref[1], t


def run_thresholds(pkg, oracle, monkeypatch, w, b, kw, each=None):
    """hlala_align_batch in a context per threshold: stage B and the pairs identical among them and equal to the oracle's; -> {threshold: counters}."""
    exp = oracle(w["graph"], w["contigs"], **kw).align_batch(b)
    ref, seen = None, {}
    for t in THRESHOLDS:
        ctx = make_ctx(pkg, monkeypatch, t, w, **kw)
        gb = ctx.batch(b); gb.align()
        ext, pairs, st = gb.chains(1), gb.pairs(), gb.stats()
        if ref is None:
            compare_chains(ext, exp["ext"], b["n_chains"], label="stage B")
            assert_pairs_match_oracle(pairs, exp["pairs"])
            assert (st.n_dp_calls, st.n_dp_iterations, st.n_dp_cells, st.n_errors) == tuple(int(x) for x in exp["stats"][:3]) + (0,)
            ref = (ext, pairs)
        else:
            assert_same_chains(ext, ref[0], t)
            assert_same_arrays(pairs, ref[1], t)
        seen[t] = counters(st)
        if each:
            each(t, gb, st)
    return seen


def test_no_long_call_only_long_calls_and_the_default(pkg, oracle, monkeypatch):
    """The whole pipeline on a small world: no call long (0, 4096), every call long (1), the default; the calls entering each class are counted alike."""
    w = synth.make_world(seed=8, G=8000, k=3)
    b = synth.make_batch(w, 300, seed=18, clip_max=48, p_no_clip=0.1)
    kw = dict(insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=777, max_columns=384)

    def census(t, gb, st):
        seeds = gb.chains(0); ok = seeds["status"] == 0
        seq_len = np.diff(b["read_off"])[np.repeat(np.arange(2 * b["n_pairs"]), np.diff(b["chain_off"]))]
        left, right = seeds["seq_begin"][ok], (seq_len - 1 - seeds["seq_end"])[ok]          # read bases left of the seed chains
        assert max(left.max(), right.max()) < 4096                                            # threshold 4096: no call is long
        for x in (left, right):                                                               # the default: both kinds, both directions
            assert (x >= DEFAULT_T).sum() >= 10 and ((x > 0) & (x < DEFAULT_T)).sum() >= 10
    seen = run_thresholds(pkg, oracle, monkeypatch, w, b, kw, census)
    assert seen["0"] == seen["1"] == seen[None] == seen["4096"]                               # (n_dp_class among them: the calls entering each class)


def test_retry_rows_filled_from_both_ends(pkg, oracle, monkeypatch):
    """The fan world (nodes with hundreds of edges and gap-path jumps): calls outgrow the 16-lane class and go through the retry rows of the 32-lane, 64-lane and
    wide classes.  Threshold 1: every call that fails is long, the back of every row stays empty -- the rows' old counters, which count the short calls, stay 0
    while the statistics still report the calls; thresholds 0 and 4096: no failing call is long, the front stays empty and the short calls lie at the back of the
    row, n_chains - 1 downwards."""
    w = synth.make_fan_world()
    b = synth.make_batch(w, 260, seed=23, max_secondary=3)
    kw = dict(insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=777, max_columns=384)
    nc = b["n_chains"]

    def rows(t, gb, st):
        cls = [int(x) for x in st.n_dp_class]
        assert sum(cls[1:]) > 0 and sum(cls[3:]) > 0
        wc = gb.work_counters(); _, retry = gb.dp_items()
        short = [[int(wc[12 + 4 * (k - 1) + 2 * p]) for p in (0, 1)] for k in range(1, 7)]
        if t == "1":
            assert not any(any(x) for x in short)
        if t in ("0", "4096"):
            assert [sum(x) for x in short] == cls[1:]
            for k in range(1, 7):
                for p in (0, 1):
                    n = short[k - 1][p]; row = retry[(2 * (k - 1) + p) * nc:(2 * (k - 1) + p + 1) * nc]
                    back = row[nc - n:] - p * nc                       # slots of the item arrays: the right extensions' follow the left ones'
                    assert len(set(back.tolist())) == n and (n == 0 or (back.min() >= 0 and back.max() < nc)), (k, p)
    seen = run_thresholds(pkg, oracle, monkeypatch, w, b, kw, rows)
    assert seen["0"] == seen["1"] == seen[None] == seen["4096"]


def test_tail_pool_reads_two_ended_rows(pkg, oracle, monkeypatch):
    """hlala_set_tail_pool(2): the broad / large / in-memory classes take the retry rows of two batches in one launch.  Two small batches on dense gene windows, every
    failing call long (threshold 1) and the default: each batch's arrays and counters equal those of the batch aligned alone with the threshold at 0, which equal the
    oracle's."""
    w = synth.make_world_m(seed=8, n_levels=60_000, n_windows=3, alleles=(4000, 5000))
    bs = [synth.make_batch_m(w, n, seed=sd, frac_gene=1.0) for n, sd in ((700, 31), (500, 33))]
    kw = dict(insert_mean=bs[0]["insert_mean"], insert_sd=bs[0]["insert_sd"], rng_seed=99, max_columns=384)
    o = oracle(w["graph"], w["contigs"], **kw)
    ref = []
    ctx0 = make_ctx(pkg, monkeypatch, "0", w, **kw)
    for b in bs:
        exp = o.align_batch(b)
        gb = ctx0.batch(b); gb.align()
        ext, pairs, st = gb.chains(1), gb.pairs(), gb.stats()
        compare_chains(ext, exp["ext"], b["n_chains"], label="stage B")
        assert_pairs_match_oracle(pairs, exp["pairs"])
        assert (st.n_dp_calls, st.n_dp_iterations, st.n_dp_cells, st.n_errors) == tuple(int(x) for x in exp["stats"][:3]) + (0,)
        ref.append((ext, pairs, counters(st)))
    assert sum(sum(r[2][4][4:]) for r in ref) > 0          # the pooled classes have work
    for t in ("1", None):
        ctx = make_ctx(pkg, monkeypatch, t, w, **kw)
        ctx.set_tail_pool(2)
        gbs = [ctx.batch(b) for b in bs]
        for g in gbs:
            g.align()
        for g, r in zip(gbs, ref):
            assert_same_arrays(g.pairs(), r[1], t)
            assert_same_chains(g.chains(1), r[0], t)
            assert counters(g.stats()) == r[2], t
