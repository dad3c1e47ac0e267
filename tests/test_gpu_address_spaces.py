"""Every launch path that hands the kernels of the paired step a differently shaped descriptor, each against the CPU oracle on a small input.

The kernels take the graph / batch descriptors by value (their pointers are then known to be global memory) or read the device copy through a view whose
pointer members are typed as global (device_common.h: DevGraphG / DevBatchG; the extension DP classes, and the pooled tail through DpPoolArgs).  A pointer that
is typed global but can point into LDS, a descriptor that is stale when it is passed by value, or a null member that a path dereferences shows up here, in
seconds, as a wrong column or a fault -- not in the benchmark.  The comparisons are those of tests/test_gpu_align.py: integers, bytes and indices bit-exact,
log likelihoods within 1e-12 relative, posteriors within 1e-9.

References are computed once per module and shared: the simple world serves the default path, the batch made from seeds, the unpaired batch and the
HLALA_DEBUG=1 run; the dense-window world serves the tail pool and the HLALA_RETHREAD=0 run."""
import ctypes as C

import numpy as np
import pytest

from tools import synth
from util import compare_chains, seeds_from_chains

pytestmark = pytest.mark.gpu

PAIR_INT = ("pair_status", "best_chain", "n_combinations", "strands_valid", "n_cols", "col_level", "col_edge",
            "col_gchar", "col_schar", "col_fromseed", "col_mapq")
UNPAIRED_INT = ("pair_status", "best_chain", "n_combinations", "n_cols", "col_level", "col_edge", "col_gchar", "col_schar", "col_fromseed", "col_mapq")


def debug_chains_clocked(ctx, gb):
    """counters[23] of the batch: the chains whose phase clocks k_project_chains added through B.dbg (0 without HLALA_DEBUG=1: B.dbg is null)."""
    buf = (C.c_ulonglong * 32)()
    ctx.lib.hlala_debug_counters.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
    ctx._check(ctx.lib.hlala_debug_counters(ctx.h, gb.b, buf), "hlala_debug_counters")
    return int(buf[23])


def assert_pairs_equal(got, ep):
    for k in PAIR_INT:
        assert np.array_equal(got[k], ep[k]), k
    assert np.allclose(got["pair_ll"], ep["pair_ll"], rtol=1e-12, atol=0)
    assert np.allclose(got["pair_mapq"], ep["pair_mapq"], rtol=1e-9, atol=1e-15)
    assert np.allclose(got["mate_mapq"], ep["mate_mapq"], rtol=1e-9, atol=1e-15)


def check_aligned(gb, b, exp, label):
    """Seed chains, extended chains, pairs and the DP work counters of an aligned batch against the oracle's."""
    compare_chains(gb.chains(0), exp["seeds"], b["n_chains"], check_ll=False, check_dp=False, label=label + ": stage A")
    compare_chains(gb.chains(1), exp["ext"], b["n_chains"], label=label + ": stage B")
    assert_pairs_equal(gb.pairs(), exp["pairs"])
    st = gb.stats()
    assert st.n_errors == 0
    assert (st.n_dp_calls, st.n_dp_iterations, st.n_dp_cells) == tuple(int(x) for x in exp["stats"][:3]), label
    return st


def check_unpaired(gb, u, e, n, stride, label):
    st = gb.stats()
    assert st.n_errors == 0 and st.n_dp_calls == 0                       # alignOneLongRead never runs the extension DP
    compare_chains(gb.chains(0), e["seeds"], u["n_chains"], check_ll=False, check_dp=False, label=label + ": seeds")
    compare_chains(gb.chains(1), e["ext"], u["n_chains"], check_dp=False, label=label + ": padded chains")
    g = gb.pairs(); x = e["pairs"]
    for key in UNPAIRED_INT:
        per = {"pair_status": n, "best_chain": n, "n_combinations": n, "n_cols": n}.get(key, n * stride)
        assert np.array_equal(np.asarray(g[key])[:per], np.asarray(x[key])[:per]), (label, key)
    assert np.allclose(g["pair_ll"][:n], x["pair_ll"][:n], rtol=1e-12, atol=0)
    assert np.allclose(g["pair_mapq"][:n], x["pair_mapq"][:n], rtol=1e-9) and np.allclose(g["mate_mapq"][:n], x["mate_mapq"][:n], rtol=1e-9)


@pytest.fixture(scope="module")
def simple(oracle):
    """One small world, 300 pairs, the oracle's result (read-only for the tests)."""
    w = synth.make_world(seed=1, G=5000, k=1)
    b = synth.make_batch(w, 300, seed=11)
    kw = dict(insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=777, max_columns=384)
    o = oracle(w["graph"], w["contigs"], **kw)
    return dict(w=w, b=b, kw=kw, o=o, exp=o.align_batch(b))


@pytest.fixture(scope="module")
def dense(oracle):
    """Dense gene windows (4000-5000 alleles, as tests/test_graph_m.py uses them to reach the broad and large classes), three batches, the oracle's results."""
    w = synth.make_world_m(seed=8, n_levels=60_000, n_windows=3, alleles=(4000, 5000))
    bs = [synth.make_batch_m(w, n, seed=sd, frac_gene=fg) for n, sd, fg in ((500, 31, 1.0), (400, 32, 0.6), (300, 33, 1.0))]
    kw = dict(insert_mean=bs[0]["insert_mean"], insert_sd=bs[0]["insert_sd"], rng_seed=99, max_columns=384)
    o = oracle(w["graph"], w["contigs"], **kw)
    return dict(w=w, bs=bs, kw=kw, exp=[o.align_batch(b) for b in bs])


def test_default_paired_path(pkg, simple):
    """(a) hlala_align_batch on a paired batch: descriptors by value in the projection, item, band, stitch and pairing kernels, the device view in the DP classes."""
    ctx = pkg.Context(simple["w"]["graph"], simple["w"]["contigs"], **simple["kw"])
    gb = ctx.batch(simple["b"]); gb.align()
    check_aligned(gb, simple["b"], simple["exp"], "default")
    assert debug_chains_clocked(ctx, gb) == 0                              # no debug buffer: B.dbg is null on this path
    gb.close(); ctx.close()


def test_batch_made_from_seeds(pkg, simple):
    """(b) A batch made from seed chains: chain_order / chain_row / every stage A input are null in its descriptor, rows are chain numbers."""
    seeds = seeds_from_chains(simple["b"], simple["exp"]["seeds"])
    exp = simple["o"].extend_seeds(seeds)
    ctx = pkg.Context(simple["w"]["graph"], simple["w"]["contigs"], **simple["kw"])
    gb = ctx.batch_from_seeds(seeds); gb.extend()
    st = gb.stats()
    assert st.n_errors == 0
    compare_chains(gb.chains(1), exp, seeds["n_chains"], label="from seeds")
    assert (st.n_dp_calls, st.n_dp_iterations, st.n_dp_cells) == tuple(int(x) for x in exp["_stats"][:3])
    gb.close(); ctx.close()


def test_unpaired_batch_and_short_long_reads(pkg, oracle, simple):
    """(c) The unpaired descriptor (one read per unit, no DP arrays in use) through the LDS projection, and a few kilobase reads through the slab-backed
    instantiation (max_columns = 16384), which shares its helpers with the paired one."""
    w = simple["w"]
    u = synth.as_unpaired(simple["b"]); n = u["n_pairs"]
    kw = dict(insert_mean=200.0, insert_sd=35.0, rng_seed=777, long_read_mode=1)
    e = oracle(w["graph"], w["contigs"], **kw).align_long_reads(u)
    ctx = pkg.Context(w["graph"], w["contigs"], **kw)
    gb = ctx.batch_unpaired(u); gb.align()
    check_unpaired(gb, u, e, n, 384, "unpaired")
    gb.close(); ctx.close()
    lr = synth.make_long_batch(w, 12, seed=8, len_lo=600, len_hi=2500)
    kw = dict(insert_mean=200.0, insert_sd=35.0, rng_seed=3, long_read_mode=1, max_columns=16384)
    e = oracle(w["graph"], w["contigs"], **kw).align_long_reads(lr)
    ctx = pkg.Context(w["graph"], w["contigs"], **kw)
    gb = ctx.batch_unpaired(lr); gb.align()
    check_unpaired(gb, lr, e, 12, 16384, "long reads")
    assert int(np.asarray(e["pairs"]["n_cols"])[:12].max()) > 600
    gb.close(); ctx.close()


def test_tail_pool_of_two_over_three_alignments_and_flush(pkg, dense):
    """(d) hlala_set_tail_pool(2): the broad / large / in-memory classes of two alignments run in one launch, whose kernels find the batches' descriptors
    through DpPoolArgs; the third alignment stays pending until hlala_flush."""
    ctx = pkg.Context(dense["w"]["graph"], dense["w"]["contigs"], **dense["kw"])
    ctx.set_tail_pool(2)
    gbs = [ctx.batch(b) for b in dense["bs"]]
    for g in gbs:
        g.align()
    ctx.flush()
    pooled = 0
    for i in (2, 0, 1):
        st = check_aligned(gbs[i], dense["bs"][i], dense["exp"][i], "tail pool, batch %d" % i)
        pooled += sum(int(x) for x in list(st.n_dp_class)[4:])
    assert pooled > 0                                                     # the pooled classes had work
    for g in gbs:
        g.close()
    ctx.close()


def test_stage_calls_on_one_batch_while_two_alignments_wait_in_the_tail_pool(pkg, dense):
    """(d') hlala_set_tail_pool(3) with two alignments pending, the third batch taken through the three stage calls: its extension runs every DP class on
    the main stream, on the slabs that the pending alignments' wide classes used on the side stream and their pooled classes have yet to use.  The stage
    call queues the pooled launches first and waits for the side stream.  Each batch is the stage-call batch once; all three match the oracle every time."""
    ctx = pkg.Context(dense["w"]["graph"], dense["w"]["contigs"], **dense["kw"])
    ctx.set_tail_pool(3)
    staged_tail = 0
    for k in range(3):
        gbs = [ctx.batch(b) for b in dense["bs"]]
        for i in range(3):
            if i != k:
                gbs[i].align()
        gbs[k].project(); gbs[k].extend(); gbs[k].pair()
        for i in range(3):
            st = check_aligned(gbs[i], dense["bs"][i], dense["exp"][i], "stage calls on batch %d, batch %d" % (k, i))
            if i == k:
                staged_tail += sum(int(x) for x in list(st.n_dp_class)[4:])
        for g in gbs:
            g.close()
    assert staged_tail > 0                                                # a stage-call batch had calls in the classes the pool defers
    ctx.close()


def test_pairing_stage_call_on_a_batch_that_waits_in_the_tail_pool(pkg, dense):
    """(d'') hlala_pair_chains on a batch whose alignment is still pending in the tail pool: the call flushes the pool first, so the pooled classes and the
    batch's second stitch pass lie in front of the pairing pass, which then takes every pair on the main stream.  Results are the oracle's."""
    ctx = pkg.Context(dense["w"]["graph"], dense["w"]["contigs"], **dense["kw"])
    ctx.set_tail_pool(3)
    gbs = [ctx.batch(b) for b in dense["bs"][:2]]
    for g in gbs:
        g.align()                                                         # two of three: both stay pending
    gbs[0].pair()
    for i in (0, 1):
        check_aligned(gbs[i], dense["bs"][i], dense["exp"][i], "pair() on a pooled batch, batch %d" % i)
    for g in gbs:
        g.close()
    ctx.close()


def test_every_dp_class_up_to_the_in_memory_one(pkg, oracle):
    """(e) A pair whose DP calls outgrow every LDS class (tests/test_full_scale.py: pair 13 255 of the 5 M-level Graph M world's gene-window batch -- the first
    13 256 pairs of that batch are the same whatever its size): the in-memory class keeps its table structure in the HBM slab, where a pointer into it is a
    global pointer, while the other classes keep theirs in LDS.  The one input known to reach that class; generating its world takes most of the test's time."""
    from hla_la_amd import dist as D
    w = synth.make_world_m(seed=2)
    b = synth.make_batch_m(w, 13256, seed=77, frac_gene=1.0)
    sub, p0, c0 = D.shard_pairs_range(b, 13255, 13256)
    kw = dict(insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], max_columns=384)
    exp = oracle(w["graph"], w["contigs"], rng_seed=(12345 + 2 * c0) & 0xFFFFFFFF, **kw).align_batch(sub)
    ctx = pkg.Context(w["graph"], w["contigs"], rng_seed=12345, **kw)
    gs = ctx.batch(sub); gs.set_first_chain(c0); gs.align()
    st = check_aligned(gs, sub, exp, "pair 13255")
    cls = [int(x) for x in st.n_dp_class]
    print("DP calls per class (16-lane, 32-lane, 64-lane, wide, broad, large, in-memory):", cls)
    assert cls[6] > 0 and all(c > 0 for c in cls[:6]), cls                # a call reaches the last class through every class before it
    gs.close(); ctx.close()


def test_debug_counters_path(pkg, simple, monkeypatch):
    """(f) HLALA_DEBUG=1 (read by hlala_create): B.dbg is non-null and the kernels add their phase clocks through it; results do not move."""
    monkeypatch.setenv("HLALA_DEBUG", "1")
    ctx = pkg.Context(simple["w"]["graph"], simple["w"]["contigs"], **simple["kw"])
    gb = ctx.batch(simple["b"]); gb.align()
    check_aligned(gb, simple["b"], simple["exp"], "HLALA_DEBUG=1")
    assert debug_chains_clocked(ctx, gb) > 0                               # the kernels went through the non-null B.dbg
    gb.close(); ctx.close()


def test_band_fail_over_and_rethreading_inside_the_projection(pkg, oracle, dense, monkeypatch):
    """(g) HLALA_DP_BAND_RISKY=1 on a linear world: band calls walk past their run and go through the fail-over list to the general 16-lane instantiation;
    HLALA_RETHREAD=0 on gene windows: the chunked re-threading DP runs inside k_project_chains instead of k_rethread_chains."""
    monkeypatch.setenv("HLALA_DP_BAND_RISKY", "1")
    w = synth.make_world(seed=32, G=6000, k=0, n_mut=0, n_largegap=0)
    b = synth.make_batch(w, 300, seed=42, indel_read_frac=0.3)
    kw = dict(insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=777, max_columns=384)
    exp = oracle(w["graph"], w["contigs"], **kw).align_batch(b)
    ctx = pkg.Context(w["graph"], w["contigs"], **kw)
    gb = ctx.batch(b); gb.align()
    st = check_aligned(gb, b, exp, "band-risky")
    assert st.n_dp_band > 0 and st.n_dp_band_failed > 0
    gb.close(); ctx.close()
    monkeypatch.delenv("HLALA_DP_BAND_RISKY")
    # work counter 3 is the draw counter of k_rethread_chains: it moves when that kernel runs, and stays 0 when the chunked form runs inside k_project_chains
    ctx = pkg.Context(dense["w"]["graph"], dense["w"]["contigs"], **dense["kw"])
    gb = ctx.batch(dense["bs"][0]); gb.project()
    assert int(gb.work_counters()[3]) > 0
    gb.close(); ctx.close()
    monkeypatch.setenv("HLALA_RETHREAD", "0")
    ctx = pkg.Context(dense["w"]["graph"], dense["w"]["contigs"], **dense["kw"])
    gb = ctx.batch(dense["bs"][0]); gb.align()
    check_aligned(gb, dense["bs"][0], dense["exp"][0], "HLALA_RETHREAD=0")
    assert int(gb.work_counters()[3]) == 0
    gb.close(); ctx.close()
