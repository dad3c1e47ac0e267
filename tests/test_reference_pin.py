"""CPU: the oracle against the reference's own extension aligner, built locally from a checkout of the reference (oracle/ref/).

Every other parity claim of this project ends at oracle/hlala_oracle.cpp, a restatement.  Here the restatement faces the text it
restates: node ranks and edge order (alignerBase), gap paths (Graph::computeGapEdgePaths), extendSeedChain (the frontier DP with its
push order, overwrite rule, patience, end-cell draw and gap-path jumps) and scoreOneAlignment, on the worlds the GPU suite leans on.

Mode 0 of the driver imposes the oracle's and the product's seed discipline on the reference's code (rng_seed + 2c on the left DP of
chain c, rng_seed + 2c + 1 on the right DP: two reference calls for a chain clipped at both ends, see oracle/ref/ref_driver.cpp).  In
mode 0 EVERY chain agrees exactly in all integer and byte outputs, none left out; log-likelihoods within rtol = 1e-12 (both sides add
the same log() terms in the same order on the same libm: the number that differ at all is printed and is expected to be zero).
Mode 1 is one reference call per chain, the reference's native discipline, in which the right DP continues the generator state the
left DP left: everything up to and including the seed's last column still agrees, and so do chains clipped at one end; the share of
chains that differ to the right of the seed is printed.  It guards the two-call scheme against hiding something the single call does.

Each family also asserts what makes its comparison mean something -- DP calls whose end cell was drawn among several best complete
cells, chains clipped at both ends, columns with level -1, columns with a '_' graph character, gap-path jumps taken -- against floors
of about half of what the oracle counts on these inputs (the inputs are deterministic; the counts are printed; gap paths are exact).

The module skips, with the reason, only when neither oracle/_ref/libhlala_ref.so nor the reference sources exist."""
import time

import numpy as np
import pytest

import ref_binding as rb
from test_oracle_kat import _linear_graph, _seed
from test_oracle_properties import _clip_batch
from tools import synth
from util import seeds_from_chains

RS = 777


@pytest.fixture(scope="module")
def ref():
    ok, why = rb.available()
    if not ok:
        pytest.skip(why)
    return rb.Reference


def project(oracle, w, b, rng_seed=RS, max_columns=384):
    """hlala_seeds_in of a batch: the oracle's own projection (stage A), chains it did not filter out."""
    o = oracle(w["graph"], w["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=rng_seed, max_columns=max_columns)
    return seeds_from_chains(b, o.align_batch(b, stop_after_projection=True)["seeds"])


def pin(oracle, ref, graph, seeds, label, tot, rng_seed=RS, max_columns=384, mode1=False):
    """Reference (mode 0, optionally mode 1 too) against the oracle on one set of seed chains; adds the oracle's counts to `tot`."""
    n = seeds["n_chains"]
    o = oracle(graph, None, rng_seed=rng_seed, max_columns=max_columns)
    o.dp_draws(reset=True)
    exp = o.extend_seeds(seeds)
    draws = o.dp_draws()
    t0 = time.time()
    r = ref(graph, rng_seed=rng_seed, max_columns=max_columns)
    got = r.extend_seeds(seeds, mode=0)
    tot["ref_seconds"] = tot.get("ref_seconds", 0.0) + time.time() - t0
    assert np.all(exp["status"][:n] == 0), label
    bad = rb.chain_diffs(got, exp, n)
    assert not bad, "%s: %d of %d chains differ from the reference, first: %s" % (label, len(bad), n, list(bad.items())[:3])
    ll_differ = int((got["ll"] != exp["ll"]).sum())
    scale = np.maximum(1.0, np.abs(got["ll"]))
    assert np.all(np.abs(exp["ll"] - got["ll"]) <= 1e-12 * scale), label
    # gap paths, as sets of (first node, last node, length)
    pr = sorted(zip(*[x.tolist() for x in r.graph_paths()])); po = sorted(zip(*[x.tolist() for x in o.graph_paths()]))
    assert pr == po, "%s: completedGapEdgePaths differ" % label

    st = exp["_stride"]
    mask = np.arange(st)[None, :] < exp["n_cols"][:n, None]
    rl = np.diff(seeds["read_off"])[seeds["chain_read"]]
    both = (seeds["chain_seq_begin"] != 0) & (seeds["chain_seq_end"] != rl - 1)
    c = dict(chains=n, ll_differ=ll_differ, tied_draws=draws["tied_draws"], jumps_taken=draws["jumps_taken"], both_clipped=int(both.sum()),
             level_m1=int(((exp["col_level"].reshape(-1, st)[:n] == -1) & mask).sum()), graph_gap=int(((exp["col_gchar"].reshape(-1, st)[:n] == ord("_")) & mask).sum()),
             paths=len(po))
    if mode1:
        got1 = r.extend_seeds(seeds, mode=1)
        fs = exp["col_fromseed"].reshape(-1, st)[:n]
        upto = np.array([np.nonzero(fs[i])[0].max() + 1 for i in range(n)])
        bad1 = rb.chain_diffs(got1, exp, n, upto=upto)
        assert not bad1, "%s (one call per chain): %d chains differ up to the seed's last column, first: %s" % (label, len(bad1), list(bad1.items())[:3])
        whole = rb.chain_diffs(got1, exp, n)
        assert all(both[i] for i in whole), "%s (one call per chain): a chain clipped at one end differs" % label
        assert np.all(got1["ll"][~both] == got["ll"][~both])
        c["mode1_differ"] = len(whole); c["mode1_chains"] = n
    print("%s: %s" % (label, c))
    for k, v in c.items():
        tot[k] = tot.get(k, 0) + v
    r.close(); o.close()
    return got, exp


def check_floors(tot, family, **floors):
    print("family %s: %s" % (family, {k: (round(v, 1) if isinstance(v, float) else v) for k, v in tot.items()}))
    if tot.get("mode1_chains"):
        print("family %s: one reference call per chain differs to the right of the seed in %.1f %% of the chains" % (family, 100.0 * tot["mode1_differ"] / tot["mode1_chains"]))
    floors = dict(FLOORS[family], **floors)
    for k, v in floors.items():
        assert tot[k] >= v, "family %s: %s = %d, expected at least %d" % (family, k, tot[k], v)


# ------------------------------------------------------------------ hand-derived cases

HAND = [("exact match", "ACGTACGTACGTACGTACGT", (), "ACGTACGTACGTACGTACGT"[4:16], 3, 8, 7),
        ("sequence-complete preferred", "ACGTACGTACGTACG" + "CCCCC", (), "ACGTACGTACGTACG"[4:15] + "A", 0, 8, 4),
        ("affine graph gap", "AAAAAAAAAAAAAAAAAAAA", (), "AAAAAACC", 0, 5, 4),
        ("gap-path jump", "ACGTACGTTTTTACGTACGT", tuple((i, "_") for i in range(8, 12)), "ACGTACGTTTTTACGTACGT"[2:8] + "ACGTACGTTTTTACGTACGT"[12:18], 0, 5, 2)]


def test_hand_derived_cases(oracle, ref):
    """The four hand-derived DP cases of test_oracle_kat.py: the reference gives the oracle's columns, and the hand-derived ones."""
    tot = {}
    res = {}
    for name, g, extra, read, b0, b1, lv0 in HAND:
        got, exp = pin(oracle, ref, _linear_graph(g, extra_edges=extra), _seed(read, b0, b1, lv0), name, tot, mode1=True)
        res[name] = got
    r = res["exact match"]
    assert r["n_cols"][0] == 12 and r["col_level"][:12].tolist() == list(range(4, 16)) and r["col_fromseed"][:12].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    r = res["sequence-complete preferred"]
    assert r["n_cols"][0] == 12 and r["col_level"][:12].tolist() == list(range(4, 16)) and bytes(r["col_gchar"][:12]) == b"ACGTACGTACGC"
    r = res["affine graph gap"]
    assert r["col_level"][:8].tolist() == [4, 5, 6, 7, 8, 9, -1, -1] and bytes(r["col_gchar"][:8]) == b"AAAAAA__" and bytes(r["col_schar"][:8]) == b"AAAAAACC"
    r = res["gap-path jump"]
    assert r["col_level"][:16].tolist() == list(range(2, 18)) and bytes(r["col_schar"][:16]) == b"GTACGT____ACGTAC"
    check_floors(tot, "hand")


def test_gap_paths_by_hand(ref):
    g = _linear_graph("ACGTAC", extra_edges=[(2, "_"), (3, "_"), (4, "_")])
    first, last, length = ref(g).graph_paths()
    assert sorted(zip(first.tolist(), last.tolist(), length.tolist())) == [(2, 3, 1), (2, 4, 2), (2, 5, 3)]


# ------------------------------------------------------------------ the worlds of the GPU suite

def test_full_pipeline_worlds(oracle, ref):
    """The five worlds of test_gpu_align.py::test_full_pipeline_matches_oracle, their batches included."""
    tot = {}
    for seed, G, k, n_pairs in [(1, 5000, 1, 300), (2, 8000, 0, 150), (3, 8000, 3, 300), (4, 3000, 10, 200), (5, 30000, 2, 400)]:
        w = synth.make_world(seed=seed, G=G, k=k)
        b = synth.make_batch(w, n_pairs, seed=seed + 10)
        pin(oracle, ref, w["graph"], project(oracle, w, b), "seed %d G %d k %d" % (seed, G, k), tot, mode1=seed in (1, 2, 4))
    check_floors(tot, "full pipeline")


def test_fan_world(oracle, ref):
    """Nodes with 320 edges and 150 gap-path jumps (make_fan_world): edge push order and the map order of the jumps are pointer order in the reference."""
    tot = {}
    w = synth.make_fan_world()
    b = synth.make_batch(w, 100, seed=23, max_secondary=3)
    pin(oracle, ref, w["graph"], project(oracle, w, b), "fan", tot, mode1=True)
    check_floors(tot, "fan")


def test_tie_heavy_worlds(oracle, ref):
    """The two worlds of test_shared_dps_with_random_end_cells: identical haplotypes, large gaps, long clips -- end cells drawn among equals."""
    tot = {}
    for k, seed in [(0, 51), (2, 52)]:
        w = synth.make_world(seed=seed, G=6000, k=k, extra_identical=3, n_largegap=2)
        b = synth.make_batch(w, 120, seed=seed + 1, p_secondary=1.0, max_secondary=6, p_random_secondary=0.0, clip_max=45)
        pin(oracle, ref, w["graph"], project(oracle, w, b), "ties k %d" % k, tot, mode1=k == 0)
    check_floors(tot, "tie-heavy")


def test_band_worlds(oracle, ref):
    """The six mostly linear worlds of test_band_kernel_and_its_fail_over_are_bit_exact (the band kernel's diet)."""
    from test_gpu_align import BAND_WORLDS
    tot = {}
    for name, wk, bk in BAND_WORLDS:
        w = synth.make_world(**wk)
        b = synth.make_batch(w, 150, **bk)
        pin(oracle, ref, w["graph"], project(oracle, w, b), "band: " + name, tot)
    check_floors(tot, "band")


def test_chain_extension_protocol_world(oracle, ref):
    """`--action testChainExtension`: 10 bases stripped from both ends of true placements (every chain takes two reference calls)."""
    tot = {}
    w = synth.make_world(seed=22, G=6000, k=1)
    b = _clip_batch(w, 200, seed=6)
    pin(oracle, ref, w["graph"], project(oracle, w, b), "clip batch", tot, mode1=True)
    assert tot["both_clipped"] == tot["chains"]
    check_floors(tot, "clip batch")


def test_reads_of_76_and_250_bases(oracle, ref):
    """Read lengths other than 150, as tools/parity_sweep.py draws them: on a stand-in world and on a Graph M world."""
    tot = {}
    w = synth.make_world(seed=61, G=7000, k=1)
    wm = synth.make_world_m(seed=9, n_levels=30_000, n_windows=2, alleles=(200, 800))
    for L in (76, 250):
        b = synth.make_batch(w, 100, seed=62 + L, read_len=L, ins_mean=float(L + 80), ins_sd=30.0, clip_max=L // 3, indel_read_frac=0.0 if L < 100 else 0.2)
        s = project(oracle, w, b, max_columns=512)
        assert np.all(np.diff(s["read_off"]) == L)
        pin(oracle, ref, w["graph"], s, "reads of %d" % L, tot, max_columns=512)
        b = synth.make_batch_m(wm, 60, seed=70 + L, read_len=L, jump_mean=float(L + 200), clip_max=L // 3, frac_gene=0.5)
        pin(oracle, ref, wm["graph"], project(oracle, wm, b, max_columns=512), "Graph M, reads of %d" % L, tot, max_columns=512)
    check_floors(tot, "read lengths")


def test_graph_m_worlds(oracle, ref):
    """Allele-rich gene windows (suffix-merged allele paths, tens to hundreds of nodes per level), reads from allele rows only."""
    tot = {}
    for seed, alleles, n_pairs in [(7, (400, 1500), 60), (8, (1500, 3000), 40)]:
        w = synth.make_world_m(seed=seed, n_levels=30_000, n_windows=2, alleles=alleles)
        b = synth.make_batch_m(w, n_pairs, seed=21, frac_gene=1.0)
        pin(oracle, ref, w["graph"], project(oracle, w, b), "Graph M seed %d (up to %d nodes per level)" % (seed, w["max_nodes_per_level"]), tot, mode1=seed == 7)
    check_floors(tot, "Graph M")


# ------------------------------------------------------------------ the committed fixtures

def _fixture_outputs(f, d):
    """Strided chain outputs `d` in the packed layout of the fixtures."""
    n = int(f["seeds"]["n_chains"]); st = d["_stride"]
    mask = (np.arange(st)[None, :] < d["n_cols"][:n, None]).reshape(-1)
    out = {k: d[k][:n] for k in ("status", "n_cols", "seq_begin", "seq_end", "ll")}
    out.update({k: d[k][:n * st][mask] for k in rb.COL_KEYS})
    return out


def test_oracle_matches_the_committed_reference_fixtures(oracle):
    """tests/golden/ref_*.npz (written by the reference, see make_ref_golden.py) against the oracle: needs no reference, so the pin holds wherever the suite runs."""
    from test_gpu_reference_pin import FIXTURES, load
    for name in FIXTURES:
        f = load(name)
        o = oracle(f["graph"], None, rng_seed=int(f["meta"]["rng_seed"]), max_columns=int(f["meta"]["max_columns"]))
        got = _fixture_outputs(f, o.extend_seeds(f["seeds"]))
        for k, v in f["exp"].items():
            if k == "ll":
                assert np.all(np.abs(got[k] - v) <= 1e-12 * np.maximum(1.0, np.abs(v))), (name, k)
            else:
                assert np.array_equal(got[k], v), (name, k)


def test_committed_fixtures_are_what_the_reference_writes(ref):
    """The reference built here, run on the fixtures' inputs, writes the fixtures' outputs (they are not stale, and not hand-made)."""
    from test_gpu_reference_pin import FIXTURES, load
    for name in FIXTURES:
        f = load(name)
        r = ref(f["graph"], rng_seed=int(f["meta"]["rng_seed"]), max_columns=int(f["meta"]["max_columns"]))
        got = _fixture_outputs(f, r.extend_seeds(f["seeds"], mode=0))
        for k, v in f["exp"].items():
            assert np.array_equal(got[k], v), (name, k)
        if f["meta"]["ref_sources_sha256"] != rb.sources_hash():
            print("%s was written by reference sources %s, this reference is %s: same outputs" % (name, f["meta"]["ref_sources_sha256"], rb.sources_hash()))


# Floors: about half of what the oracle counts on the inputs above (printed by every test), so that a change of a generator that
# empties a family of what it is there for is noticed.
FLOORS = {
    "hand": dict(chains=4, jumps_taken=1, both_clipped=1, level_m1=2, graph_gap=6, paths=4),
    "full pipeline": dict(chains=3900, tied_draws=220, jumps_taken=460, both_clipped=1400, level_m1=17000, graph_gap=23000, paths=1761),
    "fan": dict(chains=240, tied_draws=70, jumps_taken=25, both_clipped=70, level_m1=280, graph_gap=3200, paths=300),
    "tie-heavy": dict(chains=970, tied_draws=120, jumps_taken=180, both_clipped=400, level_m1=4100, graph_gap=6800, paths=1440),
    "band": dict(chains=2400, tied_draws=125, jumps_taken=380, both_clipped=940, level_m1=9000, graph_gap=13500, paths=2337),
    "clip batch": dict(chains=400, tied_draws=12, jumps_taken=50, both_clipped=400, level_m1=800, graph_gap=1400, paths=137),
    "read lengths": dict(chains=870, tied_draws=40, jumps_taken=58, both_clipped=310, level_m1=3900, graph_gap=4700, paths=718),
    "Graph M": dict(chains=290, tied_draws=21, jumps_taken=5, both_clipped=80, level_m1=540, graph_gap=570, paths=557),
}
