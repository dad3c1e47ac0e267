"""Regenerates tests/golden/ref_*.npz: seed chains and what the REFERENCE's own extension aligner makes of them.

Unlike r01_small.npz (oracle outputs), the expected outputs here are written by HLA*LA's code: oracle/_ref/libhlala_ref.so, built
from a checkout of the reference by oracle/ref/Makefile, run in mode 0 (the product's seed discipline: rng_seed + 2c on the left DP
of chain c, rng_seed + 2c + 1 on the right DP; see oracle/ref/ref_driver.cpp).  tests/test_gpu_reference_pin.py holds the HIP
kernels against these files directly, with no oracle in between.  Data only: graph description, reads, seed chains (the oracle's
stage-A projection of synthetic alignments: an input), rng_seed, and the reference's columns and log-likelihoods.

One file per DP family, each cut down to stay below the largest file that was here before (hla_nom_g.txt, about 215 KB):
  ref_linear.npz   mostly linear k = 1 world, clips up to 48 bases           (band kernel)
  ref_k10.npz      allele-rich k = 10 world                                  (frontier classes)
  ref_k0ties.npz   gap-heavy k = 0 world, identical haplotypes, long clips   (tied end cells, gap-path jumps)
  ref_fan.npz      the fan world at the levels around its fans               (hundreds of edges / jumps per node: wide classes)
  ref_graphm.npz   one gene window of a Graph M world, cut out of its graph  (suffix-merged allele paths, high node ranks)

Run (needs the reference sources; HLALA_REF_DIR names them):   python tests/golden/make_ref_golden.py
The files committed with this generator were written by the reference whose compiled sources (the REF_SRCS of oracle/ref/Makefile,
concatenated in that order) have the SHA-256
  27a1b48bad4947e236a3ca7f6e22aae6f489305138c49b521733f6e06afc76a3
which every file also carries as meta__ref_sources_sha256.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import synth                      # noqa: E402
from oracle_binding import Oracle             # noqa: E402
import ref_binding as rb                      # noqa: E402
from util import seeds_from_chains            # noqa: E402

RNG_SEED = 4242
STRIDE = 384
SEED_KEYS = ("n_reads", "read_off", "read_bases", "read_quals", "n_chains", "chain_read", "chain_seq_begin", "chain_seq_end", "chain_reverse",
             "col_off", "col_level", "col_edge", "col_gchar", "col_schar")
MAX_BYTES = 214545            # hla_nom_g.txt, the largest file here before these


def project(w, b):
    o = Oracle(w["graph"], w["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=RNG_SEED, max_columns=STRIDE)
    return seeds_from_chains(b, o.align_batch(b, stop_after_projection=True)["seeds"])


def cut(graph, seeds, lo, hi, margin):
    """Levels [lo, hi] of `graph` as a graph of its own (node / edge order kept), with the chains whose seed lies in [lo + margin, hi - margin]
    and the reads of those chains."""
    nl = graph["node_level"]
    keep_n = (nl >= lo) & (nl <= hi)
    new_n = np.cumsum(keep_n) - 1
    keep_e = keep_n[graph["edge_from"]] & keep_n[graph["edge_to"]]
    new_e = np.cumsum(keep_e) - 1
    g = dict(n_levels=hi - lo + 1, n_nodes=int(keep_n.sum()), n_edges=int(keep_e.sum()), node_level=(nl[keep_n] - lo).astype(np.int32),
             edge_from=new_n[graph["edge_from"][keep_e]].astype(np.int32), edge_to=new_n[graph["edge_to"][keep_e]].astype(np.int32),
             edge_label=graph["edge_label"][keep_e])
    chains = []
    for c in range(seeds["n_chains"]):
        lv = seeds["col_level"][seeds["col_off"][c]:seeds["col_off"][c + 1]]
        lv = lv[lv >= 0]
        if len(lv) and lv.min() >= lo + margin and lv.max() <= hi - margin:
            chains.append(c)
    reads = sorted(set(int(seeds["chain_read"][c]) for c in chains))
    rmap = {r: i for i, r in enumerate(reads)}
    ro = seeds["read_off"]
    col = [np.arange(seeds["col_off"][c], seeds["col_off"][c + 1]) for c in chains]
    idx = np.concatenate(col)
    lv = seeds["col_level"][idx]; ed = seeds["col_edge"][idx]
    assert np.all(keep_e[ed[ed >= 0]])
    s = dict(n_reads=len(reads), read_off=np.concatenate([[0], np.cumsum([ro[r + 1] - ro[r] for r in reads])]).astype(np.int32),
             read_bases=np.concatenate([seeds["read_bases"][ro[r]:ro[r + 1]] for r in reads]), read_quals=np.concatenate([seeds["read_quals"][ro[r]:ro[r + 1]] for r in reads]),
             n_chains=len(chains), chain_read=np.array([rmap[int(seeds["chain_read"][c])] for c in chains], np.int32),
             chain_seq_begin=seeds["chain_seq_begin"][chains], chain_seq_end=seeds["chain_seq_end"][chains], chain_reverse=seeds["chain_reverse"][chains],
             col_off=np.concatenate([[0], np.cumsum([len(x) for x in col])]).astype(np.int32),
             col_level=np.where(lv >= 0, lv - lo, lv).astype(np.int32), col_edge=np.where(ed >= 0, new_e[np.maximum(ed, 0)], ed).astype(np.int32),
             col_gchar=seeds["col_gchar"][idx], col_schar=seeds["col_schar"][idx])
    return g, s


def write(name, graph, seeds):
    r = rb.Reference(graph, rng_seed=RNG_SEED, max_columns=STRIDE).extend_seeds(seeds, mode=0)
    n = seeds["n_chains"]
    out = {"graph__" + k: graph[k] for k in ("n_levels", "n_nodes", "n_edges", "node_level", "edge_from", "edge_to", "edge_label")}
    out.update({"seeds__" + k: seeds[k] for k in SEED_KEYS})
    out["meta__rng_seed"] = RNG_SEED; out["meta__max_columns"] = STRIDE; out["meta__ref_sources_sha256"] = rb.sources_hash()
    for k in ("status", "n_cols", "seq_begin", "seq_end", "ll"):
        out["exp__" + k] = r[k][:n]
    mask = (np.arange(STRIDE)[None, :] < r["n_cols"][:n, None]).reshape(-1)          # columns packed chain after chain: exp__n_cols gives the offsets
    for k in ("col_level", "col_edge", "col_gchar", "col_schar", "col_fromseed"):
        out["exp__" + k] = r[k][mask]
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    rl = np.diff(seeds["read_off"])[seeds["chain_read"]]
    both = int(((seeds["chain_seq_begin"] != 0) & (seeds["chain_seq_end"] != rl - 1)).sum())
    print("wrote %s: %d bytes, %d levels, %d nodes, %d edges, %d chains (%d clipped at both ends), %d columns" %
          (name, size, graph["n_levels"], graph["n_nodes"], graph["n_edges"], n, both, int(r["n_cols"][:n].sum())))
    assert size <= MAX_BYTES, "%s is larger than the largest fixture that was here before" % name


def main():
    ok, why = rb.available()
    if not ok:
        raise SystemExit(why)
    print("reference sources sha256:", rb.sources_hash())

    w = synth.make_world(seed=31, G=3000, k=1)
    write("ref_linear.npz", w["graph"], project(w, synth.make_batch(w, 50, seed=41, clip_max=48, p_no_clip=0.0)))

    w = synth.make_world(seed=4, G=3000, k=10)
    write("ref_k10.npz", w["graph"], project(w, synth.make_batch(w, 40, seed=14)))

    w = synth.make_world(seed=51, G=3000, k=0, extra_identical=3, n_largegap=2)
    write("ref_k0ties.npz", w["graph"], project(w, synth.make_batch(w, 25, seed=52, p_secondary=1.0, max_secondary=6, p_random_secondary=0.0, clip_max=45)))

    w = synth.make_fan_world(G=1000, fan=(150, 162), gaps_out=(350, 150), gaps_in=(800, 150))
    write("ref_fan.npz", w["graph"], project(w, synth.make_batch(w, 50, seed=23, max_secondary=3)))

    w = synth.make_world_m(seed=7, n_levels=30_000, n_windows=2, alleles=(400, 1500))
    s = project(w, synth.make_batch_m(w, 300, seed=21, frac_gene=1.0))
    k = int(np.argmax(w["windows"]["n_alleles"]))
    mid = (int(w["windows"]["first_level"][k]) + int(w["windows"]["last_level"][k])) // 2            # 1800 levels from the middle of the window with most alleles
    g, s = cut(w["graph"], s, mid - 900, mid + 900, 200)
    write("ref_graphm.npz", g, s)


if __name__ == "__main__":
    main()
