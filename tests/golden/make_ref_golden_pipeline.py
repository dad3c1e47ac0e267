"""Regenerates tests/golden/ref_proj_*.npz, ref_pair_*.npz and ref_unpaired_*.npz: small batches and what the REFERENCE's own processBAM.cpp makes of them.

The expected outputs are written by HLA*LA's code: oracle/_ref/libhlala_ref.so, built from a checkout of the reference by oracle/ref/Makefile, through
ref_project_chains / ref_pair_chains / ref_mapq_unpaired of oracle/ref/ref_driver.cpp (tests/golden_pipeline.py: reference_outputs).  Data only: graph and contig
descriptions, read pairs with their alignment records, the keep mask (the oracle's decision which records pass the pre-filter of alignOneReadPair: an input), the
parameters, and the reference's seed chains / selected pairs / mapping qualities.  tests/test_gpu_reference_pin_pipeline.py holds the HIP kernels against these
files directly.

  corner       the corner CIGARs of tests/ref_pipeline.py (=/X, empty P, H, leading S and I, I next to D, long insertions, insertions at skipped levels, seeds
               at and inside gap stretches) on a gap-heavy k = 0 world
  gaps         gap-heavy k = 0 world, generated records, a share of the non-primary records hard-clipped
  fan          the fan world around its fans (hundreds of edges per node)
  graphm       one gene window of a Graph M world, cut out of its graph and its contigs
  secondaries  identical haplotypes, a secondary for every read (p_secondary = 1.0), records in reverse order, every fourth pair on one strand
  limits       tests/pair_edge_cases.limits(): 64 kept chains per mate, 128 / 129 / 1023 / 1024 combinations (ref_pair_limits.npz only; no larger than the largest
               ref_pair_*.npz that was here before it)
  ref_unpaired_long.npz   single reads of 200 to 400 bases with long-read error rates (below the 512 columns up to which the product takes reads with several
                          alignments), most with a second alignment: assignMappingQualities_unpaired (the finished chains are the oracle's: an input)
  ref_unpaired_short.npz  the mates of a tie-heavy paired batch read as single reads (several records per read, mapping qualities below 1)

Every file stays below MAX_BYTES, the bound make_ref_golden.py enforces.  Run (needs the reference sources; HLALA_REF_DIR names them):
    python tests/golden/make_ref_golden_pipeline.py
The files carry the SHA-256 over the compiled reference sources (REF_SRCS + REF_SRCS_PIPELINE of oracle/ref/Makefile, concatenated in that order) as
meta__ref_sources_sha256; the files committed with this generator were written by
  475503443a52320fcae9d922ed46e518b25e5a481548abb2318f6f8da13af851
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
import ref_pipeline as rp                     # noqa: E402
import golden_pipeline as gp                  # noqa: E402
from make_ref_golden import MAX_BYTES         # noqa: E402

RNG_SEED = 4242
STRIDE = 384


def span(b, c):
    """reference positions [first, last] a record covers"""
    n = sum(l for l, o in rp.cigar_of(b, c) if o in "M=XDN")
    return int(b["chain_pos"][c]), int(b["chain_pos"][c]) + max(n, 1) - 1


def cut_world(w, b, lo, hi, margin):
    """Levels [lo, hi] of the world as a world of its own (node / edge / contig order kept, contigs cut to their positions on those levels and dropped when no record
    is left on them) with the pairs of `b` whose records all lie on levels [lo + margin, hi - margin]."""
    g = w["graph"]; C = w["contigs"]; off = np.asarray(C["contig_off"]); lvl = np.asarray(C["contig_level"])
    pairs = []
    for p in range(b["n_pairs"]):
        ok = True
        for c in range(int(b["chain_off"][2 * p]), int(b["chain_off"][2 * p + 2])):
            h = int(b["chain_contig"][c]); a, z = span(b, c); l = lvl[off[h]:off[h + 1]]
            ok = ok and int(b["chain_offset"][c]) == 0 and a >= 0 and z < len(l) and l[a] >= lo + margin and l[z] <= hi - margin
        if ok:
            pairs.append(p)
    nb = rp.subset_units(b, pairs)
    used = sorted(set(int(x) for x in nb["chain_contig"]))
    hmap = {h: i for i, h in enumerate(used)}
    seqs, lvls, pos = [], [], np.asarray(nb["chain_pos"]).copy()
    for c in range(nb["n_chains"]):
        h = int(nb["chain_contig"][c]); l = lvl[off[h]:off[h + 1]]
        pos[c] -= int((l < lo).sum())
    for h in used:
        l = lvl[off[h]:off[h + 1]]; m = (l >= lo) & (l <= hi)
        seqs.append(np.asarray(C["contig_seq"])[off[h]:off[h + 1]][m]); lvls.append(l[m] - lo)
    nb["chain_pos"] = pos.astype(np.int32); nb["chain_contig"] = np.asarray([hmap[int(h)] for h in nb["chain_contig"]], np.int32)
    contigs = dict(n_contigs=len(used), contig_off=np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64), contig_seq=np.concatenate(seqs).astype(np.uint8),
                   contig_level=np.concatenate(lvls).astype(np.int32), contig_seqid=np.asarray(C["contig_seqid"])[used].astype(np.int32))
    nl = np.asarray(g["node_level"])
    keep_n = (nl >= lo) & (nl <= hi)
    new_n = np.cumsum(keep_n) - 1
    keep_e = keep_n[g["edge_from"]] & keep_n[g["edge_to"]]
    graph = dict(n_levels=hi - lo + 1, n_nodes=int(keep_n.sum()), n_edges=int(keep_e.sum()), node_level=(nl[keep_n] - lo).astype(np.int32),
                 edge_from=new_n[g["edge_from"][keep_e]].astype(np.int32), edge_to=new_n[g["edge_to"][keep_e]].astype(np.int32), edge_label=np.asarray(g["edge_label"])[keep_e])
    return dict(graph=graph, contigs=contigs), nb


MAX_PAIR_LIMITS_BYTES = 47851          # ref_pair_graphm.npz, the largest ref_pair_*.npz before ref_pair_limits.npz


def write(world_name, w, b, unpaired=False, long_read_mode=0, stride=STRIDE, kinds=("proj", "pair"), max_bytes=MAX_BYTES):
    o = Oracle(w["graph"], w["contigs"], insert_mean=b.get("insert_mean", 200.0), insert_sd=b.get("insert_sd", 35.0), rng_seed=RNG_SEED, long_read_mode=long_read_mode, max_columns=stride)
    res = o.align_long_reads(b) if unpaired else o.align_batch(b, stop_after_projection=True)
    status = res["seeds"]["status"][:b["n_chains"]]
    assert np.all(status >= 0)
    meta = dict(rng_seed=RNG_SEED, max_columns=stride, insert_mean=float(b.get("insert_mean", 200.0)), insert_sd=float(b.get("insert_sd", 35.0)), long_read_mode=long_read_mode,
                ref_sources_sha256=rb.sources_hash(pipeline=True))
    inputs = gp.pack_inputs(w["graph"], w["contigs"], b, status == 0, meta)
    names = ["ref_unpaired_%s.npz" % world_name] if unpaired else ["ref_%s_%s.npz" % (k, world_name) for k in kinds]
    for name in names:
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **inputs)
        exp = gp.reference_outputs(gp.load(name), name)
        np.savez_compressed(path, **inputs, **{"exp__" + k: v for k, v in exp.items()})
        size = os.path.getsize(path)
        extra = ""
        if gp.kind_of(name) != "proj":
            extra = ", %d units with several combinations, %d with mapQ < 1" % (int((exp["n_combinations"] > 1).sum()), int((exp["pair_mapq"] < 1).sum()))
        print("wrote %s: %d bytes, %d levels, %d nodes, %d edges, %d contigs, %d units, %d records (%d kept)%s" %
              (name, size, w["graph"]["n_levels"], w["graph"]["n_nodes"], w["graph"]["n_edges"], w["contigs"]["n_contigs"], b["n_pairs"], b["n_chains"], int((status == 0).sum()), extra))
        assert size <= max_bytes, "%s is larger than the largest fixture that was here before" % name


def main():
    ok, why = rb.available()
    if not ok:
        raise SystemExit(why)
    print("reference sources sha256 (aligner + pipeline):", rb.sources_hash(pipeline=True))

    w = synth.make_world(seed=51, G=3000, k=0, extra_identical=3, n_largegap=2)
    kinds = [k for k in rp.CORNER_KINDS if k not in ("skip_N", "pad", "all_I")] + list(rp.GAP_KINDS)
    b, _ = rp.corner_batch(w, synth.make_batch(w, 3 * len(kinds), seed=91, p_secondary=0.0, indel_read_frac=0.0), kinds, rb.gap_stretch_rule(w["graph"]))
    write("corner", *cut_world(w, b, 0, w["graph"]["n_levels"] - 1, 0))

    w = synth.make_world(seed=2, G=3000, k=0)
    b, _ = rp.hardclip_nonprimary(synth.make_batch(w, 40, seed=12, p_secondary=0.8), 0.5, seed=5)
    write("gaps", *cut_world(w, b, 0, w["graph"]["n_levels"] - 1, 0))

    w = synth.make_fan_world(G=1000, fan=(150, 162), gaps_out=(350, 150), gaps_in=(800, 150))
    write("fan", *cut_world(w, synth.make_batch(w, 30, seed=23, max_secondary=3), 0, w["graph"]["n_levels"] - 1, 0))

    w = synth.make_world_m(seed=7, n_levels=30_000, n_windows=2, alleles=(400, 1500))
    k = int(np.argmax(w["windows"]["n_alleles"]))
    mid = (int(w["windows"]["first_level"][k]) + int(w["windows"]["last_level"][k])) // 2
    write("graphm", *cut_world(w, synth.make_batch_m(w, 700, seed=21, frac_gene=1.0), mid - 900, mid + 900, 150))

    w = synth.make_world(seed=52, G=3000, k=2, extra_identical=3, n_largegap=2)
    b = synth.make_batch(w, 30, seed=54, p_secondary=1.0, max_secondary=6, p_random_secondary=0.3, clip_max=45)
    write("secondaries", *cut_world(w, rp.same_strand_pairs(rp.reversed_chain_order(b), every=4), 0, w["graph"]["n_levels"] - 1, 0))

    import pair_edge_cases as pe
    f = pe.limits()
    write("limits", f["world"], f["batch"], kinds=("pair",), max_bytes=MAX_PAIR_LIMITS_BYTES)

    w = synth.make_world(seed=3, G=3000, k=3)
    write("long", w, {k: v for k, v in synth.make_long_batch(w, 30, seed=5, len_lo=200, len_hi=400, p_second=0.7).items()}, unpaired=True, long_read_mode=1, stride=512)

    w = synth.make_world(seed=52, G=3000, k=2, extra_identical=3, n_largegap=2)
    b = synth.as_unpaired(synth.make_batch(w, 25, seed=53, p_secondary=1.0, max_secondary=6, p_random_secondary=0.0, clip_max=45))
    write("short", w, b, unpaired=True)


if __name__ == "__main__":
    main()
