"""The fixtures tests/golden/ref_proj_*.npz, ref_pair_*.npz and ref_unpaired_*.npz: what the REFERENCE's processBAM.cpp (built by oracle/ref/) makes of small
batches -- projected seed chains, selected pairs with their mapping qualities, unpaired mapping qualities.  Written by tests/golden/make_ref_golden_pipeline.py;
read by tests/test_gpu_reference_pin_pipeline.py (the HIP kernels against them, no oracle and no reference needed) and by tests/test_reference_pin_pipeline.py
(the oracle against them; the reference writes them again).

Layout of a file: sections graph__ (hlala_graph_desc), contigs__ (hlala_contigs_desc), batch__ (hlala_batch_in), keep (one byte per record: the oracle's decision
which records survive the pre-filter of alignOneReadPair -- an input of the reference run, and what the product's own decision is compared with), exp__ (the
reference's outputs; column arrays packed row after row, exp__n_cols gives the offsets) and meta__ (rng_seed, max_columns, insert_mean, insert_sd,
long_read_mode, ref_sources_sha256: the hash over REF_SRCS + REF_SRCS_PIPELINE of oracle/ref/Makefile).  Arrays that are ramps (node levels, edge endpoints,
level tables) are stored as differences (key + "__delta")."""
import os

import numpy as np

import ref_pipeline as rp

HERE = os.path.dirname(os.path.abspath(__file__))
WORLDS = ("corner", "gaps", "fan", "graphm", "secondaries")
PROJ_FIXTURES = tuple("ref_proj_%s.npz" % w for w in WORLDS)
PAIR_FIXTURES = tuple("ref_pair_%s.npz" % w for w in WORLDS) + ("ref_pair_limits.npz",)          # limits: tests/pair_edge_cases.limits(), the pairing stage at its capacities
UNPAIRED_FIXTURES = ("ref_unpaired_long.npz", "ref_unpaired_short.npz")
DELTA = ("graph__node_level", "graph__edge_from", "graph__edge_to", "contigs__contig_level")
GRAPH_KEYS = ("n_levels", "n_nodes", "n_edges", "node_level", "edge_from", "edge_to", "edge_label")
CONTIG_KEYS = ("n_contigs", "contig_off", "contig_seq", "contig_level", "contig_seqid")
BATCH_KEYS = ("n_pairs", "read_off", "read_bases", "read_quals", "chain_off", "read_primary", "n_chains", "chain_contig", "chain_pos", "chain_offset", "chain_as",
              "chain_reverse", "cigar_off", "cigar")
PROJ_COLS = ("col_level", "col_edge", "col_gchar", "col_schar")
PAIR_SCALARS = ("best_chain", "n_combinations", "pair_ll", "pair_mapq", "mate_mapq", "strands_valid", "n_cols")
UNPAIRED_COLS = ("col_level", "col_edge", "col_gchar", "col_schar", "col_mapq")


def kind_of(name):
    return name.split("_")[1]


def pack_inputs(graph, contigs, batch, keep, meta):
    out = {"graph__" + k: graph[k] for k in GRAPH_KEYS}
    out.update({"contigs__" + k: contigs[k] for k in CONTIG_KEYS})
    out.update({"batch__" + k: batch[k] for k in BATCH_KEYS})
    out["keep"] = np.asarray(keep, np.uint8)
    out.update({"meta__" + k: v for k, v in meta.items()})
    for k in DELTA:
        out[k + "__delta"] = np.diff(np.asarray(out.pop(k), np.int64), prepend=0).astype(np.int32)
    return out


def load(name):
    z = np.load(os.path.join(HERE, "golden", name))
    d = dict(graph={}, contigs={}, batch={}, exp={}, meta={})
    for k in z.files:
        v = z[k]
        if k.endswith("__delta"):
            k = k[:-len("__delta")]; v = np.cumsum(v.astype(np.int64)).astype(np.int32)
        if k == "keep":
            d["keep"] = v
            continue
        sec, key = k.split("__", 1)
        d[sec][key] = v.item() if v.shape == () else v
    return d


def check_projection(got, f, label):
    """Stage-A chains `got` (strided) against the reference's seed chains of projection fixture `f`: every kept record, exact."""
    e = f["exp"]; stride = got["_stride"]
    exp = rp.unpack_rows(e, e["n_cols"], stride, PROJ_COLS)
    exp.update({k: e[k] for k in ("status", "seq_begin", "seq_end", "removed_cols")})
    exp["col_fromseed"] = (np.arange(stride)[None, :] < e["n_cols"][:, None]).astype(np.uint8).reshape(-1)          # is_from_BWAseed of a seed chain: all true (:3124)
    rows = np.nonzero(f["keep"])[0]
    bad = rp.projection_diffs(got, exp, rows)
    print("%s: %d kept records of %d, %d columns" % (label, len(rows), len(f["keep"]), int(e["n_cols"][rows].sum())))
    assert not bad, "%s: the projection of %d of %d kept records differs from the reference, first: %s" % (label, len(bad), len(rows), list(bad.items())[:3])
    return len(rows)


def check_pairs(got, f, label, per_unit=2):
    """Pairs (per_unit = 1: single reads) `got` against pair / unpaired fixture `f`: every unit, with the rules of ref_pipeline.pair_diffs."""
    e = f["exp"]; stride = got["_stride"]; n = int(f["batch"]["n_pairs"])
    cols = rp.PAIR_COLS if per_unit == 2 else UNPAIRED_COLS
    exp = rp.unpack_rows(e, e["n_cols"], stride, cols)
    exp.update({k: e[k] for k in PAIR_SCALARS})
    bad, differ = rp.pair_diffs(got, exp, n, per_unit=per_unit, cols=cols)
    print("%s: %d units, %d with more than one combination, %d doubles differ at all" % (label, n, int((e["n_combinations"] > 1).sum()), differ))
    assert not bad, "%s: %d of %d units differ from the reference, first: %s" % (label, len(bad), n, list(bad.items())[:3])
    return n


def reference_outputs(f, name):
    """The exp__ section of fixture `name`, computed anew by the reference built here from the inputs `f` holds (needs oracle/_ref/libhlala_ref.so)."""
    import ref_binding as rb
    from util import seeds_from_chains
    m = f["meta"]; b = f["batch"]; stride = int(m["max_columns"]); kind = kind_of(name)
    r = rb.Reference(f["graph"], rng_seed=int(m["rng_seed"]), long_read_mode=int(m["long_read_mode"]), max_columns=stride)
    if kind == "unpaired":
        # the finished chains of the long reads and their log-likelihoods are the ORACLE's (the padding of alignOneLongRead is not pinned): inputs of the reference run
        from oracle_binding import Oracle
        n = int(b["n_pairs"])
        ext = Oracle(f["graph"], f["contigs"], rng_seed=int(m["rng_seed"]), long_read_mode=int(m["long_read_mode"]), max_columns=stride).align_long_reads(b)["ext"]
        chains = rp.finished_chains(b, ext, n)
        got = r.mapq_unpaired(chains, ext["ll"][chains["_keep"]], n)
        got["best_chain"][:n] = chains["_keep"][got["best_chain"][:n]]
        out = {k: got[k][:n] for k in PAIR_SCALARS}
        out.update(rp.pack_rows(got, n, UNPAIRED_COLS))
        return out
    proj = r.project_chains(f["contigs"], b, f["keep"], rb.gap_stretch_rule(f["graph"]))
    nc = int(b["n_chains"])
    if kind == "proj":
        out = {k: proj[k][:nc] for k in ("status", "n_cols", "seq_begin", "seq_end", "removed_cols")}
        out.update(rp.pack_rows(proj, nc, PROJ_COLS))
        return out
    n = int(b["n_pairs"])
    seeds = seeds_from_chains(b, proj)
    pairs, ext, pen = r.pair_chains(f["contigs"], seeds, seeds["_keep"], n, float(m["insert_mean"]), float(m["insert_sd"]))
    out = {k: pairs[k][:(n if k in ("n_combinations", "pair_ll", "pair_mapq", "strands_valid") else 2 * n)] for k in PAIR_SCALARS}
    out.update(rp.pack_rows(pairs, 2 * n, rp.PAIR_COLS))
    out["best_is_penalty"] = pen
    return out
