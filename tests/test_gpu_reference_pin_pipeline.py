"""GPU: the projection, pairing and mapping-quality kernels of the product against fixtures written by the REFERENCE's own processBAM.cpp.

tests/golden/ref_proj_*.npz, ref_pair_*.npz and ref_unpaired_*.npz hold small batches and what the static members of mapper::processBAM (built from the
reference's sources by oracle/ref/) make of them -- see tests/golden/make_ref_golden_pipeline.py and tests/golden_pipeline.py.  Here the product faces those files
directly, with no unit left out and -- for the projection and the pairing -- no oracle in between:

  projection  Context + batch + hlala_project_chains + chains(0) (k_project_chains, k_rethread_chains): for every kept record status, n_cols, seq_begin, seq_end,
              removed_cols, levels, edges and both character rows exact;
  pairing     hlala_align_batch + get_pairs (k_pair_chains, k_pair_multi): best_chain, n_combinations, strands_valid, n_cols, every column row and col_mapq
              exact for every pair; pair_ll within rtol 1e-12, pair_mapq / mate_mapq within rtol 1e-9 and atol 1e-15 (the bars of tests/test_gpu_align.py);
  unpaired    hlala_batch_create_unpaired + hlala_align_batch against assignMappingQualities_unpaired, the same rules.  In ref_unpaired_* only the choice of the
              maximum and the mapping qualities (pair_ll, pair_mapq, mate_mapq, best_chain, col_mapq) are the reference's: the finished chains it chose among, and so
              the column rows, are the ORACLE's (the padding of alignOneLongRead is not pinned; they were an input of the reference run).

The library's inGraphGapStretch (hlala_graph_get_gap_stretch), an input of the reference runs that wrote the fixtures, must equal the NumPy statement of the rule
(ref_pipeline.gap_stretch_rule) on every fixture graph.

The product's own decision which records it keeps (the pre-filter of alignOneReadPair, which the reference run took as an input) must equal the stored mask; a
difference is reported as such, before any chain is compared.  Once in the default configuration and once with the band kernel off (HLALA_DP_BAND=0).  The
statistics of a batch do not tell k_pair_chains' pairs from k_pair_multi's, so the test asserts that pairs with one combination (finished by k_pair_chains) and
pairs with several (k_pair_multi) were both there.

The insert-size density is pinned up to its formula (the reference build's boost::math::pdf is a stand-in: exp(-(x-m)^2 / (2 sd^2)) / (sd sqrt(2 pi))); the
pre-filter, BamTools' decoding and the padding of long reads are not pinned.  Reads tests/golden/ only: neither the reference nor anything built from it is
needed on the GPU machine."""
import numpy as np
import pytest

import golden_pipeline as gp
import ref_pipeline as rp

pytestmark = pytest.mark.gpu

ENVS = [dict(), dict(HLALA_DP_BAND="0")]
IDS = ["default", "band-off"]


def _label(name, env):
    return "%s (%s)" % (name, ", ".join("%s=%s" % kv for kv in env.items()) or "default")


def _ctx(pkg, f):
    m = f["meta"]
    ctx = _create(pkg, f, m)
    rule = rp.gap_stretch_rule(f["graph"])
    mine = ctx.graph_gap_stretch()
    assert np.array_equal(mine, rule), "inGraphGapStretch of the library differs from the rule at levels %s" % np.nonzero(mine != rule)[0][:5].tolist()
    return ctx


def _create(pkg, f, m):
    return pkg.Context(f["graph"], f["contigs"], insert_mean=float(m["insert_mean"]), insert_sd=float(m["insert_sd"]), rng_seed=int(m["rng_seed"]),
                       long_read_mode=int(m["long_read_mode"]), max_columns=int(m["max_columns"]))


def _check_keep(status, f, label):
    n = int(f["batch"]["n_chains"])
    assert np.all(status[:n] >= 0), "%s: records flagged with an error: %s" % (label, np.nonzero(status[:n] < 0)[0][:5].tolist())
    mine = (status[:n] == 0).astype(np.uint8)
    diff = np.nonzero(mine != f["keep"])[0]
    assert len(diff) == 0, "%s: the product keeps other records than the stored mask (pre-filter, not a chain mismatch): records %s" % (label, diff[:5].tolist())


@pytest.mark.parametrize("env", ENVS, ids=IDS)
def test_projection_matches_reference_fixtures(pkg, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n_kept = 0
    for name in gp.PROJ_FIXTURES:
        f = gp.load(name)
        ctx = _ctx(pkg, f)
        gb = ctx.batch(f["batch"])
        gb.project()
        got = gb.chains(0)
        _check_keep(got["status"], f, _label(name, env))
        n_kept += gp.check_projection(got, f, _label(name, env))
        gb.close(); ctx.close()
    assert n_kept > 400


@pytest.mark.parametrize("env", ENVS, ids=IDS)
def test_pairing_matches_reference_fixtures(pkg, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    single = multi = below1 = invalid = 0
    for name in gp.PAIR_FIXTURES:
        f = gp.load(name)
        ctx = _ctx(pkg, f)
        gb = ctx.batch(f["batch"])
        gb.align()
        _check_keep(gb.chains(0)["status"], f, _label(name, env))
        got = gb.pairs()
        n = int(f["batch"]["n_pairs"])
        assert np.all(got["pair_status"][:n] == 0) and gb.stats().n_errors == 0
        gp.check_pairs(got, f, _label(name, env))
        single += int((got["n_combinations"][:n] == 1).sum()); multi += int((got["n_combinations"][:n] > 1).sum())
        below1 += int((got["pair_mapq"][:n] < 1).sum()); invalid += int((got["strands_valid"][:n] == 0).sum())
        gb.close(); ctx.close()
    print("pairs with one combination %d, with several %d, mapQ < 1 %d, strands not valid %d" % (single, multi, below1, invalid))
    assert single > 50 and multi > 40 and below1 > 10 and invalid > 5


@pytest.mark.parametrize("env", ENVS, ids=IDS)
def test_unpaired_mapping_qualities_match_reference_fixtures(pkg, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    multi = below1 = 0
    for name in gp.UNPAIRED_FIXTURES:
        f = gp.load(name)
        ctx = _ctx(pkg, f)
        gb = ctx.batch_unpaired(f["batch"])
        gb.align()
        _check_keep(gb.chains(0)["status"], f, _label(name, env))
        got = gb.pairs()
        n = int(f["batch"]["n_pairs"])
        assert np.all(got["pair_status"][:n] == 0)
        gp.check_pairs(got, f, _label(name, env), per_unit=1)
        multi += int((got["n_combinations"][:n] > 1).sum()); below1 += int((got["pair_mapq"][:n] < 1).sum())
        gb.close(); ctx.close()
    assert multi > 30 and below1 > 4
