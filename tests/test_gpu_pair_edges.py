"""The pairing kernels (k_pair_chains, k_pair_multi<., false>, k_pair_multi<., true>, pair_insert_ll, pair_positions) at every capacity edge, on the batches of
tests/pair_edge_cases.py: 63 / 64 / 65 kept chains per mate, more than 64 records, 128 / 129 / 1023 / 1024 / 1025 combinations, the maximum in the last
combination and tied across strides of 64, batch sizes around the draws, chains of 192 / 193 / 481 columns, every distance around both ends of the insert-size
table, 16 / 17 / 33 sequences per level, single reads, and pairs deferred to the second pairing pass.

Every family runs fused (hlala_align_batch) and stage by stage (project, extend, pair, and pair once more on the resident batch).  Every pair that is not refused
equals the oracle's (integers, column rows and Phred bytes exactly, pair_ll within rtol 1e-12, posteriors exactly) and lies within the bounds of
tests/pair_reference.py fed with the library's own extended chains; refused pairs carry exactly pair_status -1, best_chain -1, n_combinations 0, and where
they are the batch's last pairs the others equal the run without them.  Which kernel took which pair is read off Batch.work_counters().
tests/test_gpu_reference_pin_pipeline.py holds the kernels against tests/golden/ref_pair_limits.npz (the reference's own answers at 64 chains and 1024 combinations).

Largest error / bound ratios are printed (pytest -s)."""
import numpy as np
import pytest

import pair_edge_cases as pe
import pair_reference as pr
import ref_pipeline as rp
from test_pair_reference import FAMILIES

pytestmark = pytest.mark.gpu

WC_PAIR_MULTI = 40          # csrc/batch.h: [+0] class 0 listed, [+1] fetched, [+2] class 1 listed, [+3] fetched; [+4 ..] the same of the side-stream pass
SCALARS = ("pair_status", "best_chain", "n_combinations", "strands_valid", "n_cols", "pair_mapq", "mate_mapq", "pair_ll")
GPU_FAMILIES = dict(FAMILIES, **{"records-error": lambda: pe.records(True), "too-long": pe.too_long})


def _context(pkg, f, rng_seed=5):
    b = f["batch"]
    return pkg.Context(f["world"]["graph"], f["world"]["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=rng_seed, max_columns=f["max_columns"])


def _batch(ctx, f, b):
    return ctx.batch_unpaired(b) if f.get("unpaired") else ctx.batch(b)


def _equal_runs(a, z, label):
    for k in SCALARS + rp.PAIR_COLS:
        assert np.array_equal(a[k], z[k]), (label, k)


def _against_oracle(got, exp, units, per, label, offset=0):
    """Units `units` of `got` against the oracle's outputs `exp` (whose unit numbers are the same)."""
    sg, se = got["_stride"], exp["_stride"]
    for u in units:
        rows = range(per * u, per * u + per)
        for k in ("n_combinations", "strands_valid", "pair_mapq"):
            assert got[k][u] == exp[k][u], (label, u, k, got[k][u], exp[k][u])
        assert np.isclose(got["pair_ll"][u], exp["pair_ll"][u], rtol=1e-12, atol=0), (label, u, "pair_ll")
        for r in rows:
            for k in ("best_chain", "n_cols", "mate_mapq"):
                assert got[k][r] == exp[k][r], (label, u, k, got[k][r], exp[k][r])
            n = int(exp["n_cols"][r])
            for k in rp.PAIR_COLS:
                assert np.array_equal(got[k][r * sg:r * sg + n], exp[k][r * se:r * se + n]), (label, u, k)


@pytest.mark.parametrize("name", list(GPU_FAMILIES))
def test_pairing_at_capacity_edges(pkg, oracle, name):
    f = GPU_FAMILIES[name]()
    b = f["batch"]; n = b["n_pairs"]; per = 1 if f.get("unpaired") else 2
    refused = set(f["refused"])
    ctx = _context(pkg, f)
    # fused
    gb = _batch(ctx, f, b); gb.align()
    fused = gb.pairs(); wcf = gb.work_counters(); ext = gb.chains(1); st = gb.stats()
    # stage by stage, the pairing stage twice
    gs = _batch(ctx, f, b); gs.project(); gs.extend(); gs.pair()
    staged = gs.pairs(); wcs = gs.work_counters()
    gs.pair()
    again = gs.pairs(); wca = gs.work_counters()
    _equal_runs(fused, staged, name + ": fused / staged"); _equal_runs(staged, again, name + ": pairing stage called again")
    assert np.array_equal(wcs[WC_PAIR_MULTI:WC_PAIR_MULTI + 4], wca[WC_PAIR_MULTI:WC_PAIR_MULTI + 4]), "list counters after the second call"
    # the records kept, the pairs refused
    seeds = gb.chains(0)
    if f["kept"] is not None:          # (a flagged record is not a kept one: the reads of the pairs refused for a flagged record are left out)
        reads = [r for u in range(n) if u not in f["oracle_fails"] for r in range(per * u, per * u + per)]
        assert np.array_equal(pe.kept_counts(b, seeds["status"], per)[reads], f["kept"][reads])
    got_refused = {u for u in range(n) if fused["pair_status"][u] != 0}
    assert got_refused == refused, (name, sorted(got_refused), sorted(refused))
    # the exact reference on the library's own extended chains (with the library's capacities: no answer for the refused pairs)
    units = pr.batch_units(b, ext, f["world"]["contigs"], b["insert_mean"], b["insert_sd"], unpaired=per == 1)
    assert set(pe.refused_by_capacity(units)) == refused
    s = pe.check_units(units, fused, name, per, refused=refused)
    pe.check_floors(s, f["floors"], name)
    assert s["refused"] == len(refused)
    # hlala_batch_get_stats: n_errors counts flagged chains, not pairs refused for a capacity alone
    flagged = int((seeds["status"][:b["n_chains"]] < 0).sum() + ((ext["status"][:b["n_chains"]] < 0) & (seeds["status"][:b["n_chains"]] >= 0)).sum())
    assert st.n_errors == flagged, (name, st.n_errors, flagged)
    assert flagged == {"records-error": 1, "too-long": 5}.get(name, 0), (name, flagged)
    # the oracle (without the pairs it cannot be given, which are the last ones)
    bo, exp = pe.oracle_answers(oracle, f)
    _against_oracle(fused, exp["pairs"], [u for u in range(bo["n_pairs"]) if u not in refused], per, name)
    # which kernel took which pair
    longest = [max([int(ext["n_cols"][c]) for r in range(per * u, per * u + per) for c in range(b["chain_off"][r], b["chain_off"][r + 1]) if ext["status"][c] == 0] or [0])
               for u in range(n)]
    kept_now = pe.kept_counts(b, seeds["status"], per)
    c0, c1 = pe.expected_classes(kept_now if per == 2 else np.stack([kept_now, np.ones_like(kept_now)], 1), longest, refused)
    print("%s: class 0 %d pairs, class 1 %d; fused lists main %s side %s" % (name, c0, c1, wcf[WC_PAIR_MULTI:WC_PAIR_MULTI + 4:2].tolist(), wcf[WC_PAIR_MULTI + 4:WC_PAIR_MULTI + 8:2].tolist()))
    assert (wcs[WC_PAIR_MULTI], wcs[WC_PAIR_MULTI + 2]) == (c0, c1) and (wcs[WC_PAIR_MULTI + 1] >= c0 and wcs[WC_PAIR_MULTI + 3] >= c1)
    assert (wcf[WC_PAIR_MULTI] + wcf[WC_PAIR_MULTI + 4], wcf[WC_PAIR_MULTI + 2] + wcf[WC_PAIR_MULTI + 6]) == (c0, c1)
    # ... pair by pair, as the totals above count them: 128 combinations in class 0, 129 in class 1; chains of 192 columns in class 0, of 193 in class 1
    cls = [None if u in refused or k[0] * k[1] <= 1 else pe.expected_classes(np.asarray([k]), [longest[u]]).index(1)
           for u, k in enumerate((kept_now.reshape(-1, 2) if per == 2 else np.stack([kept_now, np.ones_like(kept_now)], 1)).tolist())]
    assert (cls.count(0), cls.count(1)) == (c0, c1)
    if name == "counts":
        assert c0 >= 8 and c1 >= 5          # both k_pair_multi instances
        k = f["kept"].reshape(-1, 2).tolist()
        assert [cls[k.index(x)] for x in ([64, 2], [8, 16], [16, 8], [63, 2], [43, 3], [33, 31], [64, 16])] == [0, 0, 0, 0, 1, 1, 1]
    if name == "columns":
        assert c1 >= 6 and all(cls[u] == (0 if longest[u] <= 192 else 1) for u in range(n)) and {192, 193} <= set(longest)
        assert {cls[u] for u in range(n) if longest[u] == 192} == {0} and {cls[u] for u in range(n) if longest[u] == 193} == {1}
    if name.startswith("draws"):
        i = pe.DRAW_SIZES.index(n)
        assert (c0, c1) == ((1, 1, 3, 4, 4, 5)[i], (0, 1, 3, 3, 4, 5)[i])
    if name == "fan":
        # the pairs whose extension runs through the fan wait for the side-stream DP classes: the second pass has its own lists and combination scratch
        assert wcf[WC_PAIR_MULTI + 4] >= 1 and wcf[WC_PAIR_MULTI + 4 + 2] >= 1, "no fan pair was deferred to the second pairing pass"
    # the batch without its refused last pairs: the others come out the same
    if refused and sorted(refused) == list(range(n - len(refused), n)):
        bw = pe.without(f, sorted(refused))
        gw = _batch(ctx, f, bw); gw.align(); alone = gw.pairs()
        sg = fused["_stride"]; m = bw["n_pairs"]
        for k in SCALARS:
            cnt = m * (per if len(fused[k]) >= per * n and k in ("best_chain", "n_cols", "mate_mapq") else 1)
            assert np.array_equal(fused[k][:cnt], alone[k][:cnt]), (name, "with / without the refused pairs", k)
        for k in rp.PAIR_COLS:
            assert np.array_equal(fused[k][:per * m * sg], alone[k][:per * m * sg]), (name, "with / without the refused pairs", k)
        gw.close()
    gb.close(); gs.close(); ctx.close()
