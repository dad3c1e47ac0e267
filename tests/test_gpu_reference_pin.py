"""GPU: the extension DP and the chain scoring of the product against fixtures written by the REFERENCE's own aligner.

tests/golden/ref_*.npz hold seed chains and what mapper::aligner::extensionAligner (extendSeedChain + scoreOneAlignment, built from the
reference's sources by oracle/ref/) makes of them under the product's seed discipline -- see tests/golden/make_ref_golden.py.  Here
hlala_batch_create_from_seeds + hlala_extend_chains face those files directly, with no oracle in between and no chain left out:
status, n_cols, seq_begin, seq_end, levels, edges, both character rows and col_fromseed exact; ll within rtol = 1e-12 (the project's
bar for this quantity).  Once in the default configuration and once with the band kernel off (HLALA_DP_BAND=0), so that both DP
families face the reference; over the fixtures the band kernel, the first class and at least one class from index 3 up ran calls.

Reads tests/golden/ only: neither the reference nor anything built from it is needed on the GPU machine."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("ref_linear.npz", "ref_k10.npz", "ref_k0ties.npz", "ref_fan.npz", "ref_graphm.npz")


def load(name):
    z = np.load(os.path.join(HERE, "golden", name))
    d = dict(graph={}, seeds={}, exp={}, meta={})
    for k in z.files:
        sec, key = k.split("__", 1)
        v = z[k]
        d[sec][key] = v.item() if v.shape == () else v
    return d


def compare_with_fixture(got, exp, n, stride, label):
    """Every chain, every output the reference writes."""
    bad = []
    for k in ("status", "n_cols", "seq_begin", "seq_end"):
        for c in np.nonzero(got[k][:n] != exp[k])[0]:
            bad.append((int(c), k, int(got[k][c]), int(exp[k][c])))
    off = np.concatenate([[0], np.cumsum(exp["n_cols"])])
    for c in range(n):
        m = int(exp["n_cols"][c])
        for k in ("col_level", "col_edge", "col_gchar", "col_schar", "col_fromseed"):
            a, b = got[k][c * stride:c * stride + m], exp[k][off[c]:off[c + 1]]
            if not np.array_equal(a, b):
                j = int(np.nonzero(a != b)[0][0])
                bad.append((c, k, "first differing column %d: %d, reference %d" % (j, int(a[j]), int(b[j]))))
    ll_differ = int((got["ll"][:n] != exp["ll"]).sum())
    err = np.abs(got["ll"][:n] - exp["ll"]) / np.maximum(1.0, np.abs(exp["ll"]))
    print("%s: %d chains, %d columns, ll differs at all in %d chains, largest relative difference %.3g" % (label, n, int(off[-1]), ll_differ, float(err.max()) if n else 0.0))
    assert not bad, "%s: %d mismatches against the reference, first: %s" % (label, len(bad), bad[:3])
    assert np.all(err <= 1e-12), "%s: ll of chains %s" % (label, np.nonzero(err > 1e-12)[0][:5].tolist())


@pytest.mark.parametrize("env", [dict(), dict(HLALA_DP_BAND="0")], ids=["default", "band-off"])
def test_extension_matches_reference_fixtures(pkg, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n_band = 0
    n_class = np.zeros(7, np.int64)
    n_chains = 0
    for name in FIXTURES:
        f = load(name)
        stride = int(f["meta"]["max_columns"])
        ctx = pkg.Context(f["graph"], None, rng_seed=int(f["meta"]["rng_seed"]), max_columns=stride)
        gb = ctx.batch_from_seeds(f["seeds"])
        gb.extend()
        n = int(f["seeds"]["n_chains"])
        assert n == len(f["exp"]["n_cols"]) and n > 50
        compare_with_fixture(gb.chains(1), f["exp"], n, stride, "%s (%s)" % (name, ", ".join("%s=%s" % kv for kv in env.items()) or "default"))
        st = gb.stats()
        assert st.n_errors == 0
        print("%s: DP calls %d, band %d (failed over %d), by class %s" % (name, st.n_dp_calls, st.n_dp_band, st.n_dp_band_failed, list(st.n_dp_class)))
        n_band += st.n_dp_band; n_class += np.array(list(st.n_dp_class), np.int64); n_chains += n
        gb.close(); ctx.close()
    # both DP families and the wide end of the frontier classes faced the reference
    if env.get("HLALA_DP_BAND") == "0":
        assert n_band == 0
    else:
        assert n_band > 0
    assert n_class[0] > 0 and n_class[3:].sum() > 0, "DP calls by class over the fixtures: %s" % n_class.tolist()
    assert n_chains > 500
