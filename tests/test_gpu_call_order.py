"""The order of the pair table made on the device (hla-la_amd/csrc/kernel_callorder.hip; hlala_pair_order_gpu, hlala_set_call_order_gpu) against std::sort +
std::reverse on the host, index for index, on the cases of tests/call_order_cases.py; its counters against the host model's; and hlala_call_locus /
hlala_type_locus with the switch on against the same calls with the switch off."""
import numpy as np
import pytest

import call_order_cases as K

pytestmark = pytest.mark.gpu
CALL_KEYS = ("first_cluster", "second_cluster", "first_marginal", "second_p", "ll_max", "max_pair", "n_sort_ties")
MODEL_COUNTS = ("path", "levels", "tile_ranges", "largest_tile", "heap_sorts", "largest_heap")


@pytest.fixture(scope="module")
def ctx(pkg):
    from tools import synth
    w = synth.make_world(seed=1, G=300, k=1)
    return pkg.Context(w["graph"], w["contigs"])


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


@pytest.mark.parametrize("k", range(len(K.cases())), ids=[c[0] for c in K.cases()])
def test_pair_order_matches_reference(pkg, ctx, k):
    name, ll, ma = K.cases()[k]
    order, counts = ctx.pair_order_gpu(ll, ma)
    assert np.array_equal(order, K.references()[name]), name
    model = pkg.host_pair_order_model(ll, ma)[1]
    for key in MODEL_COUNTS:
        assert counts[key] == model[key], (name, key, counts, model)
    assert counts == ctx.call_order_counts()
    assert counts["bytes_up"] == 16 * len(ll) and counts["bytes_down"] >= 4 * len(ll)


def test_heap_branch_ran_on_the_device(pkg, ctx):
    ll, ma = K.organ_pipe(16384)
    counts = ctx.pair_order_gpu(ll, ma)[1]
    assert counts["heap_sorts"] > 0 and 16 < counts["largest_heap"] <= K.H and counts["path"] == pkg.CALL_ORDER_DEVICE


def test_refusals_write_nothing(pkg, ctx):
    ll, ma = K.organ_pipe(K.REFUSED_N)
    model = pkg.host_pair_order_model(ll, ma)[1]
    rc, text, order, counts = ctx.pair_order_gpu(ll, ma, raw=True)
    assert rc == K.E_CAPACITY and text.startswith("not available:") and (order == -7).all(), (rc, text)
    assert str(K.REFUSED_N) in text and str(model["largest_heap"]) in text and model["largest_heap"] > K.H, text
    assert counts["path"] == pkg.CALL_ORDER_REFUSED_HEAP == model["path"]
    for key in ("levels", "largest_heap"):
        assert counts[key] == model[key], (key, counts, model)
    assert 1 <= counts["heap_sorts"] <= model["heap_sorts"]         # (a refusing call runs no tile: it counts the ranges beyond the cap alone)
    ll = np.arange(5000, dtype=np.float64); ma = np.ones(5000); ll[4321] = np.nan
    rc, text, order, counts = ctx.pair_order_gpu(ll, ma, raw=True)
    assert rc == K.E_CAPACITY and text.startswith("not available:") and "NaN" in text and (order == -7).all(), (rc, text)
    assert counts["path"] == pkg.CALL_ORDER_REFUSED_NAN
    rc, text, order, counts = ctx.pair_order_gpu(np.zeros(0), np.zeros(0), raw=True)
    assert rc == K.E_ARG
    # ... and the context goes on
    name, ll, ma = K.cases()[-1]
    assert np.array_equal(ctx.pair_order_gpu(ll, ma)[0], K.references()[name])


@pytest.mark.parametrize("Cn", [120, 200])
def test_call_locus_with_the_switch(pkg, ctx, Cn):
    ll, ma, mm = K.locus_table(Cn)
    ctx.set_call_order_gpu(False)
    off = ctx.call_locus(ll, ma, mm); c_off = ctx.call_order_counts()
    ctx.set_call_order_gpu(True)
    try:
        on = ctx.call_locus(ll, ma, mm); c_on = ctx.call_order_counts()
    finally:
        ctx.set_call_order_gpu(False)
    assert c_off["path"] == pkg.CALL_ORDER_HOST and c_off["levels"] == 0 and c_off["bytes_up"] == 4 * len(ll)
    assert c_on["path"] == pkg.CALL_ORDER_DEVICE and c_on["levels"] > 0 and c_on["bytes_up"] == 0
    assert off["n_sort_ties"] > 0 and np.array_equal(on["order"], off["order"]) and np.array_equal(off["order"], K.references()[f"locus-C{Cn}"])
    for key in ("p_normalized", "cluster_marginal"):
        assert bits(on[key]) == bits(off[key]), key
    for key in CALL_KEYS:
        assert bits(np.float64(on[key])) == bits(np.float64(off[key])), key


@pytest.mark.parametrize("Cn", [120, 200])
def test_type_locus_with_the_switch(pkg, ctx, Cn):
    from tools import synth
    loc = synth.make_locus(seed=Cn, n_clusters=Cn, n_reads=40)
    seq = loc["cluster_seq"].reshape(Cn, -1)
    for a, b in K.LOCUS_DUP[Cn]:
        seq[a] = seq[b]
    ctx.set_call_order_gpu(False)
    off = ctx.type_locus(loc); c_off = ctx.call_order_counts()
    ctx.set_call_order_gpu(True)
    try:
        on = ctx.type_locus(loc); c_on = ctx.call_order_counts()
    finally:
        ctx.set_call_order_gpu(False)
    assert c_off["path"] == pkg.CALL_ORDER_HOST and c_on["path"] == pkg.CALL_ORDER_DEVICE and c_on["levels"] > 0
    assert off["n_sort_ties"] > 0 and np.array_equal(on["order"], off["order"])
    assert np.array_equal(off["order"], pkg.host_pair_order_reference(off["pairLL"], off["misAvg"]))
    for key in ("LL", "mism", "pairLL", "misAvg", "misMin", "p_normalized", "cluster_marginal"):
        assert bits(on[key]) == bits(off[key]), key
    for key in CALL_KEYS:
        assert bits(np.float64(on[key])) == bits(np.float64(off[key])), key


def test_refused_table_takes_the_host_path(pkg, ctx):
    Cn = K.REFUSED_C
    ll, ma = K.organ_pipe(Cn * (Cn + 1) // 2)
    mm = np.floor(ma / 2)
    ctx.set_call_order_gpu(False)
    off = ctx.call_locus(ll, ma, mm)
    ctx.set_call_order_gpu(True)
    try:
        on = ctx.call_locus(ll, ma, mm); c_on = ctx.call_order_counts()           # HLALA_OK: call_locus raises otherwise
    finally:
        ctx.set_call_order_gpu(False)
    assert c_on["path"] == pkg.CALL_ORDER_REFUSED_HEAP and c_on["largest_heap"] > K.H and c_on["bytes_up"] == 4 * len(ll), c_on
    assert np.array_equal(on["order"], off["order"]) and np.array_equal(on["order"], pkg.host_pair_order_reference(ll, ma))
    for key in ("p_normalized", "cluster_marginal"):
        assert bits(on[key]) == bits(off[key]), key
