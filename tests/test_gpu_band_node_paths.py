"""GPU: band-kernel calls listed by the PATH of their start node (FlatGraph::npf_* / npb_*, kernel_dp_band.hip) against the oracle, as
test_gpu_align.py::test_band_kernel_and_its_fail_over_are_bit_exact does for the level rule: columns, DP scores, iteration / cell / edge counters are the same
whichever kernel ran a call -- node paths (default), the level rule (HLALA_DP_BAND_NODES=0), no band kernel (HLALA_DP_BAND=0), forced fail-overs (HLALA_DP_BAND_RISKY=1)."""
import numpy as np
import pytest

from tools import synth
from util import compare_chains
from test_gpu_align import assert_pairs_equal

pytestmark = pytest.mark.gpu

ENVS = [dict(), dict(HLALA_DP_BAND_NODES="0"), dict(HLALA_DP_BAND="0"), dict(HLALA_DP_BAND_RISKY="1")]
ENV_IDS = ["default", "nodes-off", "band-off", "band-risky"]

_CACHE = {}          # world name -> (world, batch, oracle result): computed once, shared by the settings, never changed
_LISTS = {}          # bubble world -> band calls [direction][instantiation] of the default setting
_SEEN = {}         # world name -> {setting: (n_edges_touched, n_dp_band, n_dp_band_failed, new-call counter, tied counter)}


def _world(name, oracle):
    if name not in _CACHE:
        if name == "graph_m":
            w = synth.make_world_m(seed=7, n_levels=60_000, n_windows=3, alleles=(400, 3000)); b = synth.make_batch_m(w, 1500, seed=21, frac_gene=1.0)
        elif name == "bubbles-k1":
            w = synth.make_world(seed=61, G=9000, k=1, mut_density=0.01); b = synth.make_batch(w, 400, seed=71, clip_max=48, p_no_clip=0.0)
        else:
            w = synth.make_world(seed=62, G=9000, k=2, mut_density=0.01); b = synth.make_batch(w, 400, seed=72, clip_max=48, p_no_clip=0.0)
        exp = oracle(w["graph"], w["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=777, max_columns=384).align_batch(b)
        _CACHE[name] = (w, b, exp)
    return _CACHE[name]


def _run(pkg, oracle, name, env_id):
    w, b, exp = _world(name, oracle)
    ctx = pkg.Context(w["graph"], w["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=777, max_columns=384)
    gb = ctx.batch(b); gb.align()
    compare_chains(gb.chains(1), exp["ext"], b["n_chains"], label="stage B (%s, %s)" % (name, env_id))
    assert_pairs_equal(gb.pairs(), exp["pairs"])
    st = gb.stats(); wc = gb.work_counters()
    assert st.n_errors == 0
    assert (st.n_dp_calls, st.n_dp_iterations, st.n_dp_cells) == tuple(int(x) for x in exp["stats"][:3])
    seen = _SEEN.setdefault(name, {})
    seen[env_id] = (int(st.n_edges_touched), int(st.n_dp_band), int(st.n_dp_band_failed), int(wc[pkg.DEBUG_WC_BAND_NODES]), int(wc[pkg.DEBUG_WC_BAND_TIED]))
    print("%s / %s: DP calls %d, band %d (failed over %d), listed through a node path only %d, tied end cells %d, edges %d" % ((name, env_id, st.n_dp_calls) + seen[env_id][1:] + seen[env_id][:1]))
    assert len({v[0] for v in seen.values()}) == 1, seen          # n_edges_touched: the same number whichever kernels ran the calls
    return gb, st, wc, seen


@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_small_graph_m_world(pkg, oracle, monkeypatch, env):
    """Gene-window reads of a small Graph M world: levels of tens to hundreds of nodes, most nodes with one successor.  The CPU census of exactly this input
    (tools/dp_node_path_census.py --test-world) gives 328 level-linear calls, 1 487 node-linear ones beyond them, 1 405 of those contiguous in the path order."""
    env_id = ENV_IDS[ENVS.index(env)]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gb, st, wc, seen = _run(pkg, oracle, "graph_m", env_id)
    new = int(wc[pkg.DEBUG_WC_BAND_NODES])
    if env_id == "default":
        assert new > 0
        assert st.n_dp_band_failed <= 0.01 * st.n_dp_band
    elif env_id == "nodes-off":
        assert new == 0 and st.n_dp_band > 0
    elif env_id == "band-off":
        assert st.n_dp_band == 0 and new == 0
    else:
        assert st.n_dp_band_failed > 0
    if "default" in seen and "nodes-off" in seen:
        assert seen["default"][1] >= 2 * seen["nodes-off"][1], seen          # the census says about 5 x; 2 leaves room for call sharing and the contiguity rule
    if "default" in seen and "band-risky" in seen:
        assert seen["default"][4] > 0 or seen["band-risky"][4] > 0, seen     # an end cell drawn among tied ones, with node paths on


@pytest.mark.parametrize("name", ["bubbles-k1", "bubbles-k2"])
@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_bubble_worlds(pkg, oracle, monkeypatch, env, name):
    """Bubbles of two nodes over one / two levels every hundred levels, clips up to 48 bases: calls that start on or beside a bubble node whose path is unary."""
    env_id = ENV_IDS[ENVS.index(env)]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gb, st, wc, seen = _run(pkg, oracle, name, env_id)
    if env_id == "default":
        items, _ = gb.dp_items(); n = len(items) // 2
        # band calls by direction (left, right extensions) and instantiation (16, 32, 64 lanes): every instantiation and both directions in either world, all
        # six lists over the two (a 64-lane call needs up to 96 unary steps ahead, which a bubble every hundred levels rarely leaves: the k = 1 batch has none leftwards)
        cnt = np.array([[int(((part[part[:, 0] >= 0][:, 6] & 255) == c).sum()) for c in (2, 3, 4)] for part in (items[:n], items[n:])])
        print("%s: band calls by direction and instantiation %s" % (name, cnt.tolist()))
        assert (cnt.sum(0) > 0).all() and (cnt.sum(1) > 0).all(), (name, cnt)
        _LISTS[name] = cnt
        if len(_LISTS) == 2:
            assert (sum(_LISTS.values()) > 0).all(), _LISTS
        assert int(wc[pkg.DEBUG_WC_BAND_NODES]) > 0
    if env_id == "band-off":
        assert st.n_dp_band == 0


# ---- hand-built graphs: level 0 holds a root, levels 1 .. M three nodes (tracks 0, 1, 2), level M + 1 a sink
def _tracks(M, rng_seed=5, extra=(), par=(), redirect=()):
    """Track k's node of level i (1 .. M) has one edge to track k's node of level i + 1 (to the sink from level M), label lab[k][i]; the root one edge to every track.
    extra: (k, i, k2, label) a further edge track k level i -> track k2 level i + 1; par: (k, i, label) a further parallel edge along track k;
    redirect: (k, i, k2) the track edge of track k at level i ends in track k2.  Returns the graph, node(k, i), edge(k, i) and the labels."""
    K = 3
    rng = np.random.default_rng(rng_seed)
    lab = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=(K, M + 1))
    node = lambda k, i: 1 + (i - 1) * K + k
    sink = 1 + M * K
    nl = [0] + [i for i in range(1, M + 1) for _ in range(K)] + [M + 1]
    ef, et, el, eid = [], [], [], {}
    for k in range(K):
        ef.append(0); et.append(node(k, 1)); el.append(int(lab[k][0]))
    red = {(k, i): k2 for k, i, k2 in redirect}
    for i in range(1, M + 1):
        for k in range(K):
            eid[(k, i)] = len(ef)
            ef.append(node(k, i)); et.append(sink if i == M else node(red.get((k, i), k), i + 1)); el.append(int(lab[k][i]))
    for k, i, k2, c in extra:
        ef.append(node(k, i)); et.append(node(k2, i + 1)); el.append(ord(c))
    for k, i, c in par:
        eid[(k, i, c)] = len(ef)
        ef.append(node(k, i)); et.append(sink if i == M else node(k, i + 1)); el.append(ord(c))
    g = dict(n_levels=M + 2, n_nodes=len(nl), n_edges=len(ef), node_level=np.asarray(nl, np.int32), edge_from=np.asarray(ef, np.int32), edge_to=np.asarray(et, np.int32),
             edge_label=np.asarray(el, np.uint8))
    return g, node, eid, lab


def _seed_on_track(lab, eid, k, lv0, n, left, right):
    """A seed chain over the n track edges that leave levels lv0 .. lv0 + n - 1 of track k; `left` / `right`: the clipped read bases before / behind it (bytes)."""
    core = bytes(int(lab[k][i]) for i in range(lv0, lv0 + n))
    read = left + core + right
    return dict(n_reads=1, read_off=np.array([0, len(read)], np.int32), read_bases=np.frombuffer(read, np.uint8), read_quals=np.full(len(read), 33 + 30, np.uint8),
                n_chains=1, chain_read=np.array([0], np.int32), chain_seq_begin=np.array([len(left)], np.int32), chain_seq_end=np.array([len(left) + n - 1], np.int32),
                chain_reverse=np.array([0], np.uint8), col_off=np.array([0, n], np.int32), col_level=np.arange(lv0, lv0 + n, dtype=np.int32),
                col_edge=np.asarray([eid[(k, i)] for i in range(lv0, lv0 + n)], np.int32), col_gchar=np.frombuffer(core, np.uint8), col_schar=np.frombuffer(core, np.uint8))


def _other(c):
    return b"C" if c == ord("A") else b"A"


def _extend(pkg, oracle, graph, seeds, label):
    exp = oracle(graph, None).extend_seeds(seeds)
    ctx = pkg.Context(graph, None)
    gb = ctx.batch_from_seeds(seeds); gb.extend()
    got = gb.chains(1)
    compare_chains(got, exp, 1, label=label)
    st = gb.stats(); wc = gb.work_counters()
    assert st.n_errors == 0 and st.n_dp_calls == 1
    return got, exp, st, wc


X0, JM, NEED = 10, 3, 20          # start level of the forward cases, read bases left, steps a call of 3 bases needs: 3 + 8 + min(3 + 6, 40)


def _right_clip(lab, k=0, x0=X0):
    """Two matching bases and a mismatch behind the seed."""
    return bytes([int(lab[k][x0]), int(lab[k][x0 + 1])]) + _other(int(lab[k][x0 + 2]))


def test_hand_start_node_on_a_three_node_level_with_exactly_the_steps_it_needs(pkg, oracle):
    # track 0 branches at level X0 + NEED: its node there is not unary, the start node has exactly NEED steps
    g, node, eid, lab = _tracks(40, extra=[(0, X0 + NEED, 1, "A")])
    s = _seed_on_track(lab, eid, 0, 4, X0 - 4, b"", _right_clip(lab))
    got, exp, st, wc = _extend(pkg, oracle, g, s, "exactly need")
    assert st.n_dp_band == 1 and st.n_dp_band_failed == 0 and int(wc[pkg.DEBUG_WC_BAND_NODES]) == 1
    assert int(exp["dp_score"][1]) == 2 + 2 - 5


def test_hand_one_step_short_is_not_listed(pkg, oracle):
    g, node, eid, lab = _tracks(40, extra=[(0, X0 + NEED - 1, 1, "A")])
    s = _seed_on_track(lab, eid, 0, 4, X0 - 4, b"", _right_clip(lab))
    got, exp, st, wc = _extend(pkg, oracle, g, s, "need - 1")
    assert st.n_dp_band == 0 and int(wc[pkg.DEBUG_WC_BAND_NODES]) == 0
    # ... and the hashed class gives what the band kernel gives one step further on (the branch is beyond what the call reaches)
    g2, _, eid2, lab2 = _tracks(40, extra=[(0, X0 + NEED, 1, "A")])
    got2, _, st2, _ = _extend(pkg, oracle, g2, _seed_on_track(lab2, eid2, 0, 4, X0 - 4, b"", _right_clip(lab2)), "need")
    assert st2.n_dp_band == 1
    n = int(got["n_cols"][0])
    assert n == int(got2["n_cols"][0]) and np.array_equal(got["col_level"][:n], got2["col_level"][:n]) and np.array_equal(got["col_edge"][:n], got2["col_edge"][:n])
    assert np.array_equal(got["dp_score"][:2], got2["dp_score"][:2]) and np.array_equal(got["dp_iters"][:2], got2["dp_iters"][:2])


def test_hand_path_entered_from_a_non_primary_predecessor(pkg, oracle):
    # track 1's node of level X0 leads into track 0, whose node of level X0 + 1 has the smaller-numbered track 0 node as primary predecessor: the start node's
    # path is not contiguous in storage (one step), although what it reaches is a path
    g, node, eid, lab = _tracks(40, redirect=[(1, X0, 0)], extra=[(2, X0, 1, "A")])
    right = bytes([int(lab[1][X0]), int(lab[0][X0 + 1])]) + _other(int(lab[0][X0 + 2]))
    s = _seed_on_track(lab, eid, 1, 4, X0 - 4, b"", right)
    got, exp, st, wc = _extend(pkg, oracle, g, s, "non-primary predecessor")
    assert st.n_dp_band == 0 and int(wc[pkg.DEBUG_WC_BAND_NODES]) == 0
    n = int(got["n_cols"][0])
    assert n == X0 - 4 + 3 and int(got["col_edge"][X0 - 4]) == eid[(1, X0)] and int(got["col_edge"][X0 - 3]) == eid[(0, X0 + 1)]


def test_hand_second_of_three_parallel_edges(pkg, oracle):
    # the first step of the path has three parallel edges in creation order (track label, then two more); the read base matches the second
    g0, _, _, lab0 = _tracks(40)
    first = int(lab0[0][X0]); others = [c for c in b"ACGT" if c != first]
    g, node, eid, lab = _tracks(40, par=[(0, X0, chr(others[0])), (0, X0, chr(others[1]))])
    right = bytes([others[0], int(lab[0][X0 + 1]), int(lab[0][X0 + 2])])
    s = _seed_on_track(lab, eid, 0, 4, X0 - 4, b"", right)
    got, exp, st, wc = _extend(pkg, oracle, g, s, "parallel edges")
    assert st.n_dp_band == 1 and int(wc[pkg.DEBUG_WC_BAND_NODES]) == 1
    n = int(got["n_cols"][0]); col = X0 - 4                                  # the first column behind the seed
    assert n == X0 - 4 + 3 and int(got["col_edge"][col]) == eid[(0, X0, chr(others[0]))] and int(got["col_gchar"][col]) == others[0] and int(got["col_level"][col]) == X0


def test_hand_path_that_ends_in_a_branch_inside_the_reach_fails_over(pkg, oracle, monkeypatch):
    # RISKY lists the call as soon as the steps cover its 3 bases; the cell of the third match survives on the step past the run: fail-over to the hashed class
    monkeypatch.setenv("HLALA_DP_BAND_RISKY", "1")
    g, node, eid, lab = _tracks(40, extra=[(0, X0 + JM, 1, "A")])
    right = bytes(int(lab[0][X0 + t]) for t in range(JM))
    s = _seed_on_track(lab, eid, 0, 4, X0 - 4, b"", right)
    got, exp, st, wc = _extend(pkg, oracle, g, s, "risky fail-over")
    assert st.n_dp_band == 1 and st.n_dp_band_failed == 1 and int(wc[pkg.DEBUG_WC_BAND_WHY + 3]) == 1


def test_hand_backward_call_on_a_unary_in_path_whose_out_edges_branch(pkg, oracle):
    # every node of track 0 has a second out-edge into track 1 (not unary forward) and one in-edge (unary backward): a left extension from level 28 is a band call
    M, x0 = 40, 28
    g, node, eid, lab = _tracks(M, extra=[(0, i, 1, "ACGT"[i % 4]) for i in range(1, M)])
    left = _other(int(lab[0][x0 - 3])) + bytes([int(lab[0][x0 - 2]), int(lab[0][x0 - 1])])
    s = _seed_on_track(lab, eid, 0, x0, 6, left, b"")
    got, exp, st, wc = _extend(pkg, oracle, g, s, "backward")
    assert st.n_dp_band == 1 and st.n_dp_band_failed == 0 and int(wc[pkg.DEBUG_WC_BAND_NODES]) == 1
    assert int(got["col_level"][0]) == x0 - 3
    # the same read forward from that node is not a band call: two successors
    s2 = _seed_on_track(lab, eid, 0, 4, X0 - 4, b"", _right_clip(lab))
    _, _, st2, _ = _extend(pkg, oracle, g, s2, "forward over branching out-edges")
    assert st2.n_dp_band == 0


def test_hand_path_that_reaches_the_last_level(pkg, oracle):
    # the sink is exactly NEED steps from the start node: the staged labels end with the graph
    M = X0 + NEED - 1
    g, node, eid, lab = _tracks(M)
    s = _seed_on_track(lab, eid, 0, 4, X0 - 4, b"", _right_clip(lab))
    got, exp, st, wc = _extend(pkg, oracle, g, s, "last level")
    assert st.n_dp_band == 1 and st.n_dp_band_failed == 0 and int(wc[pkg.DEBUG_WC_BAND_NODES]) == 1
