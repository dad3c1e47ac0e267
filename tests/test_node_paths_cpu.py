"""CPU: the node-path arrays of the flatten (FlatGraph::npf_* / npb_*: what decides which extension-DP calls the band kernels take, and what they stage from) against a
definition written down independently in numpy (tools/dp_node_path_census.py): unary nodes, primary predecessors, the path order and the steps along it, in both
directions."""
import numpy as np
import pytest

from tools import synth
from tools import dp_node_path_census as npc


def _hand_graph():
    """Levels 0 .. 7, one backbone node per level (creation indices 0 .. 7) with single edges 'A', plus: level 2 -> 3 through FIVE parallel edges; a '_' edge beside
    the real edge 4 -> 5; a second node on level 6 (creation index 8) entered from node 5, leaving to node 7."""
    nl = list(range(8)) + [6]
    ef, et, lab = [], [], []
    for i in range(7):
        ef.append(i); et.append(i + 1); lab.append(ord("A"))
    for c in "CGTN":
        ef.append(2); et.append(3); lab.append(ord(c))
    ef.append(4); et.append(5); lab.append(ord("_"))
    ef += [5, 8]; et += [8, 7]; lab += [ord("C"), ord("G")]
    return dict(n_levels=8, n_nodes=9, n_edges=len(ef), node_level=np.asarray(nl, np.int32), edge_from=np.asarray(ef, np.int32), edge_to=np.asarray(et, np.int32),
                edge_label=np.asarray(lab, np.uint8))


WORLDS = {"k1": lambda: synth.make_world(seed=31, G=9000, k=1),
          "k2-bubbles": lambda: synth.make_world(seed=37, G=9000, k=2, mut_density=0.01),
          "fan-320-edges-150-jumps": lambda: synth.make_fan_world(),
          "graph_m": lambda: synth.make_world_m(seed=7, n_levels=60_000, n_windows=3, alleles=(400, 3000)),
          "hand": lambda: dict(graph=_hand_graph(), contigs=None)}


@pytest.mark.parametrize("kind", list(WORLDS))
def test_node_paths_match_their_definition(pkg, kind):
    w = WORLDS[kind]()
    gd = w["graph"]; N = gd["n_nodes"]
    H = npc.HostFlatten(pkg, gd, w["contigs"])
    assert H.F, H.error
    jumps = H.jump_nodes(); lin = H.linear(); new, order = npc.new_ids(gd)
    level = gd["node_level"][order].astype(np.int64); level_off = np.concatenate([[0], np.cumsum(np.bincount(level, minlength=gd["n_levels"]))])
    n_unary = 0
    for forward in (True, False):
        m = npc.node_path_model(gd, jumps[0 if forward else 1], forward)
        P = H.node_paths(forward)
        pos = P["pos"].astype(np.int64); node = P["node"].astype(np.int64); steps = P["steps"].astype(np.int64)
        # positions are a permutation, node is its inverse
        assert np.array_equal(np.sort(pos), np.arange(N)) and np.array_equal(node[pos], np.arange(N))
        # pos(succ(u)) = pos(u) + 1 iff u is the primary predecessor of succ(u); chains start at the nodes without a unary predecessor, in node order
        u = np.nonzero(m["unary"])[0]
        assert np.array_equal(pos[m["succ"][u]] == pos[u] + 1, m["link"][u])
        heads = np.nonzero(m["prim"] < 0)[0]
        assert np.all(np.diff(pos[heads]) > 0)
        assert np.array_equal(pos, npc.path_order(m))
        # label word and first edge by position
        assert np.array_equal(P["label"], m["word"][node]) and np.array_equal(P["eid"], m["eid"][node])
        assert np.all((P["label"] != 0) == m["unary"][node])
        # steps: 0 off the unary nodes, else 1 + the next position's when the node is the primary of its successor, capped at 255
        nxt = np.concatenate([steps[1:], [0]])
        exp = np.where(m["unary"][node], np.minimum(255, 1 + np.where(m["link"][node], nxt, 0)), 0)
        assert np.array_equal(steps, exp)
        assert np.all(pos[u] + steps[pos[u]] <= N)                 # the kernel reads positions pos .. pos + steps - 1: inside the arrays
        # walking the staged positions is walking succ: `steps` unary nodes, each but the last the predecessor of the next position's node
        for t in range(1, 5):
            sel = np.nonzero(steps >= t)[0]
            assert m["unary"][node[sel + t - 1]].all()
            sel = np.nonzero(steps >= t + 1)[0]
            assert np.array_equal(node[sel + t], m["succ"][node[sel + t - 1]])
        # every level-linear run is covered by a node run at least as long
        run = (lin["out"] if forward else lin["inn"]).astype(np.int64)
        lv = np.nonzero(run > 0)[0]
        assert np.all(level_off[lv + 1] - level_off[lv] == 1)
        assert np.all(steps[pos[level_off[lv]]] >= run[lv])
        n_unary += int(m["unary"].sum())
        if kind == "fan-320-edges-150-jumps":
            # none of the nodes with hundreds of edges or with gap-path jumps is unary
            assert not m["unary"][m["deg"] > 4].any() and (m["deg"] >= 320).any()
            jn = new[jumps[0 if forward else 1]]
            assert len(jn) >= 150 and not m["unary"][jn].any() and np.all(steps[pos[jn]] == 0)
        if kind == "graph_m":
            # the gene windows: levels of many nodes, most of which still have one successor
            wide = (level_off[1:] - level_off[:-1])[level] >= 3
            assert wide.sum() > 1000 and m["unary"][wide].mean() > 0.5
            assert (steps == 255).any()                            # (and the cap is reached on the backbone)
        if kind == "k2-bubbles":
            two = (level_off[1:] - level_off[:-1])[level] == 2
            assert two.sum() > 50 and m["unary"][two].any()
        if kind == "hand":
            s = lambda c: int(steps[pos[new[c]]])
            if forward:
                assert s(2) == 0                                   # five parallel out-edges
                assert s(4) == 0                                   # a '_' out-edge
                assert s(5) == 0                                   # two successors
                assert (s(0), s(1), s(3)) == (2, 1, 1)
                assert s(6) == 1 and s(8) == 1 and s(7) == 0       # node 6 is the primary predecessor of 7, node 8 a second one: a run of its own
                assert pos[new[7]] == pos[new[6]] + 1 and pos[new[7]] != pos[new[8]] + 1
            else:
                assert s(3) == 0 and s(5) == 0 and s(7) == 0 and s(0) == 0
                assert (s(1), s(2), s(4)) == (1, 2, 1)
                assert s(6) == 1 and s(8) == 1                     # both entered from node 5 alone; 6 is the smaller: node 5 follows it in the backward order
                assert pos[new[5]] == pos[new[6]] + 1 and pos[new[5]] != pos[new[8]] + 1
    assert n_unary > 0
    H.close()


def test_an_edge_that_skips_a_level_never_reaches_the_node_paths(pkg):
    """A node whose edge ends two levels on is not unary by definition; the flatten refuses such a graph before any path is built (Graph.cpp: edges join
    consecutive levels), so no call can be listed over it."""
    gd = _hand_graph()
    gd["edge_to"] = gd["edge_to"].copy(); gd["edge_to"][0] = 2
    m = npc.node_path_model(gd, [], True)
    assert not m["unary"][0] and m["unary"][1]
    H = npc.HostFlatten(pkg, gd, None)
    assert not H.F and "consecutive" in H.error
