"""Census (CPU): which extension-DP calls the band kernels can take when the test is the PATH of the call's start node (FlatGraph::npf_* / npb_*, flat_graph.hpp)
and not the linear run of its start level.  From the oracle's seed chains after projection + numpy, as tools/dp_track_census.py; the path order itself is the
library's (libhlala_host.so: hlala_host_node_paths).  Per world: level-linear calls (band before), node-linear calls beyond them, how many of those are contiguous
under the built order, and the iteration weight (40 + bases left) of each class.
   python tools/dp_node_path_census.py [n_levels] [n_pairs] [frac_gene] [--test-world]
The functions below are also the numpy definition the CPU test of the flatten (tests/test_node_paths_cpu.py) compares the library with."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

BAND_MARGIN, BAND_MAXJ = 8, 48          # hlala_api.hip: band_margin; batch.h: BAND_MAXJ64


def band_need(bases):
    """Steps a call must find ahead of its start node to be listed (k_dp_items): reach + the tail of sequence gaps."""
    bases = np.asarray(bases, np.int64)
    return bases + BAND_MARGIN + np.minimum(bases + 6, 40)


def new_ids(gd):
    """creation index -> level-major node id (stable in creation index), and the inverse."""
    order = np.argsort(gd["node_level"], kind="stable")
    new = np.empty(len(order), np.int64); new[order] = np.arange(len(order))
    return new, order


def node_path_model(gd, jump_nodes, forward):
    """Unary nodes, successors, primary predecessors, label words and first edges of one direction, by level-major node id.
    jump_nodes: creation indices of the nodes with a gap-path jump of two or more edges in this direction."""
    N = gd["n_nodes"]
    new, order = new_ids(gd)
    lvl = gd["node_level"][order].astype(np.int64)
    ef = new[gd["edge_from"]]; et = new[gd["edge_to"]]
    src, dst = (ef, et) if forward else (et, ef)
    eo = np.argsort(src, kind="stable")                       # CSR order: by node, creation order inside
    s = src[eo]; d = dst[eo]; lab = gd["edge_label"][eo].astype(np.uint32)
    deg = np.bincount(s, minlength=N); off = np.concatenate([[0], np.cumsum(deg)])
    dmin = np.full(N, N, np.int64); np.minimum.at(dmin, s, d)
    dmax = np.full(N, -1, np.int64); np.maximum.at(dmax, s, d)
    bad = np.bincount(s, weights=((lab == ord("_")) | (lab == 0)), minlength=N) > 0
    hasj = np.zeros(N, bool); hasj[new[np.asarray(jump_nodes, np.int64)]] = True
    unary = (deg >= 1) & (deg <= 4) & (dmin == dmax) & ~bad & ~hasj
    succ = np.where(unary, dmin, -1)
    unary &= lvl[np.clip(succ, 0, N - 1)] == lvl + (1 if forward else -1)
    succ = np.where(unary, succ, -1)
    u = np.nonzero(unary)[0]
    prim = np.full(N, N, np.int64); np.minimum.at(prim, succ[u], u); prim[prim == N] = -1
    word = np.zeros(N, np.uint32)
    for k in range(4):
        has = unary & (deg > k)
        word[has] |= lab[off[:-1][has] + k] << np.uint32(8 * k)
    eid = np.full(N, -1, np.int64); eid[unary] = eo[off[:-1][unary]]
    link = unary & (prim[np.clip(succ, 0, N - 1)] == np.arange(N))          # u is the primary predecessor of its successor
    return dict(unary=unary, succ=succ, prim=prim, word=word, eid=eid, link=link, deg=deg, level=lvl)


def chain_runs(m, cap=255):
    """Unary steps that can be walked from every node along succ, contiguous in storage or not (capped)."""
    N = len(m["succ"])
    cnt = m["unary"].astype(np.int64); nxt = np.where(m["unary"], m["succ"], np.arange(N))
    for _ in range(8):
        cnt = np.minimum(cap, cnt + cnt[nxt]); nxt = nxt[nxt]
    return cnt


def path_order(m):
    """Positions of the path order: chains from the nodes without a unary predecessor, in node order, while the chain's node is the primary of its successor."""
    succ = m["succ"].tolist(); link = m["link"].tolist()
    pos = [0] * len(succ); p = 0
    for h in np.nonzero(m["prim"] < 0)[0].tolist():
        u = h
        while True:
            pos[u] = p; p += 1
            if not link[u]:
                break
            u = succ[u]
    return np.asarray(pos, np.int64)


class HostFlatten:
    """The library's flatten of a world without a device (libhlala_host.so)."""
    def __init__(self, pkg, gd, contigs):
        so = os.environ.get("HLALA_HOST_LIB") or os.path.join(ROOT, "hla-la_amd", "libhlala_host.so")
        if not os.path.exists(so):
            import subprocess
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "hla-la_amd", "csrc"), "../libhlala_host.so"])
        self.pkg = pkg; self.lib = lib = C.CDLL(so); self.N = gd["n_nodes"]; self.L = gd["n_levels"]
        lib.hlala_host_flatten.restype = C.c_void_p
        lib.hlala_host_flatten.argtypes = [C.POINTER(pkg.GraphDesc), C.POINTER(pkg.ContigsDesc)]
        lib.hlala_host_free.argtypes = [C.c_void_p]
        lib.hlala_host_info.argtypes = [C.c_void_p, C.POINTER(pkg.GraphInfo)]
        lib.hlala_host_paths.argtypes = [C.c_void_p, pkg.c_i32p, pkg.c_i32p, pkg.c_i32p]
        lib.hlala_host_last_error.restype = C.c_char_p
        c_u32p = C.POINTER(C.c_uint32)
        lib.hlala_host_linear.argtypes = [C.c_void_p, c_u32p, pkg.c_i32p, pkg.c_u8p, pkg.c_u8p]
        lib.hlala_host_node_paths.argtypes = [C.c_void_p, C.c_int, c_u32p, pkg.c_i32p, pkg.c_i32p, pkg.c_u8p, pkg.c_i32p]
        g, self._k1 = pkg.fill_struct(pkg.GraphDesc, gd)
        if contigs is not None:
            c, self._k2 = pkg.fill_struct(pkg.ContigsDesc, contigs)
            self.F = lib.hlala_host_flatten(C.byref(g), C.byref(c))
        else:
            self.F = lib.hlala_host_flatten(C.byref(g), None)
        self.error = None if self.F else lib.hlala_host_last_error().decode()

    def jump_nodes(self):
        """(forward, backward): creation indices of the nodes a gap path of two or more edges starts / ends at (the device's jump tables, flat_graph.hpp)."""
        gi = self.pkg.GraphInfo(); self.lib.hlala_host_info(self.F, C.byref(gi))
        a = [np.zeros(gi.n_paths, np.int32) for _ in range(3)]
        if gi.n_paths:
            self.lib.hlala_host_paths(self.F, *[x.ctypes.data_as(self.pkg.c_i32p) for x in a])
        long_ = a[2] >= 2
        return a[0][long_], a[1][long_]

    def node_paths(self, forward):
        N = self.N; pkg = self.pkg
        lab = np.zeros(N, np.uint32); eid = np.zeros(N, np.int32); node = np.zeros(N, np.int32); steps = np.zeros(N, np.uint8); pos = np.zeros(N, np.int32)
        self.lib.hlala_host_node_paths(self.F, 1 if forward else 0, lab.ctypes.data_as(C.POINTER(C.c_uint32)), eid.ctypes.data_as(pkg.c_i32p), node.ctypes.data_as(pkg.c_i32p),
                                       steps.ctypes.data_as(pkg.c_u8p), pos.ctypes.data_as(pkg.c_i32p))
        return dict(label=lab, eid=eid, node=node, steps=steps, pos=pos)

    def linear(self):
        L = self.L; pkg = self.pkg
        lab = np.zeros(L, np.uint32); eid = np.zeros(L, np.int32); lo = np.zeros(L, np.uint8); li = np.zeros(L, np.uint8)
        self.lib.hlala_host_linear(self.F, lab.ctypes.data_as(C.POINTER(C.c_uint32)), eid.ctypes.data_as(pkg.c_i32p), lo.ctypes.data_as(pkg.c_u8p), li.ctypes.data_as(pkg.c_u8p))
        return dict(label=lab, eid=eid, out=lo, inn=li)

    def close(self):
        if self.F:
            self.lib.hlala_host_free(self.F); self.F = None


def dp_calls(gd, b, seeds, stride=384):
    """(forward?, start node by creation index, start level, bases left) of every extension-DP call of a batch, before sharing, from the seed chains after projection."""
    nl = gd["node_level"]; ef = gd["edge_from"]; et = gd["edge_to"]; L = gd["n_levels"]
    st = seeds["status"]; nc = seeds["n_cols"]; sb = seeds["seq_begin"].astype(np.int64); se = seeds["seq_end"].astype(np.int64)
    edges = seeds["col_edge"].reshape(-1, stride)
    read_of_chain = np.repeat(np.arange(len(b["chain_off"]) - 1), np.diff(b["chain_off"]))
    rlen = np.diff(b["read_off"])[read_of_chain].astype(np.int64)
    ok = np.nonzero((st == 0) & (nc > 0))[0]
    e0 = edges[ok, 0]; e1 = edges[ok, nc[ok] - 1]
    good = (e0 >= 0) & (e1 >= 0); ok = ok[good]; e0 = e0[good]; e1 = e1[good]
    basesR = rlen[ok] - 1 - se[ok]; nodeR = et[e1]; r = (basesR > 0) & (nl[nodeR] < L - 1)
    basesL = sb[ok]; nodeL = ef[e0]; l = (basesL > 0) & (nl[nodeL] > 0)
    fwd = np.concatenate([np.zeros(l.sum(), bool), np.ones(r.sum(), bool)])
    node = np.concatenate([nodeL[l], nodeR[r]]); bases = np.concatenate([basesL[l], basesR[r]])
    return fwd, node, nl[node], bases


def census(pkg, w, b, seeds, out=print):
    gd = w["graph"]
    H = HostFlatten(pkg, gd, w["contigs"])
    assert H.F, H.error
    jf, jb = H.jump_nodes(); new, _ = new_ids(gd); lin = H.linear()
    fwd, node, level, bases = dp_calls(gd, b, seeds)
    need = band_need(bases); short = bases <= BAND_MAXJ
    lvl_run = np.where(fwd, lin["out"][level], lin["inn"][level]).astype(np.int64)
    node_run = np.zeros(len(node), np.int64); contig_run = np.zeros(len(node), np.int64)
    for forward, jn in ((True, jf), (False, jb)):
        m = node_path_model(gd, jn, forward); runs = chain_runs(m); P = H.node_paths(forward)
        sel = fwd == forward; n = new[node[sel]]
        node_run[sel] = runs[n]; contig_run[sel] = P["steps"][P["pos"][n]]
    H.close()
    wgt = 40 + bases; tot = len(node); wtot = wgt.sum()
    level_lin = short & (lvl_run >= need); node_lin = short & (node_run >= need) & ~level_lin; contig = short & (contig_run >= need) & ~level_lin
    out("%d DP calls before sharing; reach = bases + %d + min(bases + 6, 40), bases <= %d" % (tot, BAND_MARGIN, BAND_MAXJ))
    for name, msk in (("level-linear (band before)", level_lin), ("node-linear, not level-linear (new)", node_lin), ("   of those contiguous in the path order", contig),
                      ("more than %d bases left" % BAND_MAXJ, ~short), ("neither", short & ~level_lin & ~node_lin)):
        out("   %-44s %8d  %5.1f %% of calls  %5.1f %% of iteration weight" % (name, int(msk.sum()), 100.0 * msk.sum() / max(1, tot), 100.0 * wgt[msk].sum() / max(1, wtot)))
    return dict(calls=tot, level_linear=int(level_lin.sum()), node_linear=int(node_lin.sum()), contiguous=int(contig.sum()))


def main():
    from tools import synth
    from oracle_binding import Oracle
    from conftest import load_package
    pkg = load_package()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--test-world" in sys.argv:          # the world and batch of tests/test_gpu_band_node_paths.py
        w = synth.make_world_m(seed=7, n_levels=60_000, n_windows=3, alleles=(400, 3000)); b = synth.make_batch_m(w, 1500, seed=21, frac_gene=1.0)
        print("world: make_world_m(seed=7, n_levels=60000, n_windows=3, alleles=(400, 3000)), make_batch_m(1500, seed=21, frac_gene=1.0)")
    else:
        nlev = int(args[0]) if len(args) > 0 else 1_000_000; npairs = int(args[1]) if len(args) > 1 else 6000; fg = float(args[2]) if len(args) > 2 else 0.3
        w = synth.make_world_m(seed=2, n_levels=nlev); b = synth.make_batch_m(w, npairs, seed=1000, frac_gene=fg)
        print("world: make_world_m(seed=2, n_levels=%d), make_batch_m(%d, seed=1000, frac_gene=%.2f)" % (nlev, npairs, fg))
    g = w["graph"]
    print("levels %d, nodes %d, edges %d" % (g["n_levels"], g["n_nodes"], g["n_edges"]))
    o = Oracle(g, w["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=12345, max_columns=384)
    census(pkg, w, b, o.align_batch(b, stop_after_projection=True)["seeds"])


if __name__ == "__main__":
    main()
