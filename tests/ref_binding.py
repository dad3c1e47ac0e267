"""ctypes binding of oracle/_ref/libhlala_ref.so: the reference's own extension aligner and the static members of its processBAM around it
(projection, pairing, mapping qualities; oracle/ref/), the referee of the oracle.

The library is built from a checkout of the reference by oracle/ref/Makefile; it is never committed.  `available()` builds it on
demand when the reference directory is present and says why not otherwise."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = load_package()
REF_DIR = os.environ.get("HLALA_REF_DIR", "/root/reference")
_dir = os.path.join(ROOT, "oracle", "_ref")
_so = os.path.join(_dir, "libhlala_ref.so")
_lib = None

INT_KEYS = ("status", "n_cols", "seq_begin", "seq_end")
COL_KEYS = ("col_level", "col_edge", "col_gchar", "col_schar", "col_fromseed")


def have_reference():
    return os.path.exists(os.path.join(REF_DIR, "mapper", "aligner", "extensionAligner.cpp"))


def available():
    """(True, "") when the library can be loaded (built now if the reference is here), else (False, reason)."""
    if have_reference():
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref"), "HLALA_REF_DIR=" + REF_DIR])
    if os.path.exists(_so):
        return True, ""
    return False, "no oracle/_ref/libhlala_ref.so and no reference sources at %s to build it from (oracle/ref/Makefile)" % REF_DIR


def sources_hash(pipeline=False):
    """Hash over the reference sources the library was compiled from (written by oracle/ref/Makefile): over the aligner's sources, which
    wrote the ref_*.npz fixtures of the extension stage, or (pipeline=True) over those plus processBAM.cpp and what its link needs."""
    with open(os.path.join(_dir, "ref_sources_pipeline.sha256" if pipeline else "ref_sources.sha256")) as f:
        return f.read().strip()


PROJ_OK, PROJ_REFUSED, PROJ_NOT_KEPT = 0, 1, -100       # status of Reference.project_chains (the last one is this binding's filler)
STAGE_KEYS = ("n_cols", "seq_begin", "seq_end", "col_level", "col_gchar", "col_schar")


from ref_pipeline import gap_stretch_rule          # noqa: E402,F401  (the NumPy statement of the inGraphGapStretch rule: an input of project_chains)


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(_so)
        vp = C.c_void_p
        _lib.ref_create.argtypes = [C.POINTER(P.GraphDesc)]
        _lib.ref_create.restype = vp
        _lib.ref_destroy.argtypes = [vp]
        _lib.ref_last_error.restype = C.c_char_p
        _lib.ref_graph_n_paths.argtypes = [vp]
        _lib.ref_graph_paths.argtypes = [vp, P.c_i32p, P.c_i32p, P.c_i32p]
        _lib.ref_extend_seeds.argtypes = [vp, C.POINTER(P.SeedsIn), C.POINTER(P.ChainsOut), C.c_uint32, C.c_int, C.c_int, C.c_int]
        _lib.ref_project_chains.argtypes = [vp, C.POINTER(P.ContigsDesc), C.POINTER(P.BatchIn), C.c_int, P.c_u8p, P.c_u8p, C.c_int, C.POINTER(P.ChainsOut), C.POINTER(P.ChainsOut)]
        _lib.ref_pair_chains.argtypes = [vp, C.POINTER(P.ContigsDesc), C.POINTER(P.Params), C.POINTER(P.SeedsIn), P.c_i32p, C.c_int, C.POINTER(P.ChainsOut), C.POINTER(P.PairsOut), P.c_u8p]
        _lib.ref_mapq_unpaired.argtypes = [vp, C.POINTER(P.SeedsIn), P.c_f64p, C.c_int, C.c_int, C.POINTER(P.PairsOut)]
        _lib.ref_typer_create.argtypes = [vp, C.c_char_p]
        _lib.ref_typer_create.restype = vp
        _lib.ref_typer_destroy.argtypes = [vp]
        _lib.ref_typer_include.argtypes = [vp, C.c_int, P.c_i32p, P.c_i32p, P.c_u8p]
        _lib.ref_typer_exon_positions.argtypes = [vp, C.POINTER(TyperReads), C.POINTER(P.LocusDesc), C.POINTER(P.ExonPositionsOut), P.c_f64p]
        _lib.ref_typer_infer.argtypes = [vp, C.POINTER(TyperReads), C.c_double, C.c_double, C.c_char_p, C.c_char_p, C.c_char_p]
    return _lib


class ReferenceError_(RuntimeError):
    pass


class Reference:
    """Graph + mapper::aligner::extensionAligner of the reference over a graph description dict."""

    def __init__(self, graph, rng_seed=12345, long_read_mode=0, max_columns=384):
        self.rng_seed, self.long_read_mode, self.max_columns = rng_seed, long_read_mode, max_columns
        g, self._kg = P.fill_struct(P.GraphDesc, graph)
        self.h = lib().ref_create(C.byref(g))
        if not self.h:
            raise ReferenceError_(lib().ref_last_error().decode())

    def _check(self, rc):
        if rc != 0:
            raise ReferenceError_(lib().ref_last_error().decode())

    def graph_paths(self):
        """Graph::completedGapEdgePaths as (first node, last node, length) arrays."""
        n = lib().ref_graph_n_paths(self.h)
        a = [np.zeros(n, np.int32) for _ in range(3)]
        self._check(lib().ref_graph_paths(self.h, *[x.ctypes.data_as(P.c_i32p) for x in a]))
        return a

    def extend_seeds(self, seeds_in, mode=0):
        """extendSeedChain + scoreOneAlignment per chain.  mode 0: the oracle's and the product's seed discipline (two reference calls for a chain
        clipped at both ends); mode 1: one call per chain.  dp_iters / dp_score / removed_cols stay zero: the reference does not report them."""
        s, keep = P.fill_struct(P.SeedsIn, seeds_in)
        o, d = P.alloc_chains_out(seeds_in["n_chains"], self.max_columns)
        self._check(lib().ref_extend_seeds(self.h, C.byref(s), C.byref(o), self.rng_seed & 0xFFFFFFFF, self.long_read_mode, self.max_columns, mode))
        return d

    def project_chains(self, contigs, batch_in, keep, gap_stretch, unpaired=False, stages=False):
        """processBAM::alignment2Chain on every chain with keep != 0 (transformBAMreadToInternalAlignment, checkAlignmentConcordanceWithSequence,
        PRGContigAlignment2Seed).  status: PROJ_OK / PROJ_REFUSED (transform returned false) / PROJ_NOT_KEPT.  With stages=True also returns the three
        intermediate alignments (after transform, after cleanInitialAlignment, after restrictInitialAlignmentToNoGapAreas) as a list of dicts."""
        c, kc = P.fill_struct(P.ContigsDesc, contigs)
        b, kb = P.fill_struct(P.BatchIn, batch_in)
        n = int(batch_in["n_chains"])
        keep = np.ascontiguousarray(keep, np.uint8); gap = np.ascontiguousarray(gap_stretch, np.uint8)
        assert len(keep) == n
        o, d = P.alloc_chains_out(n, self.max_columns)
        d["status"][:] = PROJ_NOT_KEPT
        st, sd = None, None
        if stages:
            st = (P.ChainsOut * 3)(); sd = []
            for i in range(3):
                x, dd = P.alloc_chains_out(n, self.max_columns)
                st[i] = x; sd.append(dd)
        n_reads = int(batch_in["n_pairs"]) * (1 if unpaired else 2)
        self._check(lib().ref_project_chains(self.h, C.byref(c), C.byref(b), n_reads, keep.ctypes.data_as(P.c_u8p), gap.ctypes.data_as(P.c_u8p), self.max_columns, C.byref(o), st))
        return (d, sd) if stages else d

    def pair_chains(self, contigs, seeds_in, chain_abs, n_pairs, insert_mean, insert_sd):
        """The kept seed chains extended and scored (ref_extend_seeds mode 0 with the seeds rng_seed + 2 * chain_abs[c] + d), then the pairing loop, the
        selection and assignMappingQualities of processBAM::alignOneReadPair.  Returns (pairs, extended chains, best_is_penalty)."""
        c, kc = P.fill_struct(P.ContigsDesc, contigs)
        s, ks = P.fill_struct(P.SeedsIn, seeds_in)
        prm = P.Params(insert_mean, insert_sd, self.rng_seed & 0xFFFFFFFF, self.long_read_mode, self.max_columns, 0)
        ca = np.ascontiguousarray(chain_abs, np.int32)
        eo, ed = P.alloc_chains_out(seeds_in["n_chains"], self.max_columns)
        po, pd = P.alloc_pairs_out(n_pairs, self.max_columns)
        pen = np.zeros(n_pairs, np.uint8)
        self._check(lib().ref_pair_chains(self.h, C.byref(c), C.byref(prm), C.byref(s), ca.ctypes.data_as(P.c_i32p), n_pairs, C.byref(eo), C.byref(po), pen.ctypes.data_as(P.c_u8p)))
        return pd, ed, pen

    def mapq_unpaired(self, chains_in, ll, n_reads):
        """Utilities::findVectorMax + assignMappingQualities_unpaired per read over finished chains (hlala_seeds_in layout, grouped by read) and their
        log-likelihoods.  Per-read outputs in the layout of hlala_pairs_out; best_chain indexes `chains_in`."""
        s, ks = P.fill_struct(P.SeedsIn, chains_in)
        ll = np.ascontiguousarray(ll, np.float64)
        po, pd = P.alloc_pairs_out(n_reads, self.max_columns)         # (allocates 2n rows; the first n are used)
        self._check(lib().ref_mapq_unpaired(self.h, C.byref(s), ll.ctypes.data_as(P.c_f64p), n_reads, self.max_columns, C.byref(po)))
        return pd

    def close(self):
        if self.h:
            lib().ref_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TyperReads(C.Structure):
    """ref_typer_reads of oracle/ref/ref_driver.cpp"""
    _fields_ = [("n_units", C.c_int32), ("paired", C.c_int32), ("rows", C.POINTER(P.SeedsIn)), ("col_mapq", P.c_u8p), ("row_mapq", P.c_f64p), ("unit_mapq", P.c_f64p),
                ("primary_reverse", P.c_u8p), ("name_off", P.c_i32p), ("names", C.c_char_p)]


def _typer_reads(rows):
    """TyperReads from the dict tests/ref_typer.py: typer_rows builds; returns (struct, keepalive)."""
    s, ks = P.fill_struct(P.SeedsIn, rows["seeds"])
    enc = [n.encode() for n in rows["names"]]
    a = dict(col_mapq=np.ascontiguousarray(rows["col_mapq"], np.uint8), row_mapq=np.ascontiguousarray(rows["row_mapq"], np.float64),
             unit_mapq=np.ascontiguousarray(rows["unit_mapq"], np.float64), primary_reverse=np.ascontiguousarray(rows["primary_reverse"], np.uint8),
             name_off=np.concatenate([[0], np.cumsum([len(x) for x in enc])]).astype(np.int32))
    t = TyperReads(); t.n_units = int(rows["n_units"]); t.paired = int(rows["paired"]); t.rows = C.pointer(s); t.names = b"".join(enc)
    for k, v in a.items():
        setattr(t, k, v.ctypes.data_as(dict(TyperReads._fields_)[k]))
    return t, (s, ks, a, enc)


class ReferenceTyper:
    """hla::HLATyper of the reference over the graph of a Reference and a graph directory (PRG/segments.txt and the segment files)."""

    def __init__(self, ref, graph_dir):
        self.ref = ref
        self.h = lib().ref_typer_create(ref.h, str(graph_dir).encode())
        if not self.h:
            raise ReferenceError_(lib().ref_last_error().decode())

    def _check(self, rc):
        if rc != 0:
            raise ReferenceError_(lib().ref_last_error().decode())

    def include(self, first, last):
        """intervalOverlapsWithGenes per (first, last) level pair"""
        f = np.ascontiguousarray(first, np.int32); l = np.ascontiguousarray(last, np.int32); o = np.zeros(max(1, len(f)), np.uint8)
        self._check(lib().ref_typer_include(self.h, len(f), f.ctypes.data_as(P.c_i32p), l.ctypes.data_as(P.c_i32p), o.ctypes.data_as(P.c_u8p)))
        return o[:len(f)]

    def exon_positions(self, rows, level_min, level_to_exon, insert_mean, insert_sd, min_alignment_columns=1000):
        """The read loops of HLATypeInference for one locus around the reference's oneReadAlignment_2_exonPositions_*, alignmentWeightedOKFraction and
        removeDoublePositionsFromRead, in the layout of hlala_exon_positions (read_pair indexes the units of `rows`) plus pos_mapq_p = mapQ_position.
        Per-mate fields no position of an entry witnesses are -1 (read_reverse: 255); pos_mapq is not written."""
        t, keep = _typer_reads(rows)
        L, kl = P.make_locus_desc(level_min, level_to_exon, insert_mean, insert_sd, 0.0, 0.0, None, min_alignment_columns)
        n = int(rows["n_units"]); ncol = int(rows["seeds"]["col_off"][-1])
        o, d = P.alloc_exon_positions_out(n, ncol + 1, 2 * ncol + 1)
        mp = np.zeros(ncol + 1, np.float64)
        self._check(lib().ref_typer_exon_positions(self.h, C.byref(t), C.byref(L), C.byref(o), mp.ctypes.data_as(P.c_f64p)))
        e = P.trim_exon_positions(o, d)
        e["pos_mapq_p"] = mp[:e["n_pos"]].copy()
        return e

    def infer(self, rows, insert_mean, insert_sd, out_dir, long_reads_mode, g_dir):
        """HLATypeInference into out_dir, with one OpenMP thread and g_dir (holding hla_nom_g.txt) as the working directory during the call."""
        t, keep = _typer_reads(rows)
        self._check(lib().ref_typer_infer(self.h, C.byref(t), insert_mean, insert_sd, str(out_dir).encode(), long_reads_mode.encode(), str(g_dir).encode()))

    def close(self):
        if self.h:
            lib().ref_typer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chain_diffs(got, exp, n_chains, upto=None):
    """Per chain, the names of the integer / byte outputs in which `got` and `exp` differ (all chains, none left out).  upto[c] limits
    the column comparison of chain c to its first upto[c] columns (and leaves n_cols / seq_end out)."""
    st = exp["_stride"]
    assert got["_stride"] == st
    out = {}
    for c in range(n_chains):
        bad = []
        for k in INT_KEYS:
            if upto is not None and k in ("n_cols", "seq_end"):
                continue
            if got[k][c] != exp[k][c]:
                bad.append(k)
        n = int(exp["n_cols"][c]) if upto is None else int(upto[c])
        if upto is not None and (got["n_cols"][c] < n or exp["n_cols"][c] < n):
            bad.append("n_cols")
        for k in COL_KEYS:
            if not np.array_equal(got[k][c * st:c * st + n], exp[k][c * st:c * st + n]):
                bad.append(k)
        if bad:
            out[c] = bad
    return out
