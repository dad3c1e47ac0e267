"""Descriptor sets, BAMs and bindings for the wide fill path (hlala_bam_fill_create_wide, hlala_host_bam_fill_model_wide, HLALA_SEEDS_GPU_FILL_WIDE): units with a mate of more
than 16 alignments, where std::sort is an introsort and the order of equal scores has no closed form.  The builders are those of tests/bam_fill_cases.py.  There is no
plain-Python expectation here -- Python's sorted() is stable, std::sort beyond 16 elements is not: the model is held against the host decoder's own std::sort on written BAMs
(tests/test_bam_fill_wide_model.py), the device against the model (tests/test_gpu_bam_fill_wide.py).  Shared by the CPU and the GPU tests; every case comes from a fixed seed."""
import ctypes as C
import os
import subprocess

import numpy as np

import bam_fill_cases as F
import bam_scan_cases as K
from conftest import ROOT, load_package

WIDE_MAX = 4096
REFS = [("chr6", 50000), ("chrUn", 9000), ("HLA-A*01", 4000)]


def load_model():
    pkg = load_package()
    so = os.environ.get("HLALA_HOST_LIB") or os.path.join(ROOT, "hla-la_amd", "libhlala_host.so")
    src = os.path.join(ROOT, "hla-la_amd", "csrc")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(os.path.join(src, f)) for f in ("bam_fill_core.h", "bam_fill_wide_core.h", "bam_fill_model.h", "host_check.cpp")):
        subprocess.check_call(["make", "-C", src, "../libhlala_host.so"])
    lib = C.CDLL(so)
    lib.hlala_host_bam_fill_model_wide.argtypes = [C.POINTER(pkg.BamFillIn), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(pkg.BamFillOut),
                                                   C.POINTER(pkg.BamFillStats), C.POINTER(C.c_int64)]
    lib.hlala_host_bam_fill_model_wide.restype = C.c_int
    lib.hlala_host_bam_fill_model.argtypes = [C.POINTER(pkg.BamFillIn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(pkg.BamFillOut), C.POINTER(pkg.BamFillStats)]
    lib.hlala_host_bam_fill_model.restype = C.c_int
    lib.hlala_host_bam_fill_wide_order.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]; lib.hlala_host_bam_fill_wide_order.restype = C.c_int
    lib.hlala_host_bam_fill_wide_adversary.argtypes = [C.c_int32, C.c_void_p]; lib.hlala_host_bam_fill_wide_adversary.restype = C.c_int
    lib.hlala_host_last_error.restype = C.c_char_p
    return lib


_adv = {}


def adversary(n):
    """scores that drive the library's std::sort into its heap sort (McIlroy's adversary, run in libhlala_host.so against std::sort itself, as the check program runs it)"""
    if n not in _adv:
        s = np.zeros(n, np.int32)
        assert load_model().hlala_host_bam_fill_wide_adversary(n, s.ctypes.data) == 0
        _adv[n] = s
    return _adv[n]


def wide_order(lib, scores):
    """fil_sort_wide on scores in file order: (places in sorted order, heap sorts entered)"""
    s = np.ascontiguousarray(scores, np.int32); out = np.zeros(len(s), np.uint32)
    h = lib.hlala_host_bam_fill_wide_order(s.ctypes.data, len(s), out.ctypes.data)
    return out, h


def run_model(lib, recs, data, first, count, hs, long_mode=False, packed=False, window=None, max_mate=WIDE_MAX, n=None, n_bytes=None, n_units=None, n_host_units=None):
    """F.run_model for hlala_host_bam_fill_model_wide: (rc, offsets, window arrays or None, counts, error text, the three wide counts)"""
    pkg = load_package()
    fin, keep = pkg.bam_fill_in(recs, data, first, count, hs, long_mode, packed, n=n, n_bytes=n_bytes, n_units=n_units, n_host_units=n_host_units)
    off = pkg.bam_fill_offsets(len(first), long_mode); st = pkg.BamFillStats(); wide = (C.c_int64 * 4)()
    ptr = [off[k].ctypes.data for k in ("read_off", "chain_off", "cigar_count", "name_off")]
    rc = lib.hlala_host_bam_fill_model_wide(C.byref(fin), max_mate, *ptr, 0, -1, None, C.byref(st), wide)
    err = lib.hlala_host_last_error().decode()
    arrs = None
    if rc == 0 and window is not None and len(first):
        out, arrs, size = pkg.bam_fill_window_arrays(off, window[0], window[1], long_mode, packed, F.CANARY)
        rc = lib.hlala_host_bam_fill_model_wide(C.byref(fin), max_mate, *ptr, window[0], window[1], C.byref(out), C.byref(st), wide)
        err = lib.hlala_host_last_error().decode()
        arrs = F.check_canaries(arrs, size)
    return rc, off, arrs, {f: int(getattr(st, f)) for f in F.COUNT_FIELDS}, err, tuple(int(x) for x in wide[:3])


def is_wide(u, long_mode=False):
    m = [sum(1 for a in u["als"] if a["mate"] == k) for k in range(1 if long_mode else 2)]
    return len(u["als"]) > 32 or max(m) > 16


def longest(u):
    return max(sum(1 for a in u["als"] if a["mate"] == k) for k in (0, 1))


def wunit(rng, name, sizes, scores=None, primary_at=None, long_mode=False):
    """F.unit with short reads and one or two CIGAR operations per alignment: a mate of 4096 stays a few hundred KiB"""
    u = F.unit(rng, name, sizes, scores=scores, primary_at=primary_at, long_mode=long_mode)
    for a in u["als"]:
        a.update(F.al(rng, a["mate"], a["AS"], a["primary"], l_seq=int(rng.integers(0, 12)), n_cigar=int(rng.integers(1, 3))))
    return u


_cases = None


def cases():
    """name -> (units, long_mode).  Few samples, many units each: a sample is one create call and a handful of windows"""
    global _cases
    if _cases is not None:
        return _cases
    rng = np.random.default_rng(4096)
    c = {}
    few = lambda m, k: int(rng.integers(-2, 3))
    # ---- the edge between the paths, every second unit wide, wide first and last, two wide units in a row
    sizes = [(17, 1), (16, 16), (18, 2), (2, 3), (31, 1), (4, 1), (16, 17), (1, 16), (17, 17), (32, 1), (33, 2), (1, 1), (3, 40), (40, 3), (20, 1)]
    c["edge_of_the_paths"] = ([wunit(rng, b"e%02d" % i, s, scores=few) for i, s in enumerate(sizes)], False)
    # ---- the strides of the wave
    c["strides_of_the_wave"] = ([wunit(rng, b"s%d" % k, (k, 1 + k % 3), scores=lambda m, j: int(rng.integers(0, 7))) for k in (63, 64, 65, 128, 129)] + [wunit(rng, b"narrow", (2, 2))], False)
    # ---- scores: all equal, two distinct, negative, the adversary
    us = [wunit(rng, b"eq%d" % k, (k, max(1, k // 5)), scores=lambda m, j: 40) for k in (17, 33, 100)]
    us.append(wunit(rng, b"two", (90, 70), scores=lambda m, j: 40 if rng.random() < 0.7 else 77))
    us.append(wunit(rng, b"neg", (50, 21), scores=lambda m, j: -int(rng.integers(1, 5)) * 1000))
    adv = adversary(256)
    us.append(wunit(rng, b"adv", (256, 256), scores=lambda m, j: int(adv[j]) if m == 0 else -int(adv[j])))
    c["scores"] = (us, False)
    # ---- primaries: first, last, tied with everything around them, two of them
    us = []
    for where, at in (("first", {0}), ("last", {39}), ("middle", {20}), ("two", {7, 31})):
        us.append(wunit(rng, b"p-" + where.encode(), (40, 23), scores=few, primary_at=(at, {min(at) % 23})))
        us.append(wunit(rng, b"t-" + where.encode(), (40, 23), scores=lambda m, j: 9, primary_at=(at, {22 - min(at) % 23})))
    c["primaries"] = (us, False)
    # ---- long-read mode
    c["long_reads"] = ([wunit(rng, b"L17", (17, 0), long_mode=True, scores=few), wunit(rng, b"L3", (3, 0), long_mode=True), wunit(rng, b"L65", (65, 0), long_mode=True, scores=lambda m, j: j % 3),
                        wunit(rng, b"L16", (16, 0), long_mode=True, scores=few)], True)
    # ---- the cap
    c["mates_of_4095_and_4096"] = ([wunit(rng, b"k4095", (4095, 2), scores=lambda m, j: int(rng.integers(0, 30))), wunit(rng, b"n", (1, 2)),
                                   wunit(rng, b"k4096", (3, 4096), scores=lambda m, j: int(rng.integers(0, 3)))], False)
    # ---- a sample without any wide unit
    c["no_wide_unit"] = (F.random_units(rng, 40, max_mate=16, host=lambda i: i == 7), False)
    # ---- host units between wide units
    us = [wunit(rng, b"h%02d" % i, (25, 2) if i % 3 == 0 else (2, 2), scores=few) for i in range(12)]
    us[4]["host"] = True; us[10]["host"] = True                   # (two narrow ones)
    c["host_units_between"] = (us, False)
    _cases = c
    return c


def refused():
    """name -> (units, what the refusal says)"""
    rng = np.random.default_rng(77)
    no_primary = wunit(rng, b"no-primary", (30, 2))
    return {"mate_of_4097": ([wunit(rng, b"a", (2, 2)), wunit(rng, b"k4097", (4097, 1), scores=lambda m, j: j % 5)], "more alignments on one mate than max_mate", None),
            "no_primary": ([wunit(rng, b"a", (2, 2)), no_primary], "without a primary", 1)}


def built_refused(name):
    units, text, strip = refused()[name]
    recs, data, first, count, hs = F.build(units, False)
    if strip is not None:                                           # (the unit's mate 0 loses its primaries after the build)
        recs = recs.copy(); k = slice(int(first[strip]), int(first[strip]) + int(count[strip]))
        recs["flags"][k] = np.where(recs["which"][k] == 0, recs["flags"][k] & 1, recs["flags"][k])
    return recs, data, first, count, hs, text


def windows(units, long_mode):
    """F.windows, and cuts directly before, behind and between the wide units"""
    n = len(units)
    w = list(F.windows(n))
    wide = [i for i, u in enumerate(units) if is_wide(u, long_mode)]
    for i in wide[:3]:
        w += [(i, 1)] + ([(i - 1, 1)] if i else []) + ([(i + 1, n - i - 1)] if i + 1 < n else [])
    for a, b in zip(wide, wide[1:]):
        if b - a > 1:
            w.append((a + 1, b - a - 1)); break
    return [x for x in dict.fromkeys(w) if x[1] > 0]


# ---------------------------------------------------------------------------------------------------------------- BAMs with wide units
def wide_bam_records(sizes, score_of, seed=43, plain=12, L=(30, 31, 32)):
    """records for units named w00, w01, ... whose mates have sizes[i] alignments with the scores score_of(i, mate, j), between `plain` ordinary pairs, shuffled; one
    primary per mate, somewhere in the middle.  Short reads: a mate of 4096 stays small"""
    rng = np.random.default_rng(seed)
    recs = []
    names = [("w%02d" % i, s) for i, s in enumerate(sizes)] + [("plain%02d" % i, (int(rng.integers(1, 4)), int(rng.integers(1, 4)))) for i in range(plain)]
    for ni, (name, sz) in enumerate(names):
        for mate, k in enumerate(sz):
            for j in range(k):
                n = int(rng.choice(L))
                seq = "".join("ACGT"[x] for x in rng.integers(0, 4, n))
                flag = 1 | (64 if mate == 0 else 128) | (16 if rng.random() < 0.5 else 0) | (256 if j != k // 2 else 0)
                AS = score_of(ni, mate, j) if ni < len(sizes) else int(rng.choice((40, 40, 77)))
                recs.append(dict(name=name, flag=flag, ref=0, pos=int(rng.integers(10100, 18000)), cigar=[(n, "M")], seq=seq, qual=[int(q) for q in rng.integers(2, 41, n)], tags=[("AS", "s", int(AS))]))
    rng.shuffle(recs)
    return REFS, recs


def bam_kinds():
    """name -> (sizes of the wide units' mates, score of (unit, mate, j))"""
    rng = np.random.default_rng(5)
    adv = adversary(256)
    sizes = [(17, 2), (3, 33), (64, 65), (256, 17)]
    return {
        "all_equal": (sizes, lambda i, m, j: 40),
        "two_scores": (sizes, lambda i, m, j: 40 if rng.random() < 0.6 else 90),
        "adversary_256": ([(256, 2), (1, 256), (17, 17)], lambda i, m, j: int(adv[j]) if (i, m) in ((0, 0), (1, 1)) else 40),
        "mate_of_4096": ([(4096, 1), (18, 1)], lambda i, m, j: int(rng.choice((40, 40, 40, 77, 90)))),
    }


def write_wide_bam(path, kind, plain=12):
    from test_bam import write_bam
    sizes, score = bam_kinds()[kind]
    refs, recs = wide_bam_records(sizes, score, plain=plain)
    write_bam(path, refs, recs, block=3000 if len(recs) < 2000 else 60000)
    return sizes


def sample_through_the_models(pkg, path, long_mode, packed, max_mate=WIDE_MAX):
    """the scan, group and name-order models in a row, then the WIDE fill model with no host unit at all: (offsets, the slices of a window over all units, unit_first,
    the three wide counts).  tests/test_bam_fill_model.py does the same with the narrow model and host units"""
    import bam_group_cases as G
    import bam_nameorder_cases as N
    from test_bam_fill_model import header_end, inflate_bam
    data = inflate_bam(path)
    rc, recs, comp, st = K.run_model(K.load_model(), data, K.scan_args(REFS, long_mode), first=header_end(data), last=True)
    assert rc == 0 and st["status"] == K.OK
    comp = np.frombuffer(comp, np.uint8)
    rc, perm, flag, counts, err = G.run_model(G.load_model(), recs, comp, long_mode)
    assert rc == 0 and counts["n_collided_runs"] == 0
    g = recs[perm]
    starts = np.nonzero(flag & 1)[0]; ends = np.append(starts[1:], len(g))
    runs = [(int(a), int(z - a)) for a, z in zip(starts, ends) if flag[a] & 4]
    off = np.array([int(g["rec_off"][a]) + 32 for a, _ in runs], np.uint64); ln = np.array([int(g["nameLen"][a]) for a, _ in runs], np.uint32)
    rc, order, _, err = N.run_model(N.load_model(), off, ln, comp)
    assert rc == 0
    first = np.array([runs[int(k)][0] for k in order], np.uint32); count = np.array([runs[int(k)][1] for k in order], np.uint32)
    rc, goff, garr, counts, err, wide = run_model(load_model(), g, comp, first, count, np.zeros(0, np.int64), long_mode, packed, window=(0, len(first)), max_mate=max_mate)
    assert rc == 0, err
    return goff, garr, first, wide


def write_beyond_bam(path):
    """a unit with 4097 alignments on a mate between wide and ordinary ones: it stays with the host under every flag"""
    from test_bam import write_bam
    rng = np.random.default_rng(6)
    sizes = [(4097, 1), (20, 20), (2, 64)]
    refs, recs = wide_bam_records(sizes, lambda i, m, j: int(rng.choice((40, 40, 77))), seed=44, plain=6)
    write_bam(path, refs, recs, block=60000)
    return sizes


def hook_model(tmp_path_factory):
    """tests/host_cpp/bam_fill_wide_hook_model.cpp as a library: filw_emul decodes with the six stand-in hooks"""
    pkg = load_package()
    so = tmp_path_factory.mktemp("fill_wide_hook_model") / "libfill_wide_hook_model.so"
    libdir = os.path.join(ROOT, "hla-la_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(so), os.path.join(ROOT, "tests", "host_cpp", "bam_fill_wide_hook_model.cpp"),
                           "-L" + libdir, "-lhlala_gpu", "-Wl,-rpath," + libdir, "-lz"])
    em = C.CDLL(str(so))
    em.filw_emul.argtypes = [C.c_char_p, C.c_int32, C.POINTER(pkg.BamInterval), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    return em
