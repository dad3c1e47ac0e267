"""The decoder's side of HLALA_SEEDS_GPU_FILL without a GPU: tests/host_cpp/bam_fill_hook_model.cpp stands in for the GPU library's five hooks (those of the name-order test,
and for the fill hook the gather through the grouping permutation plus the fill model) and calls the decoder of hla-la_amd/csrc/host_bam.cpp as hlala_bam_extract_seeds_gpu
does.  What is checked is the host code around the hook: which units the host keeps for itself and their sizes, the offsets taken from the hook, the contiguous ranges of
units asked for, the slices written where they belong, the host units filled behind them, and every way back to the host's own layout and fill.
tests/test_gpu_bam_fill.py runs the same BAMs through the real hooks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bam_scan_cases as K
from test_bam import make_records, write_bam

INTERVALS = K.INTERVALS


@pytest.fixture(scope="module")
def emul(pkg, tmp_path_factory):
    so = tmp_path_factory.mktemp("fill_hook_model") / "libfill_hook_model.so"
    libdir = os.path.join(K.ROOT, "hla-la_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(so), os.path.join(K.ROOT, "tests", "host_cpp", "bam_fill_hook_model.cpp"),
                           "-L" + libdir, "-lhlala_gpu", "-Wl,-rpath," + libdir, "-lz"])
    em = C.CDLL(str(so))
    em.fil_emul.argtypes = [C.c_char_p, C.c_int32, C.POINTER(pkg.BamInterval), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    return em


@pytest.fixture(scope="module")
def decode(pkg, emul):
    lib = pkg.load_library()
    lib.hlala_bam_last_error.restype = C.c_char_p

    def run(path, intervals=INTERVALS, long_mode=False, flags=0, threads=3, fill=True, refuse_group=False, sort_mode=0, fill_mode=0):
        arr = (pkg.BamInterval * len(intervals))()
        for i, (nm, a, b, c) in enumerate(intervals):
            arr[i] = pkg.BamInterval(nm.encode(), a, b, c)
        h = C.c_void_p()
        fl = flags | pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP | pkg.SEEDS_GPU_SORT | (pkg.SEEDS_GPU_FILL if fill else 0)
        if emul.fil_emul(str(path).encode(), len(intervals), arr, int(long_mode), threads, fl, int(refuse_group), int(sort_mode), int(fill_mode), C.byref(h)) != 0:
            raise pkg.HlalaError(lib.hlala_bam_last_error().decode(errors="replace"))
        return pkg.SeedBatch(lib, h, long_mode)
    return run


def same_sample(A, B):
    assert A.n_units == B.n_units and A.counts == B.counts and A.names() == B.names()
    a, b = A.to_dict(), B.to_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def wide_units(S, long_mode):
    """w: the units of a (host-decoded) sample with more than 16 chains on one mate"""
    co = S.to_dict()["chain_off"]; nm = 1 if long_mode else 2
    per = np.diff(co).reshape(-1, nm)
    return int((per > 16).any(axis=1).sum())


def second_bam_records():
    """mates of 15, 16 and 17 alignments with tied scores, between ordinary pairs; returns (refs, records, units with a 17-alignment mate)"""
    rng = np.random.default_rng(41)
    refs = [("chr6", 50000), ("chrUn", 9000), ("HLA-A*01", 4000)]
    recs = []
    sizes = {"wide15": (15, 2), "wide16": (16, 16), "wide17": (17, 3), "wide17b": (2, 17), "wide16c": (16, 1)}
    names = list(sizes) + ["plain%02d" % i for i in range(40)]
    for name in names:
        for mate, k in enumerate(sizes.get(name, (int(rng.integers(1, 4)), int(rng.integers(1, 4))))):
            for j in range(k):
                L = int(rng.choice((149, 150, 151)))
                seq = "".join("ACGT"[x] for x in rng.integers(0, 4, L))
                flag = 1 | (64 if mate == 0 else 128) | (16 if rng.random() < 0.5 else 0) | (256 if j != k // 2 else 0)
                recs.append(dict(name=name, flag=flag, ref=0, pos=int(rng.integers(10100, 18000)), cigar=[(L, "M")], seq=seq, qual=[int(q) for q in rng.integers(2, 41, L)],
                                 tags=[("AS", "C", int(rng.choice((40, 40, 40, 77, 90))))]))
    rng.shuffle(recs)
    return refs, recs, 2


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    p = tmp_path_factory.mktemp("fill_bam") / "t.bam"; write_bam(p, refs, recs, block=3000)
    return p


@pytest.fixture(scope="module")
def bam2(tmp_path_factory):
    refs, recs, w = second_bam_records()
    p = tmp_path_factory.mktemp("fill_bam2") / "w.bam"; write_bam(p, refs, recs, block=3000)
    return p, w


@pytest.mark.parametrize("hash_bits", [None, "8", "0"])
def test_same_sample_as_the_host_decoder(pkg, decode, emul, bam, monkeypatch, hash_bits):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                # several rounds
    if hash_bits is not None:
        monkeypatch.setenv("HLALA_BAM_TEST_HASH_BITS", hash_bits)
    lib = pkg.load_library()
    for long_mode in (False, True):
        for flags in (0, pkg.SEEDS_PACKED):
            H = pkg.bam_open_seeds(lib, bam, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
            w = wide_units(H, long_mode)
            G = decode(bam, long_mode=long_mode, flags=flags)
            on_gpu, by_host, whole = G.fill_counts()
            assert whole == 0 and on_gpu + by_host == G.n_units > 100 and H.fill_counts() == (0, 0, 0)
            if hash_bits is None:
                assert (on_gpu, by_host) == (G.n_units - w, w) and w < G.n_units / 10           # the fall-back hides no broken fill
            else:
                assert by_host >= max(1, w)
            if hash_bits == "0":
                assert by_host > on_gpu                                    # one hash per partition: nearly every unit is the host's
            same_sample(G, H)
            G.close(); H.close()
            assert emul.fil_states() == 0                                   # the state went with the last unit filled


def test_windows_asked_out_of_order(pkg, decode, emul, bam, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    lib = pkg.load_library()
    H = pkg.bam_open_seeds(lib, bam, INTERVALS, threads=3, flags=pkg.SEEDS_PACKED)
    G = decode(bam, flags=pkg.SEEDS_PACKED)
    n = G.n_units
    cuts = [(n - 7, 7), (n // 2, 40), (0, 1), (n // 2 - 30, 60), (5, n // 3), (n // 2, 40)]
    for u0, k in cuts:
        a, b = G.to_dict(u0, k), H.to_dict(u0, k)
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (u0, k, key)
        assert G.names(u0, k) == H.names(u0, k)
    assert emul.fil_states() == 1                                           # units remain: the state is the sample's
    G.close()
    assert emul.fil_states() == 0                                           # ... and goes with it
    G = decode(bam, flags=pkg.SEEDS_PACKED)
    same_sample(G, H)
    G.close(); H.close()


def test_eager_fill(pkg, decode, emul, bam, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_EAGER", "1")
    lib = pkg.load_library()
    H = pkg.bam_open_seeds(lib, bam, INTERVALS, threads=3)
    G = decode(bam)
    assert emul.fil_states() == 0 and G.fill_counts()[2] == 0 and G.fill_counts()[0] > 100
    same_sample(G, H)
    G.close(); H.close()


def test_units_beyond_16_alignments_are_host_units(pkg, decode, bam2, monkeypatch):
    p, w = bam2
    lib = pkg.load_library()
    for flags in (0, pkg.SEEDS_PACKED):
        H = pkg.bam_open_seeds(lib, p, INTERVALS, threads=3, flags=flags)
        assert wide_units(H, False) == w
        G = decode(p, flags=flags)
        assert G.fill_counts() == (G.n_units - w, w, 0) and G.n_units == 45
        same_sample(G, H)
        G.close(); H.close()


def test_the_ways_back_to_the_hosts_fill(pkg, decode, bam, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    lib = pkg.load_library()
    H = pkg.bam_open_seeds(lib, bam, INTERVALS, threads=3)
    for kw in (dict(fill_mode=1), dict(sort_mode=1), dict(refuse_group=True)):          # the fill hook, the sort hook, the group hook answers "not available"
        G = decode(bam, **kw)
        assert G.fill_counts() == (0, 0, 1)
        same_sample(G, H)
        G.close()
    P = decode(bam, fill=False)                                    # the parent's behaviour
    assert P.fill_counts() == (0, 0, 0) and P.sort_counts()[0] > 0
    same_sample(P, H)
    P.close(); H.close()


def test_the_flag_needs_the_sort_stage(pkg, bam):
    lib = pkg.load_library()
    with pytest.raises(pkg.HlalaError, match="GPU_FILL needs HLALA_SEEDS_GPU_SORT"):
        pkg.bam_open_seeds(lib, bam, INTERVALS, flags=pkg.SEEDS_GPU_FILL)
