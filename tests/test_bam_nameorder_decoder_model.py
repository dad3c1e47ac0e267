"""The decoder's side of HLALA_SEEDS_GPU_SORT without a GPU: tests/host_cpp/bam_sort_hook_model.cpp stands in for the GPU library's four hooks (those of the grouping test, and
for the sort hook the selection of the first records of clean, complete runs plus the name-order model) and calls the decoder of hla-la_amd/csrc/host_bam.cpp as
hlala_bam_extract_seeds_gpu does.  What is checked is the host code around the hook: the units of clean runs permuted through the device's order, the permutation check,
the units of collided runs merged in, and every way back to the host's own sort.  tests/test_gpu_bam_nameorder.py runs the same BAM through the real hooks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bam_scan_cases as K
from test_bam import make_records, write_bam

INTERVALS = K.INTERVALS


@pytest.fixture(scope="module")
def decode(pkg, tmp_path_factory):
    so = tmp_path_factory.mktemp("sort_hook_model") / "libsort_hook_model.so"
    libdir = os.path.join(K.ROOT, "hla-la_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(so), os.path.join(K.ROOT, "tests", "host_cpp", "bam_sort_hook_model.cpp"),
                           "-L" + libdir, "-lhlala_gpu", "-Wl,-rpath," + libdir, "-lz"])
    lib = pkg.load_library()
    em = C.CDLL(str(so))
    em.nam_emul.argtypes = [C.c_char_p, C.c_int32, C.POINTER(pkg.BamInterval), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.hlala_bam_last_error.restype = C.c_char_p

    def run(path, intervals=INTERVALS, long_mode=False, flags=0, threads=3, sort=True, refuse_group=False, sort_mode=0):
        arr = (pkg.BamInterval * len(intervals))()
        for i, (nm, a, b, c) in enumerate(intervals):
            arr[i] = pkg.BamInterval(nm.encode(), a, b, c)
        h = C.c_void_p()
        fl = flags | pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP | (pkg.SEEDS_GPU_SORT if sort else 0)
        if em.nam_emul(str(path).encode(), len(intervals), arr, int(long_mode), threads, fl, int(refuse_group), int(sort_mode), C.byref(h)) != 0:
            raise pkg.HlalaError(lib.hlala_bam_last_error().decode(errors="replace"))
        return pkg.SeedBatch(lib, h, long_mode)
    return run


def same_sample(A, B):
    assert A.n_units == B.n_units and A.counts == B.counts and A.names() == B.names()
    a, b = A.to_dict(), B.to_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    p = tmp_path_factory.mktemp("sort_bam") / "t.bam"; write_bam(p, refs, recs, block=3000)
    return p, recs, refs


@pytest.mark.parametrize("hash_bits", [None, "8", "0"])
def test_same_sample_as_the_host_decoder(pkg, decode, bam, monkeypatch, hash_bits):
    p, recs, refs = bam
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    monkeypatch.setenv("HLALA_BAM_DEBUG", "1")                  # the host also checks that neighbours ascend
    if hash_bits is not None:
        monkeypatch.setenv("HLALA_BAM_TEST_HASH_BITS", hash_bits)
    lib = pkg.load_library()
    for long_mode in (False, True):
        for flags in (0, pkg.SEEDS_PACKED):
            H = pkg.bam_open_seeds(lib, p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
            G = decode(p, long_mode=long_mode, flags=flags)
            same_sample(G, H)
            assert G.counts["incomplete"] == H.counts["incomplete"] and G.counts["seeds"] == H.counts["seeds"]
            ordered, merged, by_host = G.sort_counts()
            assert ordered + merged == G.n_units > 100 and by_host == 0 and H.sort_counts() == (0, 0, 0)
            assert (merged == 0) if hash_bits is None else (merged >= 1)
            if hash_bits == "0":
                assert merged > ordered                                 # one hash per partition: nearly every run is collided
            P = decode(p, long_mode=long_mode, flags=flags, sort=False)           # the parent's behaviour: grouped on the device, ordered by the host
            same_sample(P, H)
            assert P.sort_counts() == (0, 0, 0) and P.group_counts()[0] > 0
            G.close(); H.close(); P.close()


def test_the_ways_back_to_the_hosts_sort(pkg, decode, bam, monkeypatch):
    p = bam[0]
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    lib = pkg.load_library()
    H = pkg.bam_open_seeds(lib, p, INTERVALS, threads=3)
    for hash_bits in (None, "0"):
        if hash_bits is not None:
            monkeypatch.setenv("HLALA_BAM_TEST_HASH_BITS", hash_bits)
        G = decode(p, sort_mode=1)                                # the hook reports that it is not available
        same_sample(G, H)
        assert G.sort_counts() == (0, 0, 1) and G.group_counts()[2] == 0
        G.close()
        G = decode(p, refuse_group=True)                          # the group stage handed the sample back: nothing for the device to order
        same_sample(G, H)
        assert G.sort_counts() == (0, 0, 1) and G.group_counts() == (0, 0, 1)
        G.close()
    H.close()


@pytest.mark.parametrize("sort_mode", [2, 3])
def test_an_order_that_is_no_permutation_fails_the_call(pkg, decode, bam, monkeypatch, sort_mode):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    with pytest.raises(pkg.HlalaError, match="BAM name order on the GPU: the order is not a permutation"):
        decode(bam[0], sort_mode=sort_mode)


def test_the_flag_needs_the_group_stage(pkg, bam):
    lib = pkg.load_library()
    with pytest.raises(pkg.HlalaError, match="GPU_SORT needs HLALA_SEEDS_GPU_GROUP"):
        pkg.bam_open_seeds(lib, bam[0], INTERVALS, flags=pkg.SEEDS_GPU_SORT)
