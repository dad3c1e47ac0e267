"""The decoder's side of HLALA_SEEDS_GPU_GROUP without a GPU: tests/host_cpp/bam_group_hook_model.cpp stands in for the GPU library's hooks (zlib and the scan model for the
round, vectors for the sample-long device arrays, the group model for hlala_bam_group) and calls the decoder of hla-la_amd/csrc/host_bam.cpp as
hlala_bam_extract_seeds_gpu does.  What is checked is the host code around the hooks: rounds kept instead of scattered, the gather through perm with the partition bounds
where the top byte of the hash changes, units built by walking flag, collided runs re-sorted by the host, and every way back to the host's own grouping.
tests/test_gpu_bam_group.py runs the same cases through the real hooks."""
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
    so = tmp_path_factory.mktemp("group_hook_model") / "libgroup_hook_model.so"
    libdir = os.path.join(K.ROOT, "hla-la_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(so), os.path.join(K.ROOT, "tests", "host_cpp", "bam_group_hook_model.cpp"),
                           "-L" + libdir, "-lhlala_gpu", "-Wl,-rpath," + libdir, "-lz"])
    lib = pkg.load_library()
    em = C.CDLL(str(so))
    em.grp_emul.argtypes = [C.c_char_p, C.c_int32, C.POINTER(pkg.BamInterval), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.hlala_bam_last_error.restype = C.c_char_p

    def run(path, intervals=INTERVALS, long_mode=False, flags=0, threads=3, group=True, refuse=False):
        arr = (pkg.BamInterval * len(intervals))()
        for i, (nm, a, b, c) in enumerate(intervals):
            arr[i] = pkg.BamInterval(nm.encode(), a, b, c)
        h = C.c_void_p()
        fl = flags | pkg.SEEDS_GPU_PARSE | (pkg.SEEDS_GPU_GROUP if group else 0)
        if em.grp_emul(str(path).encode(), len(intervals), arr, int(long_mode), threads, fl, int(refuse), C.byref(h)) != 0:
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
    p = tmp_path_factory.mktemp("group_bam") / "t.bam"; write_bam(p, refs, recs, block=3000)
    return p, recs, refs


@pytest.mark.parametrize("hash_bits", [None, "8", "0"])
def test_same_sample_as_the_host_decoder(pkg, decode, bam, monkeypatch, hash_bits):
    p, recs, refs = bam
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    if hash_bits is not None:
        monkeypatch.setenv("HLALA_BAM_TEST_HASH_BITS", hash_bits)
    lib = pkg.load_library()
    for long_mode in (False, True):
        for flags in (0, pkg.SEEDS_PACKED):
            H = pkg.bam_open_seeds(lib, p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
            G = decode(p, long_mode=long_mode, flags=flags)
            same_sample(G, H)
            assert G.counts["incomplete"] == H.counts["incomplete"] and G.counts["seeds"] == H.counts["seeds"]
            grouped, regrouped, by_host = G.group_counts()
            assert grouped == len(K.expect(recs, refs, long_mode)["recs"]) > 400 and by_host == 0 and G.parse_counts()[1] > 3 and H.group_counts() == (0, 0, 0)
            assert (regrouped == 0) if hash_bits is None else (regrouped >= 1)
            P = decode(p, long_mode=long_mode, flags=flags, group=False)          # the parent's behaviour: the same records, none grouped here
            same_sample(P, H)
            assert P.group_counts() == (0, 0, 0)
            G.close(); H.close(); P.close()


def test_the_ways_back_to_the_hosts_grouping(pkg, decode, bam, tmp_path, monkeypatch):
    p = bam[0]
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    lib = pkg.load_library()
    H = pkg.bam_open_seeds(lib, p, INTERVALS, threads=3)
    G = decode(p, refuse=True)                                # the device cannot: every kept round is scattered after all
    same_sample(G, H)
    assert G.group_counts() == (0, 0, 1)
    G.close(); H.close()
    refs, recs = make_records(np.random.default_rng(8), n_names=80)
    drecs, data, at = K.decoy_input("B", 16384, refs, np.random.default_rng(31), K.header(refs))
    q = tmp_path / "decoy.bam"; K.write_bam_file(q, refs, drecs + recs, block=3000)
    H = pkg.bam_open_seeds(lib, q, INTERVALS, threads=3)
    G = decode(q); same_sample(G, H)
    assert G.group_counts()[2] == 0 and G.group_counts()[0] > 0
    G.close()
    monkeypatch.setenv("HLALA_BAM_SCAN_MAX_REHOPS", "0")      # a round falls back to the host's parse: the rounds kept so far are scattered, the later ones as they come
    G = decode(q); same_sample(G, H)
    assert G.parse_counts()[2] >= 1 and G.group_counts() == (0, 0, 1)
    G.close(); H.close()


def test_the_flag_needs_the_record_pass(pkg, bam):
    lib = pkg.load_library()
    with pytest.raises(pkg.HlalaError, match="GPU_GROUP needs HLALA_SEEDS_GPU_PARSE"):
        pkg.bam_open_seeds(lib, bam[0], INTERVALS, flags=pkg.SEEDS_GPU_GROUP)
