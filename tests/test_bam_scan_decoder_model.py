"""The decoder's side of HLALA_SEEDS_GPU_PARSE without a GPU: tests/host_cpp/bam_scan_hook_model.cpp stands in for the GPU library's hooks (zlib for the inflate kernel, the
host model for the record pass, a vector for the device round buffer) and calls the decoder of hla-la_amd/csrc/host_bam.cpp as hlala_bam_extract_seeds_gpu does.  What is
checked is the host code around the hooks: the header read by the host itself, bytes carried from round to round, descriptors turned into the decoder's records, the
fall-back of a round to the host's hop and parse, and the error texts.  tests/test_gpu_bam_scan.py runs the same cases through the real hooks."""
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
    so = tmp_path_factory.mktemp("hook_model") / "libhook_model.so"
    libdir = os.path.join(K.ROOT, "hla-la_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(so), os.path.join(K.ROOT, "tests", "host_cpp", "bam_scan_hook_model.cpp"),
                           "-L" + libdir, "-lhlala_gpu", "-Wl,-rpath," + libdir, "-lz"])
    lib = pkg.load_library()
    em = C.CDLL(str(so))
    em.dec_emul.argtypes = [C.c_char_p, C.c_int32, C.POINTER(pkg.BamInterval), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.hlala_bam_last_error.restype = C.c_char_p

    def run(path, intervals=INTERVALS, long_mode=False, flags=0, threads=3):
        arr = (pkg.BamInterval * len(intervals))()
        for i, (nm, a, b, c) in enumerate(intervals):
            arr[i] = pkg.BamInterval(nm.encode(), a, b, c)
        h = C.c_void_p()
        if em.dec_emul(str(path).encode(), len(intervals), arr, int(long_mode), threads, flags | pkg.SEEDS_GPU_PARSE, C.byref(h)) != 0:
            raise pkg.HlalaError(lib.hlala_bam_last_error().decode(errors="replace"))
        return pkg.SeedBatch(lib, h, long_mode)
    return run


def same_sample(A, B):
    assert A.n_units == B.n_units and A.counts == B.counts and A.names() == B.names()
    a, b = A.to_dict(), B.to_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_same_sample_with_records_across_rounds_and_blocks(pkg, decode, tmp_path, monkeypatch):
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    p = tmp_path / "t.bam"; write_bam(p, refs, recs, block=3000)
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    lib = pkg.load_library()
    for long_mode in (False, True):
        for flags in (0, pkg.SEEDS_PACKED):
            H = pkg.bam_open_seeds(lib, p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
            G = decode(p, long_mode=long_mode, flags=flags)
            same_sample(G, H)
            scanned, rounds, fell_back = G.parse_counts()
            assert scanned == len(recs) and rounds > 3 and fell_back == 0 and H.parse_counts() == (0, 0, 0)
            G.close(); H.close()


def test_a_round_that_falls_back_and_the_rounds_around_it(pkg, decode, tmp_path, monkeypatch):
    refs, recs = make_records(np.random.default_rng(8), n_names=80)
    drecs, data, at = K.decoy_input("B", 16384, refs, np.random.default_rng(31), K.header(refs))
    p = tmp_path / "decoy.bam"; K.write_bam_file(p, refs, drecs + recs, block=3000)
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    lib = pkg.load_library()
    H = pkg.bam_open_seeds(lib, p, INTERVALS, threads=3)
    G = decode(p); same_sample(G, H)
    assert G.parse_counts()[0] == len(drecs) + len(recs) and G.parse_counts()[2] == 0
    G.close()
    monkeypatch.setenv("HLALA_BAM_SCAN_MAX_REHOPS", "0")                     # the first round falls back, a carried record leads into the next, which is scanned
    G = decode(p); same_sample(G, H)
    scanned, rounds, fell_back = G.parse_counts()
    assert fell_back >= 1 and rounds >= 1 and 0 < scanned < len(drecs) + len(recs)
    G.close(); H.close()


def test_file_errors_carry_the_host_decoders_text(pkg, decode, tmp_path):
    lib = pkg.load_library()
    refs = [("chr6", 1000)]; iv = [("chr6", 0, 999, 0)]
    base = dict(name="r", flag=1 | 64, ref=0, pos=10, cigar=[(50, "M")], seq="A" * 50, qual=[30] * 50)
    good = dict(base, name="g", tags=[("AS", "C", 40)])
    for name, r in {"noas": dict(base, tags=[("NM", "C", 0)]), "unp": dict(base, flag=0, tags=[("AS", "C", 40)]), "corrupt": dict(base, tags=[("AS", "C", 40)], corrupt="l_seq"),
                    "tag": dict(base, tags=[("XY", "raw", b"XYi\x01")]), "type": dict(base, tags=[("XQ", "raw", b"XQ?\x01")])}.items():
        p = tmp_path / (name + ".bam"); K.write_bam_file(p, refs, [good, r, good])
        errs = []
        for opener in (lambda: pkg.bam_open_seeds(lib, p, iv, threads=2), lambda: decode(p, iv, threads=2)):
            with pytest.raises(pkg.HlalaError) as e:
                opener()
            errs.append(str(e.value))
        assert errs[0] == errs[1] and errs[0], name
    from test_bam import bgzf_block
    raw = K.serialise([good, good], K.header(refs))[0]
    for cut, text in ((len(raw) - 7, "truncated BAM record"), (20, "truncated BAM reference list"), (6, "truncated BAM header")):
        p = tmp_path / "cut.bam"; p.write_bytes(bgzf_block(raw[:cut]) + bgzf_block(b""))
        errs = []
        for opener in (lambda: pkg.bam_open_seeds(lib, p, iv, threads=2), lambda: decode(p, iv, threads=2)):
            with pytest.raises(pkg.HlalaError) as e:
                opener()
            errs.append(str(e.value))
        assert errs[0] == errs[1] == text
    with pytest.raises(pkg.HlalaError, match="GPU_PARSE"):                   # the flag belongs to the GPU entry point
        pkg.bam_open_seeds(lib, p, iv, flags=pkg.SEEDS_GPU_PARSE)
