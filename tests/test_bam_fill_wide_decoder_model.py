"""The decoder's side of HLALA_SEEDS_GPU_FILL_WIDE without a GPU: tests/host_cpp/bam_fill_wide_hook_model.cpp stands in for the GPU library's six hooks (the five of the fill
decoder test, and for the sixth the gather through the grouping permutation plus the WIDE fill model) and calls the decoder of hla-la_amd/csrc/host_bam.cpp as
hlala_bam_extract_seeds_gpu does.  What is checked is the host code around the hook: with the flag only collided units and units beyond 4096 alignments on a mate stay with
the host, the list of wide units handed over is the one the descriptors give (the stand-in refuses any other), the sample is the host decoder's to the byte -- whose order
of equal scores is std::sort's -- and where the sixth hook is absent or answers "not available" the decoder marks as without the flag and calls the fifth."""
import ctypes as C

import numpy as np
import pytest

import bam_fill_wide_cases as W
import bam_scan_cases as K
from test_bam_fill_decoder_model import same_sample, wide_units

INTERVALS = K.INTERVALS


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return W.hook_model(tmp_path_factory)


@pytest.fixture(scope="module")
def decode(pkg, emul):
    lib = pkg.load_library()
    lib.hlala_bam_last_error.restype = C.c_char_p

    def run(path, long_mode=False, flags=0, threads=3, wide=True, fill=True, fill_mode=0, wide_mode=0):
        arr = (pkg.BamInterval * len(INTERVALS))()
        for i, (nm, a, b, c) in enumerate(INTERVALS):
            arr[i] = pkg.BamInterval(nm.encode(), a, b, c)
        h = C.c_void_p()
        fl = flags | pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP | pkg.SEEDS_GPU_SORT | (pkg.SEEDS_GPU_FILL if fill else 0) | (pkg.SEEDS_GPU_FILL_WIDE if wide else 0)
        if emul.filw_emul(str(path).encode(), len(INTERVALS), arr, int(long_mode), threads, fl, int(fill_mode), int(wide_mode), C.byref(h)) != 0:
            raise pkg.HlalaError(lib.hlala_bam_last_error().decode(errors="replace"))
        return pkg.SeedBatch(lib, h, long_mode)
    return run


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("fill_wide_decoder_bams")
    out = {k: (d / (k + ".bam"), W.write_wide_bam(d / (k + ".bam"), k)) for k in W.bam_kinds()}
    out["beyond"] = (d / "beyond.bam", W.write_beyond_bam(d / "beyond.bam"))
    out["many_names"] = (d / "many.bam", W.write_wide_bam(d / "many.bam", "two_scores", plain=400))        # enough names for hashes to collide once they are cut short
    return out


@pytest.mark.parametrize("kind", sorted(W.bam_kinds()))
def test_same_sample_with_and_without_the_flag(pkg, decode, emul, bams, kind, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                # several rounds
    lib = pkg.load_library()
    path, sizes = bams[kind]
    for flags in (0, pkg.SEEDS_PACKED):
        H = pkg.bam_open_seeds(lib, path, INTERVALS, threads=3, flags=flags)
        w = wide_units(H, False)
        assert w == sum(max(s) > 16 for s in sizes) > 0
        G = decode(path, flags=flags)                                      # the sixth hook: no unit is left to the host
        assert G.fill_counts() == (G.n_units, 0, 0) and G.fill_wide_counts() == (w, 0, max(max(s) for s in sizes)) and (emul.filw_calls(1), emul.filw_calls(0)) == (1, 0)
        same_sample(G, H)
        G.close()
        N = decode(path, flags=flags, wide=False)                          # the parent's behaviour: they are host units
        assert N.fill_counts() == (N.n_units - w, w, 0) and N.fill_wide_counts() == (0, 0, 0) and (emul.filw_calls(1), emul.filw_calls(0)) == (0, 1)
        same_sample(N, H)
        N.close(); H.close()
        assert emul.fil_states() == 0


def test_the_sixth_hook_absent_or_not_available(pkg, decode, emul, bams):
    lib = pkg.load_library()
    path, sizes = bams["two_scores"]
    H = pkg.bam_open_seeds(lib, path, INTERVALS, threads=3)
    w = wide_units(H, False)
    for wide_mode, calls in ((1, (1, 1)), (2, (0, 1))):                     # "not available"; no sixth hook installed: marked as without the flag, the fifth hook fills
        G = decode(path, wide_mode=wide_mode)
        assert G.fill_counts() == (G.n_units - w, w, 0) and G.fill_wide_counts() == (0, 0, 0) and (emul.filw_calls(1), emul.filw_calls(0)) == calls
        same_sample(G, H)
        G.close()
    G = decode(path, wide_mode=1, fill_mode=1)                             # neither hook has an answer: the host lays out and fills the sample
    assert G.fill_counts() == (0, 0, 1) and G.fill_wide_counts() == (0, 0, 0)
    same_sample(G, H)
    G.close(); H.close()


def test_collided_runs_and_long_read_mode(pkg, decode, bams, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    lib = pkg.load_library()
    path, sizes = bams["all_equal"]
    L = pkg.bam_open_seeds(lib, path, INTERVALS, long_read_mode=True, threads=3)
    G = decode(path, long_mode=True)
    assert G.fill_counts()[2] == 0
    same_sample(G, L)
    G.close(); L.close()
    monkeypatch.setenv("HLALA_BAM_TEST_HASH_BITS", "0")                    # one hash per partition: the units of collided runs stay with the host
    path, sizes = bams["many_names"]
    H = pkg.bam_open_seeds(lib, path, INTERVALS, threads=3)
    G = decode(path)
    on_gpu, by_host, whole = G.fill_counts()
    assert whole == 0 and on_gpu + by_host == G.n_units and by_host > 0
    same_sample(G, H)
    G.close(); H.close()


def test_a_mate_beyond_the_cap_stays_with_the_host(pkg, decode, bams):
    lib = pkg.load_library()
    path, sizes = bams["beyond"]
    H = pkg.bam_open_seeds(lib, path, INTERVALS, threads=3, flags=pkg.SEEDS_PACKED)
    G = decode(path, flags=pkg.SEEDS_PACKED)
    assert G.fill_counts() == (G.n_units - 1, 1, 0) and G.fill_wide_counts() == (2, 1, 4097)
    same_sample(G, H)
    G.close(); H.close()


def test_the_flag_without_gpu_fill_is_refused(pkg, decode, bams):
    path, _ = bams["all_equal"]
    with pytest.raises(pkg.HlalaError, match="GPU_FILL_WIDE needs HLALA_SEEDS_GPU_FILL"):
        decode(path, fill=False)
    with pytest.raises(pkg.HlalaError, match="GPU_FILL_WIDE needs HLALA_SEEDS_GPU_FILL"):
        pkg.bam_open_seeds(pkg.load_library(), path, INTERVALS, flags=pkg.SEEDS_GPU_FILL_WIDE)
