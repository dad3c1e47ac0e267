"""The decoder's side of hlala_seed_batch_create_resident without a GPU: tests/host_cpp/bam_resident_hook_model.cpp stands in for the GPU library's hooks (the six of the wide
fill decoder test) and for the `resident` function of the fill handle, and calls the decoder's entry of hla-la_amd/csrc/host_bam.cpp (seed_batch_resident) as the GPU library does.
What is checked is the host code around the function: the host units it fills and hands over (the stand-in places the ranges of the units ITS state knows as host units, so a
unit the decoder forgot comes out wrong), src->host NULL where the window holds none, the names it copies, the units accounted as handed out by either route, the release with
the last unit, what hlala_seed_batch_window answers afterwards, and every "not available".  The window the stand-in builds must be the host decoder's, and what
hlala_host_batch_resident_model makes of it the same.  tests/test_gpu_bam_resident_decoder.py runs the same walks through the real library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bam_resident_cases as R
import bam_scan_cases as K
from test_bam import make_records, write_bam
from test_bam_fill_decoder_model import same_sample, second_bam_records

INTERVALS = K.INTERVALS
NCT = 3                                         # contigs of the stand-in's "context": the intervals' contig numbers are 0, 1, 2
WINDOW_KEYS = ("read_off", "read_bases", "read_quals", "chain_off", "read_primary", "chain_contig", "chain_pos", "chain_offset", "chain_as", "chain_reverse", "cigar_off", "cigar")
WINDOW_TYPES = (np.int64, np.uint8, np.uint8, np.int64, np.int32, np.int32, np.int32, np.int32, np.int32, np.uint8, np.int64, np.uint32)
E_ARG, E_STATE = -1, -5
CTX = 0x5EED                                    # the stand-in only records it


@pytest.fixture(scope="module")
def emul(pkg, tmp_path_factory):
    so = tmp_path_factory.mktemp("resident_hook_model") / "libresident_hook_model.so"
    libdir = os.path.join(K.ROOT, "hla-la_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(so), os.path.join(K.ROOT, "tests", "host_cpp", "bam_resident_hook_model.cpp"),
                           "-L" + libdir, "-lhlala_gpu", "-Wl,-rpath," + libdir, "-lz"])
    em = C.CDLL(str(so))
    em.res_emul.argtypes = [C.c_char_p, C.c_int32, C.POINTER(pkg.BamInterval)] + [C.c_int32] * 6 + [C.POINTER(C.c_void_p)]
    em.res_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(pkg.BatchFillStats), C.c_char_p, C.c_int32]
    em.res_batch_array.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]; em.res_batch_array.restype = C.c_int64
    em.res_batch_free.argtypes = [C.c_void_p]; em.res_batch_free.restype = None
    em.res_call.argtypes = [C.c_int, C.POINTER(C.c_int64)]; em.res_call.restype = None
    return em


@pytest.fixture(scope="module")
def model():
    return R.load_model()


@pytest.fixture(scope="module")
def decode(pkg, emul):
    lib = pkg.load_library()
    lib.hlala_bam_last_error.restype = C.c_char_p

    def run(path, long_mode=False, flags=0, threads=3, wide=True, fill=True, fill_mode=0, res_mode=0, nct=NCT):
        arr = (pkg.BamInterval * len(INTERVALS))()
        for i, (nm, a, b, c) in enumerate(INTERVALS):
            arr[i] = pkg.BamInterval(nm.encode(), a, b, c)
        h = C.c_void_p()
        fl = flags | pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP | pkg.SEEDS_GPU_SORT | (pkg.SEEDS_GPU_FILL if fill else 0) | (pkg.SEEDS_GPU_FILL_WIDE if fill and wide else 0)
        if emul.res_emul(str(path).encode(), len(INTERVALS), arr, int(long_mode), threads, fl, int(fill_mode), int(res_mode), int(nct), C.byref(h)) != 0:
            raise pkg.HlalaError(lib.hlala_bam_last_error().decode(errors="replace"))
        return pkg.SeedBatch(lib, h, long_mode)
    return run


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    p = tmp_path_factory.mktemp("resident_bam") / "t.bam"; write_bam(p, refs, recs, block=3000)
    return p


@pytest.fixture(scope="module")
def bam17(tmp_path_factory):
    refs, recs, w = second_bam_records()                    # two units with a mate of 17 alignments: host units without the WIDE flag
    p = tmp_path_factory.mktemp("resident_bam17") / "w.bam"; write_bam(p, refs, recs, block=3000)
    return p, w


def create(pkg, emul, G, u0, n):
    """(return code, text, stand-in batch or None, stats)"""
    b = C.c_void_p(); st = pkg.BatchFillStats(); text = C.create_string_buffer(512)
    rc = emul.res_create(G.h, C.c_void_p(CTX), int(u0), int(n), C.byref(b), C.byref(st), text, 512)
    return rc, text.value.decode(), (b if b.value else None), st


def batch_arrays(emul, b):
    out = {}
    for i, (k, dt) in enumerate(zip(WINDOW_KEYS, WINDOW_TYPES)):
        p = C.c_void_p(); n = emul.res_batch_array(b, i, C.byref(p))
        out[k] = np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), (n,)).copy() if n > 0 else np.zeros(0, dt)
    for i, k in enumerate(R.RULE_KEYS):
        p = C.c_void_p(); n = emul.res_batch_array(b, 13 + i, C.byref(p))
        out["m_" + k] = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (n,)).copy()
    return out


def last_call(emul):
    c = (C.c_int64 * 6)(); emul.res_call(emul.res_n_calls() - 1, c)
    return dict(zip(("ctx", "u0", "n", "host_null", "host_units", "rc"), [int(x) for x in c]))


def resident_window(pkg, emul, model, G, H, u0, n, nct=NCT):
    """one window built resident: the stand-in's batch is the host decoder's window, the model's answer the one for that window; returns the host units in it"""
    rc, text, b, st = create(pkg, emul, G, u0, n)
    assert rc == 0, text
    call = last_call(emul)
    assert (call["ctx"], call["u0"], call["n"], call["rc"]) == (CTX, u0, n, 0)
    assert call["host_null"] == (call["host_units"] == 0)                  # src->host is NULL exactly where the window holds no host unit
    want = H.to_dict(u0, n); got = batch_arrays(emul, b)
    emul.res_batch_free(b)
    for k in WINDOW_KEYS:
        assert np.array_equal(got[k], np.asarray(want[k])), (u0, n, k)
    d = {k: v for k, v in want.items() if k != "first_chain"}
    mrc, mtext, marr, first = R.run_model(model, d, nct, G.long_read_mode)
    assert mrc == 0, mtext
    for k in R.RULE_KEYS:
        assert np.array_equal(got["m_" + k][:len(marr[k])], marr[k]), (u0, n, k)
    assert (st.n_units, st.n_host_units, st.n_chains) == (n, call["host_units"], want["n_chains"])
    assert G.names(u0, n) == H.names(u0, n)
    return call["host_units"]


def cuts(n, step=50):
    return [(a, min(step, n - a)) for a in range(0, n, step)]


HOST_UNIT_CASES = ("collided", "mate_of_17", "none")


def open_case(pkg, decode, bam, bam17, monkeypatch, case, flags=0, long_mode=False, **kw):
    """(G, H, host units): the three ways a sample comes by host units -- collided hash runs, a mate of 17 alignments without the WIDE flag, none with it"""
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                # several rounds
    lib = pkg.load_library()
    if case == "collided":
        monkeypatch.setenv("HLALA_BAM_TEST_HASH_BITS", "8")
    path = bam17[0] if case == "mate_of_17" else bam
    H = pkg.bam_open_seeds(lib, path, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
    G = decode(path, long_mode=long_mode, flags=flags, wide=case != "mate_of_17", **kw)
    return G, H, G.fill_counts()[1]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("case", HOST_UNIT_CASES)
def test_every_window_resident(pkg, decode, emul, model, bam, bam17, monkeypatch, case, packed):
    G, H, by_host = open_case(pkg, decode, bam, bam17, monkeypatch, case, flags=pkg.SEEDS_PACKED if packed else 0)
    n = G.n_units
    assert G.fill_counts()[2] == 0 and {"collided": by_host > 0, "mate_of_17": by_host == bam17[1], "none": by_host == 0}[case]
    ws = cuts(n)
    assert len(ws) > 1 or case == "mate_of_17"
    seen = 0
    for i, (u0, k) in enumerate(ws):
        assert emul.fil_states() == 1 and emul.res_destroyed() == 0           # units remain: the state is alive
        seen += resident_window(pkg, emul, model, G, H, u0, k)
    assert seen == by_host                                                    # the host units handed over are the sample's, each in its window
    assert emul.fil_states() == 0 and emul.res_destroyed() == 1               # released with the last unit, once
    assert G.resident_counts() == (len(ws), n, 10 * by_host, 0)
    assert G.names() == H.names()
    # after the release: nothing is available, and the host arrays of units that only went out resident were never written
    rc, text, b, _ = create(pkg, emul, G, 0, 1)
    assert rc == E_STATE and text.startswith("not available:") and b is None and G.resident_counts()[3] == 1
    with pytest.raises(pkg.HlalaError, match="only handed out as resident windows"):
        G.window(0, 1)
    with pytest.raises(pkg.HlalaError, match="only handed out as resident windows"):
        G.window(n - 3, 3)
    d = pkg.BatchIn()
    assert G.lib.hlala_seed_batch_window(G.h, 0, 1, C.byref(d)) == E_STATE and G.lib.hlala_seed_batch_desc(G.h, C.byref(d), None) == E_STATE
    G.close(); H.close()
    assert emul.res_destroyed() == 1


def test_long_read_mode(pkg, decode, emul, model, bam, bam17, monkeypatch):
    for case in ("collided", "none"):
        G, H, by_host = open_case(pkg, decode, bam, bam17, monkeypatch, case, long_mode=True)
        seen = sum(resident_window(pkg, emul, model, G, H, u0, k) for u0, k in cuts(G.n_units))
        assert seen == by_host and emul.fil_states() == 0 and emul.res_destroyed() == 1 and G.names() == H.names()
        G.close(); H.close()
        monkeypatch.delenv("HLALA_BAM_TEST_HASH_BITS", raising=False)


def test_window_shapes(pkg, decode, emul, model, bam, bam17, monkeypatch):
    """empty windows at both ends, the first and the last unit alone, a window twice, windows in descending order, the whole sample"""
    G, H, by_host = open_case(pkg, decode, bam, bam17, monkeypatch, "collided", flags=pkg.SEEDS_PACKED)
    n = G.n_units
    for u0, k in ((0, 0), (n, 0)):
        rc, text, b, st = create(pkg, emul, G, u0, k)
        assert rc == 0 and b is not None and st.n_units == 0 and last_call(emul)["host_null"] == 1
        emul.res_batch_free(b)
    assert create(pkg, emul, G, n, 1)[0] == E_ARG and create(pkg, emul, G, -1, 1)[0] == E_ARG
    seen = resident_window(pkg, emul, model, G, H, 0, 1) + resident_window(pkg, emul, model, G, H, n - 1, 1)
    assert resident_window(pkg, emul, model, G, H, 0, 1) + resident_window(pkg, emul, model, G, H, n - 1, 1) == seen        # twice: legal and equal
    assert resident_window(pkg, emul, model, G, H, 30, 50) == resident_window(pkg, emul, model, G, H, 30, 50)
    assert emul.fil_states() == 1
    ws = [(u0, k) for u0, k in reversed(cuts(n - 2, 50))]                  # descending, over [1, n - 1): with the two single units that is every unit
    for i, (u0, k) in enumerate(ws):
        assert emul.fil_states() == 1
        resident_window(pkg, emul, model, G, H, u0 + 1, k)
    assert emul.fil_states() == 0 and emul.res_destroyed() == 1
    assert G.resident_counts()[:2] == (2 + 4 + 2 + len(ws), 4 + 100 + n - 2) and G.names() == H.names()
    G.close()
    G = decode(bam, flags=pkg.SEEDS_PACKED)                                # the whole sample as one window
    assert resident_window(pkg, emul, model, G, H, 0, n) == by_host
    assert emul.fil_states() == 0 and emul.res_destroyed() == 1
    G.close(); H.close()


def test_host_path_and_resident_windows_interleaved(pkg, decode, emul, model, bam, bam17, monkeypatch):
    """chunks of the fill are 16 units here: windows of either route share chunks; a chunk counts once, when its last unit has been handed out either way"""
    G, H, by_host = open_case(pkg, decode, bam, bam17, monkeypatch, "collided")
    n = G.n_units
    assert max(16, min(8192, n // 24 + 1)) == 16                            # (UCH of host_bam.cpp for 3 threads: the windows below straddle chunks)

    def host_window(u0, k):
        a, b = G.to_dict(u0, k), H.to_dict(u0, k)
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (u0, k, key)
    host_window(20, 10)                                                     # the host path fills the chunk of units 16 .. 31
    resident_window(pkg, emul, model, G, H, 0, 25)                          # chunk 0 went out resident only, chunk 1 both ways
    host_window(0, 16)                                                      # before the release the host path fills resident-only units, correctly
    host_window(10, 30)
    resident_window(pkg, emul, model, G, H, 60, n - 60)
    assert emul.fil_states() == 1                                           # units 48 .. 59 of chunk 3 have not been handed out (chunk 2 went through the host)
    resident_window(pkg, emul, model, G, H, 25, 20)
    assert emul.fil_states() == 1
    resident_window(pkg, emul, model, G, H, 45, 15)
    assert emul.fil_states() == 0 and emul.res_destroyed() == 1             # ... now they have
    host_window(0, 48)                                                      # chunks the host wrote stay readable
    assert G.names() == H.names()
    with pytest.raises(pkg.HlalaError, match="only handed out as resident windows"):
        G.window(30, 40)
    G.close()
    # the other way round: the host path hands out the last units
    G = decode(bam)
    resident_window(pkg, emul, model, G, H, 5, 100)
    assert emul.fil_states() == 1
    host_window(0, n)                                                       # fills everything, resident or not
    assert emul.fil_states() == 0 and emul.res_destroyed() == 1
    same_sample(G, H)
    rc, text, b, _ = create(pkg, emul, G, 0, 10)
    assert rc == E_STATE and text.startswith("not available:")
    G.close(); H.close()


def test_not_available(pkg, decode, emul, bam, bam17, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    lib = pkg.load_library()
    H = pkg.bam_open_seeds(lib, bam, INTERVALS, threads=3)
    for kw in (dict(fill=False), dict(fill_mode=1, wide=False), dict(res_mode=1)):      # without the flag; the sample handed back to the host; a handle without a resident function
        G = decode(bam, **kw)
        calls = emul.res_n_calls()
        rc, text, b, _ = create(pkg, emul, G, 0, 50)
        assert rc == E_STATE and text.startswith("not available:") and b is None and emul.res_n_calls() == calls == 0
        assert G.resident_counts() == (0, 0, 0, 1)
        same_sample(G, H)                                                    # the caller takes the host route: nothing was changed
        G.close()
    assert emul.fil_states() == 0
    # the function itself answers "not available" (a context on another device): counted, nothing handed out, the state stays
    G = decode(bam)
    emul.res_set_refuse(1)
    rc, text, b, _ = create(pkg, emul, G, 0, G.n_units)
    emul.res_set_refuse(0)
    assert rc == E_STATE and text.startswith("not available:") and b is None and G.resident_counts() == (0, 0, 0, 1) and emul.fil_states() == 1
    same_sample(G, H)
    assert emul.fil_states() == 0
    G.close(); H.close()


def test_a_refused_window_is_not_handed_out(pkg, decode, emul, model, bam, bam17, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    lib = pkg.load_library()
    H = pkg.bam_open_seeds(lib, bam, INTERVALS, threads=3)
    G = decode(bam, nct=0)                                                  # a context without contigs for these chains: hlala_batch_create refuses the window
    n = G.n_units
    d = {k: v for k, v in H.to_dict(0, n).items() if k != "first_chain"}
    mrc, mtext, _, _ = R.run_model(model, d, 0, False)
    rc, text, b, _ = create(pkg, emul, G, 0, n)
    assert rc == mrc == E_ARG and text == mtext == R.TEXT["contig"] and b is None
    assert G.resident_counts() == (0, 0, 0, 0) and emul.fil_states() == 1  # its code and text; nothing counted
    same_sample(G, H)
    assert emul.fil_states() == 0
    G.close(); H.close()


def test_without_a_resident_window_nothing_changes(pkg, decode, emul, bam, bam17, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    lib = pkg.load_library()
    for flags in (0, pkg.SEEDS_PACKED):
        H = pkg.bam_open_seeds(lib, bam, INTERVALS, threads=3, flags=flags)
        G = decode(bam, flags=flags)
        same_sample(G, H)
        assert emul.res_n_calls() == 0 and G.resident_counts() == (0, 0, 0, 0) and emul.fil_states() == 0 and emul.res_destroyed() == 1
        G.close(); H.close()


def test_a_peeked_window_is_not_handed_out(pkg, decode, emul, model, bam, bam17, monkeypatch):
    """hlala_seed_batch_peek_window (the insert-size estimate of the host program): the whole of a small sample is filled into the host arrays and the fill state lives on"""
    G, H, by_host = open_case(pkg, decode, bam, bam17, monkeypatch, "collided", flags=pkg.SEEDS_PACKED)
    n = G.n_units
    d = G.window(0, n, peek=True); w = H.window(0, n)
    assert d.n_chains == w.n_chains and emul.fil_states() == 1 and emul.res_destroyed() == 0          # every chunk is filled, none counts
    ws = cuts(n)
    for i, (u0, k) in enumerate(ws):
        assert emul.fil_states() == 1
        resident_window(pkg, emul, model, G, H, u0, k)                       # legal over peeked units, and equal
    assert emul.fil_states() == 0 and emul.res_destroyed() == 1 and G.resident_counts()[:2] == (len(ws), n)
    same_sample(G, H)                                                       # the host arrays were written by the peek: they stay readable after the release
    G.close()
    # peeked units handed out by the host route count then
    G = decode(bam, flags=pkg.SEEDS_PACKED)
    G.window(0, 100, peek=True)
    resident_window(pkg, emul, model, G, H, 50, 100)
    a, b = G.to_dict(0, 160), H.to_dict(0, 160)                            # ten chunks of 16, peeked or not
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert emul.fil_states() == 1                                           # the chunks behind them hold units nobody has asked for
    G.window(160, n - 160)
    assert emul.fil_states() == 0 and emul.res_destroyed() == 1
    G.close()
    # a sample that builds no resident windows: a peek is a window like every other
    G = decode(bam, flags=pkg.SEEDS_PACKED, res_mode=1)
    G.window(0, n, peek=True)
    assert emul.fil_states() == 0
    same_sample(G, H)
    G.close(); H.close()
