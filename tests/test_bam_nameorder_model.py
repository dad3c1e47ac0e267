"""Ordering names on the host: hlala_host_bam_name_order_model of libhlala_host.so runs the passes of hla-la_amd/csrc/kernel_bamnameorder.hip serially over the shared core
(bam_nameorder_core.h).  Every expected answer is Python's own sorted() on the names as bytes objects (bam_nameorder_cases.expect), which knows nothing of rounds, keys or
segments.  The malformed inputs run here first, and once more under ASan / UBSan in a stand-alone program (tools/bam_nameorder_check.cpp): the device test hands the same
inputs to hlala_bam_name_order only because this file shows them refused before a name is read."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bam_nameorder_cases as N


@pytest.fixture(scope="module")
def model():
    return N.load_model()


@pytest.fixture(scope="module")
def built():
    return N.built_cases()


@pytest.mark.parametrize("name", sorted(N.cases()))
def test_model_equals_the_expectation(model, built, name):
    off, ln, data, (order, n_rounds, n_equal) = built[name]
    rc, got, counts, err = N.run_model(model, off, ln, data)
    assert rc == 0 and err == ""
    assert np.array_equal(got, order)
    assert counts == dict(n=len(off), n_rounds=n_rounds, n_equal_names=n_equal)


def test_the_cases_hold_what_they_are_named_for(built):
    """the expectation itself on the cases whose answer is known by construction"""
    src = open(os.path.join(N.ROOT, "hla-la_amd", "csrc", "bam_nameorder_core.h")).read()
    assert int(re.search(r"constexpr uint32_t NAM_W = (\d+);", src).group(1)) == N.W
    assert [len(built[f"n{n}"][0]) for n in (0, 1, 2, 63, 64, 65, 129)] == [0, 1, 2, 63, 64, 65, 129]
    assert built["n0"][3][1] == 0 and built["n1"][3][1] == 1
    for d in (N.W - 1, N.W, N.W + 1, 2 * N.W - 1, 2 * N.W, 2 * N.W + 1):
        assert built[f"differ_at_{d}"][3][1] == d // N.W + 1
    off, ln, data, (order, n_rounds, n_equal) = built["nul_tails"]
    assert [N.names_of(off, ln, data)[i] for i in order] == [b"ab", b"ab\0", b"ab\0\0", b"ab\0c"]
    off, ln, data, (order, n_rounds, n_equal) = built["w_prefix_of_2w"]
    assert sorted(int(x) for x in ln) == [2, N.W, 2 * N.W] and n_rounds == 2
    off, ln, data, (order, n_rounds, n_equal) = built["equal_130"]
    assert list(order) == list(range(130)) and n_equal == 129 and n_rounds == len("one-name-130") // N.W + 1
    assert built["equal_triples"][3][2] == 10 * 2 + 2 and len(built["equal_triples"][0]) == 523
    assert len(built["compaction"][0]) == 8000 and built["compaction"][3][1] >= 24 // N.W + 1
    assert built["long_300"][3][1] == 299 // N.W + 1 and built["long_4096"][3][1] == 4095 // N.W + 1 == 586
    assert int(built["long_65535"][1].max()) == 65535 and built["long_65535"][3][1] <= 3
    assert sorted(set(int(x) % 8 for x in built["every_alignment"][0])) == list(range(8))
    assert built["overlapping"][3][2] >= 30
    off, ln, data, _ = built["last_ends_the_buffer"]
    assert int((off + ln).max()) == len(data)
    assert len(built["realistic_20000"][0]) == 20000 and built["realistic_20000"][3][2] == 0


@pytest.mark.parametrize("name", sorted(N.malformed()))
def test_malformed_arguments_are_refused_before_anything_runs(model, name):
    off, ln, data, n, n_bytes, text = N.malformed()[name]
    rc, order, counts, err = N.run_model(model, off, ln, data, n=n, n_bytes=n_bytes)
    assert rc == N.E_ARG and text in err and err.startswith("hlala_host_bam_name_order_model: ")


def test_null_arguments_are_refused(pkg, model):
    off, ln, data = N.cases()["n2"]
    o, k, d = off.copy(), ln.copy(), data.copy(); order = np.zeros(2, np.uint32); st = pkg.BamNameOrderStats()
    f = model.hlala_host_bam_name_order_model
    good = [o.ctypes.data, k.ctypes.data, 2, d.ctypes.data, d.size, order.ctypes.data, C.byref(st)]
    assert f(*good) == 0
    for at in (0, 1, 3, 5, 6):
        bad = list(good); bad[at] = None
        assert f(*bad) == N.E_ARG and b"null argument" in model.hlala_host_last_error()
    z = pkg.BamNameOrderStats(); z.n = 5; z.ms_wall = 1.0
    assert f(None, None, 0, None, 0, None, C.byref(z)) == 0 and (z.n, z.n_rounds, z.n_equal_names) == (0, 0, 0)


def test_abi_additions(pkg):
    lib = pkg.load_library()
    assert lib.hlala_abi_sizeof(b"hlala_bam_name_order_stats") == C.sizeof(pkg.BamNameOrderStats) == 3 * 8 + 7 * 8
    assert pkg.SEEDS_GPU_SORT == 16 and lib.hlala_abi_version() == pkg.ABI_VERSION
    for s in ("hlala_bam_name_order", "hlala_seed_batch_sort_counts"):
        assert hasattr(lib, s) and s in pkg.EXPORTED_SYMBOLS
    # the flag belongs to the GPU entry point and to HLALA_SEEDS_GPU_GROUP
    with pytest.raises(pkg.HlalaError, match="GPU_"):
        pkg.bam_open_seeds(lib, "/nonexistent.bam", [("chr6", 0, 10, 0)], flags=pkg.SEEDS_GPU_SORT)


def test_model_under_sanitizers(model, built, tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is what builds libhlala_host.so as well"
    exe = tmp_path / "bam_nameorder_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe),
                           os.path.join(N.ROOT, "tools", "bam_nameorder_check.cpp")])
    cases, want = [], []
    for name in sorted(built):
        off, ln, data, _ = built[name]
        cases.append((off, ln, data, None))
        rc, order, counts, _ = N.run_model(model, off, ln, data)
        want.append([rc] + [counts[f] for f in N.COUNT_FIELDS] + [N.fnv(order.tobytes())])
    for name, (off, ln, data, n, n_bytes, _) in sorted(N.malformed().items()):
        if n is not None:
            continue                     # (a count that is not the array's: the library call above; the program sizes its buffers by the count)
        cases.append((off, ln, data, n_bytes))
        want.append([N.E_ARG, 0, 0, 0, N.fnv(b"")])
    path = tmp_path / "cases.bin"
    N.write_check_file(path, cases)
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(want)
    for line, w in zip(lines, want):
        assert [int(x) for x in line.split()] == w
