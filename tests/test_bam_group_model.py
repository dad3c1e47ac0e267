"""Grouping BAM record descriptors by read name on the host: hlala_host_bam_group_model of libhlala_host.so runs the passes of hla-la_amd/csrc/kernel_bamgroup.hip serially
over the shared core (bam_group_core.h).  Every expected answer comes from the descriptor list (bam_group_cases.expect: sort by (hash, order), split by hash, compare
names).  The malformed inputs run here first, and once more under ASan / UBSan in a stand-alone program (tools/bam_group_check.cpp): the device test hands the same inputs
to hlala_bam_group only because this file shows them refused before a descriptor is followed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_group_cases as G


@pytest.fixture(scope="module")
def model():
    return G.load_model()


@pytest.fixture(scope="module")
def built():
    return G.built_cases()


@pytest.mark.parametrize("name", sorted(G.cases()))
def test_model_equals_the_expectation(model, built, name):
    recs, data = built[name]
    for long_mode in (False, True):
        perm, flag, counts = G.expect(recs, data, long_mode)
        rc, gp, gf, gc, err = G.run_model(model, recs, data, long_mode)
        assert rc == 0 and err == ""
        assert np.array_equal(gp, perm) and np.array_equal(gf, flag) and gc == counts


def test_the_cases_hold_what_they_are_named_for(built):
    """the expectation itself on the cases whose answer is known by construction"""
    e = {k: G.expect(*built[k], False) for k in built}
    assert [len(built[f"n{n}"][0]) for n in (0, 1, 2, 63, 64, 65, 4097)] == [0, 1, 2, 63, 64, 65, 4097]
    assert e["last_byte_full_hash"][2]["n_collided_runs"] == 0 and e["last_byte_full_hash"][2]["n_units_complete"] == 12
    assert e["last_byte_same_hash"][2] == dict(n_recs=24, n_runs=1, n_collided_runs=1, n_units_complete=0, n_units_incomplete=0)
    assert e["prefix_same_hash"][2] == dict(n_recs=8, n_runs=1, n_collided_runs=1, n_units_complete=0, n_units_incomplete=0)
    assert sorted(set(int(x) % 16 for x in built["every_alignment"][0]["rec_off"])) == list(range(16))
    assert e["every_alignment_collided"][2]["n_runs"] == 1
    r3 = built["three_intervals"][0]
    assert len(r3) == 10 and len(set(int(x) for x in r3["rec_off"])) == 6 and e["three_intervals"][2]["n_units_complete"] == 3
    assert e["primary_secondary_mates"][2] == dict(n_recs=32, n_runs=15, n_collided_runs=0, n_units_complete=4, n_units_incomplete=11)
    assert G.expect(*built["primary_secondary_mates"], True)[2]["n_units_complete"] == 8
    assert e["collided_2"][2]["n_collided_runs"] == 1 and e["collided_aba"][2]["n_collided_runs"] == 1
    big = e["collided_5004"]
    assert big[2]["n_runs"] == 3 and big[2]["n_collided_runs"] == 1 and list(np.flatnonzero(big[1])) == [0, 2, 5006]
    w = e["runs_across_wavefronts"][2]
    assert w["n_collided_runs"] == 1 and w["n_units_incomplete"] >= 1


@pytest.mark.parametrize("name", sorted(G.malformed()))
def test_malformed_descriptors_are_refused_before_anything_runs(model, name):
    recs, data, n, n_bytes, text = G.malformed()[name]
    rc, perm, flag, counts, err = G.run_model(model, recs, data, False, n=n, n_bytes=n_bytes)
    assert rc == G.E_ARG and text in err


def test_abi_additions(pkg):
    lib = pkg.load_library()
    assert lib.hlala_abi_sizeof(b"hlala_bam_group_stats") == C.sizeof(pkg.BamGroupStats) == 5 * 8 + 8 * 8
    assert pkg.SEEDS_GPU_GROUP == 8 and lib.hlala_abi_version() == pkg.ABI_VERSION
    for s in ("hlala_bam_group", "hlala_bam_group_rounds", "hlala_seed_batch_group_counts"):
        assert hasattr(lib, s)
    # the flag belongs to the GPU entry point and to HLALA_SEEDS_GPU_PARSE
    with pytest.raises(pkg.HlalaError, match="GPU_GROUP"):
        pkg.bam_open_seeds(lib, "/nonexistent.bam", [("chr6", 0, 10, 0)], flags=pkg.SEEDS_GPU_GROUP)


def test_model_under_sanitizers(model, built, tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is what builds libhlala_host.so as well"
    exe = tmp_path / "bam_group_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe),
                           os.path.join(G.ROOT, "tools", "bam_group_check.cpp")])
    cases, want = [], []
    for name in sorted(built):
        recs, data = built[name]
        for long_mode in (False, True):
            cases.append((recs, data, long_mode, None))
            rc, perm, flag, counts, _ = G.run_model(model, recs, data, long_mode)
            want.append((rc, counts, G.fnv(perm.tobytes()), G.fnv(flag.tobytes())))
    for name, (recs, data, n, n_bytes, _) in sorted(G.malformed().items()):
        if n is not None:
            continue                     # (a count that is not the array's: the library call above; the program sizes its buffers by the count)
        cases.append((recs, data, False, n_bytes))
        want.append((G.E_ARG, dict.fromkeys(G.COUNT_FIELDS, 0), G.fnv(b""), G.fnv(b"")))
    path = tmp_path / "cases.bin"
    G.write_check_file(path, cases)
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(want)
    for line, (rc, counts, hp, hf) in zip(lines, want):
        got = [int(x) for x in line.split()]
        assert got == [rc] + [counts[f] for f in G.COUNT_FIELDS] + [hp, hf]
