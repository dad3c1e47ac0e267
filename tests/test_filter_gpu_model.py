"""The typer's filter stage in the device's formulation, without a device (hla-la_amd/csrc/filter_gpu_model.h over filter_gpu_core.h; hlala_host_filter_model): its
outputs must equal hlala_filter_positions -- the specification, which calls the library's std::sort -- byte for byte and counter for counter, and both the oracle.
tests/test_gpu_filter_positions.py then holds hlala_filter_positions_gpu against the same host function on the same cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import filter_gpu_cases as F
import oracle_binding as ob
from conftest import ROOT


@pytest.fixture(scope="module")
def host(pkg):
    lib = C.CDLL(pkg.LIB_PATH)                      # host code of the product library: no GPU needed
    return lambda e, prm=None: pkg.filter_positions(lib, e, prm)


def test_abi_additions(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "hlala_filter_positions_gpu") and "hlala_filter_positions_gpu" in pkg.EXPORTED_SYMBOLS
    assert pkg.FILTER_GPU_MAX_BUCKET == 4096 == F.MAX_BUCKET
    header = open(os.path.join(ROOT, "include", "hlala_gpu.h")).read()
    assert re.search(r"#define\s+HLALA_FILTER_GPU_MAX_BUCKET\s+4096\b", header) and re.search(r"#define\s+HLALA_ABI_VERSION\s+7\b", header)
    lib.hlala_abi_version.restype = C.c_int
    assert lib.hlala_abi_version() == 7 == pkg.ABI_VERSION


@pytest.mark.parametrize("k", range(len(F.worlds())), ids=[w[0] for w in F.worlds()])
def test_model_matches_host_and_oracle(pkg, oracle, host, k):
    name, e, prm = F.worlds()[k]
    want = host(e, prm)
    F.check_equal(pkg.host_filter_model(e, prm), want, name)
    F.check_equal(ob.filter_positions(e, prm), want, name + " (oracle)")


def test_worlds_exercise_the_filters(host):
    seen = {}
    for name, e, prm in F.worlds():
        for key, v in host(e, prm)[2].items():
            seen[key] = seen.get(key, 0) + v
    assert all(v > 0 for v in seen.values()), seen            # every one of the twelve counters moves somewhere


def test_suite_tells_the_tie_order(pkg, host):
    """more than 20 entries tie at the top weight and carry different alleles: a stable order picks another first 20 than the library's sort.  Judged on the HOST's answer."""
    differ = 0
    for n, minor in F.TIE_BUCKETS:
        e = F.tie_bucket(n, minor)
        assert 21 <= n <= 64 and np.sum(e["read_weighted_ok"][::2] == 1.0) > 20
        want = host(e)
        F.check_equal(pkg.host_filter_model(e, tie_rule=0), want, f"tie bucket {n} {minor}")
        differ += not np.array_equal(pkg.host_filter_model(e, tie_rule=1)[0], want[0])
    assert differ >= 8, differ


@pytest.mark.parametrize("k", range(4), ids=[c[0] for c in F.genotype_cases()])
def test_genotypes(pkg, oracle, host, k):
    name, e, prm = F.genotype_cases()[k]
    want = host(e, prm)
    got = pkg.host_filter_model(e, prm)
    F.check_equal(got, want, name)
    F.check_equal(ob.filter_positions(e, prm), want, name + " (oracle)")
    assert got[3]["buckets"] == 8 and got[3]["largest_bucket"] >= 600
    if "strand" in name:
        assert want[2]["strand_removed_alleles"] > 0 and want[2]["strand_positions_with_removed"] > want[2]["strand_removed_alleles"]


def test_single_buckets_and_adversary(pkg, host):
    for n in (0, 1, 15, 16, 17, 19, 20, 21, 63, 64, 65, 128, 129, 4095, 4096):
        e = F.single_bucket(n)
        got = pkg.host_filter_model(e)
        F.check_equal(got, host(e), f"single bucket {n}")
        assert got[3]["largest_bucket"] == n and got[3]["buckets_sorted"] == (n >= 20)
    for n in (64, 1000, 4096):
        e = F.adversary_bucket(n)
        got = pkg.host_filter_model(e)
        F.check_equal(got, host(e), f"adversary {n}")
        assert got[3]["heap_sorts"] >= 1


@pytest.mark.parametrize("k", range(5), ids=[c[0] for c in F.empty_cases()])
def test_empty_loci(pkg, host, k):
    name, e, prm = F.empty_cases()[k]
    got = pkg.host_filter_model(e, prm)
    F.check_equal(got, host(e, prm), name)
    assert got[3]["buckets"] == 0


@pytest.mark.parametrize("k", range(4), ids=[c[0] for c in F.host_only_cases()])
def test_parameter_edges(pkg, host, k):
    name, e, prm = F.host_only_cases()[k]
    F.check_equal(pkg.host_filter_model(e, prm), host(e, prm), name)


def test_refusals(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    for name, e, prm, code in F.refusals():
        rc, text, use, ign, st, counts = pkg.host_filter_model(e, prm, raw=True)
        assert rc == code, (name, rc, text)
        assert (use == 0xAA).all() and (ign == 0xAA).all(), name                        # nothing written
        if code == F.E_CAPACITY:
            assert text.startswith("not available:") and "4097" in text, text
        if name in F.HOST_REFUSES:
            with pytest.raises(pkg.HlalaError):
                pkg.filter_positions(lib, e, prm)


def test_byte_counts(pkg):
    e = F.genotype_locus()
    nr, np_, nch = e["n_reads"], e["n_pos"], e["n_chars"]
    base = 4 * (nr + 1) + 4 * np_ + np_ + np_ + 4 * (np_ + 1) + nch + 16 * nr       # pos_off, pos_exon, pos_mapq, pos_mate, geno_off, geno_chars, read_weighted_ok
    c = pkg.host_filter_model(e)[3]
    assert c["bytes_up"] == base and c["bytes_down"] == np_ + nr
    c = pkg.host_filter_model(e, pkg.default_filter_params(long_read_strand_filter=1))[3]
    assert c["bytes_up"] == base + 2 * nr                                               # ... and read_reverse with the strand filter


def test_check_program():
    """tools/filter_gpu_check.cpp under ASan / UBSan: the model against hlala_filter_positions on heap buffers of exactly their sizes; it fails unless its adversary
    buckets reach the heap sort and unless a bucket of 4097 is refused"""
    src = os.path.join(ROOT, "hla-la_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", src, "../bin/filter_gpu_check"])
    out = subprocess.run([os.path.join(ROOT, "hla-la_amd", "bin", "filter_gpu_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0].startswith("random ") and int(lines[0].split()[1]) >= 30
    assert lines[1].startswith("single ") and int(lines[1].split()[1]) >= 49
    adv = dict(x.split(":") for x in lines[2].split()[1:])
    assert lines[2].startswith("adversary ") and sorted(adv, key=int) == ["64", "1000", "4096"] and all(int(v) >= 1 for v in adv.values())
    assert lines[3] == "refused 4097"
