"""The wide fill path without a GPU: the order rule (hla-la_amd/csrc/bam_fill_wide_core.h: fil_sort_wide) and the wide layout of the host model (bam_fill_model.h;
hlala_host_bam_fill_model_wide).  std::sort beyond 16 elements is an introsort and leaves equal scores in an order with no closed form, so nothing here is held against a
Python sort: tools/bam_fill_wide_check.cpp holds the rule against std::sort + std::reverse itself (under ASan / UBSan, and it fails unless adversary inputs reach the heap
sort), and written BAMs whose units have 17 to 4096 alignments on a mate go through the scan, group, name-order and WIDE fill models and must give the host decoder's sample
in every array -- the host decoder calls the real std::sort.  tests/test_gpu_bam_fill_wide.py then holds the device against this model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_fill_cases as F
import bam_fill_wide_cases as W
import bam_scan_cases as K


@pytest.fixture(scope="module")
def model():
    return W.load_model()


def test_abi_additions(pkg):
    lib = pkg.load_library()
    assert pkg.SEEDS_GPU_FILL_WIDE == 64 and pkg.BAM_FILL_WIDE_MAX == W.WIDE_MAX and lib.hlala_abi_version() == pkg.ABI_VERSION == 7
    for s in ("hlala_bam_fill_create_wide", "hlala_bam_fill_wide_stats", "hlala_seed_batch_fill_wide_counts"):
        assert hasattr(lib, s) and s in pkg.EXPORTED_SYMBOLS
    with pytest.raises(pkg.HlalaError, match="GPU_FILL_WIDE needs HLALA_SEEDS_GPU_FILL"):
        pkg.bam_open_seeds(lib, "/nonexistent.bam", [("chr6", 0, 10, 0)], flags=pkg.SEEDS_GPU_FILL_WIDE)


def test_the_cases_hold_what_they_are_named_for():
    c = W.cases()
    sizes = lambda name: [tuple(sum(1 for a in u["als"] if a["mate"] == m) for m in (0, 1)) for u in c[name][0]]
    assert sizes("edge_of_the_paths")[:3] == [(17, 1), (16, 16), (18, 2)] and (32, 1) in sizes("edge_of_the_paths") and (16, 17) in sizes("edge_of_the_paths")
    e = [W.is_wide(u) for u in c["edge_of_the_paths"][0]]
    assert e[0] and e[-1] and not e[1] and e[8:11] == [True, True, True] and e[0:6] == [True, False, True, False, True, False]
    assert [s[0] for s in sizes("strides_of_the_wave")[:5]] == [63, 64, 65, 128, 129]
    assert [max(s) for s in sizes("mates_of_4095_and_4096")] == [4095, 2, 4096]
    assert not any(W.is_wide(u) for u in c["no_wide_unit"][0]) and max(max(s) for s in sizes("no_wide_unit")) == 16
    for u in c["scores"][0][:3]:
        assert len({a["AS"] for a in u["als"]}) == 1
    assert len({a["AS"] for a in c["scores"][0][3]["als"]}) == 2 and all(a["AS"] < 0 for a in c["scores"][0][4]["als"])
    two = [u for u in c["primaries"][0] if u["name"].endswith(b"two")]
    assert all(sum(a["primary"] and a["mate"] == 0 for a in u["als"]) == 2 for u in two)
    assert c["long_reads"][1] and [len(u["als"]) for u in c["long_reads"][0]] == [17, 3, 65, 16]


def test_the_adversary_reaches_the_heap_sort_and_small_mates_keep_the_closed_form(model):
    for n in (64, 100, 256, 1000, 4096):
        order, heaps = W.wide_order(model, W.adversary(n))
        assert heaps >= 1 and sorted(order.tolist()) == list(range(n)), n
        assert (np.diff(W.adversary(n)[order]) <= 0).all()
    rng = np.random.default_rng(3)
    for n in range(0, 17):                                  # up to 16: descending score, equal scores in descending file order (bam_fill_core.h: fil_before)
        s = rng.integers(0, 3, n).astype(np.int32)
        order, heaps = W.wide_order(model, s)
        assert heaps == 0 and order.tolist() == sorted(range(n), key=lambda k: (-int(s[k]), -k))
    assert W.wide_order(model, np.zeros(4097, np.int32))[1] == -1


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name", sorted(W.cases()))
def test_wide_model_on_the_cases(model, name, packed):
    """what can be said without knowing the order of ties: per read the chains are the mate's alignments, scores descending; the primary is a primary of the mate with
    no primary before it; a sample without wide units gives the narrow model's outputs"""
    units, long_mode = W.cases()[name]
    recs, data, first, count, hs = F.build(units, long_mode)
    n = len(units); nm = 1 if long_mode else 2
    rc, off, arr, counts, err, wide = W.run_model(model, recs, data, first, count, hs, long_mode, packed, window=(0, n))
    assert rc == 0, err
    filled = [u for u in units if not u["host"]]
    nw = sum(W.is_wide(u, long_mode) for u in filled)
    assert wide == (nw, nw * nm, max([W.longest(u) for u in filled if W.is_wide(u, long_mode)], default=0))
    co = off["chain_off"]
    for ui, u in enumerate(units):
        for m in range(nm):
            r = ui * nm + m
            als = [a for a in u["als"] if a["mate"] == m]
            assert co[r + 1] - co[r] == len(als)
            if u["host"]:
                continue
            AS = arr["chain_as"][co[r]:co[r + 1]]
            assert sorted(AS.tolist()) == sorted(a["AS"] for a in als) and (np.diff(AS) <= 0).all()
            p = int(arr["read_primary"][r]) - int(co[r])
            assert 0 <= p < len(als) and off["read_off"][r + 1] - off["read_off"][r] in {len(a["codes"]) for a in als if a["primary"] and a["AS"] == AS[p]}
            assert not any(a["primary"] for a in als if a["AS"] > AS[p])
    if nw == 0:
        rcN, offN, arrN, countsN, _ = F.run_model(model, recs, data, first, count, hs, long_mode, packed, window=(0, n))
        assert rcN == 0 and countsN == counts and all(np.array_equal(off[k], offN[k]) for k in off) and all(np.array_equal(arr[k], arrN[k]) for k in arr)
    else:
        assert F.run_model(model, recs, data, first, count, hs, long_mode, packed)[0] == F.E_ARG            # the narrow model keeps refusing them


def test_refusals(pkg, model):
    for name in W.refused():
        recs, data, first, count, hs, text = W.built_refused(name)
        rc, off, arr, counts, err, wide = W.run_model(model, recs, data, first, count, hs)
        assert rc == F.E_ARG and text in err and err.startswith("hlala_host_bam_fill_model_wide: "), (name, err)
    recs, data, first, count, hs = F.build(W.cases()["edge_of_the_paths"][0], False)
    for mm in (0, 16, 4097, -1):
        rc, _, _, _, err, _ = W.run_model(model, recs, data, first, count, hs, max_mate=mm)
        assert rc == F.E_ARG and "max_mate outside (16, 4096]" in err
    rc, _, _, _, err, _ = W.run_model(model, recs, data, first, count, hs, max_mate=32)                      # a cap of the caller's below the library's
    assert rc == F.E_ARG and "than max_mate" in err
    assert W.run_model(model, recs, data, first, count, hs, max_mate=40)[0] == 0
    # the narrow entry keeps its text
    recs, data, first, count, hs, long_mode, *_ = F.apply(F.malformed()["mate_of_17"][0])
    assert "more than 16 alignments" in F.run_model(model, recs, data, first, count, hs)[4]
    for name, (change, text) in sorted(F.malformed().items()):                                            # the present refusals keep their texts on the wide entry
        if name == "mate_of_17":
            continue
        recs, data, first, count, hs, long_mode, n, n_bytes, n_units, n_host = F.apply(change)
        rc, _, _, _, err, _ = W.run_model(model, recs, data, first, count, hs, long_mode, n=n, n_bytes=n_bytes, n_units=n_units, n_host_units=n_host)
        assert rc == F.E_ARG and text in err, (name, err)


def test_check_program_under_sanitizers(model, tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is what builds libhlala_host.so as well"
    exe = tmp_path / "bam_fill_wide_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe),
                           os.path.join(F.ROOT, "tools", "bam_fill_wide_check.cpp")])
    inputs, want = [], []

    def digest(recs, data, first, count, hs, long_mode, packed, n_bytes):
        n = len(first)
        rc, off, arrs, counts, _, wide = W.run_model(model, recs, data, first, count, hs, long_mode, packed, window=(0, n) if n else None, n_bytes=n_bytes)
        h = F.fnv(b"")
        if rc == 0 and n:
            for k in ("read_off", "chain_off", "cigar_count", "name_off"):
                h = F.fnv(off[k].tobytes(), h)
            for k in ("read_primary", "read_bases_packed" if packed else "read_bases", "read_quals", "chain_contig", "chain_pos", "chain_offset", "chain_as", "chain_reverse", "cigar_off_end", "cigar",
                      "name_chars"):
                h = F.fnv(arrs[k].tobytes(), h)
        return [rc] + [counts[f] if rc == 0 else 0 for f in F.COUNT_FIELDS] + [h] + (list(wide) if rc == 0 else [0, 0, 0])
    for name in sorted(W.cases()):
        if name == "mates_of_4095_and_4096":
            continue                                          # (FNV in Python over its arrays takes seconds; the rule at 4095 and 4096 is the program's first part)
        units, long_mode = W.cases()[name]
        recs, data, first, count, hs = F.build(units, long_mode)
        inputs.append((recs, data, first, count, hs, long_mode, name < "m", None)); want.append(digest(*inputs[-1]))
    for name in W.refused():
        recs, data, first, count, hs, text = W.built_refused(name)
        inputs.append((recs, data, first, count, hs, False, False, None)); want.append([F.E_ARG] + [0] * 7 + [F.fnv(b"")] + [0, 0, 0])
    path = tmp_path / "cases.bin"
    F.write_check_file(path, inputs)
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0].startswith("order-rule ") and int(lines[0].split()[1]) > 10000
    adv = dict(x.split(":") for x in lines[1].split()[1:])
    assert lines[1].startswith("adversary ") and sorted(adv, key=int) == ["64", "100", "256", "1000", "4096"] and all(int(v) >= 1 for v in adv.values())
    assert len(lines) - 2 == len(want)
    for line, w in zip(lines[2:], want):
        assert [int(x) for x in line.split()] == w


# ---- written BAMs: the models in a row against the host decoder, which calls std::sort

@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("fill_wide_bams")
    return {k: (d / (k + ".bam"), W.write_wide_bam(d / (k + ".bam"), k)) for k in W.bam_kinds()}


@pytest.mark.parametrize("kind", sorted(W.bam_kinds()))
def test_wide_model_equals_the_host_decoder(pkg, bams, kind):
    from test_bam_fill_model import assert_equals_the_host_sample
    lib = pkg.load_library()
    path, sizes = bams[kind]
    for long_mode, packed in ((False, False), (False, True), (True, True)) if kind != "mate_of_4096" else ((False, True),):
        H = pkg.bam_open_seeds(lib, path, K.INTERVALS, long_read_mode=long_mode, threads=3, flags=pkg.SEEDS_PACKED if packed else 0)
        goff, garr, first, wide = W.sample_through_the_models(pkg, path, long_mode, packed)
        per = np.diff(H.to_dict()["chain_off"]).reshape(-1, 1 if long_mode else 2)
        assert H.n_units == len(first) and not (first == F.HOST).any()
        assert wide[0] == int(((per > 16).any(axis=1) | (per.sum(axis=1) > 32)).sum()) and wide[2] == (per.max() if wide[0] else 0)
        if not long_mode:                                  # (long-read mode keeps the primaries only: the same files, no wide unit)
            assert sorted(tuple(x) for x in per.tolist() if max(x) > 16) == sorted(s for s in sizes if max(s) > 16)
        assert_equals_the_host_sample(H, goff, garr, first, long_mode, packed)
        H.close()
