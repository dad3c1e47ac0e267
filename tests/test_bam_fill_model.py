"""The layout and the fill on the host: hlala_host_bam_fill_model of libhlala_host.so runs the passes of hla-la_amd/csrc/kernel_bamfill.hip serially over the shared core
(bam_fill_core.h).  Every expected array is a plain-Python statement of the rule (bam_fill_cases.expect: sorted() by score, reversed(), the first primary), which knows
nothing of ranks, lanes or scans.  The malformed inputs run here first, and once more under ASan / UBSan in a stand-alone program (tools/bam_fill_check.cpp), which also
holds the order rule against std::sort + std::reverse for every count up to 16: the device test hands the same inputs to hlala_bam_fill_create only because this file
shows them refused before a record byte is read.  Last, real BAMs go through the scan, group and name-order models and then the fill model, and equal the host decoder's
sample array for array."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_fill_cases as F
import bam_scan_cases as K
from test_bam import make_records, write_bam
from test_bam_fill_decoder_model import second_bam_records, wide_units


@pytest.fixture(scope="module")
def model():
    return F.load_model()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name", sorted(F.cases()))
def test_model_equals_the_expectation(model, name, packed):
    units, long_mode, recs, data, first, count, hs = F.built_case(name)
    off, arr = F.expect(units, long_mode, packed)
    nm = 1 if long_mode else 2
    for w in F.windows(len(units)) or [None]:
        rc, goff, garr, counts, err = F.run_model(model, recs, data, first, count, hs, long_mode, packed, window=w)
        assert rc == 0 and err == ""
        for k in off:
            assert np.array_equal(goff[k], off[k]), k
        if len(units):
            assert counts == dict(n_units=len(units), n_host_units=sum(u["host"] for u in units), n_reads=len(units) * nm, n_chains=int(off["chain_off"][-1]), n_cigar=int(off["cigar_count"][-1]),
                                  n_bases=int(off["read_off"][-1]), n_name_bytes=int(off["name_off"][-1]))
        if w is not None:
            want = F.window_of(off, arr, w[0], w[1], long_mode, packed)
            for k in want:
                assert np.array_equal(garr[k], want[k]), (w, k)


def test_the_cases_hold_what_they_are_named_for():
    c = F.cases()
    assert [len(c[f"units_{n}"][0]) for n in (0, 1, 63, 64, 65, 257)] == [0, 1, 63, 64, 65, 257]
    for k in (1, 2, 15, 16):
        sizes = [sum(a["mate"] == m for a in u["als"]) for u in c[f"mate_{k}"][0] for m in (0, 1)]
        assert k in sizes and max(sizes) <= 16
        u = c[f"mate_{k}_all_equal"][0][0]
        assert len({a["AS"] for a in u["als"]}) == 1 and len(u["als"]) == 2 * k
        order, _ = F.rule(u["als"], 0)
        assert [id(a) for a in order] == [id(a) for a in reversed([a for a in u["als"] if a["mate"] == 0])]       # equal scores: descending file order
    u = c["mate_16_ties_at_the_top"][0][0]
    top = [a["AS"] for a in F.rule(u["als"], 0)[0]]
    assert top[0] == top[1] == top[2] and len(set(top[-4:])) == 4
    for where, at in (("first", 0), ("middle", 3), ("last", 6)):
        u = c[f"primary_{where}"][0][0]
        assert [a["primary"] for a in u["als"] if a["mate"] == 0].index(True) == at
    u = c["two_primaries_of_different_l_seq"][0][0]
    for m in (0, 1):
        ls = [len(a["codes"]) for a in u["als"] if a["mate"] == m and a["primary"]]
        assert len(ls) == 2 and ls[0] != ls[1]
    got = sorted({len(a["codes"]) for u in c["l_seq_edges"][0] for a in u["als"] if a["primary"]})
    assert got == [0, 1, 2, 63, 64, 65, 149, 150, 151, 257]
    u = c["base_codes_and_quality_bytes"][0][0]
    assert set(range(16)) <= set(u["als"][0]["codes"]) and {0, 222, 223, 255} <= set(u["als"][0]["quals"])
    assert sorted({len(a["cigar"]) for u in c["n_cigar_edges"][0] for a in u["als"]}) == [1, 63, 64, 65, 300]
    _, _, recs, _, first, count, _ = F.built_case("n_cigar_edges")
    assert ((recs["rec_off"] + 32 + recs["l_read_name"]) % 2 == 1).any() and len({int(x) % 4 for x in recs["rec_off"] + 32 + recs["l_read_name"]}) > 1
    assert sorted(len(u["name"]) for u in c["name_lengths"][0]) == [1, 2, 254]
    _, _, recs, _, first, _, _ = F.built_case("one_record_two_intervals")
    assert recs["rec_off"][0] == recs["rec_off"][1] and (recs["contig"][0], recs["pos"][0]) != (recs["contig"][1], recs["pos"][1])
    assert [sum(u["host"] for u in c[f"host_units_{k}"][0]) for k in ("none", "first", "last", "every_second", "all")] == [0, 1, 1, 18, 37]
    assert c["host_units_first"][0][0]["host"] and c["host_units_last"][0][-1]["host"]
    assert c["long_reads_65"][1] and all(a["mate"] == 0 for u in c["long_reads_65"][0] for a in u["als"])


@pytest.mark.parametrize("name", sorted(F.malformed()))
def test_malformed_arguments_are_refused_before_anything_runs(model, name):
    change, text = F.malformed()[name]
    recs, data, first, count, hs, long_mode, n, n_bytes, n_units, n_host = F.apply(change)
    rc, off, arrs, counts, err = F.run_model(model, recs, data, first, count, hs, long_mode, n=n, n_bytes=n_bytes, n_units=n_units, n_host_units=n_host)
    assert rc == F.E_ARG and text in err and err.startswith("hlala_host_bam_fill_model: ")
    assert all((a == 0).all() for a in off.values())                 # nothing written


def test_null_arguments_and_no_units(pkg, model):
    units, long_mode, recs, data, first, count, hs = F.built_case("units_1")
    fin, keep = pkg.bam_fill_in(recs, data, first, count, hs)
    off = pkg.bam_fill_offsets(1); st = pkg.BamFillStats()
    f = model.hlala_host_bam_fill_model
    good = [C.byref(fin), off["read_off"].ctypes.data, off["chain_off"].ctypes.data, off["cigar_count"].ctypes.data, off["name_off"].ctypes.data, 0, -1, None, C.byref(st)]
    assert f(*good) == 0
    for at in (0, 1, 2, 3, 4, 8):
        bad = list(good); bad[at] = None
        assert f(*bad) == F.E_ARG and b"null argument" in model.hlala_host_last_error()
    bad = list(good); bad[5:8] = [0, 1, C.byref(pkg.BamFillOut())]
    assert f(*bad) == F.E_ARG and b"null argument" in model.hlala_host_last_error()
    bad = list(good); bad[5:7] = [1, 1]
    assert f(*bad) == F.E_ARG and b"units outside the sample" in model.hlala_host_last_error()
    z = pkg.BamFillStats(); z.n_units = 5; z.ms_wall = 1.0
    empty, _ = pkg.bam_fill_in(recs[:0], data[:0], first[:0], count[:0], hs[:0])
    assert f(C.byref(empty), None, None, None, None, 0, -1, None, C.byref(z)) == 0 and (z.n_units, z.n_chains, z.ms_wall) == (0, 0, 0.0)


def test_abi_additions(pkg):
    lib = pkg.load_library()
    assert lib.hlala_abi_sizeof(b"hlala_bam_fill_stats") == C.sizeof(pkg.BamFillStats) == 9 * 8 + 11 * 8
    assert lib.hlala_abi_sizeof(b"hlala_bam_fill_in") == C.sizeof(pkg.BamFillIn) and lib.hlala_abi_sizeof(b"hlala_bam_fill_out") == C.sizeof(pkg.BamFillOut) == 12 * 8
    assert pkg.SEEDS_GPU_FILL == 32 and lib.hlala_abi_version() == pkg.ABI_VERSION == 7
    for s in ("hlala_bam_fill_create", "hlala_bam_fill_window", "hlala_bam_fill_destroy", "hlala_seed_batch_fill_counts"):
        assert hasattr(lib, s) and s in pkg.EXPORTED_SYMBOLS
    with pytest.raises(pkg.HlalaError, match="GPU_FILL needs HLALA_SEEDS_GPU_SORT"):
        pkg.bam_open_seeds(lib, "/nonexistent.bam", [("chr6", 0, 10, 0)], flags=pkg.SEEDS_GPU_FILL)


def test_model_under_sanitizers(model, tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is what builds libhlala_host.so as well"
    exe = tmp_path / "bam_fill_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe),
                           os.path.join(F.ROOT, "tools", "bam_fill_check.cpp")])
    inputs, want = [], []

    def digest(recs, data, first, count, hs, long_mode, packed, n_bytes):
        n = len(first)
        rc, off, arrs, counts, _ = F.run_model(model, recs, data, first, count, hs, long_mode, packed, window=(0, n) if n else None, n_bytes=n_bytes)
        h = F.fnv(b"")
        if rc == 0 and n:
            for k in ("read_off", "chain_off", "cigar_count", "name_off"):
                h = F.fnv(off[k].tobytes(), h)
            for k in ("read_primary", "read_bases_packed" if packed else "read_bases", "read_quals", "chain_contig", "chain_pos", "chain_offset", "chain_as", "chain_reverse", "cigar_off_end", "cigar",
                      "name_chars"):
                h = F.fnv(arrs[k].tobytes(), h)
        return [rc] + [counts[f] if rc == 0 else 0 for f in F.COUNT_FIELDS] + [h]
    for name in sorted(F.cases()):
        units, long_mode, recs, data, first, count, hs = F.built_case(name)
        for packed in (False, True):
            inputs.append((recs, data, first, count, hs, long_mode, packed, None)); want.append(digest(*inputs[-1]))
    for name, (change, _) in sorted(F.malformed().items()):
        recs, data, first, count, hs, long_mode, n, n_bytes, n_units, n_host = F.apply(change)
        if n is not None or n_units is not None or n_host is not None:
            continue                     # (a count that is not the array's: the library call above; the program sizes its buffers by the counts)
        inputs.append((recs, data, first, count, hs, long_mode, False, n_bytes)); want.append([F.E_ARG] + [0] * 7 + [F.fnv(b"")])
    path = tmp_path / "cases.bin"
    F.write_check_file(path, inputs)
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "order-rule 6400"
    assert len(lines) - 1 == len(want)
    for line, w in zip(lines[1:], want):
        assert [int(x) for x in line.split()] == w


# ---- real BAMs: scan, group and name-order models, then the fill model, against the host decoder

def inflate_bam(path):
    import zlib
    raw = open(path, "rb").read(); out = b""; o = 0
    while o < len(raw):
        bsize = int.from_bytes(raw[o + 16:o + 18], "little") + 1
        out += zlib.decompress(raw[o + 18:o + bsize - 8], -15); o += bsize
    return np.frombuffer(out, np.uint8)


def header_end(data):
    b = data.tobytes(); o = 8 + int.from_bytes(b[4:8], "little"); n_ref = int.from_bytes(b[o:o + 4], "little"); o += 4
    for _ in range(n_ref):
        o += 4 + int.from_bytes(b[o:o + 4], "little") + 4
    return o


def sample_through_the_models(pkg, path, refs, long_mode, packed):
    """the four models in a row, the host's side between them written out here: (offsets, the slices of a window over all units, unit_first, grouped descriptors)"""
    import bam_group_cases as G
    import bam_nameorder_cases as N
    nm = 1 if long_mode else 2
    data = inflate_bam(path)
    rc, recs, comp, st = K.run_model(K.load_model(), data, K.scan_args(refs, long_mode), first=header_end(data), last=True)
    assert rc == 0 and st["status"] == K.OK
    comp = np.frombuffer(comp, np.uint8)
    rc, perm, flag, counts, err = G.run_model(G.load_model(), recs, comp, long_mode)
    assert rc == 0 and counts["n_collided_runs"] == 0
    g = recs[perm]                                                      # the grouped order
    starts = np.nonzero(flag & 1)[0]; ends = np.append(starts[1:], len(g))
    runs = [(int(a), int(z - a)) for a, z in zip(starts, ends) if flag[a] & 4]                  # clean, complete runs: the units, in run order
    off = np.array([int(g["rec_off"][a]) + 32 for a, _ in runs], np.uint64); ln = np.array([int(g["nameLen"][a]) for a, _ in runs], np.uint32)
    rc, order, _, err = N.run_model(N.load_model(), off, ln, comp)
    assert rc == 0
    first, count, hs = [], [], []
    for k in order:
        a, c = runs[int(k)]
        mates = [[i for i in range(a, a + c) if g["which"][i] == m] for m in range(nm)]
        if max(len(x) for x in mates) > pkg.BAM_FILL_MAX_MATE:           # a host unit: its sizes by the rule (one primary per mate in these files)
            first.append(F.HOST)
            for x in mates:
                hs += [int(g["l_seq"][[i for i in x if g["flags"][i] & 2][0]]), len(x), int(g["n_cigar"][x].sum())]
            hs.append(int(g["nameLen"][a]) + 1)
        else:
            first.append(a)
        count.append(c)
    first = np.array(first, np.uint32); count = np.array(count, np.uint32)
    rc, goff, garr, counts, err = F.run_model(F.load_model(), g, comp, first, count, np.array(hs, np.int64), long_mode, packed, window=(0, len(first)))
    assert rc == 0, err
    return goff, garr, first


def assert_equals_the_host_sample(H, goff, garr, first, long_mode, packed):
    nm = 1 if long_mode else 2
    h = H.to_dict(); names = H.names()
    ro, co = goff["read_off"], goff["chain_off"]
    assert np.array_equal(ro, h["read_off"]) and np.array_equal(co, h["chain_off"]) and np.array_equal(goff["cigar_count"], h["cigar_off"][co]) and len(first) == H.n_units
    assert np.array_equal(np.diff(goff["name_off"]), [len(x) + 1 for x in names])
    lut = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)
    for u in range(H.n_units):
        if first[u] == F.HOST:
            continue                                                     # (the model leaves a host unit's ranges alone: the decoder test sees the host fill them)
        assert garr["name_chars"][goff["name_off"][u]:goff["name_off"][u + 1]].tobytes() == names[u].encode() + b"\0"
        for r in range(u * nm, (u + 1) * nm):
            b, c = slice(int(ro[r]), int(ro[r + 1])), slice(int(co[r]), int(co[r + 1]))
            if packed:
                at = (int(ro[r]) + r + 1) >> 1; L = b.stop - b.start
                by = garr["read_bases_packed"][at:at + (L + 1) // 2]; nib = np.empty(2 * len(by), np.uint8); nib[0::2] = by >> 4; nib[1::2] = by & 15
                assert np.array_equal(lut[nib[:L]], h["read_bases"][b])
            else:
                assert np.array_equal(garr["read_bases"][b], h["read_bases"][b])
            assert np.array_equal(garr["read_quals"][b], h["read_quals"][b]) and garr["read_primary"][r] == h["read_primary"][r]
            for k in ("chain_contig", "chain_pos", "chain_offset", "chain_as", "chain_reverse"):
                assert np.array_equal(garr[k][c], h[k][c]), k
            assert np.array_equal(garr["cigar_off_end"][c], h["cigar_off"][c.start + 1:c.stop + 1])
            g = slice(int(h["cigar_off"][c.start]), int(h["cigar_off"][c.stop]))
            assert np.array_equal(garr["cigar"][g], h["cigar"][g])


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("fill_model_bams")
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    write_bam(d / "t.bam", refs, recs, block=3000)
    refs2, recs2, w2 = second_bam_records()
    write_bam(d / "w.bam", refs2, recs2, block=3000)
    return d / "t.bam", d / "w.bam", w2


@pytest.mark.parametrize("long_mode", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_real_bams_through_the_models_equal_the_host_decoder(pkg, bams, long_mode, packed):
    t, wbam, w2 = bams
    lib = pkg.load_library()
    refs = [("chr6", 50000), ("chrUn", 9000), ("HLA-A*01", 4000)]
    for path, want_w in ((t, None), (wbam, w2)):
        H = pkg.bam_open_seeds(lib, path, K.INTERVALS, long_read_mode=long_mode, threads=3, flags=pkg.SEEDS_PACKED if packed else 0)
        goff, garr, first = sample_through_the_models(pkg, path, refs, long_mode, packed)
        w = int((first == F.HOST).sum())
        assert w == wide_units(H, long_mode) and w < H.n_units / 10 and H.n_units > 40
        if want_w is not None and not long_mode:
            assert w == want_w
        assert_equals_the_host_sample(H, goff, garr, first, long_mode, packed)
        H.close()
