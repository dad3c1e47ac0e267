"""The BAM record pass on the GPU (hla-la_amd/csrc/kernel_bamscan.hip: k_bam_guess, k_bam_link, k_bam_starts, k_bam_parse, k_bam_scan2, k_bam_emit) behind hlala_bam_scan
and Inflater.bam_scan.  Every input of tests/test_bam_scan_model.py, valid and malformed, goes through the device; descriptors, compact bytes and every integer field of
the stats (the re-hops included) must equal the host model's bit for bit at each slice size, and the valid ones the expectation written from the record list.  The
malformed inputs go to the device only because the model test shows the shared core bounded on them: here they check the status reporting, not fault behaviour."""
import struct

import numpy as np
import pytest

import bam_scan_cases as K

pytestmark = pytest.mark.gpu
SLICES = (64, 256, 4096, 0)


@pytest.fixture(scope="module")
def model():
    return K.load_model()


@pytest.fixture(scope="module")
def valid():
    return K.valid_cases()


@pytest.fixture(scope="module")
def inflater(pkg):
    f = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    yield f
    f.close()


def eff(S):
    return S or 16384


def both(model, inflater, data, refs, first=0, last=False, cap_recs=None, cap_compact=None, **kw):
    """the call on the device and in the model: everything equal (canaries: K.check_outputs); returns the device's (rc, descriptors, compact, stats)"""
    want = K.run_model(model, data, K.scan_args(refs, **kw), first=first, last=last, cap_recs=cap_recs, cap_compact=cap_compact)
    a, keep = K.scan_args(refs, **kw)
    cr, cc = K.caps(data, a.n_intervals)
    buf = np.frombuffer(bytes(data), np.uint8)
    rc, recs, comp, st = inflater.bam_scan(buf, a, first=first, last=last, cap_recs=cr if cap_recs is None else cap_recs, cap_compact=cc if cap_compact is None else cap_compact,
                                           guard=K.GUARD, canary=K.CANARY)
    got = (rc,) + K.check_outputs(rc, recs, comp, st)
    assert got[0] == want[0] and got[3] == want[3], (got[3], want[3])
    assert got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
    return got


@pytest.mark.parametrize("S", SLICES)
def test_valid_inputs_equal_model_and_expectation(model, inflater, valid, S):
    for name, recs, data, first, refs, kw in valid:
        exp = K.expect(recs, refs, kw.get("long_mode", False), kw.get("hash_mask", K.M64), kw.get("first_seq", 0))
        for last in (False, True):
            got = both(model, inflater, data, refs, first=first, last=last, slice_bytes=S, **kw)
            K.assert_equals_expectation(got, exp, data, len(recs), len(data), eff(S))
    _, recs, data, _, refs, _ = valid[0]
    starts = K.serialise(recs)[1]
    for k in (1, 7, len(recs) - 1, len(recs)):                                              # `first` at a few offsets
        got = both(model, inflater, data, refs, first=starts[k] if k < len(recs) else len(data), slice_bytes=S)
        K.assert_equals_expectation(got, K.expect(recs[k:], refs), data, len(recs) - k, len(data), eff(S))


def test_device_times_are_reported(pkg, inflater, valid):
    _, recs, data, _, refs, _ = valid[0]
    a, keep = K.scan_args(refs)
    rc, r, c, st = inflater.bam_scan(np.frombuffer(data, np.uint8), a)
    assert rc == 0 and st.status == 0 and len(r) == st.n_recs > 0 and len(c) == st.compact_bytes > 0
    assert st.ms_guess > 0 and st.ms_link > 0 and st.ms_starts > 0 and st.ms_parse > 0 and st.ms_scan > 0 and st.ms_emit > 0 and st.ms_wall > 0


@pytest.mark.parametrize("S", SLICES)
def test_partial_record_and_truncated_tail(model, inflater, valid, S):
    _, recs, data, _, refs, _ = valid[0]
    one = K.serialise(recs[:1])[0]
    for cut in (1, 3, 4, 20, len(one) - 1):
        for last in (False, True):
            got = both(model, inflater, one[:cut], refs, last=last, slice_bytes=S)
            assert got[3]["status"] == (K.BAD_LENGTH if last else K.OK) and got[3]["n_records"] == 0
    k = 30
    whole = K.serialise(recs[:k])[0]; nxt = K.serialise(recs[k:k + 1])[0]
    exp = K.expect(recs[:k], refs)
    for extra in (2, 4, 36, len(nxt) - 1):
        got = both(model, inflater, whole + nxt[:extra], refs, slice_bytes=S)
        K.assert_equals_expectation(got, exp, whole + nxt[:extra], k, len(whole), eff(S))
        got = both(model, inflater, whole + nxt[:extra], refs, last=True, slice_bytes=S)
        assert (got[3]["status"], got[3]["status_record"], got[3]["consumed"]) == (K.BAD_LENGTH, k, len(whole))


@pytest.mark.parametrize("S", SLICES)
def test_decoys_and_an_implausible_true_record(model, inflater, valid, S):
    refs = valid[0][4]
    h = K.header(refs)
    for kind in ("qual", "B", "Z"):
        recs, data, at = K.decoy_input(kind, eff(S), refs, np.random.default_rng(31), h)
        got = both(model, inflater, data, refs, first=len(h), last=True, slice_bytes=S)
        assert got[3]["n_rehops"] >= 1
        K.assert_equals_expectation(got, K.expect(recs, refs), data, len(recs), len(data), eff(S))
        none = both(model, inflater, data, refs, first=len(h), last=True, slice_bytes=S, max_rehops=0)
        assert none[3]["status"] == K.TOO_MANY_REHOPS and len(none[1]) == 0 and none[2] == b""
        exact = both(model, inflater, data, refs, first=len(h), last=True, slice_bytes=S, max_rehops=got[3]["n_rehops"])
        assert exact[3] == got[3]
    recs, data = K.aligned_implausible(eff(S), refs, np.random.default_rng(32))
    got = both(model, inflater, data, refs, last=True, slice_bytes=S)
    assert got[3]["n_rehops"] >= 1
    K.assert_equals_expectation(got, K.expect(recs, refs), data, len(recs), len(data), eff(S))


@pytest.mark.parametrize("S", (64, 0))
def test_corruptions_report_status_and_record(model, inflater, valid, S):
    refs = valid[0][4]
    for name, (recs, status, which) in K.corruptions().items():
        got = both(model, inflater, K.serialise(recs)[0], refs, last=True, slice_bytes=S)
        assert (got[3]["status"], got[3]["status_record"]) == (status, which), name
    recs = [K.plain("r%d" % i, flag=1 | (64 if i % 2 else 128)) for i in range(8)]
    data, starts = K.serialise(recs)
    for v in (0, 31, -1, (1 << 28) + 1):
        bad = bytearray(data); bad[starts[5]:starts[5] + 4] = struct.pack("<i", v)
        got = both(model, inflater, bytes(bad), refs, slice_bytes=S)
        assert (got[3]["status"], got[3]["status_record"], got[3]["n_records"], got[3]["consumed"]) == (K.BAD_LENGTH, 5, 5, starts[5])
    two = list(recs); two[2] = K.plain("x", tags=[("NM", "C", 0)]); two[6] = K.plain("y", corrupt="l_seq")
    got = both(model, inflater, K.serialise(two)[0], refs, slice_bytes=S)
    assert (got[3]["status"], got[3]["status_record"]) == (K.NO_AS, 2)
    two[2], two[6] = two[6], two[2]
    d2, s2 = K.serialise(two)
    got = both(model, inflater, d2, refs, slice_bytes=S)
    assert (got[3]["status"], got[3]["status_record"]) == (K.CORRUPT_RECORD, 2)
    for at, want in ((7, (K.CORRUPT_RECORD, 2)), (1, (K.BAD_LENGTH, 1))):
        bad = bytearray(d2); bad[s2[at]:s2[at] + 4] = struct.pack("<i", 7)
        got = both(model, inflater, bytes(bad), refs, slice_bytes=S)
        assert (got[3]["status"], got[3]["status_record"]) == want
    # two failing records in one wavefront and in two: the lower index whatever the order the waves finish in
    many = [K.plain("m%d" % i, flag=1 | (64 if i % 2 else 128)) for i in range(400)]
    many[70] = K.plain("x", flag=0); many[300] = K.plain("y", tags=[]); many[77] = K.plain("z", corrupt="otags")
    got = both(model, inflater, K.serialise(many)[0], refs, slice_bytes=S)
    assert (got[3]["status"], got[3]["status_record"]) == (K.UNPAIRED, 70)


def test_arguments_and_capacity(pkg, model, inflater, valid):
    _, recs, data, _, refs, _ = valid[0]
    buf = np.frombuffer(data, np.uint8)
    exp = K.expect(recs, refs)
    with pytest.raises(pkg.HlalaError, match=r"\(-1\)"):
        inflater.bam_scan(buf, K.scan_args(refs)[0], first=len(data) + 1)
    for S in (1, 32, 63, 96, 3000):
        with pytest.raises(pkg.HlalaError, match=r"\(-1\)"):
            inflater.bam_scan(buf, K.scan_args(refs, slice_bytes=S)[0])
    b, keep = K.scan_args(refs); keep[0][1] = keep[0][2] + 1
    with pytest.raises(pkg.HlalaError, match=r"\(-1\)"):
        inflater.bam_scan(buf, b)
    nr, nc = len(exp["recs"]), len(exp["compact"])
    for cr, cc in ((nr - 1, nc), (nr, nc - 1), (0, 0)):
        got = both(model, inflater, data, refs, cap_recs=cr, cap_compact=cc)
        assert got[0] == K.E_CAPACITY and got[3]["n_recs"] == nr and got[3]["compact_bytes"] == nc
    got = both(model, inflater, data, refs, cap_recs=nr, cap_compact=nc)
    K.assert_equals_expectation(got, exp, data, len(recs), len(data), 16384)
    got = both(model, inflater, b"", refs)                                                   # no byte at all
    assert got[0] == 0 and got[3]["n_slices"] == 0 and got[3]["n_records"] == 0


def test_random_and_changed_bytes_report_like_the_model(model, inflater, valid):
    refs = valid[0][4]
    seen = set()
    for i, b in enumerate(K.random_buffers()):
        seen.add(both(model, inflater, b, refs, last=bool(i % 2), slice_bytes=(64, 0)[i % 3 == 0])[3]["status"])
    _, data, changed = K.byte_changes()
    for i, b in enumerate(changed):
        seen.add(both(model, inflater, b, refs, last=bool(i % 2), slice_bytes=64)[3]["status"])
    assert {K.OK, K.BAD_LENGTH, K.CORRUPT_RECORD} <= seen


@pytest.mark.parametrize("S", (256, 0))
def test_a_call_of_2500_records(model, inflater, S):
    from test_bam import make_records
    refs, recs = make_records(np.random.default_rng(41), n_names=600, lengths=(149, 150, 151, 97))
    recs = recs[:2500]
    assert len(recs) == 2500
    h = K.header(refs)
    data = K.serialise(recs, h)[0]
    for kw in (dict(), dict(long_mode=True, first_seq=123456789)):
        got = both(model, inflater, data, refs, first=len(h), last=True, slice_bytes=S, **kw)
        K.assert_equals_expectation(got, K.expect(recs, refs, kw.get("long_mode", False), first_seq=kw.get("first_seq", 0)), data, 2500, len(data), eff(S))


# ---------------------------------------------------------------------------------------------------------------- the decoder with HLALA_SEEDS_GPU_PARSE
def _rounds(path, seg_bytes):
    """(non-empty blocks, rounds) of the decoder: blocks are taken into a round while they fit seg_bytes"""
    from test_gpu_inflate import _blocks_of
    sizes = [isz for _, _, isz in _blocks_of(path)[1] if isz]
    rounds = 0; i = 0
    while i < len(sizes):
        seg = 0
        while i < len(sizes) and (seg == 0 or seg + sizes[i] <= seg_bytes):
            seg += sizes[i]; i += 1
        rounds += 1
    return len(sizes), rounds


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    from test_bam import make_records, write_bam
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    p = tmp_path_factory.mktemp("gpu_bam_scan") / "t.bam"
    write_bam(p, refs, recs, block=3000)
    return p, refs, recs


def test_bam_decoded_with_gpu_parse_is_the_same_sample(pkg, inflater, bam, monkeypatch):
    from test_gpu_inflate import INTERVALS, _same_sample
    p, refs, recs = bam
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                   # records straddle rounds and blocks
    lib = pkg.load_library()
    n_blocks, n_rounds = _rounds(p, 65536)
    assert n_blocks > 50 and n_rounds > 3
    for long_mode in (False, True):
        for flags in (0, pkg.SEEDS_PACKED):
            H = pkg.bam_open_seeds(lib, p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
            G = inflater.bam_open_seeds(p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags | pkg.SEEDS_GPU_PARSE)
            _same_sample(G, H)
            assert G.parse_counts() == (len(recs), n_rounds, 0)              # every record, every round: the fall-back hides no broken kernel
            assert G.inflate_counts() == (n_blocks, 0, 0)
            assert H.parse_counts() == (0, 0, 0)
            up, down = G.transfer_bytes()
            assert 0 < down < sum(len(K.record_body(r)) for r in recs) and up > 0            # less comes back than the records hold: the tags stay there
            assert G.n_units > 50
            G.close(); H.close()


def test_a_round_with_too_many_rehops_is_parsed_by_the_host(pkg, inflater, bam, tmp_path, monkeypatch):
    from test_gpu_inflate import INTERVALS, _same_sample
    _, refs, recs = bam
    lib = pkg.load_library()
    drecs, data, at = K.decoy_input("B", 16384, refs, np.random.default_rng(31), K.header(refs))      # the decoy on a slice start of the first round
    p = tmp_path / "decoy.bam"
    K.write_bam_file(p, refs, drecs + recs[:300], block=3000)
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    n_blocks, n_rounds = _rounds(p, 65536)
    assert n_rounds >= 2
    H = pkg.bam_open_seeds(lib, p, INTERVALS, threads=3)
    G = inflater.bam_open_seeds(p, INTERVALS, threads=3, flags=pkg.SEEDS_GPU_PARSE)
    _same_sample(G, H)
    assert G.parse_counts() == (len(drecs) + 300, n_rounds, 0)               # the default cap mends the wrong guess on the device
    G.close()
    monkeypatch.setenv("HLALA_BAM_SCAN_MAX_REHOPS", "0")
    G = inflater.bam_open_seeds(p, INTERVALS, threads=3, flags=pkg.SEEDS_GPU_PARSE)
    _same_sample(G, H)
    scanned, on_gpu, fell_back = G.parse_counts()
    assert fell_back >= 1 and on_gpu + fell_back == n_rounds and scanned < len(drecs) + 300
    assert G.inflate_counts() == (n_blocks, 0, 0)
    G.close(); H.close()


def test_file_errors_carry_the_host_decoders_text(pkg, inflater, tmp_path):
    lib = pkg.load_library()
    refs = [("chr6", 1000)]
    iv = [("chr6", 0, 999, 0)]
    base = dict(name="r", flag=1 | 64, ref=0, pos=10, cigar=[(50, "M")], seq="A" * 50, qual=[30] * 50)
    good = dict(base, name="g", tags=[("AS", "C", 40)])
    cases = {"noas": dict(base, tags=[("NM", "C", 0)]), "unp": dict(base, flag=0, tags=[("AS", "C", 40)]), "corrupt": dict(base, tags=[("AS", "C", 40)], corrupt="l_seq"),
             "tag": dict(base, tags=[("XY", "raw", b"XYi\x01")])}
    texts = {}
    for name, r in cases.items():
        p = tmp_path / (name + ".bam")
        K.write_bam_file(p, refs, [good, r, good])
        errs = []
        for opener in (lambda: pkg.bam_open_seeds(lib, p, iv, threads=2), lambda: inflater.bam_open_seeds(p, iv, threads=2, flags=pkg.SEEDS_GPU_PARSE)):
            with pytest.raises(pkg.HlalaError) as e:
                opener()
            errs.append(str(e.value))
        assert errs[0] == errs[1], name
        texts[name] = errs[0]
    assert "AS" in texts["noas"] and "IsPaired" in texts["unp"] and texts["corrupt"] == "corrupt BAM record" and texts["tag"] == "corrupt BAM tag"
    # a file cut inside its last record
    p = tmp_path / "cut.bam"
    from test_bam import bgzf_block
    raw = K.serialise([good, good], K.header(refs))[0]
    p.write_bytes(bgzf_block(raw[:-7]) + bgzf_block(b""))
    errs = []
    for opener in (lambda: pkg.bam_open_seeds(lib, p, iv, threads=2), lambda: inflater.bam_open_seeds(p, iv, threads=2, flags=pkg.SEEDS_GPU_PARSE)):
        with pytest.raises(pkg.HlalaError) as e:
            opener()
        errs.append(str(e.value))
    assert errs[0] == errs[1] == "truncated BAM record"
    with pytest.raises(pkg.HlalaError, match="GPU_PARSE"):                                   # the flag belongs to the GPU entry point
        pkg.bam_open_seeds(lib, p, iv, flags=pkg.SEEDS_GPU_PARSE)


def test_hla_la_with_gpu_parse_writes_the_same_files(pkg, tmp_path):
    """the world of test_gpu_inflate.test_hla_la_with_gpu_inflate_writes_the_same_files, --gpuParse 1 against --gpuParse 0"""
    import ctypes as C
    import os
    import subprocess
    from tools import synth
    from test_bam import batch_records, write_bam
    from test_end_to_end import write_graph_dir
    from test_graph_files import write_contigs_dir, write_graph_txt
    from test_gpu_inflate import EXE, ROOT, _stub
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "hla-la_amd", "csrc"), "../bin/HLA-LA"])
    gdir = tmp_path / "graph"; gdir.mkdir()
    w = synth.make_world(seed=12, G=4000, k=1, n_mut=6, mut_density=0.03)
    lib = C.CDLL(pkg.LIB_PATH)
    write_graph_dir(gdir, w["H"], [(1200, 1470), (1900, 2176)])
    write_graph_txt(gdir / "PRG" / "graph.txt", w["graph"], np.random.default_rng(2))
    write_contigs_dir(gdir, w["contigs"], np.random.default_rng(3))
    b = synth.make_batch(w, 300, seed=77, haps=(2, 5))
    contigs, intervals = pkg.load_contigs_dir(lib, gdir, extended_reference_genome=False)
    clen = np.diff(w["contigs"]["contig_off"])
    bam = tmp_path / "premade.bam"
    recs = batch_records(b, np.random.default_rng(1))
    write_bam(bam, [(iv[0], int(clen[i])) for i, iv in enumerate(intervals)], recs, block=30000)
    _stub(tmp_path / "bwa", "#!/bin/bash\nif [ \"$1\" = index ]; then touch $2.sa $2.ann $2.bwt; fi\nexit 0\n")
    _stub(tmp_path / "samtools", f"#!/bin/bash\ncase \"$1\" in\n view) cat > /dev/null ;;\n sort) while [ $# -gt 0 ]; do if [ \"$1\" = -o ]; then cp {bam} \"$2\"; fi; shift; done ;;\n"
                                  " index) touch \"$2.bai\" ;;\nesac\nexit 0\n")
    (tmp_path / "r1.fq").write_text("@r\nA\n+\nI\n"); (tmp_path / "r2.fq").write_text("@r\nA\n+\nI\n")
    base = [EXE, "--action", "HLA", "--maxThreads", "2", "--sampleID", "S1", "--PRG_graph_dir", str(gdir), "--FASTQU", str(tmp_path / "r1.fq"), "--FASTQ1", str(tmp_path / "r1.fq"),
            "--FASTQ2", str(tmp_path / "r2.fq"), "--bwa_bin", str(tmp_path / "bwa"), "--samtools_bin", str(tmp_path / "samtools"), "--mapAgainstCompleteGenome", "0", "--longReads", "0",
            "--loci", "A", "--rngSeed", "5"]
    outs = {}
    for g in ("0", "1"):
        outs[g] = tmp_path / ("out" + g)
        r = subprocess.run(base + ["--outputDirectory", str(outs[g]), "--gpuParse", g], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Processed 300 protoSeeds (read pairs)" in r.stdout and "End-to-end: " in r.stdout
        assert (f"BAM records: {len(recs)} scanned on the GPU in 1 rounds, 0 rounds parsed again on the host" in r.stdout) == (g == "1"), r.stdout[-2000:]
        assert ("BAM records:" in r.stdout) == (g == "1") and ("BGZF inflate:" in r.stdout) == (g == "1")          # 1 implies --gpuInflate 1
    files = sorted(os.listdir(outs["0"] / "hla"))
    assert files == sorted(os.listdir(outs["1"] / "hla")) and "R1_bestguess.txt" in files
    for fn in files:
        assert (outs["1"] / "hla" / fn).read_bytes() == (outs["0"] / "hla" / fn).read_bytes(), fn
    assert (outs["1"] / "reads_per_level.txt").read_bytes() == (outs["0"] / "reads_per_level.txt").read_bytes()
