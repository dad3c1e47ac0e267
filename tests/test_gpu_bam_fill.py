"""The layout and the fill on the GPU (hla-la_amd/csrc/kernel_bamfill.hip: k_fil_rank, k_fil_host, k_fil_src around hipcub's scan; k_fil_chain, k_fil_cigar, k_fil_names,
k_fil_bases per window; k_fil_append in the decoder) behind hlala_bam_fill_create / _window and Inflater.bam_fill_create.  Every input of tests/test_bam_fill_model.py goes
through the device: offsets, counts and every slice of every window must equal the host model's bit for bit, and the plain-Python expectation.  The malformed inputs go
to the entry point only because the model test shows them refused before a record byte is read: nothing is uploaded for them.  Then the decoder with all five stage flags
and HLA-LA --gpuFill 1."""
import numpy as np
import pytest

import bam_fill_cases as F
import bam_scan_cases as K

pytestmark = pytest.mark.gpu
INTERVALS = K.INTERVALS
ALL_STAGES = 2 | 8 | 16 | 32          # SEEDS_GPU_PARSE | _GROUP | _SORT | _FILL


@pytest.fixture(scope="module")
def model():
    return F.load_model()


@pytest.fixture(scope="module")
def inflater(pkg):
    f = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    yield f
    f.close()


def both(pkg, model, inflater, name=None, packed=False, built=None):
    units, long_mode, recs, data, first, count, hs = built or F.built_case(name)
    off, arr = F.expect(units, long_mode, packed)
    fin, keep = pkg.bam_fill_in(recs, data, first, count, hs, long_mode, packed)
    rc, h, goff, st = inflater.bam_fill_create(fin, len(first), long_mode, packed)
    assert rc == 0, inflater.last_error()
    want = F.run_model(model, recs, data, first, count, hs, long_mode, packed)
    counts = {f: int(getattr(st, f)) for f in F.COUNT_FIELDS}
    assert counts == want[3], (counts, want[3])
    if not len(units):
        assert h is None and st.ms_wall == 0 and st.bytes_h2d == 0
        return st, []
    try:
        for k in off:
            assert np.array_equal(goff[k], want[1][k]) and np.array_equal(goff[k], off[k]), k
        times = []
        for w in F.windows(len(units)):
            rc, garr, ws = h.window(w[0], w[1], F.CANARY)
            assert rc == 0, h.last_error()
            garr = F.check_canaries(garr, pkg.bam_fill_window_arrays(goff, w[0], w[1], long_mode, packed)[2])
            marr = F.run_model(model, recs, data, first, count, hs, long_mode, packed, window=w)[2]
            exp = F.window_of(off, arr, w[0], w[1], long_mode, packed)
            for k in exp:
                assert np.array_equal(garr[k], marr[k]) and np.array_equal(garr[k], exp[k]), (w, k)
            assert (ws.n_units, ws.n_chains) == (w[1], len(exp["chain_as"]))
            times.append([ws.ms_chain, ws.ms_cigar, ws.ms_names, ws.ms_bases, ws.ms_d2h, ws.ms_wall])
        rc, _, _ = h.window(len(units), 1)
        assert rc == F.E_ARG and "units outside the sample" in h.last_error()
        rc, _, _ = h.window(-1, 1)
        assert rc == F.E_ARG
        rc, garr, ws = h.window(len(units) // 2, 0)
        assert rc == 0 and ws.n_units == 0 and ws.ms_wall == 0
    finally:
        h.close()
    return st, times


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name", sorted(F.cases()))
def test_device_equals_model_and_expectation(pkg, model, inflater, name, packed):
    st, times = both(pkg, model, inflater, name, packed)
    t = [st.ms_h2d, st.ms_rank, st.ms_scan, st.ms_src, st.ms_d2h, st.ms_wall]
    print(name, packed, " ".join(f"{x:.3f}" for x in t), "| windows:", " ; ".join(" ".join(f"{x:.3f}" for x in w) for w in times[:3]))
    if len(F.cases()[name][0]):
        assert all(x > 0 for x in t) and all(x[-1] > 0 for x in times)


def test_small_cases_after_a_large_one(pkg, model, inflater):
    """3000 units, 30 of them host units, more than one block in every kernel; then small cases on the same inflater"""
    units, long_mode = F.large_case()
    recs, data, first, count, hs = F.build(units, long_mode)
    both(pkg, model, inflater, built=(units, long_mode, recs, data, first, count, hs), packed=True)
    both(pkg, model, inflater, built=(units, long_mode, recs, data, first, count, hs), packed=False)
    for name in ("units_1", "mate_16", "host_units_all", "units_0", "n_cigar_edges"):
        both(pkg, model, inflater, name, packed=True)


def test_two_handles_live_side_by_side(pkg, model, inflater):
    """a fill state does not refer to the inflater: two of them answer in turn, one after the inflater that made it is gone"""
    other = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    A = F.built_case("units_65"); B = F.built_case("l_seq_edges")
    fa, keep_a = pkg.bam_fill_in(*A[2:7], A[1], True); fb, keep_b = pkg.bam_fill_in(*B[2:7], B[1], False)
    ha = other.bam_fill_create(fa, len(A[4]), A[1], True)
    hb = inflater.bam_fill_create(fb, len(B[4]), B[1], False)
    other.close()
    assert ha[0] == 0 and hb[0] == 0
    for (units, lm, recs, data, first, count, hs), (rc, h, goff, st), packed in ((A, ha, True), (B, hb, False), (A, ha, True)):
        off, arr = F.expect(units, lm, packed)
        rc, garr, ws = h.window(1, len(units) - 1, F.CANARY)
        exp = F.window_of(off, arr, 1, len(units) - 1, lm, packed)
        assert rc == 0
        for k in exp:
            assert np.array_equal(garr[k][:len(exp[k])], exp[k]), k
    ha[1].close(); hb[1].close()


@pytest.mark.parametrize("name", sorted(F.malformed()))
def test_argument_errors(pkg, inflater, name):
    change, text = F.malformed()[name]
    recs, data, first, count, hs, long_mode, n, n_bytes, n_units, n_host = F.apply(change)
    fin, keep = pkg.bam_fill_in(recs, data, first, count, hs, long_mode, False, n=n, n_bytes=n_bytes, n_units=n_units, n_host_units=n_host)
    rc, h, off, st = inflater.bam_fill_create(fin, len(first), long_mode, False)
    assert rc == F.E_ARG and h is None and text in inflater.last_error() and inflater.last_error().startswith("hlala_bam_fill_create: ")
    assert all((a == 0).all() for a in off.values()) and st.bytes_h2d == 0


# ---------------------------------------------------------------------------------------------------------------- the decoder with HLALA_SEEDS_GPU_FILL
@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    from test_bam import make_records, write_bam
    from test_bam_fill_decoder_model import second_bam_records
    d = tmp_path_factory.mktemp("gpu_bam_fill")
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    write_bam(d / "t.bam", refs, recs, block=3000)
    refs2, recs2, w2 = second_bam_records()
    write_bam(d / "w.bam", refs2, recs2, block=3000)
    return d / "t.bam", d / "w.bam", w2


def same_sample(A, B):
    assert A.n_units == B.n_units and A.counts == B.counts and A.names() == B.names()
    a, b = A.to_dict(), B.to_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("hash_bits", [None, "0"])
def test_bam_decoded_with_gpu_fill_is_the_same_sample(pkg, inflater, bams, monkeypatch, hash_bits):
    from test_bam_fill_decoder_model import wide_units
    assert ALL_STAGES == pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP | pkg.SEEDS_GPU_SORT | pkg.SEEDS_GPU_FILL
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                   # several rounds: the kept descriptors and bytes have grown round by round
    if hash_bits is not None:
        monkeypatch.setenv("HLALA_BAM_TEST_HASH_BITS", hash_bits)
    lib = pkg.load_library()
    t, wbam, w2 = bams
    for path in (t, wbam):
        for long_mode in (False, True):
            for flags in (0, pkg.SEEDS_PACKED):
                H = pkg.bam_open_seeds(lib, path, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
                D = inflater.bam_open_seeds(path, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags | ALL_STAGES)
                w = wide_units(H, long_mode)
                on_gpu, by_host, whole = D.fill_counts()
                assert D.parse_counts()[2] == 0 and D.group_counts()[2] == 0 and D.sort_counts()[2] == 0 and H.fill_counts() == (0, 0, 0) and D.n_units > 40
                if hash_bits is None:
                    assert (on_gpu, by_host, whole) == (D.n_units - w, w, 0) and w < D.n_units / 10          # the fall-back hides no broken kernel
                    if path == wbam and not long_mode:
                        assert w == w2
                else:
                    assert on_gpu + by_host == D.n_units and by_host >= max(1, w) and whole == 0
                n = D.n_units                                               # windows out of order first, then the whole sample
                for u0, k in ((n - 5, 5), (n // 2, 9), (0, 1)):
                    a, b = D.to_dict(u0, k), H.to_dict(u0, k)
                    for key in a:
                        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (u0, k, key)
                same_sample(D, H)
                assert sum(D.fill_ms()) > 0 if on_gpu else True
                D.close(); H.close()
    with pytest.raises(pkg.HlalaError, match="GPU_FILL needs HLALA_SEEDS_GPU_SORT"):        # the flag without the sort stage
        inflater.bam_open_seeds(t, INTERVALS, threads=3, flags=pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP | pkg.SEEDS_GPU_FILL)


def test_a_sample_freed_before_it_is_filled_and_an_eager_one(pkg, inflater, bams, monkeypatch):
    lib = pkg.load_library()
    t = bams[0]
    D = inflater.bam_open_seeds(t, INTERVALS, threads=3, flags=ALL_STAGES)
    assert D.fill_counts()[0] > 100 and D.names(3, 2)
    D.close()                                                           # the fill state goes with the batch
    monkeypatch.setenv("HLALA_BAM_EAGER", "1")
    H = pkg.bam_open_seeds(lib, t, INTERVALS, threads=3, flags=pkg.SEEDS_PACKED)
    D = inflater.bam_open_seeds(t, INTERVALS, threads=3, flags=pkg.SEEDS_PACKED | ALL_STAGES)
    assert D.fill_counts()[2] == 0 and sum(D.fill_ms()) > 0
    same_sample(D, H)
    D.close(); H.close()


def test_hla_la_with_gpu_fill_writes_the_same_files(pkg, tmp_path):
    """the world of test_gpu_bam_nameorder.test_hla_la_with_gpu_sort_writes_the_same_files, --gpuFill 1 against the default"""
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
        r = subprocess.run(base + ["--outputDirectory", str(outs[g])] + (["--gpuFill", "1"] if g == "1" else []), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Processed 300 protoSeeds (read pairs)" in r.stdout and "End-to-end: " in r.stdout
        line = [x for x in r.stdout.splitlines() if x.startswith("BAM fill: ")]
        assert len(line) == (1 if g == "1" else 0), r.stdout[-2000:]
        if g == "1":
            words = line[0].split()
            assert line[0] == f"BAM fill: {words[2]} units filled on the GPU, 0 units filled by the host" and int(words[2]) > 0, line[0]
            assert "BAM name order:" in r.stdout and "BAM grouping:" in r.stdout and "BAM records:" in r.stdout and "BGZF inflate:" in r.stdout       # 1 implies every stage below it
    files = sorted(os.listdir(outs["0"] / "hla"))
    assert files == sorted(os.listdir(outs["1"] / "hla")) and "R1_bestguess.txt" in files
    for fn in files:
        assert (outs["1"] / "hla" / fn).read_bytes() == (outs["0"] / "hla" / fn).read_bytes(), fn
    assert (outs["1"] / "reads_per_level.txt").read_bytes() == (outs["0"] / "reads_per_level.txt").read_bytes()
