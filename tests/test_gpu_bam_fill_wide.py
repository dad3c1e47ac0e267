"""Mates beyond 16 alignments laid out and filled on the GPU (hla-la_amd/csrc/kernel_bamfill.hip: k_fil_wide_rank, k_fil_wide_src beside the narrow kernels, which leave a
wide unit alone) behind hlala_bam_fill_create_wide, hlala_batch_create_from_fill and HLALA_SEEDS_GPU_FILL_WIDE.  The device's offsets, counts and every slice of every window
must equal the wide host model's bit for bit -- tests/test_bam_fill_wide_model.py holds that model against std::sort itself -- and a BAM decoded with all stage flags plus the
new one must be the host decoder's sample to the byte, with counts that say the device filled the wide units."""
import ctypes as C

import numpy as np
import pytest

import bam_fill_cases as F
import bam_fill_wide_cases as W
import bam_resident_cases as R
import bam_scan_cases as K

pytestmark = pytest.mark.gpu
INTERVALS = K.INTERVALS
ALL_STAGES = 2 | 8 | 16 | 32          # SEEDS_GPU_PARSE | _GROUP | _SORT | _FILL
WIDE = 64                             # SEEDS_GPU_FILL_WIDE


@pytest.fixture(scope="module")
def model():
    return W.load_model()


@pytest.fixture(scope="module")
def inflater(pkg):
    f = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    yield f
    f.close()


@pytest.fixture(scope="module")
def ctx(pkg):
    w = R.world()
    return pkg.Context(w["graph"], w["contigs"], device=0)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name", sorted(W.cases()))
def test_device_equals_the_wide_model(pkg, model, inflater, name, packed):
    units, long_mode = W.cases()[name]
    recs, data, first, count, hs = F.build(units, long_mode)
    fin, keep = pkg.bam_fill_in(recs, data, first, count, hs, long_mode, packed)
    rc, h, goff, st = inflater.bam_fill_create_wide(fin, len(first), long_mode, packed)
    assert rc == 0 and h is not None, inflater.last_error()
    try:
        rcM, moff, _, mcounts, err, mwide = W.run_model(model, recs, data, first, count, hs, long_mode, packed)
        assert rcM == 0, err
        assert {f: int(getattr(st, f)) for f in F.COUNT_FIELDS} == mcounts
        for k in moff:
            assert np.array_equal(goff[k], moff[k]), k
        ws = h.wide_stats()
        assert ws[:3] == mwide and (ws[3] > 0) == (mwide[0] > 0)
        print(name, packed, "wide units %d, wide reads %d, longest mate %d, k_fil_wide_rank + k_fil_wide_src %d us" % ws)
        for w in W.windows(units, long_mode):
            rc, garr, wst = h.window(w[0], w[1], F.CANARY)
            assert rc == 0, h.last_error()
            garr = F.check_canaries(garr, pkg.bam_fill_window_arrays(goff, w[0], w[1], long_mode, packed)[2])
            marr = W.run_model(model, recs, data, first, count, hs, long_mode, packed, window=w)[2]
            for k in marr:
                assert np.array_equal(garr[k], marr[k]), (w, k)
        if mwide[0] == 0:                                    # a sample without wide units: what hlala_bam_fill_create gives, and nothing wide ran
            rc, hn, noff, nst = inflater.bam_fill_create(fin, len(first), long_mode, packed)
            assert rc == 0 and all(np.array_equal(goff[k], noff[k]) for k in goff) and hn.wide_stats() == (0, 0, 0, 0)
            a = h.window(0, len(units), F.CANARY)[1]; b = hn.window(0, len(units), F.CANARY)[1]
            assert all(np.array_equal(a[k], b[k]) for k in a)
            hn.close()
        else:                                                # the narrow entry point keeps refusing them with its present text
            rc, hn, _, _ = inflater.bam_fill_create(fin, len(first), long_mode, packed)
            assert rc == F.E_ARG and hn is None and inflater.last_error() == "hlala_bam_fill_create: a filled unit with more than 16 alignments on one mate"
    finally:
        h.close()


def test_refusals(pkg, inflater):
    for name in W.refused():
        recs, data, first, count, hs, text = W.built_refused(name)
        fin, keep = pkg.bam_fill_in(recs, data, first, count, hs, False, False)
        rc, h, off, st = inflater.bam_fill_create_wide(fin, len(first))
        assert rc == F.E_ARG and h is None and text in inflater.last_error() and inflater.last_error().startswith("hlala_bam_fill_create_wide: "), (name, inflater.last_error())
        assert all((a == 0).all() for a in off.values()) and st.bytes_h2d == 0
    recs, data, first, count, hs = F.build(W.cases()["edge_of_the_paths"][0], False)
    fin, keep = pkg.bam_fill_in(recs, data, first, count, hs, False, False)
    for mm in (16, 4097, 0):
        rc, h, _, _ = inflater.bam_fill_create_wide(fin, len(first), max_mate=mm)
        assert rc == F.E_ARG and h is None and "max_mate outside (16, 4096]" in inflater.last_error()
    rc, h, _, _ = inflater.bam_fill_create_wide(fin, len(first), max_mate=39)            # the longest mate there has 40
    assert rc == F.E_ARG and h is None and "than max_mate" in inflater.last_error()
    rc, h, _, _ = inflater.bam_fill_create_wide(fin, len(first), max_mate=40)
    assert rc == 0 and h.wide_stats()[2] == 40
    h.close()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name", ["edge_of_the_paths", "strides_of_the_wave", "long_reads"])
def test_batch_from_a_window_with_wide_units(pkg, ctx, model, inflater, name, packed):
    """all thirteen arrays of hlala_debug_batch_inputs equal those of hlala_batch_create on the downloaded window, and nothing is staged for the wide units"""
    units, long_mode = W.cases()[name]
    units = R.below(units)
    recs, data, first, count, hs = F.build(units, long_mode)
    fin, keep = pkg.bam_fill_in(recs, data, first, count, hs, long_mode, packed)
    rc, h, off, st = inflater.bam_fill_create_wide(fin, len(first), long_mode, packed)
    assert rc == 0, inflater.last_error()
    try:
        n = len(units)
        rc, arr, _ = h.window(0, n, F.CANARY)                                            # the whole sample, downloaded
        assert rc == 0
        arr = F.check_canaries(arr, pkg.bam_fill_window_arrays(off, 0, n, long_mode, packed)[2])
        arr["cigar_off"] = np.concatenate([np.zeros(1, np.int64), arr["cigar_off_end"]])
        if packed:
            arr["read_bases_packed"] = np.concatenate([arr["read_bases_packed"], np.zeros(4, np.uint8)])
        for u0, k in W.windows(units, long_mode):
            d = R.batch_in(off, arr, u0, k, long_mode, packed)
            s, keep2 = pkg.fill_struct(pkg.BatchIn, d)
            b = C.c_void_p()
            rcH = (ctx.lib.hlala_batch_create_unpaired if long_mode else ctx.lib.hlala_batch_create)(ctx.h, C.byref(s), C.byref(b))
            assert rcH == 0, ctx.last_error()
            bH = pkg.Batch(ctx, b, d["n_chains"], d["n_pairs"]); inH = bH.inputs(); bH.close()
            rcR, bR, rst = ctx.batch_from_fill(h, u0, k, None)
            assert rcR == 0, ctx.last_error()
            inR = bR.inputs(); bR.close()
            assert (rst.n_units, rst.n_host_units, rst.n_pieces, rst.n_chains) == (k, 0, 0, d["n_chains"])
            assert sorted(inR) == sorted(inH) == sorted(R.INPUT_KEYS)
            for key in R.INPUT_KEYS:
                assert np.array_equal(inR[key], inH[key]), (u0, k, key)
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------------------------- the decoder with HLALA_SEEDS_GPU_FILL_WIDE
@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_bam_fill_wide")
    out = {k: (d / (k + ".bam"), W.write_wide_bam(d / (k + ".bam"), k)) for k in W.bam_kinds()}
    out["beyond"] = (d / "beyond.bam", W.write_beyond_bam(d / "beyond.bam"))
    return out


def same_sample(A, B):
    assert A.n_units == B.n_units and A.counts == B.counts and A.names() == B.names()
    a, b = A.to_dict(), B.to_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("kind", sorted(W.bam_kinds()) + ["beyond"])
def test_bam_decoded_with_the_wide_flag_is_the_same_sample(pkg, inflater, bams, monkeypatch, kind):
    assert ALL_STAGES | WIDE == pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP | pkg.SEEDS_GPU_SORT | pkg.SEEDS_GPU_FILL | pkg.SEEDS_GPU_FILL_WIDE
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                   # several rounds
    lib = pkg.load_library()
    path, sizes = bams[kind]
    wide = sum(16 < max(s) <= W.WIDE_MAX for s in sizes); beyond = sum(max(s) > W.WIDE_MAX for s in sizes)
    for flags in (0, pkg.SEEDS_PACKED):
        H = pkg.bam_open_seeds(lib, path, INTERVALS, threads=3, flags=flags)
        D = inflater.bam_open_seeds(path, INTERVALS, threads=3, flags=flags | ALL_STAGES | WIDE | pkg.SEEDS_VERIFY_CRC)
        assert D.parse_counts()[2] == 0 and D.group_counts()[2] == 0 and D.sort_counts()[2] == 0
        assert D.fill_counts() == (D.n_units - beyond, beyond, 0) and D.fill_wide_counts() == (wide, beyond, max(max(s) for s in sizes))       # the fall-back hides no broken kernel
        n = D.n_units
        for u0, k in ((n - 3, 3), (0, 1)):                                   # windows out of order first, then the whole sample
            a, b = D.to_dict(u0, k), H.to_dict(u0, k)
            for key in a:
                assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (u0, k, key)
        same_sample(D, H)
        D.close()
        if kind == "two_scores":                                             # without the new flag they stay host units, as before
            N = inflater.bam_open_seeds(path, INTERVALS, threads=3, flags=flags | ALL_STAGES)
            assert N.fill_counts() == (N.n_units - wide, wide, 0) and N.fill_wide_counts() == (0, 0, 0)
            same_sample(N, H)
            N.close()
        H.close()
    with pytest.raises(pkg.HlalaError, match="GPU_FILL_WIDE needs HLALA_SEEDS_GPU_FILL"):
        inflater.bam_open_seeds(path, INTERVALS, threads=3, flags=pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP | pkg.SEEDS_GPU_SORT | WIDE)


def test_hla_la_with_gpu_fill_wide(pkg, tmp_path):
    """the world of test_gpu_bam_fill.test_hla_la_with_gpu_fill_writes_the_same_files, one run with --gpuFillWide 1: it implies --gpuFill 1, prints its line, and types"""
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
    write_bam(bam, [(iv[0], int(clen[i])) for i, iv in enumerate(intervals)], batch_records(b, np.random.default_rng(1)), block=30000)
    _stub(tmp_path / "bwa", "#!/bin/bash\nif [ \"$1\" = index ]; then touch $2.sa $2.ann $2.bwt; fi\nexit 0\n")
    _stub(tmp_path / "samtools", f"#!/bin/bash\ncase \"$1\" in\n view) cat > /dev/null ;;\n sort) while [ $# -gt 0 ]; do if [ \"$1\" = -o ]; then cp {bam} \"$2\"; fi; shift; done ;;\n"
                                  " index) touch \"$2.bai\" ;;\nesac\nexit 0\n")
    (tmp_path / "r1.fq").write_text("@r\nA\n+\nI\n"); (tmp_path / "r2.fq").write_text("@r\nA\n+\nI\n")
    cmd = [EXE, "--action", "HLA", "--maxThreads", "2", "--sampleID", "S1", "--PRG_graph_dir", str(gdir), "--FASTQU", str(tmp_path / "r1.fq"), "--FASTQ1", str(tmp_path / "r1.fq"),
           "--FASTQ2", str(tmp_path / "r2.fq"), "--bwa_bin", str(tmp_path / "bwa"), "--samtools_bin", str(tmp_path / "samtools"), "--mapAgainstCompleteGenome", "0", "--longReads", "0",
           "--loci", "A", "--rngSeed", "5", "--outputDirectory", str(tmp_path / "out"), "--gpuFillWide", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Processed 300 protoSeeds (read pairs)" in r.stdout and "End-to-end: " in r.stdout
    line = [x for x in r.stdout.splitlines() if x.startswith("BAM wide fill: ")]
    assert len(line) == 1 and line[0].startswith("BAM wide fill: 0 wide units filled on the GPU, 0 units beyond 4096 alignments on a mate left to the host, longest mate "), r.stdout[-2000:]
    fill = [x for x in r.stdout.splitlines() if x.startswith("BAM fill: ")]
    assert len(fill) == 1 and fill[0].endswith(" units filled on the GPU, 0 units filled by the host") and "BAM name order:" in r.stdout
    assert "R1_bestguess.txt" in os.listdir(tmp_path / "out" / "hla")
