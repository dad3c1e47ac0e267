"""hlala_seed_batch_create_resident on the device: a sample decoded with every GPU stage hands its windows to the aligner without the window coming down
(hlala_seed_batch_window) and going up again (hlala_batch_create).  One small BAM of the synthetic context tests/test_gpu_bam_resident.py uses is decoded twice with all
fill flags; one decode is walked by window + hlala_batch_create, the other by create_resident, in windows of 1, 127, 128, 129 and 50 units.  The thirteen arrays of
hlala_debug_batch_inputs must be equal bit for bit, and so must hlala_pairs_out after hlala_align_batch on both.  With host units (collided hash runs; a mate of 17
alignments without the WIDE flag) and without, packed and ASCII; in long-read mode the inputs are compared (the context is a short-read one: nothing is aligned there).
Refusals come back with the host path's code and text, the resident walk downloads no window, the counters match the walk, two samples of one process do not disturb
each other, and HLA-LA --gpuResident 1 writes the files it writes without it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bam_resident_cases as R

pytestmark = pytest.mark.gpu
ALL_STAGES = 2 | 8 | 16 | 32          # SEEDS_GPU_PARSE | _GROUP | _SORT | _FILL
WIDE = 64                             # SEEDS_GPU_FILL_WIDE
SIZES = (1, 127, 128, 129, 50)
N_PAIRS = 450
PAIR_KEYS_EXACT = ("pair_status", "best_chain", "n_combinations", "n_cols", "col_level", "col_edge", "col_gchar", "col_schar", "col_mapq", "pair_ll", "pair_mapq")


@pytest.fixture(scope="module")
def inflater(pkg):
    f = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    yield f
    f.close()


@pytest.fixture(scope="module")
def ctx(pkg):
    w = R.world()
    return pkg.Context(w["graph"], w["contigs"], device=0)


@pytest.fixture(scope="module")
def world_bams(tmp_path_factory):
    """(plain BAM, BAM with a mate of 17 alignments, BAM whose last two units are refused, intervals): read pairs of the synthetic world, so that every window aligns"""
    import sys
    sys.path.insert(0, R.ROOT)
    from tools import synth
    from test_bam import batch_records, write_bam
    w = R.world()
    b = synth.make_batch(w, N_PAIRS, seed=31)
    nct = R.n_contigs()
    lens = [int(x) for x in np.diff(w["contigs"]["contig_off"])]
    refs = [("hap%d" % i, lens[i]) for i in range(nct)]
    intervals = [("hap%d" % i, 0, lens[i] - 1, i) for i in range(nct)]
    recs = batch_records(b, np.random.default_rng(7))
    d = tmp_path_factory.mktemp("gpu_bam_resident_decoder")
    write_bam(d / "plain.bam", refs, recs, block=20000)
    # a mate of 17 alignments: sixteen secondary copies of one alignment of pair 200, with lower scores
    src = next(r for r in recs if r["name"] == "pair%07d" % 200 and r["flag"] & 64 and not r["flag"] & 256)
    wide = recs + [dict(src, flag=src["flag"] | 256, tags=[("AS", "i", max(1, int(src["tags"][0][2]) - 1 - k % 3))]) for k in range(16)]
    write_bam(d / "mate17.bam", refs, wide, block=20000)
    # the last two units in name order: a chain on a contig the context does not have (chain_contig == n_contigs), a paired read of 1025 bases
    one = next(r for r in recs if not r["flag"] & 256)
    bad = []
    for mate in (64, 128):
        bad.append(dict(one, name="zzy_contig", flag=1 | mate, ref=nct, pos=10, tags=[("AS", "i", 50)]))
        seq = "ACGT" * 256 + "A"
        bad.append(dict(one, name="zzz_long", flag=1 | mate, ref=0, pos=10, cigar=[(1025, "M")], seq=seq, qual=[30] * 1025, tags=[("AS", "i", 50)]))
    L = sum(l for l, o in one["cigar"] if o in "MDN=X")
    assert lens[0] > 1100 and L + 10 < 3000
    write_bam(d / "refused.bam", refs + [("extra", 3000)], recs + bad, block=20000)
    return d / "plain.bam", d / "mate17.bam", d / "refused.bam", intervals, intervals + [("extra", 0, 2999, nct)]


def cuts(n, sizes=SIZES):
    out, a, i = [], 0, 0
    while a < n:
        k = min(sizes[i % len(sizes)], n - a); out.append((a, k)); a += k; i += 1
    return out


def host_batch(pkg, ctx, D, u0, n):
    """hlala_seed_batch_window + hlala_batch_create / _unpaired: (return code, Batch or None, text)"""
    d = D.window(u0, n)
    b = C.c_void_p()
    rc = (ctx.lib.hlala_batch_create_unpaired if D.long_read_mode else ctx.lib.hlala_batch_create)(ctx.h, C.byref(d), C.byref(b))
    return rc, (pkg.Batch(ctx, b, d.n_chains, n) if rc == 0 else None), (ctx.last_error() if rc else "")


def same_batches(bH, bR, align):
    a, b = bH.inputs(), bR.inputs()
    assert sorted(a) == sorted(b) and len([k for k in a if isinstance(a[k], np.ndarray)]) >= 13
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    if align:
        bH.align(); bR.align()
        p, q = bH.pairs(), bR.pairs()
        for k in p:
            assert np.array_equal(np.asarray(p[k]), np.asarray(q[k])), k
        assert all(k in p for k in PAIR_KEYS_EXACT)


def walk(pkg, ctx, DH, DR, windows, align):
    """the windows on both decodes; returns (windows built resident, units in them, host units in them)"""
    host_units = 0
    for u0, n in windows:
        rcH, bH, textH = host_batch(pkg, ctx, DH, u0, n)
        rcR, bR, st = DR.create_resident(ctx, u0, n)
        assert rcH == 0 and rcR == 0, (u0, n, textH, ctx.last_error())
        assert (st.n_units, st.n_chains) == (n, bH.n_chains) and (st.n_pieces > 0) == (st.n_host_units > 0)
        host_units += st.n_host_units
        same_batches(bH, bR, align)
        bH.close(); bR.close()
    return len(windows), sum(n for _, n in windows), host_units


CASES = {"collided": ("plain", True, "8"), "mate_of_17": ("mate17", False, None), "none": ("plain", True, None)}      # BAM, the WIDE flag, HLALA_BAM_TEST_HASH_BITS


def open_two(pkg, inflater, world_bams, monkeypatch, case, packed, long_mode=False):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                   # several rounds
    which, wide, bits = CASES[case]
    if bits is not None:
        monkeypatch.setenv("HLALA_BAM_TEST_HASH_BITS", bits)
    path = {"plain": world_bams[0], "mate17": world_bams[1]}[which]
    flags = ALL_STAGES | (WIDE if wide else 0) | (pkg.SEEDS_PACKED if packed else 0)
    DH = inflater.bam_open_seeds(path, world_bams[3], long_read_mode=long_mode, threads=3, flags=flags)
    DR = inflater.bam_open_seeds(path, world_bams[3], long_read_mode=long_mode, threads=3, flags=flags)
    assert DH.fill_counts() == DR.fill_counts() and DR.fill_counts()[2] == 0 and DR.n_units == N_PAIRS
    return DH, DR


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_resident_walk_equals_the_host_walk(pkg, ctx, inflater, world_bams, monkeypatch, case, packed):
    DH, DR = open_two(pkg, inflater, world_bams, monkeypatch, case, packed)
    by_host = DR.fill_counts()[1]
    assert {"collided": by_host > 0, "mate_of_17": by_host == 1, "none": by_host == 0}[case]
    up0, down0 = DR.transfer_bytes(); upH0, downH0 = DH.transfer_bytes()
    ws = cuts(DR.n_units)
    assert [k for _, k in ws[:5]] == list(SIZES)
    nw, nu, nh = walk(pkg, ctx, DH, DR, ws, align=True)
    assert nu == DR.n_units and nh == by_host
    built, units, pieces, fell_back = DR.resident_counts()
    assert (built, units, fell_back) == (nw, nu, 0) and (pieces > 0) == (by_host > 0) and DH.resident_counts() == (0, 0, 0, 0)
    # no window came down on the resident walk: a few words per window (the violation slots, the count of prepared chains); the host walk brought every array down
    down = DR.transfer_bytes()[1] - down0; downH = DH.transfer_bytes()[1] - downH0
    assert down <= 64 * nw and downH > 2 * 100 * DR.n_units and (DR.transfer_bytes()[0] - up0 > 0)
    assert DR.names() == DH.names()                                          # copied by the host, from its working memory
    rc, b, st = DR.create_resident(ctx, 0, 1)                                # every unit has been handed out: the state is released
    assert rc == -5 and b is None and ctx.last_error().startswith("not available:") and DR.resident_counts()[3] == 1
    with pytest.raises(pkg.HlalaError, match="only handed out as resident windows"):
        DR.window(0, 1)
    DH.close(); DR.close()


def test_long_read_mode_inputs(pkg, ctx, inflater, world_bams, monkeypatch):
    for case, packed in (("collided", True), ("none", False)):
        DH, DR = open_two(pkg, inflater, world_bams, monkeypatch, case, packed, long_mode=True)
        nw, nu, nh = walk(pkg, ctx, DH, DR, cuts(DR.n_units), align=False)
        assert nu == DR.n_units and nh == DR.fill_counts()[1] and DR.resident_counts()[:2] == (nw, nu) and DR.names() == DH.names()
        DH.close(); DR.close()
        monkeypatch.delenv("HLALA_BAM_TEST_HASH_BITS", raising=False)


def test_windows_twice_interleaved_and_out_of_order(pkg, ctx, inflater, world_bams, monkeypatch):
    DH, DR = open_two(pkg, inflater, world_bams, monkeypatch, "collided", True)
    n = DR.n_units
    walk(pkg, ctx, DH, DR, [(n, 0), (0, 0), (n - 1, 1), (0, 1), (n - 1, 1), (300, 129), (300, 129)], align=False)
    a, b = DR.to_dict(290, 20), DH.to_dict(290, 20)                          # the host path over units that went out resident, before the release
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    walk(pkg, ctx, DH, DR, [(1 + u0, k) for u0, k in reversed(cuts(n - 2, (128,)))], align=False)      # descending, over [1, n - 1): with the two single units that is every unit
    rc, b, st = DR.create_resident(ctx, 0, 1)
    assert rc == -5 and ctx.last_error().startswith("not available:")       # released with the last unit
    a, b = DR.to_dict(290, 20), DH.to_dict(290, 20)                          # the chunks the host wrote stay readable
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    DH.close(); DR.close()


def test_a_peeked_sample_still_goes_resident(pkg, ctx, inflater, world_bams, monkeypatch):
    """what the host program does with a sample of fewer than 4000 units: the insert-size window covers it whole, as a peek; every batch behind it is built on the device"""
    DH, DR = open_two(pkg, inflater, world_bams, monkeypatch, "collided", True)
    n = DR.n_units
    assert DR.window(0, n, peek=True).n_chains == DH.window(0, n).n_chains
    nw, nu, nh = walk(pkg, ctx, DH, DR, cuts(n, (128,)), align=True)
    assert DR.resident_counts() == (nw, n, DR.resident_counts()[2], 0) and nh == DR.fill_counts()[1]
    rc, b, st = DR.create_resident(ctx, 0, 1)
    assert rc == -5 and ctx.last_error().startswith("not available:")       # released with the last batch
    a, b = DR.to_dict(), DH.to_dict()                                        # the peek wrote the host arrays
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    DH.close(); DR.close()


def test_refusals_are_the_host_path_s(pkg, ctx, inflater, world_bams, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    for packed in (False, True):
        flags = ALL_STAGES | WIDE | (pkg.SEEDS_PACKED if packed else 0)
        DH = inflater.bam_open_seeds(world_bams[2], world_bams[4], threads=3, flags=flags)
        DR = inflater.bam_open_seeds(world_bams[2], world_bams[4], threads=3, flags=flags)
        n = DR.n_units
        assert n == N_PAIRS + 2 and DR.names(n - 2, 2) == ["zzy_contig", "zzz_long"] and DR.fill_counts() == (n, 0, 0)
        seen = set()
        for u0, k in ((n - 2, 1), (n - 1, 1), (n - 40, 40)):
            rcH, bH, textH = host_batch(pkg, ctx, DH, u0, k)
            rcR, bR, st = DR.create_resident(ctx, u0, k)
            assert rcH != 0 and bH is None and (rcR, ctx.last_error()) == (rcH, textH) and bR is None, (u0, k, rcH, textH, rcR, ctx.last_error())
            seen.add(textH)
        assert R.TEXT["contig"] in seen and len(seen) == 2
        assert DR.resident_counts() == (0, 0, 0, 0)                          # nothing was handed out
        walk(pkg, ctx, DH, DR, [(n - 42, 40), (0, 129)], align=True)         # the windows in front of them pass, on the same state
        DH.close(); DR.close()                                               # (units remain: the fill state goes with the sample)


def test_two_samples_in_one_process(pkg, ctx, inflater, world_bams, monkeypatch):
    """ordinary use of the host program: a second sample decoded after the first is freed, and beside it"""
    DH, DR = open_two(pkg, inflater, world_bams, monkeypatch, "none", True)
    walk(pkg, ctx, DH, DR, cuts(DR.n_units, (200,)), align=False)
    DR.close()                                                               # the first is freed before the second opens
    DR2 = inflater.bam_open_seeds(world_bams[1], world_bams[3], threads=3, flags=ALL_STAGES | pkg.SEEDS_PACKED)
    DH2 = inflater.bam_open_seeds(world_bams[1], world_bams[3], threads=3, flags=ALL_STAGES | pkg.SEEDS_PACKED)
    walk(pkg, ctx, DH2, DR2, cuts(DR2.n_units, (200,)), align=False)
    assert DR2.resident_counts()[:2] == (3, DR2.n_units) and DR2.fill_counts()[1] == 1
    DR2.close(); DH2.close()
    # both alive: their windows take turns
    A = inflater.bam_open_seeds(world_bams[0], world_bams[3], threads=3, flags=ALL_STAGES | WIDE)
    B = inflater.bam_open_seeds(world_bams[1], world_bams[3], threads=3, flags=ALL_STAGES | pkg.SEEDS_PACKED)
    HB = pkg.bam_open_seeds(pkg.load_library(), world_bams[1], world_bams[3], threads=3, flags=pkg.SEEDS_PACKED)       # (B's sample as the host decoder gives it)
    for w in cuts(A.n_units, (150,)):
        walk(pkg, ctx, DH, A, [w], align=False)
        walk(pkg, ctx, HB, B, [w], align=False)
    assert A.resident_counts()[:2] == (3, A.n_units) and B.resident_counts()[:2] == (3, B.n_units)
    assert A.names() == DH.names() and B.names() == HB.names()
    A.close(); B.close(); DH.close(); HB.close()


def test_a_sample_without_a_fill_state_falls_back(pkg, ctx, inflater, world_bams):
    D = inflater.bam_open_seeds(world_bams[0], world_bams[3], threads=3, flags=pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP | pkg.SEEDS_GPU_SORT)
    H = pkg.bam_open_seeds(pkg.load_library(), world_bams[0], world_bams[3], threads=3)
    for S in (D, H):
        rc, b, st = S.create_resident(ctx, 0, 50)
        assert rc == -5 and b is None and ctx.last_error().startswith("not available:") and S.resident_counts() == (0, 0, 0, 1)
        rc, b, _ = host_batch(pkg, ctx, S, 0, 50)                            # the caller's existing route
        assert rc == 0
        b.close()
    D.close(); H.close()


def test_hla_la_with_gpu_resident_writes_the_same_files(pkg, tmp_path):
    """the world of test_gpu_bam_fill.test_hla_la_with_gpu_fill_writes_the_same_files, --gpuResident 1 against the default."""
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
            "--loci", "A", "--rngSeed", "5", "--batchPairs", "128"]
    outs = {}
    for g in ("0", "1"):
        outs[g] = tmp_path / ("out" + g)
        r = subprocess.run(base + ["--outputDirectory", str(outs[g])] + (["--gpuResident", "1"] if g == "1" else []), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Processed 300 protoSeeds (read pairs)" in r.stdout and "End-to-end: " in r.stdout
        line = [x for x in r.stdout.splitlines() if x.startswith("BAM windows: ")]
        assert len(line) == (1 if g == "1" else 0), r.stdout[-2000:]
        if g == "1":
            windows = line[0]
            assert "BAM fill: " in r.stdout and "BAM name order:" in r.stdout and "BGZF inflate:" in r.stdout       # 1 implies --gpuFill 1 and every stage below it
    files = sorted(os.listdir(outs["0"] / "hla"))
    assert files == sorted(os.listdir(outs["1"] / "hla")) and "R1_bestguess.txt" in files
    for fn in files:
        assert (outs["1"] / "hla" / fn).read_bytes() == (outs["0"] / "hla" / fn).read_bytes(), fn
    assert (outs["1"] / "reads_per_level.txt").read_bytes() == (outs["0"] / "reads_per_level.txt").read_bytes()
    assert windows == "BAM windows: 3 built on the GPU, 0 through the host", windows
