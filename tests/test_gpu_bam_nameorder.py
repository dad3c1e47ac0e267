"""The read-name order on the GPU (hla-la_amd/csrc/kernel_bamnameorder.hip: k_nam_init, k_nam_key, k_nam_seg, k_nam_mark, k_nam_scatter around hipcub's radix sort and scan;
k_nam_select and k_nam_units in the decoder) behind hlala_bam_name_order and Inflater.bam_name_order.  Every input of tests/test_bam_nameorder_model.py goes through the
device: order, n_rounds and n_equal_names must equal the host model's bit for bit, and Python's own sorted().  The malformed inputs go to the entry point only because the
model test shows them refused before a name is read: nothing is uploaded for them.  Then the decoder with SEEDS_GPU_PARSE | SEEDS_GPU_GROUP | SEEDS_GPU_SORT and
HLA-LA --gpuSort 1."""
import numpy as np
import pytest

import bam_nameorder_cases as N
import bam_scan_cases as K

pytestmark = pytest.mark.gpu
INTERVALS = K.INTERVALS


@pytest.fixture(scope="module")
def model():
    return N.load_model()


@pytest.fixture(scope="module")
def built():
    return N.built_cases()


@pytest.fixture(scope="module")
def inflater(pkg):
    f = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    yield f
    f.close()


def both(model, inflater, off, ln, data, expected):
    want = N.run_model(model, off, ln, data)
    rc, order, st = inflater.bam_name_order(off, ln, data)
    counts = {f: int(getattr(st, f)) for f in N.COUNT_FIELDS}
    assert rc == want[0] == 0
    assert counts == want[2], (counts, want[2])
    assert np.array_equal(order, want[1]) and np.array_equal(order, expected[0])
    assert (counts["n_rounds"], counts["n_equal_names"]) == expected[1:]
    return st


@pytest.mark.parametrize("name", sorted(N.cases()))
def test_device_equals_model_and_expectation(model, inflater, built, name):
    off, ln, data, expected = built[name]
    st = both(model, inflater, off, ln, data, expected)
    times = [st.ms_h2d, st.ms_key, st.ms_sort, st.ms_mark, st.ms_scatter, st.ms_d2h, st.ms_wall]
    print(name, st.n_rounds, " ".join(f"{t:.3f}" for t in times))
    assert all(t > 0 for t in times) if len(off) else all(t == 0 for t in times)


def test_a_small_case_after_a_large_one_on_one_handle(pkg, model, built):
    """the buffers grow for the large case and are reused, larger than needed, by the small ones"""
    f = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    try:
        for name in ("n2", "realistic_20000", "n65", "compaction", "nul_tails", "n0", "n1"):
            both(model, f, *built[name])
    finally:
        f.close()


@pytest.mark.parametrize("name", sorted(N.malformed()))
def test_argument_errors(inflater, name):
    off, ln, data, n, n_bytes, text = N.malformed()[name]
    rc, order, st = inflater.bam_name_order(off, ln, data, n=n, n_bytes=n_bytes)
    assert rc == N.E_ARG and order.size == 0 and text in inflater.last_error() and inflater.last_error().startswith("hlala_bam_name_order: ")


# ---------------------------------------------------------------------------------------------------------------- the decoder with HLALA_SEEDS_GPU_SORT
@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    from test_bam import make_records, write_bam
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    p = tmp_path_factory.mktemp("gpu_bam_nameorder") / "t.bam"
    write_bam(p, refs, recs, block=3000)
    return p, refs, recs


def same_sample(A, B):
    assert A.n_units == B.n_units and A.counts == B.counts and A.names() == B.names()
    a, b = A.to_dict(), B.to_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("hash_bits", [None, "0"])
def test_bam_decoded_with_gpu_sort_is_the_same_sample(pkg, inflater, bam, monkeypatch, hash_bits):
    p, refs, recs = bam
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                   # several rounds: the arena the names are ordered in has grown round by round
    if hash_bits is not None:
        monkeypatch.setenv("HLALA_BAM_TEST_HASH_BITS", hash_bits)
    lib = pkg.load_library()
    fl = pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP | pkg.SEEDS_GPU_SORT
    for long_mode in (False, True):
        for flags in (0, pkg.SEEDS_PACKED):
            H = pkg.bam_open_seeds(lib, p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
            D = inflater.bam_open_seeds(p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags | fl)
            same_sample(D, H)
            assert D.parse_counts()[2] == 0 and D.group_counts()[2] == 0 and H.sort_counts() == (0, 0, 0) and D.n_units > 50
            ordered, merged, by_host = D.sort_counts()
            if hash_bits is None:
                assert (ordered, merged, by_host) == (D.n_units, 0, 0)       # every unit, none merged in: the fall-back hides no broken kernel
            else:
                assert ordered + merged == D.n_units and merged >= 1 and by_host == 0
            D.close(); H.close()
    with pytest.raises(pkg.HlalaError, match="GPU_SORT needs HLALA_SEEDS_GPU_GROUP"):        # the flag without the grouping stage
        inflater.bam_open_seeds(p, INTERVALS, threads=3, flags=pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_SORT)


def test_hla_la_with_gpu_sort_writes_the_same_files(pkg, tmp_path):
    """the world of test_gpu_bam_group.test_hla_la_with_gpu_group_writes_the_same_files, --gpuSort 1 against the default"""
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
        r = subprocess.run(base + ["--outputDirectory", str(outs[g])] + (["--gpuSort", "1"] if g == "1" else []), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Processed 300 protoSeeds (read pairs)" in r.stdout and "End-to-end: " in r.stdout
        line = [x for x in r.stdout.splitlines() if x.startswith("BAM name order: ")]
        assert len(line) == (1 if g == "1" else 0), r.stdout[-2000:]
        if g == "1":
            words = line[0].split()
            assert line[0] == f"BAM name order: {words[3]} units ordered on the GPU, 0 units merged in by the host" and int(words[3]) > 0, line[0]
            assert "BAM grouping:" in r.stdout and "BAM records:" in r.stdout and "BGZF inflate:" in r.stdout       # 1 implies --gpuGroup 1, which implies --gpuParse 1 and --gpuInflate 1
    files = sorted(os.listdir(outs["0"] / "hla"))
    assert files == sorted(os.listdir(outs["1"] / "hla")) and "R1_bestguess.txt" in files
    for fn in files:
        assert (outs["1"] / "hla" / fn).read_bytes() == (outs["0"] / "hla" / fn).read_bytes(), fn
    assert (outs["1"] / "reads_per_level.txt").read_bytes() == (outs["0"] / "reads_per_level.txt").read_bytes()
