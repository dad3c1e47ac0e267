"""Grouping BAM records by read name on the GPU (hla-la_amd/csrc/kernel_bamgroup.hip: k_grp_len, k_grp_append, k_grp_iota, k_grp_mark, k_grp_fold, k_grp_emit around
hipcub's radix sort and scan) behind hlala_bam_group and Inflater.bam_group.  Every input of tests/test_bam_group_model.py goes through the device: perm, flag and the five
counts must equal the host model's bit for bit, and the expectation written from the descriptor list.  The malformed inputs go to the entry point only because the model test
shows them refused before a descriptor is followed: nothing is uploaded for them.  Then the decoder with SEEDS_GPU_PARSE | SEEDS_GPU_GROUP and HLA-LA --gpuGroup 1."""
import numpy as np
import pytest

import bam_group_cases as G
import bam_scan_cases as K

pytestmark = pytest.mark.gpu
INTERVALS = K.INTERVALS


@pytest.fixture(scope="module")
def model():
    return G.load_model()


@pytest.fixture(scope="module")
def built():
    return G.built_cases()


@pytest.fixture(scope="module")
def inflater(pkg):
    f = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    yield f
    f.close()


def both(pkg, model, inflater, recs, data, long_mode, rounds=None):
    want = G.run_model(model, recs, data, long_mode)
    rc, perm, flag, st = inflater.bam_group(recs, data, long_mode, rounds=rounds)
    counts = {f: int(getattr(st, f)) for f in G.COUNT_FIELDS}
    assert rc == want[0] == 0
    assert np.array_equal(perm, want[1]) and np.array_equal(flag, want[2]) and counts == want[3], (counts, want[3])
    return perm, flag, counts, st


@pytest.mark.parametrize("name", sorted(G.cases()))
def test_device_equals_model_and_expectation(pkg, model, inflater, built, name):
    recs, data = built[name]
    for long_mode in (False, True):
        perm, flag, counts, st = both(pkg, model, inflater, recs, data, long_mode)
        e = G.expect(recs, data, long_mode)
        assert np.array_equal(perm, e[0]) and np.array_equal(flag, e[1]) and counts == e[2]
        times = [st.ms_h2d, st.ms_append, st.ms_sort, st.ms_mark, st.ms_fold, st.ms_emit, st.ms_d2h, st.ms_wall]
        print(name, long_mode, " ".join(f"{t:.3f}" for t in times))
        assert all(t > 0 for t in times) if len(recs) else all(t == 0 for t in times[:-1])


def test_appended_in_rounds_of_uneven_size(pkg, model, inflater, built):
    recs, data = built["rounds"]
    assert sum(G.ROUNDS) == len(recs)
    one = both(pkg, model, inflater, recs, data, False)
    many = both(pkg, model, inflater, recs, data, False, rounds=G.ROUNDS)
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])
    both(pkg, model, inflater, recs, data, True, rounds=(0, 1, 63, 0, 65, 2000, 0))
    big, bdata = built["collided_5004"]                                        # the long run across rounds, then a smaller sample on the same handle
    both(pkg, model, inflater, big, bdata, False, rounds=(4, 5000, len(big) - 5004))
    both(pkg, model, inflater, *built["n65"], False, rounds=(64, 1))


@pytest.mark.parametrize("name", sorted(G.malformed()))
def test_argument_errors(pkg, inflater, name):
    recs, data, n, n_bytes, text = G.malformed()[name]
    rc, perm, flag, st = inflater.bam_group(recs, data, n=n, n_bytes=n_bytes)
    assert rc == G.E_ARG and text in inflater.last_error()
    if n is None:
        rc, perm, flag, st = inflater.bam_group(recs, data, rounds=(len(recs),), n_bytes=n_bytes)
        assert rc == G.E_ARG and text in inflater.last_error()


def test_round_sizes_must_add_up(pkg, inflater, built):
    recs, data = built["n65"]
    for rounds in ((64,), (64, 2), (66, -1), (1 << 40,)):
        rc, _, _, _ = inflater.bam_group(recs, data, rounds=rounds)
        assert rc == G.E_ARG and "round sizes" in inflater.last_error()


# ---------------------------------------------------------------------------------------------------------------- the decoder with HLALA_SEEDS_GPU_GROUP
@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    from test_bam import make_records, write_bam
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    p = tmp_path_factory.mktemp("gpu_bam_group") / "t.bam"
    write_bam(p, refs, recs, block=3000)
    return p, refs, recs


def same_sample(A, B):
    assert A.n_units == B.n_units and A.counts == B.counts and A.names() == B.names()
    a, b = A.to_dict(), B.to_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("hash_bits", [None, "0"])
def test_bam_decoded_with_gpu_group_is_the_same_sample(pkg, inflater, bam, monkeypatch, hash_bits):
    p, refs, recs = bam
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                   # several rounds: k_grp_append several times, the arrays grow
    if hash_bits is not None:
        monkeypatch.setenv("HLALA_BAM_TEST_HASH_BITS", hash_bits)
    lib = pkg.load_library()
    for long_mode in (False, True):
        n_desc = len(K.expect(recs, refs, long_mode)["recs"])
        assert n_desc > 400
        for flags in (0, pkg.SEEDS_PACKED):
            H = pkg.bam_open_seeds(lib, p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
            D = inflater.bam_open_seeds(p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags | pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP)
            same_sample(D, H)
            assert D.parse_counts()[1] > 3 and D.parse_counts()[2] == 0 and H.group_counts() == (0, 0, 0)
            grouped, regrouped, by_host = D.group_counts()
            if hash_bits is None:
                assert (grouped, regrouped, by_host) == (n_desc, 0, 0)       # every descriptor, no run handed back: the fall-back hides no broken kernel
            else:
                assert grouped == n_desc and regrouped >= 1 and by_host == 0
            assert D.n_units > 50
            D.close(); H.close()


def test_a_round_parsed_by_the_host_hands_the_grouping_back(pkg, inflater, bam, tmp_path, monkeypatch):
    _, refs, recs = bam
    lib = pkg.load_library()
    drecs, data, at = K.decoy_input("B", 16384, refs, np.random.default_rng(31), K.header(refs))
    p = tmp_path / "decoy.bam"
    K.write_bam_file(p, refs, drecs + recs[:300], block=3000)
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    fl = pkg.SEEDS_GPU_PARSE | pkg.SEEDS_GPU_GROUP
    H = pkg.bam_open_seeds(lib, p, INTERVALS, threads=3)
    D = inflater.bam_open_seeds(p, INTERVALS, threads=3, flags=fl)
    same_sample(D, H)
    assert D.group_counts()[0] > 0 and D.group_counts()[1:] == (0, 0)
    D.close()
    monkeypatch.setenv("HLALA_BAM_SCAN_MAX_REHOPS", "0")
    D = inflater.bam_open_seeds(p, INTERVALS, threads=3, flags=fl)
    same_sample(D, H)
    assert D.parse_counts()[2] >= 1 and D.group_counts() == (0, 0, 1)
    D.close(); H.close()
    with pytest.raises(pkg.HlalaError, match="GPU_GROUP needs HLALA_SEEDS_GPU_PARSE"):       # the flag without the record pass
        inflater.bam_open_seeds(p, INTERVALS, threads=3, flags=pkg.SEEDS_GPU_GROUP)


def test_hla_la_with_gpu_group_writes_the_same_files(pkg, tmp_path):
    """the world of test_gpu_bam_scan.test_hla_la_with_gpu_parse_writes_the_same_files, --gpuGroup 1 against the default"""
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
        r = subprocess.run(base + ["--outputDirectory", str(outs[g])] + (["--gpuGroup", "1"] if g == "1" else []), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Processed 300 protoSeeds (read pairs)" in r.stdout and "End-to-end: " in r.stdout
        line = [x for x in r.stdout.splitlines() if x.startswith("BAM grouping: ")]
        assert len(line) == (1 if g == "1" else 0), r.stdout[-2000:]
        if g == "1":
            words = line[0].split()
            assert line[0] == f"BAM grouping: {words[2]} records grouped on the GPU, 0 hash runs regrouped on the host" and int(words[2]) > 0, line[0]
            assert "BAM records:" in r.stdout and "BGZF inflate:" in r.stdout                               # 1 implies --gpuParse 1, which implies --gpuInflate 1
    files = sorted(os.listdir(outs["0"] / "hla"))
    assert files == sorted(os.listdir(outs["1"] / "hla")) and "R1_bestguess.txt" in files
    for fn in files:
        assert (outs["1"] / "hla" / fn).read_bytes() == (outs["0"] / "hla" / fn).read_bytes(), fn
    assert (outs["1"] / "reads_per_level.txt").read_bytes() == (outs["0"] / "reads_per_level.txt").read_bytes()
