"""BGZF inflate on the GPU (hla-la_amd/csrc/kernel_inflate.hip: k_bgzf_inflate, one wavefront per block) behind hlala_bgzf_inflate, hlala_bam_extract_seeds_gpu and
`HLA-LA --gpuInflate 1`.  Expected bytes are zlib's; expected statuses are those of the host model, which runs the same decoder core (tests/test_inflate_model.py shows
the core bounded on every malformed stream used here: on the device they check the error reporting, not fault behaviour)."""
import ctypes as C
import os
import stat
import subprocess

import numpy as np
import pytest

import inflate_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hla-la_amd", "bin", "HLA-LA")
CANARY = 0x5A
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vectors():
    """[(name, stream, isize, zlib's bytes or None, status of the host model)], valid and malformed interleaved"""
    so = os.path.join(ROOT, "hla-la_amd", "libhlala_host.so")
    host = C.CDLL(so)
    host.hlala_host_inflate_model.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32]
    valid = [(n, s, z, d) for n, s, z, d in V.valid_vectors()]
    bad = [(n, s, z, None) for n, s, z, _, _ in V.malformed_vectors() + V.truncation_vectors()]
    flip, fdata = V.flip_stream()
    for bit in range(8 * len(flip)):                             # every single-bit flip: accepted ones with zlib's bytes, rejected ones with None
        s = bytearray(flip); s[bit >> 3] ^= 1 << (bit & 7)
        z, err = V.zlib_inflate(s)
        bad.append(("flip_%d" % bit, bytes(s), len(fdata), z if err is None and len(z) == len(fdata) else None))
    out = []
    for i in range(max(len(valid), len(bad))):
        out += valid[i:i + 1] + bad[i:i + 1]
    res = []
    for n, s, z, d in out:
        buf = np.zeros(z + 1, np.uint8)
        st = host.hlala_host_inflate_model(bytes(s), len(s), buf.ctypes.data, z)
        if d is not None and not n.startswith("flip_"):
            assert st == 0, n
        if st == 0:
            assert d is not None and buf[:z].tobytes() == d, n                 # (the model never accepts what zlib does not give)
        res.append((n, s, z, d if st == 0 else None, st))
    return res


def layout(vec, rng):
    """the streams in shuffled memory order with gaps, the output ranges in another shuffled order with gaps; canaries everywhere else"""
    n = len(vec)
    corder = rng.permutation(n); uorder = rng.permutation(n)
    coff = np.zeros(n, np.int64); uoff = np.zeros(n, np.int64)
    at = 7
    for i in corder:
        coff[i] = at; at += len(vec[i][1]) + int(rng.integers(0, 9))
    comp = np.full(at + 5, CANARY, np.uint8)
    for i in range(n):
        comp[coff[i]:coff[i] + len(vec[i][1])] = np.frombuffer(vec[i][1], np.uint8)
    at = 13
    for i in uorder:
        uoff[i] = at; at += vec[i][2] + int(rng.integers(1, 40))
    out = np.full(at + 11, CANARY, np.uint8)
    blocks = [(int(coff[i]), len(vec[i][1]), vec[i][2], int(uoff[i])) for i in range(n)]
    return comp, out, blocks


@pytest.fixture(scope="module")
def inflater(pkg):
    f = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    yield f
    f.close()


@pytest.mark.parametrize("n_blocks", [1, 65, None])
def test_vectors_through_one_call(pkg, inflater, vectors, n_blocks):
    vec = vectors if n_blocks is None else vectors[:n_blocks]
    comp, out, blocks = layout(vec, np.random.default_rng(len(vec)))
    if n_blocks is None:
        assert sum(len(v[1]) for v in vec) > 3 * pkg.INFLATE_MIN_CHUNK                # the call spans several chunks
    status, st = inflater.inflate(comp, blocks, out)
    covered = np.zeros(out.size, bool)
    n_bad = 0
    for (name, s, isize, data, want), (co, cl, isz, uo), got in zip(vec, blocks, status):
        assert got == want, (name, pkg.INFLATE_STATUS[got], pkg.INFLATE_STATUS[want])
        covered[uo:uo + isz] = True
        if want == 0:
            assert out[uo:uo + isz].tobytes() == data, name
        else:
            n_bad += 1
    assert (out[~covered] == CANARY).all(), "bytes outside the blocks' ranges were written"
    assert st.n_blocks == len(vec) and st.n_rejected == n_bad and st.n_ok == len(vec) - n_bad
    if n_blocks is None:
        assert n_bad > 100 and st.n_ok >= 70 and st.ms_kernel > 0


def test_descriptors_are_validated_before_anything_runs(pkg, inflater):
    stream = V.deflate(b"hello hello hello hello")
    comp = np.frombuffer(stream, np.uint8).copy(); n = len(stream)
    out = np.full(200, CANARY, np.uint8)
    for blocks in ([(0, n, 23, 0), (0, n, 23, 22)],                   # overlapping outputs
                   [(0, n, 23, 30), (0, n, 23, 0), (0, n, 23, 52)],   # ... not adjacent in the list
                   [(1, n, 23, 0)],                                   # compressed range ends outside comp
                   [(n + 1, 0, 23, 0)],
                   [(0, n, 23, 178)],                                 # output range ends outside out
                   [(0, n, 23, 1 << 40)],
                   [((1 << 64) - 1, 2, 23, 0)],
                   [(0, n, 65537, 0)]):                               # more than 64 KiB of payload
        with pytest.raises(pkg.HlalaError, match=r"\(-1\)"):
            inflater.inflate(comp, blocks, out)
        assert (out == CANARY).all()
    status, st = inflater.inflate(comp, [(0, n, 23, 0), (0, n, 23, 23), (0, n, 0, 23)], out)      # adjacent ranges and an empty one are fine
    assert status.tolist() == [0, 0, V.OUTPUT_SIZE] and out[:46].tobytes() == b"hello hello hello hello" * 2 and (out[46:] == CANARY).all()
    status, st = inflater.inflate(comp, [], out)
    assert len(status) == 0 and st.n_blocks == 0
    with pytest.raises(pkg.HlalaError):
        pkg.Inflater(pkg.load_library(), chunk_bytes=pkg.INFLATE_MIN_CHUNK - 1)


INTERVALS = [("chr6", 10000, 20000, 0), ("HLA-A*01", 0, 3999, 1), ("chr6", 19000, 30000, 2)]


def _same_sample(A, B):
    assert A.n_units == B.n_units and A.counts == B.counts and A.names() == B.names()
    a, b = A.to_dict(), B.to_dict()
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def _blocks_of(path):
    """(offset of the payload, its length, isize) of every BGZF block of the file"""
    raw = open(path, "rb").read(); o = 0; out = []
    while o < len(raw):
        bsize = int.from_bytes(raw[o + 16:o + 18], "little") + 1
        out.append((o + 18, bsize - 26, int.from_bytes(raw[o + bsize - 4:o + bsize], "little")))
        o += bsize
    return raw, out


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    from test_bam import make_records, write_bam
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    p = tmp_path_factory.mktemp("gpu_inflate") / "t.bam"
    write_bam(p, refs, recs, block=3000)
    return p, refs, recs


def test_bam_decoded_with_gpu_inflate_is_the_same_sample(pkg, inflater, bam, monkeypatch):
    from test_bam import check, expected_batch
    p, refs, recs = bam
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                   # records straddle rounds
    lib = pkg.load_library()
    n_nonempty = sum(1 for _, _, isz in _blocks_of(p)[1] if isz)
    assert n_nonempty > 50
    for long_mode in (False, True):
        for flags in (0, pkg.SEEDS_PACKED):
            H = pkg.bam_open_seeds(lib, p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
            G = inflater.bam_open_seeds(p, INTERVALS, long_read_mode=long_mode, threads=3, flags=flags)
            _same_sample(G, H)
            assert G.inflate_counts() == (n_nonempty, 0, 0)                  # nothing rejected: the host engine never stood in for the kernel
            assert H.inflate_counts() == (0, 0, n_nonempty)
            t = G.timing(); assert t["inflate"] > 0 and t["threads"] == 3
            assert G.n_units > 50
            G.close(); H.close()
    # ... and it is the sample the record list says (the check of tests/test_bam.py)
    b, names, cnt, counts = inflater.bam_extract_seeds_gpu(p, INTERVALS, threads=1)
    units, examined, n_seeds, n_inc = expected_batch(recs, refs, INTERVALS, False)
    check(b, names, cnt, units, examined, n_seeds, n_inc, False)


def test_a_corrupt_block_fails_like_the_host_path(pkg, inflater, bam, tmp_path):
    p, refs, recs = bam
    raw, blocks = _blocks_of(p)
    lib = pkg.load_library()
    # a payload byte of block 5 whose change zlib rejects (most single-byte changes of a dynamic block's header are)
    off, clen, isize = blocks[5]
    choice = None
    for k in range(0, 40):
        s = bytearray(raw[off:off + clen]); s[k] ^= 0xFF
        z, err = V.zlib_inflate(s)
        if err is not None:
            choice = k; break
    assert choice is not None
    bad = bytearray(raw); bad[off + choice] ^= 0xFF
    q = tmp_path / "corrupt.bam"; q.write_bytes(bytes(bad))
    errs = []
    for opener in (lambda: pkg.bam_open_seeds(lib, q, INTERVALS, threads=3), lambda: inflater.bam_open_seeds(q, INTERVALS, threads=3)):
        with pytest.raises(pkg.HlalaError) as e:
            opener()
        errs.append(str(e.value))
    assert errs[0] == errs[1] == "BGZF inflate failed"


def _stub(path, text):
    path.write_text(text)
    path.chmod(path.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)


def test_hla_la_with_gpu_inflate_writes_the_same_files(pkg, tmp_path):
    from tools import synth
    from test_bam import batch_records, write_bam
    from test_end_to_end import write_graph_dir
    from test_graph_files import write_contigs_dir, write_graph_txt
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
    base = [EXE, "--action", "HLA", "--maxThreads", "2", "--sampleID", "S1", "--PRG_graph_dir", str(gdir), "--FASTQU", str(tmp_path / "r1.fq"), "--FASTQ1", str(tmp_path / "r1.fq"),
            "--FASTQ2", str(tmp_path / "r2.fq"), "--bwa_bin", str(tmp_path / "bwa"), "--samtools_bin", str(tmp_path / "samtools"), "--mapAgainstCompleteGenome", "0", "--longReads", "0",
            "--loci", "A", "--rngSeed", "5"]
    outs = {}
    for g in ("0", "1"):
        outs[g] = tmp_path / ("out" + g)
        r = subprocess.run(base + ["--outputDirectory", str(outs[g]), "--gpuInflate", g], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Processed 300 protoSeeds (read pairs)" in r.stdout and "End-to-end: " in r.stdout
        # which path ran: with 1 every non-empty block of the BAM went through the GPU and none had to be redone; with 0 the program says nothing about it
        n_blocks = sum(1 for _, _, isz in _blocks_of(bam)[1] if isz)
        assert (f"BGZF inflate: {n_blocks} blocks on the GPU, 0 rejected there and inflated again on the host, 0 on the host only" in r.stdout) == (g == "1"), r.stdout[-2000:]
        assert ("BGZF inflate:" in r.stdout) == (g == "1")
    files = sorted(os.listdir(outs["0"] / "hla"))
    assert files == sorted(os.listdir(outs["1"] / "hla")) and "R1_bestguess.txt" in files
    for fn in files:
        assert (outs["1"] / "hla" / fn).read_bytes() == (outs["0"] / "hla" / fn).read_bytes(), fn
    assert (outs["1"] / "reads_per_level.txt").read_bytes() == (outs["0"] / "reads_per_level.txt").read_bytes()
