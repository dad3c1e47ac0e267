"""BGZF inflate on the GPU with the block's history in LDS (hla-la_amd/csrc/kernel_inflate_lds.hip: k_bgzf_inflate_lds, one workgroup of two wavefronts per block),
chosen per inflater with hlala_inflater_set_kernel, behind the same entry points as k_bgzf_inflate (tests/test_gpu_inflate.py).  Expected bytes are zlib's; expected
statuses are those of the host model of this kernel, which tests/test_inflate_lds_model.py shows equal to the first kernel's model and bounded on every stream used here."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import inflate_lds_vectors as L
import inflate_vectors as V
from test_gpu_inflate import CANARY, EXE, INTERVALS, ROOT, _blocks_of, _same_sample, _stub, layout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vectors(pkg):
    """[(name, stream, isize, zlib's bytes or None, status of the host model)]: the interleaved valid / malformed / bit-flip set of tests/test_gpu_inflate.py and, spread
    among it, the vectors made for the ring, the batches and the rounds"""
    valid = [(n, s, z, d) for n, s, z, d in V.valid_vectors()]
    bad = [(n, s, z, None) for n, s, z, _, _ in V.malformed_vectors() + V.truncation_vectors()]
    flip, fdata = V.flip_stream()
    for bit in range(8 * len(flip)):
        s = bytearray(flip); s[bit >> 3] ^= 1 << (bit & 7)
        z, err = V.zlib_inflate(s)
        bad.append(("flip_%d" % bit, bytes(s), len(fdata), z if err is None and len(z) == len(fdata) else None))
    new = [(n, s, z, d) for n, s, z, d in L.lds_valid_vectors()] + [(n, s, z, None) for n, s, z, _, _ in L.lds_error_vectors()]
    out = []
    for i in range(max(len(valid), len(bad), len(new))):
        out += new[i:i + 1] + valid[i:i + 1] + bad[i:i + 1]
    res = []
    for n, s, z, d in out:
        st, got = pkg.host_inflate_lds_model(s, z)
        if d is not None and not n.startswith("flip_"):
            assert st == 0, n
        if st == 0:
            assert d is not None and got == d, n                 # (the model never accepts what zlib does not give)
        res.append((n, s, z, d if st == 0 else None, st))
    return res


@pytest.fixture(scope="module")
def inflater_handle(pkg):
    f = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    yield f
    f.close()


@pytest.fixture()
def inflater(pkg, inflater_handle):
    inflater_handle.set_kernel(pkg.INFLATE_KERNEL_LDS)
    return inflater_handle


def check_call(pkg, vec, blocks, out, status, st):
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
    return n_bad


@pytest.mark.parametrize("n_blocks", [1, 65, None])
def test_vectors_through_one_call(pkg, inflater, vectors, n_blocks):
    vec = vectors if n_blocks is None else vectors[:n_blocks]
    comp, out, blocks = layout(vec, np.random.default_rng(len(vec)))
    if n_blocks is None:
        assert sum(len(v[1]) for v in vec) > 3 * pkg.INFLATE_MIN_CHUNK                # the call spans several chunks
    assert inflater.kernel == pkg.INFLATE_KERNEL_LDS
    status, st = inflater.inflate(comp, blocks, out)
    n_bad = check_call(pkg, vec, blocks, out, status, st)
    if n_blocks is None:
        assert n_bad > 100 and st.n_ok >= 130 and st.ms_kernel > 0


def test_the_two_kernels_on_one_inflater(pkg, inflater, vectors):
    vec = vectors[:200]
    comp, out0, blocks = layout(vec, np.random.default_rng(3))
    res = []
    for kind in (pkg.INFLATE_KERNEL_LDS, pkg.INFLATE_KERNEL_HBM, pkg.INFLATE_KERNEL_LDS, pkg.INFLATE_KERNEL_HBM):
        inflater.set_kernel(kind)
        assert inflater.kernel == kind
        out = out0.copy()
        status, st = inflater.inflate(comp, blocks, out)
        check_call(pkg, vec, blocks, out, status, st)
        # (a rejected block's range may hold what was placed before the error: compare what the caller receives, the accepted blocks and everything outside the ranges)
        for (co, cl, isz, uo), s in zip(blocks, status):
            if s != 0:
                out[uo:uo + isz] = 0
        res.append((status.copy(), out))
    for status, out in res[1:]:
        assert np.array_equal(status, res[0][0]) and np.array_equal(out, res[0][1])
    inflater.set_kernel(pkg.INFLATE_KERNEL_LDS)
    for kind in (2, -1, 7, 1 << 20):
        with pytest.raises(pkg.HlalaError, match=r"\(-1\)"):                  # HLALA_E_ARG
            inflater.set_kernel(kind)
        assert inflater.kernel == pkg.INFLATE_KERNEL_LDS                      # the choice stays as it was
    lib = pkg.load_library()
    assert lib.hlala_inflater_set_kernel(None, 0) == -1 and lib.hlala_inflater_get_kernel(None) == -1
    fresh = pkg.Inflater(lib, device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    assert fresh.kernel == pkg.INFLATE_KERNEL_HBM                             # a new handle has kind 0
    fresh.close()


def test_flush_at_every_alignment(pkg, inflater):
    """output ranges at every offset mod 16 and of 1 to 17, 63, 64 and 65 bytes: unaligned head, 4-byte stores, tail; canaries on both sides of every range"""
    vec = L.alignment_vectors()
    at = 0; blocks = []; coff = 0; comp = bytearray()
    for name, s, isize, data, a in vec:
        at = ((at + 40) & ~15) + 16 + a                                       # at least 24 canary bytes between two ranges
        blocks.append((coff, len(s), isize, at)); comp += s; coff += len(s); at += isize
    out = np.full(at + 64, CANARY, np.uint8)
    assert sorted(set(b[3] % 16 for b in blocks)) == list(range(16))
    status, st = inflater.inflate(np.frombuffer(bytes(comp), np.uint8).copy(), blocks, out)
    covered = np.zeros(out.size, bool)
    for (name, s, isize, data, a), (co, cl, isz, uo), got in zip(vec, blocks, status):
        assert got == 0 and out[uo:uo + isz].tobytes() == data, name
        covered[uo:uo + isz] = True
    assert (out[~covered] == CANARY).all(), "bytes outside the blocks' ranges were written"


def test_crc_behind_the_lds_kernel(pkg, inflater, vectors):
    vec = [v for v in vectors if v[4] == 0][:60]
    comp, out, blocks = layout(vec, np.random.default_rng(9))
    expect = np.array([zlib.crc32(v[3]) for v in vec], np.uint32)
    status, st, got = inflater.inflate(comp, blocks, out, crc=expect, want_crc=True)
    assert (status == 0).all() and np.array_equal(got, expect) and inflater.ms_crc > 0
    wrong = expect.copy(); wrong[7] ^= 1; wrong[31] ^= 0x80000000
    status, st, got = inflater.inflate(comp, blocks, out, crc=wrong, want_crc=True)
    assert [i for i, s in enumerate(status) if s != 0] == [7, 31] and status[7] == status[31] == 8 and pkg.INFLATE_STATUS[8] == "crc mismatch"
    assert np.array_equal(got, expect) and st.n_rejected == 2
    for v, (co, cl, isz, uo) in zip(vec, blocks):
        assert out[uo:uo + isz].tobytes() == v[3]


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    from test_bam import make_records, write_bam
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    p = tmp_path_factory.mktemp("gpu_inflate_lds") / "t.bam"
    write_bam(p, refs, recs, block=3000)
    return p, refs, recs


def test_bam_decoded_with_the_lds_kernel_is_the_same_sample(pkg, inflater, bam, monkeypatch):
    from test_bam import check, expected_batch
    p, refs, recs = bam
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                   # records straddle rounds
    lib = pkg.load_library()
    n_nonempty = sum(1 for _, _, isz in _blocks_of(p)[1] if isz)
    assert n_nonempty > 50
    for flags in (0, pkg.SEEDS_GPU_PARSE, pkg.SEEDS_VERIFY_CRC):             # host destination, device destination, k_bgzf_crc32 behind the kernel
        H = pkg.bam_open_seeds(lib, p, INTERVALS, threads=3, flags=flags & ~pkg.SEEDS_GPU_PARSE)
        G = inflater.bam_open_seeds(p, INTERVALS, threads=3, flags=flags)
        _same_sample(G, H)
        assert G.inflate_counts() == (n_nonempty, 0, 0)                       # nothing rejected: the host engine never stood in for the kernel
        if flags & pkg.SEEDS_GPU_PARSE:
            assert G.parse_counts()[0] == len(recs) and G.parse_counts()[2] == 0      # ... and no round fell back to the host's record pass
        if flags & pkg.SEEDS_VERIFY_CRC:
            assert G.crc_counts()[0] == n_nonempty                            # k_bgzf_crc32 read what k_bgzf_inflate_lds wrote
        assert G.n_units > 50
        G.close(); H.close()
    assert inflater.kernel == pkg.INFLATE_KERNEL_LDS
    b, names, cnt, counts = inflater.bam_extract_seeds_gpu(p, INTERVALS, threads=1)
    units, examined, n_seeds, n_inc = expected_batch(recs, refs, INTERVALS, False)
    check(b, names, cnt, units, examined, n_seeds, n_inc, False)


def test_a_corrupt_block_fails_like_the_host_path(pkg, inflater, bam, tmp_path):
    p, refs, recs = bam
    raw, blocks = _blocks_of(p)
    lib = pkg.load_library()
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


def test_hla_la_with_the_lds_kernel_writes_the_same_files(pkg, tmp_path):
    import ctypes as C
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
    n_blocks = sum(1 for _, _, isz in _blocks_of(bam)[1] if isz)
    outs = {}
    for g, extra in (("0", ["--gpuInflate", "0", "--gpuInflateKernel", "1"]), ("1", ["--gpuInflate", "1", "--gpuInflateKernel", "1"])):
        outs[g] = tmp_path / ("out" + g)
        r = subprocess.run(base + ["--outputDirectory", str(outs[g])] + extra, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Processed 300 protoSeeds (read pairs)" in r.stdout and "End-to-end: " in r.stdout
        # with --gpuInflate 1 every non-empty block went through k_bgzf_inflate_lds and none had to be redone; without it the kernel choice means nothing and nothing is said
        assert (f"BGZF inflate: {n_blocks} blocks on the GPU, 0 rejected there and inflated again on the host, 0 on the host only" in r.stdout) == (g == "1"), r.stdout[-2000:]
        assert ("BGZF inflate kernel: k_bgzf_inflate_lds" in r.stdout) == (g == "1"), r.stdout[-2000:]
    files = sorted(os.listdir(outs["0"] / "hla"))
    assert files == sorted(os.listdir(outs["1"] / "hla")) and "R1_bestguess.txt" in files
    for fn in files:
        assert (outs["1"] / "hla" / fn).read_bytes() == (outs["0"] / "hla" / fn).read_bytes(), fn
    assert (outs["1"] / "reads_per_level.txt").read_bytes() == (outs["0"] / "reads_per_level.txt").read_bytes()
