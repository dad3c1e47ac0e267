"""The CRC-32 of inflated BGZF blocks on the GPU (hla-la_amd/csrc/kernel_crc32.hip: k_bgzf_crc32, one wavefront per block behind k_bgzf_inflate) behind
hlala_bgzf_inflate_crc, HLALA_SEEDS_VERIFY_CRC in the three decoders and `HLA-LA --verifyCRC 1`.  Expected CRCs are zlib.crc32, expected bytes zlib's."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import crc32_cases as K
import inflate_vectors as V
from test_gpu_inflate import CANARY, EXE, INTERVALS, ROOT, _blocks_of, _same_sample, _stub, vectors  # noqa: F401  (vectors: the module fixture of the inflate test)

pytestmark = pytest.mark.gpu
MISMATCH = 8          # HLALA_INFLATE_CRC_MISMATCH
TEXT = "BGZF block CRC mismatch"


@pytest.fixture(scope="module")
def inflater(pkg):
    f = pkg.Inflater(pkg.load_library(), device=0, chunk_bytes=pkg.INFLATE_MIN_CHUNK)
    yield f
    f.close()


def layout(streams, sizes, rng):
    """tests/test_gpu_inflate.py::layout -- streams in shuffled memory order with gaps, output ranges in another shuffled order with gaps, canaries everywhere else --
    with the output range of block i starting at an address that is i mod 16 (mod 16)"""
    n = len(streams)
    corder = rng.permutation(n); uorder = rng.permutation(n)
    coff = np.zeros(n, np.int64); uoff = np.zeros(n, np.int64)
    at = 7
    for i in corder:
        coff[i] = at; at += len(streams[i]) + int(rng.integers(0, 9))
    comp = np.full(at + 5, CANARY, np.uint8)
    for i in range(n):
        comp[coff[i]:coff[i] + len(streams[i])] = np.frombuffer(streams[i], np.uint8)
    at = 13
    for i in uorder:
        at += 1 + (i - at - 1) % 16
        uoff[i] = at; at += sizes[i] + int(rng.integers(1, 40))
    out = np.full(at + 11, CANARY, np.uint8)
    blocks = [(int(coff[i]), len(streams[i]), sizes[i], int(uoff[i])) for i in range(n)]
    return comp, out, blocks


@pytest.fixture(scope="module")
def placed():
    """every case twice, as a stored block and as a zlib-compressed one: (data per block, zlib's CRC per block, comp, blocks, size of out)"""
    datas = []; streams = []
    for _, d in K.cases():
        datas += [d, d]; streams += [K.stored(d), K.deflated(d)]
    comp, out, blocks = layout(streams, [len(d) for d in datas], np.random.default_rng(5))
    assert {b[3] % 16 for b in blocks} == set(range(16)) == {b[3] % 16 for b in blocks if b[2] >= 4095}
    crcs = np.array([zlib.crc32(d) for d in datas], np.uint32)
    return datas, crcs, comp, blocks, out.size


def _check_bytes(out, blocks, datas):
    covered = np.zeros(out.size, bool)
    for d, (co, cl, isz, uo) in zip(datas, blocks):
        covered[uo:uo + isz] = True
        assert out[uo:uo + isz].tobytes() == d
    assert (out[~covered] == CANARY).all(), "bytes outside the blocks' ranges were written"


def test_cases_with_the_right_crcs(pkg, inflater, placed):
    datas, crcs, comp, blocks, nout = placed
    assert sum(b[1] for b in blocks) > pkg.INFLATE_MIN_CHUNK                       # more than one chunk
    out = np.full(nout, CANARY, np.uint8)
    status, st, got = inflater.inflate(comp, blocks, out, crc=crcs, want_crc=True)
    assert (status == 0).all() and st.n_ok == len(blocks) and st.n_rejected == 0
    assert np.array_equal(got, crcs), [i for i in range(len(blocks)) if got[i] != crcs[i]][:10]
    _check_bytes(out, blocks, datas)
    assert inflater.ms_crc > 0
    # the CRCs alone
    out2 = np.full(nout, CANARY, np.uint8)
    status, st, got = inflater.inflate(comp, blocks, out2, want_crc=True)
    assert (status == 0).all() and np.array_equal(got, crcs) and np.array_equal(out2, out)
    # neither: the call of before
    out3 = np.full(nout, CANARY, np.uint8)
    res = inflater.inflate(comp, blocks, out3)
    assert len(res) == 2 and (res[0] == 0).all() and np.array_equal(out3, out) and res[1].n_ok == len(blocks)


def test_a_wrong_expected_crc_is_reported_for_its_block_only(pkg, inflater, placed):
    datas, crcs, comp, blocks, nout = placed
    wrong = crcs.copy()
    hit = np.arange(len(blocks)) % 3 == 0
    for i in np.nonzero(hit)[0]:
        wrong[i] ^= np.uint32(1 << (int(i) % 32))
    out = np.full(nout, CANARY, np.uint8)
    status, st, got = inflater.inflate(comp, blocks, out, crc=wrong, want_crc=True)
    assert np.array_equal(status, np.where(hit, MISMATCH, 0))
    assert st.n_rejected == int(hit.sum()) and st.n_ok == len(blocks) - int(hit.sum())
    assert np.array_equal(got, crcs)
    _check_bytes(out, blocks, datas)                                                # the mismatching blocks' bytes are delivered as well
    assert pkg.INFLATE_STATUS[MISMATCH] == "crc mismatch"


def test_every_flipped_payload_bit_of_a_stored_block_is_caught(pkg, inflater):
    """one bit flipped in the payload of a stored block: the length is unchanged, inflate accepts, the CRC cannot match.  Places: the first and the last byte of the block and of
    the segments of lanes 0, 1, 32 and 63 (for 257 bytes lanes 0..30 own nothing: there the first lane that owns a byte stands in as well)"""
    rng = np.random.default_rng(9)
    streams = []; sizes = []; expect = []; flipped = []
    for n in (257, 65536):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        first_owner = min(j for j in range(64) if K.segment(n, j)[1] > K.segment(n, j)[0])
        places = {0, n - 1}
        for j in (0, 1, 32, 63, first_owner):
            lo, hi = K.segment(n, j)
            if hi > lo:
                places |= {lo, hi - 1}
        assert len(places) >= 5
        streams.append(K.stored(data)); sizes.append(n); expect.append(zlib.crc32(data)); flipped.append(None)       # the block itself: accepted
        for k, i in enumerate(sorted(places)):
            s = bytearray(K.stored(data)); s[K.stored_position(i)] ^= 1 << (k % 8)
            d = bytearray(data); d[i] ^= 1 << (k % 8)
            assert V.zlib_inflate(s)[0] == bytes(d)
            streams.append(bytes(s)); sizes.append(n); expect.append(zlib.crc32(data)); flipped.append(bytes(d))
    comp, out, blocks = layout(streams, sizes, rng)
    status, st, got = inflater.inflate(comp, blocks, out, crc=np.array(expect, np.uint32), want_crc=True)
    for i, f in enumerate(flipped):
        assert status[i] == (0 if f is None else MISMATCH), (i, sizes[i])
        if f is not None:
            assert got[i] == zlib.crc32(f) and out[blocks[i][3]:blocks[i][3] + sizes[i]].tobytes() == f
    assert st.n_rejected == sum(f is not None for f in flipped)


def test_device_addresses_at_every_residue(pkg, inflater):
    """In the staging buffer of a chunk the outputs of its blocks stand one behind the other, whatever uoff says: 16 blocks of 4097 bytes in one chunk start at device
    offsets 0, 4097, 2 * 4097, ... = every residue mod 16 (L = 68: several 16-byte loads per lane between a head and a tail of bytes)"""
    rng = np.random.default_rng(16)
    datas = [rng.integers(0, 256, 4097, dtype=np.uint8).tobytes() for _ in range(16)]
    streams = [K.stored(d) for d in datas]
    assert sum(len(s) for s in streams) + 16 * 16 < pkg.INFLATE_MIN_CHUNK           # one chunk
    at = 0; blocks = []
    for k, s in enumerate(streams):
        blocks.append((at, len(s), 4097, k * 4100)); at += len(s)
    comp = np.frombuffer(b"".join(streams), np.uint8)
    out = np.full(16 * 4100, CANARY, np.uint8)
    status, st, got = inflater.inflate(comp, blocks, out, want_crc=True)
    assert (status == 0).all() and got.tolist() == [zlib.crc32(d) for d in datas]
    _check_bytes(out, blocks, datas)


def test_the_vector_set_keeps_its_inflate_statuses(pkg, inflater, vectors):
    from test_gpu_inflate import layout as plain_layout
    comp, out, blocks = plain_layout(vectors, np.random.default_rng(len(vectors)))
    assert sum(len(v[1]) for v in vectors) > 3 * pkg.INFLATE_MIN_CHUNK             # the call spans several chunks: the CRC kernel runs per chunk, on chunk-local indices
    expect = np.array([zlib.crc32(d) if d is not None else 0x12345678 for _, _, _, d, _ in vectors], np.uint32)
    status, st, got = inflater.inflate(comp, blocks, out, crc=expect, want_crc=True)
    n_bad = 0
    for (name, s, isize, data, want), (co, cl, isz, uo), stt, crc in zip(vectors, blocks, status, got):
        assert stt == want and stt != MISMATCH, (name, pkg.INFLATE_STATUS[stt], pkg.INFLATE_STATUS[want])
        if want == 0:
            assert crc == zlib.crc32(data) and out[uo:uo + isz].tobytes() == data, name
        else:
            assert crc == 0, name
            n_bad += 1
    assert n_bad > 100 and st.n_rejected == n_bad and st.n_ok == len(vectors) - n_bad >= 70


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    from test_bam import make_records, write_bam
    refs, recs = make_records(np.random.default_rng(8), n_names=400, lengths=(149, 150, 151, 97))
    p = tmp_path_factory.mktemp("gpu_bgzf_crc") / "t.bam"
    write_bam(p, refs, recs, block=3000)
    return p


def _openers(pkg, inflater, path, flags):
    lib = pkg.load_library()
    return [("host", lambda: pkg.bam_open_seeds(lib, path, INTERVALS, threads=3, flags=flags)),
            ("gpu inflate", lambda: inflater.bam_open_seeds(path, INTERVALS, threads=3, flags=flags)),
            ("gpu inflate + parse", lambda: inflater.bam_open_seeds(path, INTERVALS, threads=3, flags=flags | pkg.SEEDS_GPU_PARSE))]


def test_bam_decoded_with_the_flag_is_the_same_sample(pkg, inflater, bam, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")                         # several rounds
    sizes = [isz for _, _, isz in _blocks_of(bam)[1]]
    n_all = len(sizes); n_nonempty = sum(1 for s in sizes if s)
    assert n_nonempty > 50 and n_all > n_nonempty                                  # (the end-of-file block is empty)
    H = pkg.bam_open_seeds(pkg.load_library(), bam, INTERVALS, threads=3)
    assert H.crc_counts() == (0, 0, 0)
    for name, opener in _openers(pkg, inflater, bam, pkg.SEEDS_VERIFY_CRC):
        S = opener()
        _same_sample(S, H)
        c = S.crc_counts()
        assert sum(c[:2]) == n_all and c[2] == 0, (name, c)
        assert c[0] == S.inflate_counts()[0] == (0 if name == "host" else n_nonempty), (name, c)
        S.close()
    for name, opener in _openers(pkg, inflater, bam, 0):
        S = opener()
        assert S.crc_counts() == (0, 0, 0), name
        S.close()
    H.close()


def test_corrupt_files_fail_with_one_text_on_every_path(pkg, inflater, bam, tmp_path, monkeypatch):
    monkeypatch.setenv("HLALA_BAM_SEGMENT_BYTES", "65536")
    raw, blocks = _blocks_of(bam)
    off, clen, isize = blocks[5]
    # (a) the stored CRC field of block 5, one bit
    a = bytearray(raw); a[off + clen + 1] ^= 0x10
    pa = tmp_path / "crc_field.bam"; pa.write_bytes(bytes(a))
    # (b) a payload bit of block 5 that zlib still inflates to isize bytes, but other ones
    good = V.zlib_inflate(raw[off:off + clen])[0]
    assert good is not None and len(good) == isize and zlib.crc32(good) == int.from_bytes(raw[off + clen:off + clen + 4], "little")
    choice = None
    for bit in range(8 * clen - 1, -1, -1):
        s = bytearray(raw[off:off + clen]); s[bit >> 3] ^= 1 << (bit & 7)
        z, err = V.zlib_inflate(s)
        if err is None and len(z) == isize and z != good:
            choice = bit; break
    assert choice is not None
    b = bytearray(raw); b[off + (choice >> 3)] ^= 1 << (choice & 7)
    pb = tmp_path / "payload.bam"; pb.write_bytes(bytes(b))
    for path in (pa, pb):
        for name, opener in _openers(pkg, inflater, path, pkg.SEEDS_VERIFY_CRC):
            with pytest.raises(pkg.HlalaError) as e:
                opener()
            assert str(e.value) == TEXT, (path.name, name)
    # without the flag nobody looks at the field: the default did not move
    H = pkg.bam_open_seeds(pkg.load_library(), bam, INTERVALS, threads=3)
    for name, opener in _openers(pkg, inflater, pa, 0):
        S = opener()
        _same_sample(S, H)
        S.close()
    H.close()


def test_hla_la_with_verify_crc_writes_the_same_files(pkg, tmp_path):
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
    n_blocks = len(_blocks_of(bam)[1])
    outs = {}
    for name, extra in (("plain", []), ("crc", ["--gpuParse", "1", "--verifyCRC", "1"])):
        outs[name] = tmp_path / ("out_" + name)
        r = subprocess.run(base + ["--outputDirectory", str(outs[name])] + extra, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Processed 300 protoSeeds (read pairs)" in r.stdout
        m = re.findall(r"^BGZF CRC-32: (\d+) blocks verified on the GPU, (\d+) on the host$", r.stdout, re.M)
        if name == "plain":
            assert m == [] and "BGZF CRC-32:" not in r.stdout
        else:
            assert len(m) == 1 and int(m[0][0]) + int(m[0][1]) == n_blocks and int(m[0][0]) > 0, r.stdout[-2000:]
    files = sorted(os.listdir(outs["plain"] / "hla"))
    assert files == sorted(os.listdir(outs["crc"] / "hla")) and "R1_bestguess.txt" in files
    for fn in files:
        assert (outs["crc"] / "hla" / fn).read_bytes() == (outs["plain"] / "hla" / fn).read_bytes(), fn
    assert (outs["crc"] / "reads_per_level.txt").read_bytes() == (outs["plain"] / "reads_per_level.txt").read_bytes()
