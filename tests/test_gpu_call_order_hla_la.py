"""HLA-LA --gpuCallOrder 1: the order of every locus's pair table made on the GPU (hlala_set_call_order_gpu).  The switch changes where the order is made, not one
byte of what the program writes: the files under hla/ and reads_per_level.txt of the small BAM of tests/test_gpu_filter_hla_la.py, with and without it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_gpu_call_order_writes_the_same_files(pkg, tmp_path):
    from tools import synth
    from test_bam import batch_records, write_bam
    from test_end_to_end import write_graph_dir
    from test_graph_files import write_contigs_dir, write_graph_txt
    from test_hla_la_binary import EXE, ROOT, _stub
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "hla-la_amd", "csrc"), "../bin/HLA-LA"])
    gdir = tmp_path / "graph"; gdir.mkdir()
    w = synth.make_world(seed=12, G=4000, k=1, n_mut=6, mut_density=0.03)
    lib = C.CDLL(pkg.LIB_PATH)
    write_graph_dir(gdir, w["H"], [(1200, 1470), (1900, 2176)])
    write_graph_txt(gdir / "PRG" / "graph.txt", w["graph"], np.random.default_rng(2))
    write_contigs_dir(gdir, w["contigs"], np.random.default_rng(3))
    b = synth.make_batch(w, 700, seed=77, haps=(2, 5))
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
    for name, extra in (("host", []), ("gpu", ["--gpuCallOrder", "1"])):
        out = tmp_path / name
        r = subprocess.run(base + ["--outputDirectory", str(out)] + extra, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Processed 700 protoSeeds (read pairs)" in r.stdout
        outs[name] = (out, r.stdout)
    assert "Pair table order:" not in outs["host"][1]
    line = [x for x in outs["gpu"][1].splitlines() if x.startswith("Pair table order: ")]
    assert line == ["Pair table order: 1 loci on the GPU, 0 on the host"], outs["gpu"][1][-2000:]
    files = sorted(os.listdir(outs["host"][0] / "hla"))
    assert files == sorted(os.listdir(outs["gpu"][0] / "hla")) and "R1_bestguess.txt" in files and len(files) == 9
    for fn in files:
        assert (outs["gpu"][0] / "hla" / fn).read_bytes() == (outs["host"][0] / "hla" / fn).read_bytes(), fn
    assert (outs["gpu"][0] / "reads_per_level.txt").read_bytes() == (outs["host"][0] / "reads_per_level.txt").read_bytes()
