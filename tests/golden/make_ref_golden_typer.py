"""Regenerates tests/golden/ref_typer_<family>.npz: what the REFERENCE's own typer (hla/HLATyper.cpp) makes of the sample families of tests/ref_typer.py.

The expected outputs are written by HLA*LA's code: oracle/_ref/libhlala_ref.so, built from a checkout of the reference by oracle/ref/Makefile, through
ref_typer_include / ref_typer_exon_positions / ref_typer_infer of oracle/ref/ref_driver.cpp.  Data only: the family's parameters (world, sample and graph
directory are rebuilt from their seeds), the include decision, digests of the alignments the reference was fed (the oracle's, pinned by
tests/test_reference_pin_pipeline.py) with their mapping qualities, the reference's exon positions per locus and the files HLATypeInference wrote, byte for
byte.  tests/test_gpu_reference_pin_typer.py holds the HIP kernels and the host writer against these files directly; tests/test_reference_pin_typer.py checks
that they are what the reference writes today.

Every file stays below MAX_BYTES, the size of the largest fixture that was here before.  Run (needs the reference sources; HLALA_REF_DIR names them):
    python tests/golden/make_ref_golden_typer.py
The files carry the SHA-256 over the compiled reference sources (REF_SRCS + REF_SRCS_PIPELINE of oracle/ref/Makefile) as meta__ref_sources_sha256, and their
bytes depend on their content alone: a second run reproduces them bit for bit."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package              # noqa: E402
from oracle_binding import Oracle              # noqa: E402
import ref_binding as rb                       # noqa: E402
import ref_typer as rt                         # noqa: E402

MAX_BYTES = 138652            # ref_fan.npz, the largest fixture here before these


def main():
    ok, why = rb.available()
    if not ok:
        raise SystemExit(why)
    sha = rb.sources_hash(pipeline=True)
    print("reference sources sha256 (aligner + pipeline):", sha)
    pkg = load_package(); lib = C.CDLL(pkg.LIB_PATH)
    for family in rt.FAMILIES:
        case = rt.build_case(family); w, b = case["world"], case["batch"]
        with tempfile.TemporaryDirectory() as tmp:
            gdir = os.path.join(tmp, "graph"); rt.write_graph_dir(gdir, case)
            o = Oracle(w["graph"], w["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=5, long_read_mode=1 if case["long_mode"] else 0, max_columns=case["stride"])
            pairs = (o.align_batch(b) if case["paired"] else o.align_long_reads(b))["pairs"]
            T = pkg.Typer(lib, gdir); loci = {}
            for locus in rt.LOCI:
                L = T.locus(locus); loci[locus] = (L.level_min, L.level_to_exon); L.free()
            T.close()
            ref = rt.reference_run(rb, case, gdir, pairs, tmp, loci)
        path = rt.fixture_path(family)
        rt.save_fixture(path, rt.pack_fixture(family, ref, sha))
        size = os.path.getsize(path)
        print("wrote %s: %d bytes; %d levels, %d units (%d included), %d bytes of files" %
              (os.path.basename(path), size, w["graph"]["n_levels"], b["n_pairs"], int(ref["include"].sum()), sum(len(v) for v in ref["files"].values())))
        assert size <= MAX_BYTES, "%s is larger than the largest fixture that was here before" % path


if __name__ == "__main__":
    main()
