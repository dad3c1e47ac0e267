"""The overflow class of the pairing stage (hlala_set_pair_overflow; k_pair_overflow, csrc/kernel_pair_overflow.hip) on the families of
tests/pair_overflow_cases.py and on the families of tests/pair_edge_cases.py that hold pairs beyond the capacities.

With the class on, only pairs with a flagged record are refused; every other pair equals the oracle's (integers, column rows and Phred bytes exactly, pair_ll
within rtol 1e-12, posteriors exactly) and lies within the bounds of tests/pair_reference.py without capacities, fused and stage by stage.  Pairs within the
capacities are bit-identical with the class on and off, and so are the list counters of the pairing kernels; with the class off the pairs beyond the
capacities carry the refusal they always had.  A pair that needs more than the per-wave slab is refused and counted, whichever wave draws it.

Statistics and the pairing stage's time with the class on and off are printed (pytest -s)."""
import numpy as np
import pytest

import pair_edge_cases as pe
import pair_overflow_cases as po
import pair_reference as pr
import ref_pipeline as rp

pytestmark = pytest.mark.gpu

WC_PAIR_MULTI, WC_PAIR_OVER = 40, 72          # csrc/batch.h; WC_PAIR_OVER: [+0] listed, [+1] fetched, [+2] scored, [+3] refused for want of slab; [+4 ..] the side-stream pass
SCALARS = ("pair_status", "best_chain", "n_combinations", "strands_valid", "n_cols", "pair_mapq", "mate_mapq", "pair_ll")
PER_READ = ("best_chain", "n_cols", "mate_mapq")
SCRATCH = 64 << 20          # 1 MiB per wave: every pair of every family fits (the largest, 65 x 65 under 384 columns, needs 49 368 bytes)
FAMILIES = dict(po.NEW_FAMILIES, counts=pe.counts, unpaired=pe.unpaired, fan=pe.fan, **{"records-error": lambda: pe.records(True)})


def _context(pkg, f, rng_seed=5):
    b = f["batch"]
    return pkg.Context(f["world"]["graph"], f["world"]["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=rng_seed, max_columns=f["max_columns"])


def _batch(ctx, f, b):
    return ctx.batch_unpaired(b) if f.get("unpaired") else ctx.batch(b)


def _fused(ctx, f):
    gb = _batch(ctx, f, f["batch"]); gb.align()
    out = (gb.pairs(), gb.work_counters(), gb.pair_overflow_counts(), gb.stats())
    gb.close()
    return out


def _equal_runs(a, z, label):
    for k in SCALARS + rp.PAIR_COLS:
        assert np.array_equal(a[k], z[k]), (label, k)


def _equal_units(a, z, units, per, label):
    """Units `units` of two runs: every scalar and every column row, bit for bit."""
    st = a["_stride"]
    assert st == z["_stride"]
    for u in units:
        rows = slice(per * u, per * u + per)
        for k in SCALARS:
            s = rows if k in PER_READ else slice(u, u + 1)
            assert np.array_equal(a[k][s], z[k][s]), (label, u, k)
        for k in rp.PAIR_COLS:
            assert np.array_equal(a[k][per * u * st:(per * u + per) * st], z[k][per * u * st:(per * u + per) * st]), (label, u, k)


def _refusal(got, units, per, label):
    for u in units:
        assert got["pair_status"][u] == -1 and got["n_combinations"][u] == 0 and all(got["best_chain"][r] == -1 and got["n_cols"][r] == 0 for r in range(per * u, per * u + per)), (label, u)


def _against_oracle(got, exp, units, per, label):
    sg, se = got["_stride"], exp["_stride"]
    for u in units:
        for k in ("n_combinations", "strands_valid", "pair_mapq"):
            assert got[k][u] == exp[k][u], (label, u, k, got[k][u], exp[k][u])
        assert np.isclose(got["pair_ll"][u], exp["pair_ll"][u], rtol=1e-12, atol=0), (label, u, "pair_ll")
        for r in range(per * u, per * u + per):
            for k in PER_READ:
                assert got[k][r] == exp[k][r], (label, u, k, got[k][r], exp[k][r])
            n = int(exp["n_cols"][r])
            for k in rp.PAIR_COLS:
                assert np.array_equal(got[k][r * sg:r * sg + n], exp[k][r * se:r * se + n]), (label, u, k)


def _sets(f):
    """(pairs with a flagged record, pairs that a capacity alone keeps from the pairing kernels)."""
    flagged = set(f["oracle_fails"])
    return flagged, set(f["beyond"] if "beyond" in f else f["refused"]) - flagged


@pytest.mark.parametrize("name", list(FAMILIES))
def test_overflow_class_scores_what_the_capacities_refuse(pkg, oracle, name):
    f = FAMILIES[name]()
    b = f["batch"]; n = b["n_pairs"]; per = 1 if f.get("unpaired") else 2
    flagged, beyond = _sets(f)
    inside = [u for u in range(n) if u not in beyond and u not in flagged]
    ctx = _context(pkg, f)
    ctx.set_pair_overflow(SCRATCH)          # (on the parent commit: no such method)
    assert ctx.pair_overflow() == (SCRATCH, SCRATCH // pkg.PAIR_OVERFLOW_WAVES)
    # ---- class on: fused; stage by stage, the pairing stage twice
    gb = _batch(ctx, f, b); gb.align()
    fused = gb.pairs(); wcf = gb.work_counters(); ext = gb.chains(1); seeds = gb.chains(0); st_on = gb.stats(); cf = gb.pair_overflow_counts()
    gs = _batch(ctx, f, b); gs.project(); gs.extend(); gs.pair()
    staged = gs.pairs(); wcs = gs.work_counters(); cs = gs.pair_overflow_counts()
    gs.pair()
    again = gs.pairs(); ca = gs.pair_overflow_counts()
    _equal_runs(fused, staged, name + ": fused / staged"); _equal_runs(staged, again, name + ": pairing stage called again")
    nb = len(beyond)
    assert cf == cs == ca == (nb, nb, 0), (name, cf, cs, ca, nb)
    assert wcs[WC_PAIR_OVER] == nb and wcs[WC_PAIR_OVER + 4] == 0 and wcf[WC_PAIR_OVER] + wcf[WC_PAIR_OVER + 4] == nb
    # ---- only flagged pairs are refused
    reads = [r for u in range(n) if u not in flagged for r in range(per * u, per * u + per)]
    assert np.array_equal(pe.kept_counts(b, seeds["status"], per)[reads], f["kept"][reads])
    got_refused = {u for u in range(n) if fused["pair_status"][u] != 0}
    assert got_refused == flagged, (name, sorted(got_refused), sorted(flagged))
    # ---- the exact reference without capacities, on the library's own extended chains
    units = pr.batch_units(b, ext, f["world"]["contigs"], b["insert_mean"], b["insert_sd"], unpaired=per == 1, capacities=False)
    assert set(pe.refused_by_capacity(units)) == flagged
    with_cap = pr.batch_units(b, ext, f["world"]["contigs"], b["insert_mean"], b["insert_sd"], unpaired=per == 1, want_columns=False)
    assert set(pe.refused_by_capacity(with_cap)) == flagged | beyond, "the family's pairs beyond the capacities are not the ones pair_reference refuses"
    s = pe.check_units(units, fused, name, per, refused=flagged)
    po.check_floors(s, f, name)
    assert s["refused"] == len(flagged)
    # ---- the oracle (without the pairs it cannot be given, which are the last ones)
    bo, exp = pe.oracle_answers(oracle, f)
    _against_oracle(fused, exp["pairs"], [u for u in range(bo["n_pairs"]) if u not in flagged], per, name)
    # hlala_batch_get_stats: n_errors keeps counting flagged chains only
    n_flagged = int((seeds["status"][:b["n_chains"]] < 0).sum() + ((ext["status"][:b["n_chains"]] < 0) & (seeds["status"][:b["n_chains"]] >= 0)).sum())
    assert st_on.n_errors == n_flagged == (1 if name == "records-error" else 0)
    if "deferred" in f and beyond:
        # the pair beyond the capacities that waits for the side-stream DP classes was listed by the second pairing pass, which has its own list, counters and slabs
        assert wcf[WC_PAIR_OVER + 4] >= 1 and wcf[WC_PAIR_OVER + 4 + 2] == wcf[WC_PAIR_OVER + 4], (name, wcf[WC_PAIR_OVER:WC_PAIR_OVER + 8].tolist())
    # ---- class off: pairs within the capacities do not move, the others carry the refusal they always had
    ctx.set_pair_overflow(0)
    assert ctx.pair_overflow() == (0, 0)
    off, wco, co, st_off = _fused(ctx, f)
    assert co == (0, 0, 0) and not wco[WC_PAIR_OVER:WC_PAIR_OVER + 8].any()
    _equal_units(fused, off, inside, per, name + ": class on / off")
    assert np.array_equal(wcf[WC_PAIR_MULTI:WC_PAIR_MULTI + 8], wco[WC_PAIR_MULTI:WC_PAIR_MULTI + 8]), (name, "list counters of k_pair_multi with the class on / off")
    _refusal(off, beyond | flagged, per, name + ": class off")
    assert {u for u in range(n) if off["pair_status"][u] != 0} == beyond | flagged
    # ---- on again: both answers come back
    ctx.set_pair_overflow(SCRATCH)
    on2, wc2, c2, _ = _fused(ctx, f)
    _equal_runs(fused, on2, name + ": on, off, on"); assert c2 == (nb, nb, 0)
    ctx.set_pair_overflow(0)
    off2, _, c3, _ = _fused(ctx, f)
    _equal_units(off, off2, range(n), per, name + ": off, on, off"); assert c3 == (0, 0, 0)
    print("%s: %d pairs beyond the capacities; pairing stage %.3f ms with the class on, %.3f ms off" % (name, nb, st_on.ms_pair, st_off.ms_pair))
    gb.close(); gs.close(); ctx.close()


def test_a_pair_beyond_the_slab_is_refused_and_counted(pkg):
    """over-counts under a slab that holds 65 x 16 (and 130 x 3, 129 x 1, 128 x 2) but not 65 x 65: exactly that pair is refused, the counts are (6, 5, 1), and
    every other pair is what it is under a large slab."""
    f = po.over_counts(); n = f["batch"]["n_pairs"]
    need = lambda n1, n2: pkg.pair_overflow_need(n1, n2, f["max_columns"])
    slab = (need(65, 16) + 15) // 16 * 16
    assert need(65, 16) <= slab < need(65, 65) and all(need(a, c) <= slab for a, c in po.OVER_COUNTS if (a, c) != (65, 65))
    ctx = _context(pkg, f)
    ctx.set_pair_overflow(SCRATCH)
    large, _, cl, _ = _fused(ctx, f)
    ctx.set_pair_overflow(slab * pkg.PAIR_OVERFLOW_WAVES)
    assert ctx.pair_overflow() == (slab * pkg.PAIR_OVERFLOW_WAVES, slab)
    small, _, csm, _ = _fused(ctx, f)
    big = po.OVER_COUNTS.index((65, 65))
    assert cl == (6, 6, 0) and csm == (6, 5, 1), (cl, csm)
    assert {u for u in range(n) if small["pair_status"][u] != 0} == {big}
    _refusal(small, [big], 2, "65 x 65 under the small slab")
    _equal_units(large, small, [u for u in range(n) if u != big], 2, "large / small slab")
    # a slab one step of 16 bytes short of 65 x 16 refuses that pair as well (130 x 3 needs 48 bytes less and stays)
    ctx.set_pair_overflow((slab - 16) * pkg.PAIR_OVERFLOW_WAVES)
    tiny, _, ct, _ = _fused(ctx, f)
    assert ct == (6, 4, 2) and {u for u in range(n) if tiny["pair_status"][u] != 0} == {big, po.OVER_COUNTS.index((65, 16))}
    ctx.close()


def test_arguments_and_the_need_formula(pkg):
    f = po.over_columns()
    ctx = _context(pkg, f)
    with pytest.raises(pkg.HlalaError, match=r"\(-1\)"):          # HLALA_E_ARG
        ctx.set_pair_overflow(-1)
    assert ctx.pair_overflow() == (0, 0)
    ctx.set_pair_overflow(1000003)
    assert ctx.pair_overflow() == (1000003, 1000003 // 64 // 16 * 16)
    ctx.set_pair_overflow(0)
    assert ctx.pair_overflow() == (0, 0)
    ctx.close()
    need = pkg.pair_overflow_need
    # 40 nc + 8 n1 n2 + 8 S W + 11 S (include/hlala_gpu.h), by hand
    assert need(65, 16, 384) == 40 * 81 + 8 * 1040 + 8 * 384 * 2 + 11 * 384 == 21928
    assert need(130, 3, 512) == 40 * 133 + 8 * 390 + 8 * 512 * 3 + 11 * 512 == 26360
    assert need(66, 99, 384, unpaired=True) == 40 * 66 + 8 * 66 + 8 * 384 * 2 + 11 * 384 == 13536
    for a in (1, 2, 64, 65, 128, 129, 1000):
        for c in (1, 3, 64, 65, 700):
            for S in (16, 384, 512, 1024):
                v = need(a, c, S)
                assert need(a + 1, c, S) >= v and need(a, c + 1, S) >= v and need(a, c, S + 1) >= v and v > 0
                assert need(a + 1, c, S, True) >= need(a, c, S, True) and need(a, c, S + 1, True) >= need(a, c, S, True) and need(a, c + 1, S, True) == need(a, c, S, True)


def test_hla_la_reports_the_overflow_class(pkg, tmp_path):
    """`HLA-LA --pairOverflow <MiB>`: unset, the program says nothing new; set, it reports the one pair of the sample that has 65 kept alignments on a mate; on a
    sample without such a pair hla/* is the same to the byte either way."""
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
    plain = synth.make_batch(w, 300, seed=77, haps=(2, 5))
    extra = pe.explode(synth.make_batch(w, 1, seed=91, p_secondary=0.0, indel_read_frac=0.0, p_no_clip=1.0))          # one record per read, [150 M]
    reads = pe.explode(plain) + [pe.with_variants(extra[0], 65), extra[1]]          # (the oracle keeps all 65 and scores the pair: 65 combinations)
    samples = {"plain": plain, "over": pe.assemble(reads, plain["insert_mean"], plain["insert_sd"])}
    contigs, intervals = pkg.load_contigs_dir(lib, gdir, extended_reference_genome=False)
    clen = np.diff(w["contigs"]["contig_off"])
    (tmp_path / "r1.fq").write_text("@r\nA\n+\nI\n"); (tmp_path / "r2.fq").write_text("@r\nA\n+\nI\n")
    line = "Pairs beyond the pairing capacities:"
    outs = {}
    for name, b in samples.items():
        d = tmp_path / name; d.mkdir()
        bam = d / "premade.bam"
        write_bam(bam, [(iv[0], int(clen[i])) for i, iv in enumerate(intervals)], batch_records(b, np.random.default_rng(1)), block=30000)
        _stub(d / "bwa", "#!/bin/bash\nif [ \"$1\" = index ]; then touch $2.sa $2.ann $2.bwt; fi\nexit 0\n")
        _stub(d / "samtools", f"#!/bin/bash\ncase \"$1\" in\n view) cat > /dev/null ;;\n sort) while [ $# -gt 0 ]; do if [ \"$1\" = -o ]; then cp {bam} \"$2\"; fi; shift; done ;;\n"
                              " index) touch \"$2.bai\" ;;\nesac\nexit 0\n")
        base = [EXE, "--action", "HLA", "--maxThreads", "2", "--sampleID", "S1", "--PRG_graph_dir", str(gdir), "--FASTQU", str(tmp_path / "r1.fq"), "--FASTQ1", str(tmp_path / "r1.fq"),
                "--FASTQ2", str(tmp_path / "r2.fq"), "--bwa_bin", str(d / "bwa"), "--samtools_bin", str(d / "samtools"), "--mapAgainstCompleteGenome", "0", "--longReads", "0",
                "--loci", "A", "--rngSeed", "5"]
        for mib in (None, "16"):
            o = outs[name, mib] = d / ("out" + (mib or "-unset"))
            r = subprocess.run(base + ["--outputDirectory", str(o)] + (["--pairOverflow", mib] if mib else []), capture_output=True, text=True, timeout=600, cwd=str(d))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert "Processed %d protoSeeds (read pairs)" % b["n_pairs"] in r.stdout
            want = None if mib is None else "%s %d scored in the overflow class, 0 refused\n" % (line, 1 if name == "over" else 0)
            assert (want in r.stdout and r.stdout.count(line) == 1) if want else line not in r.stdout, r.stdout[-2000:]
    files = sorted(os.listdir(outs["plain", None] / "hla"))
    assert files == sorted(os.listdir(outs["plain", "16"] / "hla")) and "R1_bestguess.txt" in files
    for fn in files:
        assert (outs["plain", "16"] / "hla" / fn).read_bytes() == (outs["plain", None] / "hla" / fn).read_bytes(), fn
    assert (outs["plain", "16"] / "reads_per_level.txt").read_bytes() == (outs["plain", None] / "reads_per_level.txt").read_bytes()


def test_overflow_class_matches_the_reference_fixture(pkg):
    """tests/golden/ref_pair_overflow.npz: 65 x 1, 1 x 65, 65 x 16 and 41 x 25 kept chains and what the reference's own processBAM makes of them
    (tests/golden/make_ref_golden_pair_overflow.py).  The kernels against the file directly, with the class on; with it off, all four pairs are refused."""
    import golden_pipeline as gp
    f = gp.load("ref_pair_overflow.npz"); m = f["meta"]; n = int(f["batch"]["n_pairs"])
    ctx = pkg.Context(f["graph"], f["contigs"], insert_mean=float(m["insert_mean"]), insert_sd=float(m["insert_sd"]), rng_seed=int(m["rng_seed"]),
                      long_read_mode=int(m["long_read_mode"]), max_columns=int(m["max_columns"]))
    gb = ctx.batch(f["batch"]); gb.align()
    assert np.all(gb.pairs()["pair_status"][:n] == -1) and gb.pair_overflow_counts() == (0, 0, 0)
    ctx.set_pair_overflow(SCRATCH)
    gb.pair()
    status = gb.chains(0)["status"][:int(f["batch"]["n_chains"])]
    assert np.all(status >= 0) and np.array_equal((status == 0).astype(np.uint8), f["keep"])
    got = gb.pairs()
    assert np.all(got["pair_status"][:n] == 0) and gb.stats().n_errors == 0 and gb.pair_overflow_counts() == (n, n, 0)
    assert f["exp"]["n_combinations"].tolist() == po.over_fixture()["n_comb"]
    gp.check_pairs(got, f, "ref_pair_overflow.npz")
    gb.close(); ctx.close()
