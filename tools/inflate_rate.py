#!/usr/bin/env python3
"""BGZF inflate and the BAM record pass: the host decoder against GPU inflate and against GPU inflate + parse on one BAM (its output is meant for
profiles/inflate_gpu.txt and profiles/bam_scan_gpu.txt).

A sample is drawn with the generators of bench.py's end-to-end leg (tools/synth.py: make_world_m, make_batch_m, BamWriter on tools/graphm/bamwriter.cpp;
reference names of tools/graphm_dir.py) and written coordinate-sorted at level 1, at least --min-inflated-gb of records.  hlala_bam_extract_seeds_opt and
hlala_bam_extract_seeds_gpu then decode it alternately: one warm-up each, --runs timed runs each, the same thread count.  Printed per run: the six phase times
of hlala_seed_batch_timing; for the GPU path also the blocks by who inflated them; and once, hlala_bgzf_inflate on all blocks of the file (hlala_inflate_stats:
upload, kernel, download, wall; blocks/s and inflated GB/s).  The third path, hlala_bam_extract_seeds_gpu with HLALA_SEEDS_GPU_PARSE, runs in the same alternation;
every run also prints the bytes that crossed PCIe each way (hlala_seed_batch_transfer_bytes) and, for the third path, records / rounds / rounds that fell back.  Last,
hlala_bam_scan alone on the first --scan-mb MiB of the inflated file at slices of 4, 16 and 64 KiB: device time per pass (median and range over --runs calls), re-hops,
and the share of the kept records that is tags (what compaction saves).  There is no threshold: the yardstick is the host decoder on the same file and box.
--verify-crc (its output is meant for profiles/bgzf_crc.txt): every decoder runs with and without HLALA_SEEDS_VERIFY_CRC, alternating in the same call -- six decodes per
round --, and hlala_bgzf_inflate_crc on all blocks reports the summed device time of k_bgzf_crc32 beside that of k_bgzf_inflate over the same chunks.  The cost of the flag
is read against the flag-off runs of the same call; on the host decoder it is the cost of the host's own CRC pass on the threads of that run.
The fourth path (its output is meant for profiles/bam_group_gpu.txt): HLALA_SEEDS_GPU_PARSE | HLALA_SEEDS_GPU_GROUP in the same alternation; its group phase and wall clock are
read against the third path's of the same call, and hlala_bam_group alone on the descriptors of the first --scan-mb MiB reports the device time per pass.
The fifth path (its output is meant for profiles/bam_nameorder_gpu.txt): HLALA_SEEDS_GPU_PARSE | HLALA_SEEDS_GPU_GROUP | HLALA_SEEDS_GPU_SORT in the same alternation; its sort
phase and wall clock are read against the fourth path's of the same call, and hlala_bam_name_order alone on the unit names of the first --scan-mb MiB reports the device
time per pass and the rounds it took.
The sixth path (its output is meant for profiles/bam_fill_gpu.txt): all of the fifth plus HLALA_SEEDS_GPU_FILL in the same alternation; its layout phase (layout + fill with
HLALA_BAM_EAGER=1, which the caller sets for both) and wall clock are read against the fifth path's of the same call; every run prints the units the device filled and the
host units, the device time of the window passes (hlala_seed_batch_fill_ms) and the bytes moved each way.  --paths a,b restricts the alternation to the named paths.
--wide-units N (its output is meant for profiles/bam_fill_wide_gpu.txt): one synthetic fill state of N pairs in which --wide-share of the units carry 17 to 200 alignments
on mate 0 (uniform; the scores drawn from four values, 70 % of them the same one), laid out by hlala_bam_fill_create -- the wide units handed in as host units, which is
what the decoder does with them without HLALA_SEEDS_GPU_FILL_WIDE -- and by hlala_bam_fill_create_wide, alternating; then every window through
hlala_batch_create_from_fill on both states, the first with the host units' ranges staged, the second with nothing to stage.
--wide-bam-pairs N (the same file): a BAM of N pairs written here, not by the generators above -- 2 x 100 bases on one reference, --wide-share of the pairs with 17 to 200
alignments on mate 0 (uniform; AS 40 with probability 0.7, else 60 / 77 / 90), every other mate with 1 to 3, one primary per mate, records shuffled -- decoded with
HLALA_SEEDS_GPU_FILL alone and with HLALA_SEEDS_GPU_FILL | HLALA_SEEDS_GPU_FILL_WIDE, alternating (the caller sets HLALA_BAM_EAGER=1 so that the fill lies inside the decode):
host units, the layout + fill phase and the wall clock of each.
--inflate-kernels hbm,lds (its output is meant for profiles/inflate_lds_gpu.txt): the named inflate kernels (hlala_inflater_set_kernel) alternate on ONE inflater -- in the
decoder paths `gpu` and `gpu+parse`, which run once per kernel beside the host decoder in every round, and in hlala_bgzf_inflate on all blocks in one call, which prints
upload / kernel / download / wall, blocks/s and GB/s per kernel and run (one warm-up each) and checks that the kernels leave the same bytes.  Nothing else runs.
--resident-decoder (the seventh path; its output is meant for profiles/bam_resident_decoder_gpu.txt): the generated BAM decoded with all of the sixth path's flags plus
HLALA_SEEDS_GPU_FILL_WIDE and HLALA_BAM_EAGER unset, then "window asked for -> batch created" summed over the sample's windows of --resident-window units on a context of the
sample's world: hlala_seed_batch_window + hlala_batch_create (the sixth path) against hlala_seed_batch_create_resident, alternating in one call, one warm-up and --runs timed
runs each, a fresh decode per run; PCIe bytes each way from hlala_seed_batch_transfer_bytes.  Nothing else runs."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bgzf_blocks(path):
    """[(payload offset, payload bytes, isize)] of the non-empty blocks, and the file's bytes (memory-mapped)"""
    raw = np.memmap(path, np.uint8, "r"); o = 0; out = []
    n = raw.size
    while o < n:
        xlen = int(raw[o + 10]) | (int(raw[o + 11]) << 8)
        bsize = (int(raw[o + 16]) | (int(raw[o + 17]) << 8)) + 1          # (the BC subfield is the first one in every block this repository writes)
        isize = int.from_bytes(raw[o + bsize - 4:o + bsize].tobytes(), "little")
        if isize:
            out.append((o + 12 + xlen, bsize - 12 - xlen - 8, isize))
        o += bsize
    return raw, out


def scan_alone(P, inf, inflated, intervals, args):
    """hlala_bam_scan on the first --scan-mb MiB of the inflated file (host memory: the upload is part of the call and timed on its own)"""
    n_ref = int(inflated[8 + int(inflated[4:8].view("<i4")[0]):][:4].view("<i4")[0]); o = 12 + int(inflated[4:8].view("<i4")[0])
    by_name = {}
    for i, iv in enumerate(intervals):
        by_name.setdefault(iv[0], []).append(i)
    ref_iv = []
    for _ in range(n_ref):
        ln = int(inflated[o:o + 4].view("<i4")[0]); nm = inflated[o + 4:o + 4 + ln - 1].tobytes().decode(); o += 8 + ln
        ref_iv.append(by_name.get(nm, []))
    n = min(inflated.size, args.scan_mb << 20)
    data = inflated[:n]
    passes = ("h2d", "guess", "link", "starts", "parse", "scan", "emit", "d2h", "wall")
    for S in (4096, 16384, 65536):
        a, keep = P.bam_scan_in(n_ref, ref_iv, [iv[1:] for iv in intervals], slice_bytes=S)
        rc, _, _, st = inf.bam_scan(data, a, first=o, cap_recs=0, cap_compact=0)                     # how much comes back
        if st.status != 0:
            print("hlala_bam_scan, slices of %d: status %s at record %d" % (S, P.BAMSCAN_STATUS[st.status], st.status_record)); continue
        nr, nc = st.n_recs, st.compact_bytes
        t = {k: [] for k in passes}
        for i in range(args.runs + 1):
            rc, recs, comp, st = inf.bam_scan(data, a, first=o, cap_recs=nr, cap_compact=nc)
            assert rc == 0 and st.status == 0
            if i:
                for k in passes:
                    t[k].append(getattr(st, "ms_" + k))
        print("hlala_bam_scan alone, %.3f GB inflated, slices of %d KiB: %d records (%d kept, %d descriptors), %d slices, %d re-hops (cap %d); %.3f GB of compact bytes + %.3f GB of descriptors come back" % (
            n / 1e9, S >> 10, st.n_records, st.n_kept, st.n_recs, st.n_slices, st.n_rehops, P.BAMSCAN_DEFAULT_MAX_REHOPS, nc / 1e9, nr * P.BAM_REC_DTYPE.itemsize / 1e9))
        print("    ms per pass, median (min .. max) of %d calls: %s" % (args.runs, "  ".join("%s %.2f (%.2f .. %.2f)" % (k, float(np.median(t[k])), min(t[k]), max(t[k])) for k in passes)))
        dev = sum(float(np.median(t[k])) for k in ("guess", "link", "starts", "parse", "scan", "emit"))
        print("    the six passes: %.2f ms = %.2f GB/s of inflated bytes; consumed %.3f GB" % (dev, n / 1e9 / (dev / 1e3), st.consumed / 1e9))
    kept = (recs, comp) if st.status == 0 else None
    if st.status == 0 and st.n_kept:
        print("share of the scanned bytes that comes back as compact bytes: %.3f (all records are examined; %.3f of them are kept; what is dropped of a kept record is its length field and its tags)" % (
            nc / max(1, st.consumed - o), st.n_kept / max(1, st.n_records)))
        print("    -> with records of one kind, length field + tags are about %.3f of a kept record" % (1.0 - (nc / max(1, st.consumed - o)) / (st.n_kept / max(1, st.n_records))))
    return kept


def group_alone(P, inf, recs, comp, args):
    """hlala_bam_group on the descriptors and compact bytes hlala_bam_scan has just returned (host memory: the upload is part of the call and timed on its own)"""
    passes = ("h2d", "append", "sort", "mark", "fold", "emit", "d2h", "wall")
    t = {k: [] for k in passes}
    for i in range(args.runs + 1):
        rc, perm, flag, st = inf.bam_group(recs, comp)
        assert rc == 0, inf.last_error()
        if i:
            for k in passes:
                t[k].append(getattr(st, "ms_" + k))
    print("hlala_bam_group alone: %d descriptors (%.3f GB of compact bytes uploaded with them), %d runs, %d collided, %d complete and %d incomplete units" % (
        st.n_recs, comp.size / 1e9, st.n_runs, st.n_collided_runs, st.n_units_complete, st.n_units_incomplete))
    print("    ms per pass, median (min .. max) of %d calls: %s" % (args.runs, "  ".join("%s %.3f (%.3f .. %.3f)" % (k, float(np.median(t[k])), min(t[k]), max(t[k])) for k in passes)))
    dev = sum(float(np.median(t[k])) for k in ("append", "sort", "mark", "fold", "emit"))
    print("    append + sort + mark + fold + emit: %.3f ms = %.1f M descriptors/s" % (dev, st.n_recs / 1e6 / max(1e-9, dev / 1e3)))
    return perm, flag


def name_order_alone(P, inf, recs, comp, perm, flag, args):
    """hlala_bam_name_order on the names of the units hlala_bam_group has just found: the first records of clean, complete runs, in run order (host memory: the upload is
    part of the call and timed on its own; the decoder uploads nothing)"""
    first = perm[(flag & 5) == 5]
    off = recs["rec_off"][first].astype(np.uint64) + 32; ln = recs["nameLen"][first].astype(np.uint32)
    passes = ("h2d", "key", "sort", "mark", "scatter", "d2h", "wall")
    t = {k: [] for k in passes}
    for i in range(args.runs + 1):
        rc, order, st = inf.bam_name_order(off, ln, comp)
        assert rc == 0, inf.last_error()
        if i:
            for k in passes:
                t[k].append(getattr(st, "ms_" + k))
    b = comp.tobytes()
    names = [b[int(o):int(o) + int(k)] for o, k in zip(off, ln)]
    assert all(names[int(order[k - 1])] < names[int(order[k])] for k in range(1, len(order))), "the device's order does not ascend"
    print("hlala_bam_name_order alone: %d unit names of %d .. %d bytes (%.3f GB of compact bytes uploaded with them), %d rounds, %d equal names; the order ascends (checked here)" % (
        st.n, int(ln.min()), int(ln.max()), comp.size / 1e9, st.n_rounds, st.n_equal_names))
    print("    ms per pass summed over the rounds, median (min .. max) of %d calls: %s" % (args.runs, "  ".join("%s %.3f (%.3f .. %.3f)" % (k, float(np.median(t[k])), min(t[k]), max(t[k])) for k in passes)))
    dev = sum(float(np.median(t[k])) for k in ("key", "sort", "mark", "scatter"))
    print("    key + sort + mark + scatter: %.3f ms = %.1f M names/s" % (dev, st.n / 1e6 / max(1e-9, dev / 1e3)))


def resident_alone(P, lib, args):
    """--resident-units N (its output is meant for profiles/bam_resident_gpu.txt): hlala_batch_create_from_fill against hlala_bam_fill_window + hlala_batch_create on one
    synthetic fill state of N pairs (2 x 150 bases, one alignment of one CIGAR operation per mate, every 1000th unit a host unit), cut into windows of --resident-window
    units.  Per run and path the wall clock from "window asked for" to "batch created", summed over the windows; the paths alternate in one call, one warm-up each.  The
    sample's arrays are page-locked in place (hlala_host_register), as a caller pins a seed batch's."""
    import ctypes as C
    from tools import synth
    N, Wn = args.resident_units, args.resident_window
    w = synth.make_world(seed=11, G=4000, k=1)
    ctx = P.Context(w["graph"], w["contigs"], device=args.device)
    inf = P.Inflater(lib, device=args.device, chunk_bytes=0)
    rng = np.random.default_rng(7)
    L, NAME = 150, 9
    body = 32 + NAME + 1 + 4 + (L + 1) // 2 + L; stride = (body + 7) & ~7
    host = np.arange(N) % 1000 == 499
    dev_units = np.nonzero(~host)[0]
    nrec = 2 * len(dev_units)
    data = np.zeros((nrec, stride), np.uint8)
    data[:, 32:32 + NAME] = np.frombuffer(b"0123456789", np.uint8)[(np.repeat(dev_units, 2)[:, None] // 10 ** np.arange(NAME - 1, -1, -1)) % 10] + 0
    data[:, 32 + NAME + 1:32 + NAME + 5] = np.frombuffer(np.uint32(L << 4).tobytes(), np.uint8)
    data[:, 32 + NAME + 5:body] = rng.integers(0, 64, (nrec, body - 32 - NAME - 5), dtype=np.uint8)
    recs = np.zeros(nrec, P.BAM_REC_DTYPE)
    recs["order"] = np.arange(nrec); recs["rec_off"] = np.arange(nrec, dtype=np.uint64) * stride; recs["contig"] = rng.integers(0, w["contigs"]["n_contigs"], nrec)
    recs["pos"] = rng.integers(0, 3000, nrec); recs["as"] = rng.integers(50, 150, nrec); recs["l_seq"] = L; recs["n_cigar"] = 1; recs["nameLen"] = NAME
    recs["which"] = np.arange(nrec) % 2; recs["flags"] = 2 | rng.integers(0, 2, nrec).astype(np.uint8); recs["l_read_name"] = NAME + 1
    first = np.full(N, P.BAM_FILL_HOST, np.uint32); first[dev_units] = np.arange(len(dev_units), dtype=np.uint32) * 2
    count = np.full(N, 2, np.uint32)
    hs = np.tile(np.array([L, 1, 1, L, 1, 1, NAME + 1], np.int64), int(host.sum()))
    fin, keep = P.bam_fill_in(recs, data.reshape(-1), first, count, hs, False, True)
    rc, h, off, st = inf.bam_fill_create(fin, N, False, True)
    assert rc == 0, inf.last_error()
    nR, nC, nB, nG = 2 * N, int(off["chain_off"][-1]), int(off["read_off"][-1]), int(off["cigar_count"][-1])
    print("hlala_batch_create_from_fill alone: %d pairs (%d host units), %d chains, %.3f GB of bases and qualities unpacked; layout %.1f ms wall; windows of %d units" % (
        N, int(host.sum()), nC, 2 * nB / 1e9, st.ms_wall, Wn))
    # the sample's host arrays (packed); the host units' ranges hold what the host's own fill would leave: a primary and an ascending CIGAR end
    S = dict(read_primary=np.zeros(nR, np.int32), read_bases_packed=np.zeros((nB + nR + 1) // 2 + 2, np.uint8), read_quals=np.zeros(nB, np.uint8), chain_contig=np.zeros(nC, np.int32),
             chain_pos=np.zeros(nC, np.int32), chain_offset=np.zeros(nC, np.int32), chain_as=np.zeros(nC, np.int32), chain_reverse=np.zeros(nC, np.uint8), cigar_off=np.zeros(nC + 1, np.int64),
             cigar=np.zeros(nG, np.uint32), name_chars=np.zeros(int(off["name_off"][-1]), np.uint8))
    lib.hlala_host_register.argtypes = [C.c_void_p, C.c_size_t]
    pinned = sum(lib.hlala_host_register(a.ctypes.data, a.nbytes) == 0 for a in S.values() if a.nbytes)
    print("    the sample's host arrays page-locked in place: %d of %d" % (pinned, sum(1 for a in S.values() if a.nbytes)))
    hr = np.nonzero(np.repeat(host, 2))[0]

    def fill_host_units():
        S["read_primary"][hr] = off["chain_off"][hr]; S["cigar_off"][off["chain_off"][hr] + 1] = off["cigar_count"][hr] + 1
    lib.hlala_bam_fill_window.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(P.BamFillOut), C.POINTER(P.BamFillStats)]
    lib.hlala_batch_create_from_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(P.BatchFillSrc), C.POINTER(C.c_void_p), C.POINTER(P.BatchFillStats)]
    at = lambda k, i: S[k].ctypes.data + i * S[k].itemsize      # noqa: E731

    def slices(u0):
        r0 = 2 * u0; b0, c0, g0 = int(off["read_off"][r0]), int(off["chain_off"][r0]), int(off["cigar_count"][r0])
        return P.BamFillOut(read_primary=at("read_primary", r0), read_bases=None, read_bases_packed=at("read_bases_packed", (b0 + r0 + 1) >> 1), read_quals=at("read_quals", b0),
                            chain_contig=at("chain_contig", c0), chain_pos=at("chain_pos", c0), chain_offset=at("chain_offset", c0), chain_as=at("chain_as", c0), chain_reverse=at("chain_reverse", c0),
                            cigar_off_end=at("cigar_off", c0 + 1), cigar=at("cigar", g0), name_chars=at("name_chars", int(off["name_off"][u0])))
    wins = [(u, min(Wn, N - u)) for u in range(0, N, Wn)]
    res = {"sixth": [], "resident": []}; kern = []; moved = {}
    for run in range(args.runs + 1):
        for path in ("sixth", "resident"):
            total = 0.0; up = down = 0; km = np.zeros(7)
            for u0, n in wins:
                out = slices(u0); b = C.c_void_p(); r0, r1 = 2 * u0, 2 * (u0 + n)
                t = time.perf_counter()
                if path == "sixth":
                    ws = P.BamFillStats()
                    rc = lib.hlala_bam_fill_window(h.h, u0, n, C.byref(out), C.byref(ws)); assert rc == 0, h.last_error()
                    fill_host_units()
                    d = P.BatchIn(n_pairs=n, n_chains=int(off["chain_off"][r1] - off["chain_off"][r0]), first_read=r0)
                    for k, ty in P.BatchIn._fields_:
                        if k in S and k != "name_chars":
                            setattr(d, k, C.cast(S[k].ctypes.data, ty))
                    d.read_off = C.cast(off["read_off"].ctypes.data + 8 * r0, P.c_i64p); d.chain_off = C.cast(off["chain_off"].ctypes.data + 8 * r0, P.c_i64p)
                    d.read_primary = C.cast(at("read_primary", r0), P.c_i32p)
                    rc = lib.hlala_batch_create(ctx.h, C.byref(d), C.byref(b)); assert rc == 0, ctx.last_error()
                    down += ws.bytes_d2h; up += int(out_bytes(off, r0, r1))
                else:
                    fill_host_units()
                    src = P.BatchFillSrc(off["read_off"].ctypes.data, off["chain_off"].ctypes.data, off["cigar_count"].ctypes.data, C.pointer(out)); rs = P.BatchFillStats()
                    rc = lib.hlala_batch_create_from_fill(ctx.h, h.h, u0, n, C.byref(src), C.byref(b), C.byref(rs)); assert rc == 0, ctx.last_error()
                    up += rs.bytes_h2d; down += rs.bytes_d2h
                    km += [rs.ms_chain, rs.ms_cigar, rs.ms_bases, rs.ms_patch, rs.ms_reads, rs.ms_chains, rs.ms_chain_read]
                total += time.perf_counter() - t
                lib.hlala_batch_destroy(b)
            if run:
                res[path].append(total * 1e3); moved[path] = (up, down)
                if path == "resident":
                    kern.append(km)
    for path in ("sixth", "resident"):
        v = res[path]
        print("window asked for -> batch created, %s path, all %d windows: median %.1f ms, range %.1f .. %.1f of %d runs; PCIe up %.3f GB, down %.3f GB per run" % (
            path, len(wins), float(np.median(v)), min(v), max(v), len(v), moved[path][0] / 1e9, moved[path][1] / 1e9))
    k = np.median(np.array(kern), axis=0)
    print("device ms summed over the windows, median of %d runs: k_fil_chain %.3f  k_fil_cigar %.3f  k_fil_bases %.3f  k_res_patch %.3f  k_res_reads %.3f  k_res_chains %.3f  k_res_chain_read %.3f" % (
        (len(kern),) + tuple(k)))
    lib.hlala_host_unregister.argtypes = [C.c_void_p]
    for a in S.values():
        if a.nbytes:
            lib.hlala_host_unregister(a.ctypes.data)
    h.close(); inf.close()


def wide_state(P, N, share, n_contigs, L=100, NAME=9):
    """the descriptors of --wide-units: (recs, data, unit_first with every unit filled, unit_first with the wide units as host units, unit_count, their host sizes, wide)"""
    rng = np.random.default_rng(17)
    wide = rng.random(N) < share
    c = np.stack([np.where(wide, rng.integers(17, 201, N), rng.integers(1, 4, N)), rng.integers(1, 4, N)], axis=1).astype(np.int64)        # alignments per unit and mate
    per = c.reshape(-1); n = int(per.sum())
    start = np.concatenate([[0], np.cumsum(per)])
    mate_of = np.repeat(np.arange(2 * N), per); j = np.arange(n) - start[mate_of]                  # the read and the place in it of every record
    prim = j == rng.integers(0, 1 << 30, 2 * N)[mate_of] % per[mate_of]
    body = np.where(prim, 32 + NAME + 1 + 4 + (L + 1) // 2 + L, 32 + NAME + 1 + 4); body = (body + 7) & ~7
    rec_off = np.concatenate([[0], np.cumsum(body)]).astype(np.uint64)
    data = rng.integers(0, 64, int(rec_off[-1]), dtype=np.uint8)
    recs = np.zeros(n, P.BAM_REC_DTYPE)
    recs["order"] = np.arange(n); recs["rec_off"] = rec_off[:-1]; recs["contig"] = rng.integers(0, n_contigs, n); recs["pos"] = rng.integers(0, 3000, n)
    recs["as"] = rng.choice(np.array([40, 40, 40, 40, 40, 40, 40, 60, 77, 90]), n); recs["l_seq"] = np.where(prim, L, 0); recs["n_cigar"] = 1; recs["nameLen"] = NAME
    recs["which"] = mate_of % 2; recs["flags"] = np.where(prim, 2, 0).astype(np.uint8) | rng.integers(0, 2, n).astype(np.uint8); recs["l_read_name"] = NAME + 1
    first_all = start[0:2 * N:2].astype(np.uint32); count = (c[:, 0] + c[:, 1]).astype(np.uint32)
    first_narrow = np.where(wide, P.BAM_FILL_HOST, first_all).astype(np.uint32)
    hs = np.stack([np.full(N, L), c[:, 0], c[:, 0], np.full(N, L), c[:, 1], c[:, 1], np.full(N, NAME + 1)], axis=1)[wide].astype(np.int64).reshape(-1)
    return recs, data, first_all, first_narrow, count, hs, wide


def wide_alone(P, lib, args):
    """--wide-units N: see the module docstring.  The narrow state's host units are 'filled' from the wide state's download of the same window -- the bytes the host's own
    sort and fill would leave; what that host fill costs is NOT in these figures."""
    from tools import synth
    N, share, Wn = args.wide_units, args.wide_share, args.resident_window
    w = synth.make_world(seed=11, G=4000, k=1)
    ctx = P.Context(w["graph"], w["contigs"], device=args.device)
    inf = P.Inflater(lib, device=args.device, chunk_bytes=0)
    recs, data, first_all, first_narrow, count, hs, wide = wide_state(P, N, share, int(w["contigs"]["n_contigs"]))
    n = len(recs)
    print("wide fill alone: %d pairs, %d of them wide (17 .. 200 alignments on mate 0, uniform; scores 40 with probability 0.7, else 60 / 77 / 90), %d descriptors, %.3f GB of record bytes; windows of %d units" % (
        N, int(wide.sum()), n, data.size / 1e9, Wn))
    fin_n, keep_n = P.bam_fill_in(recs, data, first_narrow, count, hs, False, True)
    fin_w, keep_w = P.bam_fill_in(recs, data, first_all, count, np.zeros(0, np.int64), False, True)
    lay = {"narrow": [], "wide": []}; dev = []
    hn = hw = None
    for run in range(args.runs + 1):
        for path in ("narrow", "wide"):
            rc, h, off, st = inf.bam_fill_create(fin_n, N, False, True) if path == "narrow" else inf.bam_fill_create_wide(fin_w, N, False, True)
            assert rc == 0, inf.last_error()
            if run:
                lay[path].append((st.ms_wall, st.ms_rank + st.ms_host + st.ms_scan + st.ms_src))
                if path == "wide":
                    dev.append(h.wide_stats())
            if run == args.runs:
                if path == "narrow":
                    hn, off_n = h, off
                else:
                    hw, off_w = h, off
            else:
                h.close()
    assert all(np.array_equal(off_n[k], off_w[k]) for k in off_n), "the two layouts differ"
    for path in ("narrow", "wide"):
        v = [x[0] for x in lay[path]]; k = [x[1] for x in lay[path]]
        print("layout (upload, passes, download of the offsets), %s state, host units %d: wall median %.2f ms, range %.2f .. %.2f of %d runs; of it layout kernels and scans on the device %.3f ms" % (
            path, int(wide.sum()) if path == "narrow" else 0, float(np.median(v)), min(v), max(v), len(v), float(np.median(k))))
    u = [x[3] for x in dev]
    print("k_fil_wide_rank + k_fil_wide_src: median %.0f us, range %.0f .. %.0f of %d runs (%d wide units, %d wide reads, longest mate %d)" % ((float(np.median(u)), min(u), max(u), len(u)) + dev[0][:3]))
    wins = [(a, min(Wn, N - a)) for a in range(0, N, Wn)]
    host_slices = {}
    for u0, k in wins:                                      # what the host would have filled: taken from the wide state, outside the timed part
        rc, arrs, _ = hw.window(u0, k); assert rc == 0, hw.last_error()
        host_slices[u0] = arrs
    res = {"narrow": [], "wide": []}; moved = {}
    for run in range(args.runs + 1):
        for path, h in (("narrow", hn), ("wide", hw)):
            total = 0.0; pieces = up = 0
            for u0, k in wins:
                t = time.perf_counter()
                rc, b, rs = ctx.batch_from_fill(h, u0, k, host_slices[u0] if path == "narrow" and wide[u0:u0 + k].any() else None)
                assert rc == 0, ctx.last_error()
                total += time.perf_counter() - t
                pieces += rs.n_pieces; up += rs.bytes_h2d
                b.close()
            if run:
                res[path].append(total * 1e3); moved[path] = (pieces, up)
    for path in ("narrow", "wide"):
        v = res[path]
        print("hlala_batch_create_from_fill, %s state, all %d windows: median %.1f ms, range %.1f .. %.1f of %d runs; %d pieces staged, %.3f GB up per run" % (
            path, len(wins), float(np.median(v)), min(v), max(v), len(v), moved[path][0], moved[path][1] / 1e9))
    hn.close(); hw.close(); inf.close()


def wide_bam(P, lib, args):
    """--wide-bam-pairs N: see the module docstring"""
    import struct
    import zlib
    N, share = args.wide_bam_pairs, args.wide_share
    rng = np.random.default_rng(23)
    L = 100
    wide = rng.random(N) < share
    c0 = np.where(wide, rng.integers(17, 201, N), rng.integers(1, 4, N)); c1 = rng.integers(1, 4, N)
    t0 = time.time()
    seq = bytes(rng.integers(0, 256, (L + 1) // 2, dtype=np.uint8)) + bytes(rng.integers(2, 41, L, dtype=np.uint8).tolist())      # (one sequence for every primary: the fill copies it, whatever it holds)
    cig = struct.pack("<I", (L << 4) | 0)
    out = []
    for u in range(N):
        name = b"p%07d\0" % u
        for mate, k in ((0, int(c0[u])), (1, int(c1[u]))):
            prim = int(rng.integers(0, k)); AS = rng.choice((40, 40, 40, 40, 40, 40, 40, 60, 77, 90), k); pos = rng.integers(1000, 40000, k); rev = rng.integers(0, 2, k)
            for j in range(k):
                flag = 1 | (64 if mate == 0 else 128) | (16 if rev[j] else 0) | (0 if j == prim else 256)
                body = struct.pack("<iiBBHHHiiii", 0, int(pos[j]), len(name), 60, 0, 1, flag, L, -1, -1, 0) + name + cig + seq + b"ASC" + bytes([int(AS[j])])
                out.append(struct.pack("<i", len(body)) + body)
    n_rec = len(out)
    order = rng.permutation(n_rec)
    raw = b"BAM\x01" + struct.pack("<ii", 0, 1) + struct.pack("<i", 5) + b"chr6\0" + struct.pack("<i", 50000) + b"".join(out[i] for i in order)
    tmp = tempfile.mkdtemp(prefix="hlala_wide_bam_"); bam = os.path.join(tmp, "wide.bam")
    with open(bam, "wb") as f:
        for i in list(range(0, len(raw), 60000)) + [len(raw)]:
            d = raw[i:i + 60000]
            co = zlib.compressobj(1, zlib.DEFLATED, -15); comp = co.compress(d) + co.flush()
            f.write(struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, 6) + b"BC" + struct.pack("<HH", 2, len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(d) & 0xFFFFFFFF, len(d)))
    print("wide BAM: %d pairs, %d of them wide (17 .. 200 alignments on mate 0, uniform; AS 40 with probability 0.7, else 60 / 77 / 90), %d records, %.3f GB inflated; written in %.1f s; HLALA_BAM_EAGER=%s" % (
        N, int(wide.sum()), n_rec, len(raw) / 1e9, time.time() - t0, os.environ.get("HLALA_BAM_EAGER", "unset")))
    intervals = [("chr6", 0, 49999, 0)]
    inf = P.Inflater(lib, device=args.device, chunk_bytes=args.chunk_mb << 20)
    base = P.SEEDS_PACKED | P.SEEDS_GPU_PARSE | P.SEEDS_GPU_GROUP | P.SEEDS_GPU_SORT | P.SEEDS_GPU_FILL
    res = {"fill": [], "fill+wide": []}
    for run in range(args.runs + 1):
        for path, fl in (("fill", base), ("fill+wide", base | P.SEEDS_GPU_FILL_WIDE)):
            t = time.time(); S = inf.bam_open_seeds(bam, intervals, threads=args.threads, flags=fl); wall = time.time() - t
            tm = S.timing(); fc = S.fill_counts(); wc = S.fill_wide_counts(); fm = S.fill_ms(); units = S.n_units; S.close()
            if run:
                res[path].append((tm["layout"], wall, fc, wc, sum(fm[:4])))
                print("%-10s wall %.3f s  layout + fill %.4f s  units %d: filled on the GPU %d, host units %d, whole sample by the host %d; wide units on the GPU %d, beyond the cap %d, longest mate %d; window kernels %.3f ms" % (
                    path, wall, tm["layout"], units, fc[0], fc[1], fc[2], wc[0], wc[1], wc[2], sum(fm[:4])))
    for path in ("fill", "fill+wide"):
        for j, what in ((0, "layout + fill phase"), (1, "decode, wall")):
            v = [x[j] for x in res[path]]
            print("%s, %s: median %.4f s, range %.4f .. %.4f of %d runs; host units %d" % (what, path, float(np.median(v)), min(v), max(v), len(v), res[path][0][2][1]))
    inf.close()
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


def resident_decoder(P, lib, inf, w, bam, intervals, args):
    """--resident-decoder (the seventh path; its output is meant for profiles/bam_resident_decoder_gpu.txt): the BAM is decoded with every GPU stage, HLALA_BAM_EAGER unset,
    and its windows of --resident-window units become batches of a context of the sample's world -- by hlala_seed_batch_window + hlala_batch_create (the sixth path, the
    sample page-locked window by window as the host program does) and by hlala_seed_batch_create_resident (the seventh), alternating in one call, one warm-up and --runs
    timed runs each, a fresh decode per run.  Printed per run: the wall clock from "window asked for" to "batch created" summed over the windows, and the bytes that
    crossed PCIe each way during the walk (hlala_seed_batch_transfer_bytes; for the sixth path plus what hlala_batch_create uploads, computed from the window)."""
    import ctypes as C
    assert not os.environ.get("HLALA_BAM_EAGER"), "the seventh path is measured with HLALA_BAM_EAGER unset"
    t0 = time.time()
    ctx = P.Context(w["graph"], w["contigs"], device=args.device)
    print("context of the sample's world: %.1f s" % (time.time() - t0))
    flags = P.SEEDS_PACKED | P.SEEDS_GPU_PARSE | P.SEEDS_GPU_GROUP | P.SEEDS_GPU_SORT | P.SEEDS_GPU_FILL | P.SEEDS_GPU_FILL_WIDE
    lib.hlala_seed_batch_pin.argtypes = [C.c_void_p, C.c_int]
    lib.hlala_batch_destroy.argtypes = [C.c_void_p]
    Wn = args.resident_window
    res = {"sixth": [], "resident": []}; moved = {}; info = rcnt = None
    for run in range(args.runs + 1):
        for path in ("sixth", "resident"):
            S = inf.bam_open_seeds(bam, intervals, threads=args.threads, flags=flags)
            N = S.n_units; wins = [(u, min(Wn, N - u)) for u in range(0, N, Wn)]
            if path == "sixth":
                lib.hlala_seed_batch_pin(S.h, 2)
            up0, down0 = S.transfer_bytes(); total = 0.0; up = 0
            for u0, n in wins:
                b = C.c_void_p()
                t = time.perf_counter()
                if path == "sixth":
                    d = S.window(u0, n)
                    rc = lib.hlala_batch_create(ctx.h, C.byref(d), C.byref(b)); assert rc == 0, ctx.last_error()
                    total += time.perf_counter() - t
                    nr = 2 * n; nb = int(d.read_off[nr] - d.read_off[0]); c0, c1 = int(d.chain_off[0]), int(d.chain_off[nr]); ng = int(d.cigar_off[c1] - d.cigar_off[c0])
                    up += (nb + nr + 1) // 2 + nb + 17 * (c1 - c0) + 4 * ng + 4 * (3 * nr + 2 * (c1 - c0) + 3)
                else:
                    st = P.BatchFillStats()
                    rc = lib.hlala_seed_batch_create_resident(S.h, ctx.h, u0, n, C.byref(b), C.byref(st)); assert rc == 0, ctx.last_error()
                    total += time.perf_counter() - t
                lib.hlala_batch_destroy(b)
            up1, down1 = S.transfer_bytes()
            if run:
                res[path].append(total * 1e3); moved[path] = (up + up1 - up0, down1 - down0)
                print("%-9s run %d: window asked for -> batch created, all %d windows: %.1f ms; PCIe up %.3f GB, down %.3f GB" % (path, run, len(wins), total * 1e3, (up + up1 - up0) / 1e9, (down1 - down0) / 1e9))
            info = (N, S.fill_counts(), S.fill_wide_counts())
            if path == "resident":
                rcnt = S.resident_counts()
            S.close()
    print("the sample: %d units; filled on the GPU %d, host units %d; wide units %d; resident windows %d with %d units, %d pieces of host units staged, %d fell back; windows of %d units" % (
        info[0], info[1][0], info[1][1], info[2][0], rcnt[0], rcnt[1], rcnt[2], rcnt[3], Wn))
    for path in ("sixth", "resident"):
        v = res[path]
        print("window asked for -> batch created, %s path: median %.1f ms, range %.1f .. %.1f of %d runs; PCIe up %.3f GB, down %.3f GB per run" % (
            path, float(np.median(v)), min(v), max(v), len(v), moved[path][0] / 1e9, moved[path][1] / 1e9))
    print("every resident run below every sixth-path run: %s (slowest resident %.1f ms, fastest sixth %.1f ms)" % (max(res["resident"]) < min(res["sixth"]), max(res["resident"]), min(res["sixth"])))
    ctx.close()


def out_bytes(off, r0, r1):
    """the bytes hlala_batch_create uploads for reads [r0, r1) of a packed sample: packed bases, qualities, 17 bytes per chain + its CIGAR, the 32-bit offset arrays"""
    nb = int(off["read_off"][r1] - off["read_off"][r0]); nc = int(off["chain_off"][r1] - off["chain_off"][r0]); ng = int(off["cigar_count"][r1] - off["cigar_count"][r0])
    return (nb + r1 - r0 + 1) // 2 + nb + 17 * nc + 4 * ng + 4 * (3 * (r1 - r0) + 2 * nc + 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resident-units", type=int, default=0, help="only hlala_batch_create_from_fill against hlala_bam_fill_window + hlala_batch_create, on a synthetic fill state of this many pairs")
    ap.add_argument("--resident-window", type=int, default=262144, help="units per window of --resident-units and --resident-decoder")
    ap.add_argument("--resident-decoder", action="store_true", help="only the seventh path: the generated BAM decoded with every GPU stage, its windows through hlala_seed_batch_window + hlala_batch_create against hlala_seed_batch_create_resident")
    ap.add_argument("--wide-units", type=int, default=0, help="only hlala_bam_fill_create_wide against hlala_bam_fill_create with the wide units as host units, on a synthetic fill state of this many pairs")
    ap.add_argument("--wide-bam-pairs", type=int, default=0, help="only the decoder with HLALA_SEEDS_GPU_FILL against HLALA_SEEDS_GPU_FILL | HLALA_SEEDS_GPU_FILL_WIDE on a BAM of this many pairs written here")
    ap.add_argument("--wide-share", type=float, default=0.05, help="share of the units of --wide-units / --wide-bam-pairs that carry 17 to 200 alignments on mate 0")
    ap.add_argument("--pairs", type=int, default=1 << 20, help="pairs per generated chunk of the sample")
    ap.add_argument("--levels", type=int, default=5_000_000, help="levels of the Graph M world (bench.py --levels)")
    ap.add_argument("--min-inflated-gb", type=float, default=1.0, help="chunks are added until the BAM holds this much inflated")
    ap.add_argument("--threads", type=int, default=0, help="decoder threads of both paths (0 = the decoder's default)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk-mb", type=int, default=0, help="compressed MiB staged per launch (0 = the library's default)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--scan-mb", type=int, default=256, help="inflated MiB handed to hlala_bam_scan alone (below 4096)")
    ap.add_argument("--verify-crc", action="store_true", help="every decoder with and without HLALA_SEEDS_VERIFY_CRC in the same alternation; k_bgzf_crc32's device time beside the inflate kernel's")
    ap.add_argument("--inflate-kernels", default="", help="comma-separated inflate kernels (hbm, lds) that alternate on one inflater: decoder paths gpu and gpu+parse, and all blocks in one call")
    ap.add_argument("--bam", default="", help="use this BAM (reference names PRG_<n>) instead of generating one; needs --levels of the world it was made from")
    ap.add_argument("--paths", default="", help="comma-separated paths that alternate (default: all), e.g. gpu+parse+group+sort,gpu+parse+group+sort+fill")
    ap.add_argument("--no-gpu", action="store_true", help="host engine only (a box without a GPU: checks the generator and the host figures)")
    args = ap.parse_args()
    import importlib.util
    spec = importlib.util.spec_from_file_location("hla_la_amd", os.path.join(ROOT, "hla-la_amd", "__init__.py"), submodule_search_locations=[os.path.join(ROOT, "hla-la_amd")])
    P = importlib.util.module_from_spec(spec); sys.modules["hla_la_amd"] = P; spec.loader.exec_module(P)
    from tools import graphm_dir, synth
    lib = P.load_library()
    lib.hlala_bam_inflate_engine.restype = __import__("ctypes").c_char_p
    if args.resident_units > 0:
        resident_alone(P, lib, args)
        return
    if args.wide_units > 0:
        wide_alone(P, lib, args)
        return
    if args.wide_bam_pairs > 0:
        wide_bam(P, lib, args)
        return
    t0 = time.time()
    w = synth.make_world_m(seed=2, n_levels=args.levels)
    clen = np.diff(w["contigs"]["contig_off"]); names = graphm_dir.ref_names(w)
    intervals = [(nm, 0, int(clen[i]) - 1, i) for i, nm in enumerate(names)]
    tmp = None
    bam = args.bam
    if not bam:
        tmp = tempfile.mkdtemp(prefix="hlala_inflate_rate_"); bam = os.path.join(tmp, "sample.bam")
        bw = synth.BamWriter(bam, [(nm, int(clen[i])) for i, nm in enumerate(names)], threads=0, level=1)
        k = 0; inflated = 0
        while inflated < args.min_inflated_gb * 1e9:
            bk = synth.make_batch_m(w, args.pairs, seed=3000 + k, frac_gene=0.04); nm, _ = synth.scrambled_names(k, args.pairs)
            bw.append_batch(bk, nm, order="coordinate")
            # (bytes of the records just written: 36 fixed + name + NUL + the AS tag per alignment, the CIGARs, bases and qualities of the primaries)
            inflated += bk["n_chains"] * (36 + nm.shape[1] + 1 + 7) + 4 * len(bk["cigar"]) + int(1.5 * len(bk["read_bases"]))
            del bk
            k += 1
        bw.close()
    raw, blocks = bgzf_blocks(bam)
    n_inflated = sum(b[2] for b in blocks); n_comp = sum(b[1] for b in blocks)
    print("sample: %s, %.3f GB of BAM, %d BGZF blocks, %.3f GB inflated (ratio %.2f); world and sample made in %.1f s" % (
        "generated" if tmp else bam, raw.size / 1e9, len(blocks), n_inflated / 1e9, n_inflated / max(1, n_comp), time.time() - t0))
    if n_inflated < args.min_inflated_gb * 1e9:
        print("WARNING: the file holds %.3f GB inflated, less than the %.3f GB asked for (--min-inflated-gb)" % (n_inflated / 1e9, args.min_inflated_gb))
    print("host engine: %s; decoder threads: %s" % (lib.hlala_bam_inflate_engine().decode(), args.threads or "default"))
    inf = None if args.no_gpu else P.Inflater(lib, device=args.device, chunk_bytes=args.chunk_mb << 20)
    keys = ("index", "inflate", "parse", "group", "name_sort", "layout")
    if args.resident_decoder:
        assert inf, "--resident-decoder needs a GPU"
        resident_decoder(P, lib, inf, w, bam, intervals, args)
        inf.close()
        if tmp:
            import shutil
            shutil.rmtree(tmp, ignore_errors=True)
        return

    def run(label, opener, timed):
        t = time.time(); S = opener(); wall = time.time() - t
        tm = S.timing(); cnt = S.inflate_counts(); pc = S.parse_counts(); tb = S.transfer_bytes(); cc = S.crc_counts(); gc = S.group_counts(); sc = S.sort_counts(); fc = S.fill_counts(); fm = S.fill_ms(); units = S.n_units; S.close()
        if timed and args.verify_crc:
            print("%-13s wall %.3f s  %s  threads %d  units %d  blocks gpu/retried/host %d/%d/%d  CRC verified gpu/host/rechecked %d/%d/%d" % (
                label, wall, "  ".join("%s %.3f" % (k, tm[k]) for k in keys), tm["threads"], units, cnt[0], cnt[1], cnt[2], cc[0], cc[1], cc[2]))
        elif timed:
            print("%-15s wall %.3f s  %s  threads %d  units %d  blocks gpu/retried/host %d/%d/%d  records on the GPU %d in %d rounds, %d rounds fell back  PCIe up %.3f GB, down %.3f GB  grouped on the GPU %d, runs regrouped %d, by the host %d  ordered on the GPU %d, merged in %d, by the host %d" % (
                label, wall, "  ".join("%s %.3f" % (k, tm[k]) for k in keys), tm["threads"], units, cnt[0], cnt[1], cnt[2], pc[0], pc[1], pc[2], tb[0] / 1e9, tb[1] / 1e9, gc[0], gc[1], gc[2], sc[0], sc[1], sc[2]))
            if fc != (0, 0, 0):
                print("%-15s filled on the GPU %d units, host units %d, by the host %d; window passes on the device: chain %.3f, cigar %.3f, names %.3f, bases %.3f, download %.3f ms" % (
                    "", fc[0], fc[1], fc[2], fm[0], fm[1], fm[2], fm[3], fm[4]))
        return tm["inflate"], tm["inflate"] + tm["parse"], wall, tm["group"], tm["name_sort"], tm["layout"], tb[0] / 1e9, tb[1] / 1e9, sum(fm[:4]), fm[4]
    host = lambda: P.bam_open_seeds(lib, bam, intervals, threads=args.threads, flags=P.SEEDS_PACKED)                 # noqa: E731
    gpu = (lambda: inf.bam_open_seeds(bam, intervals, threads=args.threads, flags=P.SEEDS_PACKED)) if inf else None      # noqa: E731
    gpu_parse = (lambda: inf.bam_open_seeds(bam, intervals, threads=args.threads, flags=P.SEEDS_PACKED | P.SEEDS_GPU_PARSE)) if inf else None      # noqa: E731
    gpu_group = (lambda: inf.bam_open_seeds(bam, intervals, threads=args.threads, flags=P.SEEDS_PACKED | P.SEEDS_GPU_PARSE | P.SEEDS_GPU_GROUP)) if inf else None      # noqa: E731
    gpu_sort = (lambda: inf.bam_open_seeds(bam, intervals, threads=args.threads, flags=P.SEEDS_PACKED | P.SEEDS_GPU_PARSE | P.SEEDS_GPU_GROUP | P.SEEDS_GPU_SORT)) if inf else None      # noqa: E731
    gpu_fill = (lambda: inf.bam_open_seeds(bam, intervals, threads=args.threads, flags=P.SEEDS_PACKED | P.SEEDS_GPU_PARSE | P.SEEDS_GPU_GROUP | P.SEEDS_GPU_SORT | P.SEEDS_GPU_FILL)) if inf else None      # noqa: E731
    order = ["host", "gpu", "gpu+parse", "gpu+parse+group", "gpu+parse+group+sort", "gpu+parse+group+sort+fill"]
    openers = {"host": host, "gpu": gpu, "gpu+parse": gpu_parse, "gpu+parse+group": gpu_group, "gpu+parse+group+sort": gpu_sort, "gpu+parse+group+sort+fill": gpu_fill}
    if args.paths:
        order = [k for k in order if k in args.paths.split(",")]
    res = {k: [] for k in order}
    kinds = {"hbm": P.INFLATE_KERNEL_HBM, "lds": P.INFLATE_KERNEL_LDS}
    kernels = [k for k in args.inflate_kernels.split(",") if k]
    assert all(k in kinds for k in kernels), "--inflate-kernels: hbm and lds are the kernels"
    if kernels and inf:
        def with_kernel(kind, opener):
            def f():
                inf.set_kernel(kind)
                return opener()
            return f
        order = ["host"] if "host" in order else []
        for pth, opener in (("gpu", gpu), ("gpu+parse", gpu_parse)):
            if not args.paths or pth in args.paths.split(","):
                for kn in kernels:
                    openers["%s[%s]" % (pth, kn)] = with_kernel(kinds[kn], opener); order.append("%s[%s]" % (pth, kn))
        res = {k: [] for k in order}
    if args.verify_crc:
        V = P.SEEDS_PACKED | P.SEEDS_VERIFY_CRC
        openers["host+crc"] = lambda: P.bam_open_seeds(lib, bam, intervals, threads=args.threads, flags=V)                 # noqa: E731
        openers["gpu+crc"] = (lambda: inf.bam_open_seeds(bam, intervals, threads=args.threads, flags=V)) if inf else None      # noqa: E731
        openers["gpu+parse+crc"] = (lambda: inf.bam_open_seeds(bam, intervals, threads=args.threads, flags=V | P.SEEDS_GPU_PARSE)) if inf else None      # noqa: E731
        order = ["host", "host+crc", "gpu", "gpu+crc", "gpu+parse", "gpu+parse+crc"]
        res = {k: [] for k in order}
    for i in range(args.runs + 1):
        for k in order:
            if openers[k]:
                res[k].append(run(k, openers[k], i > 0))
    for k in order:
        if len(res[k]) > 1:
            v = [x[0] for x in res[k][1:]]
            print("inflate phase, %s: median %.3f s (%.2f GB/s inflated) of %s" % (k, float(np.median(v)), n_inflated / 1e9 / float(np.median(v)), ["%.3f" % x for x in v]))
            for j, what in ((1, "inflate + parse phases"), (3, "group phase"), (4, "sort phase"), (5, "layout + fill phase"), (2, "decode, wall"), (6, "PCIe up, GB"), (7, "PCIe down, GB")):
                v = [x[j] for x in res[k][1:]]
                print("%s, %s: median %.3f%s, range %.3f .. %.3f of %d runs" % (what, k, float(np.median(v)), "" if j >= 6 else " s", min(v), max(v), len(v)))
    if len(res.get("gpu+parse", [])) > 1 and len(res.get("gpu+parse+group", [])) > 1:
        for j, what in ((3, "group phase"), (2, "decode, wall")):
            a = float(np.median([x[j] for x in res["gpu+parse"][1:]])); b = float(np.median([x[j] for x in res["gpu+parse+group"][1:]]))
            print("HLALA_SEEDS_GPU_GROUP against gpu+parse, %s: %+.3f s (median %.3f with against %.3f without)" % (what, b - a, b, a))
    if len(res.get("gpu+parse+group", [])) > 1 and len(res.get("gpu+parse+group+sort", [])) > 1:
        for j, what in ((4, "sort phase"), (2, "decode, wall")):
            a = float(np.median([x[j] for x in res["gpu+parse+group"][1:]])); b = float(np.median([x[j] for x in res["gpu+parse+group+sort"][1:]]))
            print("HLALA_SEEDS_GPU_SORT against gpu+parse+group, %s: %+.3f s (median %.3f with against %.3f without)" % (what, b - a, b, a))
    if len(res.get("gpu+parse+group+sort", [])) > 1 and len(res.get("gpu+parse+group+sort+fill", [])) > 1:
        for j, what in ((5, "layout + fill phase"), (2, "decode, wall")):
            a = float(np.median([x[j] for x in res["gpu+parse+group+sort"][1:]])); b = float(np.median([x[j] for x in res["gpu+parse+group+sort+fill"][1:]]))
            print("HLALA_SEEDS_GPU_FILL against gpu+parse+group+sort, %s: %+.3f s (median %.3f with against %.3f without)" % (what, b - a, b, a))
        for j, what in ((8, "window kernels, device ms"), (9, "window downloads, device ms")):
            v = [x[j] for x in res["gpu+parse+group+sort+fill"][1:]]
            print("HLALA_SEEDS_GPU_FILL, %s: median %.3f, range %.3f .. %.3f of %d runs" % (what, float(np.median(v)), min(v), max(v), len(v)))
    if args.verify_crc:
        for k in ("host", "gpu", "gpu+parse"):
            if len(res[k]) > 1 and len(res[k + "+crc"]) > 1:
                for j, what in ((0, "inflate phase"), (2, "decode, wall")):
                    a = float(np.median([x[j] for x in res[k][1:]])); b = float(np.median([x[j] for x in res[k + "+crc"][1:]]))
                    print("cost of HLALA_SEEDS_VERIFY_CRC, %s, %s: %+.3f s (median %.3f with against %.3f without; %.3f GB inflated)" % (k, what, b - a, b, a, n_inflated / 1e9))
    if inf:
        # the kernel and its copies alone: every block of the file in one call, into one pageable buffer
        out = np.empty(n_inflated, np.uint8); desc = []; u = 0
        for off, clen_, isize in blocks:
            desc.append((off, clen_, isize, u)); u += isize
        if kernels:
            # the kernels alternate on the one inflater: every block of the file in one call, one warm-up call each, then --runs calls each
            per = {kn: [] for kn in kernels}; ref = None
            for i in range(args.runs + 1):
                for kn in kernels:
                    inf.set_kernel(kinds[kn])
                    status, st = inf.inflate(raw, desc, out)
                    assert int((status != 0).sum()) == 0 and st.n_rejected == 0, "the GPU rejected blocks of a valid file"
                    if i == 0:
                        if ref is None:
                            ref = out.copy()
                        else:
                            assert np.array_equal(ref, out), "the kernels leave different bytes"
                        continue
                    per[kn].append((st.ms_kernel, st.ms_wall))
                    print("hlala_bgzf_inflate [%s], all blocks in one call, run %d: upload %.1f ms, kernel %.1f ms, download %.1f ms (device times summed over the chunks; they overlap), "
                          "wall %.1f ms: %.0f blocks/s, %.2f GB/s inflated; kernel alone %.2f GB/s" % (kn, i, st.ms_h2d, st.ms_kernel, st.ms_d2h, st.ms_wall, st.n_blocks / (st.ms_wall / 1e3),
                                                                                                    n_inflated / 1e9 / (st.ms_wall / 1e3), n_inflated / 1e9 / (st.ms_kernel / 1e3)))
            print("the kernels left the same %d bytes (compared after the warm-up calls)" % out.size)
            for kn in kernels:
                for j, what in ((0, "kernel ms summed over the chunks"), (1, "wall ms")):
                    v = [x[j] for x in per[kn]]
                    print("%s, %s: median %.1f, range %.1f .. %.1f of %d runs" % (kn, what, float(np.median(v)), min(v), max(v), len(v)))
            if len(kernels) == 2:
                a, b = kernels
                for j, what in ((0, "kernel"), (1, "wall")):
                    va = [x[j] for x in per[a]]; vb = [x[j] for x in per[b]]
                    print("%s against %s, %s: slowest %s run %.1f ms, fastest %s run %.1f ms: every %s run is %s than every %s run; ratio of the medians %.2f" % (
                        b, a, what, b, max(vb), a, min(va), b, "faster" if max(vb) < min(va) else "NOT faster", a, float(np.median(va)) / float(np.median(vb))))
            inf.close()
            if tmp:
                import shutil
                shutil.rmtree(tmp, ignore_errors=True)
            return
        for i in range(2):
            status, st = inf.inflate(raw, desc, out)
        assert int((status != 0).sum()) == 0 and st.n_rejected == 0, "the GPU rejected blocks of a valid file"
        print("hlala_bgzf_inflate, all blocks in one call (second call): upload %.1f ms, kernel %.1f ms, download %.1f ms (device times summed over the chunks; they overlap), "
              "wall %.1f ms: %.0f blocks/s, %.2f GB/s inflated" % (st.ms_h2d, st.ms_kernel, st.ms_d2h, st.ms_wall, st.n_blocks / (st.ms_wall / 1e3), n_inflated / 1e9 / (st.ms_wall / 1e3)))
        print("kernel alone: %.2f GB/s inflated; download alone: %.2f GB/s" % (n_inflated / 1e9 / (st.ms_kernel / 1e3), n_inflated / 1e9 / max(1e-9, st.ms_d2h / 1e3)))
        if args.verify_crc:
            # the same call with the CRC kernel behind the inflate kernel of every chunk; expected values from the file
            expect = np.array([int.from_bytes(raw[off + clen_:off + clen_ + 4].tobytes(), "little") for off, clen_, _ in blocks], np.uint32)
            tk = []; tc = []; tw = []
            for i in range(args.runs + 1):
                status, st, got = inf.inflate(raw, desc, out, crc=expect, want_crc=True)
                assert int((status != 0).sum()) == 0 and np.array_equal(got, expect), "the GPU reports CRC mismatches on a valid file"
                if i:
                    tk.append(st.ms_kernel); tc.append(inf.ms_crc); tw.append(st.ms_wall)
            med = lambda v: "%.1f (%.1f .. %.1f)" % (float(np.median(v)), min(v), max(v))      # noqa: E731
            print("hlala_bgzf_inflate_crc, all blocks in one call, ms summed over the chunks, median (min .. max) of %d calls after one warm-up: k_bgzf_inflate %s, k_bgzf_crc32 %s, wall %s" % (
                args.runs, med(tk), med(tc), med(tw)))
            print("k_bgzf_crc32 alone: %.1f GB/s inflated, %.3f of the inflate kernel's device time" % (n_inflated / 1e9 / (float(np.median(tc)) / 1e3), float(np.median(tc)) / float(np.median(tk))))
        if args.scan_mb > 0:
            kept = scan_alone(P, inf, out, intervals, args)
            if kept is not None and len(kept[0]):
                perm, flag = group_alone(P, inf, kept[0], kept[1], args)
                name_order_alone(P, inf, kept[0], kept[1], perm, flag, args)
        inf.close()
    if tmp:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
