"""hlala_filter_positions (host) against hlala_filter_positions_gpu (device) on three synthetic loci, the two paths alternating in ONE process: one warm-up and
--runs timed calls each.  Prints per locus the median and range of both paths, the device milliseconds per launch (hlala_filter_gpu_times; timed in a further
set of calls, so that the events do not sit in the wall clocks) and the bytes each way.  The outputs of the two paths are compared on every locus.

    python tools/filter_rate.py [--runs 5] [--device 0] [--out profiles/filter_gpu.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def flat_locus(rng, n_reads, n_exon, span=(20, 120)):
    """the statistics of tests/test_filters.py: synth_positions, built with numpy (40 000 reads in a Python loop take minutes)"""
    truth = rng.integers(0, 4, n_exon)
    a = rng.integers(0, n_exon - 30, n_reads); ln = rng.integers(span[0], span[1], n_reads); b = np.minimum(n_exon, a + ln)
    cnt = (b - a).astype(np.int64); off = np.concatenate([[0], np.cumsum(cnt)]); npos = int(off[-1])
    read = np.repeat(np.arange(n_reads), cnt); x = (np.arange(npos) - off[read] + a[read]).astype(np.int32)
    dirty = rng.random(n_reads) < 0.3
    w = np.ones((n_reads, 2)); w[dirty, 0] = 1.0 - rng.integers(1, 6, dirty.sum()) / 150.0; w[dirty, 1] = 1.0 - rng.integers(0, 4, dirty.sum()) / 150.0
    base = truth[x].copy(); err = dirty[read] & (rng.random(npos) < 0.15); base[err] = rng.integers(0, 4, err.sum())
    ins = rng.random(npos) < 0.01; gap = rng.random(npos) < 0.005
    glen = 1 + ins.astype(np.int64); goff = np.concatenate([[0], np.cumsum(glen)])
    chars = np.full(int(goff[-1]), ord("T"), np.uint8); first = np.frombuffer(b"ACGT", np.uint8)[base].copy(); first[gap] = ord("_"); chars[goff[:-1]] = first
    e = dict(read_pair=np.arange(n_reads, dtype=np.int32), read_weighted_ok=w.reshape(-1).copy(), read_fraction_ok=np.ones(2 * n_reads), read_distance=np.full(n_reads, 200, np.int32),
             read_cols_nongap=np.full(2 * n_reads, 150, np.int32), pos_off=off.astype(np.int32), pos_exon=x, pos_level=(1000 + x).astype(np.int32),
             pos_mate=(1 + ((x - a[read]) * 2 // np.maximum(1, cnt[read]))).astype(np.uint8), pos_mapq=np.where(rng.random(npos) < 0.05, ord("#"), ord("I")).astype(np.uint8),
             pos_novel_gap=np.zeros(npos, np.int32), geno_off=goff.astype(np.int32), geno_chars=chars, qual_chars=np.full(len(chars), 70, np.uint8),
             read_reverse=(rng.random(2 * n_reads) < 0.07).astype(np.uint8))
    e.update(n_reads=n_reads, n_pos=npos, n_chars=len(chars))
    return e


def thin_locus(n_reads=4000, per=70):
    rng = np.random.default_rng(3)
    e = flat_locus(rng, n_reads, 200, span=(per, per + 1))
    e["pos_exon"] = np.arange(e["n_pos"], dtype=np.int32)              # every position an exon position of its own
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5); ap.add_argument("--device", type=int, default=0); ap.add_argument("--out", default="")
    args = ap.parse_args()
    from conftest import load_package
    from tools import synth
    P = load_package()
    lib = C.CDLL(P.LIB_PATH)
    w = synth.make_world(seed=11, G=4000, k=1)
    ctx = P.Context(w["graph"], w["contigs"], insert_mean=200.0, insert_sd=35.0, rng_seed=5, device=args.device)
    loci = [("4000 reads x 546 positions", flat_locus(np.random.default_rng(3), 4000, 546)),
            ("40000 reads x 546 positions", flat_locus(np.random.default_rng(4), 40000, 546, span=(20, 84))),       # (reads of 20-83 positions: about 3800 entries per bucket, under the 4096)
            ("one entry per exon position (280000)", thin_locus())]
    lines = [f"tools/filter_rate.py --runs {args.runs}: hlala_filter_positions (host) and hlala_filter_positions_gpu alternating in one process; seconds, median [min .. max]"]
    for name, e in loci:
        host, gpu = [], []
        for k in range(args.runs + 1):                                   # the first round is the warm-up
            t = time.perf_counter(); h = P.filter_positions(lib, e); th = time.perf_counter() - t
            t = time.perf_counter(); rc, text, use, ign, st, counts = P.filter_positions_gpu(ctx, e, raw=True); tg = time.perf_counter() - t
            if rc != 0:
                break
            assert np.array_equal(use, h[0]) and np.array_equal(ign, h[1]) and st == h[2], name
            if k:
                host.append(th); gpu.append(tg)
        if rc != 0:
            lines.append(f"{name}: {e['n_pos']} positions: refused ({rc}): {text}; host {th:.4f} s")
            continue
        P.filter_gpu_times(ctx, True)
        ms = []
        for k in range(args.runs):
            P.filter_positions_gpu(ctx, e); ms.append(P.filter_gpu_times(ctx, True))
        P.filter_gpu_times(ctx, False)
        med = lambda v: statistics.median(v)
        lines.append(f"{name}: {e['n_pos']} positions, {counts['buckets']} buckets, largest {counts['largest_bucket']}, sorted {counts['buckets_sorted']}, heap sorts {counts['heap_sorts']}")
        lines.append(f"    host   {med(host):.4f} [{min(host):.4f} .. {max(host):.4f}]")
        lines.append(f"    device {med(gpu):.4f} [{min(gpu):.4f} .. {max(gpu):.4f}]   bytes up {counts['bytes_up']}, down {counts['bytes_down']}")
        lines.append("    device ms per launch, median [min .. max]: " + ", ".join(f"{k} {med([m[k] for m in ms]):.3f} [{min(m[k] for m in ms):.3f} .. {max(m[k] for m in ms):.3f}]" for k in ms[0]))
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
