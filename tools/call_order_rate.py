"""hlala_call_locus with the order of the pair table made on the host (std::sort + std::reverse, the default) against the same call with the order made on the device
(hlala_set_call_order_gpu), the two paths alternating in ONE process on the tables of tests/test_call.py: table_rows at C = 3000 with duplicated clusters and at
C = 5000: one warm-up and --runs timed calls each, the orders compared every time.  Prints per table the median and range of the whole call on both paths, the
counters of the device path, and its device milliseconds per phase (hlala_call_order_times; timed in a further set of calls, so that the events do not sit in the
wall clocks).

    python tools/call_order_rate.py [--runs 7] [--device 0] [--out profiles/call_order_gpu.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7); ap.add_argument("--device", type=int, default=0); ap.add_argument("--out", default="")
    ap.add_argument("--clusters", default="3000,5000")
    args = ap.parse_args()
    from conftest import load_package
    from test_call import table_rows
    from tools import synth
    P = load_package()
    w = synth.make_world(seed=11, G=4000, k=1)
    ctx = P.Context(w["graph"], w["contigs"], insert_mean=200.0, insert_sd=35.0, rng_seed=5, device=args.device)
    dups = {3000: ((5, 17), (2999, 0), (1500, 1499), (1501, 1499))}
    med = statistics.median
    lines = [f"tools/call_order_rate.py --runs {args.runs}: hlala_call_locus, the order on the host and on the device alternating in one process; seconds of the whole call, median [min .. max]"]
    for Cn in (int(x) for x in args.clusters.split(",")):
        ll, ma, mm = table_rows(Cn, np.random.default_rng(100 + Cn), dups.get(Cn, ()))
        host, gpu, counts = [], [], None
        for k in range(args.runs + 1):                                   # the first round is the warm-up
            ctx.set_call_order_gpu(False)
            t = time.perf_counter(); h = ctx.call_locus(ll, ma, mm); th = time.perf_counter() - t
            ctx.set_call_order_gpu(True)
            t = time.perf_counter(); g = ctx.call_locus(ll, ma, mm); tg = time.perf_counter() - t
            counts = ctx.call_order_counts()
            assert np.array_equal(g["order"], h["order"]), Cn
            if k:
                host.append(th); gpu.append(tg)
        ctx.call_order_times(True)
        ms = []
        for k in range(args.runs):
            ctx.call_locus(ll, ma, mm); ms.append(ctx.call_order_times(True))
        ctx.call_order_times(False); ctx.set_call_order_gpu(False)
        path = ("host", "device", "refused: NaN", "refused: heap range", "refused: no scratch")[counts["path"]]
        lines.append(f"C = {Cn} ({len(ll)} pairs, {h['n_sort_ties']} adjacent ties): device path: {path}, {counts['levels']} levels, {counts['tile_ranges']} tile ranges (largest {counts['largest_tile']}), "
                     f"heap sorts {counts['heap_sorts']} (largest {counts['largest_heap']}), bytes down {counts['bytes_down']}")
        lines.append(f"    order on the host   {med(host):.4f} [{min(host):.4f} .. {max(host):.4f}]")
        lines.append(f"    order on the device {med(gpu):.4f} [{min(gpu):.4f} .. {max(gpu):.4f}]   every device run below every host run: {'yes' if max(gpu) < min(host) else 'NO'}")
        lines.append("    device ms per phase, median [min .. max]: " + ", ".join(f"{k} {med([m[k] for m in ms]):.3f} [{min(m[k] for m in ms):.3f} .. {max(m[k] for m in ms):.3f}]" for k in ms[0]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
