"""Tail of the main-stream DP kernels: dp_tail.py [pairs [levels]]   (library built with `make EXTRA=-DHLALA_DP_TIMING=2`; HLALA_LIB_PATH names it)

In that build every wavefront of k_dp<DpTinyJF,0>, <DpTiny,0>, <DpMid,1>, <DpSmall,2> and <DpWide,3> notes the chip's constant-rate clock (100 MHz) when it finds its
last list empty; counters[16 + 2 i] holds the complement of the earliest, [17 + 2 i] the latest of launch i (kernel_dp.hip: dp_class_run).  Latest - earliest is the
time the kernel's slowest calls held it while the wavefronts that had run dry sat idle.  One resident Graph M batch, aligned twice; the second alignment is reported,
with the stage times of the same batch."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package          # noqa: E402
from tools import synth                    # noqa: E402

KERNELS = ("k_dp<DpTinyJF,0> jump-free 16-lane", "k_dp<DpTiny,0>   general 16-lane", "k_dp<DpMid,1>    32-lane", "k_dp<DpSmall,2>  64-lane", "k_dp<DpWide,3>   wide")


def main():
    n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 1_048_576
    levels = int(sys.argv[2]) if len(sys.argv) > 2 else 5_000_000
    P = load_package()
    w = synth.make_world_m(seed=2, n_levels=levels)
    b = synth.make_batch_m(w, n_pairs, seed=1000)
    ctx = P.Context(w["graph"], w["contigs"], insert_mean=b["insert_mean"], insert_sd=b["insert_sd"], rng_seed=12345, max_columns=384)
    gb = ctx.batch(b)
    gb.align(); gb.stats()
    gb.align(); st = gb.stats()
    buf = (C.c_ulonglong * 32)()
    ctx.lib.hlala_debug_counters.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
    ctx._check(ctx.lib.hlala_debug_counters(ctx.h, gb.b, buf), "hlala_debug_counters")
    print("library %s, HLALA_DP_LONG_BASES=%s, %d pairs, Graph M of %d levels" % (os.environ.get("HLALA_LIB_PATH", "(default)"), os.environ.get("HLALA_DP_LONG_BASES", "(default)"), n_pairs, levels))
    t0 = None
    for i, name in enumerate(KERNELS):
        lo, hi = buf[16 + 2 * i], buf[17 + 2 * i]
        if lo == 0 and hi == 0:
            print("  %-36s no clocks (not a -DHLALA_DP_TIMING=2 build, or the kernel did not run)" % name); continue
        first = (~lo) & 0xFFFFFFFFFFFFFFFF
        t0 = first if t0 is None else t0
        print("  %-36s first wavefront out of work at %8.3f ms, last at %8.3f ms: tail %7.3f ms" % (name, (first - t0) * 1e-5, (hi - t0) * 1e-5, (hi - first) * 1e-5))
    print("  stages: project %.2f extend %.2f (dp main %.2f, retry %.2f) pair %.2f ms; calls per class %s" % (st.ms_project, st.ms_extend, st.ms_dp_main, st.ms_extend_retry, st.ms_pair, [int(x) for x in st.n_dp_class]))


if __name__ == "__main__":
    main()
