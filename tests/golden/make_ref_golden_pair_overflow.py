"""Regenerates tests/golden/ref_pair_overflow.npz: the batch of tests/pair_overflow_cases.over_fixture() -- pairs beyond the capacities of the pairing kernels: 65
kept chains on either mate, 1040 and 1025 combinations -- and what the REFERENCE's own processBAM.cpp makes of it (ref_pair_chains of oracle/ref/ref_driver.cpp),
written by write() of make_ref_golden_pipeline.py, whose layout, provenance hash and size cap for ref_pair_limits.npz it shares.
tests/test_gpu_pair_overflow.py holds the kernels, with the overflow class on, against the file directly.  Run (needs the reference sources; HLALA_REF_DIR names them):
    python tests/golden/make_ref_golden_pair_overflow.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ref_golden_pipeline import MAX_PAIR_LIMITS_BYTES, rb, write          # noqa: E402
import pair_overflow_cases as po              # noqa: E402


def main():
    ok, why = rb.available()
    if not ok:
        raise SystemExit(why)
    f = po.over_fixture()
    write("overflow", f["world"], f["batch"], kinds=("pair",), max_bytes=MAX_PAIR_LIMITS_BYTES)


if __name__ == "__main__":
    main()
