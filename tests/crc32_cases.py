"""Cases of the CRC-32 tests (tests/test_crc32_model.py on the CPU, tests/test_gpu_bgzf_crc.py on the device): byte strings at the lengths where the split of
hla-la_amd/csrc/crc32_core.h changes shape, and raw DEFLATE streams that hold them.  Expected values are zlib.crc32 everywhere."""
import struct
import zlib

import numpy as np

# 64 lanes, segments of L = max(4, ceil(n / 64) rounded up to a multiple of 4) bytes aligned to the END of the block: up to 256 bytes L is 4 and leading lanes are
# empty or short, L steps from 4 to 8 between 256 and 257, 65536 is the largest block (L = 1024)
LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536]
CHECK = (b"123456789", 0xCBF43926)


def seg_len(n):
    return max(4, ((n + 63) // 64 + 3) // 4 * 4)


def segment(n, j):
    """[lo, hi) of lane j"""
    L = seg_len(n)
    return max(0, n - (64 - j) * L), max(0, n - (63 - j) * L)


def contents(n, seed):
    """(kind, bytes) of length n: all zero (only the initial value tells lengths apart), all 0xFF, random, zeros followed by data"""
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    lead = bytes(n - n // 3) + rnd[:n // 3]
    return [("zero", bytes(n)), ("ff", b"\xff" * n), ("random", rnd), ("leading_zeros", lead)]


def cases():
    """[(name, bytes)]: every length with every content, and the check string"""
    out = [("check", CHECK[0])]
    for n in LENGTHS:
        for kind, data in contents(n, 1000 + n):
            out.append(("%s_%d" % (kind, n), data))
    return out


def stored(data):
    """raw DEFLATE of `data` as stored blocks (at most 65535 bytes each)"""
    parts = [data[i:i + 65535] for i in range(0, len(data), 65535)] or [b""]
    out = bytearray()
    for k, p in enumerate(parts):
        out += struct.pack("<BHH", 1 if k == len(parts) - 1 else 0, len(p), ~len(p) & 0xFFFF) + p
    return bytes(out)


def stored_position(i):
    """where byte i of the data stands in stored(data)"""
    return 5 * (i // 65535 + 1) + i


def deflated(data):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


def write_case_file(path, datas):
    """the format tools/crc32_check.cpp reads: int32 number of cases; per case u32 n, data[n]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(datas)))
        for d in datas:
            f.write(struct.pack("<I", len(d))); f.write(d)
