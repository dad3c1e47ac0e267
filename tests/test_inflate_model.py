"""The DEFLATE decoder core of the BGZF inflate kernel (hla-la_amd/csrc/inflate_core.h) on the host: hlala_host_inflate_model of libhlala_host.so is the core
plus a serial copy loop.  Every expected answer is zlib's.  The malformed streams run here first: the device test hands the same streams to the kernel only
because this file shows the core bounded on them (tools/asan_host.sh runs it under ASan / UBSan)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import inflate_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


@pytest.fixture(scope="module")
def model():
    so = os.environ.get("HLALA_HOST_LIB") or os.path.join(ROOT, "hla-la_amd", "libhlala_host.so")
    src = os.path.join(ROOT, "hla-la_amd", "csrc")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(os.path.join(src, f)) for f in ("inflate_core.h", "host_check.cpp")):
        subprocess.check_call(["make", "-C", src, "../libhlala_host.so"])
    lib = C.CDLL(so)
    lib.hlala_host_inflate_model.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]; lib.hlala_host_inflate_model.restype = C.c_int

    def run(stream, isize):
        """(status, output bytes); the stream and the output sit in exactly-sized heap buffers between canaries, which must survive"""
        comp = np.full(len(stream) + 32, CANARY, np.uint8); comp[16:16 + len(stream)] = np.frombuffer(bytes(stream), np.uint8)
        out = np.full(isize + 32, CANARY, np.uint8)
        rc = lib.hlala_host_inflate_model(comp.ctypes.data + 16, len(stream), out.ctypes.data + 16, isize)
        assert (out[:16] == CANARY).all() and (out[16 + isize:] == CANARY).all(), "the model wrote outside [0, isize)"
        return rc, out[16:16 + isize].tobytes()
    return run


@pytest.fixture(scope="module")
def valid():
    return V.valid_vectors()


def test_valid_streams_equal_zlib(model, valid):
    names = [v[0] for v in valid]
    for want in ("mixed_0_l0", "mixed_65536_l9", "strategy_fixed", "strategy_huffman_only", "strategy_rle", "fibonacci_15bit", "flush_sync", "flush_full", "zeros_rle",
                 "noise_l0", "bam_like", "trailing_garbage", "distance_32768", "distance_equals_produced", "one_distance_code", "literals_only",
                 "repeat_crosses_boundary", "matches_65", "matches_129"):
        assert want in names
    for name, stream, isize, data in valid:
        rc, out = model(stream, isize)
        assert rc == V.OK, (name, rc)
        assert out == data, name


def test_the_vectors_are_what_they_claim(valid):
    """the properties the issue names, checked on the streams themselves"""
    by = {v[0]: v for v in valid}
    # Fibonacci frequencies: a dynamic block (BTYPE 2) whose literal code reaches 15 bits -- beyond the primary table
    fib = by["fibonacci_15bit"]
    assert len(fib[3]) == 46367 and (fib[1][0] >> 1) & 3 == 2
    # incompressible bytes at level 0: two stored blocks (65535 + 1)
    n0 = by["noise_l0"][1]
    assert n0[0] & 7 == 0 and len(n0) == 65536 + 2 * 5
    # two identical random 32 KiB halves: zlib itself stores them (its matches stop short of 32 768)
    half = by["distance_32768"][3][:32768]
    assert len(V.deflate(half + half, 9)) > 65536
    # all zeros with Z_RLE: distance 1, length 258
    assert len(by["zeros_rle"][1]) < 400


@pytest.mark.parametrize("maker", [V.malformed_vectors, V.truncation_vectors])
def test_malformed_streams_are_rejected(model, maker):
    vec = maker()
    assert len(vec) > 20
    for name, stream, isize, _, status in vec:
        rc, _ = model(stream, isize)
        assert rc != V.OK and 1 <= rc <= 7, (name, rc)
        if status is not None:
            assert rc == status, (name, rc, status)


def test_every_single_bit_flip(model):
    """model OK => zlib accepts the flipped stream with exactly isize bytes, and the bytes are equal.  zlib accepts most flips, so both branches are taken."""
    stream, data = V.flip_stream()
    assert 40 <= len(stream) <= 80
    rc, out = model(stream, len(data))
    assert rc == V.OK and out == data
    accepted = rejected = zlib_ok = 0
    for bit in range(8 * len(stream)):
        s = bytearray(stream); s[bit >> 3] ^= 1 << (bit & 7)
        z, err = V.zlib_inflate(s)
        zlib_ok += err is None
        rc, out = model(bytes(s), len(data))
        if rc == V.OK:
            accepted += 1
            assert err is None and len(z) == len(data) and out == z, bit
        else:
            rejected += 1
            assert 1 <= rc <= 7
    assert accepted >= 1 and rejected >= 1, (accepted, rejected, zlib_ok)


def test_random_bytes_terminate(model):
    """any input terminates with a status; whatever the model accepts is what zlib gives"""
    rng = np.random.default_rng(9)
    for i in range(300):
        s = bytes(rng.integers(0, 256, int(rng.integers(1, 200)), dtype=np.uint8))
        s = bytes([(s[0] & 0xF8) | (1, 3, 5)[i % 3]]) + s[1:]            # final block; stored / fixed / dynamic
        isize = int(rng.integers(0, 300))
        rc, out = model(s, isize)
        assert 0 <= rc <= 7
        if rc == V.OK:
            z, err = V.zlib_inflate(s)
            assert err is None and z == out
