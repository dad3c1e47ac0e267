"""The host model of the inflate kernel with the history in LDS (hla-la_amd/csrc/inflate_lds_core.h, inflate_lds_model.h; hlala_host_inflate_lds_model of
libhlala_host.so) against the model of the first kernel (hlala_host_inflate_model) and against zlib, the word-wise token function against token() step by step, and the
same text under ASan / UBSan in a stand-alone program (tools/inflate_lds_check.cpp).  No device."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import inflate_lds_vectors as L
import inflate_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


@pytest.fixture(scope="module")
def host():
    h = C.CDLL(os.path.join(ROOT, "hla-la_amd", "libhlala_host.so"))
    h.hlala_host_inflate_model.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32]
    h.hlala_host_inflate_lds_model.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32]
    h.hlala_host_inflate_lds_rounds.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)]
    h.hlala_host_inflate_lds_token_steps.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    return h


@pytest.fixture(scope="module")
def cases():
    """[(name, stream, isize, zlib's bytes or None)]: the vectors of both kernels, every single-bit flip of flip_stream, random bytes"""
    out = [(n, s, z, d) for n, s, z, d in V.valid_vectors() + L.lds_valid_vectors()]
    out += [(n, s, z, None) for n, s, z, _, _ in V.malformed_vectors() + V.truncation_vectors() + L.lds_error_vectors()]
    out += [(n, s, z, d) for n, s, z, d, _ in L.alignment_vectors()[::16]]
    flip, fdata = V.flip_stream()
    for bit in range(8 * len(flip)):
        s = bytearray(flip); s[bit >> 3] ^= 1 << (bit & 7)
        out.append(("flip_%d" % bit, bytes(s), len(fdata), None))
    rng = np.random.default_rng(77)
    for i in range(300):
        n = int(rng.integers(1, 400))
        s = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        s[0] = (s[0] & 0xF8) | int(rng.integers(0, 8)) if i % 3 else (s[0] & 0xF8) | 3      # two in three start with the fixed code, final block
        out.append(("random_%d" % i, bytes(s), int(rng.integers(0, 700)), None))
    return out


def both(host, s, isize):
    a = np.full(isize + 16, CANARY, np.uint8); b = np.full(isize + 16, CANARY, np.uint8)
    ra = host.hlala_host_inflate_model(bytes(s), len(s), a.ctypes.data + 8, isize)
    rb = host.hlala_host_inflate_lds_model(bytes(s), len(s), b.ctypes.data + 8, isize)
    assert (b[:8] == CANARY).all() and (b[8 + isize:] == CANARY).all(), "the model wrote outside [0, isize)"
    return ra, rb, a[8:8 + isize], b[8:8 + isize]


def test_the_ring_rule_holds_for_the_constants():
    R, B, T = L.params()
    assert R % 64 == 0 and R >= 32768 + B and 2 * R > 65536 and B >= 258 and T == 64
    # what the kernel keeps in LDS beside the ring (tables 3200, window 512, two units, state) must leave it at or below 160 KiB / 4
    assert R + 3200 + 512 + 2 * (4 * T + 28) + 36 <= 40960


def test_same_status_and_bytes_as_the_first_model(host, cases):
    n_ok = 0
    for name, s, isize, data in cases:
        ra, rb, a, b = both(host, s, isize)
        assert ra == rb, (name, ra, rb)
        if ra == 0:
            assert np.array_equal(a, b), name
            n_ok += 1
            if data is not None:
                assert b.tobytes() == data, name
        elif data is not None and not name.startswith("flip_"):
            pytest.fail("%s: a valid stream was refused with status %d" % (name, ra))
    assert n_ok > 150


def test_expected_statuses_of_the_new_malformed_vectors(host):
    for name, s, isize, _, want in L.lds_error_vectors():
        ra, rb, _, _ = both(host, s, isize)
        assert ra == rb == want, (name, ra, rb, want)


def test_token_w_equals_token_step_by_step(host, cases):
    cap = 8192
    tok = np.zeros(2 * cap, np.uint32); rc = np.zeros(2 * cap, np.int32); bits = np.zeros(2 * cap, np.uint64)
    steps = compared = 0
    for name, s, isize, data in cases:
        n = host.hlala_host_inflate_lds_token_steps(bytes(s), len(s), cap, tok.ctypes.data, rc.ctypes.data, bits.ctypes.data)
        if n <= 0:
            continue                                    # the stream does not start with a compressed block
        compared += 1; steps += n
        t = tok[:2 * n].reshape(n, 2); r = rc[:2 * n].reshape(n, 2); b = bits[:2 * n].reshape(n, 2)
        assert np.array_equal(r[:, 0], r[:, 1]), name                       # result: token, end of block, or a status
        assert np.array_equal(b[:, 0], b[:, 1]), name                       # bits consumed
        is_tok = r[:, 0] == -1
        assert np.array_equal(t[is_tok, 0], t[is_tok, 1]), name             # the token
    assert compared > 300 and steps > 100000


def test_rounds_follow_the_batches(host):
    """the kernel's barrier count, read from the model: one round per unit and one more in which the last unit is placed"""
    R, B, T = L.params()
    r = C.c_int32()
    out = np.zeros(65536, np.uint8)

    def rounds(stream, isize):
        st = host.hlala_host_inflate_lds_rounds(bytes(stream), len(stream), out.ctypes.data, isize, C.byref(r))
        return st, r.value
    assert rounds(b"", 0) == (V.INPUT_EXHAUSTED, 2)
    assert rounds(V.fixed_block([]).done(), 0) == (0, 2)
    assert rounds(V.fixed_block([1] * (T - 1)).done(), T - 1) == (0, 2)
    assert rounds(V.fixed_block([1] * T).done(), T) == (0, 3)                # the end of the block is a batch of its own
    assert rounds(V.fixed_block([1] * (T + 1)).done(), T + 1) == (0, 3)
    assert rounds(L.stored(b"abc").done(), 3) == (0, 2)
    w = L.stored(b"abc", final=False); V.fixed_block([5], w=w)
    assert rounds(w.done(), 4) == (0, 3)
    v = dict((x[0], x) for x in L.lds_valid_vectors())
    for delta, want in ((-1, 3), (0, 3), (1, 3)):                            # two batches whatever the first one's last token is
        name, s, isize, _ = v["batch_bytes_B%+d" % delta]
        assert rounds(s, isize) == (0, want), name


def test_the_model_under_sanitizers_in_a_program_of_its_own(host, cases, tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is what builds libhlala_host.so as well"
    exe = tmp_path / "inflate_lds_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe),
                           os.path.join(ROOT, "tools", "inflate_lds_check.cpp")])
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for name, s, isize, data in cases:
            f.write(struct.pack("<II", len(s), isize) + bytes(s))
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    rr = C.c_int32()
    for (name, s, isize, data), line in zip(cases, lines):
        st, rounds, h = line.split()
        out = np.zeros(isize + 1, np.uint8)
        want = host.hlala_host_inflate_lds_rounds(bytes(s), len(s), out.ctypes.data, isize, C.byref(rr))
        assert (int(st), int(rounds)) == (want, rr.value), name
        if want == 0:
            assert int(h, 16) == zlib.crc32(out[:isize].tobytes()), name
