"""The CRC-32 split of hla-la_amd/csrc/crc32_core.h on the host (hlala_host_crc32_model of libhlala_host.so: the 64 lanes of k_bgzf_crc32 in a loop) against zlib.crc32, and
the same core under ASan / UBSan in a stand-alone program (tools/crc32_check.cpp).  No device."""
import ctypes as C
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import crc32_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    host = C.CDLL(os.path.join(ROOT, "hla-la_amd", "libhlala_host.so"))
    host.hlala_host_crc32_model.argtypes = [C.c_void_p, C.c_uint32]
    host.hlala_host_crc32_model.restype = C.c_uint32

    def run(data):
        buf = np.frombuffer(data, np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
        return int(host.hlala_host_crc32_model(buf.ctypes.data, len(data)))
    return run


def test_check_string(model):
    assert model(K.CHECK[0]) == K.CHECK[1] == zlib.crc32(K.CHECK[0])


def test_every_case_equals_zlib(model):
    for name, data in K.cases():
        assert model(data) == zlib.crc32(data), name


def test_segments_tile_the_block():
    """the split the cases are chosen for: 64 segments, in order, that cover [0, n) exactly; the short ones lead"""
    for n in K.LENGTHS + [300, 1000, 65280]:
        at = 0
        for j in range(64):
            lo, hi = K.segment(n, j)
            assert lo == at and hi >= lo and hi - lo <= K.seg_len(n)
            at = hi
        assert at == n and K.seg_len(n) % 4 == 0 and 64 * K.seg_len(n) >= n
    assert K.seg_len(256) == 4 and K.seg_len(257) == 8 and K.seg_len(65536) == 1024


def test_any_single_bit_changes_the_crc(model):
    data = bytearray(np.random.default_rng(4).integers(0, 256, 257, dtype=np.uint8).tobytes())
    ref = model(bytes(data))
    for bit in range(0, 8 * len(data), 7):
        data[bit >> 3] ^= 1 << (bit & 7)
        assert model(bytes(data)) == zlib.crc32(bytes(data)) != ref
        data[bit >> 3] ^= 1 << (bit & 7)


def test_the_core_under_sanitizers_in_a_program_of_its_own(model, tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is what builds libhlala_host.so as well"
    exe = tmp_path / "crc32_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe),
                           os.path.join(ROOT, "tools", "crc32_check.cpp")])
    cases = K.cases()
    K.write_case_file(tmp_path / "cases.bin", [d for _, d in cases])
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    for (name, data), line in zip(cases, lines):
        assert int(line, 16) == zlib.crc32(data), name
