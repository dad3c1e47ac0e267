"""Name arrays for the ordering stage (hlala_bam_name_order / hlala_host_bam_name_order_model), the expectation -- Python's own sorted() on bytes objects, whose comparison
is memcmp and then length -- and the model's binding.  Shared by tests/test_bam_nameorder_model.py (CPU) and tests/test_gpu_bam_nameorder.py: the device is handed exactly
what the model has been shown to take.  Every case comes from a fixed seed."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from conftest import ROOT, load_package

W = 7                        # bam_nameorder_core.h: NAM_W, the name bytes a round looks at (test_bam_nameorder_model.py holds the header against it)
M64 = (1 << 64) - 1
E_ARG, E_DEVICE = -1, -2
COUNT_FIELDS = ("n", "n_rounds", "n_equal_names")
SHORT = bytes([0x00, 0x41, 0xFF])        # random names over three byte values share prefixes across rounds


def place(names, seed=1, align=None, tail=True):
    """names laid into one buffer in a shuffled storage order with gaps of 0..5 noise bytes (align(i): the offset of name i modulo 8; tail=False: the last name stored ends
    the buffer).  Returns (name_off, name_len, data)."""
    rng = np.random.default_rng(seed)
    buf = bytearray(rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8).tobytes())
    off = np.zeros(len(names), np.uint64)
    for i in rng.permutation(len(names)):
        buf += rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8).tobytes()
        if align is not None:
            while len(buf) % 8 != align(int(i)) % 8:
                buf.append(0x5A)
        off[i] = len(buf); buf += names[i]
    if tail:
        buf += rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tobytes()
    return off, np.array([len(x) for x in names], np.uint32), np.frombuffer(bytes(buf), np.uint8)


def names_of(off, ln, data):
    b = data.tobytes()
    return [b[int(o):int(o) + int(k)] for o, k in zip(off, ln)]


def lcp(a, b):
    n = min(len(a), len(b)); k = 0
    while k < n and a[k] == b[k]:
        k += 1
    return k


def expect(names):
    """(order, n_rounds, n_equal_names) from the names alone.  Two different names leave each other's segment in round lcp // W (their keys are equal, valid-byte counts
    included, exactly in the rounds r with (r + 1) W <= lcp); a name that occurs more than once stays with its copies until it ends, in round len // W."""
    order = sorted(range(len(names)), key=lambda i: (names[i], i))
    distinct = sorted(set(names))
    copies = {}
    for x in names:
        copies[x] = copies.get(x, 0) + 1
    last = -1
    for k, x in enumerate(distinct):
        near = max(lcp(x, distinct[k - 1]) if k else 0, lcp(x, distinct[k + 1]) if k + 1 < len(distinct) else 0)
        last = max(last, len(x) // W if copies[x] > 1 else near // W)
    return np.array(order, np.uint32), last + 1, len(names) - len(distinct)


def random_names(rng, n, lo=1, hi=40, alphabet=SHORT, distinct=True):
    out, seen = [], set()
    while len(out) < n:
        x = bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), int(rng.integers(lo, hi + 1))))
        if distinct and x in seen:
            continue
        seen.add(x); out.append(x)
    return out


def differ_at(rng, d):
    """a pair and a triple that first differ at byte d"""
    a = bytes(rng.integers(1, 255, 3 * W, dtype=np.uint8)); b = bytes(rng.integers(1, 255, 3 * W + 2, dtype=np.uint8))
    sub = lambda x, v: x[:d] + bytes([v]) + x[d + 1:]           # noqa: E731
    return [sub(a, 9), sub(a, 200), sub(b, 255), sub(b, 0), sub(b, 128)]


def realistic(rng, n):
    seen = set()
    while len(seen) < n:
        seen.add(b"A00123:45:HXXXXXXXX:1:1101:%d:%d" % (int(rng.integers(1000, 33000)), int(rng.integers(1000, 37000))))
    out = sorted(seen)
    return [out[int(i)] for i in rng.permutation(n)]


def cases():
    """name -> (name_off, name_len, data)"""
    out = {}
    rng = np.random.default_rng(2026)
    # wave and block edges
    for n in (0, 1, 2, 63, 64, 65, 129):
        out[f"n{n}"] = place(random_names(rng, n), seed=n)
    # chunk edges
    for d in (W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1):
        out[f"differ_at_{d}"] = place(differ_at(rng, d), seed=d)
    p = bytes(rng.integers(1, 255, 2 * W, dtype=np.uint8))
    out["w_prefix_of_2w"] = place([p, p[:W], b"zz"], seed=3)
    # NUL and high bytes
    out["nul_tails"] = place([b"ab\0c", b"ab\0\0", b"ab\0", b"ab"], seed=4)
    q = b"QRSTUV"                                              # W - 1 bytes
    out["nul_at_chunk_edge"] = place([q + b"\0" + q + b"\0", q + b"\0" + q, q + b"\0\0", q + b"\0", q, q + b"\0" + q + b"\0\0", q + b"\0" + b"\0" * W, q + b"\0" + b"\0" * (W - 1)], seed=5)
    hb = []
    for at in (0, W - 1, W, 2 * W - 1):
        pre = bytes(rng.integers(1, 255, at, dtype=np.uint8))
        hb += [pre + bytes([v]) + b"tail" for v in (0xFF, 0x7F, 0x80, 0x01)]
    out["high_bytes"] = place(hb, seed=6)
    # equal names
    out["equal_130"] = place([b"one-name-130"] * 130, seed=7)
    base = random_names(rng, 500, 4, 30)
    trip = [x for x in base[:10] for _ in range(2)] + [base[499] + b"x"] * 3
    mixed = base + trip
    out["equal_triples"] = place([mixed[int(i)] for i in rng.permutation(len(mixed))], seed=8)
    # compaction: 5000 names share 24 bytes (unresolved for four rounds); 3000 are alone after the first round (distinct within their first W bytes, first bytes of every value)
    shared = b"shared-prefix-of-24-bytes"[:24]
    many = [shared + b"%04x" % i + bytes(rng.integers(0, 256, int(rng.integers(0, 5)), dtype=np.uint8)) for i in range(5000)]
    solo = [bytes([i % 256, 1 + i // 256]) + bytes(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8)) for i in range(3000)]
    both = many + solo
    out["compaction"] = place([both[int(i)] for i in rng.permutation(len(both))], seed=9)
    # long names
    stem = bytes(rng.integers(0, 256, 296, dtype=np.uint8))
    out["long_300"] = place([stem + struct.pack(">I", int(v)) for v in rng.permutation(1 << 16)[:64]], seed=10)
    stem = bytes(rng.integers(0, 256, 4095, dtype=np.uint8))
    out["long_4096"] = place([stem + b"\x80", stem + b"\x7f"], seed=11)
    huge = bytes(rng.integers(0, 256, 65535, dtype=np.uint8))
    out["long_65535"] = place(random_names(rng, 20) + [huge, huge[:10], huge[:W]], seed=12)
    # placement
    out["every_alignment"] = place(random_names(rng, 64), seed=13, align=lambda i: i)
    data = np.frombuffer(bytes(SHORT[int(v)] for v in rng.integers(0, 3, 260)), np.uint8)
    off = np.array([i % 200 for i in range(230)], np.uint64); ln = np.array([1 + (i * 7) % 40 for i in range(230)], np.uint32)       # windows of one buffer; 30 of them twice
    out["overlapping"] = (off, ln, data)
    out["last_ends_the_buffer"] = place(random_names(rng, 33), seed=14, tail=False)
    # realistic
    out["realistic_20000"] = place(realistic(rng, 20000), seed=15)
    return out


_BUILT = None


def built_cases():
    """the cases and their expectation, computed once and shared: name -> (name_off, name_len, data, (order, n_rounds, n_equal_names))"""
    global _BUILT
    if _BUILT is None:
        _BUILT = {k: (o, ln, d, expect(names_of(o, ln, d))) for k, (o, ln, d) in cases().items()}
    return _BUILT


def load_model():
    pkg = load_package()
    so = os.environ.get("HLALA_HOST_LIB") or os.path.join(ROOT, "hla-la_amd", "libhlala_host.so")
    src = os.path.join(ROOT, "hla-la_amd", "csrc")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(os.path.join(src, f)) for f in ("bam_nameorder_core.h", "bam_nameorder_model.h", "host_check.cpp")):
        subprocess.check_call(["make", "-C", src, "../libhlala_host.so"])
    lib = C.CDLL(so)
    lib.hlala_host_bam_name_order_model.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(pkg.BamNameOrderStats)]
    lib.hlala_host_bam_name_order_model.restype = C.c_int
    lib.hlala_host_last_error.restype = C.c_char_p
    return lib


GUARD, CANARY = 64, 0xC7


def run_model(lib, off, ln, data, n=None, n_bytes=None):
    """(rc, order, counts, error text); the output between canaries, which must survive; with a return code other than 0 nothing may have been written"""
    pkg = load_package()
    off = np.ascontiguousarray(off, np.uint64).copy(); ln = np.ascontiguousarray(ln, np.uint32).copy(); data = np.ascontiguousarray(data, np.uint8).copy()
    k = len(off)
    order = np.full(2 * GUARD + 4 * k, CANARY, np.uint8); st = pkg.BamNameOrderStats()
    rc = lib.hlala_host_bam_name_order_model(off.ctypes.data if k else None, ln.ctypes.data if k else None, k if n is None else n, data.ctypes.data if data.size else None,
                                             data.size if n_bytes is None else n_bytes, order.ctypes.data + GUARD, C.byref(st))
    assert (order[:GUARD] == CANARY).all() and (order[len(order) - GUARD:] == CANARY).all()
    if rc != 0:
        assert (order == CANARY).all()
    return rc, order[GUARD:GUARD + 4 * k].view(np.uint32), {f: int(getattr(st, f)) for f in COUNT_FIELDS}, lib.hlala_host_last_error().decode()


def malformed():
    """name -> (name_off, name_len, data, n or None, n_bytes or None, what the refusal says)"""
    off, ln, data = place(random_names(np.random.default_rng(77), 40), seed=16, tail=False)
    out = {}
    out["name_beyond_buffer"] = (off, ln, data, None, len(data) - 1, "beyond the byte buffer")
    o = off.copy(); o[7] = M64 - 3
    out["name_off_wraps"] = (o, ln, data, None, None, "beyond the byte buffer")
    o = off.copy(); o[9] = len(data)
    out["name_off_at_the_end"] = (o, ln, data, None, None, "beyond the byte buffer")
    k = ln.copy(); k[11] = 0
    out["name_len_0"] = (off, k, data, None, None, "name_len 0")
    k = ln.copy(); k[5] = 65536
    out["name_len_65536"] = (off, k, np.concatenate([data, np.zeros(70000, np.uint8)]), None, None, "longer than 65535")
    out["no_bytes"] = (off, ln, data[:0], None, None, "beyond the byte buffer")
    out["too_many"] = (off, ln, data, 1 << 31, None, "2^31")
    out["negative_n"] = (off, ln, data, -1, None, "negative")
    return out


def write_check_file(path, cases_):
    """[(name_off, name_len, data, n_bytes)] in the format tools/bam_nameorder_check.cpp reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases_)))
        for off, ln, data, n_bytes in cases_:
            nb = len(data) if n_bytes is None else n_bytes
            f.write(struct.pack("<qQ", len(off), nb))
            f.write(np.ascontiguousarray(off, np.uint64).tobytes()); f.write(np.ascontiguousarray(ln, np.uint32).tobytes()); f.write(bytes(data[:nb]))


def fnv(b: bytes):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & M64
    return h
