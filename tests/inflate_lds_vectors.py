"""Raw DEFLATE test vectors for the inflate kernel that keeps a block's history in a ring in LDS (hla-la_amd/csrc/kernel_inflate_lds.hip; rules in inflate_lds_core.h):
tests/test_inflate_lds_model.py on the host model, tests/test_gpu_inflate_lds.py on the device.  Built with the helpers of tests/inflate_vectors.py from the kernel's own
constants -- R bytes of ring, at most B bytes and T tokens per batch, read from the host library --, so that they follow the constants.  Every valid stream is checked
against zlib here, every malformed one is checked to be refused by zlib (or to give another size).
A valid vector is (name, stream, isize, bytes); a malformed one (name, stream, isize, None, expected status)."""
import ctypes as C
import os
import zlib

import numpy as np

import inflate_vectors as V
from inflate_vectors import BitWriter, dynamic_block, fixed_block, zlib_inflate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params():
    """(R, B, batch_tokens) of hlala_host_inflate_lds_params"""
    h = C.CDLL(os.path.join(ROOT, "hla-la_amd", "libhlala_host.so"))
    r, b, t = C.c_int32(), C.c_int32(), C.c_int32()
    h.hlala_host_inflate_lds_params(C.byref(r), C.byref(b), C.byref(t))
    assert r.value % 64 == 0 and r.value >= 32768 + b.value and b.value >= 258 and t.value >= 2
    return r.value, b.value, t.value


def stored(data, final=True, w=None):
    """inflate_vectors.stored_block for long payloads: the bytes are appended at once (the writer stands on a byte boundary behind LEN / NLEN)"""
    w = w or BitWriter()
    w.bits(1 if final else 0, 1); w.bits(0, 2); w.align()
    w.bits(len(data), 16); w.bits(~len(data) & 0xFFFF, 16)
    assert w.n == 0 and len(data) <= 65535
    w.out += bytes(data)
    return w


def noise(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


# A dynamic code that gives every literal, the end of block, every length and every distance symbol a code: 256 literals of 9 bits (1/2), end of block 5 bits (1/32),
# length symbol 257 2 bits (1/4), 258 .. 285 7 bits (28/128); distances 28 of 5 bits and 2 of 4.
DYN_LL = [9] * 256 + [5, 2] + [7] * 28
DYN_DL = [5] * 28 + [4] * 2


def block(kind, tokens, data, final, w):
    """`tokens` as a fixed or dynamic block, or -- stored -- the bytes `data` they stand for"""
    if kind == "fixed":
        return fixed_block(tokens, final=final, w=w)
    if kind == "dynamic":
        return dynamic_block(DYN_LL, DYN_DL, tokens, final=final, w=w)
    return stored(data, final=final, w=w)


def expand(prefix, tokens):
    """the bytes `tokens` add behind `prefix`"""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            for _ in range(n):
                out.append(out[-d])
    return bytes(out[len(prefix):])


def lds_valid_vectors():
    R, B, T = params()
    v = []
    # ---- 1. wrap: stored bytes up to R - k, then a match, a literal, a match: one of them straddles output offset R
    for k in (1, 129, 257, 258):
        head = noise(R - k, k)
        for D in (1, 2, 3, 63, 64, 65, 258, 32767, 32768):
            w = stored(head, final=False); fixed_block([(258, D), 7, (258, D)], w=w)
            v.append(("wrap_k%d_D%d" % (k, D), w.done(), None))
    w = stored(noise(R - 10, 5), final=False); fixed_block(list(range(60, 100)), w=w)
    v.append(("wrap_literals", w.done(), None))
    w = stored(noise(R - 100, 6), final=False); stored(noise(300, 7), final=False, w=w); fixed_block([(258, 200), (100, 32768), 9, (3, 1)], w=w)
    v.append(("wrap_stored", w.done(), None))
    # ---- 2. a stored block longer than the ring: its last R bytes are the history
    w = stored(noise(65000, 8), final=False); fixed_block([(258, 32768), (258, 1), (20, 65)], w=w)
    v.append(("stored_longer_than_ring", w.done(), None))
    # ---- 3. literals behind a far match in ONE batch (the match, then T - 1 literals): what R >= 32768 + B is for
    for D in sorted({32768, 32767, R - B}):
        toks = []
        n = 32768
        while n + 258 + T - 1 <= 65536 - 20:
            toks += [(258, D)] + [(37 * i + n) & 255 for i in range(T - 1)]; n += 258 + T - 1
        w = stored(noise(32768, 9), final=False); fixed_block(toks, w=w)
        v.append(("far_match_then_literals_D%d" % D, w.done(), None))
    # ---- 4. every way a batch closes
    for n in (T - 1, T, T + 1, 2 * T, 2 * T + 1):          # (T tokens: the end of the block is the first token of the next batch)
        v.append(("tokens_%d" % n, fixed_block([(11 * i) & 255 for i in range(n)]).done(), None))
    n258 = (B - 1 - 4) // 258                                # literal, n258 matches of 258, a shorter match, three literals: B + delta bytes in one batch
    rest = B - 1 - 258 * n258 - 3
    assert 3 <= rest - 1 and rest + 1 <= 258 and 1 + n258 + 1 + 3 < T
    for delta in (-1, 0, 1):
        toks = [65] + [(258, 1)] * n258 + [(rest + delta, 1), 66, 67, 68] + [69, (258, 5), 70]
        v.append(("batch_bytes_B%+d" % delta, fixed_block(toks).done(), None))
    toks = [65] + [(258, 1)] * (n258 + 1) + [66, (258, 300)]  # the token that would pass B is a 258-byte match
    v.append(("batch_bytes_match_over_B", fixed_block(toks).done(), None))
    w = fixed_block(list(b"abc") + [(30, 3)], final=False); fixed_block([], w=w)
    v.append(("empty_final_fixed", w.done(), None))
    w = fixed_block(list(b"abc") + [(30, 3)], final=False); stored(b"", w=w)
    v.append(("empty_final_stored", w.done(), None))
    v.append(("isize_0_fixed", fixed_block([]).done(), None))
    v.append(("isize_0_stored", stored(b"").done(), None))
    v.append(("isize_0_dynamic", dynamic_block(DYN_LL, DYN_DL, []).done(), None))
    w = stored(noise(65536 - 258, 10), final=False); fixed_block([(258, 5)], w=w)
    v.append(("isize_65536_ends_in_a_match", w.done(), None))
    # ---- 5. several DEFLATE blocks across the wrap: block A ends and block B's tables are built while A's last batch is still to be placed
    head = noise(R - 700, 11)
    ta = [1, 2, 3, (258, 32768), 200, (100, 3), (40, 30000)] + list(range(90, 150)) + [(60, 61)]
    tb = [250, (258, 32768), 251, (258, 1), (77, 32767), 9, 8, 7] + [(258, 400)] * 2 + list(range(30, 50))
    da = expand(head, ta); db = expand(head + da, tb)
    assert len(head) + len(da) < R < len(head) + len(da) + len(db)
    for ka in ("fixed", "dynamic", "stored"):
        for kb in ("fixed", "dynamic", "stored"):
            w = stored(head, final=False); block(ka, ta, da, False, w); block(kb, tb, db, True, w)
            v.append(("blocks_%s_%s" % (ka, kb), w.done(), head + da + db))
    co = zlib.compressobj(6, zlib.DEFLATED, -15); s = b""
    parts = [V.mixed(R - 300, 31), V.mixed(600, 32), V.bam_like(5000, 6), b"", V.mixed(2000, 33)]
    for p in parts:
        s += co.compress(p) + co.flush(zlib.Z_SYNC_FLUSH)
    s += co.flush()
    v.append(("sync_flush_across_R", s, b"".join(parts)))
    out = []
    for name, stream, data in v:
        z, err = zlib_inflate(stream)
        assert err is None, (name, err)
        assert data is None or z == data, name
        assert len(z) <= 65536, name
        out.append((name, stream, len(z), z))
    names = [x[0] for x in out]
    assert len(set(names)) == len(names)
    sizes = dict((x[0], x[2]) for x in out)
    assert sizes["stored_longer_than_ring"] == 65536 and sizes["isize_65536_ends_in_a_match"] == 65536 and sizes["batch_bytes_B+0"] == B + 260
    assert all(sizes["wrap_k%d_D1" % k] == R - k + 517 for k in (1, 129, 257, 258))
    return out


def lds_error_vectors():
    """a valid full batch (T literals), then a batch whose FIRST token is the error: the decoding side finds it while the batch before is being placed; and the same
    errors at the very first token of the stream"""
    R, B, T = params()
    lits = [(7 * i + 1) & 255 for i in range(T)]
    m = []
    m.append(("far_distance_second_batch", fixed_block(lits + [(3, T + 1), 5]).done(), T + 4, V.FAR_DISTANCE))
    m.append(("output_size_second_batch", fixed_block(lits + [5]).done(), T, V.OUTPUT_SIZE))
    m.append(("output_size_second_batch_match", fixed_block(lits + [(9, 2)]).done(), T + 8, V.OUTPUT_SIZE))
    m.append(("bad_symbol_second_batch", fixed_block(lits + [("sym", 286), 5]).done(), T + 1, V.BAD_SYMBOL))
    m.append(("bad_distance_symbol_second_batch", fixed_block(lits + [("dsym", 3, 30)]).done(), T + 3, V.BAD_SYMBOL))
    s = fixed_block([65] * T + [66] * 10).done()                      # literals below 144 have 8 bits: token T starts at bit 3 + 8 T and is cut after five bits
    m.append(("input_exhausted_second_batch", s[:(3 + 8 * T) // 8 + 1], T + 10, V.INPUT_EXHAUSTED))
    m.append(("far_distance_first_token", fixed_block([(5, 1), 5]).done(), 6, V.FAR_DISTANCE))
    m.append(("output_size_first_token", fixed_block([5]).done(), 0, V.OUTPUT_SIZE))
    m.append(("bad_symbol_first_token", fixed_block([("sym", 287)]).done(), 1, V.BAD_SYMBOL))
    m.append(("input_exhausted_first_token", fixed_block([200, 201]).done()[:1], 2, V.INPUT_EXHAUSTED))
    # a full batch that wraps, then the error: stored bytes to R - 20, T literals, the error
    head = noise(R - 20, 12)
    w = stored(head, final=False); fixed_block(lits + [5], w=w)
    m.append(("output_size_behind_the_wrap", w.done(), R - 20 + T, V.OUTPUT_SIZE))
    out = []
    for name, stream, isize, status in m:
        z, err = zlib_inflate(stream)
        assert err is not None or len(z) != isize, (name, "zlib accepts this stream with exactly isize bytes")
        out.append((name, stream, isize, None, status))
    return out


ALIGN_SIZES = tuple(range(1, 18)) + (63, 64, 65)


def alignment_vectors():
    """(name, stream, isize, bytes, uoff mod 16): small blocks for every alignment of the output range against the 4-byte stores of the flush"""
    out = []
    for n in ALIGN_SIZES:
        data = V.mixed(n, 100 + n)
        s = V.deflate(data, 6) if n % 2 else fixed_block(list(data[:n - n // 2]) + ([(n // 2, 1)] if n // 2 >= 3 else list(data[:n // 2]))).done()
        z, err = zlib_inflate(s)
        assert err is None and len(z) == n, n
        for a in range(16):
            out.append(("align_%d_at_%d" % (n, a), s, n, z, a))
    return out
