"""Raw DEFLATE test vectors of the BGZF inflate (tests/test_inflate_model.py on the host model, tests/test_gpu_inflate.py on the device).
Valid streams come from zlib or from the bit writer below (streams zlib never emits); every expected answer is zlib's (decompressobj(-15)).
A vector is (name, stream bytes, isize, expected bytes or None for a malformed stream)."""
import struct
import zlib

import numpy as np

OK, RESERVED_BTYPE, STORED_LEN, BAD_CODE, BAD_SYMBOL, FAR_DISTANCE, INPUT_EXHAUSTED, OUTPUT_SIZE = range(8)      # HLALA_INFLATE_* of include/hlala_gpu.h


def zlib_inflate(stream, limit=1 << 17):
    """(bytes, None) when zlib accepts the raw DEFLATE stream (trailing bytes ignored), (None, message) otherwise."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(stream), limit)
    except zlib.error as e:
        return None, str(e)
    if not d.eof:
        return None, "incomplete stream" if not d.unconsumed_tail else "more output than the limit"
    return out, None


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(bytes(data)) + co.flush()


# ---------------------------------------------------------------------------------------------- bit writer (RFC 1951, 3.1.1)
class BitWriter:
    def __init__(self):
        self.out = bytearray(); self.acc = 0; self.n = 0

    def bits(self, value, count):
        """`count` bits of `value`, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << count) - 1)) << self.n; self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def code(self, code, length):
        """a Huffman code, most significant bit first"""
        for i in range(length - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: (code, length)} of RFC 3.2.2"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt = [0] * 16; code = 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1; nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l); nxt[l] += 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def put_tokens(w, tokens, lit, dist):
    """tokens: ints (literals), (length, distance) pairs, ("sym", s) raw literal/length symbols, ("dsym", length, d) a match with a raw distance symbol"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t]); continue
        if t[0] == "sym":
            w.code(*lit[t[1]]); continue
        rawd = t[0] == "dsym"
        length, d = (t[1], t[2]) if rawd else t
        k = max(i for i in range(29) if LEN_BASE[i] <= length)
        if length == 258:
            k = 28
        w.code(*lit[257 + k]); w.bits(length - LEN_BASE[k], LEN_EXTRA[k])
        if rawd:
            w.code(*dist[d]); continue
        j = max(i for i in range(30) if DIST_BASE[i] <= d)
        w.code(*dist[j]); w.bits(d - DIST_BASE[j], DIST_EXTRA[j])
    w.code(*lit[256])


def fixed_block(tokens, final=True, w=None):
    w = w or BitWriter()
    w.bits(1 if final else 0, 1); w.bits(1, 2)
    put_tokens(w, tokens, FIXED_LIT, FIXED_DIST)
    return w


def stored_block(data, final=True, w=None, nlen=None):
    w = w or BitWriter()
    w.bits(1 if final else 0, 1); w.bits(0, 2); w.align()
    w.bits(len(data), 16); w.bits((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
    for b in data:
        w.bits(b, 8)
    return w


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_header(w, hlit, hdist, cl_lengths, cl_symbols, final=True, hclen=19):
    """cl_lengths: the 19 code lengths of the code length code (by symbol); cl_symbols: its symbols in stream order, (16|17|18, extra) for the repeats"""
    w.bits(1 if final else 0, 1); w.bits(2, 2)
    w.bits(hlit - 257, 5); w.bits(hdist - 1, 5); w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl_lengths[CL_ORDER[i]], 3)
    cl = canonical(cl_lengths)
    for s in cl_symbols:
        if isinstance(s, tuple):
            w.code(*cl[s[0]]); w.bits(s[1], {16: 2, 17: 3, 18: 7}[s[0]])
        else:
            w.code(*cl[s])


FLAT_CL = [4] * 13 + [5] * 6          # a complete code length code that gives every symbol a code: 13 codes of 4 bits, 6 of 5


def expand_cl(symbols):
    """the code lengths a sequence of code length symbols stands for"""
    out = []
    for s in symbols:
        if isinstance(s, tuple):
            out += [out[-1]] * (3 + s[1]) if s[0] == 16 else [0] * ((3 if s[0] == 17 else 11) + s[1])
        else:
            out.append(s)
    return out


def compact_cl(lengths):
    """code length symbols for `lengths` with the runs of zeros sent as 17 / 18"""
    out = []; i = 0
    while i < len(lengths):
        j = i
        while j < len(lengths) and lengths[j] == 0:
            j += 1
        run = j - i
        if run >= 3:
            run = min(run, 138); out.append((18, run - 11) if run >= 11 else (17, run - 3)); i += run
        else:
            out.append(lengths[i]); i += 1
    assert expand_cl(out) == list(lengths)
    return out


def dynamic_block(lit_lengths, dist_lengths, tokens, final=True, w=None, compact=False):
    """a dynamic block: the code lengths sent one by one (or with zero runs, compact=True) in the flat code length code, then the tokens (None: the header alone)"""
    w = w or BitWriter()
    hlit = max(257, len(lit_lengths)); hdist = max(1, len(dist_lengths))
    ll = list(lit_lengths) + [0] * (hlit - len(lit_lengths)); dl = list(dist_lengths) + [0] * (hdist - len(dist_lengths))
    dynamic_header(w, hlit, hdist, FLAT_CL, compact_cl(ll + dl) if compact else ll + dl, final)
    if tokens is not None:
        put_tokens(w, tokens, canonical(ll), canonical(dl))
    return w


def lit_only_lengths(symbols):
    """complete code over `symbols` + end-of-block, all of one length (the count is padded to a power of two by giving short codes to the first symbols)"""
    syms = sorted(set(symbols) | {256})
    n = len(syms); k = 1
    while (1 << k) < n:
        k += 1
    short = (1 << k) - n                 # that many symbols get k - 1 bits (each takes the room of two k-bit codes)
    ll = [0] * 257
    for i, s in enumerate(syms):
        ll[s] = k - 1 if i < short else k
    if n == 1:
        raise ValueError("one symbol")
    return ll


# ---------------------------------------------------------------------------------------------- payloads
def fibonacci_payload():
    """22 symbols with Fibonacci frequencies (46 367 bytes): Z_HUFFMAN_ONLY gives a dynamic block with 15-bit literal codes"""
    f = [1, 1]
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    rng = np.random.default_rng(5)
    data = np.concatenate([np.full(n, 40 + i, np.uint8) for i, n in enumerate(f)])
    rng.shuffle(data)
    return data.tobytes()


def bam_like(n, seed=3):
    rng = np.random.default_rng(seed); out = bytearray()
    while len(out) < n:
        name = b"read%06d\0" % int(rng.integers(0, 10 ** 6)); l = 150
        seq = bytes(rng.integers(0, 256, (l + 1) // 2, dtype=np.uint8)); qual = bytes(rng.integers(2, 41, l, dtype=np.uint8))
        body = struct.pack("<iiBBHHHiiii", 0, int(rng.integers(0, 10 ** 7)), len(name), 60, 0, 1, 99, l, 0, 0, 300) + name + struct.pack("<I", (l << 4)) + seq + qual + b"ASC\x64NMC\x01"
        out += struct.pack("<i", len(body)) + body
    return bytes(out[:n])


def mixed(n, seed):
    """text-like bytes with repeats: literals and matches at many distances"""
    rng = np.random.default_rng(seed); words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + b" "
    return bytes(out[:n])


# ---------------------------------------------------------------------------------------------- the vectors
def valid_vectors():
    v = []
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 63, 64, 65, 257, 258, 259, 4095, 65535, 65536):
        data = mixed(n, n)
        for level in (0, 1, 6, 9):
            v.append(("mixed_%d_l%d" % (n, level), deflate(data, level), data))
    big = mixed(30000, 7)
    for nm, st in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        v.append(("strategy_" + nm, deflate(big, 6, st), big))
        v.append(("strategy_%s_bam" % nm, deflate(bam_like(20000), 6, st), bam_like(20000)))
    fib = fibonacci_payload()
    v.append(("fibonacci_15bit", deflate(fib, 6, zlib.Z_HUFFMAN_ONLY), fib))
    for nm, fl in (("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH)):
        co = zlib.compressobj(6, zlib.DEFLATED, -15); s = b""
        parts = [mixed(5000, 11), b"", bam_like(7000, 4), mixed(300, 12)]
        for p in parts:
            s += co.compress(p) + co.flush(fl)
        s += co.flush()
        v.append(("flush_" + nm, s, b"".join(parts)))
    zeros = bytes(65536)
    v.append(("zeros_rle", deflate(zeros, 6, zlib.Z_RLE), zeros))
    v.append(("zeros_l9", deflate(zeros, 9), zeros))
    noise = bytes(rng.integers(0, 256, 65536, dtype=np.uint8))
    v.append(("noise_l0", deflate(noise, 0), noise))
    v.append(("noise_l6", deflate(noise, 6), noise))
    bl = bam_like(65280)
    v.append(("bam_like", deflate(bl, 6), bl))
    v.append(("trailing_garbage", deflate(big, 6) + bytes(rng.integers(0, 256, 37, dtype=np.uint8)), big))

    # ---- streams zlib never writes
    half = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    toks = []
    left = 32768
    while left:
        n = min(258, left)
        if left - n in (1, 2):
            n -= 3
        toks.append((n, 32768)); left -= n
    w = stored_block(half, final=False); fixed_block(toks, w=w)
    v.append(("distance_32768", w.done(), half + half))
    v.append(("distance_equals_produced", fixed_block([65, 66, 67, (3, 3), (6, 6), (12, 12), 68, (25, 25)]).done(), None))
    # one distance code of one bit: literals a, b, then matches at distance 1 (distance symbol 0 = the code "0")
    ll = [0] * 286
    for s, l in ((97, 2), (98, 2), (256, 2), (257, 3), (285, 3)):
        ll[s] = l
    v.append(("one_distance_code", dynamic_block(ll, [1], [97, 98, (3, 1), 97, (258, 1), (3, 1)]).done(), None))
    v.append(("literals_only", dynamic_block(lit_only_lengths(b"hello world"), [0], list(b"hello world hello")).done(), None))
    # Code-length repeats that cross from the literal/length lengths into the distance lengths (RFC 3.2.7: "the code length repeat codes can cross from HLIT + 257
    # to the HDIST + 1 code lengths").  Literals 1..63 have 7 bits, symbols 129..258 (literals, end-of-block, lengths 3 and 4) have 8 bits: a complete code.  The run
    # of eights is sent as "8" + repeats that end three lengths into the distance alphabet, whose lengths are 8, 8, 8, 1, 2, 3, 4, 5, 6, 8 (complete as well).
    ll = [0] + [7] * 63 + [0] * 65 + [8] * 130
    dl = [8, 8, 8, 1, 2, 3, 4, 5, 6, 8]
    cl_syms = [0, 7] + [(16, 3)] * 9 + [(16, 2), (16, 0)] + [(18, 65 - 11)] + [8] + [(16, 3)] * 22 + [1, 2, 3, 4, 5, 6, 8]
    assert expand_cl(cl_syms) == ll + dl and len(ll) == 259
    w = BitWriter(); dynamic_header(w, 259, len(dl), FLAT_CL, cl_syms, True)
    put_tokens(w, [1, 2, 3, 200, 201, (3, 4), 63, (4, 2), 255, (4, 11)], canonical(ll), canonical(dl))
    v.append(("repeat_crosses_boundary", w.done(), None))
    for n in (65, 129):
        toks = [10, 20, 30, 40, 50, 60, 70] + [(3 + (i % 40), 1 + (i * 5) % 7) for i in range(n)]
        v.append(("matches_%d" % n, fixed_block(toks).done(), None))
    out = []
    for name, stream, data in v:
        z, err = zlib_inflate(stream)
        assert err is None, (name, err)
        if data is not None:
            assert z == data, name
        out.append((name, stream, len(z), z))
    return out


def malformed_vectors():
    """(name, stream, isize, None, expected status or None)"""
    m = []
    w = BitWriter(); w.bits(1, 1); w.bits(3, 2); w.bits(0, 13)
    m.append(("reserved_btype", w.done(), 10, RESERVED_BTYPE))
    m.append(("len_nlen_mismatch", stored_block(b"abcdef", nlen=0x1234).done(), 6, STORED_LEN))
    # code length code over-subscribed: three codes of 1 bit
    w = BitWriter(); dynamic_header(w, 257, 1, [1, 1, 1] + [0] * 16, [], True); w.bits(0, 64)
    m.append(("cl_code_oversubscribed", w.done(), 4, BAD_CODE))
    w = BitWriter(); dynamic_header(w, 257, 1, [2, 2, 2] + [0] * 16, [], True); w.bits(0, 64)
    m.append(("cl_code_incomplete", w.done(), 4, BAD_CODE))
    ll = [0] * 257
    ll[97] = 1; ll[98] = 1; ll[256] = 1
    m.append(("lit_code_oversubscribed", dynamic_block(ll, [1], None).done() + bytes(8), 4, BAD_CODE))
    ll = [0] * 257
    ll[97] = 2; ll[98] = 2; ll[256] = 2
    m.append(("lit_code_incomplete", dynamic_block(ll, [1], None).done() + bytes(8), 4, BAD_CODE))
    ll = [0] * 257
    ll[97] = 1; ll[256] = 1
    m.append(("dist_code_incomplete", dynamic_block(ll, [2, 2, 2], None).done() + bytes(8), 4, BAD_CODE))
    m.append(("dist_code_oversubscribed", dynamic_block(ll, [1, 1, 1], None).done() + bytes(8), 4, BAD_CODE))
    ll = [0] * 257
    ll[97] = 1; ll[98] = 1                                              # complete, but no end-of-block code
    m.append(("no_end_of_block", dynamic_block(ll, [1], None).done() + bytes(8), 4, BAD_CODE))
    w = BitWriter(); dynamic_header(w, 257, 1, FLAT_CL, [(16, 0), 1, 1], True); w.bits(0, 64)
    m.append(("repeat_16_first", w.done(), 4, BAD_CODE))
    w = BitWriter(); w.bits(1, 1); w.bits(2, 2); w.bits(30, 5); w.bits(0, 5); w.bits(15, 4); w.bits(0, 200)        # HLIT = 287
    m.append(("hlit_287", w.done(), 4, BAD_CODE))
    w = BitWriter(); w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(30, 5); w.bits(15, 4); w.bits(0, 200)        # HDIST = 31
    m.append(("hdist_31", w.done(), 4, BAD_CODE))
    w = BitWriter(); dynamic_header(w, 257, 1, FLAT_CL, [1, 1] + [(18, 127)] * 3, True); w.bits(0, 64)      # a repeat beyond HLIT + HDIST
    m.append(("repeat_past_the_end", w.done(), 4, BAD_CODE))
    m.append(("symbol_286", fixed_block([97, ("sym", 286)]).done(), 1, BAD_SYMBOL))
    m.append(("distance_symbol_30", fixed_block([97, 98, 99, ("dsym", 3, 30)]).done(), 6, BAD_SYMBOL))
    m.append(("distance_too_far", fixed_block([97, 98, 99, (3, 4)]).done(), 6, FAR_DISTANCE))
    m.append(("distance_too_far_first", fixed_block([(3, 1)]).done(), 3, FAR_DISTANCE))
    good = fixed_block(list(b"abcabc") + [(10, 3)]).done()
    m.append(("one_byte_more", good, 15, OUTPUT_SIZE))
    m.append(("one_byte_less", good, 17, OUTPUT_SIZE))
    m.append(("literal_past_isize", fixed_block(list(b"abcd")).done(), 3, OUTPUT_SIZE))
    m.append(("stored_past_isize", stored_block(b"abcdef").done(), 5, OUTPUT_SIZE))
    m.append(("stored_truncated", stored_block(b"abcdef").done()[:8], 6, INPUT_EXHAUSTED))
    m.append(("empty_stream", b"", 0, INPUT_EXHAUSTED))
    m.append(("no_final_block", fixed_block(list(b"abc"), final=False).done(), 3, INPUT_EXHAUSTED))
    # one unused 1-bit distance pattern: the code "1" of a distance code that only has "0"
    ll = [0] * 286
    for s, l in ((97, 2), (98, 2), (256, 2), (257, 3), (285, 3)):
        ll[s] = l
    w = BitWriter(); dynamic_header(w, 286, 1, FLAT_CL, ll + [1], True)
    lit = canonical(ll); w.code(*lit[97]); w.code(*lit[257]); w.bits(1, 1); w.code(*lit[256])
    m.append(("unused_distance_code", w.done(), 4, BAD_SYMBOL))
    # a match in a block without distance codes
    ll2 = list(ll)
    w = BitWriter(); dynamic_header(w, 286, 1, FLAT_CL, ll2 + [0], True)
    w.code(*lit[97]); w.code(*lit[257]); w.bits(0, 1); w.code(*lit[256])
    m.append(("match_without_distance_code", w.done(), 4, BAD_SYMBOL))
    out = []
    for name, stream, isize, status in m:
        z, err = zlib_inflate(stream)
        assert err is not None or len(z) != isize, (name, "zlib accepts this stream with exactly isize bytes")
        out.append((name, stream, isize, None, status))
    return out


def truncation_vectors():
    """a small stream of mixed content cut at every byte"""
    data = mixed(150, 21)
    s = deflate(data, 6)
    assert zlib_inflate(s)[0] == data
    return [("truncated_%d" % k, s[:k], len(data), None, None) for k in range(len(s))]


def flip_stream():
    """about 60 bytes of mixed content: a fixed block, a stored block and a dynamic block in one stream"""
    w = fixed_block(list(b"abcab") + [(4, 3), 120] + list(b"wxyz") + [(5, 9)], final=False)
    stored_block(b"STORED BYTES", final=False, w=w)
    ll = [0] * 286
    for s, l in ((97, 3), (98, 3), (99, 3), (100, 3), (101, 3), (256, 3), (257, 3), (258, 4), (285, 4)):
        ll[s] = l
    dynamic_block(ll, [2, 2, 2, 2], [97, 98, 99, (3, 2), 100, (4, 4), 101, (258, 3), 99, 98], w=w, compact=True)
    s = w.done()
    z, err = zlib_inflate(s)
    assert err is None
    return s, z
