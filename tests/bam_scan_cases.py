"""Inputs and expectations of the BAM record pass (hla-la_amd/csrc/bam_scan_core.h; hlala_host_bam_scan_model on the host, hlala_bam_scan on the device).

Records are those of test_bam.make_records, serialised as test_bam.write_bam serialises them (plus a few more tag types and the hooks the malformed inputs need).
The expectation -- descriptors, compact bytes, examined, consumed, the first failing record -- is written out here from the RECORD LIST, with the rules of the
host decoder in plain Python: it never looks at the serialised bytes it did not build itself.

Decoys are bytes inside a record that look like records: a chain of three fake records (37 bytes each) in the qualities or in a B tag, placed so that the chain begins
exactly on a slice start while the true entry of that slice lies behind it.  With slices of 64 bytes three fakes (111 bytes) cover the slice, so there the chain is one
fake whose length leads to the next TRUE record (one fake + two true records make the three).  A Z tag cannot hold a zero byte, so its decoy is one fake record of
non-zero bytes whose length reaches beyond the buffer: the chain 'passes with the records that fit'."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from conftest import load_package
from test_bam import INT_FMT, OPS, SEQ16, make_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_LENGTH, CORRUPT_RECORD, CORRUPT_TAG, UNKNOWN_TAG_TYPE, NO_AS, UNPAIRED, TOO_MANY_REHOPS = range(8)
E_ARG, E_CAPACITY = -1, -4
CANARY = 0xC3
GUARD = 64
INTERVALS = [("chr6", 10000, 20000, 0), ("HLA-A*01", 0, 3999, 1), ("chr6", 19000, 30000, 2)]      # overlapping intervals: a record can be taken twice
STAT_FIELDS = ("n_records", "n_kept", "n_recs", "examined", "consumed", "compact_bytes", "status", "status_record", "n_slices", "n_rehops")
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------- serialisation
def tag_bytes(tags):
    out = b""
    for tag, ty, v in tags:
        if ty == "raw":
            out += v                                               # bytes as they are (malformed tags)
        elif ty in INT_FMT:
            out += tag.encode() + ty.encode() + struct.pack(INT_FMT[ty], v)
        elif ty in "ZH":
            out += tag.encode() + ty.encode() + (v if isinstance(v, bytes) else v.encode()) + b"\0"
        elif ty == "A":
            out += tag.encode() + b"A" + v.encode()
        elif ty == "f":
            out += tag.encode() + b"f" + struct.pack("<f", v)
        elif ty == "B":                                            # v = (element type, bytes of the elements)
            et, payload = v
            es = {"c": 1, "C": 1, "s": 2, "S": 2}.get(et, 4)
            assert len(payload) % es == 0
            out += tag.encode() + b"B" + et.encode() + struct.pack("<I", len(payload) // es) + payload
        else:
            raise ValueError(ty)
    return out


def record_body(r):
    """the record behind its length field, as test_bam.write_bam writes it; r['corrupt'] in (None, 'l_seq', 'otags', 'l_read_name') damages the fixed part"""
    name = r["name"].encode() + b"\0"; cig = b"".join(struct.pack("<I", (l << 4) | OPS.index(o)) for l, o in r["cigar"])
    seq = r["seq"]; packed = bytearray((len(seq) + 1) // 2)
    for i, ch in enumerate(seq):
        packed[i // 2] |= SEQ16.index(ch) << (4 if i % 2 == 0 else 0)
    l_seq, l_name = len(seq), len(name)
    c = r.get("corrupt")
    if c == "l_seq":
        l_seq = -5
    elif c == "otags":
        l_seq += 100000
    elif c == "l_read_name":
        l_name = 0
    return struct.pack("<iiBBHHHiiii", r["ref"], r["pos"], l_name, r.get("mapq", 60), 0, len(r["cigar"]), r["flag"], l_seq, r.get("next_ref", -1), r.get("next_pos", -1), 0) \
        + name + cig + bytes(packed) + bytes(r["qual"]) + tag_bytes(r.get("tags", []))


def header(refs):
    raw = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", len(refs))
    for nm, ln in refs:
        raw += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    return raw


def serialise(records, prefix=b""):
    """(bytes, offset of every record's length field)"""
    parts = [prefix]; at = len(prefix); starts = []
    for r in records:
        b = record_body(r)
        starts.append(at); parts.append(struct.pack("<i", len(b)) + b); at += 4 + len(b)
    return b"".join(parts), starts


def write_bam_file(path, refs, records, block=3000):
    """the records behind the header of `refs`, in BGZF blocks cut every `block` bytes (test_bam.write_bam, with the tag types and hooks of record_body)"""
    from test_bam import bgzf_block
    raw = serialise(records, header(refs))[0]
    with open(path, "wb") as f:
        for i in range(0, len(raw), block):
            f.write(bgzf_block(raw[i:i + block]))
        f.write(bgzf_block(b""))


def ref_intervals_of(refs, intervals=INTERVALS):
    """per reference id the numbers of its intervals, in interval order (the decoder's intervalsOfRef)"""
    return [[i for i, iv in enumerate(intervals) if iv[0] == nm] for nm, _ in refs]


# ---------------------------------------------------------------------------------------------------------------- the expectation
def hash_name(b):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & M64
    h ^= h >> 29; h = (h * 0xbf58476d1ce4e5b9) & M64; h ^= h >> 32
    return h


def expect(records, refs, long_mode=False, hash_mask=M64, first_seq=0, intervals=INTERVALS):
    """dict(recs = structured array, compact = bytes, examined, n_kept, fail = (status, record) or None) from the record list.  A record may carry
    tag_status: the status its tags give once they are walked (CORRUPT_TAG / UNKNOWN_TAG_TYPE: the malformed tag stands before any AS)."""
    pkg = load_package()
    riv = ref_intervals_of(refs, intervals)
    out = []; compact = b""; examined = 0; kept = 0; fail = None
    for ri, r in enumerate(records):
        try:
            if r.get("corrupt"):
                raise ValueError(CORRUPT_RECORD)
            fl = r["flag"]
            if fl & 4 or (long_mode and fl & 256) or r["ref"] < 0 or r["ref"] >= len(refs):
                continue
            mine = []; ex = 0; walked = None
            for rank, ii in enumerate(riv[r["ref"]]):
                _, a, b, contig = intervals[ii]
                ex += 1
                if not r["cigar"]:
                    continue
                stop = r["pos"] + sum(l for l, o in r["cigar"] if o in "MDN=X") - 1
                if not (a <= r["pos"] <= b and a <= stop <= b):
                    continue
                if not long_mode and not fl & 1:
                    raise ValueError(UNPAIRED)
                if walked is None:
                    if r.get("tag_status"):
                        raise ValueError(r["tag_status"])
                    AS = [v for t, ty, v in r["tags"] if t == "AS" and ty in INT_FMT]
                    if not AS:
                        raise ValueError(NO_AS)
                    walked = AS[0]
                primary = not fl & 256
                mine.append((hash_name(r["name"].encode()) & hash_mask, ((first_seq + ri) << 8) | min(len(mine), 255), len(compact), contig, r["pos"] - a, walked, len(r["seq"]) if primary else 0,
                             len(r["cigar"]), len(r["name"]), 0 if long_mode else (0 if fl & 64 else 1), (1 if fl & 16 else 0) | (2 if primary else 0), len(r["name"]) + 1, 0))
            examined += ex
            if mine:
                kept += 1; out += mine
                body = record_body(r)
                compact += body[:32 + len(r["name"]) + 1 + 4 * len(r["cigar"]) + (len(r["seq"]) + 1) // 2 + len(r["seq"])]
        except ValueError as e:
            if fail is None:
                fail = (e.args[0], ri)
    return dict(recs=np.array(out, dtype=pkg.BAM_REC_DTYPE), compact=compact, examined=examined, n_kept=kept, fail=fail)


# ---------------------------------------------------------------------------------------------------------------- inputs
def fake_chain(k, tail):
    """k fake records of 37 bytes; the last one's length leads `tail` bytes beyond the chain (to the next true record)"""
    out = b""
    for i in range(k):
        out += struct.pack("<iiiBBHHHiiii", 33 + (tail if i == k - 1 else 0), -1, -1, 1, 0, 0, 0, 4, 0, -1, -1, 0) + b"\0"
    assert len(out) == 37 * k
    return out


Z_FAKE = bytes([1, 1, 1, 0x0F]) + b"\xff" * 4 + b"\x01" * 4 + bytes([2, 1, 1, 1, 1, 1, 1, 1]) + b"\x01" * 4 + b"\xff" * 4 + b"\x01" * 8 + b"x"      # 36 bytes of header + 1 of name; the Z tag's NUL ends the name


def plain(name, pos=12000, flag=1 | 64, ref=0, L=50, tags=None, **kw):
    return dict(name=name, flag=flag, ref=ref, pos=pos, cigar=[(L, "M")], seq="ACGT" * (L // 4) + "A" * (L % 4), qual=[30] * L, tags=[("AS", "C", 40)] if tags is None else tags, **kw)


def decoy_input(kind, S, refs, rng, prefix=b""):
    """(records, data, decoy offset): a few records, the carrier of the decoy (kind: 'qual', 'B', 'Z'), a few more.  The decoy starts on a multiple of S inside the carrier and
    the carrier ends less than S bytes later, so that slice's true entry is the record behind the carrier."""
    _, some = make_records(rng, n_names=6)
    before, after = some[:len(some) // 2], some[len(some) // 2:]
    k = 1 if S < 256 else 3
    base = len(serialise(before, prefix)[0])

    def carrier(pad):
        if kind == "qual":
            decoy = fake_chain(k, 4)                                                        # behind the qualities: AS:C:40, four bytes
            L = pad + len(decoy)
            r = dict(name="carrier", flag=1 | 64, ref=0, pos=12000, cigar=[(L, "M")], seq="A" * L, qual=[33] * pad + list(decoy), tags=[("AS", "C", 40)])
        elif kind == "B":
            decoy = fake_chain(k, 0)
            r = plain("carrier", tags=[("AS", "C", 40), ("XB", "B", ("C", b"\x07" * pad + decoy))])
        else:
            decoy = Z_FAKE
            r = plain("carrier", tags=[("AS", "C", 40), ("XZ", "Z", b"z" * pad + decoy)])
        return r, record_body(r).rindex(decoy)
    _, off0 = carrier(0)
    D = 37 * k
    # where the decoy lands with `pad` bytes in front of it: for the qualities the packed bases in front of them grow with the read as well
    where = (lambda pad: off0 - (D + 1) // 2 + (pad + D + 1) // 2 + pad) if kind == "qual" else (lambda pad: off0 + pad)
    pad = next(p for p in range(1, 4 * S) if (base + 4 + where(p)) % S == 0)
    r, off = carrier(pad)
    assert off == where(pad) and (base + 4 + off) % S == 0, (kind, S)
    records = before + [r] + after
    data, starts = serialise(records, prefix)
    return records, data, base + 4 + off


def aligned_implausible(S, refs, rng, prefix=b""):
    """a TRUE record that bam_plausible rejects (next_refID >= n_ref), starting exactly on a multiple of S: the record before it is padded with a Z tag behind its AS"""
    _, some = make_records(rng, n_names=5)
    base = len(serialise(some, prefix)[0])
    filler0 = plain("filler", tags=[("AS", "C", 40), ("XZ", "Z", b"")])
    pad = (-(base + 4 + len(record_body(filler0)))) % S
    filler = plain("filler", tags=[("AS", "C", 40), ("XZ", "Z", b"p" * pad)])
    odd = plain("odd", pos=12500, flag=1 | 128, next_ref=len(refs) + 4)
    records = some + [filler, odd] + some[:3]
    data, starts = serialise(records, prefix)
    assert starts[len(some) + 1] % S == 0
    return records, data


def corruptions():
    """{name: (records, status, failing record)}: each alone, in the middle of ordinary records (record 2 of 5)"""
    def around(r):
        return [plain("a"), plain("b", flag=1 | 128), r, plain("c"), plain("d", flag=1 | 128)]
    return {
        "otags": (around(plain("x", corrupt="otags")), CORRUPT_RECORD, 2),
        "l_seq": (around(plain("x", corrupt="l_seq")), CORRUPT_RECORD, 2),
        "l_read_name": (around(plain("x", corrupt="l_read_name")), CORRUPT_RECORD, 2),
        "corrupt_unmapped": (around(plain("x", flag=1 | 4, corrupt="l_seq")), CORRUPT_RECORD, 2),                       # before any filter
        "unknown_tag": (around(plain("x", tags=[("NM", "C", 1), ("XQ", "raw", b"XQ?\x01"), ("AS", "C", 40)], tag_status=UNKNOWN_TAG_TYPE)), UNKNOWN_TAG_TYPE, 2),
        "tag_runs_off": (around(plain("x", tags=[("NM", "C", 1), ("XY", "raw", b"XYi\x01")], tag_status=CORRUPT_TAG)), CORRUPT_TAG, 2),
        "b_tag_runs_off": (around(plain("x", tags=[("XB", "raw", b"XBBi\xff\xff\xff\x7f")], tag_status=CORRUPT_TAG)), CORRUPT_TAG, 2),
        "b_tag_cut": (around(plain("x", tags=[("XB", "raw", b"XBBi\x01")], tag_status=CORRUPT_TAG)), CORRUPT_TAG, 2),
        "z_tag_open": (around(plain("x", tags=[("XZ", "raw", b"XZZabc")], tag_status=CORRUPT_TAG)), CORRUPT_TAG, 2),
        "no_as": (around(plain("x", tags=[("NM", "C", 0), ("AS", "Z", "text"), ("XS", "f", 1.5), ("XA", "A", "q")])), NO_AS, 2),
        "unpaired": (around(plain("x", flag=0)), UNPAIRED, 2),
    }


# ---------------------------------------------------------------------------------------------------------------- running the model
def load_model():
    pkg = load_package()
    so = os.environ.get("HLALA_HOST_LIB") or os.path.join(ROOT, "hla-la_amd", "libhlala_host.so")
    src = os.path.join(ROOT, "hla-la_amd", "csrc")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(os.path.join(src, f)) for f in ("bam_scan_core.h", "bam_scan_model.h", "host_check.cpp")):
        subprocess.check_call(["make", "-C", src, "../libhlala_host.so"])
    lib = C.CDLL(so)
    lib.hlala_host_bam_scan_model.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32, C.POINTER(pkg.BamScanIn), C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.POINTER(pkg.BamScanStats)]
    lib.hlala_host_bam_scan_model.restype = C.c_int
    return lib


def scan_args(refs, long_mode=False, hash_mask=M64, first_seq=0, slice_bytes=0, max_rehops=None, intervals=INTERVALS):
    pkg = load_package()
    return pkg.bam_scan_in(len(refs), ref_intervals_of(refs, intervals), [iv[1:] for iv in intervals], long_mode, hash_mask, first_seq, slice_bytes, max_rehops)


def stats_dict(st):
    return {k: int(getattr(st, k)) for k in STAT_FIELDS}


def caps(data, n_intervals=len(INTERVALS)):
    return len(data) // 36 * max(1, n_intervals), len(data)


def run_model(lib, data, args, first=0, last=False, cap_recs=None, cap_compact=None):
    """(rc, descriptors, compact bytes, stats dict): data in an exactly-sized buffer, both outputs between canaries, which must survive; with a status other than OK
    (or a return code other than 0) nothing may have been written at all"""
    pkg = load_package()
    a, keep = args
    buf = np.frombuffer(bytes(data), np.uint8).copy() if len(data) else np.zeros(0, np.uint8)
    cr, cc = caps(data, a.n_intervals)
    cr = cr if cap_recs is None else cap_recs; cc = cc if cap_compact is None else cap_compact
    recs = np.full(2 * GUARD + cr * pkg.BAM_REC_DTYPE.itemsize, CANARY, np.uint8); comp = np.full(2 * GUARD + cc, CANARY, np.uint8)
    st = pkg.BamScanStats()
    rc = lib.hlala_host_bam_scan_model(buf.ctypes.data if buf.size else None, buf.size, first, int(bool(last)), C.byref(a), recs.ctypes.data + GUARD, cr, comp.ctypes.data + GUARD, cc, C.byref(st))
    return (rc,) + check_outputs(rc, recs, comp, st)


def check_outputs(rc, recs, comp, st):
    """canaries around (and, where nothing may be written, all over) the two output arrays of a call made with GUARD; returns (descriptors, compact bytes, stats dict)"""
    pkg = load_package()
    ok = rc == 0 and st.status == OK
    nr = st.n_recs * pkg.BAM_REC_DTYPE.itemsize if ok else 0; ncb = st.compact_bytes if ok else 0
    assert (recs[:GUARD] == CANARY).all() and (recs[GUARD + nr:] == CANARY).all(), "descriptors written outside [0, n_recs)"
    assert (comp[:GUARD] == CANARY).all() and (comp[GUARD + ncb:] == CANARY).all(), "compact bytes written outside [0, compact_bytes)"
    return recs[GUARD:GUARD + nr].copy().view(pkg.BAM_REC_DTYPE), comp[GUARD:GUARD + ncb].tobytes(), stats_dict(st)


def assert_equals_expectation(got, exp, data, n_records, consumed, S, first_seq=0):
    rc, recs, comp, st = got
    assert rc == 0 and st["status"] == OK and st["status_record"] == -1, st
    assert st["n_records"] == n_records and st["consumed"] == consumed and st["n_slices"] == (len(data) + S - 1) // S, st
    assert st["examined"] == exp["examined"] and st["n_kept"] == exp["n_kept"] and st["n_recs"] == len(exp["recs"]) and st["compact_bytes"] == len(exp["compact"]), st
    assert recs.tobytes() == exp["recs"].tobytes()
    assert comp == exp["compact"]
    assert (np.diff(recs["order"].astype(np.int64)) >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- the cases both suites run
def valid_cases():
    """[(name, records, data, first, refs, kwargs of scan_args)] -- every one must scan to its expectation at every slice size"""
    out = []
    refs, recs = make_records(np.random.default_rng(21), n_names=40, lengths=(149, 150, 151, 97))
    h = header(refs)
    out.append(("plain", recs, serialise(recs)[0], 0, refs, {}))
    out.append(("behind_header", recs, serialise(recs, h)[0], len(h), refs, {}))
    out.append(("long_mode_masked", recs, serialise(recs, b"\x07" * 3)[0], 3, refs, dict(long_mode=True, hash_mask=(0xFF << 56) | 0xF, first_seq=(1 << 40) + 5)))
    for k in (0, 1, 64, 65):
        out.append(("n%d" % k, recs[:k], serialise(recs[:k], h)[0], len(h), refs, {}))
    rng = np.random.default_rng(22)
    longs = []
    for i, L in enumerate((20000, 70000, 33333, 66000)):
        seq = "".join("ACGT"[j] for j in rng.integers(0, 4, L))
        longs.append(dict(name="long%d" % i, flag=0 if i % 2 else 16, ref=0, pos=10000, cigar=[(2000 + i, "M"), (L - 2000 - i, "S")], seq=seq, qual=[int(q) for q in rng.integers(2, 41, L)],
                          tags=[("NM", "i", 5), ("AS", "i", 1000 + i)]))
    out.append(("long_reads", longs + recs[:4], serialise(longs + recs[:4], h)[0], len(h), refs, dict(long_mode=True)))
    return out


def random_buffers():
    """300 buffers of random bytes, a third of them with a plausible length in front"""
    rng = np.random.default_rng(23); out = []
    for i in range(300):
        b = bytearray(rng.integers(0, 256, int(rng.integers(0, 400)), dtype=np.uint8).tobytes())
        if i % 3 == 0 and len(b) >= 4:
            b[:4] = struct.pack("<i", int(rng.integers(32, 120)))
        out.append(bytes(b))
    return out


def byte_changes():
    """every single-byte change (three values each) of the first 200 bytes of a small valid buffer"""
    refs, recs = make_records(np.random.default_rng(24), n_names=3)
    data = serialise(recs[:6])[0]
    assert len(data) > 400
    out = []
    for i in range(200):
        for v in (0x00, 0xFF, data[i] ^ 0x10):
            if v != data[i]:
                b = bytearray(data); b[i] = v; out.append(bytes(b))
    return refs, data, out
