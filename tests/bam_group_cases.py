"""Descriptor arrays for the grouping stage (hlala_bam_group / hlala_host_bam_group_model), the expectation written from the record list, and the model's binding.
Shared by tests/test_bam_group_model.py (CPU) and tests/test_gpu_bam_group.py: the device is handed exactly what the model has been shown to take."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np

from conftest import ROOT, load_package

M64 = (1 << 64) - 1
TOP_BYTE = 0xFF << 56
START, COLLIDED, COMPLETE = 1, 2, 4
COUNT_FIELDS = ("n_recs", "n_runs", "n_collided_runs", "n_units_complete", "n_units_incomplete")
E_ARG, E_DEVICE = -1, -2


def hash_name(name: bytes, mask=M64):
    """host_bam.cpp: hash_name"""
    h = 0xcbf29ce484222325
    for b in name:
        h = ((h ^ b) * 0x100000001b3) & M64
    h ^= h >> 29; h = (h * 0xbf58476d1ce4e5b9) & M64; h ^= h >> 32
    return h & mask


def build(items, mask=M64, align=None, seed=1):
    """items: [dict(name=bytes, which=0|1, primary=bool, copies=k (descriptors of this one record: intervals), hash=int or None)] in file order.
    Returns (descriptors, bytes): every record gets 32 bytes of noise, its name and a NUL at a rec_off with rec_off % 16 == align (None: whatever comes)."""
    pkg = load_package()
    rng = np.random.default_rng(seed)
    n = sum(it.get("copies", 1) for it in items)
    recs = np.zeros(n, pkg.BAM_REC_DTYPE)
    buf = bytearray(rng.integers(1, 255, int(rng.integers(0, 7)), dtype=np.uint8).tobytes())
    k = 0
    for seq, it in enumerate(items):
        if align is not None:
            a = align(seq) if callable(align) else align
            while len(buf) % 16 != a:
                buf.append(0x5A)
        off = len(buf)
        name = it["name"]
        buf += rng.integers(0, 256, 32, dtype=np.uint8).tobytes() + name + b"\0"
        h = it.get("hash")
        h = hash_name(name, mask) if h is None else h
        for rank in range(it.get("copies", 1)):
            r = recs[k]; k += 1
            r["hash"] = h; r["order"] = (seq << 8) | min(rank, 255); r["rec_off"] = off; r["contig"] = rank; r["pos"] = seq; r["as"] = 40; r["l_seq"] = 100 if it.get("primary", True) else 0
            r["n_cigar"] = 1; r["nameLen"] = len(name); r["which"] = it.get("which", 0); r["flags"] = 2 if it.get("primary", True) else 0; r["l_read_name"] = min(255, len(name) + 1)
    return recs, np.frombuffer(bytes(buf), np.uint8).copy()


def name_of(recs, data, i):
    o = int(recs["rec_off"][i]) + 32
    return bytes(data[o:o + int(recs["nameLen"][i])])


def expect(recs, data, long_mode):
    """(perm, flag, counts) from the descriptor list: sort by (hash, order), split by hash, compare names"""
    n = len(recs)
    perm = sorted(range(n), key=lambda i: (int(recs["hash"][i]), i))          # (ascending order: the index is the order)
    flag = np.zeros(n, np.uint8)
    runs = collided = complete = incomplete = 0
    i = 0
    while i < n:
        j = i + 1
        while j < n and recs["hash"][perm[j]] == recs["hash"][perm[i]]:
            j += 1
        runs += 1
        names = {name_of(recs, data, perm[k]) for k in range(i, j)}
        if len(names) > 1:
            flag[i] = START | COLLIDED; collided += 1
        else:
            prim = {int(recs["which"][perm[k]]) for k in range(i, j) if recs["flags"][perm[k]] & 2}
            ok = (0 in prim) if long_mode else (0 in prim and 1 in prim)
            flag[i] = START | (COMPLETE if ok else 0)
            complete += ok; incomplete += not ok
        i = j
    return np.array(perm, np.uint32), flag, dict(n_recs=n, n_runs=runs, n_collided_runs=collided, n_units_complete=int(complete), n_units_incomplete=int(incomplete))


def pair(name, **kw):
    return [dict(name=name, which=0, **kw), dict(name=name, which=1, **kw)]


def random_names(rng, k, lo=8, hi=40):
    out, seen = [], set()
    while len(out) < k:
        nm = bytes(rng.integers(33, 127, int(rng.integers(lo, hi + 1)), dtype=np.uint8))
        if nm not in seen:
            seen.add(nm); out.append(nm)
    return out


def sized(n, seed):
    """n descriptors: pairs with an occasional secondary, shuffled as a coordinate-sorted file would have them"""
    rng = np.random.default_rng(seed)
    items = []
    for nm in random_names(rng, n // 2 + 1):
        items += pair(nm)
        if rng.random() < 0.2:
            items.append(dict(name=nm, which=int(rng.integers(0, 2)), primary=False))
    items = [items[i] for i in rng.permutation(len(items))][:n]
    return items


def cases():
    """name -> (items, kwargs of build)"""
    rng = np.random.default_rng(77)
    out = {}
    for n in (0, 1, 2, 63, 64, 65, 4097):
        out[f"n{n}"] = (sized(n, 100 + n), {})
    out["name_lengths"] = ([x for L in (1, 15, 16, 17, 254) for nm in random_names(rng, 3, L, L) for x in pair(nm)], {})
    base = random_names(rng, 6, 9, 33)
    last_byte = [x for nm in base for x in pair(nm + b"A") + pair(nm + b"B")]
    out["last_byte_full_hash"] = (last_byte, {})
    out["last_byte_same_hash"] = (last_byte, dict(mask=0))                       # collided runs whose names differ in the last byte (8-byte steps and the tail)
    out["prefix_same_hash"] = (pair(b"read/1") + pair(b"read/12") + pair(b"read/123456789012345") + pair(b"read/1234567890123456"), dict(mask=0))
    out["every_alignment"] = ([x for k in range(32) for x in pair(b"aligned-name-%02d-xyzw" % k)], dict(align=lambda seq: seq % 16))
    out["every_alignment_collided"] = ([x for k in range(32) for x in pair(b"aligned-name-%02d-xyzw" % (k // 2))], dict(align=lambda seq: (seq * 7) % 16, mask=0))
    out["three_intervals"] = (pair(b"before") + [dict(name=b"thrice", which=0, copies=3), dict(name=b"thrice", which=1, copies=3)] + pair(b"after"), {})
    combos = []
    kinds = [(0, True), (0, False), (1, True), (1, False)]
    for k, sub in enumerate(s for r in range(1, 5) for s in itertools.combinations(kinds, r)):
        combos += [dict(name=b"combo-%02d" % k, which=w, primary=p) for (w, p) in sub]
    out["primary_secondary_mates"] = (combos, {})
    out["collided_2"] = (pair(b"keep") + [dict(name=b"x1", which=0, hash=5 << 56), dict(name=b"x2", which=1, hash=5 << 56)], {})
    out["collided_aba"] = ([dict(name=b"A-name", which=0, hash=9), dict(name=b"B-name", which=0, hash=9), dict(name=b"A-name", which=1, hash=9)] + pair(b"other"), {})
    big = [x for nm in random_names(rng, 2502) for x in pair(nm, hash=0x37 << 56)]
    out["collided_5004"] = (pair(b"lower", hash=0x36 << 56) + big + pair(b"upper", hash=0x38 << 56), {})          # one whole partition as hash_mask = the top byte makes it
    # clean runs longer than a wavefront: the only primaries at the far ends, and one foreign name as the very last record of a run of 200
    long_run = [dict(name=b"long-clean", which=0, primary=False)] * 150 + [dict(name=b"long-clean", which=1, primary=True)]
    long_run = [dict(name=b"long-clean", which=0, primary=True)] + long_run
    half = [dict(name=b"long-half", which=0, primary=(k == 70)) for k in range(141)]
    tail = [dict(name=b"long-tail", which=k & 1, hash=77) for k in range(199)] + [dict(name=b"long-tail-other", which=0, hash=77)]
    out["runs_across_wavefronts"] = (sized(37, 5) + long_run + half + tail + sized(11, 6), {})
    out["rounds"] = (sized(1 + 63 + 65 + 2000, 9), {})
    return out


ROUNDS = (1, 63, 65, 2000)


def built_cases():
    return {k: build(items, **kw) for k, (items, kw) in cases().items()}


def load_model():
    pkg = load_package()
    so = os.environ.get("HLALA_HOST_LIB") or os.path.join(ROOT, "hla-la_amd", "libhlala_host.so")
    src = os.path.join(ROOT, "hla-la_amd", "csrc")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(os.path.join(src, f)) for f in ("bam_group_core.h", "bam_group_model.h", "host_check.cpp")):
        subprocess.check_call(["make", "-C", src, "../libhlala_host.so"])
    lib = C.CDLL(so)
    lib.hlala_host_bam_group_model.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(pkg.BamGroupStats)]
    lib.hlala_host_bam_group_model.restype = C.c_int
    lib.hlala_host_last_error.restype = C.c_char_p
    return lib


GUARD, CANARY = 64, 0xC7


def run_model(lib, recs, data, long_mode=False, n=None, n_bytes=None):
    """(rc, perm, flag, counts, error text); both outputs between canaries, which must survive; with a return code other than 0 nothing may have been written"""
    pkg = load_package()
    recs = np.ascontiguousarray(recs, pkg.BAM_REC_DTYPE).copy(); data = np.ascontiguousarray(data, np.uint8).copy()
    k = len(recs)
    perm = np.full(2 * GUARD + 4 * k, CANARY, np.uint8); flag = np.full(2 * GUARD + k, CANARY, np.uint8); st = pkg.BamGroupStats()
    rc = lib.hlala_host_bam_group_model(recs.ctypes.data if k else None, k if n is None else n, data.ctypes.data if data.size else None, data.size if n_bytes is None else n_bytes, int(bool(long_mode)),
                                        perm.ctypes.data + GUARD, flag.ctypes.data + GUARD, C.byref(st))
    for a in (perm, flag):
        assert (a[:GUARD] == CANARY).all() and (a[len(a) - GUARD:] == CANARY).all()
        if rc != 0:
            assert (a == CANARY).all()
    return rc, perm[GUARD:GUARD + 4 * k].view(np.uint32), flag[GUARD:GUARD + k], {f: int(getattr(st, f)) for f in COUNT_FIELDS}, lib.hlala_host_last_error().decode()


def malformed():
    """name -> (recs, data, n or None, n_bytes or None, what the refusal says)"""
    recs, data = build(sized(40, 3))
    out = {}
    out["name_beyond_buffer"] = (recs, data, None, int(recs["rec_off"][-1]) + 32 + int(recs["nameLen"][-1]) - 1, "beyond the byte buffer")
    r = recs.copy(); r["rec_off"][7] = M64 - 16
    out["rec_off_wraps"] = (r, data, None, None, "beyond the byte buffer")
    r = recs.copy(); r["nameLen"][11] = 0
    out["name_len_0"] = (r, data, None, None, "nameLen 0")
    r = recs.copy(); r["order"][20], r["order"][21] = recs["order"][21], recs["order"][20]
    out["not_ascending"] = (r, data, None, None, "ascending")
    r = recs.copy(); r["which"][3] = 2
    out["third_mate"] = (r, data, None, None, "mate")
    out["too_many"] = (recs, data, 1 << 31, None, "2^31")
    out["negative_n"] = (recs, data, -1, None, "negative")
    return out


def write_check_file(path, cases_):
    """[(recs, data, long_mode, n_bytes)] in the format tools/bam_group_check.cpp reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases_)))
        for recs, data, long_mode, n_bytes in cases_:
            nb = len(data) if n_bytes is None else n_bytes
            f.write(struct.pack("<qQi", len(recs), nb, int(long_mode)))
            f.write(recs.tobytes()); f.write(bytes(data[:nb]))


def fnv(b: bytes):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & M64
    return h
