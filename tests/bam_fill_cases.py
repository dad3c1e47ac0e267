"""Descriptor sets for the fill stage (hlala_bam_fill_create / _window, hlala_host_bam_fill_model), the expectation -- a plain-Python statement of the rule that uses sorted()
and reversed(), as sortChainsInSeeds uses std::sort and std::reverse -- and the model's binding.  Shared by tests/test_bam_fill_model.py (CPU) and tests/test_gpu_bam_fill.py:
the device is handed exactly what the model has been shown to take.  Every case comes from a fixed seed.

A case is a list of units.  A unit is dict(name=bytes, host=bool, als=[alignment, ...]) with its alignments in file order; an alignment is dict(mate, AS, primary, codes (the
4-bit base codes), quals, cigar (words), contig, pos, rev).  build() lays every alignment out as a BAM record body at an arbitrary (mostly odd) offset of one byte buffer."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from conftest import ROOT, load_package

E_ARG, E_DEVICE = -1, -2
HOST = 0xFFFFFFFF
SEQ16 = b"=ACMGRSVTWYHKDBN"
COUNT_FIELDS = ("n_units", "n_host_units", "n_reads", "n_chains", "n_cigar", "n_bases", "n_name_bytes")


def al(rng, mate, AS, primary, l_seq=None, n_cigar=None, codes=None, quals=None):
    L = int(rng.integers(0, 40)) if l_seq is None else l_seq
    k = int(rng.integers(1, 5)) if n_cigar is None else n_cigar
    return dict(mate=mate, AS=int(AS), primary=bool(primary), codes=[int(x) for x in rng.integers(0, 16, L)] if codes is None else list(codes),
                quals=[int(x) for x in rng.integers(0, 256, L)] if quals is None else list(quals), cigar=[int(x) for x in rng.integers(0, 1 << 32, k, dtype=np.uint64)],
                contig=int(rng.integers(0, 9)), pos=int(rng.integers(-5, 1 << 30)), rev=bool(rng.integers(0, 2)), spare=int(rng.integers(0, 16)))


def unit(rng, name, sizes=(2, 2), host=False, scores=None, primary_at=None, long_mode=False):
    """a unit whose mates have sizes[m] alignments, interleaved in file order; scores: a function of (mate, k) (default: random with ties); primary_at[m]: which
    alignment of the mate (in file order) is primary (default: a random one, and sometimes a second one)"""
    nm = 1 if long_mode else 2
    als = []
    for m in range(nm):
        prim = {int(rng.integers(0, sizes[m]))} if primary_at is None else set(primary_at[m])
        if primary_at is None and sizes[m] > 1 and rng.random() < 0.3:
            prim.add(int(rng.integers(0, sizes[m])))
        keys = sorted(float(x) for x in rng.random(sizes[m]))
        for k in range(sizes[m]):
            als.append((keys[k], al(rng, m, scores(m, k) if scores else rng.integers(-3, 6), k in prim)))
    als = [a for _, a in sorted(als, key=lambda x: x[0])]        # the mates interleave, each in its own order
    return dict(name=bytes(name), host=bool(host), als=als)


def rule(als, m):
    """the mate's alignments in the order sortChainsInSeeds leaves, and the place of the first primary in it"""
    order = list(reversed(sorted([a for a in als if a["mate"] == m], key=lambda a: a["AS"])))
    return order, next(i for i, a in enumerate(order) if a["primary"])


def build(units, long_mode=False, seed=5):
    """(recs, data, unit_first, unit_count, host_sizes): the descriptors grouped by unit, the byte buffer, the unit arrays, the sizes of the host units"""
    pkg = load_package()
    rng = np.random.default_rng(seed)
    nm = 1 if long_mode else 2
    buf = bytearray(rng.integers(0, 256, 3, dtype=np.uint8).tobytes())
    recs, first, count, host_sizes = [], [], [], []
    seq = 1000
    for u in units:
        count.append(len(u["als"]))
        if u["host"]:
            first.append(HOST)
            for m in range(nm):
                order, prim = rule(u["als"], m)
                host_sizes += [len(order[prim]["codes"]), len(order), sum(len(a["cigar"]) for a in order)]
            host_sizes.append(len(u["name"]) + 1)
            continue
        first.append(len(recs))
        for a in u["als"]:
            buf += rng.integers(0, 256, 1 + 2 * int(rng.integers(0, 3)), dtype=np.uint8).tobytes()
            off = len(buf)
            L = len(a["codes"]); packed = bytearray((L + 1) // 2)
            for i, c in enumerate(a["codes"]):
                packed[i // 2] |= c << (4 if i % 2 == 0 else 0)
            if L % 2:
                packed[-1] |= a["spare"]                      # (the spare nibble of the record's last byte: a packed sample holds the byte as it lies)
            buf += rng.integers(0, 256, 32, dtype=np.uint8).tobytes() + u["name"] + b"\0" + b"".join(struct.pack("<I", w) for w in a["cigar"]) + bytes(packed) + bytes(a["quals"])
            recs.append((int(rng.integers(0, 1 << 63)), seq, off, a["contig"], a["pos"], a["AS"], len(a["codes"]) if a["primary"] else 0, len(a["cigar"]), len(u["name"]),
                         a["mate"], (1 if a["rev"] else 0) | (2 if a["primary"] else 0), len(u["name"]) + 1, 0))
            seq += 256
    buf += rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tobytes()
    return (np.array(recs, pkg.BAM_REC_DTYPE) if recs else np.zeros(0, pkg.BAM_REC_DTYPE), np.frombuffer(bytes(buf), np.uint8), np.array(first, np.uint32), np.array(count, np.uint32),
            np.array(host_sizes, np.int64))


def expect(units, long_mode=False, packed=False):
    """offsets and the whole sample's arrays from the units alone (the ranges of host units: zeros, as a cleared window leaves them)"""
    nm = 1 if long_mode else 2
    ro, co, gc, no = [0], [0], [0], [0]
    prim, bases, quals, contig, pos, offset, AS, rev, cig_end, cigar, names, pk = [], [], [], [], [], [], [], [], [], [], [], {}
    for ui, u in enumerate(units):
        names += ([0] * (len(u["name"]) + 1)) if u["host"] else (list(u["name"]) + [0])
        no.append(len(names))
        for m in range(nm):
            r = ui * nm + m
            order, p = rule(u["als"], m)
            pa = order[p]
            if u["host"]:
                prim.append(0); bases += [0] * len(pa["codes"]); quals += [0] * len(pa["codes"])
                for a in order:
                    contig.append(0); pos.append(0); offset.append(0); AS.append(0); rev.append(0); cig_end.append(0); cigar += [0] * len(a["cigar"])
            else:
                prim.append(co[-1] + p)
                L = len(pa["codes"]); by = bytearray((L + 1) // 2)
                for i, c in enumerate(pa["codes"]):
                    by[i // 2] |= c << (4 if i % 2 == 0 else 0)
                if L % 2:
                    by[-1] |= pa["spare"]
                pk[(ro[-1] + r + 1) >> 1] = bytes(by)
                bases += [SEQ16[c] for c in pa["codes"]]; quals += [(q + 33) % 256 for q in pa["quals"]]
                for a in order:
                    contig.append(a["contig"]); pos.append(a["pos"]); offset.append(0); AS.append(a["AS"]); rev.append(1 if a["rev"] else 0)
                    cigar += a["cigar"]; cig_end.append(len(cigar))
            ro.append(len(bases)); co.append(len(contig)); gc.append(len(cigar))
    nR = len(units) * nm
    packed_arr = np.zeros((len(bases) + nR + 1) // 2 + 2, np.uint8)
    for at, by in pk.items():
        packed_arr[at:at + len(by)] = np.frombuffer(by, np.uint8)
    off = dict(read_off=np.array(ro, np.int64), chain_off=np.array(co, np.int64), cigar_count=np.array(gc, np.int64), name_off=np.array(no, np.int64))
    arr = dict(read_primary=np.array(prim, np.int32), read_bases=np.array(bases, np.uint8), read_bases_packed=packed_arr, read_quals=np.array(quals, np.uint8), chain_contig=np.array(contig, np.int32),
               chain_pos=np.array(pos, np.int32), chain_offset=np.array(offset, np.int32), chain_as=np.array(AS, np.int32), chain_reverse=np.array(rev, np.uint8),
               cigar_off_end=np.array(cig_end, np.int64), cigar=np.array(cigar, np.uint32), name_chars=np.array(names, np.uint8))
    if packed:
        arr["read_bases"] = np.zeros(0, np.uint8)
    else:
        arr["read_bases_packed"] = np.zeros(0, np.uint8)
    return off, arr


def window_of(off, arr, u0, n, long_mode=False, packed=False):
    """the slices of expect()'s arrays a window of units [u0, u0 + n) holds"""
    nm = 1 if long_mode else 2
    r0, r1 = u0 * nm, (u0 + n) * nm
    ro, co, gc, no = off["read_off"], off["chain_off"], off["cigar_count"], off["name_off"]
    b, c, g = slice(int(ro[r0]), int(ro[r1])), slice(int(co[r0]), int(co[r1])), slice(int(gc[r0]), int(gc[r1]))
    p = slice((int(ro[r0]) + r0 + 1) >> 1, (int(ro[r1]) + r1 + 1) >> 1)
    out = dict(read_primary=arr["read_primary"][r0:r1], read_quals=arr["read_quals"][b], cigar=arr["cigar"][g], name_chars=arr["name_chars"][int(no[u0]):int(no[u0 + n])])
    out["read_bases"] = arr["read_bases"][0:0] if packed else arr["read_bases"][b]
    out["read_bases_packed"] = arr["read_bases_packed"][p] if packed else arr["read_bases_packed"][0:0]
    for k in ("chain_contig", "chain_pos", "chain_offset", "chain_as", "chain_reverse", "cigar_off_end"):
        out[k] = arr[k][c]
    return out


def windows(n_units):
    """(first unit, units): one unit, the last unit, all, two halves in reverse order, the same window twice"""
    if n_units == 0:
        return []
    h = n_units // 2
    w = [(0, 1), (n_units - 1, 1), (0, n_units), (h, n_units - h), (0, h), (h // 2, max(1, h // 2)), (h // 2, max(1, h // 2))]
    return [x for x in w if x[1] > 0]


def random_units(rng, n, long_mode=False, host=lambda i: False, max_mate=4, name_len=(1, 24)):
    out, seen = [], set()
    while len(out) < n:
        name = bytes(int(x) for x in rng.integers(33, 127, int(rng.integers(name_len[0], name_len[1] + 1))))
        if name in seen:
            continue
        seen.add(name)
        out.append(unit(rng, name, (int(rng.integers(1, max_mate + 1)), int(rng.integers(1, max_mate + 1))), host=host(len(out)), long_mode=long_mode))
    return out


_cases = None


def cases():
    """name -> (units, long_mode)"""
    global _cases
    if _cases is not None:
        return _cases
    rng = np.random.default_rng(2026)
    c = {}
    for n in (0, 1, 63, 64, 65, 257):
        c[f"units_{n}"] = (random_units(rng, n), False)
    # ---- mate sizes and ties
    for k in (1, 2, 15, 16):
        c[f"mate_{k}"] = ([unit(rng, b"m%d" % k, (k, max(1, 17 - k) if k < 16 else 16)), unit(rng, b"n%d" % k, (1, k))], False)
        c[f"mate_{k}_all_equal"] = ([unit(rng, b"e%d" % k, (k, k), scores=lambda m, j: 7)], False)
        c[f"mate_{k}_ties_at_the_top"] = ([unit(rng, b"t%d" % k, (k, k), scores=lambda m, j: 50 if j % 3 != 1 or j < 2 else 10 + j)], False)
    # ---- primaries
    for where, at in (("first", 0), ("middle", 3), ("last", 6)):
        c[f"primary_{where}"] = ([unit(rng, b"p" + where.encode(), (7, 7), primary_at=({at}, {at})), unit(rng, b"q" + where.encode(), (7, 7), scores=lambda m, j: 3, primary_at=({at}, {at}))], False)
    u = unit(rng, b"two-primaries", (5, 4), scores=lambda m, j: (9, 9, 4, 9, 1)[j], primary_at=({0, 3}, {1, 2}))
    for a, L in zip([x for x in u["als"] if x["primary"]], (11, 30, 7, 18)):
        a.update(al(rng, a["mate"], a["AS"], True, l_seq=L))
    c["two_primaries_of_different_l_seq"] = ([u], False)
    # ---- sequences and qualities
    us = []
    for L in (0, 1, 2, 63, 64, 65, 149, 150, 151, 257):
        x = unit(rng, b"len%d" % L, (2, 3))
        for a in x["als"]:
            if a["primary"]:
                a.update(al(rng, a["mate"], a["AS"], True, l_seq=L))
        us.append(x)
    c["l_seq_edges"] = (us, False)
    x = unit(rng, b"codes", (1, 1), primary_at=({0}, {0}))
    x["als"][0].update(al(rng, x["als"][0]["mate"], 5, True, codes=list(range(16)) + [15, 0, 9], quals=[0, 222, 223, 255] * 4 + [0, 222, 223]))
    x["als"][1].update(al(rng, x["als"][1]["mate"], 5, True, codes=list(range(15, -1, -1)), quals=[255, 223, 222, 0] * 4))
    c["base_codes_and_quality_bytes"] = ([x], False)
    # ---- CIGARs and names
    us = []
    for k in (1, 63, 64, 65, 300):
        x = unit(rng, b"cig%d" % k, (2, 2))
        for a in x["als"]:
            a.update(al(rng, a["mate"], a["AS"], a["primary"], n_cigar=k))
        us.append(x)
    c["n_cigar_edges"] = (us, False)
    c["name_lengths"] = ([unit(rng, b"Z"), unit(rng, bytes(int(v) for v in rng.integers(33, 127, 254))), unit(rng, b"ab")], False)
    # ---- one record taken for two intervals: two descriptors, one rec_off
    x = unit(rng, b"two-intervals", (2, 2))
    twin = dict(x["als"][0]); twin.update(contig=x["als"][0]["contig"] + 1, pos=x["als"][0]["pos"] - 100, twin_of=0)
    x["als"].insert(1, twin)
    c["one_record_two_intervals"] = ([x, unit(rng, b"after")], False)
    # ---- host units
    for name, fn in (("none", lambda i: False), ("first", lambda i: i == 0), ("last", lambda i: i == 36), ("every_second", lambda i: i % 2 == 1), ("all", lambda i: True)):
        c[f"host_units_{name}"] = (random_units(rng, 37, host=fn), False)
    c["host_unit_of_17"] = ([unit(rng, b"a"), unit(rng, b"big", (17, 3), host=True, primary_at=({2}, {1})), unit(rng, b"c")], False)
    # ---- long-read mode
    c["long_reads_65"] = (random_units(rng, 65, long_mode=True, host=lambda i: i % 9 == 4), True)
    c["long_reads_mate_16"] = ([unit(rng, b"L16", (16, 0), long_mode=True, scores=lambda m, j: j % 4)], True)
    _cases = c
    return c


def built_case(name, seed=5):
    units, long_mode = cases()[name]
    recs, data, first, count, hs = build(units, long_mode, seed)
    # (the twin of one_record_two_intervals shares its sibling's record: one rec_off for two descriptors)
    for u in units:
        for i, a in enumerate(u["als"]):
            if "twin_of" in a and not u["host"]:
                g = int(first[units.index(u)]) + i
                recs[g]["rec_off"] = recs[int(first[units.index(u)]) + a["twin_of"]]["rec_off"]
    return units, long_mode, recs, data, first, count, hs


def large_case():
    rng = np.random.default_rng(99)
    return random_units(rng, 3000, host=lambda i: i % 97 == 5, max_mate=6), False


def malformed():
    """name -> (kwargs of changes to a valid input, what the refusal says); apply() makes the input"""
    return {
        "unit_beyond_the_descriptors": (dict(first_at=(3, "n - 1")), "beyond the descriptors"),
        "unit_first_wraps": (dict(first_at=(3, 0xFFFFFFF0)), "beyond the descriptors"),
        "unit_count_0": (dict(count_at=(5, 0)), "unit_count 0"),
        "record_beyond_the_buffer": (dict(n_bytes="short"), "beyond the byte buffer"),
        "rec_off_wraps": (dict(rec=(7, "rec_off", (1 << 64) - 8)), "beyond the byte buffer"),
        "l_seq_beyond_the_buffer": (dict(rec=(0, "l_seq", 1 << 30), primary0=True), "beyond the byte buffer"),
        "negative_l_seq": (dict(rec=(2, "l_seq", -1)), "negative l_seq"),
        "mate_2": (dict(rec=(4, "which", 2)), "mate is not 0 / 1"),
        "mate_1_in_long_read_mode": (dict(long_mode=True), "mate is not 0 / 1"),
        "mate_of_17": (dict(units="mate17"), "more than 16 alignments"),
        "no_primary": (dict(units="noprimary"), "without a primary"),
        "host_units_short": (dict(n_host_units=0), "more host units than n_host_units"),
        "host_units_long": (dict(n_host_units=3), "fewer host units than n_host_units"),
        "host_size_negative": (dict(host_size=(1, -1)), "host unit's size"),
        "too_many_chains": (dict(host_size=(1, 0x7FFFFFFF)), "2^31 - 1 chains"),
        "too_many_descriptors": (dict(n=1 << 31), "2^31"),
        "negative_n_units": (dict(n_units=-1), "negative"),
    }


def apply(change):
    """a valid input (20 units, two of them host units) with one thing wrong: (recs, data, first, count, host_sizes, long_mode, n, n_bytes, n_units, n_host_units)"""
    rng = np.random.default_rng(31)
    long_mode = bool(change.get("long_mode"))
    units = random_units(rng, 20, host=lambda i: i in (6, 13))
    if change.get("units") == "mate17":
        units[2] = unit(rng, b"seventeen", (17, 2))
    if change.get("units") == "noprimary":
        units[2] = unit(rng, b"no-primary", (3, 2))
    recs, data, first, count, hs = build(units, False)
    if change.get("units") == "noprimary":                    # (the unit's mate 1 loses its primaries after the build: rule() needs one)
        recs = recs.copy(); k = slice(int(first[2]), int(first[2]) + int(count[2]))
        recs["flags"][k] = np.where(recs["which"][k] == 1, recs["flags"][k] & 1, recs["flags"][k])
    recs = recs.copy(); first = first.copy(); count = count.copy(); hs = hs.copy()
    n = n_bytes = n_units = n_host = None
    if "first_at" in change:
        i, v = change["first_at"]; first[i] = len(recs) - 1 if v == "n - 1" else v
        if v == "n - 1":
            count[i] = 2
    if "count_at" in change:
        i, v = change["count_at"]; count[i] = v
    if change.get("n_bytes") == "short":
        n_bytes = int(recs["rec_off"].max()) + 20
    if "rec" in change:
        i, f, v = change["rec"]
        if change.get("primary0"):
            i = int(np.nonzero(recs["flags"] & 2)[0][0])
        recs[f][i] = v
    if "host_size" in change:
        i, v = change["host_size"]; hs[i] = v
    n = change.get("n"); n_units = change.get("n_units"); n_host = change.get("n_host_units")
    return recs, data, first, count, hs, long_mode, n, n_bytes, n_units, n_host


def load_model():
    pkg = load_package()
    so = os.environ.get("HLALA_HOST_LIB") or os.path.join(ROOT, "hla-la_amd", "libhlala_host.so")
    src = os.path.join(ROOT, "hla-la_amd", "csrc")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(os.path.join(src, f)) for f in ("bam_fill_core.h", "bam_fill_model.h", "host_check.cpp")):
        subprocess.check_call(["make", "-C", src, "../libhlala_host.so"])
    lib = C.CDLL(so)
    lib.hlala_host_bam_fill_model.argtypes = [C.POINTER(pkg.BamFillIn), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(pkg.BamFillOut), C.POINTER(pkg.BamFillStats)]
    lib.hlala_host_bam_fill_model.restype = C.c_int
    lib.hlala_host_last_error.restype = C.c_char_p
    return lib


CANARY = 0xA5


def run_model(lib, recs, data, first, count, hs, long_mode=False, packed=False, window=None, n=None, n_bytes=None, n_units=None, n_host_units=None):
    """(rc, offsets, window arrays or None, counts, error text).  window = (first unit, units): the model lays the sample out (a first call) and fills that window (a second
    one, with slices sized from the offsets); every slice has one spare element behind it, which must survive"""
    pkg = load_package()
    fin, keep = pkg.bam_fill_in(recs, data, first, count, hs, long_mode, packed, n=n, n_bytes=n_bytes, n_units=n_units, n_host_units=n_host_units)
    off = pkg.bam_fill_offsets(len(first), long_mode); st = pkg.BamFillStats()
    ptr = [off[k].ctypes.data for k in ("read_off", "chain_off", "cigar_count", "name_off")]
    rc = lib.hlala_host_bam_fill_model(C.byref(fin), *ptr, 0, -1, None, C.byref(st))
    err = lib.hlala_host_last_error().decode()
    arrs = None
    if rc == 0 and window is not None and len(first):
        out, arrs, size = pkg.bam_fill_window_arrays(off, window[0], window[1], long_mode, packed, CANARY)
        rc = lib.hlala_host_bam_fill_model(C.byref(fin), *ptr, window[0], window[1], C.byref(out), C.byref(st))
        err = lib.hlala_host_last_error().decode()
        arrs = check_canaries(arrs, size)
    return rc, off, arrs, {f: int(getattr(st, f)) for f in COUNT_FIELDS}, err


def check_canaries(arrs, size):
    """the spare element behind every slice still holds the canary; returns the slices without it"""
    out = {}
    for k, a in arrs.items():
        assert a[size[k]:].tobytes() == bytes([CANARY]) * a[size[k]:].nbytes, k
        out[k] = a[:size[k]]
    return out


def write_check_file(path, inputs):
    """[(recs, data, first, count, host_sizes, long_mode, packed, n_bytes or None)] in the format tools/bam_fill_check.cpp reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(inputs)))
        for recs, data, first, count, hs, long_mode, packed, n_bytes in inputs:
            nb = len(data) if n_bytes is None else n_bytes
            nm = 1 if long_mode else 2
            f.write(struct.pack("<qQqqii", len(recs), nb, len(first), len(hs) // (3 * nm + 1), int(long_mode), int(packed)))
            f.write(recs.tobytes()); f.write(bytes(data[:nb])); f.write(np.ascontiguousarray(first, np.uint32).tobytes()); f.write(np.ascontiguousarray(count, np.uint32).tobytes())
            f.write(np.ascontiguousarray(hs, np.int64)[:len(hs) // (3 * nm + 1) * (3 * nm + 1)].tobytes())


def fnv(b: bytes, h=0xcbf29ce484222325):
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & ((1 << 64) - 1)
    return h
