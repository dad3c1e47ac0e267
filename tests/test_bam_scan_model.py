"""The BAM record pass on the host: hlala_host_bam_scan_model of libhlala_host.so runs the passes of hla-la_amd/csrc/kernel_bamscan.hip serially over the shared core
(bam_scan_core.h).  Every expected answer comes from the record list (bam_scan_cases.expect).  The malformed and random inputs run here first, and once more under
ASan / UBSan in a stand-alone program (tools/bam_scan_check.cpp): the device test hands the same inputs to the kernels only because this file shows the core bounded on them."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bam_scan_cases as K

SLICES = (64, 256, 4096, 0)            # 0 = the default, 16 KiB


@pytest.fixture(scope="module")
def model():
    return K.load_model()


@pytest.fixture(scope="module")
def valid():
    return K.valid_cases()


def eff(S):
    return S or 16384


@pytest.mark.parametrize("S", SLICES)
def test_valid_inputs_equal_the_expectation(model, valid, S):
    names = [v[0] for v in valid]
    assert names == ["plain", "behind_header", "long_mode_masked", "n0", "n1", "n64", "n65", "long_reads"]
    for name, recs, data, first, refs, kw in valid:
        exp = K.expect(recs, refs, kw.get("long_mode", False), kw.get("hash_mask", K.M64), kw.get("first_seq", 0))
        assert exp["fail"] is None
        for last in (False, True):
            got = K.run_model(model, data, K.scan_args(refs, slice_bytes=S, **kw), first=first, last=last)
            K.assert_equals_expectation(got, exp, data, len(recs), len(data), eff(S))
        if name == "plain":
            assert len(exp["recs"]) > exp["n_kept"] > 20 and exp["examined"] > len(exp["recs"])          # records in two intervals; records examined and not kept
        if name == "long_reads":
            assert max(len(K.record_body(r)) for r in recs) > 65536 > eff(S) and exp["n_kept"] >= 4


def test_first_at_a_few_offsets(model, valid):
    _, recs, data, _, refs, _ = valid[0]
    starts = K.serialise(recs)[1]
    for k in (1, 7, len(recs) - 1, len(recs)):
        first = starts[k] if k < len(recs) else len(data)
        exp = K.expect(recs[k:], refs)
        got = K.run_model(model, data, K.scan_args(refs, slice_bytes=256), first=first)
        K.assert_equals_expectation(got, exp, data, len(recs) - k, len(data), 256)


@pytest.mark.parametrize("S", SLICES)
def test_partial_record_and_truncated_tail(model, valid, S):
    _, recs, data, _, refs, _ = valid[0]
    one = K.serialise(recs[:1])[0]
    for cut in (1, 3, 4, 20, len(one) - 1):                                                 # only a partial record: nothing found, nothing consumed
        rc, r, c, st = K.run_model(model, one[:cut], K.scan_args(refs, slice_bytes=S))
        assert rc == 0 and st["status"] == K.OK and st["n_records"] == 0 and st["consumed"] == 0 and len(r) == 0 and c == b""
        rc, r, c, st = K.run_model(model, one[:cut], K.scan_args(refs, slice_bytes=S), last=True)
        assert rc == 0 and st["status"] == K.BAD_LENGTH and st["status_record"] == 0 and st["consumed"] == 0
    k = 30
    whole = K.serialise(recs[:k])[0]; nxt = K.serialise(recs[k:k + 1])[0]
    exp = K.expect(recs[:k], refs)
    for extra in (2, 4, 36, len(nxt) - 1):
        data = whole + nxt[:extra]
        got = K.run_model(model, data, K.scan_args(refs, slice_bytes=S))
        K.assert_equals_expectation(got, exp, data, k, len(whole), eff(S))                   # consumed points at the tail
        rc, r, c, st = K.run_model(model, data, K.scan_args(refs, slice_bytes=S), last=True)
        assert rc == 0 and (st["status"], st["status_record"], st["consumed"], st["n_records"]) == (K.BAD_LENGTH, k, len(whole), k) and len(r) == 0 and c == b""


@pytest.mark.parametrize("S", SLICES)
@pytest.mark.parametrize("kind", ["qual", "B", "Z"])
def test_decoys_force_a_rehop_and_change_nothing(model, valid, kind, S):
    refs = valid[0][4]
    h = K.header(refs)
    recs, data, at = K.decoy_input(kind, eff(S), refs, np.random.default_rng(31), h)
    assert at % eff(S) == 0
    exp = K.expect(recs, refs)
    assert exp["fail"] is None and "carrier" in [r["name"] for r in recs]
    got = K.run_model(model, data, K.scan_args(refs, slice_bytes=S), first=len(h), last=True)
    assert got[3]["n_rehops"] >= 1                                                          # the decoy does what it is for
    K.assert_equals_expectation(got, exp, data, len(recs), len(data), eff(S))
    # without any re-hop allowed the call gives up, and writes nothing
    rc, r, c, st = K.run_model(model, data, K.scan_args(refs, slice_bytes=S, max_rehops=0), first=len(h), last=True)
    assert rc == 0 and st["status"] == K.TOO_MANY_REHOPS and len(r) == 0 and c == b""
    # ... and a cap of exactly the re-hops needed is enough
    got2 = K.run_model(model, data, K.scan_args(refs, slice_bytes=S, max_rehops=got[3]["n_rehops"]), first=len(h), last=True)
    assert got2[3] == got[3]


@pytest.mark.parametrize("S", SLICES)
def test_a_true_record_that_is_not_plausible(model, valid, S):
    refs = valid[0][4]
    recs, data = K.aligned_implausible(eff(S), refs, np.random.default_rng(32))
    exp = K.expect(recs, refs)
    got = K.run_model(model, data, K.scan_args(refs, slice_bytes=S), last=True)
    assert got[3]["n_rehops"] >= 1
    K.assert_equals_expectation(got, exp, data, len(recs), len(data), eff(S))
    assert b"odd" in got[2]


@pytest.mark.parametrize("S", (64, 0))
def test_each_corruption_gives_its_status_and_record(model, valid, S):
    refs = valid[0][4]
    cases = K.corruptions()
    assert len(cases) >= 9
    for name, (recs, status, which) in cases.items():
        exp = K.expect(recs, refs)
        assert exp["fail"] == (status, which), name
        rc, r, c, st = K.run_model(model, K.serialise(recs)[0], K.scan_args(refs, slice_bytes=S), last=True)
        assert rc == 0 and (st["status"], st["status_record"]) == (status, which), (name, st)
        assert len(r) == 0 and c == b"" and st["n_records"] == len(recs)
    # an unpaired record is fine as a long read
    recs = cases["unpaired"][0]
    got = K.run_model(model, K.serialise(recs)[0], K.scan_args(refs, slice_bytes=S, long_mode=True))
    K.assert_equals_expectation(got, K.expect(recs, refs, long_mode=True), K.serialise(recs)[0], len(recs), len(K.serialise(recs)[0]), eff(S))


@pytest.mark.parametrize("S", (64, 0))
def test_bad_length_on_the_true_chain_and_two_corruptions(model, valid, S):
    refs = valid[0][4]
    recs = [K.plain("r%d" % i, flag=1 | (64 if i % 2 else 128)) for i in range(8)]
    data, starts = K.serialise(recs)
    for v in (0, 31, -1, (1 << 28) + 1):
        bad = bytearray(data); bad[starts[5]:starts[5] + 4] = struct.pack("<i", v)
        rc, r, c, st = K.run_model(model, bytes(bad), K.scan_args(refs, slice_bytes=S))
        assert rc == 0 and (st["status"], st["status_record"], st["n_records"], st["consumed"]) == (K.BAD_LENGTH, 5, 5, starts[5]) and len(r) == 0 and c == b""
    # two corruptions: the record with the lower index is reported, whichever pass finds it
    two = list(recs); two[2] = K.plain("x", tags=[("NM", "C", 0)]); two[6] = K.plain("y", corrupt="l_seq")
    rc, r, c, st = K.run_model(model, K.serialise(two)[0], K.scan_args(refs, slice_bytes=S))
    assert (st["status"], st["status_record"]) == (K.NO_AS, 2)
    two[2], two[6] = two[6], two[2]
    rc, r, c, st = K.run_model(model, K.serialise(two)[0], K.scan_args(refs, slice_bytes=S))
    assert (st["status"], st["status_record"]) == (K.CORRUPT_RECORD, 2)
    d2, s2 = K.serialise(two); bad = bytearray(d2); bad[s2[7]:s2[7] + 4] = struct.pack("<i", 7)          # a bad length behind a corrupt record
    rc, r, c, st = K.run_model(model, bytes(bad), K.scan_args(refs, slice_bytes=S))
    assert (st["status"], st["status_record"], st["n_records"]) == (K.CORRUPT_RECORD, 2, 7)
    bad = bytearray(d2); bad[s2[1]:s2[1] + 4] = struct.pack("<i", 7)                                       # ... and in front of it
    rc, r, c, st = K.run_model(model, bytes(bad), K.scan_args(refs, slice_bytes=S))
    assert (st["status"], st["status_record"], st["n_records"]) == (K.BAD_LENGTH, 1, 1)


def test_arguments_and_capacity(model, valid):
    _, recs, data, _, refs, _ = valid[0]
    exp = K.expect(recs, refs)
    a = K.scan_args(refs)
    assert K.run_model(model, data, a, first=len(data) + 1)[0] == K.E_ARG
    for S in (1, 32, 63, 96, 3000):
        assert K.run_model(model, data, K.scan_args(refs, slice_bytes=S))[0] == K.E_ARG
    for damage in ("decreasing", "outside", "start"):
        b, keep = K.scan_args(refs)
        off, flat, cols = keep
        if damage == "decreasing":
            off[1] = off[2] + 1
        elif damage == "outside":
            flat[0] = len(K.INTERVALS)
        else:
            off[0] = 1
        assert K.run_model(model, data, (b, keep))[0] == K.E_ARG, damage
    nr, nc = len(exp["recs"]), len(exp["compact"])
    for cr, cc in ((nr - 1, nc), (nr, nc - 1), (0, 0)):
        rc, r, c, st = K.run_model(model, data, K.scan_args(refs), cap_recs=cr, cap_compact=cc)
        assert rc == K.E_CAPACITY and st["n_recs"] == nr and st["compact_bytes"] == nc             # the needed sizes; nothing was written (run_model checks)
    got = K.run_model(model, data, K.scan_args(refs), cap_recs=nr, cap_compact=nc)                    # exactly enough
    K.assert_equals_expectation(got, exp, data, len(recs), len(data), 16384)


def _bounded(model, refs, buffers, S):
    seen = set()
    for b in buffers:
        for last in (False, True):
            rc, r, c, st = K.run_model(model, b, K.scan_args(refs, slice_bytes=S), last=last)        # (canaries: run_model)
            assert rc == 0 and 0 <= st["status"] <= 7 and 0 <= st["consumed"] <= len(b) and st["n_records"] <= len(b) // 36
            seen.add(st["status"])
    return seen


def test_random_bytes_terminate(model, valid):
    refs = valid[0][4]
    bufs = K.random_buffers()
    assert len(bufs) == 300
    seen = _bounded(model, refs, bufs, 64) | _bounded(model, refs, bufs, 0)
    assert K.BAD_LENGTH in seen and K.OK in seen


def test_every_single_byte_change_terminates(model):
    refs, data, changed = K.byte_changes()
    assert len(changed) >= 500
    seen = _bounded(model, refs, changed, 64)
    assert {K.OK, K.BAD_LENGTH, K.CORRUPT_RECORD} <= seen


# ---- the same malformed and random inputs under ASan + UBSan, in a stand-alone program run as a child process
def write_cases(path, cases):
    """[(data, first, last, refs, kwargs of scan_args)] in the format tools/bam_scan_check.cpp reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for data, first, last, refs, kw in cases:
            a, (off, flat, cols) = K.scan_args(refs, **kw)
            m = int(off[a.n_ref]) if a.n_ref else 0
            f.write(struct.pack("<QQiiiiQQIi", len(data), first, int(last), a.long_read_mode, a.n_ref, a.n_intervals, a.hash_mask, a.first_seq, a.slice_bytes, a.max_rehops))
            f.write(off[:a.n_ref + 1].tobytes() + flat[:m].tobytes() + b"".join(col[:a.n_intervals].tobytes() for col in cols) + bytes(data))


def fnv(b):
    h = 0xcbf29ce484222325
    for x in np.frombuffer(b, np.uint8).tolist():
        h = ((h ^ x) * 0x100000001b3) & K.M64
    return h


def test_the_core_under_sanitizers_in_a_program_of_its_own(model, valid, tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is what builds libhlala_host.so as well"
    exe = tmp_path / "bam_scan_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe),
                           os.path.join(K.ROOT, "tools", "bam_scan_check.cpp")])
    refs = valid[0][4]
    cases = []
    for S in (64, 0):
        for b in K.random_buffers():
            cases.append((b, 0, len(b) % 2, refs, dict(slice_bytes=S)))
        for recs, _, _ in K.corruptions().values():
            cases.append((K.serialise(recs)[0], 0, 1, refs, dict(slice_bytes=S)))
        for kind in ("qual", "B", "Z"):
            recs, data, _ = K.decoy_input(kind, 64 if S else 16384, refs, np.random.default_rng(31), b"")
            cases.append((data, 0, 1, refs, dict(slice_bytes=S)))
            cases.append((data, 0, 1, refs, dict(slice_bytes=S, max_rehops=0)))
    _, data, changed = K.byte_changes()
    cases += [(b, 0, 1, refs, dict(slice_bytes=64)) for b in changed]
    name, recs, data, first, _, kw = valid[-1]
    cases.append((data, first, 1, refs, kw))                                                  # and valid ones: the long reads, the masked hashes
    name, recs, data, first, _, kw = valid[2]
    cases.append((data, first, 0, refs, kw))
    write_cases(tmp_path / "cases.bin", cases)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    for (data, first, last, _, kw), line in zip(cases, lines):                                # the sanitized build computes what the library computes
        rc, recs_, comp, st = K.run_model(model, data, K.scan_args(refs, **kw), first=first, last=bool(last))
        want = [rc] + [st[k] for k in K.STAT_FIELDS] + [fnv(recs_.tobytes()), fnv(comp)]
        assert [int(x) for x in line.split()] == want, line


def test_the_binding_mirrors_the_structs(pkg):
    import ctypes as C
    lib = pkg.load_library()
    for name, size in (("hlala_bam_rec", pkg.BAM_REC_DTYPE.itemsize), ("hlala_bam_scan_in", C.sizeof(pkg.BamScanIn)), ("hlala_bam_scan_stats", C.sizeof(pkg.BamScanStats))):
        assert lib.hlala_abi_sizeof(name.encode()) == size, name
    assert pkg.BAM_REC_DTYPE.itemsize == 48 and lib.hlala_abi_version() == pkg.ABI_VERSION == 7
    lib.hlala_bam_scan_status_text.restype = C.c_char_p; lib.hlala_bam_scan_status_text.argtypes = [C.c_int32]
    texts = [lib.hlala_bam_scan_status_text(i).decode() for i in range(9)]
    assert texts[0] == texts[7] == texts[8] == "" and texts[1] == "truncated BAM record" and texts[2] == "corrupt BAM record" and texts[3] == "corrupt BAM tag"
    assert texts[4] == "unknown BAM tag type" and texts[5] == "Can't get AS tag!" and "IsPaired" in texts[6]
