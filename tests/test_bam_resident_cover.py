"""The accounting of units handed out by resident windows and by the host's fill (hla-la_amd/csrc/bam_resident_cover.h) under ASan and UBSan: tools/bam_resident_cover_check.cpp
is a program of its own that runs random window sequences -- overlapping, empty, ending at the sample's end, asked for twice, whole chunks -- against a count per unit."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cover_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is what builds libhlala_host.so as well"
    exe = tmp_path / "bam_resident_cover_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", str(exe),
                           os.path.join(ROOT, "tools", "bam_resident_cover_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 15 * 6 and all("chunks counted once each" in x for x in lines)
