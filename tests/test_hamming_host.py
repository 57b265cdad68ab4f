"""packBinaryRows (reconstructor_amd/host/PackBinaryRows.h) turns the 32 floats a binary descriptor crosses the reference's boundary as
back into its bytes; it is pure C++.  No GPU here: tests/cpp/hamming_host_test.cpp includes the header alone and checks the round trip
of every byte value, the refusal of 0.5 / -1 / 256 / NaN, wrong row lengths and the empty input.  Built as an executable of its own with
the address and undefined-behaviour sanitizers, so that a conversion of a value outside the byte range is a failure."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hamming_host(tmp_path):
    exe = str(tmp_path / "hamming_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "hamming_host_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all cases pass" in r.stdout
