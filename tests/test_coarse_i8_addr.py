"""The LDS addresses of the int8 coarse kernel's 16x16x64 shape are a per-lane constant plus the ring buffer's address plus an
immediate (csrc/coarse_i8_addr.h): plain integer functions with a host path.  No GPU here: tests/cpp/coarse_i8_addr_test.cpp includes
that header alone and checks, for every lane, k-step, row block, half and ring buffer, that the sum is the address the kernel computed
in one piece before, that every immediate fits the 16-bit offset field and that the sixteen lanes of a ds_read_b128 group hit sixteen
distinct 16-byte chunks.  Built as an executable of its own with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_coarse_i8_addr(tmp_path):
    exe = str(tmp_path / "coarse_i8_addr_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "coarse_i8_addr_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all cases pass" in r.stdout
