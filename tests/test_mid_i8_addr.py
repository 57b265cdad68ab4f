"""The fragment and LDS index arithmetic of the middle tier's int8 sweep on MFMA (csrc/mid_i8_addr.h): plain integer functions with a
host path.  No GPU here: tests/cpp/mid_i8_addr_test.cpp includes that header alone and checks that the four waves' A fragments cover the
512-row tile exactly once through the images' swizzle, that staging a query batch is a bijection, that a B fragment is the staged chunk of
the same k range as the A fragment it meets, and that the sixteen lanes of a ds_read_b128 group hit sixteen distinct positions of the bank
line.  Built as an executable of its own with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mid_i8_addr(tmp_path):
    exe = str(tmp_path / "mid_i8_addr_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "mid_i8_addr_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all cases pass" in r.stdout
