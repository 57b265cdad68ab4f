"""The batched top-2 fold of the coarse kernels (csrc/top2_fold.h) is pure integer logic with a host path.  No GPU here:
tests/cpp/top2_fold_test.cpp includes that header alone and checks top2_fold2 / top2_fold4 against a sort -- exhaustively on small
values, on random 32-bit keys with the padded-row key 0xFFFFFFFF in every position, and on chains of 32 keys folded by four, by
two and key by key.  Built as an executable of its own with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_top2_fold(tmp_path):
    exe = str(tmp_path / "top2_fold_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "top2_fold_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all cases pass" in r.stdout
