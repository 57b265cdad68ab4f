"""The robust losses of the bundle adjuster (csrc/ba_loss.h) are plain C++ with a host path.  No GPU here: tests/cpp/ba_loss_test.cpp
includes that header alone and checks rho, rho' and the row weight against long double -- the closed forms, a centred difference of
rho, Huber on both sides of its scale and bitwise the identity below it, s = 0, and non-finite s under every kind.  Built as an
executable of its own with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ba_loss(tmp_path):
    exe = str(tmp_path / "ba_loss_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ba_loss_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all cases pass" in r.stdout
