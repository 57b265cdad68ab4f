"""The host side of the ORB stage (csrc/orb_layout.h: option ranges, level sizes, offsets, quotas, the pattern check; csrc/orb_pattern.h:
the built-in table) is pure C++.  No GPU here: tests/cpp/orb_host_test.cpp includes those headers alone and checks every layout
against values it derives from the inputs, the refusals, and the umax and blur tables against their formulas.  Built as an
executable of its own with the address and undefined-behaviour sanitizers, so that an index past an array's end is a failure."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_orb_host(tmp_path):
    exe = str(tmp_path / "orb_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "orb_host_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all cases pass" in r.stdout
