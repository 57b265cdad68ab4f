"""Shared intrinsics, the host side (csrc/ba_tied.h): validation of cam_group, normalisation of the groups, the per-camera tables and
the column map of the tied system are DATA built by pure host code.  No GPU here: tests/cpp/ba_tied_test.cpp includes that header
alone, plans random group assignments (none, one group, several, singletons, groups with constant members, cameras 0 and 1 inside
groups, both gauge flags on and off) and checks every plan against values it derives from the inputs: the map is a function onto
0 .. n' - 1, sources ascend, n' matches the formula, singletons are normalised, every rejection fires.  Built as an executable of its
own with the address and undefined-behaviour sanitizers, so that an index past a vector's end is a failure and not luck."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ba_tied_plan(tmp_path):
    exe = str(tmp_path / "ba_tied_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ba_tied_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all cases pass" in r.stdout
