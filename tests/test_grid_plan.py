"""The plan of the matcher's grid call (csrc/grid_plan.h) is DATA built by pure host code: groups of pairs, pipeline chunks, the order of
a chunk's work items per XCD, the layout of the middle tier's workspace and the predicates that choose the kernels.  No GPU here:
tests/cpp/grid_plan_test.cpp includes that header alone, plans the smallest grids at which each rule can go wrong and checks the
invariants of every plan against values it derives from the inputs.  Built as an executable of its own with the address and
undefined-behaviour sanitizers, so that an index past a vector's end is a failure and not luck."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_plan(tmp_path):
    exe = str(tmp_path / "grid_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "grid_plan_test.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "all cases pass" in r.stdout
