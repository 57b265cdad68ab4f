"""Shared intrinsics through the C++ adapters (reconstructor_amd/host/HipBundleAdjuster.h, HipBundleSession.h):
BundleAdjuster::setSharedIntrinsics + adjust and the incremental adapter give the bits of rcn_ba_solve_tied on the same containers, view by
view, every member's PinholeCamera equal afterwards; with an empty map they give rcn_ba_solve's (tests/cpp/ba_tied_adapter_test.cpp, built
by __graft_entry__.build())."""
import os
import subprocess

import pytest

from reconstructor_amd import synth_ba
from test_cpp_adapter import _write_ba_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_driver_builds_without_a_gpu():
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "ba_tied_adapter_test"))


@pytest.mark.gpu
def test_cpp_adapters_with_groups_are_the_c_call(tmp_path):
    """13 views: intrinsics constant up to the ninth, the bounded-intrinsics branch with two groups and views of their own from the tenth on."""
    binary = os.path.join(ROOT, "tests", "cpp", "ba_tied_adapter_test")
    assert os.path.exists(binary), "run __graft_entry__.build() first"
    sc = synth_ba.make_scene(13, 180, obs_per_point=4, seed=29)
    inp = tmp_path / "scene.bin"
    with open(inp, "wb") as f:
        _write_ba_scene(f, sc, [3 * i + 1 for i in range(13)])
    r = subprocess.run([binary, str(inp)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ba_tied_adapter_test ok" in r.stdout, r.stdout + r.stderr
