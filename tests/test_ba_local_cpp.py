"""The local adjustment through the C++ adapter (reconstructor_amd/host/HipBundleSession.h): IncrementalBundleAdjuster::adjustLocal after
every registered view -- the window it frees is the containers' covisibility, only the window's views and the landmarks it sees move,
the sub-problem has the sizes the containers say -- and a global adjust at the end (tests/cpp/local_ba_adapter_test.cpp, built by
__graft_entry__.build())."""
import os
import subprocess

import pytest

from reconstructor_amd import synth_ba
from test_cpp_adapter import _write_ba_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_driver_builds_without_a_gpu():
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "local_ba_adapter_test"))


@pytest.mark.gpu
@pytest.mark.parametrize("nc,npts,window", [(9, 200, 3), (14, 300, 5)])
def test_adjust_local_frees_the_covisible_window_and_nothing_else(tmp_path, nc, npts, window):
    binary = os.path.join(ROOT, "tests", "cpp", "local_ba_adapter_test")
    assert os.path.exists(binary), "run __graft_entry__.build() first"
    sc = synth_ba.make_scene(nc, npts, obs_per_point=4, seed=29)
    inp = tmp_path / "scene.bin"
    with open(inp, "wb") as f:
        _write_ba_scene(f, sc, [3 * i + 1 for i in range(nc)])
    r = subprocess.run([binary, str(inp), str(window)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "local_ba_adapter_test ok" in r.stdout, r.stdout + r.stderr
