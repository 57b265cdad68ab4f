"""The robust loss through the C++ adapters (reconstructor_amd/host/HipBundleAdjuster.h, HipBundleSession.h): BundleAdjuster::setLoss +
adjust and the incremental adapter give the bits of rcn_ba_solve_robust on the same containers, view by view, the loss report included;
switched off again they give rcn_ba_solve's (tests/cpp/ba_loss_adapter_test.cpp, built by __graft_entry__.build())."""
import os
import subprocess

import pytest

import ba_loss_ref as R
from reconstructor_amd import synth_ba
from test_cpp_adapter import _write_ba_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_driver_builds_without_a_gpu():
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "ba_loss_adapter_test"))


@pytest.mark.gpu
@pytest.mark.parametrize("nc,npts", [(6, 100), (11, 150)])
def test_cpp_adapters_with_a_loss_are_the_c_calls(tmp_path, nc, npts):
    """6 views: intrinsics constant; 11: the bounded-intrinsics branch from the tenth view on.  8 % of the observations displaced by 20 px
    or more per axis, so that the loss has something to do."""
    binary = os.path.join(ROOT, "tests", "cpp", "ba_loss_adapter_test")
    assert os.path.exists(binary), "run __graft_entry__.build() first"
    base = synth_ba.make_scene(nc, npts, obs_per_point=4, seed=23)
    sc, _ = R.plant_outliers(base, len(base["obs_cam"]) * 8 // 100, 23)
    inp = tmp_path / "scene.bin"
    with open(inp, "wb") as f:
        _write_ba_scene(f, sc, [3 * i + 1 for i in range(nc)])
    r = subprocess.run([binary, str(inp)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ba_loss_adapter_test ok" in r.stdout, r.stdout + r.stderr
