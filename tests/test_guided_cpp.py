"""GuidedMatcher (reconstructor_amd/host/HipGuidedMatcher.h) run by tests/cpp/guided_adapter_test: matchFeatures on the reference's
feature type equals reconstructor_amd.guided.match_pair and the contract bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import guided_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "guided_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


@pytest.mark.gpu
@pytest.mark.parametrize("cross", [0, 1])
def test_adapter_equals_python_match_pair(gpu_ctx, tmp_path, cross):
    from reconstructor_amd import guided
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    q, xy1, t, xy2, F = guided_ref.shape_case(300, 515, 128, seed=77)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(q), len(t), q.shape[1], cross], np.int32).tobytes() + np.asarray(F, np.float64).tobytes() + q.tobytes() + t.tobytes() +
                xy1.astype(np.int32).tobytes() + xy2.astype(np.int32).tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    got = np.fromfile(tmp_path / "out.bin", np.int32)
    want = guided.match_pair(gpu_ctx, q, xy1, t, xy2, F, guided.options(cross_check=cross))
    ref = guided_ref.match_pair(q, xy1, t, xy2, F, cross_check=cross)[0]
    n = int((ref >= 0).sum())
    assert np.array_equal(got, want) and np.array_equal(got, ref) and n > 50
    assert r.stdout.split() == ["matches", str(n), "threw", "1"]
