"""FeatureSuperPointPost (reconstructor_amd/host/HipFeatureSuperPoint.h) run by tests/cpp/keypoint_adapter_test on the golden
logits: processKeypoints returns the stored keypoints in the reference's container, detectPost the same keypoints with the
oracle's descriptor rows; a capacity smaller than the keypoint count grows instead of truncating."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "keypoint_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [2048, 100])
def test_adapter_reproduces_the_golden_keypoints_and_oracle_rows(tmp_path, capacity):
    from oracle import orc
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    g = np.load(os.path.join(ROOT, "tests", "golden", "keypoints_small.npz"))
    img = 1
    n = int(g["counts"][img])
    dmap = np.random.default_rng(17).standard_normal((256, 15, 20)).astype(np.float32)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([120, 160], np.int32).tobytes() + g["logits"][img].tobytes() + dmap.tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(capacity)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.split()[:4] == ["keypoints", str(n), "features", str(n)]
    raw = open(tmp_path / "out.bin", "rb").read()
    kp = np.dtype([("xy", np.int32, 2), ("conf", np.float32)])
    feat = np.dtype([("xy", np.int32, 2), ("conf", np.float32), ("desc", np.float32, 256)])
    assert np.frombuffer(raw, np.int32, 1)[0] == n
    a = np.frombuffer(raw, kp, n, 4)
    off = 4 + n * kp.itemsize
    assert np.frombuffer(raw, np.int32, 1, off)[0] == n and len(raw) == off + 4 + n * feat.itemsize
    b = np.frombuffer(raw, feat, n, off + 4)
    assert np.array_equal(a["xy"], g["xy"][img, :n]) and np.array_equal(b["xy"], a["xy"]) and a["conf"].tobytes() == b["conf"].tobytes()
    assert np.allclose(a["conf"], g["conf"][img, :n], rtol=2.0 ** -21 + 2.0 ** -19, atol=0)      # as in test_keypoints_gpu.py
    assert b["desc"].tobytes() == orc.desc_sample(dmap, a["xy"]).tobytes()
