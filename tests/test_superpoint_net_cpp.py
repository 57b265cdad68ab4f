"""FeatureSuperPointNet (reconstructor_amd/host/HipFeatureSuperPoint.h) run by tests/cpp/superpoint_net_adapter_test: the host
detect on one 40 x 72 image equals reconstructor_amd.superpoint_net.detect on the same image and weights in count,
coordinates, confidences and row bits; with an initial capacity of 1 the buffers grow once and the call runs again; prepImg
is the division by the double 255.0."""
import os
import subprocess

import numpy as np
import pytest

import spnet_ref as R
from reconstructor_amd import superpoint_net as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "superpoint_net_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [2048, 1])
def test_host_detect_equals_python_detect(gpu_ctx, tmp_path, capacity):
    import torch
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    H, W = 40, 72
    img = R.image(H, W)
    params = SP.pack_state_dict(R.weights())
    with SP.Net(gpu_ctx, params) as net:
        want = SP.detect(gpu_ctx, net, torch.from_numpy(np.array(img)[None]).cuda(), 512)
    n = int(want["counts"][0])
    assert 1 < n <= 512
    bytes256 = np.arange(256, dtype=np.uint8)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([H, W], np.int32).tobytes() + np.array([params.size], np.int64).tobytes() + params.tobytes() + img.tobytes() + bytes256.tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(capacity)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.split()[:4] == ["features", str(n), "runs", "2" if capacity < n else "1"]
    raw = open(tmp_path / "out.bin", "rb").read()
    feat = np.dtype([("xy", np.int32, 2), ("conf", np.float32), ("desc", np.float32, 256)])
    assert np.frombuffer(raw, np.int32, 1)[0] == n and len(raw) == 4 + n * feat.itemsize + 256 * 4
    got = np.frombuffer(raw, feat, n, 4)
    assert np.array_equal(got["xy"], want["xy"][0, :n].cpu().numpy())
    assert got["conf"].tobytes() == want["conf"][0, :n].cpu().numpy().tobytes()
    assert got["desc"].tobytes() == want["rows"][0, :n].cpu().numpy().tobytes()
    assert np.frombuffer(raw, np.float32, 256, 4 + n * feat.itemsize).tobytes() == SP.prep_u8(bytes256).tobytes()
