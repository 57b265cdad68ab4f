"""reconstructor::Utils::DenseCloud (reconstructor_amd/host/HipDenseCloud.h) run by tests/cpp/mvs_adapter_test: on the containers a caller
of the reference holds it gives the cloud of reconstructor_amd.mvs.dense_cloud and of the contract byte for byte, and the driver's own
plain loops over csrc/mvs_geom.h agree with it."""
import os
import subprocess

import numpy as np
import pytest

import mvs_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "mvs_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_adapter_equals_python_dense_cloud_and_a_plain_loop(gpu_ctx, tmp_path):
    import torch
    from reconstructor_amd import imgprep, mvs
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    sc, _ = M.small_case(40, 56, n=4, D=12, seed=11)
    K = sc["intrinsics"].copy()
    K[:, 4:] = 0.04, -0.01
    views = np.array([[0, 1, 2, 3], [1, 2, 0, -1], [3, 0, -1, -1]], np.int32)
    ranges = np.array([[3.0, 8.0], [3.5, 7.0], [2.5, 9.0]])
    opt = dict(radius=2, min_sources=1, min_consistent=1, stride=2, max_cost=0.4, rel_tol=0.02)
    D = 12
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([4, 40, 56, 3, 3, D, opt["radius"], opt["min_sources"], opt["min_consistent"], opt["stride"]], np.int32).tobytes() +
                np.array([opt["max_cost"], opt["rel_tol"]]).tobytes() + sc["poses34"].tobytes() + K.tobytes() + views.tobytes() + ranges.tobytes() +
                sc["gray"].tobytes() + sc["rgb"].tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "dense.ply")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    got = np.fromfile(tmp_path / "out.bin", np.uint8).view(M.VERTEX_DTYPE)
    inv = np.stack([M.inv_depths(a, b, D) for a, b in ranges])
    want = M.dense_cloud(sc["poses34"], K, sc["gray"], sc["rgb"], views, inv, **opt)
    py = mvs.dense_cloud((gpu_ctx, sc["poses34"], K), torch.as_tensor(np.array(sc["gray"])).cuda(), torch.as_tensor(np.array(sc["rgb"])).cuda(), views, inv, opt=mvs.options(**opt))
    assert got.tobytes() == want["vertices"].tobytes() == py["vertices"].tobytes() and len(got) > 300
    assert r.stdout.split() == ["vertices", str(len(got)), "plain", str(len(got)), "equal", "1", "maps", "1", "threw", "2"]
    with open(tmp_path / "dense.ply", "rb") as f:
        assert f.read().endswith(got.tobytes())
    assert imgprep.VERTEX_DTYPE == M.VERTEX_DTYPE
