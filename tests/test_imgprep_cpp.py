"""reconstructor::Utils::ImagePrep (reconstructor_amd/host/HipImagePrep.h) run by tests/cpp/imgprep_adapter_test on the golden
inputs: readImg from a padded buffer, reshapeImg, extractFeatureColors and both saveCloud overloads agree with the golden outputs
of tests/img_ref.py; a Triangulator batch (HipTriangulator.h) gives every landmark the colour of the first feature of its track."""
import os
import subprocess

import numpy as np
import pytest

import img_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "imgprep_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter headers and their driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_adapter_agrees_with_the_golden_outputs(tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    g = np.load(os.path.join(ROOT, "tests", "golden", "imgprep_small.npz"))
    ims = g["images"]
    n, H, W = ims.shape[:3]
    K, L, C = g["xy_int"].shape[1], len(g["xyz"]), len(g["poses34"])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([n, H, W, 24, K, L, C], np.int32).tobytes() + ims.tobytes() + g["xy_int"].tobytes() + g["counts"].tobytes() +
                g["first_img"].tobytes() + g["first_feat"].tobytes() + g["xyz"].tobytes() + g["inlier"].tobytes() + g["poses34"].tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "plain.ply"), str(tmp_path / "flags.ply")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = open(tmp_path / "out.bin", "rb").read()
    off = 0
    rows, cols = g["gray"].shape[1:]
    for i in range(n):
        assert np.frombuffer(raw, np.int32, 2, off).tolist() == [rows, cols]
        assert np.frombuffer(raw, np.float64, 1, off + 8)[0] == float(g["factor"])
        off += 16
        assert raw[off:off + rows * cols * 3] == g["rgb"][i].tobytes()
        off += rows * cols * 3
        assert raw[off:off + rows * cols] == g["gray"][i].tobytes()
        off += rows * cols
        m = min(int(g["counts"][i]), K)
        assert np.array_equal(np.frombuffer(raw, np.int32, 3 * m, off).reshape(m, 3), g["feat_rgba"][i, :m, :3])
        off += 12 * m
    assert np.frombuffer(raw, np.int32, 2, off).tolist() == [rows, cols]
    off += 8
    assert raw[off:off + rows * cols * 3] == img_ref.resize_linear_u8(ims[0], rows, cols).tobytes()          # reshapeImg swaps nothing
    off += rows * cols * 3
    order = np.frombuffer(raw, np.int32, C, off)
    assert off + 4 * C == len(raw) and sorted(order.tolist()) == list(range(C))
    # the driver's landmarks index features only up to min(count, K): the golden colours of indices past that are black there too
    assert img_ref.read_ply(tmp_path / "flags.ply").tobytes() == img_ref.cloud_vertices(g["xyz"], g["lm_rgba"], g["inlier"], g["poses34"][order]).tobytes()
    assert img_ref.read_ply(tmp_path / "plain.ply").tobytes() == img_ref.cloud_vertices(g["xyz"], g["lm_rgba"], None, g["poses34"][order]).tobytes()
    words = r.stdout.split()
    assert words[0] == "landmarks" and words[2] == "coloured" and int(words[1]) == int(words[3]) > 0
