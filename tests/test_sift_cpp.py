"""FeatureClassic (reconstructor_amd/host/HipFeatureClassic.h) run by tests/cpp/sift_adapter_test on the golden images: the host
detect equals reconstructor_amd.sift.detect_and_compute bit for bit -- featCoord is the truncation of the keypoint, the 128
floats are the row; with an initial capacity of 1 the buffers grow and the call runs again; detectBatch leaves the capped rows on
the device; prepImg converts floats as cv::Mat::convertTo does."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "sift_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [4096, 1])
def test_host_detect_equals_python_detect(gpu_ctx, tmp_path, capacity):
    import torch
    from reconstructor_amd import sift
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    imgs = np.load(os.path.join(ROOT, "tests", "golden", "sift_small.npz"))["images"]
    n, H, W = imgs.shape
    K = 48
    dev = torch.from_numpy(imgs).cuda()
    want = {k: v.cpu().numpy() for k, v in sift.detect_and_compute(gpu_ctx, dev, 256).items()}
    capped = {k: v.cpu().numpy() for k, v in sift.detect_and_compute(gpu_ctx, dev, K).items()}
    counts = want["counts"]
    assert (counts > K).all() and (counts <= 256).all()
    values = np.array([-3.0, -0.5, 0.0, 0.5, 1.5, 2.5, 2.4999, 100.49, 100.5, 101.5, 254.5, 255.0, 255.5, 300.0, 17.0, 0.51], np.float32)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([n, H, W], np.int32).tobytes() + imgs.tobytes() + values.tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(capacity), str(K)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    runs, cap = 0, capacity                         # a call that finds more than the buffers hold grows them to that count and runs again
    for c in counts:
        runs += 2 if c > cap else 1
        cap = max(cap, int(c))
    assert r.stdout.split() == ["images", str(n), "runs", str(runs)] and (runs > n) == (capacity == 1)
    raw = open(tmp_path / "out.bin", "rb").read()
    feat = np.dtype([("xy", np.int32, 2), ("desc", np.float32, 128)])
    off = 0
    for i in range(n):
        m = int(np.frombuffer(raw, np.int32, 1, off)[0])
        off += 4
        assert m == counts[i]
        got = np.frombuffer(raw, feat, m, off)
        off += m * feat.itemsize
        assert np.array_equal(got["xy"], want["xy_int"][i, :m]) and np.array_equal(got["xy"], np.trunc(want["xy"][i, :m]).astype(np.int32))
        assert got["desc"].tobytes() == want["rows"][i, :m].tobytes()
    assert np.array_equal(np.frombuffer(raw, np.int32, n, off), counts)
    off += 4 * n
    for i in range(n):
        m = int(np.frombuffer(raw, np.int32, 1, off)[0])
        off += 4
        assert m == K
        assert np.array_equal(np.frombuffer(raw, np.int32, 2 * m, off).reshape(m, 2), capped["xy_int"][i])
        off += 8 * m
    assert raw[off:off + n * K * 128 * 4] == capped["rows"].tobytes()
    off += n * K * 128 * 4
    assert np.frombuffer(raw, np.uint8, 16, off).tolist() == [0, 0, 0, 0, 2, 2, 2, 100, 100, 102, 254, 255, 255, 255, 17, 1] and off + 16 == len(raw)
