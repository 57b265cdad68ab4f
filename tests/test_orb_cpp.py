"""FeatureClassic(Detector::Orb) (reconstructor_amd/host/HipFeatureClassic.h) run by tests/cpp/orb_adapter_test: the host detect
equals reconstructor_amd.orb.detect_and_compute bit for bit -- featCoord is the truncation of the keypoint, the 32 floats are
the row; with an initial capacity of 1 the buffers grow and the call runs again; detectBatch leaves the capped rows on the
device; setOrbPattern reaches the kernel."""
import os
import subprocess

import numpy as np
import pytest

import orb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "orb_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN) and os.path.exists(os.path.join(ROOT, "tests", "cpp", "sift_adapter_test"))


@pytest.mark.gpu
@pytest.mark.parametrize("capacity,own", [(4096, 0), (1, 0), (4096, 1)])
def test_host_detect_equals_python_detect(gpu_ctx, tmp_path, capacity, own):
    import torch
    from reconstructor_amd import orb
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    imgs = np.stack([orb_ref.corner_image(128, 160, s, n_rect=70) for s in (31, 32, 33)])
    n, H, W = imgs.shape
    K = 24
    pattern = np.random.default_rng(4).integers(-15, 16, 1024).astype(np.int8)
    opt = orb.options(pattern=pattern) if own else None
    dev = torch.from_numpy(imgs).cuda()
    want = {k: v.cpu().numpy() for k, v in orb.detect_and_compute(gpu_ctx, dev, 512, opt).items()}
    capped = {k: v.cpu().numpy() for k, v in orb.detect_and_compute(gpu_ctx, dev, K, opt).items()}
    counts = want["counts"]
    assert (counts > K).all() and (counts <= 512).all()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([n, H, W], np.int32).tobytes() + imgs.tobytes() + pattern.tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(capacity), str(K), str(own)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    runs, cap = 0, capacity                         # a call that finds more than the buffers hold grows them to that count and runs again
    for c in counts:
        runs += 2 if c > cap else 1
        cap = max(cap, int(c))
    assert r.stdout.split() == ["images", str(n), "runs", str(runs)] and (runs > n) == (capacity == 1)
    raw = open(tmp_path / "out.bin", "rb").read()
    feat = np.dtype([("xy", np.int32, 2), ("desc", np.float32, 32)])
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
    assert raw[off:off + n * K * 32 * 4] == capped["rows"].tobytes() and off + n * K * 32 * 4 == len(raw)
