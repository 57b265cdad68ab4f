"""HipImageMatcher (reconstructor_amd/host/HipImageMatcher.h) run by tests/cpp/retrieval_adapter_test on the golden scene: match
fills the partners retrieval.image_pairs retrieves, under the caller's own image ids and whatever order the map was filled in;
with top_k >= n - 1 it fills what FakeImgMatcher does (ImageMatcher.cpp:6-23: every other image); matchDevice returns the list."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "retrieval_adapter_test")
FIRST, STEP = 10, 3


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


def _run(tmp_path, scene, counts, top_k):
    n, K, D = scene.shape
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([n, K, D, FIRST, STEP], np.int32).tobytes() + counts.astype(np.int32).tobytes() + scene.tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(top_k), "8", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["images", str(n)], r.stderr + r.stdout
    raw = np.fromfile(tmp_path / "out.bin", np.int32)
    off, partners = 0, {}
    for s in range(n):
        img, m = int(raw[off]), int(raw[off + 1])
        assert img == FIRST + s * STEP
        partners[s] = raw[off + 2:off + 2 + m].tolist()
        off += 2 + m
    P = int(raw[off])
    pairs = raw[off + 1:off + 1 + 2 * P].reshape(P, 2)
    assert off + 1 + 2 * P == len(raw)
    return partners, pairs


@pytest.mark.gpu
@pytest.mark.parametrize("top_k", [3, 11, 20])
def test_host_match_equals_python_image_pairs(gpu_ctx, tmp_path, top_k):
    import torch
    from reconstructor_amd import retrieval
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    scene = np.load(os.path.join(ROOT, "tests", "golden", "retrieval_small.npz"))["scene"]
    n, K, D = scene.shape
    counts = np.full(n, K, np.int32)
    counts[4] = 31                                            # ragged: the adapter pads to the largest image
    scene = scene.copy()
    scene[4, 31:] = 0
    dev, cn = torch.from_numpy(scene).cuda(), torch.from_numpy(counts).cuda()
    cb = retrieval.train_codebook(gpu_ctx, dev, cn, n_centroids=8, iterations=5)
    want = retrieval.image_pairs(gpu_ctx, cb, dev, cn, top_k=top_k)
    cb.close()
    partners, pairs = _run(tmp_path, scene, counts, top_k)
    assert np.array_equal(pairs, want + FIRST)                # matchDevice: ids first + slot
    exp = {s: [] for s in range(n)}
    for a, b in want.tolist():
        exp[a].append(FIRST + b * STEP)
        exp[b].append(FIRST + a * STEP)
    assert partners == {s: sorted(v) for s, v in exp.items()}
    if top_k >= n - 1:                                        # FakeImgMatcher: every other image
        assert all(partners[s] == [FIRST + t * STEP for t in range(n) if t != s] for s in range(n))
    else:
        assert len(want) < n * (n - 1) // 2
