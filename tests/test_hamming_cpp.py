"""HipHammingMatcher (reconstructor_amd/host/HipFeatureMatcher.h) run by tests/cpp/hamming_adapter_test: matchFeatures on rows of 32
floats equals reconstructor_amd.hamming.match_pair on the bytes bit for bit, and a row with a non-integer value throws."""
import os
import subprocess

import numpy as np
import pytest

import hamming_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "hamming_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_adapter_equals_python_match_pair(gpu_ctx, tmp_path):
    from reconstructor_amd import hamming
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    q, t = hamming_ref.planted_pair(np.random.default_rng(21), 300, 515)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(q), len(t)], np.int32).tobytes() + q.astype(np.float32).tobytes() + t.astype(np.float32).tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    got = np.fromfile(tmp_path / "out.bin", np.int32)
    want = hamming.match_pair(gpu_ctx, q, t)
    ref, n = hamming_ref.match_pair(q, t)
    assert np.array_equal(got, want) and np.array_equal(got, ref) and n > 50
    assert r.stdout.split() == ["matches", str(n), "threw", "1"]
