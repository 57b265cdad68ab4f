"""FeatureMatcherSuperglueAssign (reconstructor_amd/host/HipSuperGlueMatcher.h) run by tests/cpp/superglue_adapter_test on a
planted pair in the network's [descSize][featuresNum] layout: matchFeatures fills the reference's std::map at its 0.5
threshold, the batched form leaves the same table (and that of the pair's leading features) in HBM."""
import os
import subprocess

import numpy as np
import pytest

import sg_ref
from test_superglue_ref import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "superglue_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


def reference_map(d0, d1):
    """The std::map FeatureMatcherSuperglue.cpp:76-87 fills, and the rows whose decision may turn within the tolerance."""
    S = (d0.astype(np.float64) @ d1.astype(np.float64).T / 16.0).astype(np.float32)
    logP = sg_ref.assign(S)[0]
    sel, (rows, _) = sg_ref.select(logP), sg_ref.undecided(logP, TOL + 1e-5)          # + the fp32 rounding of the scores (< 2^-20 * 12)
    return {i: int(t) for i, t in enumerate(sel["matches0"]) if t != -1 and sel["mscores0"][i] > 0.5}, rows


@pytest.mark.gpu
def test_adapter_fills_the_reference_map(tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    m, n, D = 70, 91, 256
    d0, d1, target = sg_ref.planted_case(m, n, 123)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([m, n, D], np.int32).tobytes() + np.ascontiguousarray(d0.T).tobytes() + np.ascontiguousarray(d1.T).tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), np.int32)
    k = int(raw[0])
    got = {int(q): int(t) for q, t in raw[1:1 + 2 * k].reshape(-1, 2)}
    assert list(got) == sorted(got)
    want, rows = reference_map(d0, d1)
    assert rows.sum() <= 0.02 * m
    assert {q: t for q, t in got.items() if not rows[q]} == {q: t for q, t in want.items() if not rows[q]}
    assert sum(got.get(i) == target[i] for i in range(m) if target[i] >= 0) >= 0.9 * (target >= 0).sum()
    stride = int(raw[1 + 2 * k])
    counts = raw[2 + 2 * k:4 + 2 * k]
    table = raw[4 + 2 * k:].reshape(2, stride)
    assert stride == m + 5 and (table[:, m:] == -1).all() and (table[1, m - 3:] == -1).all()
    assert {i: int(t) for i, t in enumerate(table[0]) if t != -1} == got and counts[0] == k
    want1, rows1 = reference_map(d0[:m - 3], d1[:n - 2])
    got1 = {i: int(t) for i, t in enumerate(table[1]) if t != -1}
    assert counts[1] == len(got1) and {q: t for q, t in got1.items() if not rows1[q]} == {q: t for q, t in want1.items() if not rows1[q]}
