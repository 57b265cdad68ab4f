"""FeatureMatcherSuperglueNet (reconstructor_amd/host/HipSuperGlueMatcher.h) run by tests/cpp/superglue_gnn_adapter_test on a
planted pair with the seeded two-layer net: matchFeatures takes the reference's argument list (features with pixel
coordinates, a confidence and a descriptor; the image shapes) and fills its std::map at the 0.5 threshold; the batched form
leaves the same table (and that of the pair's leading features) in HBM."""
import os
import subprocess

import numpy as np
import pytest

import gnn_ref
import sg_ref
from reconstructor_amd import superglue_gnn as G
from test_superglue_gnn_ref import LOGP_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "superglue_gnn_adapter_test")
SHAPES = ((481, 641), (403, 377))                 # (height, width), odd: the centre is size / 2 in integers


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


def pixel_pair(m, n, seed):
    k0, s0, d0, k1, s1, d1, target = G.planted_inputs(np.random.default_rng(seed), m, n, int(round(0.6 * min(m, n))))
    px0 = np.rint(k0 * 400 + 320).astype(np.float32)
    px1 = np.rint(k1 * 250 + 190).astype(np.float32)
    return (px0, s0, d0, px1, s1, d1), target


def reference_map(sd, inp):
    """The std::map FeatureMatcherSuperglue.cpp:76-87 fills, and the rows whose decision may turn within the tolerance."""
    md = gnn_ref.forward(sd, gnn_ref.TYPES2, *inp, shapes=SHAPES)
    logP = sg_ref.assign(gnn_ref.scores(*md), alpha=float(sd["bin_score"]))[0]
    sel, (rows, _) = sg_ref.select(logP), sg_ref.undecided(logP, LOGP_TOL[2])
    return {i: int(t) for i, t in enumerate(sel["table"]) if t != -1}, rows


@pytest.mark.gpu
def test_adapter_fills_the_reference_map(tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    m, n = 70, 91
    sd = gnn_ref.weights(2)
    inp, target = pixel_pair(m, n, 321)
    params, types, bin_score = G.fold_state_dict(sd)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([2, m, n, *SHAPES[0], *SHAPES[1]], np.int32).tobytes() + np.float64(bin_score).tobytes() + np.array(types, np.int32).tobytes() +
                np.int64(params.size).tobytes() + params.tobytes())
        for a in inp:
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([BIN, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    raw = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), np.int32)
    k = int(raw[0])
    got = {int(q): int(t) for q, t in raw[1:1 + 2 * k].reshape(-1, 2)}
    assert list(got) == sorted(got)
    want, rows = reference_map(sd, inp)
    assert rows.sum() <= 0.02 * m
    assert {q: t for q, t in got.items() if not rows[q]} == {q: t for q, t in want.items() if not rows[q]}
    assert sum(got.get(i) == target[i] for i in range(m) if target[i] >= 0) >= 0.9 * (target >= 0).sum()
    stride = int(raw[1 + 2 * k])
    counts = raw[2 + 2 * k:4 + 2 * k]
    table = raw[4 + 2 * k:].reshape(2, stride)
    assert stride == m + 5 and (table[:, m:] == -1).all() and (table[1, m - 3:] == -1).all()
    assert {i: int(t) for i, t in enumerate(table[0]) if t != -1} == got and counts[0] == k
    want1, rows1 = reference_map(sd, tuple(a[:c] for a, c in zip(inp, (m - 3,) * 3 + (n - 2,) * 3)))
    got1 = {i: int(t) for i, t in enumerate(table[1]) if t != -1}
    assert counts[1] == len(got1) and {q: t for q, t in got1.items() if not rows1[q]} == {q: t for q, t in want1.items() if not rows1[q]}
