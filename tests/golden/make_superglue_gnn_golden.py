"""Writes tests/golden/superglue_gnn_small.npz: the inputs and the float64 matching descriptors (tests/gnn_ref.py, two layers:
self, cross) of the three smallest shared cases, and a digest of the seeded weights (the weights themselves are megabytes).
Run from the repository root: python tests/golden/make_superglue_gnn_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import gnn_ref  # noqa: E402
from test_superglue_gnn_ref import GOLDEN_CASES, weights_digest  # noqa: E402

out = {"weights_sha256": np.array(weights_digest(gnn_ref.weights(2)))}
for m, n in GOLDEN_CASES:
    inp, md = gnn_ref.case(m, n)
    for name, a in zip(("kpts0", "scores0", "d0", "kpts1", "scores1", "d1"), inp):
        out["%s_%d_%d" % (name, m, n)] = a
    out["mdesc0_%d_%d" % (m, n)], out["mdesc1_%d_%d" % (m, n)] = md
np.savez_compressed(os.path.join(HERE, "superglue_gnn_small.npz"), **out)
print("wrote", os.path.join(HERE, "superglue_gnn_small.npz"))
