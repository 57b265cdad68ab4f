"""Writes tests/golden/superpoint_net_small.npz: the images and the float64 logits and descriptors (normalised) of the three
smallest cases of tests/spnet_ref.py, plus a digest of the seeded weights (the weights themselves are 5 MB and are not
stored).  To stay under 100 KB the descriptors of the 40 x 72 case are kept for every second cell in each direction.

    python tests/golden/make_superpoint_net_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import spnet_ref  # noqa: E402
from test_superpoint_net_ref import desc_subset, weights_digest  # noqa: E402

out = {"weights_sha256": np.array(weights_digest(spnet_ref.weights()))}
for H, W in spnet_ref.GOLDEN_SHAPES:
    img, lg, ds = spnet_ref.case(H, W)
    out["image_%d_%d" % (H, W)] = img
    out["logits_%d_%d" % (H, W)] = lg
    out["desc_%d_%d" % (H, W)] = desc_subset(ds, H, W)
path = os.path.join(HERE, "superpoint_net_small.npz")
np.savez(path, **out)
print(path, os.path.getsize(path), "bytes")
