"""Generates tests/golden/triangulate_small.npz: a seeded batch of 2..6-view tracks with every kind of rejection (displaced
observations, far points, points at world z <= 0, radial distortion on some cameras) and the (xyz, status) of the
canonical restatement of the kernel (tests/tri_ref.py); the script refuses to write if the numpy-SVD restatement
disagrees on a status or on X beyond rounding.  Run from the repo root."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import tri_ref  # noqa: E402

PATH = os.path.join(HERE, "triangulate_small.npz")


def make():
    c = tri_ref.make_tracks(12, 400, 2, 6, seed=21, defect_rate=0.3, distortion=True)
    c.pop("points_gt")
    xyz, status = tri_ref.canonical_tracks(**c)
    x2, s2 = tri_ref.numpy_tracks(**c)
    ok = status == 0
    assert np.array_equal(status, s2)
    assert np.all(np.abs(xyz[ok] - x2[ok]) <= 1e-9 * np.abs(x2[ok]).max(1, keepdims=True))
    return dict(xyz=xyz, status=status, **c)


if __name__ == "__main__":
    g = make()
    np.savez_compressed(PATH, **g)
    print("tracks %d, statuses %s" % (len(g["status"]), np.bincount(g["status"], minlength=4)))
