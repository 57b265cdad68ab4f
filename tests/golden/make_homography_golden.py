"""Writes tests/golden/homography_small.npz from the restatement (tests/homography_ref.py): two planted-homography scenes
and the edge cases, as one batch of rcn_homography_ransac with its expected outputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import homography_ref as hr  # noqa: E402


def main():
    pairs = [(lambda s: (s["xy1"], s["xy2"]))(hr.scene(1, 0.3, n=200)), (lambda s: (s["xy1"], s["xy2"]))(hr.scene(2, 0.6, n=260))]
    pairs += [c[1:] for c in hr.edge_cases()]
    off = np.zeros(len(pairs) + 1, np.int64)
    off[1:] = np.cumsum([len(p[0]) for p in pairs])
    xy1 = np.concatenate([np.asarray(p[0], np.int32).reshape(-1, 2) for p in pairs])
    xy2 = np.concatenate([np.asarray(p[1], np.int32).reshape(-1, 2) for p in pairs])
    want = hr.find_batch(off, xy1, xy2)
    np.savez_compressed(os.path.join(HERE, "homography_small.npz"), off=off, xy1=xy1, xy2=xy2, **want)


if __name__ == "__main__":
    main()
