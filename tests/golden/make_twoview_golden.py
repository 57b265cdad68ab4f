"""Generator of tests/golden/twoview_small.npz: the inputs of a handful of pairs as one rcn_twoview_init batch and the outputs
of tests/twoview_ref.py on them.  Run from the repository root: python tests/golden/make_twoview_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import twoview_ref as tv  # noqa: E402


def make():
    scenes = [tv.scene_pair(21, 0.2, n=120), tv.scene_pair(22, 0.5, n=150), tv.scene_pair(23, 0.0, n=40, distortion=True),
              tv.scene_pair(24, 0.3, n=90, planar=True)]
    pairs = [(s["xy1"], s["xy2"], s["K1"], s["K2"]) for s in scenes]
    s = scenes[0]
    pairs += [(s["xy1"][:4], s["xy2"][:4], s["K1"], s["K2"]), (np.repeat(s["xy1"][:1], 20, 0), np.repeat(s["xy2"][:1], 20, 0), s["K1"], s["K2"])]
    off = np.zeros(len(pairs) + 1, np.int64)
    off[1:] = np.cumsum([len(p[0]) for p in pairs])
    xy1 = np.concatenate([p[0] for p in pairs]).astype(np.int32)
    xy2 = np.concatenate([p[1] for p in pairs]).astype(np.int32)
    K1 = np.stack([p[2] for p in pairs]).astype(np.float64)
    K2 = np.stack([p[3] for p in pairs]).astype(np.float64)
    r = tv.two_view_init_batch(off, xy1, xy2, K1, K2)
    return dict(off=off, xy1=xy1, xy2=xy2, intr6_1=K1, intr6_2=K2, E=r["E"], pose34=r["pose34"], mask=r["mask"],
                cheir_mask=r["cheir_mask"], count=r["count"], iterations=r["iterations"])


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "twoview_small.npz"), **make())
