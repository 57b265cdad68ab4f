"""Writes tests/golden/orb_small.npz: two 96 x 128 byte images and one 97 x 131 image, and what tests/orb_ref.py gives for
them at K = 256 and nfeatures = 24 (small enough that both cuts bind on level 0: 2 quota = 10 below its candidates): counts, the keypoint
fields, the float rows and the packed bytes, padded as the GPU pads them.  The images are rectangles of random grey levels, turned
by random angles, over mild noise (orb_ref.corner_image)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orb_ref  # noqa: E402

K, NFEATURES, RECTANGLES = 256, 24, 60
SHAPES = ((96, 128), (96, 128), (97, 131))
FIELDS = ("xy", "xy_int", "size", "angle", "response", "octave", "rows", "packed")


def images():
    return [orb_ref.corner_image(h, w, seed=40 + i, n_rect=RECTANGLES) for i, (h, w) in enumerate(SHAPES)]


def make():
    g = {}
    counts, cands = [], []
    for i, im in enumerate(images()):
        r = orb_ref.detect_and_compute(im, K, dict(nfeatures=NFEATURES))
        g["image%d" % i] = im
        for k in FIELDS:
            g["%s%d" % (k, i)] = r[k]
        counts.append(r["count"])
        L = r["layout"]
        cands.append(sum(len(orb_ref.nms(orb_ref.fast_scores(r["levels"][l], L["fast_threshold"]), L["edge_threshold"])[0])
                         for l in range(L["n_levels"]) if L["active"][l]))
    g["counts"] = np.array(counts, np.int32)
    g["candidates"] = np.array(cands, np.int32)
    return g


if __name__ == "__main__":
    g = make()
    print("keypoints %s of %s candidates" % (g["counts"].tolist(), g["candidates"].tolist()))
    path = os.path.join(HERE, "orb_small.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
