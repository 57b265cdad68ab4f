"""Writes tests/golden/sift_small.npz: 3 grey images of 120 x 160 (uint8) and what tests/sift_ref.py gives for them -- the
candidates, the keypoints in canonical order (no cap) and their 128-element rows -- on the fp32 pyramid of sift_ref.pyramid_f32,
the sequence the GPU runs bit for bit.

The images are anisotropic Gaussian blobs at non-integer centres over a smooth low-amplitude texture: integer-centred
symmetric blobs would put gradients exactly on the borders of the orientation bins.  Every keypoint is stored with whether
its margin (the distance of its nearest decision from flipping, sift_ref) exceeds the guard, every row element likewise.
The share of keypoints inside the guard band must not exceed 2 %: a condition on the input, asserted here and in
tests/test_sift_ref.py; the first seed for which it holds is used."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sift_ref  # noqa: E402

N, H, W = 3, 120, 160
MAX_SHARE = 0.02


def images(seed):
    from reconstructor_amd.synth import blob_image
    rng = np.random.default_rng(seed)
    out = []
    for i in range(N):
        nb = (28, 40, 52)[i]                    # the three images differ in how many keypoints they have
        blobs = [(rng.uniform(8, W - 8), rng.uniform(8, H - 8), rng.uniform(1.2, 5.0), rng.uniform(1.2, 5.0), rng.uniform(0.0, 3.1),
                  rng.uniform(30.0, 120.0) * rng.choice([-1.0, 1.0])) for _ in range(nb)]
        out.append(np.rint(blob_image(H, W, blobs, texture=4.0, seed=seed * 10 + i)).astype(np.uint8))
    return np.stack(out)


def make(seed):
    ims = images(seed)
    g = dict(images=ims)
    per = [sift_ref.detect_and_compute(sift_ref.pyramid_f32(im)) for im in ims]
    g["counts"] = np.array([r["count"] for r in per], dtype=np.int32)
    g["unsure"] = np.array([r["unsure"] for r in per], dtype=np.int32)
    g["cand_counts"] = np.array([len(r["candidates"]) for r in per], dtype=np.int32)
    g["candidates"] = np.concatenate([np.array(sorted(r["candidates"]), dtype=np.int16).reshape(-1, 4) for r in per])
    for k in ("x", "y", "size", "angle", "response", "octave", "ident", "rows"):
        g[k] = np.concatenate([r[k] for r in per])
    g["ident"] = g["ident"].astype(np.int16)
    g["sure"] = np.concatenate([r["margin"] > sift_ref.GUARD for r in per])
    g["row_sure"] = np.packbits(np.concatenate([r["row_margin"] > sift_ref.GUARD for r in per]), axis=1)
    return g


def band_share(g):
    return (float((~g["sure"]).sum()) + float(g["unsure"].sum())) / max(1, len(g["sure"]))


if __name__ == "__main__":
    for seed in range(1, 100):
        g = make(seed)
        share = band_share(g)
        print("seed %d: %s keypoints of %s candidates, %.2f %% inside the guard band" % (seed, g["counts"].tolist(), g["cand_counts"].tolist(), 100 * share))
        if share <= MAX_SHARE and g["counts"].min() > 20:
            break
    else:
        raise SystemExit("no seed keeps the guard band")
    g["seed"] = np.int32(seed)
    path = os.path.join(HERE, "sift_small.npz")
    np.savez_compressed(path, **g)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
