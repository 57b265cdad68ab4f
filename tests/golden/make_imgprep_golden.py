"""Writes tests/golden/imgprep_small.npz: seeded inputs of the image-preparation stage and what tests/img_ref.py gives for them.

    images        3 decoded BGR images of 37 x 50: two of seeded noise, one smooth gradient (a wrong weight shows on the
                  gradient, a wrong index on the noise)
    rgb, gray     img_ref.prepare(image, "bgr", 24) of each: 16 x 24; factor
    xy_int        12 keypoint slots per image (x, y): the four corners, the edges, one outside; counts = 9, 12, 15 (K above and
                  below); feat_rgba = img_ref.feat_colors
    first_img, first_feat, lm_rgba   20 landmarks, two with an index out of range
    xyz, inlier, poses34             their positions, a third of them outliers, 3 cameras; vertices = img_ref.cloud_vertices with
                  the flags, vertices_plain without
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import img_ref  # noqa: E402

N, H, W, MAX_SIZE, K, L, C = 3, 37, 50, 24, 12, 20, 3


def images(seed=11):
    rng = np.random.default_rng(seed)
    ims = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    ims[2] = np.stack([(5 * x + y) % 256, (255 - 3 * y - x) % 256, (2 * x + 4 * y) % 256], -1).astype(np.uint8)
    return ims


def rotation(w):
    t = np.linalg.norm(w)
    k = w / t
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def make():
    rng = np.random.default_rng(12)
    ims = images()
    prep = [img_ref.prepare(im, "bgr", MAX_SIZE) for im in ims]
    rgb, gray = np.stack([p[0] for p in prep]), np.stack([p[1] for p in prep])
    rows, cols = gray.shape[1:]
    xy = np.stack([rng.integers(0, cols, (N, K)), rng.integers(0, rows, (N, K))], -1).astype(np.int32)
    xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3] = (0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1)
    xy[:, 4], xy[:, 5] = (cols, 3), (5, -1)                                     # outside: zero bytes
    counts = np.array([9, 12, 15], np.int32)
    feat = np.stack([img_ref.feat_colors(rgb[i], xy[i], counts[i]) for i in range(N)])
    first_img = rng.integers(0, N, L).astype(np.int32)
    first_feat = rng.integers(0, 9, L).astype(np.int32)
    first_img[3], first_feat[7] = N, -1
    lm = img_ref.landmark_colors(feat, first_img, first_feat)
    xyz = rng.normal(size=(L, 3)) * 3 + (0, 0, 8)
    inlier = (np.arange(L) % 3 != 1).astype(np.uint8)
    poses = np.stack([np.concatenate([rotation(rng.normal(size=3) * 0.3), rng.normal(size=(3, 1))], 1).reshape(12) for _ in range(C)])
    return dict(images=ims, rgb=rgb, gray=gray, factor=np.float64(prep[0][2]), xy_int=xy, counts=counts, feat_rgba=feat,
                first_img=first_img, first_feat=first_feat, lm_rgba=lm, xyz=xyz, inlier=inlier, poses34=poses,
                vertices=img_ref.cloud_vertices(xyz, lm, inlier, poses), vertices_plain=img_ref.cloud_vertices(xyz, lm, None, poses))


if __name__ == "__main__":
    out = os.path.join(HERE, "imgprep_small.npz")
    np.savez_compressed(out, **make())
    print(out, os.path.getsize(out), "bytes")
