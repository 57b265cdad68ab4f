"""Generator of tests/golden/pnp_small.npz: the inputs of a handful of views as one rcn_pnp_ransac batch and the outputs of
tests/pnp_ref.py on them.  Run from the repository root: python tests/golden/make_pnp_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pnp_ref  # noqa: E402


def make():
    pts, views = pnp_ref.scene_views(4, 0.4, n_cams=5, n_pts=300)
    views = views + [dict(landmark=views[0]["landmark"][:3], xy=views[0]["xy"][:3], intr6=views[0]["intr6"]),
                     dict(landmark=np.full(20, 7, np.int32), xy=views[1]["xy"][:20], intr6=views[1]["intr6"])]
    off = np.zeros(len(views) + 1, np.int64)
    off[1:] = np.cumsum([len(v["landmark"]) for v in views])
    lm = np.concatenate([v["landmark"] for v in views]).astype(np.int32)
    xy = np.concatenate([v["xy"] for v in views]).astype(np.int32)
    intr = np.stack([v["intr6"] for v in views]).astype(np.float64)
    r = pnp_ref.pnp_ransac_batch(off, lm, xy, pts, intr)
    return dict(off=off, landmark=lm, xy=xy, points=pts, intr6=intr, pose34=r["pose34"], ransac_pose34=r["ransac_pose34"],
                mask=r["mask"], count=r["count"], iterations=r["iterations"])


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "pnp_small.npz"), **make())
