"""Writes tests/golden/mvs_small.npz: small ray-cast scenes with the contract's answer (tests/mvs_ref.py), so that a change of the
contract shows up as a diff.  Run from the repository root:  python tests/golden/make_mvs_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mvs_ref as M  # noqa: E402


def main():
    cases = {}
    sc, inv = M.small_case(24, 40, n=3, D=6)
    cases["wall_40x24"] = (sc, M.all_views(3, 2), np.tile(inv, (3, 1)), dict(radius=2, min_sources=1, min_consistent=1), -1)
    sc, inv = M.small_case(17, 33, n=4, D=3, seed=2)
    cases["wall_33x17_stride2"] = (sc, M.all_views(4, 3), np.tile(inv, (4, 1)), dict(radius=1, min_sources=2, min_consistent=1, stride=2), 60)
    sc, inv = M.small_case(30, 36, n=3, D=8, seed=4)
    sc["intrinsics"][:, 4:] = 0.05, -0.01
    inv2 = np.stack([inv, inv[::-1], np.repeat(inv[2:6], 2)])
    cases["distorted_ties_36x30"] = (sc, np.array([[0, 1, 2], [1, 2, 0], [2, 0, -1]], np.int32), inv2, dict(radius=3, min_sources=1, min_consistent=1, max_cost=0.3, rel_tol=0.02), -1)
    out = {}
    for name, (sc, views, inv, opt, cap) in cases.items():
        o = dict(M.DEFAULTS, **opt)
        r = M.dense_cloud(sc["poses34"], sc["intrinsics"], sc["gray"], sc["rgb"], views, inv, capacity=None if cap < 0 else cap, **o)
        out.update({name + ".poses34": sc["poses34"], name + ".intrinsics": sc["intrinsics"], name + ".gray": sc["gray"], name + ".rgb": sc["rgb"],
                    name + ".views": np.asarray(views, np.int32), name + ".inv": inv,
                    name + ".iopt": np.array([o["radius"], o["min_sources"], o["min_consistent"], o["stride"]], np.int32),
                    name + ".fopt": np.array([o["max_cost"], o["rel_tol"]]), name + ".capacity": np.array(cap, np.int64),
                    name + ".fused": np.array([r["written"], r["total"]], np.int64)})
        for k in ("plane", "depth", "cost", "mask", "counts", "vertices"):
            out[name + "." + k] = r[k]
        print(name, "valid", int((r["plane"] >= 0).sum()), "kept", r["counts"].tolist(), "fused", r["written"], r["total"])
    np.savez_compressed(os.path.join(HERE, "mvs_small.npz"), **out)


if __name__ == "__main__":
    main()
