"""Time of rcn_twoview_init (two-view initialisation): HIP events on a stream of its own around the
call (the host entry: its copies in and out are inside the interval), 3 warm-up calls, median of --reps; next to it the time
of the numpy restatement (tests/twoview_ref.py, one run) on the same inputs.  Prints one JSON line stamped with the source
hash.

    python tools/twoview_timing.py [--reps 30] [--cases pair269,pair2000,top8,w06]

Pairs are generated in numpy from a seed (tests/twoview_ref.scene_pair: a random relative pose, points 3 .. 8 in front of
the first camera, pixels truncated to integers, a share w of the second image's pixels random).  pair269 has the size of
the 25-image loop's initial pair, pair2000 a dense pair (the LDS path's limit is 2048 entries), top8 eight pairs of 1000
entries in one call (a caller trying its top-m pairs), w06 one pair of 1500 entries at w = 0.6 (close to the iteration cap)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cases", default="pair269,pair2000,top8,w06")
    ap.add_argument("--no-ref", action="store_true", help="skip the numpy restatement")
    a = ap.parse_args()
    import torch
    import bench
    import twoview_ref as tv
    from reconstructor_amd import _lib, twoview
    ctx = _lib.Context(0)
    cfg = {"pair269": (1, 269, 0.1, 1), "pair2000": (1, 2000, 0.2, 2), "top8": (8, 1000, 0.3, 3), "w06": (1, 1500, 0.6, 4)}
    out = {"tool": "twoview_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "cases": {}}
    st = torch.cuda.Stream()
    for name in a.cases.split(","):
        npairs, n, w, seed = cfg[name]
        sc = [tv.scene_pair(1000 * seed + p, w, n=n) for p in range(npairs)]
        off = np.arange(npairs + 1, dtype=np.int64) * n
        xy1, xy2 = np.concatenate([s["xy1"] for s in sc]), np.concatenate([s["xy2"] for s in sc])
        K1, K2 = np.stack([s["K1"] for s in sc]), np.stack([s["K2"] for s in sc])
        torch.cuda.synchronize()
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, st.cuda_stream))
        for _ in range(3):
            r = twoview.two_view_init(ctx, off, xy1, xy2, K1, K2)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(a.reps):
            e0.record(st)
            r = twoview.two_view_init(ctx, off, xy1, xy2, K1, K2)
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, None))
        c = {"pairs": npairs, "entries_per_pair": n, "wrong_share": w, "ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4),
             "iterations": r["iterations"].tolist(), "inliers": r["count"][:, 0].tolist(), "in_front": r["count"][:, 1].tolist()}
        if not a.no_ref:
            t0 = time.perf_counter()
            want = tv.two_view_init_batch(off, xy1, xy2, K1, K2)
            c["numpy_restatement_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            c["equal_bits"] = all(np.asarray(r[k]).tobytes() == np.asarray(want[k]).astype(np.asarray(r[k]).dtype).tobytes()
                                  for k in ("E", "pose34", "mask", "cheir_mask", "count", "iterations"))
        out["cases"][name] = c
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
