"""Device time of rcn_pnp_ransac_device (view registration), HIP events on a stream of its own around
the call, 3 warm-up calls, median of --reps; prints one JSON line stamped with the source hash.

    python tools/pnp_timing.py [--reps 30] [--cases one,cand13,cand13_single,big,huge]

Views are generated in numpy from a seed: scene points uniform in a cube, a camera looking at it, pixels truncated to
integers with 0.5 px noise, a share w of the entries given a random other landmark.  The sizes follow the next-view cases
(tools/next_view_timing.py): one candidate of the 25-image case (~2000 entries), its 13 candidates in one call and as 13
calls, 500 candidates x 25 000 entries (w = 0.3), one 25 000-entry view at w = 0.6.
Per case: ms, iterations, entry projections (iterations x entries: every hypothesis scored to the end, the work without
pruning) and their rate against the fp64 vector peak of the CUs in use (one CU per view; 38 flop per projection).  With
RCN_LIB pointing at the diagnostic build the case is also timed with RCN_PNP_PRUNE=0: what the exact pruning removes."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VECTOR_PEAK = 78.6e12      # MI355X data sheet, 256 CUs
FLOP_PER_PROJECTION = 38


def make_views(nv, n, w, n_pts, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, (n_pts, 3))
    K = np.array([600.0, 600.0, 256.0, 168.0, 0.0, 0.0])
    lm, xy = [], []
    for v in range(nv):
        a = rng.normal(0, 0.2, 3)
        th = np.linalg.norm(a)
        k = a / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        t = np.array([0, 0, 5.0]) + rng.normal(0, 0.3, 3)
        l = rng.integers(0, n_pts, n)
        c = pts[l] @ R.T + t
        p = np.trunc(np.stack([K[0] * c[:, 0] / c[:, 2] + K[2], K[1] * c[:, 1] / c[:, 2] + K[3]], 1) + rng.normal(0, 0.5, (n, 2)))
        bad = rng.random(n) < w
        l[bad] = rng.integers(0, n_pts, int(bad.sum()))
        lm.append(l.astype(np.int32))
        xy.append(p.astype(np.int32))
    return pts, lm, xy, np.tile(K, (nv, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cases", default="one,cand13,cand13_single,big,huge")
    a = ap.parse_args()
    import torch
    import bench
    from reconstructor_amd import _lib
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    diag = b"DIAGNOSTIC" in ctx.lib.rcn_version()
    cfg = {"one": (1, 2000, 0.1, 3000, 1), "cand13": (13, 2000, 0.1, 3000, 2), "cand13_single": (13, 2000, 0.1, 3000, 2),
           "big": (500, 25000, 0.3, 330000, 3), "huge": (1, 25000, 0.6, 330000, 4)}
    out = {"tool": "pnp_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "diagnostic_build": diag, "cases": {}}
    st = torch.cuda.Stream()
    for name in a.cases.split(","):
        nv, n, w, n_pts, seed = cfg[name]
        pts, lm, xy, K = make_views(nv, n, w, n_pts, seed)
        for v in range(nv):
            ctx.check(ctx.lib.rcn_coords_upload(ctx.h, v, xy[v].ctypes.data, n))
        t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dt)).to(dev)
        X, K_d = t(pts, np.float64), t(K, np.float64)
        lm_d = t(np.concatenate(lm), np.int32)
        ft_d = t(np.tile(np.arange(n, dtype=np.int32), nv), np.int32)
        img_d = t(np.arange(nv), np.int32)
        off_d = t(np.arange(nv + 1, dtype=np.int64) * n, np.int64)
        off1_d = t([0, n], np.int64)
        pose = torch.zeros((nv, 12), dtype=torch.float64, device=dev)
        rpose = torch.zeros((nv, 12), dtype=torch.float64, device=dev)
        mask = torch.zeros(nv * n, dtype=torch.uint8, device=dev)
        cnt = torch.zeros(nv, dtype=torch.int32, device=dev)
        its = torch.zeros(nv, dtype=torch.int32, device=dev)

        def call():
            if name.endswith("_single"):          # the same views, one call each
                for v in range(nv):
                    ctx.check(ctx.lib.rcn_pnp_ransac_device(ctx.h, 1, off1_d.data_ptr(), lm_d.data_ptr() + 4 * v * n, ft_d.data_ptr(),
                                                            img_d.data_ptr() + 4 * v, n_pts, X.data_ptr(), K_d.data_ptr() + 48 * v, None,
                                                            pose.data_ptr() + 96 * v, rpose.data_ptr() + 96 * v, mask.data_ptr() + v * n,
                                                            cnt.data_ptr() + 4 * v, its.data_ptr() + 4 * v))
            else:
                ctx.check(ctx.lib.rcn_pnp_ransac_device(ctx.h, nv, off_d.data_ptr(), lm_d.data_ptr(), ft_d.data_ptr(), img_d.data_ptr(), n_pts,
                                                        X.data_ptr(), K_d.data_ptr(), None, pose.data_ptr(), rpose.data_ptr(), mask.data_ptr(),
                                                        cnt.data_ptr(), its.data_ptr()))

        def measure():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = []
            for _ in range(a.reps):
                e0.record(st)
                call()
                e1.record(st)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return float(np.median(ms)), float(np.min(ms))

        torch.cuda.synchronize()
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, st.cuda_stream))
        med, mn = measure()
        it, c = its.cpu().numpy(), cnt.cpu().numpy()
        proj = int(it.astype(np.int64).sum()) * n
        cus = min(nv, 256) if not name.endswith("_single") else 1
        r = {"views": nv, "entries_per_view": n, "wrong_share": w, "ms_median": round(med, 4), "ms_min": round(mn, 4),
             "iterations_max": int(it.max()), "iterations_sum": int(it.sum()), "inliers_min": int(c.min()),
             "projections_unpruned": proj, "gproj_per_s": round(proj / med / 1e6, 2),
             "frac_fp64_vector_peak_of_cus_in_use": round(proj * FLOP_PER_PROJECTION / (med * 1e-3) / (FP64_VECTOR_PEAK * cus / 256), 4)}
        if diag:
            os.environ["RCN_PNP_PRUNE"] = "0"
            r["ms_median_no_pruning"] = round(measure()[0], 4)
            del os.environ["RCN_PNP_PRUNE"]
        out["cases"][name] = r
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, None))
        ctx.check(ctx.lib.rcn_coords_clear(ctx.h))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
