"""Milliseconds per call of batched multi-view triangulation (csrc/triangulate.hip) through its three entries, and the
numpy-SVD restatement of the reference's steps (tests/tri_ref.py) as the CPU figure.  Prints one JSON line.

    python tools/triangulate_timing.py [--reps N]

Cases: 4096 two-view tracks (one new view's worth), 100k tracks of 2..8 views, 1M two-view tracks (synth_ba scenes,
camera 0 at the identity).  host = rcn_triangulate (upload, launches, download); device = rcn_triangulate_device on
arrays already in HBM, compaction included; session = rcn_ba_session_triangulate (appending to a session).  Median of
--reps calls after one warm-up call each."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    ts.sort()
    return round(ts[len(ts) // 2], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import tri_ref
    from reconstructor_amd import _lib, ba
    from reconstructor_amd import triangulate as tri
    import ctypes as C

    ctx = _lib.Context(0)
    cases = {"4k_2view": (25, 4096, 2, 2), "100k_2to8": (25, 100_000, 2, 8), "1M_2view": (25, 1 << 20, 2, 2)}
    out = {"tool": "triangulate_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "ms": {}}
    for name, (nc, nt, lo, hi) in cases.items():
        c = tri_ref.make_tracks(nc, nt, lo, hi, seed=7)
        flat = {k: c[k] for k in ("poses34", "intrinsics", "trk_off", "obs_cam", "obs_xy")}
        r = {}
        xyz, st = tri.triangulate_tracks(ctx, **flat)
        r["accepted"] = int((st == 0).sum())
        r["host"] = _median_ms(lambda: tri.triangulate_tracks(ctx, **flat), args.reps)
        dev = torch.device("cuda", 0)
        P = torch.from_numpy(np.ascontiguousarray(flat["poses34"])).to(dev)
        K = torch.from_numpy(np.ascontiguousarray(flat["intrinsics"])).to(dev)
        off = torch.from_numpy(flat["trk_off"]).to(dev)
        cam = torch.from_numpy(flat["obs_cam"]).to(dev)
        xy = torch.from_numpy(flat["obs_xy"]).to(dev)
        X = torch.empty((nt, 3), dtype=torch.float64, device=dev)
        S = torch.empty(nt, dtype=torch.uint8, device=dev)
        comp = torch.empty((nt, 3), dtype=torch.float64, device=dev)
        cnt = torch.empty(1, dtype=torch.int32, device=dev)
        pb = _lib.TriangulationProblem(len(P), nt, cam.numel(), 0, P.data_ptr(), K.data_ptr(), off.data_ptr(), cam.data_ptr(), xy.data_ptr())
        torch.cuda.synchronize()

        def device_call():
            ctx.check(ctx.lib.rcn_triangulate_device(ctx.h, C.byref(pb), 4.0, 1.0, X.data_ptr(), S.data_ptr(), comp.data_ptr(), 0, cnt.data_ptr()))
            ctx.check(ctx.lib.rcn_synchronize(ctx.h))
        r["device"] = _median_ms(device_call, args.reps)
        assert int(cnt.cpu()[0]) == r["accepted"]
        ses = ba.BaSession(ctx)
        try:
            for p, k in zip(flat["poses34"], flat["intrinsics"]):
                ses.add_camera(np.concatenate([ba._rot_to_angle_axis(p.reshape(3, 4)[:, :3]), p.reshape(3, 4)[:, 3]]), k)
            r["session"] = _median_ms(lambda: ses.triangulate(flat["trk_off"], flat["obs_cam"], flat["obs_xy"], poses34=flat["poses34"]),
                                      min(args.reps, 3))
        finally:
            ses.close()
        t = time.perf_counter()
        tri_ref.numpy_tracks(**flat)
        r["numpy_cpu"] = round(1e3 * (time.perf_counter() - t), 1)
        out["ms"][name] = r
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
