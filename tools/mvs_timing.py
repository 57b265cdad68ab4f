"""Times of the dense stage on ray-cast scenes: 25 views of 336 x 512 (the prepared size of the reference's
fountain photographs) and of 480 x 640, D = 128 planes, S = 4 sources, R = 3.  HIP events on a stream of its own around each phase,
one warm-up call first, median / min / max of --reps.

It records per case
    views_ms          rcn_ba_session_mvs_views (sources and depth ranges of all cameras; waits, so the host round trip is inside)
    undistort_ms      rcn_img_undistort_device, grey and colour planes
    sweep_ms          rcn_mvs_sweep_device, all views in one launch
    consistency_ms    rcn_mvs_consistency_device
    fuse_ms           rcn_mvs_fuse_device (stride 1)
    samples           pixels x D x S, and sweep_ns_per_sample
    floor_ms          the arithmetic floor of section 32: samples x 18 separately rounded fp64 operations at the vector fp64 rate without
                      FMA (39.3e12 / s), and samples x 4 source bytes at 8 TB/s; sweep_over_floor
    contract_s        the numpy contract (tests/mvs_ref.py) on the host for ONE view and --contract-planes planes of the same input, and
                      contract_s_scaled, that time scaled to all views and planes; contract_over_sweep
Nothing here is a pass condition.  Writes one JSON document, stamped with the source hash, to profiles/mvs_timing.json (and prints it).

    python tools/mvs_timing.py [--views 25] [--planes 128] [--sources 4] [--reps 5] [--out profiles/mvs_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_OPS_PER_SAMPLE = 18           # w, u, v: 6 products + 6 sums; 2 quotients; 2 products + 2 sums + 2 floors of the 1/32 grid
FP64_OPS_PER_S = 39.3e12           # MI355X vector fp64 without FMA (half of the 78.6 TFLOP/s that count an FMA as two)
BYTES_PER_S = 8.0e12


def timed(st, reps, fn):
    import torch
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median=round(float(np.median(ms)), 3), min=round(float(np.min(ms)), 3), max=round(float(np.max(ms)), 3))


def case(ctx, st, rows, cols, a):
    import torch
    import mvs_ref
    from reconstructor_amd import ba, mvs, synth_ba, synth_mvs
    lib, h = ctx.lib, ctx.h
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    n, D, S = a.views, a.planes, a.sources
    sc = synth_mvs.wall_scene(n, rows, cols, 1.2 * cols, (0.25, 0.1, 1.0), 5.0, baseline=0.12)
    ses = ba.BaSession(ctx)
    for i in range(n):
        R = sc["poses34"][i].reshape(3, 4)
        ses.add_camera(np.concatenate([synth_ba.rot_to_angle_axis(R[:, :3]), R[:, 3]]), sc["intrinsics"][i])
    rng = np.random.default_rng(1)
    L = 4000
    xy = np.c_[rng.uniform(-1.5, 1.5, L), rng.uniform(-1.0, 1.0, L)]
    pts = np.c_[xy, 5.0 - 0.25 * xy[:, 0] - 0.1 * xy[:, 1]]
    ses.add_points(pts)
    seen = np.stack([np.sort(rng.choice(n, 6, replace=False)) for _ in range(L)])
    ses.add_observations(np.repeat(np.arange(L), 6), seen.reshape(-1), np.zeros((6 * L, 2), np.int32))
    P34 = ba.poses34_from_angle_axis(ses.cameras()[0])
    r = {"rows": rows, "cols": cols, "views": n, "planes": D, "sources": S, "radius": 3}
    src, rngs = mvs.session_views(ses, S, P34)
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        mvs.session_views(ses, S, P34)
        t.append(1e3 * (time.perf_counter() - t0))
    r["views_ms"] = dict(median=round(float(np.median(t)), 3), min=round(min(t), 3), max=round(max(t), 3))
    views = np.ascontiguousarray(np.c_[np.arange(n), src], np.int32)
    inv = np.stack([mvs.inv_depths(lo / 1.25, hi * 1.25, D) for lo, hi in rngs])
    H = mvs.view_homographies(P34, sc["intrinsics"], views, inv)
    gray, rgb = torch.as_tensor(sc["gray"]).cuda(), torch.as_tensor(sc["rgb"]).cuda()
    g2, c2 = torch.empty_like(gray), torch.empty_like(rgb)
    Kd, Pd, Hd, invd = (torch.as_tensor(x).cuda() for x in (sc["intrinsics"], P34, H, inv))
    px = n * rows * cols
    plane = torch.empty(px, dtype=torch.int16, device="cuda")
    depth, cost = torch.empty(px, dtype=torch.float32, device="cuda"), torch.empty(px, dtype=torch.float32, device="cuda")
    mask, counts = torch.empty(px, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    vert, fused = torch.empty((px, 16), dtype=torch.uint8, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    opt = mvs.options(radius=3)
    torch.cuda.synchronize()
    ctx.check(lib.rcn_set_stream(h, st.cuda_stream))
    vp = views.ctypes.data

    def undistort():
        ctx.check(lib.rcn_img_undistort_device(h, P(gray), rows * cols, cols, 1, n, rows, cols, P(Kd), P(g2)))
        ctx.check(lib.rcn_img_undistort_device(h, P(rgb), rows * cols * 3, cols * 3, 3, n, rows, cols, P(Kd), P(c2)))

    r["undistort_ms"] = timed(st, a.reps, undistort)
    r["sweep_ms"] = timed(st, a.reps, lambda: ctx.check(lib.rcn_mvs_sweep_device(h, P(g2), rows * cols, cols, n, rows, cols, vp, n, S, P(Hd), P(invd), D, C.byref(opt),
                                                                                  P(plane), P(depth), P(cost))))
    r["consistency_ms"] = timed(st, a.reps, lambda: ctx.check(lib.rcn_mvs_consistency_device(h, vp, n, S, P(Pd), P(Kd), n, rows, cols, P(plane), P(depth), C.byref(opt),
                                                                                              P(mask), P(counts))))
    r["fuse_ms"] = timed(st, a.reps, lambda: ctx.check(lib.rcn_mvs_fuse_device(h, vp, n, S, P(Pd), P(Kd), n, P(c2), rows, cols, P(depth), P(mask), C.byref(opt), px,
                                                                                P(vert), P(fused))))
    st.synchronize()
    ctx.check(lib.rcn_set_stream(h, None))
    true = np.stack([mvs_ref.true_depths(sc, v) for v in range(n)])
    d, m = depth.cpu().numpy().reshape(n, rows, cols), mask.cpu().numpy().reshape(n, rows, cols).astype(bool)
    r["valid_share"] = round(float((plane.cpu().numpy() >= 0).mean()), 4)
    r["kept_share"] = round(float(m.mean()), 4)
    r["vertices"] = int(fused[0].item())
    r["kept_median_abs_depth_error"] = float("%.3g" % np.median(np.abs(d[m] - true[m]))) if m.any() else None
    r["samples"] = px * D * S
    r["sweep_ns_per_sample"] = float("%.3g" % (1e6 * r["sweep_ms"]["median"] / r["samples"]))
    r["floor_ms"] = round(1e3 * max(r["samples"] * FP64_OPS_PER_SAMPLE / FP64_OPS_PER_S, r["samples"] * 4 / BYTES_PER_S), 3)
    r["sweep_over_floor"] = round(r["sweep_ms"]["median"] / r["floor_ms"], 1)
    if a.contract_planes > 0:
        k = min(a.contract_planes, D)
        und = np.stack([mvs_ref.undistort(sc["gray"][i], sc["intrinsics"][i]) for i in range(n)])
        t0 = time.perf_counter()
        want = mvs_ref.sweep_view(und, int(views[0, 0]), [int(s) for s in views[0, 1:]], H[0][:, :k], inv[0][:k], radius=3)
        r["contract_s"] = round(time.perf_counter() - t0, 3)
        r["contract_planes"] = k
        r["contract_s_scaled"] = round(r["contract_s"] * (D / k) * n, 1)
        r["contract_over_sweep"] = round(1e3 * r["contract_s_scaled"] / r["sweep_ms"]["median"], 0)
        one = mvs.sweep(ctx, g2, views[:1], H[:1, :, :k], inv[:1, :k], opt)
        r["contract_equal"] = bool(all(np.array_equal(x.cpu().numpy()[0].view(np.uint8), y.view(np.uint8)) for x, y in zip(one, want)))
    ses.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=25)
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--contract-planes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvs_timing.json"))
    a = ap.parse_args()
    import torch
    import bench
    from reconstructor_amd import _lib, mvs
    ctx = _lib.Context(0)
    st = torch.cuda.Stream()
    doc = {"tool": "mvs_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "warm_up": 1,
           "layout": mvs.layout(336, 512, a.views, a.planes, a.sources)}
    doc["fountain_336x512"] = case(ctx, st, 336, 512, a)
    doc["vga_480x640"] = case(ctx, st, 480, 640, a)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
