"""Time of rcn_sift_detect_and_compute_device (SIFT) at 512 x 384 and 480 x 640 for batches of n byte
images: HIP events on a stream of its own around the call, 3 warm-up calls, median of --reps.  Per shape and batch size it
prints the time per image, the keypoints per image, the split pyramid / detect / describe timed through the three staged
calls (on at most 25 images: their pyramids live in a buffer of the caller's, 39 MB per VGA image), and the pyramid's traffic
floor: every layer written once, read once by the blur that follows and once by the extrema stage, at 8 TB/s.  The split by kernel comes from running the same command under `rocprofv3 --kernel-trace --stats -- python
tools/sift_timing.py --reps 3 --n 25` (profiles/).  There is no OpenCV on these machines to time against, so no baseline
is given.  One JSON line stamped with the source hash.

    python tools/sift_timing.py [--reps 10] [--n 25,1000] [--shapes 512x384,480x640] [--K 4096]

Images are synthetic: anisotropic blobs over a smooth texture (reconstructor_amd.synth.blob_image), 8 distinct ones repeated."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def images(H, W, n_distinct, seed=1):
    from reconstructor_amd.synth import blob_image
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_distinct):
        blobs = [(rng.uniform(6, W - 6), rng.uniform(6, H - 6), rng.uniform(1.0, 6.0), rng.uniform(1.0, 6.0), rng.uniform(0.0, 3.1),
                  rng.uniform(30.0, 120.0) * rng.choice([-1.0, 1.0])) for _ in range(H * W // 250)]
        out.append(np.rint(blob_image(H, W, blobs, texture=4.0, seed=seed + i)).astype(np.uint8))
    return np.stack(out)


def timed(st, reps, fn):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", default="25,1000")
    ap.add_argument("--shapes", default="512x384,480x640")
    ap.add_argument("--K", type=int, default=4096)
    a = ap.parse_args()
    import ctypes as C
    import torch
    import bench
    from reconstructor_amd import _lib, sift
    ctx = _lib.Context(0)
    out = {"tool": "sift_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "K": a.K, "cases": {}}
    st = torch.cuda.Stream()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for shape in a.shapes.split(","):
        H, W = (int(v) for v in shape.split("x"))
        L = sift.layout(H, W)
        base = torch.from_numpy(images(H, W, 8)).cuda()
        written = L["floats_per_image"] * 4
        read = sum(h * w * 4 * (2 * L["n_layers"] - 1) for h, w in zip(L["oct_h"], L["oct_w"])) + H * W      # S + 2 blurs read a layer each, the extrema read all
        for n in [int(x) for x in a.n.split(",")]:
            img = base.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
            kp = sift._outputs(n, a.K, img.device)
            rows = torch.empty((n, a.K, 128), dtype=torch.float32, device="cuda")
            ns = min(n, 25)
            pyr = torch.empty((ns, L["floats_per_image"]), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ctx.check(ctx.lib.rcn_set_stream(ctx.h, st.cuda_stream))
            kpp = sift._kp_ptrs(kp)

            def whole():
                ctx.check(ctx.lib.rcn_sift_detect_and_compute_device(ctx.h, P(img), sift.INPUT_U8, H * W, W, 1, n, H, W, None, a.K, *kpp, P(rows)))

            def pyramid():
                ctx.check(ctx.lib.rcn_sift_pyramid_device(ctx.h, P(img), sift.INPUT_U8, H * W, W, 1, ns, H, W, None, P(pyr)))

            def detect():
                ctx.check(ctx.lib.rcn_sift_detect_device(ctx.h, P(pyr), ns, H, W, None, a.K, *kpp))

            def describe():
                ctx.check(ctx.lib.rcn_sift_describe_device(ctx.h, P(pyr), ns, H, W, None, a.K, P(kp["xy"]), P(kp["size"]), P(kp["angle"]), P(kp["octave"]),
                                                           P(kp["counts"]), P(rows)))

            w_ms, w_min = timed(st, a.reps, whole)
            cnt = kp["counts"].cpu().numpy()
            p_ms, _ = timed(st, a.reps, pyramid)
            d_ms, _ = timed(st, a.reps, detect)
            r_ms, _ = timed(st, a.reps, describe)
            ctx.check(ctx.lib.rcn_set_stream(ctx.h, None))
            out["cases"]["%s_n%d" % (shape, n)] = {
                "n": n, "H": H, "W": W, "us_per_image": round(1e3 * w_ms / n, 2), "us_per_image_min": round(1e3 * w_min / n, 2),
                "staged_images": ns, "pyramid_us_per_image": round(1e3 * p_ms / ns, 2), "detect_us_per_image": round(1e3 * d_ms / ns, 2),
                "describe_us_per_image": round(1e3 * r_ms / ns, 2),
                "keypoints_per_image": [int(cnt.min()), float(cnt.mean()), int(cnt.max())],
                "pyramid_mb_per_image": round(written / 1e6, 2),
                "pyramid_traffic_floor_us_per_image": round(1e6 * (written + read) / 8e12, 2)}
            del img, kp, rows, pyr
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
