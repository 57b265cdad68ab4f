"""Time of rcn_orb_detect_and_compute_device (ORB) at 512 x 384 and 480 x 640 for batches of n byte
images: HIP events on a stream of its own around the call, 3 warm-up calls, median of --reps, as tools/sift_timing.py.  Per
shape and batch size it reports the time per image, the keypoints per image, the split pyramid / detect / describe timed
through the three staged calls (on at most 25 images), and the pyramid's traffic floor at 8 TB/s: every level written once;
every level that yields keypoints read by FAST, by the blur and by describe; its blurred copy written and read once.  It also times rcn_sift_detect_and_compute_device on the same images in the same run.  There is
no OpenCV on these machines to time against, so no baseline is given and no time is a pass condition.  Writes one JSON
document, stamped with the source hash, to profiles/orb_timing.json (and prints it).

    python tools/orb_timing.py [--reps 5] [--n 25,1000] [--shapes 512x384,480x640] [--K 4096] [--out profiles/orb_timing.json]

Images are synthetic: turned rectangles of random grey levels over mild noise, 8 distinct ones repeated."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def images(H, W, n_distinct, seed=1):
    out = []
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for i in range(n_distinct):
        rng = np.random.default_rng(seed + i)
        img = np.full((H, W), 110.0)
        for _ in range(H * W // 500):
            cx, cy, a, b, t = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(4, 30), rng.uniform(4, 30), rng.uniform(0, math.pi)
            u = (xx - cx) * math.cos(t) + (yy - cy) * math.sin(t)
            v = -(xx - cx) * math.sin(t) + (yy - cy) * math.cos(t)
            img[(np.abs(u) < a) & (np.abs(v) < b)] = rng.uniform(10, 245)
        img += rng.integers(-2, 3, size=(H, W))
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", default="25,1000")
    ap.add_argument("--shapes", default="512x384,480x640")
    ap.add_argument("--K", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orb_timing.json"))
    a = ap.parse_args()
    import ctypes as C
    import torch
    import bench
    from reconstructor_amd import _lib, orb, sift
    ctx = _lib.Context(0)
    out = {"tool": "orb_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "K": a.K, "cases": {}}
    st = torch.cuda.Stream()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for shape in a.shapes.split(","):
        H, W = (int(v) for v in shape.split("x"))
        L = orb.layout(H, W)
        base = torch.from_numpy(images(H, W, 8)).cuda()
        px = [h * w for h, w in zip(L["level_h"], L["level_w"])]
        act = [p for p, on in zip(px, L["active"]) if on]
        # every level: 1 write; a level with keypoints: read by FAST, blur and describe; its blurred copy: 1 write + 1 read
        traffic = sum(px) + 3 * sum(act) + 2 * sum(act)
        for n in [int(x) for x in a.n.split(",")]:
            img = base.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
            kp = orb._outputs(n, a.K, img.device)
            rows = torch.empty((n, a.K, 32), dtype=torch.float32, device="cuda")
            srows = torch.empty((n, a.K, 128), dtype=torch.float32, device="cuda")
            ns = min(n, 25)
            pyr = torch.empty((ns, L["bytes_per_image"]), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.check(ctx.lib.rcn_set_stream(ctx.h, st.cuda_stream))
            kpp = orb._kp_ptrs(kp)

            def whole():
                ctx.check(ctx.lib.rcn_orb_detect_and_compute_device(ctx.h, P(img), orb.INPUT_U8, H * W, W, 1, n, H, W, None, a.K, *kpp, P(rows), None))

            def pyramid():
                ctx.check(ctx.lib.rcn_orb_pyramid_device(ctx.h, P(img), orb.INPUT_U8, H * W, W, 1, ns, H, W, None, P(pyr)))

            def detect():
                ctx.check(ctx.lib.rcn_orb_detect_device(ctx.h, P(pyr), ns, H, W, None, a.K, *kpp))

            def describe():
                ctx.check(ctx.lib.rcn_orb_describe_device(ctx.h, P(pyr), ns, H, W, None, a.K, P(kp["xy"]), P(kp["octave"]), P(kp["counts"]), P(rows), None))

            def sift_whole():
                ctx.check(ctx.lib.rcn_sift_detect_and_compute_device(ctx.h, P(img), sift.INPUT_U8, H * W, W, 1, n, H, W, None, a.K, *kpp, P(srows)))

            w_ms, w_min = timed(st, a.reps, whole)
            cnt = kp["counts"].cpu().numpy()
            p_ms, _ = timed(st, a.reps, pyramid)
            d_ms, _ = timed(st, a.reps, detect)
            r_ms, _ = timed(st, a.reps, describe)
            s_ms, _ = timed(st, a.reps, sift_whole)
            scnt = kp["counts"].cpu().numpy()
            ctx.check(ctx.lib.rcn_set_stream(ctx.h, None))
            out["cases"]["%s_n%d" % (shape, n)] = {
                "n": n, "H": H, "W": W, "us_per_image": round(1e3 * w_ms / n, 2), "us_per_image_min": round(1e3 * w_min / n, 2),
                "staged_images": ns, "pyramid_us_per_image": round(1e3 * p_ms / ns, 2), "detect_us_per_image": round(1e3 * d_ms / ns, 2),
                "describe_us_per_image": round(1e3 * r_ms / ns, 2),
                "keypoints_per_image": [int(cnt.min()), float(cnt.mean()), int(cnt.max())],
                "pyramid_kb_per_image": round(L["bytes_per_image"] / 1e3, 1),
                "traffic_floor_us_per_image": round(1e6 * traffic / 8e12, 3),
                "sift_us_per_image": round(1e3 * s_ms / n, 2), "sift_keypoints_per_image": [int(scnt.min()), float(scnt.mean()), int(scnt.max())]}
            del img, kp, rows, srows, pyr
    ctx.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
