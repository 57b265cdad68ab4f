"""Time of rcn_img_prepare_device (image preparation) for n = 25 and n = 200 photographs of 2048 x 3072 x 3
and n = 1000 of 1024 x 1536 x 3, all to 336 x 512, the images resident in HBM: HIP events on a stream of its own around the call,
3 warm-up calls, median of --reps.  Per case it prints the time per image, the traffic floor -- the bytes of the source lines the
tables actually touch plus the output, at 8 TB/s -- and the fraction of that rate the time implies; beside them, for the time
only, the same resize in eager torch on the same GPU (F.interpolate, bilinear, on float planes that are already converted: its
values differ) and tests/img_ref.py's prepare of one image on the CPU.  The colour and cloud kernels are timed once, at K = 2000
keypoints per image and L = 100 000 landmarks.  One JSON line stamped with the source hash.

    python tools/img_prepare_timing.py [--reps 20] [--cases 25x2048x3072,200x2048x3072,1000x1024x1536] [--max-size 512]

Images are seeded noise generated on the device: the kernel's time does not depend on the pixel values."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8e12


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


def touched_source_rows(imgprep, H, rows):
    s, _, _ = imgprep.resize_tables(H, rows, horizontal=False)
    return len(np.union1d(np.clip(s, 0, H - 1), np.clip(s + 1, 0, H - 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default="25x2048x3072,200x2048x3072,1000x1024x1536")
    ap.add_argument("--max-size", type=int, default=512)
    a = ap.parse_args()
    import ctypes as C
    import torch
    import torch.nn.functional as F
    import bench
    import img_ref
    from reconstructor_amd import _lib, imgprep
    ctx = _lib.Context(0)
    out = {"tool": "img_prepare_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "cases": {}}
    st = torch.cuda.Stream()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    gen = torch.Generator(device="cuda").manual_seed(1)
    for case in a.cases.split(","):
        n, H, W = (int(v) for v in case.split("x"))
        rows, cols, _ = imgprep.reshape_size(H, W, a.max_size)
        src = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
        rgb = torch.empty((n, rows, cols, 3), dtype=torch.uint8, device="cuda")
        gray = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")
        opt = imgprep.options()
        torch.cuda.synchronize()
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, st.cuda_stream))

        def prepare():
            ctx.check(ctx.lib.rcn_img_prepare_device(ctx.h, P(src), H * W * 3, W * 3, 3, n, H, W, rows, cols, C.byref(opt), P(rgb), P(gray)))

        ms, ms_min = timed(st, a.reps, prepare)
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, None))
        nt = min(n, 25)
        planes = src[:nt].permute(0, 3, 1, 2).float().contiguous()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            t_ms, _ = timed(st, a.reps, lambda: F.interpolate(planes, size=(rows, cols), mode="bilinear", antialias=False))
        del planes
        one = src[0].cpu().numpy()
        t0 = time.perf_counter()
        ref_rgb, ref_gray, _ = img_ref.prepare(one, "bgr", a.max_size)
        cpu_s = time.perf_counter() - t0
        same = bool(np.array_equal(rgb[0].cpu().numpy(), ref_rgb) and np.array_equal(gray[0].cpu().numpy(), ref_gray))
        floor_bytes = touched_source_rows(imgprep, H, rows) * W * 3 + rows * cols * 4
        us = 1e3 * ms / n
        out["cases"][case] = {
            "n": n, "src": [H, W], "dst": [rows, cols], "plan": imgprep.plan(W, cols), "us_per_image": round(us, 3), "us_per_image_min": round(1e3 * ms_min / n, 3),
            "source_mb_per_image": round(H * W * 3 / 1e6, 2), "floor_mb_per_image": round(floor_bytes / 1e6, 3),
            "floor_us_per_image": round(1e6 * floor_bytes / HBM_BYTES_PER_S, 3), "fraction_of_hbm_rate": round(floor_bytes / HBM_BYTES_PER_S / (us * 1e-6), 4),
            "torch_interpolate_us_per_image": round(1e3 * t_ms / nt, 3), "torch_images": nt, "cpu_reference_ms_per_image": round(1e3 * cpu_s, 1),
            "equals_reference": same}
        del src, rgb, gray
    # the gathers, once
    n, K, L, Cn, rows, cols = 25, 2000, 100000, 1000, 336, 512
    rgb = torch.randint(0, 256, (n, rows, cols, 3), dtype=torch.uint8, device="cuda", generator=gen)
    xy = torch.stack([torch.randint(0, cols, (n, K), device="cuda", generator=gen), torch.randint(0, rows, (n, K), device="cuda", generator=gen)], -1).int().contiguous()
    counts = torch.full((n,), K, dtype=torch.int32, device="cuda")
    feat = torch.empty((n, K, 4), dtype=torch.uint8, device="cuda")
    fi = torch.randint(0, n, (L,), device="cuda", generator=gen).int()
    ff = torch.randint(0, K, (L,), device="cuda", generator=gen).int()
    lm = torch.empty((L, 4), dtype=torch.uint8, device="cuda")
    xyz = torch.randn((L, 3), dtype=torch.float64, device="cuda", generator=gen)
    inl = (torch.arange(L, device="cuda") % 3 != 0).to(torch.uint8)
    poses = torch.randn((Cn, 12), dtype=torch.float64, device="cuda", generator=gen)
    verts = torch.empty((2 * L + Cn, 16), dtype=torch.uint8, device="cuda")
    nv = C.c_int64()
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_set_stream(ctx.h, st.cuda_stream))
    f_ms, _ = timed(st, a.reps, lambda: ctx.check(ctx.lib.rcn_feat_colors_device(ctx.h, P(rgb), n, rows, cols, P(xy), P(counts), K, P(feat))))
    l_ms, _ = timed(st, a.reps, lambda: ctx.check(ctx.lib.rcn_landmark_colors_device(ctx.h, P(feat), n, K, L, P(fi), P(ff), P(lm))))
    c_ms, _ = timed(st, a.reps, lambda: ctx.check(ctx.lib.rcn_cloud_vertices_device(ctx.h, P(xyz), P(lm), P(inl), L, P(poses), Cn, P(verts), C.byref(nv))))
    ctx.check(ctx.lib.rcn_set_stream(ctx.h, None))
    out["gathers"] = {"n": n, "K": K, "L": L, "C": Cn, "feat_colors_us": round(1e3 * f_ms, 2), "landmark_colors_us": round(1e3 * l_ms, 2),
                      "cloud_vertices_us": round(1e3 * c_ms, 2), "vertices": nv.value}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
