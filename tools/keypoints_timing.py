"""Time of rcn_kp_detect_device (keypoint extraction) at 480 x 640 for batches of n images: HIP
events on a stream of its own around the call, 3 warm-up calls, median of --reps.  Per batch size it prints the time per
image, the NMS rounds per image, and the share of the time in the two halves that can be timed from outside -- the heat
stage (k_kp_plane / k_kp_cell + k_kp_heat) and the exact stages (k_kp_threshold + k_kp_nms, timed through rcn_kp_nms_device
on the heat map the first call returned) -- next to the numpy greedy loop of tests/kp_ref.py on one image of the same batch
and the traffic floor (1.25 MB of logits in, keypoints out, + 1.2 MB when the heat map is requested, at 8 TB/s).  The
split by kernel comes from running the same command under `rocprofv3 --kernel-trace --stats -- python tools/keypoints_timing.py
--reps 3 --n 25` (profiles/).  One JSON line stamped with the source hash.

    python tools/keypoints_timing.py [--reps 20] [--n 25,1000] [--mode reference|softmax] [--K 2048]

Logits are synthetic: unit normal noise with 1.5 % of the positions raised to 5.5 .. 9 -- about 2 000 candidates above 0.015
per image in the reference mode, whose plane-wide normalisation leaves nothing above the threshold on plain noise at this size."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 480, 640


def logits_batch(n_distinct, seed=1):
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((n_distinct, 65, H // 8, W // 8)).astype(np.float32)
    peak = rng.random(lg.shape) < 0.015
    lg[peak] = rng.uniform(5.5, 9.0, int(peak.sum())).astype(np.float32)
    return lg


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", default="25,1000")
    ap.add_argument("--mode", default="reference", choices=["reference", "softmax"])
    ap.add_argument("--K", type=int, default=2048)
    ap.add_argument("--no-ref", action="store_true", help="skip the numpy greedy loop")
    a = ap.parse_args()
    import ctypes as C
    import torch
    import bench
    import kp_ref
    from reconstructor_amd import _lib, keypoints
    ctx = _lib.Context(0)
    mode = keypoints.HEAT_REFERENCE if a.mode == "reference" else keypoints.HEAT_SOFTMAX
    thresh = 0.015 if a.mode == "reference" else 0.5
    base = torch.from_numpy(logits_batch(25)).cuda()
    out = {"tool": "keypoints_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "mode": a.mode, "H": H, "W": W, "K": a.K, "cases": {}}
    st = torch.cuda.Stream()
    P = lambda t: C.c_void_p(t.data_ptr())
    for n in [int(x) for x in a.n.split(",")]:
        lg = base.repeat((n + 24) // 25, 1, 1, 1)[:n].contiguous()
        xy = torch.empty((n, a.K, 2), dtype=torch.int32, device="cuda")
        conf = torch.empty((n, a.K), dtype=torch.float32, device="cuda")
        counts = torch.empty((n,), dtype=torch.int32, device="cuda")
        rounds = torch.empty((n,), dtype=torch.int32, device="cuda")
        heat = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, st.cuda_stream))
        si, sc, sy, sx = lg.stride()

        def detect(heat_out):
            ctx.check(ctx.lib.rcn_kp_detect_device(ctx.h, P(lg), si, sc, sy, sx, n, H, W, mode, thresh, 4, 4, a.K, P(xy), P(conf), P(counts),
                                                   P(heat) if heat_out else None, P(rounds)))

        def nms_only():
            ctx.check(ctx.lib.rcn_kp_nms_device(ctx.h, P(heat), n, H, W, thresh, 4, 4, a.K, P(xy), P(conf), P(counts), P(rounds)))

        d_ms, d_min = timed(st, a.reps, lambda: detect(False))
        h_ms, _ = timed(st, a.reps, lambda: detect(True))
        n_ms, _ = timed(st, a.reps, nms_only)
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, None))
        cnt, rnd = counts.cpu().numpy(), rounds.cpu().numpy()
        bytes_in, bytes_out = 65 * (H // 8) * (W // 8) * 4, a.K * 12 + 4
        c = {"n": n, "us_per_image": round(1e3 * d_ms / n, 2), "us_per_image_min": round(1e3 * d_min / n, 2),
             "us_per_image_with_heat_out": round(1e3 * h_ms / n, 2),
             "share_exact_stages": round(min(1.0, n_ms / d_ms), 3), "share_heat_stage": round(max(0.0, 1 - n_ms / d_ms), 3),
             "keypoints_per_image": [int(cnt.min()), float(cnt.mean()), int(cnt.max())],
             "rounds_per_image": [int(rnd.min()), float(rnd.mean()), int(rnd.max())],
             "traffic_floor_us_per_image": round(1e6 * (bytes_in + bytes_out) / 8e12, 3),
             "traffic_floor_us_per_image_with_heat_out": round(1e6 * (bytes_in + bytes_out + H * W * 4) / 8e12, 3)}
        if not a.no_ref:
            h0 = heat[0].cpu().numpy()
            t0 = time.perf_counter()
            want = kp_ref.nms_greedy(h0, thresh, 4, 4, a.K)
            c["numpy_greedy_us_per_image"] = round(1e6 * (time.perf_counter() - t0), 1)
            c["equal_to_numpy_greedy"] = bool(np.array_equal(want[0], xy[0].cpu().numpy()) and want[2] == cnt[0])
        out["cases"]["n%d" % n] = c
        del lg, xy, conf, counts, rounds, heat
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
