"""Times SuperPoint's network (rcn_sp_net_forward_device) against the fp32 torch transcription of the
published forward run eagerly on the same GPU on the same data: n images of H x W, best of 3 host-clock timings, each ending
in a synchronisation, after a warm-up call.  Prints one JSON line per shape.

    python tools/superpoint_net_timing.py [--shapes 480x640:25,480x640:100,240x320:1000] [--repeat 3] [--no-torch]

Flops are derived, not measured: per input pixel 2 * 9 * Cin * Cout / (pixels per output pixel) summed over the layers,
169.6 kFLOP."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from reconstructor_amd import _lib, superpoint_net as SP  # noqa: E402

PEAK_TFLOPS = 157.3            # fp32 matrix peak of an MI355X
POOLS_BEFORE = {"conv1a": 0, "conv1b": 0, "conv2a": 1, "conv2b": 1, "conv3a": 2, "conv3b": 2}      # every other layer: 3


def flops_per_pixel():
    return sum(2.0 * k * k * ci * co / 4 ** POOLS_BEFORE.get(name, 3) for name, co, ci, k in SP.layer_table())


def torch_forward(sd, imgs):
    """The published forward; sd: CUDA tensors.  Returns (logits [n][65][Hc][Wc], desc [n][256][Hc][Wc], normalised)."""
    c = lambda name, x, pad: F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=pad)
    x = imgs[:, None]
    for name in ("conv1a", "conv1b", None, "conv2a", "conv2b", None, "conv3a", "conv3b", None, "conv4a", "conv4b"):
        x = F.max_pool2d(x, 2, 2) if name is None else F.relu(c(name, x, 1))
    desc = c("convDb", F.relu(c("convDa", x, 1)), 0)
    return c("convPb", F.relu(c("convPa", x, 1)), 0), desc / torch.norm(desc, p=2, dim=1, keepdim=True)


def best_of(fn, sync, repeat):
    fn()
    sync()                                   # warm-up: workspace growth, kernel load
    best = float("inf")
    for _ in range(repeat):
        t = time.perf_counter()
        fn()
        sync()
        best = min(best, time.perf_counter() - t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="480x640:25,480x640:100,240x320:1000")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    sd = SP.random_weights(2038)
    sd_dev = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    with torch.no_grad(), _lib.Context(0) as ctx, SP.Net.from_state_dict(ctx, sd) as net:
        for item in a.shapes.split(","):
            shape, n = item.split(":")
            H, W = (int(v) for v in shape.split("x"))
            n = int(n)
            imgs = torch.from_numpy(np.random.default_rng(H + n).random((n, H, W), dtype=np.float32)).cuda()
            lg = torch.empty((n, H // 8, W // 8, 65), device="cuda")
            ds = torch.empty((n, H // 8, W // 8, 256), device="cuda")
            torch.cuda.synchronize()

            def run_ours():
                ctx.check(ctx.lib.rcn_sp_net_forward_device(ctx.h, net.h, imgs.data_ptr(), SP.INPUT_F32, H * W, W, 1, n, H, W, SP.NORMALIZE_DESC,
                                                            lg.data_ptr(), ds.data_ptr()))
            ours = best_of(run_ours, lambda: ctx.check(ctx.lib.rcn_synchronize(ctx.h)), a.repeat)
            res = dict(shape=[H, W], images=n, seconds=ours, ms_per_image=1e3 * ours / n, tflops=n * H * W * flops_per_pixel() / ours / 1e12)
            res["fraction_of_fp32_matrix_peak"] = res["tflops"] / PEAK_TFLOPS
            if not a.no_torch:
                ref = [None]

                def run_torch():
                    ref[0] = torch_forward(sd_dev, imgs)
                res["torch_eager_seconds"] = best_of(run_torch, torch.cuda.synchronize, a.repeat)
                res["speedup_over_torch_eager"] = res["torch_eager_seconds"] / ours
                res["max_rel_dev_from_torch"] = float(max((o.permute(0, 3, 1, 2) - r).abs().max() / r.abs().max() for o, r in zip((lg, ds), ref[0])))
                ref[0] = None
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
