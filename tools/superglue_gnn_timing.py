"""Times the graph network (rcn_sg_net_forward_device) against the fp32 torch transcription of the
published forward run eagerly on the same GPU on the same data: 18 layers, B pairs at 1900 x 1900, 1024 x 1024 and 128 x 128,
best of 3 host-clock timings, each ending in a synchronisation.  Prints one JSON line per shape.

    python tools/superglue_gnn_timing.py [--pairs 1900:32,1024:64,128:512] [--layers 18] [--repeat 3]

Flops are derived, not measured: per point of a K-point image with a Ks-point source, per layer, 2 * (4 * 256^2) for q, k, v
and the merge, 2 * (512^2 + 512 * 256) for the MLP, 4 * 256 * Ks for QK^T and PV."""
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

from reconstructor_amd import _lib, superglue_gnn as G  # noqa: E402

PEAK_TFLOPS = 157.3            # fp32 matrix peak of an MI355X


def flops(K, L):
    enc = 2 * sum(a * b for a, b in zip(G.ENC[:-1], G.ENC[1:]))
    layer = 2 * 4 * 256 * 256 + 2 * (512 * 512 + 512 * 256) + 4 * 256 * K
    return 2 * K * (enc + L * layer + 2 * 256 * 256)


def torch_forward(sd, types, k0, s0, d0, k1, s1, d1):
    """The published forward, batched [B][C][K], unfolded BatchNorm in eval mode; sd: CUDA tensors."""
    conv = lambda name, x: F.conv1d(x, sd[name + ".weight"], sd[name + ".bias"])
    bn = lambda name, x: F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"], False, 0.0, G.BN_EPS)

    def enc(k, s, d):
        x = torch.cat([k.transpose(1, 2), s[:, None]], dim=1)
        for i in range(5):
            x = conv("kenc.encoder.%d" % (3 * i), x)
            if i < 4:
                x = F.relu(bn("kenc.encoder.%d" % (3 * i + 1), x))
        return d.transpose(1, 2) + x

    def attn(p, x, src):
        B = x.shape[0]
        q, k, v = (conv(p + "attn.proj.%d" % i, a).view(B, 64, 4, -1) for i, a in enumerate((x, src, src)))
        prob = torch.softmax(torch.einsum("bdhn,bdhm->bhnm", q, k) / 8.0, dim=-1)
        return conv(p + "attn.merge", torch.einsum("bhnm,bdhm->bdhn", prob, v).contiguous().view(B, 256, -1))

    x0, x1 = enc(k0, s0, d0), enc(k1, s1, d1)
    for l, t in enumerate(types):
        p = "gnn.layers.%d." % l
        a0, a1 = (x1, x0) if t == G.CROSS else (x0, x1)
        deltas = [conv(p + "mlp.3", F.relu(bn(p + "mlp.1", conv(p + "mlp.0", torch.cat([x, attn(p, x, s)], dim=1))))) for x, s in ((x0, a0), (x1, a1))]
        x0, x1 = x0 + deltas[0], x1 + deltas[1]
    return conv("final_proj", x0).transpose(1, 2), conv("final_proj", x1).transpose(1, 2)


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
    ap.add_argument("--pairs", default="1900:32,1024:64,128:512")
    ap.add_argument("--layers", type=int, default=18)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    L = a.layers
    sd = G.random_weights(2038, L)
    types = [G.SELF, G.CROSS] * (L // 2) + [G.SELF] * (L % 2)
    sd_dev = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    with torch.no_grad(), _lib.Context(0) as ctx, G.Net.from_state_dict(ctx, sd, types) as net:
        for item in a.pairs.split(","):
            K, B = (int(v) for v in item.split(":"))
            rng = np.random.default_rng(K)
            one = G.planted_inputs(rng, K, K, int(0.6 * K))[:6]
            t = [torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x, (B,) + x.shape))).cuda() for x in one]
            out = (torch.empty((B, K, 256), device="cuda"), torch.empty((B, K, 256), device="cuda"))
            torch.cuda.synchronize()

            def run_ours():
                ctx.check(ctx.lib.rcn_sg_net_forward_device(ctx.h, net.h, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), K * 256, 256, 1,
                                                            t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), K * 256, 256, 1, None, None, None, None,
                                                            B, K, K, 256, out[0].data_ptr(), out[1].data_ptr()))
            ours = best_of(run_ours, lambda: ctx.check(ctx.lib.rcn_synchronize(ctx.h)), a.repeat)
            res = dict(shape=[K, K], pairs=B, layers=L, seconds=ours, tflops=B * flops(K, L) / ours / 1e12)
            res["fraction_of_fp32_matrix_peak"] = res["tflops"] / PEAK_TFLOPS
            if not a.no_torch:
                ref = [None]

                def run_torch():
                    ref[0] = torch_forward(sd_dev, types, *t)
                res["torch_eager_seconds"] = best_of(run_torch, torch.cuda.synchronize, a.repeat)
                res["speedup_over_torch_eager"] = res["torch_eager_seconds"] / ours
                res["max_rel_dev_from_torch"] = float(max((o - r).abs().max() / r.abs().max() for o, r in zip(out, ref[0])))
                ref[0] = None
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
