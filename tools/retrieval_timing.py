"""Times of the retrieval ImageMatcher (rcn_retr_*) at n = 1000 images, K = 4096, D = 256 and at K = 2048,
D = 128, with C = 64 centroids, 10 Lloyd steps and k = 20: HIP events on a stream of its own around each stage, 2 warm-up calls,
median of --reps.  Per shape it prints the stages (training, assignment of all rows, encoding = assignment + segment sums +
normalisation, similarity, top-k, pairs, and the one call), the same stages written in eager fp32 torch on the same GPU (cdist /
argmin, index_add_, matmul, topk), and rcn_match_grid_device over the retrieved list against the full grid (one warm-up, one timed
call each; --no-grid skips them).  One JSON line stamped with the source hash.

    python tools/retrieval_timing.py [--reps 5] [--shapes 4096x256,2048x128] [--n 1000] [--no-grid]

The scene is a ring (retrieval.ring_scene's construction, built on the device): image i sees K consecutive rows of a pool of
n * K / 4 unit rows, so that an image overlaps its three neighbours on either side."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(n, K, D, noise=0.05, seed=1):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    step = K // 4
    pool = torch.nn.functional.normalize(torch.randn((n * step, D), device="cuda", generator=g), dim=1)
    out = torch.empty((n, K, D), dtype=torch.float32, device="cuda")
    for i in range(n):
        idx = (i * step + torch.randperm(K, device="cuda", generator=g)) % (n * step)
        out[i] = torch.nn.functional.normalize(pool[idx] + noise * torch.randn((K, D), device="cuda", generator=g), dim=1)
    return out


def timed(st, reps, fn, warm=2):
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 3)


def torch_stages(st, reps, x, mu, k):
    """the same pipeline in eager fp32 torch"""
    import torch
    n, K, D = x.shape
    Cn = mu.shape[0]
    flat = x.view(-1, D)
    img = torch.arange(n, device="cuda").repeat_interleave(K)
    state = {}

    def assign():
        state["a"] = torch.cat([torch.cdist(flat[i:i + (1 << 20)], mu).argmin(1) for i in range(0, flat.shape[0], 1 << 20)])

    def lloyd():
        m = mu.clone()
        sub = flat[::16]
        for _ in range(10):
            a = torch.cdist(sub, m).argmin(1)
            S = torch.zeros_like(m).index_add_(0, a, sub)
            cnt = torch.bincount(a, minlength=Cn).clamp(min=1)
            m = S / cnt[:, None]

    def encode():
        a = state["a"]
        S = torch.zeros((n * Cn, D), device="cuda").index_add_(0, img * Cn + a, flat)
        cnt = torch.bincount(img * Cn + a, minlength=n * Cn).view(n, Cn, 1)
        V = S.view(n, Cn, D) - cnt * mu[None]
        V = torch.sign(V) * torch.sqrt(torch.abs(V))
        state["G"] = torch.nn.functional.normalize(V.view(n, -1), dim=1)

    def sim():
        state["sim"] = state["G"] @ state["G"].T

    def topk():
        s = state["sim"].clone()
        s.fill_diagonal_(-2.0)
        state["nbr"] = s.topk(k, dim=1).indices

    with torch.cuda.stream(st):
        return {"train": timed(st, reps, lloyd), "assign": timed(st, reps, assign), "encode_behind_assign": timed(st, reps, encode),
                "similarity": timed(st, reps, sim), "topk": timed(st, reps, topk)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="4096x256,2048x128")
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--no-grid", action="store_true")
    a = ap.parse_args()
    import torch
    import bench
    from reconstructor_amd import _lib, retrieval
    from reconstructor_amd.matcher import HipL2Matcher, all_pairs
    ctx = _lib.Context(0)
    L, h = ctx.lib, ctx.h
    n, Cn, k = a.n, 64, 20
    out = {"tool": "retrieval_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "n": n,
           "C": Cn, "steps": 10, "k": k, "cases": {}}
    st = torch.cuda.Stream()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for shape in a.shapes.split(","):
        K, D = (int(v) for v in shape.split("x"))
        x = scene(n, K, D)
        torch.cuda.synchronize()
        cb = retrieval.train_codebook(ctx, x, None, Cn, 10)
        mu = torch.from_numpy(cb.centroids()).cuda()
        asg = torch.empty((n * K,), dtype=torch.int32, device="cuda")
        G = torch.empty((n, Cn * D), dtype=torch.float32, device="cuda")
        sim = torch.empty((n, n), dtype=torch.float64, device="cuda")
        nbr = torch.empty((n, k), dtype=torch.int32, device="cuda")
        prs = torch.empty((n * k, 2), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
        host = np.zeros((n * k, 2), np.int32)
        hc = C.c_int32(0)
        opt = retrieval.options(Cn, 10, 0, k)
        torch.cuda.synchronize()
        ctx.check(L.rcn_set_stream(h, st.cuda_stream))

        def train():
            hh = C.c_void_p()
            ctx.check(L.rcn_retr_codebook_train_device(h, P(x), None, n, K, D, C.byref(opt), C.byref(hh)))
            L.rcn_retr_codebook_destroy(hh)

        stages = {
            "train": timed(st, a.reps, train),
            "assign": timed(st, a.reps, lambda: ctx.check(L.rcn_retr_assign_device(h, cb.h, P(x), n * K, P(asg)))),
            "encode": timed(st, a.reps, lambda: ctx.check(L.rcn_retr_encode_device(h, cb.h, P(x), None, n, K, D, P(G)))),
            "similarity": timed(st, a.reps, lambda: ctx.check(L.rcn_retr_similarity_device(h, P(G), n, Cn * D, D, P(sim)))),
            "topk": timed(st, a.reps, lambda: ctx.check(L.rcn_retr_topk_device(h, P(sim), n, k, P(nbr)))),
            "pairs": timed(st, a.reps, lambda: ctx.check(L.rcn_retr_pairs_device(h, P(nbr), n, k, 0, P(prs), n * k, P(cnt)))),
            "image_pairs": timed(st, a.reps, lambda: ctx.check(L.rcn_retr_image_pairs(h, cb.h, P(x), None, n, K, D, 0, k, host.ctypes.data, n * k, C.byref(hc)))),
        }
        pairs = host[:hc.value].copy()
        step = K // 4
        ring = np.minimum((pairs[:, 0] - pairs[:, 1]) % n, (pairs[:, 1] - pairs[:, 0]) % n)
        case = {"K": K, "D": D, "train_row_stride": retrieval_stride(n, K), "ms": stages, "torch_fp32_ms": torch_stages(st, a.reps, x, mu, k),
                "assign_plus_encode_share_of_3100_ms_grid": round((stages["assign"] + stages["encode"]) / 3100.0, 4),
                "pairs": int(hc.value), "pairs_overlapping": int((ring * step < K).sum()), "full_grid_pairs": n * (n - 1) // 2}
        if not a.no_grid:
            m = HipL2Matcher(ctx=ctx)
            m.upload_batch_device(0, n, x.data_ptr(), K, D)
            grid = all_pairs(n)
            table = torch.empty((len(grid), K), dtype=torch.int32, device="cuda")
            counts = torch.empty((len(grid),), dtype=torch.int32, device="cuda")
            case["match_grid_retrieved_ms"] = timed(st, 1, lambda: m.match_grid_device(pairs, table.data_ptr(), K, counts.data_ptr()), warm=1)
            kept = int(counts[:len(pairs)].sum().item())
            case["match_grid_full_ms"] = timed(st, 1, lambda: m.match_grid_device(grid, table.data_ptr(), K, counts.data_ptr()), warm=1)
            case["matches_kept"], case["matches_full"] = kept, int(counts.sum().item())
            m.clear()
            del table, counts
        ctx.check(L.rcn_set_stream(h, None))
        out["cases"][shape] = case
        cb.close()
        del x, G, sim, asg
    ctx.close()
    print(json.dumps(out))


def retrieval_stride(n, K):
    s = 1
    while n * -(-K // s) > 2 ** 18:
        s += 1
    return s


if __name__ == "__main__":
    main()
