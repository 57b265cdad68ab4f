"""Times the optimal-matching layer (rcn_sg_assign_device) against the fp32 torch transcription of the
published forward run eagerly on the same GPU on the same scores.

    python tools/superglue_timing.py [--pairs 300] [--iterations 100] [--reps 3] [--quick] [--out FILE.json]

Shapes: 1900 x 1900 and 1024 x 1024 on the banded path, 128 x 128 on the fused path and with the banded path forced.  For the
banded shapes the chunk budget (rcn_sg_set_chunk_bytes) is swept over one pair, 64 MiB, 192 MiB and no limit.  Reported per
run: milliseconds (best of reps), bytes/s against "one matrix read per iteration", exp/s at two per element per iteration.
--quick: the first shape alone, once after the warm-up call, no chunk sweep and no torch: for a profiler run.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_scores(B, m, n, seed):
    """Planted matches plus noise, as the tests' cases but built on the GPU: noise of deviation 0.75, 60 % of the rows
    planted at 12 on a random permutation."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    S = 0.75 * torch.randn((B, m, n), generator=g, device="cuda", dtype=torch.float32)
    k = int(0.6 * min(m, n))
    for b in range(B):
        cols = torch.randperm(n, generator=g, device="cuda")[:k]
        S[b, torch.arange(k, device="cuda"), cols] = 12.0
    return S


def torch_forward(S, alpha, iterations):
    """log_optimal_transport as published, batched, fp32, eager."""
    import torch
    B, m, n = S.shape
    a = torch.tensor(alpha, device=S.device, dtype=S.dtype)
    Z = torch.cat([torch.cat([S, a.expand(B, m, 1)], -1), a.expand(B, 1, n + 1)], 1)
    ms, ns = torch.tensor(float(m), device=S.device), torch.tensor(float(n), device=S.device)
    norm = -(ms + ns).log()
    log_mu = torch.cat([norm.expand(m), ns.log()[None] + norm])[None].expand(B, -1)
    log_nu = torch.cat([norm.expand(n), ms.log()[None] + norm])[None].expand(B, -1)
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iterations):
        u = log_mu - torch.logsumexp(Z + v.unsqueeze(1), dim=2)
        v = log_nu - torch.logsumexp(Z + u.unsqueeze(2), dim=1)
    Z = Z + u.unsqueeze(2) + v.unsqueeze(1) - norm
    mx0, mx1 = Z[:, :-1, :-1].max(2), Z[:, :-1, :-1].max(1)
    return mx0.indices, mx1.indices, mx0.values.exp()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from reconstructor_amd import _lib, superglue
    ctx = _lib.Context(0)
    L, h = ctx.lib, ctx.h
    results = []

    def timed(fn):
        fn()
        best = float("inf")
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            best = min(best, time.perf_counter() - t0)
        return best

    def run(B, m, n, path, chunk, S, out, label):
        opt = superglue.options(ctx, path=path, iterations=args.iterations)
        superglue.set_chunk_bytes(ctx, chunk)

        def call():
            ctx.check(L.rcn_sg_assign_device(h, S.data_ptr(), m * n, n, 1, None, None, B, m, n, C.byref(opt), *out))
            ctx.check(L.rcn_synchronize(h))
        t = timed(call)
        work = float(B) * m * n * args.iterations
        r = dict(shape=[m, n], pairs=B, path=label, chunk_bytes=chunk, ms=1e3 * t, us_per_pair=1e6 * t / B,
                 matrix_GBps=4 * work / t / 1e9, exp_per_s=2 * work / t)
        results.append(r)
        print(json.dumps(r), flush=True)
        return t

    plan = [(1900, superglue.PATH_BANDED, "banded"), (1024, superglue.PATH_BANDED, "banded"), (128, superglue.PATH_FUSED, "fused"),
            (128, superglue.PATH_BANDED, "banded")]
    if args.quick:
        plan, args.reps = [(1900, superglue.PATH_BANDED, "banded")], 1
    for k, path, label in plan:
        B, m, n = args.pairs, k, k
        S = make_scores(B, m, n, seed=k)
        o = superglue._outputs(B, m, n, None, False, S.device)
        out = superglue._out_args(o)
        torch.cuda.synchronize()
        chunks = [0] if (label == "fused" or k == 128 or args.quick) else [1, 64 << 20, 192 << 20, 0]
        for chunk in chunks:
            run(B, m, n, path, chunk, S, out, label)
        superglue.set_chunk_bytes(ctx, 0)
        if not args.no_torch and not args.quick and not (k == 128 and label == "banded"):
            t = timed(lambda: (torch_forward(S, 1.0, args.iterations), torch.cuda.synchronize()))
            i0 = torch_forward(S, 1.0, args.iterations)[0]
            mine = o["matches0"]          # the last run's result
            agree = float(((mine == i0) | (mine < 0)).float().mean())
            r = dict(shape=[m, n], pairs=B, path="torch eager fp32", ms=1e3 * t, us_per_pair=1e6 * t / B, rows_agreeing_where_matched=agree)
            results.append(r)
            print(json.dumps(r), flush=True)
        del S, o, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
