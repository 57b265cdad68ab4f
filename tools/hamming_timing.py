"""Times of the Hamming matcher for all-pairs grids of n images x K rows of 256 bits, and of the parent's code
on the same box in the same run: HIP events on a stream of its own around each call, 3 warm-up calls, median of --reps.

Per case (n x K) it records
    ingest_ms              rcn_bits_upload_batch_device: allocation + k_ham_expand
    top2_knn_ms            rcn_hamming_knn2_device: k_ham_top2 and the write of the (j0, d0, j1, d1) table
    grid_ms                rcn_match_grid_hamming_device: k_ham_top2, the claim and the emit
    pair_distances         sum over pairs of K x K
    l2_float               (a) rcn_match_grid_device on the same bytes as rows of 32 floats: what the ORB branch used until now
                           (call time, and coarse_ms per call from rcn_match_profile)
    int8_d256              (b) the int8 coarse pass on a D = 256 grid of the same n and K: the same four 16x16x64 MFMAs per tile of
                           distances and the same fold (coarse_ms per call from rcn_match_profile, and the call time)
The kernels' own times come from a second run under rocprofv3 --kernel-trace --stats (tracing slows the host: never in the timed
run); --kernel-stats CSV merges that run's per-kernel averages into the document.  Nothing here is a pass condition.  Writes one
JSON document, stamped with the source hash, to profiles/hamming_timing.json (and prints it).

    python tools/hamming_timing.py [--reps 5] [--cases 256x4096,25x500] [--kernel-stats CSV] [--out profiles/hamming_timing.json]
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def binary_images(n, K, seed=1):
    """n images of K rows drawn from a world of 4 K random rows, each with about 12 of its 256 bits flipped: uint8 [n][K][32]."""
    rng = np.random.default_rng(seed)
    world = rng.integers(0, 256, (4 * K, 32), dtype=np.uint8)
    out = np.empty((n, K, 32), np.uint8)
    for i in range(n):
        pick = rng.choice(len(world), size=K, replace=False)
        flips = np.packbits(rng.random((K, 256)) < 12.0 / 256.0, axis=1, bitorder="little")
        out[i] = world[pick] ^ flips
    return out


def timed(st, reps, fn, warm=3):
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
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


def kernel_stats(path):
    """kernel name -> (calls, average microseconds) from a rocprofv3 kernel_stats CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("kernel") or ""
            if "AverageNs" in row:
                out[name] = (int(row["Calls"]), round(float(row["AverageNs"]) / 1e3, 2))
            elif "avg_us" in row:
                out[name] = (int(row["calls"]), round(float(row["avg_us"]), 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--cases", default="256x4096,25x500")
    ap.add_argument("--skip-parent", action="store_true", help="the Hamming calls only (the run under the profiler)")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hamming_timing.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        doc = json.load(open(a.out))
        ks = kernel_stats(a.kernel_stats)
        doc["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (--skip-parent --reps 1 --warm 1)",
                               "kernels": {k: {"calls": c, "avg_us": us} for k, (c, us) in sorted(ks.items()) if "k_ham_" in k}}
        json.dump(doc, open(a.out, "w"), indent=1)
        print(json.dumps(doc["kernel_trace"], indent=1))
        return
    import torch
    import bench
    from reconstructor_amd import _lib, synth
    from reconstructor_amd.matcher import HipL2Matcher, all_pairs
    ctx = _lib.Context(0)
    lib, h = ctx.lib, ctx.h
    m = HipL2Matcher(ctx=ctx)
    st = torch.cuda.Stream()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    doc = {"tool": "hamming_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "warm_up": a.warm,
           "staging": "plain loads through registers into two LDS buffers (no LDS-DMA ring)", "cases": {}}
    for case in a.cases.split(","):
        n, K = (int(v) for v in case.split("x"))
        n_pairs = n * (n - 1) // 2
        by_host = binary_images(n, K)
        by = torch.from_numpy(by_host).cuda()
        out = torch.empty((n_pairs, K), dtype=torch.int32, device="cuda")
        cnt = torch.empty((n_pairs,), dtype=torch.int32, device="cuda")
        knn = torch.empty((n_pairs, K, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.check(lib.rcn_set_stream(h, st.cuda_stream))

        def ingest():
            ctx.check(lib.rcn_bits_upload_batch_device(h, 0, n, P(by), None, K, 32))

        def grid():
            ctx.check(lib.rcn_match_grid_hamming_device(h, None, n_pairs, 0.7, P(out), K, P(cnt)))

        def top2_knn():
            ctx.check(lib.rcn_hamming_knn2_device(h, None, n_pairs, P(knn), K))

        r = {"n": n, "K": K, "pairs": n_pairs, "pair_distances": n_pairs * K * K}
        r["ingest_ms"], r["ingest_ms_min"] = timed(st, a.reps, ingest, a.warm)
        r["top2_knn_ms"], r["top2_knn_ms_min"] = timed(st, a.reps, top2_knn, a.warm)
        r["grid_ms"], r["grid_ms_min"] = timed(st, a.reps, grid, a.warm)
        r["matches"] = int(cnt.sum().item())
        r["pair_distances_per_s_top2_knn"] = float("%.4g" % (r["pair_distances"] / (r["top2_knn_ms"] * 1e-3)))
        ctx.check(lib.rcn_bits_clear(h))
        del knn
        if not a.skip_parent:
            pairs = all_pairs(n)

            def parent(rows_dev, D):
                m.clear()
                m.upload_batch_device(0, n, rows_dev.data_ptr(), K, D)
                m.profile(True)

                def call():
                    m.match_grid_device(pairs, out.data_ptr(), K, cnt.data_ptr())

                call()
                ctx.check(lib.rcn_synchronize(h))
                m.stats()                                     # what the first call (conversion included) recorded is read and dropped
                ms, ms_min = timed(st, a.reps, call, a.warm - 1)
                s = m.stats()
                m.profile(False)
                calls = max(1, s["profiled_calls"])
                res = {"D": D, "grid_ms": ms, "grid_ms_min": ms_min, "coarse_ms_per_call": round(s["coarse_ms"] / calls, 4),
                       "coarse_launches_per_call": s["coarse_launches"] // calls, "coarse_dtype": s["coarse_dtype"], "used_mfma_path": s["used_mfma_path"],
                       "matches": int(cnt.sum().item())}
                m.clear()
                return res

            as_float = by.to(torch.float32)
            torch.cuda.synchronize()
            r["l2_float"] = parent(as_float, 32)
            del as_float
            fl = torch.from_numpy(np.stack(synth.descriptor_set("superpoint", n, K, n_world=4 * K, seed=1234))).cuda()
            torch.cuda.synchronize()
            r["int8_d256"] = parent(fl, 256)
            del fl
            r["top2_knn_over_int8_coarse"] = round(r["top2_knn_ms"] / r["int8_d256"]["coarse_ms_per_call"], 3)
            r["grid_over_l2_float_grid"] = round(r["grid_ms"] / r["l2_float"]["grid_ms"], 3)
        ctx.check(lib.rcn_set_stream(h, None))
        doc["cases"][case] = r
        del by, out, cnt
        torch.cuda.empty_cache()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
