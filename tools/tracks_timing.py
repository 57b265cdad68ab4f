"""Times of track building on synthetic match lists, next to the loop a user runs today: HIP events on a stream of
its own around each call, 3 warm-up calls, median of --reps.

Scenes: n images of K keypoints; image i sees K landmarks drawn from a window of 3 K landmarks that slides by K / 4 per image, so
near images overlap and far ones do not.  A pair's list holds the keypoints of shared landmarks (80 % of them), of which 2 % are
shuffled among themselves into wrong matches (they make the conflicts).  Pairs: all n (n - 1) / 2, or every image with its next
--neighbours images (a retrieved list).

Per case it records
    build_ms               rcn_tracks_build_device with every output (pixels, feat_track, statistics)
    phase_ms               hook, flatten, conflicts, scans, scatter, sort from the library's own events (rcn_tracks_last_phase_ms)
    floor                  the traffic floor: entries read once, the parent array and the outputs written once, at the 6.29 TB/s a
                           float4 copy reaches on this part
    host_loop_ms           tools/tracks_host_loop.cpp (single thread, g++ -O2, built here) on the same host lists: union-find,
                           components, the same conflict rule and length filter; it needs no copy when the lists are on the host
    lists_d2h_ms           the copy of the resident lists to pageable host memory it would need when they are not
Nothing here is a pass condition.  Writes one JSON document, stamped with the source hash, to profiles/tracks_timing.json.

    python tools/tracks_timing.py [--reps 5] [--cases 100x4096xall,1000x4096x11] [--out profiles/tracks_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_BYTES_PER_S = 6.29e12


def scene(n, K, neighbours, seed=1):
    rng = np.random.default_rng(seed)
    world = (n - 1) * (K // 4) + 3 * K
    lm = [np.sort((i * (K // 4) + rng.permutation(3 * K)[:K]) % world) for i in range(n)]
    lm = [rng.permutation(l) for l in lm]
    pairs, offs, qt = [], [0], []
    total = 0
    for a in range(n):
        for b in range(a + 1, n if neighbours is None else min(n, a + 1 + neighbours)):
            _, fa, fb = np.intersect1d(lm[a], lm[b], assume_unique=True, return_indices=True)
            keep = rng.random(len(fa)) < 0.8
            fa, fb = fa[keep], fb[keep]
            wrong = np.nonzero(rng.random(len(fa)) < 0.02)[0]
            if len(wrong) > 1:
                fb[wrong] = fb[rng.permutation(wrong)]
            pairs.append((a, b))
            qt.append(np.stack([fa, fb], 1).astype(np.int32))
            total += len(fa)
            offs.append(total)
    return (np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(offs, np.int64),
            np.concatenate(qt).astype(np.int32) if qt else np.zeros((0, 2), np.int32))


def host_loop_lib(tmp):
    so = os.path.join(tmp, "tracks_host_loop.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "tracks_host_loop.cpp")])
    lib = C.CDLL(so)
    lib.tracks_host_loop.restype = C.c_double
    lib.tracks_host_loop.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    return lib


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--cases", default="100x4096xall,1000x4096x11")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_timing.json"))
    a = ap.parse_args()
    import torch
    import bench
    from reconstructor_amd import _lib, nextview, tracks
    ctx = _lib.Context(0)
    lib, h = ctx.lib, ctx.h
    st = torch.cuda.Stream()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    doc = {"tool": "tracks_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "warm_up": a.warm,
           "floor_bytes_per_s": HBM_COPY_BYTES_PER_S, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        host = host_loop_lib(tmp)
        for case in a.cases.split(","):
            n, K, nb = case.split("x")
            n, K, nb = int(n), int(K), None if nb == "all" else int(nb)
            pairs, offs, qt = scene(n, K, nb)
            xy = np.ascontiguousarray(np.random.default_rng(2).integers(0, 4000, (K, 2)), np.int32)
            for i in range(n):
                ctx.check(lib.rcn_coords_upload(h, i, xy.ctypes.data, K))
            nextview.upload_lists(ctx, pairs, offs, qt)
            ids, node_off = tracks.layout(ctx)
            N, E = int(node_off[-1]), int(offs[-1])
            r = {"n": n, "K": K, "pairs": len(pairs), "nodes": N, "entries": E}
            for policy, name in ((tracks.DROP_TRACK, "drop_track"), (tracks.DROP_IMAGE, "drop_image")):
                opt = tracks.options(conflict=policy)
                cap_t, cap_o = N // 2, N
                dev = torch.device("cuda", 0)
                mk = lambda m, dt=torch.int32: torch.empty((max(m, 1),), dtype=dt, device=dev)      # noqa: E731
                counts, off, oi, of, oxy, ft, stats = mk(2), mk(cap_t + 1), mk(cap_o), mk(cap_o), mk(2 * cap_o), mk(N), mk(8, torch.int64)
                torch.cuda.synchronize()
                ctx.check(lib.rcn_set_stream(h, st.cuda_stream))

                def build():
                    ctx.check(lib.rcn_tracks_build_device(h, C.byref(opt), 0, None, None, cap_t, cap_o, P(counts), P(off), P(oi), P(of), None, P(oxy),
                                                          P(ft), P(stats)))

                q = {}
                q["build_ms"], q["build_ms_min"] = timed(st, a.reps, build, a.warm)
                ph = []
                for _ in range(a.reps):
                    build()
                    ph.append(tracks.phase_ms(ctx))
                q["phase_ms"] = dict(zip(("hook", "flatten", "conflicts", "scans", "scatter", "sort"), np.round(np.median(ph, axis=0), 4).tolist()))
                ctx.check(lib.rcn_set_stream(h, None))
                c, s = counts.cpu().numpy(), stats.cpu().numpy()
                q["tracks"], q["observations"] = int(c[0]), int(c[1])
                q["stats"] = dict(zip(tracks.STATS[:7], s[:7].tolist()))
                floor_bytes = 8 * E + 4 * N + 4 * N + 16 * int(c[1]) + 4 * (int(c[0]) + 1)
                q["floor"] = {"bytes": floor_bytes, "ms": round(floor_bytes / HBM_COPY_BYTES_PER_S * 1e3, 4)}
                q["build_over_floor"] = round(q["build_ms"] / q["floor"]["ms"], 1)
                hc = np.zeros(2, np.int64)
                sa, sb = np.searchsorted(ids, pairs[:, 0]).astype(np.int32), np.searchsorted(ids, pairs[:, 1]).astype(np.int32)
                ms = [host.tracks_host_loop(len(pairs), sa.ctypes.data, sb.ctypes.data, offs.ctypes.data, qt.ctypes.data, len(ids), node_off.ctypes.data,
                                            2, 0, int(policy == tracks.DROP_IMAGE), hc.ctypes.data) for _ in range(3)]
                q["host_loop_ms"] = round(float(np.median(ms)), 3)
                q["host_loop_equal_counts"] = bool(hc[0] == c[0] and hc[1] == c[1])
                q["host_loop_over_build"] = round(q["host_loop_ms"] / q["build_ms"], 2)
                r[name] = q
                del counts, off, oi, of, oxy, ft, stats
            # the copy of the lists the host loop needs when they live in HBM only
            ent = torch.from_numpy(qt).cuda()
            torch.cuda.synchronize()
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                ent.cpu()
                t.append((time.perf_counter() - t0) * 1e3)
            r["lists_d2h_ms"] = round(float(np.median(t)), 3)
            del ent
            nextview.clear_lists(ctx)
            ctx.check(lib.rcn_coords_clear(h))
            doc["cases"][case] = r
            torch.cuda.empty_cache()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
