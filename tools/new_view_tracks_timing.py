"""Time of step 3's candidate collection for one new view at three sizes; prints one JSON line per size,
stamped with the source hash.

    python tools/new_view_tracks_timing.py [--reps 20] [--sizes ref25,v200,big]

Per size, for the first unregistered image v of the scene:
  device_ms     rcn_new_view_tracks_device: HIP events around the call (its staged copy of the registered images' table
                included) after warm-up, median of --reps
  grow_view_ms  rcn_ba_session_grow_view: the candidates, their triangulation, the commit and the one copy back, wall clock
                around the (synchronous) call after warm-up, median of --reps
  host_loop_ms  the C++ walk of reconstructor_amd/host/HipTriangulator.h (Triangulator::newViewTracks, the loop
                triangulateMatchedLandmarks has always run) on the reference's containers holding the same lists and ids,
                timed inside tests/cpp/new_view_tracks_adapter_test --time-host-loop, median of --reps
The device's candidate count must equal the host loop's, or the tool fails.

Scenes are tools/next_view_timing.py's three (images x keypoints, registered): ref25 25 x 1500, 12; v200 200 x 2000, 100; big
1000 x 4096, 500 -- the same visibility model and per-pair sampling, generated in numpy from a seed, with the lists of the
pairs (v, registered image) only (the walk reads no other list).  A keypoint of a registered image is a landmark when its
scene point is seen by at least two registered images; 80 % of v's keypoints on such points count as attached by step 1."""
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
BIN = os.path.join(ROOT, "tests", "cpp", "new_view_tracks_adapter_test")

CFG = {"ref25": (25, 1500, 12, 3000, 0.5, 400, 1), "v200": (200, 2000, 100, 40000, 0.05, 200, 2),
       "big": (1000, 4096, 500, 330000, 0.01241, 64, 3)}


def scene(n_img, K, n_reg, n_pts, vis, per_pair, seed):
    rng = np.random.default_rng(seed)
    point_of = [rng.choice(n_pts, size=min(K, int(vis * n_pts)), replace=False).astype(np.int64) for _ in range(n_img)]
    coords = [np.column_stack([rng.integers(-8, 520, len(p)), rng.integers(-8, 344, len(p))]).astype(np.int32) for p in point_of]
    v = n_reg
    seen = np.zeros(n_pts, np.int64)
    for i in range(n_reg):
        seen[point_of[i]] += 1
    ids = {i: np.where(seen[point_of[i]] >= 2, point_of[i], -1).astype(np.int32) for i in range(n_reg)}
    ids[v] = np.where((seen[point_of[v]] >= 2) & (rng.random(len(point_of[v])) < 0.8), point_of[v], -1).astype(np.int32)
    feat_v = np.full(n_pts, -1, np.int64)
    feat_v[point_of[v]] = np.arange(len(point_of[v]))
    lists = {}
    for r in rng.permutation(n_reg):                                      # the order the caller's registeredImages iterates in
        common = np.flatnonzero(feat_v[point_of[r]] >= 0)
        if len(common) > per_pair:
            common = rng.choice(common, per_pair, replace=False)
        if len(common):
            lists[int(r)] = np.column_stack([feat_v[point_of[r][common]], common]).astype(np.int32)
    return {"v": v, "coords": coords, "ids": ids, "lists": lists}


def host_loop_ms(s, reps):
    v = s["v"]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "walk.txt")
        with open(path, "w") as f:
            f.write("view %d %d %d\n%s\n" % (v, len(s["ids"][v]), len(s["lists"]), " ".join(map(str, s["ids"][v].tolist()))))
            for r, m in s["lists"].items():
                f.write("%d %d %d\n%s\n%s\n" % (r, len(s["ids"][r]), len(m), " ".join(map(str, s["ids"][r].tolist())),
                                              " ".join(map(str, m.reshape(-1).tolist()))))
        w = subprocess.run([BIN, "--time-host-loop", path, str(reps)], capture_output=True, text=True, check=True, timeout=600).stdout.split()
    return int(w[2]), float(w[4]), float(w[6])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="ref25,v200,big")
    a = ap.parse_args()
    import torch
    import bench
    from reconstructor_amd import _lib, ba, newview, nextview
    if not os.path.exists(BIN):
        raise SystemExit("build first: python __graft_entry__.py")
    ctx = _lib.Context(0)
    dev = torch.device("cuda", 0)
    for name in a.sizes.split(","):
        t0 = time.time()
        s = scene(*CFG[name])
        gen_s = time.time() - t0
        v, reg = s["v"], list(s["lists"])
        n_tracks_host, host_med, host_min = host_loop_ms(s, a.reps)
        for i in [v] + reg:
            ctx.check(ctx.lib.rcn_coords_upload(ctx.h, i, s["coords"][i].ctypes.data, len(s["coords"][i])))
        pairs = np.asarray([(v, r) for r in reg], np.int32)
        offs = np.concatenate([[0], np.cumsum([len(s["lists"][r]) for r in reg])]).astype(np.int64)
        nextview.upload_lists(ctx, pairs, offs, np.concatenate([s["lists"][r] for r in reg]))
        table = newview.LandmarkIds(ctx)
        t_img = np.concatenate([np.full(len(s["ids"][i]), i, np.int32) for i in [v] + reg])
        t_feat = np.concatenate([np.arange(len(s["ids"][i]), dtype=np.int32) for i in [v] + reg])
        t_id = np.concatenate([s["ids"][i] for i in [v] + reg])

        def fill_table():
            table.reset()
            table.set(t_img[t_id != -1], t_feat[t_id != -1], t_id[t_id != -1])
        fill_table()
        K = len(s["coords"][v])
        reg_a, cam_a = np.asarray(reg, np.int32), np.arange(1, len(reg) + 1, dtype=np.int32)      # camera row 0 is v's
        out = [torch.zeros(n, dtype=torch.int32, device=dev) for n in (1, K + 1, 2 * K, 4 * K, 3 * K)]

        def call():
            ctx.check(ctx.lib.rcn_new_view_tracks_device(ctx.h, v, len(reg), reg_a.ctypes.data, 0, cam_a.ctypes.data, K,
                                                         *[t.data_ptr() for t in out]))
        torch.cuda.synchronize()
        st = torch.cuda.Stream()                      # a stream of its own (handle 0 would mean the ctx's own stream)
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, st.cuda_stream))
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(a.reps):
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        n_tracks = int(out[0].item())
        if n_tracks != n_tracks_host:
            raise SystemExit("%s: the device found %d candidates, the host loop %d" % (name, n_tracks, n_tracks_host))
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, None))
        # the session entry, with made-up cameras: the pixels are random, so hardly a candidate is accepted; when one is, the
        # table is refilled outside the timed region so that every repetition starts from the same one
        ses = ba.BaSession(ctx)
        for k in range(len(reg) + 1):
            ses.add_camera([0.0, 0.02 * k, 0.0, 0.1 * k, 0.0, 5.0], [600.0, 600.0, 256.0, 168.0, 0.0, 0.0])
        P = ba.poses34_from_angle_axis(ses.cameras()[0])
        gms, added = [], 0
        src, status = np.zeros((K, 3), np.int32), np.zeros(K, np.uint8)
        n_found, first, n_added = C.c_int32(), C.c_int32(), C.c_int32()
        for r in range(a.reps + 3):
            t0 = time.perf_counter()
            ctx.check(ctx.lib.rcn_ba_session_grow_view(ses.h, P.ctypes.data, v, 0, len(reg), reg_a.ctypes.data, cam_a.ctypes.data, 4.0, 1.0,
                                                       C.byref(n_found), src.ctypes.data, status.ctypes.data, C.byref(first), C.byref(n_added)))
            t1 = time.perf_counter()
            if n_found.value != n_tracks_host:
                raise SystemExit("%s: grow_view found %d candidates, the host loop %d" % (name, n_found.value, n_tracks_host))
            if n_added.value:                             # the commit changed the table: the next repetition starts from the same one
                added += n_added.value
                fill_table()
            if r >= 3:
                gms.append(1e3 * (t1 - t0))
        ses.close()
        print(json.dumps({"tool": "new_view_tracks_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0),
                          "size": name, "images": len(s["coords"]), "keypoints_v": K, "registered_visited": len(reg),
                          "list_entries": int(offs[-1]), "free_features_v": int((s["ids"][v] == -1).sum()), "candidates": n_tracks,
                          "reps": a.reps, "device_ms": round(float(np.median(ms)), 4), "device_ms_min": round(float(np.min(ms)), 4),
                          "grow_view_ms": round(float(np.median(gms)), 4), "grow_view_ms_min": round(float(np.min(gms)), 4),
                          "grow_view_landmarks_added": added, "host_loop_ms": round(host_med, 4), "host_loop_ms_min": round(host_min, 4),
                          "scene_gen_s": round(gen_s, 1)}), flush=True)
        nextview.clear_lists(ctx)
        ctx.check(ctx.lib.rcn_coords_clear(ctx.h))
    ctx.close()


if __name__ == "__main__":
    main()
