"""Device time of rcn_corr_2d3d_device (the next-view search) at three sizes, HIP events around the
call after warm-up; prints one JSON line per size.

    python tools/next_view_timing.py [--reps 20]

Scenes are generated in numpy from a seed (no Python transcription: the large case has ~10^6 observations):
  ref25   25 images x 1500 keypoints, 12 registered
  v200    200 images x 2000 keypoints, 100 registered
  big     1000 images x 4096 keypoints, 500 registered, ~300k landmarks
Every image sees a random subset of the scene points; a pair's list holds the points both images see (sampled down to at
most `per_pair` matches, canonical i < j, mirror on); landmarks are the points seen by >= 2 registered images, their tracks
those observations.  Bytes moved are counted from the kernels' own traffic model."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s achievable)


def scene(n_img, K, n_reg, n_pts, vis, per_pair, seed):
    rng = np.random.default_rng(seed)
    point_of = []
    for i in range(n_img):
        p = rng.choice(n_pts, size=min(K, int(vis * n_pts)), replace=False)
        point_of.append(p.astype(np.int64))
    coords = [np.column_stack([rng.integers(-8, 520, len(p)), rng.integers(-8, 344, len(p))]).astype(np.int32) for p in point_of]
    feat_of = []
    for p in point_of:
        m = np.full(n_pts, -1, np.int64)
        m[p] = np.arange(len(p))
        feat_of.append(m)
    pairs, offs, qt = [], [0], []
    for i in range(n_img):
        for j in range(i + 1, n_img):
            common = point_of[i][feat_of[j][point_of[i]] >= 0]
            if len(common) > per_pair:
                common = rng.choice(common, per_pair, replace=False)
            if not len(common):
                continue
            pairs.append((i, j))
            qt.append(np.column_stack([feat_of[i][common], feat_of[j][common]]))
            offs.append(offs[-1] + len(common))
    qt = np.concatenate(qt).astype(np.int32)
    img = np.concatenate([np.full(len(point_of[i]), i) for i in range(n_reg)])
    feat = np.concatenate([np.arange(len(point_of[i])) for i in range(n_reg)])
    pts = np.concatenate([point_of[i] for i in range(n_reg)])
    order = np.lexsort((rng.random(len(pts)), pts))
    img, feat, pts = img[order], feat[order], pts[order]
    cnt = np.bincount(pts, minlength=n_pts)
    keep = cnt[pts] >= 2
    img, feat, pts = img[keep], feat[keep], pts[keep]
    _, starts = np.unique(pts, return_index=True)
    pt_off = np.append(starts, len(pts)).astype(np.int32)
    return {"coords": coords, "pairs": np.asarray(pairs, np.int32), "offsets": np.asarray(offs, np.int64), "qt": qt,
            "pt_off": pt_off, "obs_img": img.astype(np.int32), "obs_feat": feat.astype(np.int32),
            "cand": np.arange(n_reg, n_img, dtype=np.int32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="ref25,v200,big")
    a = ap.parse_args()
    import torch
    from reconstructor_amd import _lib, nextview
    ctx = _lib.Context(0)
    cfg = {"ref25": (25, 1500, 12, 3000, 0.5, 400, 1), "v200": (200, 2000, 100, 40000, 0.05, 200, 2),
           "big": (1000, 4096, 500, 330000, 0.01241, 64, 3)}
    for name in a.sizes.split(","):
        t0 = time.time()
        s = scene(*cfg[name])
        gen_s = time.time() - t0
        for i, xy in enumerate(s["coords"]):
            ctx.check(ctx.lib.rcn_coords_upload(ctx.h, i, xy.ctypes.data, len(xy)))
        nextview.upload_lists(ctx, s["pairs"], s["offsets"], s["qt"], mirror=True)
        dev = torch.device("cuda", 0)
        g = [torch.as_tensor(s[k]).to(dev) for k in ("pt_off", "obs_img", "obs_feat", "cand")]
        shp = torch.tensor([[336, 512]] * len(s["cand"]), dtype=torch.int32, device=dev)
        n_cand, n_obs, n_pts = len(s["cand"]), len(s["obs_img"]), len(s["pt_off"]) - 1
        coff = torch.zeros(n_cand + 1, dtype=torch.int64, device=dev)
        cap = 1 << 26
        lm = torch.empty(cap, dtype=torch.int32, device=dev)
        ft = torch.empty(cap, dtype=torch.int32, device=dev)
        tot = torch.zeros(1, dtype=torch.int64, device=dev)
        cells = torch.zeros(n_cand, dtype=torch.int32, device=dev)
        outside = torch.zeros(n_cand, dtype=torch.int32, device=dev)

        def call():
            ctx.check(ctx.lib.rcn_corr_2d3d_device(ctx.h, n_pts, n_obs, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), n_cand,
                                                   g[3].data_ptr(), shp.data_ptr(), coff.data_ptr(), lm.data_ptr(), ft.data_ptr(),
                                                   cap, tot.data_ptr(), cells.data_ptr(), outside.data_ptr()))
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
        total = int(tot.item())
        ld = max(1, (n_obs + 4095) // 4096) * 4096
        n_ent = int(s["offsets"][-1])
        # hit rows: memset + compaction read, plus the walk's scattered 4-byte stores; lists read once per candidate batch
        byts = 2 * 4 * ld * n_cand + 4 * total + 8 * n_ent * max(1, -(-n_cand * 4 * ld // (1 << 30))) + 8 * total + 12 * n_obs
        med = float(np.median(ms))
        print(json.dumps({"size": name, "images": len(s["coords"]), "registered": int(len(s["coords"]) - n_cand), "landmarks": n_pts,
                          "observations": n_obs, "list_entries": n_ent, "candidates": n_cand, "entries_out": total,
                          "ms_median": round(med, 4), "ms_min": round(float(np.min(ms)), 4), "bytes_model": int(byts),
                          "gb_per_s": round(byts / med / 1e6, 1), "frac_hbm_peak": round(byts / med / 1e-3 / HBM_PEAK, 3),
                          "scene_gen_s": round(gen_s, 1)}), flush=True)
        ctx.check(ctx.lib.rcn_set_stream(ctx.h, None))
        ctx.check(ctx.lib.rcn_coords_clear(ctx.h))
    ctx.close()


if __name__ == "__main__":
    main()
