"""Times of guided matching on cfg-2-shaped data -- n images x K rows x D = 256 over one synthetic cloud seen by n
cameras -- and of the parent's match + filter on the same pairs in the same run: HIP events on a stream of its own around each call,
warm-up calls first, median of --reps.

It records
    parent_match_filter_ms     rcn_match_grid_device + rcn_match_table_filter_device (what the pair loop ran until now)
    filter_model_ms            rcn_match_grid_device + rcn_match_table_filter_model_device (the same, keeping F: the guided grid's input)
    guided_grid_ms             rcn_match_guided_device alone on the filter's models, one-way and cross-checked
    grid_guided_ms             rcn_match_grid_guided as a whole (host results: the copy of the table is inside)
    guided_over_parent         guided_grid_ms / parent_match_filter_ms: the figure the issue asks for
    candidates                 in-band (query, train) combinations and their share of K x K
    repeated                   a second scene whose descriptors repeat (every world descriptor is worn by two points far apart): matches and
                               correct matches (by world point) of the filtered table and of the guided table
Nothing here is a pass condition.  Writes one JSON document, stamped with the source hash, to profiles/guided_timing.json (and prints it).

    python tools/guided_timing.py [--images 100] [--rows 4096] [--reps 3] [--out profiles/guided_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(n, K, D, seed, repeat=False, noise=0.08):
    """n images of K keypoints of one cloud of 4 K points: rows [n][K][D] float32 (unit norm), coordinates [n][K][2] int32, world ids [n][K].
    repeat: points w and w + 2 K wear the same descriptor (a repeated structure)."""
    rng = np.random.default_rng(seed)
    W = 4 * K
    base = rng.standard_normal((W, D)).astype(np.float32)
    if repeat:
        base[W // 2:] = base[:W // 2]
    X = np.c_[rng.uniform(-3, 3, W), rng.uniform(-2, 2, W), rng.uniform(6, 12, W)]
    Kc = np.array([[1200., 0, 1000], [0, 1200., 750], [0, 0, 1]])
    rows = np.empty((n, K, D), np.float32)
    xy = np.empty((n, K, 2), np.int32)
    ids = np.empty((n, K), np.int32)
    for i in range(n):
        ang = 0.004 * i
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        tr = np.array([-0.05 * i, 0.004 * i, 0.01 * i])
        sel = rng.permutation(W)[:K]
        r = base[sel] + np.float32(noise) * rng.standard_normal((K, D)).astype(np.float32)
        rows[i] = r / np.linalg.norm(r, axis=1, keepdims=True)
        p = (Kc @ ((R @ X[sel].T).T + tr).T).T
        xy[i] = np.rint(p[:, :2] / p[:, 2:] + rng.normal(0, 0.5, (K, 2))).astype(np.int32)
        ids[i] = sel
    return rows, xy, ids


def timed(st, reps, fn, warm=1):
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
    return round(float(np.median(ms)), 3), round(float(np.min(ms)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--repeat-images", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_timing.json"))
    a = ap.parse_args()
    import torch
    import bench
    from reconstructor_amd import _lib, guided
    from reconstructor_amd.matcher import HipL2Matcher, all_pairs
    ctx = _lib.Context(0)
    lib, h = ctx.lib, ctx.h
    m = HipL2Matcher(ctx=ctx)
    st = torch.cuda.Stream()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    doc = {"tool": "guided_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "warm_up": 1}

    def load(rows, xy):
        m.clear()
        dev = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        m.upload_batch_device(0, len(rows), dev.data_ptr(), rows.shape[1], rows.shape[2])
        m.upload_coords_batch(0, list(xy))
        return dev

    n, K, D = a.images, a.rows, a.dim
    pairs = all_pairs(n)
    n_pairs = len(pairs)
    rows, xy, _ = scene(n, K, D, seed=1)
    keep = load(rows, xy)
    out = torch.empty((n_pairs, K), dtype=torch.int32, device="cuda")
    cnt = torch.empty((n_pairs,), dtype=torch.int32, device="cuda")
    ver = torch.empty((n_pairs,), dtype=torch.int32, device="cuda")
    F = torch.zeros((n_pairs, 9), dtype=torch.float64, device="cuda")
    out_g = torch.empty((n_pairs, K), dtype=torch.int32, device="cuda")
    cnt_g = torch.empty((n_pairs,), dtype=torch.int32, device="cuda")
    cand = torch.zeros((n_pairs,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.check(lib.rcn_set_stream(h, st.cuda_stream))
    pp = pairs.ctypes.data

    def parent():
        ctx.check(lib.rcn_match_grid_device(h, pp, n_pairs, 0.7, P(out), K, P(cnt)))
        ctx.check(lib.rcn_match_table_filter_device(h, pp, n_pairs, P(out), K, P(cnt), P(ver)))

    def with_model():
        ctx.check(lib.rcn_match_grid_device(h, pp, n_pairs, 0.7, P(out), K, P(cnt)))
        ctx.check(lib.rcn_match_table_filter_model_device(h, pp, n_pairs, P(out), K, P(cnt), P(ver), P(F)))

    def guided_grid(opt):
        return lambda: ctx.check(lib.rcn_match_guided_device(h, pp, n_pairs, P(F), C.byref(opt), P(out_g), K, P(cnt_g), P(cand)))

    r = {"n": n, "K": K, "D": D, "pairs": n_pairs}
    r["parent_match_filter_ms"], r["parent_match_filter_ms_min"] = timed(st, a.reps, parent)
    r["filter_model_ms"], r["filter_model_ms_min"] = timed(st, a.reps, with_model)
    st.synchronize()
    r["pairs_with_model"] = int((ver > 0).sum().item())
    r["matches_filtered"] = int(cnt.sum().item())
    one, cross = guided.options(), guided.options(cross_check=1)
    r["guided_grid_ms"], r["guided_grid_ms_min"] = timed(st, a.reps, guided_grid(one))
    st.synchronize()
    r["matches_guided"] = int(cnt_g.sum().item())
    r["candidates"] = int(cand.sum().item())
    r["candidates_per_row"] = round(r["candidates"] / max(1, r["pairs_with_model"] * K), 2)
    r["candidate_share_of_KxK"] = float("%.3g" % (r["candidates"] / max(1, r["pairs_with_model"] * K * K)))
    r["guided_grid_cross_ms"], r["guided_grid_cross_ms_min"] = timed(st, a.reps, guided_grid(cross))
    st.synchronize()
    r["matches_guided_cross"] = int(cnt_g.sum().item())
    host_out = np.empty((n_pairs, K), np.int32)
    host_cnt, host_ver = np.empty(n_pairs, np.int32), np.empty(n_pairs, np.int32)

    def whole():
        ctx.check(lib.rcn_match_grid_guided(h, pp, n_pairs, 0.7, C.byref(one), host_out.ctypes.data, K, host_cnt.ctypes.data, host_ver.ctypes.data))

    r["grid_guided_ms"], r["grid_guided_ms_min"] = timed(st, a.reps, whole)
    r["guided_over_parent"] = round(r["guided_grid_ms"] / r["parent_match_filter_ms"], 3)
    doc["cfg2"] = r
    del keep, out, cnt, ver, F, out_g, cnt_g, cand
    torch.cuda.empty_cache()

    # the matches gained where descriptors repeat
    n2 = a.repeat_images
    rows, xy, ids = scene(n2, K, D, seed=2, repeat=True)
    keep = load(rows, xy)
    pairs2 = all_pairs(n2)
    opt = guided.options()
    table, counts, status = guided.grid_guided(ctx, pairs2, K, 0.7, opt)
    base_t = torch.empty((len(pairs2), K), dtype=torch.int32, device="cuda")
    base_c = torch.empty((len(pairs2),), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.match_grid_device(pairs2, base_t.data_ptr(), K, base_c.data_ptr())
    m.filter_table_device(pairs2, base_t.data_ptr(), K, base_c.data_ptr())
    ctx.check(lib.rcn_synchronize(h))
    base = base_t.cpu().numpy()

    def correct(tab):
        good = 0
        for p, (i, j) in enumerate(pairs2):
            q = np.flatnonzero(tab[p] >= 0)
            good += int((ids[i][q] == ids[j][tab[p][q]]).sum())
        return good
    doc["repeated"] = {"n": n2, "K": K, "pairs": len(pairs2), "pairs_with_model": int((status > 0).sum()),
                       "matches_filtered": int((base >= 0).sum()), "correct_filtered": correct(base),
                       "matches_guided": int((table >= 0).sum()), "correct_guided": correct(table)}
    del keep
    ctx.check(lib.rcn_set_stream(h, None))
    m.clear()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
