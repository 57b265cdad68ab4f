"""Host mirror of the deterministic part of the reference's addNextView over librcn.so (no CPU fallback).

    SequentialReconstructor::calc2d3dMatches              SequentialReconstructor.cpp:643-695
    SequentialReconstructor::rankNextImages               SequentialReconstructor.cpp:697-759
    step 1 of triangulateMatchedLandmarks                 SequentialReconstructor.cpp:497-512 (ba.BaSession.attach)

The match lists featureMatches[(a, b)] are uploaded once (`upload_lists` / `upload_feature_matches`) and stay in HBM; every
call of `corr_2d3d` then takes the landmark graph (CSR over the tracks, (image, feature) per observation) and the candidates
and returns, per candidate, the (landmark, feature) entries in the reference's order and the MatchDensity score.
DESIGN.md section 16 says why the list walk reproduces the reference's loop.
"""
import ctypes as C

import numpy as np

from . import _lib

MIN_2D3D_MATCH_NUM = 30          # SequentialReconstructor.h:240
MATCH_DENSITY, MATCH_TOTAL = "density", "total"
ATTACHED, REJECT_DEPTH, REJECT_REPROJECTION, REJECT_TAKEN = 0, 1, 2, 3


def lists_from_dict(feature_matches):
    """{(a, b): {feature of a: feature of b}} (or any iterable of (f, g) pairs per key) -> (pairs[n, 2], offsets[n + 1] int64,
    qt[total, 2]) in the dict's key order and each map's own order: rcn_match_compact_begin's layout."""
    pairs, offs, qt = [], [0], []
    for (a, b), m in feature_matches.items():
        items = list(m.items()) if hasattr(m, "items") else list(m)
        pairs.append((int(a), int(b)))
        qt.extend((int(f), int(g)) for f, g in items)
        offs.append(len(qt))
    return (np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(offs, np.int64),
            np.asarray(qt, np.int32).reshape(-1, 2))


def upload_lists(ctx, pairs, offsets, qt, mirror=False):
    """rcn_match_lists_upload: the directed lists stay resident in the ctx until the next upload.  mirror: a directed pair
    that was not given but whose reverse was is that reverse's inverse."""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    offsets = np.ascontiguousarray(offsets, np.int64)
    qt = np.ascontiguousarray(qt, np.int32).reshape(-1, 2)
    if len(offsets) != len(pairs) + 1:
        raise ValueError("offsets needs n_pairs + 1 entries")
    ctx.check(ctx.lib.rcn_match_lists_upload(ctx.h, len(pairs), pairs.ctypes.data, offsets.ctypes.data,
                                             qt.ctypes.data if len(qt) else None, 1 if mirror else 0))


def upload_feature_matches(ctx, feature_matches, mirror=False):
    upload_lists(ctx, *lists_from_dict(feature_matches), mirror=mirror)


def clear_lists(ctx):
    ctx.check(ctx.lib.rcn_match_lists_clear(ctx.h))


def set_workspace_bytes(ctx, nbytes):
    ctx.check(ctx.lib.rcn_corr_set_workspace_bytes(ctx.h, int(nbytes)))


def graph_arrays(tracks):
    """Tracks [[(image, feature), ...], ...] in landmark order -> (pt_off, obs_img, obs_feat)."""
    off = np.zeros(len(tracks) + 1, np.int32)
    img, feat = [], []
    for j, t in enumerate(tracks):
        for i, f in t:
            img.append(int(i))
            feat.append(int(f))
        off[j + 1] = len(img)
    return off, np.asarray(img, np.int32), np.asarray(feat, np.int32)


def corr_2d3d(ctx, pt_off, obs_img, obs_feat, candidates, shapes, capacity=None):
    """calc2d3dMatches + the MatchDensity score for every candidate (rcn_corr_2d3d).  shapes: (rows, cols) per candidate.
    Returns (cand_off[n_cand + 1] int64, landmark[total], feature[total], cells[n_cand], outside[n_cand]): candidate k's
    entries are landmark / feature[cand_off[k]:cand_off[k + 1]] in the reference's order."""
    off = np.ascontiguousarray(pt_off, np.int32)
    img = np.ascontiguousarray(obs_img, np.int32)
    feat = np.ascontiguousarray(obs_feat, np.int32)
    cand = np.ascontiguousarray(candidates, np.int32)
    shp = np.ascontiguousarray(shapes, np.int32).reshape(-1, 2)
    if len(shp) != len(cand):
        raise ValueError("one (rows, cols) per candidate")
    n = len(cand)
    cap = int(capacity) if capacity is not None else max(1, min(len(img) * max(n, 1), 1 << 22))
    coff = np.zeros(n + 1, np.int64)
    cells, outside = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    total = C.c_int64(0)
    for _ in range(2):
        lm, ft = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        rc = ctx.lib.rcn_corr_2d3d(ctx.h, len(off) - 1, off.ctypes.data, img.ctypes.data if len(img) else None,
                                   feat.ctypes.data if len(img) else None, n, cand.ctypes.data if n else None,
                                   shp.ctypes.data if n else None, coff.ctypes.data, lm.ctypes.data, ft.ctypes.data, cap,
                                   C.byref(total), cells.ctypes.data, outside.ctypes.data)
        if rc != _lib.RCN_OK and total.value > cap and capacity is None:      # too small a guess: once more, exactly sized
            cap = int(total.value)
            continue
        ctx.check(rc)
        break
    t = int(total.value)
    return coff, lm[:t], ft[:t], cells[:n], outside[:n]


def corr_2d3d_device(ctx, pt_off, obs_img, obs_feat, candidates, shapes, capacity):
    """rcn_corr_2d3d_device on torch tensors in HBM (inputs may be numpy; they are copied to the device first).  Returns
    device tensors (cand_off, landmark[capacity], feature[capacity], total[1], cells, outside)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a: a.to(dev).contiguous() if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, np.int32)).to(dev)
    off, img, feat, cand = t(pt_off), t(obs_img), t(obs_feat), t(candidates)
    shp = t(shapes).reshape(-1, 2)
    n = cand.numel()
    coff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    lm = torch.full((max(int(capacity), 1),), -7, dtype=torch.int32, device=dev)
    ft = torch.full((max(int(capacity), 1),), -7, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    cells = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    outside = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.rcn_corr_2d3d_device(ctx.h, off.numel() - 1, img.numel(), off.data_ptr(), img.data_ptr(), feat.data_ptr(), n,
                                           cand.data_ptr(), shp.data_ptr(), coff.data_ptr(), lm.data_ptr(), ft.data_ptr(),
                                           int(capacity), total.data_ptr(), cells.data_ptr(), outside.data_ptr()))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return coff, lm, ft, total, cells[:n], outside[:n]


def rank_next_images(candidates, counts, scores, mode=MATCH_DENSITY, min_matches=MIN_2D3D_MATCH_NUM):
    """rankNextImages over per-candidate entry counts and density scores, as a deterministic rule:
    MATCH_DENSITY  candidates with score > min_matches, score descending, then image id ascending; ties are kept.  The
                   reference's std::map<score, imgId> keeps only one image per score (whichever its unordered_map iteration
                   reaches last), so the first element equals the reference's choice whenever the top score is unique.
    MATCH_TOTAL    every candidate, image id descending (the reference's map is keyed by image id, :703-713: the counts do
                   not order anything)."""
    cand = [int(c) for c in candidates]
    if mode == MATCH_TOTAL:
        return sorted(cand, reverse=True)
    if mode != MATCH_DENSITY:
        raise ValueError("Wrong next image ranking mode!")
    sc = [int(s) for s in scores]
    keep = [(s, c) for s, c in zip(sc, cand) if s > min_matches]
    return [c for s, c in sorted(keep, key=lambda t: (-t[0], t[1]))]


def attach(ctx, pose34, intr6, points, landmark, feat, xy, max_projection_error=4.0):
    """Step 1 of triangulateMatchedLandmarks (rcn_landmark_attach): status per entry (0 attached, 1 depth, 2 reprojection,
    3 feature already taken by an earlier attached entry)."""
    P = np.ascontiguousarray(pose34, np.float64).reshape(12)
    K = np.ascontiguousarray(intr6, np.float64).reshape(6)
    X = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    lm = np.ascontiguousarray(landmark, np.int32)
    ft = np.ascontiguousarray(feat, np.int32)
    xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    n = len(lm)
    st = np.zeros(max(n, 1), np.uint8)
    cnt = C.c_int32(0)
    ctx.check(ctx.lib.rcn_landmark_attach(ctx.h, P.ctypes.data, K.ctypes.data, len(X), X.ctypes.data if len(X) else None, n,
                                          lm.ctypes.data if n else None, ft.ctypes.data if n else None, xy.ctypes.data if n else None,
                                          float(max_projection_error), st.ctypes.data, C.byref(cnt)))
    return st[:n]
