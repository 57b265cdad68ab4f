"""Host mirror of the reference's two-view initialisation over librcn.so (no CPU fallback).

    SequentialReconstructor::chooseInitialPair            SequentialReconstructor.cpp:325-375
    GeometricFilter::estimateEssential                    GeometricFilter.cpp:10-37
    essentialMatToPose                                    SequentialReconstructor.cpp:284-317

cv::findEssentialMat in its two-camera form (5-point RANSAC) plus cv::recoverPose on the search's mask, for a batch of pairs
per call.  `choose_initial_pair` is the canonical choice of the pair (host code over the CSR
offsets), `two_view_init` takes host arrays, `two_view_init_device` pair ids against the resident lists and coordinates,
and ba.BaSession.init_pair starts a session from one pair.

`geometry` / `geometry_device` run the E search, the homography search (homography.py) and the classification of DESIGN.md
section 27 on the same entries in one call; `choose_initial_pair_by_geometry` walks the largest pairs down to the first one
that is not degenerate.
"""
import ctypes as C

import numpy as np

from . import _lib


def default_options(ctx):
    o = _lib.TwoViewOptions()
    ctx.lib.rcn_twoview_default_options(C.byref(o))
    return o


def choose_initial_pair(pairs, offsets):
    """The pair with the most matches, the lexicographically first (i, j) among equals (the reference sorts an
    unordered_map's entries with an unstable sort: its choice among equals is an accident).  pairs: n x (i, j) image ids,
    offsets: n + 1 CSR offsets of the pairs' lists.  Returns (i, j, index of the pair)."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    size = np.diff(np.asarray(offsets, np.int64))
    if len(pairs) == 0 or len(size) != len(pairs):
        raise ValueError("choose_initial_pair: n pairs need n + 1 offsets, n > 0")
    order = np.lexsort((pairs[:, 1], pairs[:, 0], -size))       # last key first: size descending, then i, then j
    k = int(order[0])
    return int(pairs[k, 0]), int(pairs[k, 1]), k


def pair_entries(qt, xy_a, xy_b):
    """One pair's list (n x (feature of a, feature of b), any order) -> its entries in canonical order (ascending query
    feature): (qt sorted, xy1, xy2)."""
    qt = np.asarray(qt, np.int32).reshape(-1, 2)
    qt = qt[np.argsort(qt[:, 0], kind="stable")]
    return qt, np.asarray(xy_a, np.int32).reshape(-1, 2)[qt[:, 0]], np.asarray(xy_b, np.int32).reshape(-1, 2)[qt[:, 1]]


def two_view_init(ctx, off, xy1, xy2, intr6_1, intr6_2, options=None):
    """rcn_twoview_init: pair p owns entries off[p] .. off[p + 1] of xy1 / xy2.  Returns dict(E[n_pairs, 9],
    pose34[n_pairs, 12], mask[total], cheir_mask[total], count[n_pairs, 2], iterations[n_pairs]); count[:, 0] -1: no model,
    -2: < 5 entries; count[:, 1] entries of the cheirality mask."""
    off = np.ascontiguousarray(off, np.int64)
    xy1 = np.ascontiguousarray(xy1, np.int32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.int32).reshape(-1, 2)
    npairs = len(off) - 1
    K1 = np.ascontiguousarray(intr6_1, np.float64).reshape(npairs, 6)
    K2 = np.ascontiguousarray(intr6_2, np.float64).reshape(npairs, 6)
    n = len(xy1)
    if len(xy2) != n:
        raise ValueError("two_view_init: xy1 and xy2 differ in length")
    out = dict(E=np.zeros((npairs, 9)), pose34=np.zeros((npairs, 12)), mask=np.zeros(max(n, 1), np.uint8),
               cheir_mask=np.zeros(max(n, 1), np.uint8), count=np.zeros((max(npairs, 1), 2), np.int32),
               iterations=np.zeros(max(npairs, 1), np.int32))
    ctx.check(ctx.lib.rcn_twoview_init(ctx.h, npairs, off.ctypes.data, xy1.ctypes.data if n else None, xy2.ctypes.data if n else None,
                                       K1.ctypes.data if npairs else None, K2.ctypes.data if npairs else None,
                                       C.byref(options) if options is not None else None, out["E"].ctypes.data,
                                       out["pose34"].ctypes.data, out["mask"].ctypes.data, out["cheir_mask"].ctypes.data,
                                       out["count"].ctypes.data, out["iterations"].ctypes.data))
    out["mask"], out["cheir_mask"] = out["mask"][:n], out["cheir_mask"][:n]
    out["count"], out["iterations"] = out["count"][:npairs], out["iterations"][:npairs]
    return out


def two_view_init_device(ctx, pairs, intr6_1, intr6_2, capacity, options=None, want_qt=True):
    """rcn_twoview_init_device: pairs n x (a, b) image ids (host), intr6_1 / intr6_2 float64 torch tensors in HBM (n x 6);
    the entries come from the resident lists (nextview.upload_feature_matches) and coordinates.  Only enqueues: returns
    device tensors dict(off, qt, E, pose34, mask, cheir_mask, count, iterations) that are valid after rcn_synchronize."""
    import torch
    dev = intr6_1.device
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n, cap = len(pairs), int(capacity)
    out = dict(off=torch.zeros(n + 1, dtype=torch.int64, device=dev), qt=torch.zeros((max(cap, 1), 2), dtype=torch.int32, device=dev),
               E=torch.zeros((n, 9), dtype=torch.float64, device=dev), pose34=torch.zeros((n, 12), dtype=torch.float64, device=dev),
               mask=torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev), cheir_mask=torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev),
               count=torch.zeros((max(n, 1), 2), dtype=torch.int32, device=dev), iterations=torch.zeros(max(n, 1), dtype=torch.int32, device=dev))
    ctx.check(ctx.lib.rcn_twoview_init_device(ctx.h, n, pairs.ctypes.data if n else None, intr6_1.data_ptr(), intr6_2.data_ptr(),
                                              C.byref(options) if options is not None else None, cap, out["off"].data_ptr(),
                                              out["qt"].data_ptr() if want_qt else None, out["E"].data_ptr(), out["pose34"].data_ptr(),
                                              out["mask"].data_ptr(), out["cheir_mask"].data_ptr(), out["count"].data_ptr(),
                                              out["iterations"].data_ptr()))
    return out


LABELS = ("NO_MODEL", "PANORAMIC", "PLANAR", "SMALL_BASELINE", "GENERAL")       # RCN_TV_* of include/rcn.h
NO_MODEL, PANORAMIC, PLANAR, SMALL_BASELINE, GENERAL = range(5)


def geometry_default_options(ctx):
    o = _lib.TwoViewGeometryOptions()
    ctx.lib.rcn_twoview_geometry_default_options(C.byref(o))
    return o


def _ref(o):
    return C.byref(o) if o is not None else None


def geometry(ctx, off, xy1, xy2, intr6_1, intr6_2, options=None, tv_options=None, h_options=None):
    """rcn_twoview_geometry: two_view_init's outputs (the same bits), homography.find's as H, h_mask, h_count, h_iterations
    (the same bits), and per pair ratio = count_H / count_E, median_angle (lower median of the parallax angle over the
    cheirality mask, in the loop's 180 acos / 3.1415 unit) and label (index into LABELS)."""
    off = np.ascontiguousarray(off, np.int64)
    xy1 = np.ascontiguousarray(xy1, np.int32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.int32).reshape(-1, 2)
    npairs = len(off) - 1
    K1 = np.ascontiguousarray(intr6_1, np.float64).reshape(npairs, 6)
    K2 = np.ascontiguousarray(intr6_2, np.float64).reshape(npairs, 6)
    n = len(xy1)
    if len(xy2) != n:
        raise ValueError("geometry: xy1 and xy2 differ in length")
    m, q = max(n, 1), max(npairs, 1)
    out = dict(E=np.zeros((npairs, 9)), pose34=np.zeros((npairs, 12)), mask=np.zeros(m, np.uint8), cheir_mask=np.zeros(m, np.uint8),
               count=np.zeros((q, 2), np.int32), iterations=np.zeros(q, np.int32), H=np.zeros((npairs, 9)), h_mask=np.zeros(m, np.uint8),
               h_count=np.zeros(q, np.int32), h_iterations=np.zeros(q, np.int32), ratio=np.zeros(q), median_angle=np.zeros(q),
               label=np.zeros(q, np.int32))
    ctx.check(ctx.lib.rcn_twoview_geometry(ctx.h, npairs, off.ctypes.data, xy1.ctypes.data if n else None, xy2.ctypes.data if n else None,
                                           K1.ctypes.data if npairs else None, K2.ctypes.data if npairs else None, _ref(tv_options),
                                           _ref(h_options), _ref(options), *[out[k].ctypes.data for k in
                                           ("E", "pose34", "mask", "cheir_mask", "count", "iterations", "H", "h_mask", "h_count",
                                            "h_iterations", "ratio", "median_angle", "label")]))
    for k in ("mask", "cheir_mask", "h_mask"):
        out[k] = out[k][:n]
    for k in ("count", "iterations", "h_count", "h_iterations", "ratio", "median_angle", "label"):
        out[k] = out[k][:npairs]
    return out


def geometry_device(ctx, pairs, intr6_1, intr6_2, capacity, options=None, tv_options=None, h_options=None, want_qt=True):
    """rcn_twoview_geometry_device: as two_view_init_device, with the homography's and the classification's outputs beside
    the E search's.  Only enqueues: the device tensors are valid after rcn_synchronize."""
    import torch
    dev = intr6_1.device
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n, cap = len(pairs), int(capacity)
    m, q = max(cap, 1), max(n, 1)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)      # noqa: E731
    out = dict(off=z(n + 1, torch.int64), qt=z((m, 2), torch.int32), E=z((q, 9), torch.float64), pose34=z((q, 12), torch.float64),
               mask=z(m, torch.uint8), cheir_mask=z(m, torch.uint8), count=z((q, 2), torch.int32), iterations=z(q, torch.int32),
               H=z((q, 9), torch.float64), h_mask=z(m, torch.uint8), h_count=z(q, torch.int32), h_iterations=z(q, torch.int32),
               ratio=z(q, torch.float64), median_angle=z(q, torch.float64), label=z(q, torch.int32))
    ctx.check(ctx.lib.rcn_twoview_geometry_device(ctx.h, n, pairs.ctypes.data if n else None, intr6_1.data_ptr(), intr6_2.data_ptr(),
                                                  _ref(tv_options), _ref(h_options), _ref(options), cap, out["off"].data_ptr(),
                                                  out["qt"].data_ptr() if want_qt else None, *[out[k].data_ptr() for k in
                                                  ("E", "pose34", "mask", "cheir_mask", "count", "iterations", "H", "h_mask", "h_count",
                                                   "h_iterations", "ratio", "median_angle", "label")]))
    return out


def choose_initial_pair_by_geometry(ctx, pairs, offsets, xy1, xy2, intr6_1, intr6_2, options=None, tv_options=None, h_options=None):
    """The initial pair with a degeneracy check.  pairs n x (i, j), offsets n + 1 CSR offsets into xy1 / xy2 (every pair's
    entries in ascending query-feature order), intr6_1 / intr6_2 n x 6.  The candidates are the top_m pairs in
    choose_initial_pair's order (size descending, then (i, j)); one geometry call runs on all of them; the choice is the first
    GENERAL candidate, else the first PLANAR one (a moving camera in front of a plane is not degenerate for five points),
    else candidate 0 with fallback=True: the reference's choice.  Returns dict(pair=(i, j), index, position, fallback,
    pose34, E, count, candidates=indices of the candidates, table=the geometry call's outputs over the candidates)."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    offsets = np.asarray(offsets, np.int64)
    size = np.diff(offsets)
    if len(pairs) == 0 or len(size) != len(pairs):
        raise ValueError("choose_initial_pair_by_geometry: n pairs need n + 1 offsets, n > 0")
    o = options if options is not None else geometry_default_options(ctx)
    if o.top_m < 1:
        raise ValueError("choose_initial_pair_by_geometry: top_m >= 1")
    order = np.lexsort((pairs[:, 1], pairs[:, 0], -size))[:int(o.top_m)]
    xy1 = np.asarray(xy1, np.int32).reshape(-1, 2)
    xy2 = np.asarray(xy2, np.int32).reshape(-1, 2)
    K1 = np.asarray(intr6_1, np.float64).reshape(len(pairs), 6)
    K2 = np.asarray(intr6_2, np.float64).reshape(len(pairs), 6)
    sel = [np.arange(offsets[k], offsets[k + 1]) for k in order]
    idx = np.concatenate(sel) if sel else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sel])]).astype(np.int64)
    table = geometry(ctx, off, xy1[idx], xy2[idx], K1[order], K2[order], o, tv_options, h_options)
    pos, fallback = 0, True
    for want in (GENERAL, PLANAR):
        hit = np.flatnonzero(table["label"] == want)
        if len(hit):
            pos, fallback = int(hit[0]), False
            break
    k = int(order[pos])
    return dict(pair=(int(pairs[k, 0]), int(pairs[k, 1])), index=k, position=pos, fallback=fallback, pose34=table["pose34"][pos].copy(),
                E=table["E"][pos].copy(), count=table["count"][pos].copy(), candidates=[int(v) for v in order], table=table)


def pose6_from_pose34(ctx, pose34):
    """rcn_pose34_to_pose6: the camera block (angle-axis, translation) rcn_ba_session_init_pair stores for the pose."""
    p = np.ascontiguousarray(pose34, np.float64).reshape(12)
    out = np.zeros(6)
    ctx.check(ctx.lib.rcn_pose34_to_pose6(p.ctypes.data, out.ctypes.data))
    return out


def smoke(ctx, seed=4, n=300, wrong_share=0.3):
    """One seeded pair of n entries with a share of wrong matches: the planted relative pose is recovered up to the unit
    baseline (used by __graft_entry__.smoke).  Returns (count, planted, iterations, rotation error in rad, angle between
    the translation directions in rad)."""
    rng = np.random.default_rng(seed)
    K1 = np.array([900.0, 910.0, 640.0, 480.0, 0.0, 0.0])
    K2 = np.array([880.0, 905.0, 650.0, 470.0, 0.0, 0.0])
    w = rng.normal(0, 0.15, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(0, 1, 3)
    t /= np.linalg.norm(t)
    X = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2, 2, n), rng.uniform(3, 8, n)], 1)
    Y = X @ R.T + t
    p1 = np.stack([K1[0] * X[:, 0] / X[:, 2] + K1[2], K1[1] * X[:, 1] / X[:, 2] + K1[3]], 1)
    p2 = np.stack([K2[0] * Y[:, 0] / Y[:, 2] + K2[2], K2[1] * Y[:, 1] / Y[:, 2] + K2[3]], 1)
    bad = rng.random(n) < wrong_share
    p2[bad] = np.stack([rng.uniform(0, 1280, int(bad.sum())), rng.uniform(0, 960, int(bad.sum()))], 1)
    r = two_view_init(ctx, [0, n], np.trunc(p1).astype(np.int32), np.trunc(p2).astype(np.int32), K1, K2)
    planted = int((~bad).sum())
    count, cheir = int(r["count"][0, 0]), int(r["count"][0, 1])
    assert count == int(r["mask"].sum()) and cheir == int(r["cheir_mask"].sum()), "two-view: counts differ from the masks"
    assert count >= 0.8 * planted and cheir >= 0.95 * count, "two-view: %d inliers (%d in front) of %d planted" % (count, cheir, planted)
    P = r["pose34"].reshape(3, 4)
    rot = float(np.arccos(np.clip((np.trace(P[:, :3] @ R.T) - 1) / 2, -1, 1)))
    tdir = float(np.arccos(np.clip(P[:, 3] @ t, -1, 1)))
    assert rot <= 2e-2 and tdir <= 5e-2, "two-view: planted pose not recovered (rotation %.2e rad, translation %.2e rad)" % (rot, tdir)
    return count, planted, int(r["iterations"][0]), rot, tdir


def _smoke_pair(seed, n, wrong_share, baseline):
    rng = np.random.default_rng(seed)
    K1 = np.array([900.0, 910.0, 640.0, 480.0, 0.0, 0.0])
    K2 = np.array([880.0, 905.0, 650.0, 470.0, 0.0, 0.0])
    w = rng.normal(0, 0.15, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(0, 1, 3)
    t *= baseline / np.linalg.norm(t)
    X = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2, 2, n), rng.uniform(3, 8, n)], 1)
    Y = X @ R.T + t
    p1 = np.stack([K1[0] * X[:, 0] / X[:, 2] + K1[2], K1[1] * X[:, 1] / X[:, 2] + K1[3]], 1)
    p2 = np.stack([K2[0] * Y[:, 0] / Y[:, 2] + K2[2], K2[1] * Y[:, 1] / Y[:, 2] + K2[3]], 1)
    bad = rng.random(n) < wrong_share
    p2[bad] = np.stack([rng.uniform(0, 1280, int(bad.sum())), rng.uniform(0, 960, int(bad.sum()))], 1)
    return np.trunc(p1).astype(np.int32), np.trunc(p2).astype(np.int32), K1, K2


def smoke_geometry(ctx, seed=6, n=300, wrong_share=0.2):
    """One seeded general pair and one seeded pure rotation (baseline 0) through `geometry` in one call: GENERAL and
    PANORAMIC.  The E search runs without its depth cut (distance_threshold 1e9): at 50 baselines it drops exactly the
    entries without parallax, and a pure rotation would end as NO_MODEL (section 27).  Returns (labels, ratios, angles)."""
    a1, a2, K1, K2 = _smoke_pair(seed, n, wrong_share, 1.0)
    b1, b2, _, _ = _smoke_pair(seed + 1, n, wrong_share, 0.0)
    tv = default_options(ctx)
    tv.distance_threshold = 1e9
    r = geometry(ctx, [0, n, 2 * n], np.concatenate([a1, b1]), np.concatenate([a2, b2]), [K1, K1], [K2, K2], tv_options=tv)
    labels = [LABELS[int(v)] for v in r["label"]]
    assert labels == ["GENERAL", "PANORAMIC"], "two-view geometry: labels %s, ratios %s, angles %s" % (labels, r["ratio"], r["median_angle"])
    assert int(r["h_count"][0]) == int(r["h_mask"][:n].sum()) and int(r["h_count"][1]) == int(r["h_mask"][n:].sum()), "two-view geometry: H counts differ from the masks"
    return labels, [float(v) for v in r["ratio"]], [float(v) for v in r["median_angle"]]
