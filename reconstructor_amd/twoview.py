"""Host mirror of the reference's two-view initialisation over librcn.so (no CPU fallback).

    SequentialReconstructor::chooseInitialPair            SequentialReconstructor.cpp:325-375
    GeometricFilter::estimateEssential                    GeometricFilter.cpp:10-37
    essentialMatToPose                                    SequentialReconstructor.cpp:284-317

cv::findEssentialMat in its two-camera form (5-point RANSAC) plus cv::recoverPose on the search's mask, for a batch of pairs
per call.  `choose_initial_pair` is the canonical choice of the pair (host code over the CSR
offsets), `two_view_init` takes host arrays, `two_view_init_device` pair ids against the resident lists and coordinates,
and ba.BaSession.init_pair starts a session from one pair.
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
