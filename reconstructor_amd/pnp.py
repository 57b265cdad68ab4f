"""Host mirror of the reference's registerImagePnP over librcn.so (no CPU fallback).

    SequentialReconstructor::registerImagePnP             SequentialReconstructor.cpp:559-638

cv::solvePnPRansac in its P3P mode plus a refit on the inliers, for a batch of views per call.
`pnp_ransac` takes host arrays, `pnp_ransac_device` torch tensors in HBM (what nextview.corr_2d3d_device left), and
ba.BaSession.pnp runs one view against the points a session keeps in HBM.
"""
import ctypes as C

import numpy as np

from . import _lib


def default_options(ctx):
    o = _lib.PnpOptions()
    ctx.lib.rcn_pnp_default_options(C.byref(o))
    return o


def pnp_ransac(ctx, off, landmark, xy, points, intr6, options=None):
    """rcn_pnp_ransac: view v owns entries off[v] .. off[v + 1] of landmark / xy.  Returns dict(pose34[n_views, 12],
    ransac_pose34[n_views, 12], mask[total], count[n_views], iterations[n_views]); count -1: no model, -2: < 4 entries."""
    off = np.ascontiguousarray(off, np.int64)
    lm = np.ascontiguousarray(landmark, np.int32)
    xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
    X = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    nv = len(off) - 1
    K = np.ascontiguousarray(intr6, np.float64).reshape(nv, 6)
    n = len(lm)
    out = dict(pose34=np.zeros((nv, 12)), ransac_pose34=np.zeros((nv, 12)), mask=np.zeros(max(n, 1), np.uint8),
               count=np.zeros(max(nv, 1), np.int32), iterations=np.zeros(max(nv, 1), np.int32))
    ctx.check(ctx.lib.rcn_pnp_ransac(ctx.h, nv, off.ctypes.data, lm.ctypes.data if n else None, xy.ctypes.data if n else None,
                                     len(X), X.ctypes.data if len(X) else None, K.ctypes.data if nv else None,
                                     C.byref(options) if options is not None else None, out["pose34"].ctypes.data,
                                     out["ransac_pose34"].ctypes.data, out["mask"].ctypes.data, out["count"].ctypes.data,
                                     out["iterations"].ctypes.data))
    out["mask"], out["count"], out["iterations"] = out["mask"][:n], out["count"][:nv], out["iterations"][:nv]
    return out


def pnp_ransac_device(ctx, off, landmark, feat, view_img, n_points, points_ptr, intr6, options=None):
    """rcn_pnp_ransac_device on torch tensors in HBM: off (int64, n_views + 1), landmark / feat (int32, at least off[-1]
    entries), view_img (int32 image ids), intr6 (float64, n_views x 6); points_ptr: device address of n_points x 3 doubles
    (rcn_ba_session_points_device) or a float64 tensor.  Only enqueues: returns device tensors dict(pose34, ransac_pose34,
    mask, count, iterations) that are valid after rcn_synchronize."""
    import torch
    dev = off.device
    nv = off.numel() - 1
    if isinstance(points_ptr, torch.Tensor):
        points_ptr = points_ptr.data_ptr()
    out = dict(pose34=torch.zeros((nv, 12), dtype=torch.float64, device=dev), ransac_pose34=torch.zeros((nv, 12), dtype=torch.float64, device=dev),
               mask=torch.zeros(max(landmark.numel(), 1), dtype=torch.uint8, device=dev),
               count=torch.zeros(max(nv, 1), dtype=torch.int32, device=dev), iterations=torch.zeros(max(nv, 1), dtype=torch.int32, device=dev))
    ctx.check(ctx.lib.rcn_pnp_ransac_device(ctx.h, nv, off.data_ptr(), landmark.data_ptr(), feat.data_ptr(), view_img.data_ptr(),
                                            int(n_points), points_ptr, intr6.data_ptr(),
                                            C.byref(options) if options is not None else None, out["pose34"].data_ptr(),
                                            out["ransac_pose34"].data_ptr(), out["mask"].data_ptr(), out["count"].data_ptr(),
                                            out["iterations"].data_ptr()))
    return out


def smoke(ctx, seed=3, n=300, wrong_share=0.3):
    """One seeded view of n entries with a share of wrong landmarks: the planted pose is recovered (used by
    __graft_entry__.smoke).  Returns (count, planted, iterations, rotation error in rad, relative centre error)."""
    from . import synth_ba
    sc = synth_ba.make_scene(6, 600, obs_per_point=6, seed=seed)
    rng = np.random.default_rng(seed)
    o = np.flatnonzero(sc["obs_cam"] == 2)[:n]
    assert len(o) == n
    lm = sc["obs_pt"][o].astype(np.int32)
    xy = np.trunc(sc["obs_uv"][o]).astype(np.int32)
    bad = rng.random(n) < wrong_share
    lm[bad] = rng.integers(0, 600, int(bad.sum()))
    X, K = sc["points_gt"].astype(np.float64), sc["intr_gt"][2].astype(np.float64)
    G = synth_ba.poses_to_34(sc["poses_gt"][2:3]).reshape(3, 4)

    def within(P):
        l = X[lm] @ P[:, :3].T + P[:, 3]
        x, y = l[:, 0] / l[:, 2], l[:, 1] / l[:, 2]
        r = x * x + y * y
        d = K[4] * r + K[5] * r * r
        return ((K[0] * (x + d) + K[2] - xy[:, 0]) ** 2 + (K[1] * (y + d) + K[3] - xy[:, 1]) ** 2).astype(np.float32) <= np.float32(16.0)

    r = pnp_ransac(ctx, [0, n], lm, xy, X, K)
    planted = int(within(G).sum())
    count = int(r["count"][0])
    assert count == int(r["mask"].sum()) and count >= 0.9 * planted, "PnP: %d inliers of %d planted" % (count, planted)
    P = r["pose34"].reshape(3, 4)
    assert int(within(P).sum()) >= 0.99 * planted, "PnP: the refit loses planted entries"
    rot = float(np.arccos(np.clip((np.trace(P[:, :3] @ G[:, :3].T) - 1) / 2, -1, 1)))
    c, cg = -P[:, :3].T @ P[:, 3], -G[:, :3].T @ G[:, 3]
    cen = float(np.linalg.norm(c - cg) / np.linalg.norm(X[lm[~bad]].mean(0) - cg))
    assert rot <= 5e-3 and cen <= 5e-3, "PnP: planted pose not recovered (rotation %.2e rad, centre %.2e)" % (rot, cen)
    return count, planted, int(r["iterations"][0]), rot, cen
