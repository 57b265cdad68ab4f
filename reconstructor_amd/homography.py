"""Host mirror of the batched homography RANSAC over librcn.so (no CPU fallback).

cv::findHomography(src, dst, RANSAC, 3.0, mask, 2000, 0.995) on integer pixels for a batch of pairs per call (DESIGN.md
section 27): `find` takes host arrays, `find_device` pair ids against the resident lists and coordinates.  The two-view
classification built on it is twoview.geometry.
"""
import ctypes as C

import numpy as np

from . import _lib


def default_options(ctx):
    o = _lib.HomographyOptions()
    ctx.lib.rcn_homography_default_options(C.byref(o))
    return o


def find(ctx, off, xy1, xy2, options=None):
    """rcn_homography_ransac: pair p owns entries off[p] .. off[p + 1] of xy1 (src) / xy2 (dst).  Returns dict(H[n_pairs, 9],
    mask[total], count[n_pairs], iterations[n_pairs]); count -1: no model, -2: < 4 entries."""
    off = np.ascontiguousarray(off, np.int64)
    xy1 = np.ascontiguousarray(xy1, np.int32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.int32).reshape(-1, 2)
    npairs = len(off) - 1
    n = len(xy1)
    if len(xy2) != n:
        raise ValueError("homography.find: xy1 and xy2 differ in length")
    out = dict(H=np.zeros((npairs, 9)), mask=np.zeros(max(n, 1), np.uint8), count=np.zeros(max(npairs, 1), np.int32),
               iterations=np.zeros(max(npairs, 1), np.int32))
    ctx.check(ctx.lib.rcn_homography_ransac(ctx.h, npairs, off.ctypes.data, xy1.ctypes.data if n else None, xy2.ctypes.data if n else None,
                                            C.byref(options) if options is not None else None, out["H"].ctypes.data,
                                            out["mask"].ctypes.data, out["count"].ctypes.data, out["iterations"].ctypes.data))
    out["mask"], out["count"], out["iterations"] = out["mask"][:n], out["count"][:npairs], out["iterations"][:npairs]
    return out


def find_device(ctx, pairs, capacity, options=None, device=None, want_qt=True):
    """rcn_homography_ransac_device: pairs n x (a, b) image ids (host); the entries come from the resident lists
    (nextview.upload_feature_matches) and coordinates.  Only enqueues: returns device tensors dict(off, qt, H, mask, count,
    iterations) that are valid after rcn_synchronize."""
    import torch
    dev = device if device is not None else torch.device("cuda", 0)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n, cap = len(pairs), int(capacity)
    out = dict(off=torch.zeros(n + 1, dtype=torch.int64, device=dev), qt=torch.zeros((max(cap, 1), 2), dtype=torch.int32, device=dev),
               H=torch.zeros((max(n, 1), 9), dtype=torch.float64, device=dev), mask=torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev),
               count=torch.zeros(max(n, 1), dtype=torch.int32, device=dev), iterations=torch.zeros(max(n, 1), dtype=torch.int32, device=dev))
    ctx.check(ctx.lib.rcn_homography_ransac_device(ctx.h, n, pairs.ctypes.data if n else None, C.byref(options) if options is not None else None,
                                                   cap, out["off"].data_ptr(), out["qt"].data_ptr() if want_qt else None, out["H"].data_ptr(),
                                                   out["mask"].data_ptr(), out["count"].data_ptr(), out["iterations"].data_ptr()))
    return out
