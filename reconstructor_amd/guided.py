"""Host mirror of guided matching: the exact 2-NN of every query row inside the epipolar band of its pair, over librcn.so (no CPU
fallback).

    options               rcn_guided_default_options with overrides
    match_guided          rcn_match_guided: table, counts and in-band combinations of a pair list, F per pair from the host
    match_guided_device   rcn_match_guided_device: the same on CUDA tensors (asynchronous on the ctx stream)
    match_pair            rcn_match_pair_guided: one pair straight from host rows and coordinates
    knn2                  rcn_guided_knn2_device: (j0, j1, candidates, 0) and the two squared distances per query row
    filter_model_device   rcn_match_table_filter_model_device: the epipolar filter of a device table, keeping every pair's F
    grid_guided           rcn_match_grid_guided: match, filter keeping the model, guided re-match of the pairs that have one

The images' fp32 rows (rcn_desc_*) and integer coordinates (rcn_coords_upload*) must be resident; matcher.HipL2Matcher uploads both.
Nothing here computes a distance or a band for a caller; smoke() restates one planted answer to check the run it made.
"""
import ctypes as C

import numpy as np

from . import _lib


def options(**kw):
    o = _lib.GuidedOptions()
    lib = _lib.load()
    lib.rcn_guided_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("guided: no option " + k)
        setattr(o, k, v)
    return o


def _pairs(pairs):
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    return pairs, len(pairs)


def _F(F, P):
    F = np.ascontiguousarray(F, np.float64).reshape(-1, 9)
    if len(F) != P:
        raise ValueError("guided: one F (9 doubles) per pair")
    return F


def match_guided(ctx, pairs, F, out_stride, opt=None):
    """Returns (out [P][out_stride], counts [P], cand [P]) on the host."""
    pairs, P = _pairs(pairs)
    F = _F(F, P)
    opt = opt or options()
    out = np.full((max(P, 1), max(1, int(out_stride))), -1, np.int32)
    counts = np.zeros(max(P, 1), np.int32)
    cand = np.zeros(max(P, 1), np.int64)
    ctx.check(ctx.lib.rcn_match_guided(ctx.h, pairs.ctypes.data if P else None, P, F.ctypes.data if P else None, C.byref(opt),
                                       out.ctypes.data, out.shape[1], counts.ctypes.data, cand.ctypes.data))
    return out[:P], counts[:P], cand[:P]


def match_guided_device(ctx, pairs, F_dev, out_stride, opt=None, out=None, counts=None, want_cand=True):
    """F_dev: float64 CUDA tensor [P][9].  Returns CUDA tensors (out, counts, cand or None); asynchronous on the ctx stream."""
    import torch
    pairs, P = _pairs(pairs)
    opt = opt or options()
    dev = torch.device("cuda", ctx.device)
    if F_dev.dtype != torch.float64 or not F_dev.is_cuda or not F_dev.is_contiguous() or F_dev.numel() != 9 * P:
        raise ValueError("guided: F_dev must be a contiguous float64 CUDA tensor [P][9]")
    if out is None:
        out = torch.empty((max(P, 1), max(1, int(out_stride))), dtype=torch.int32, device=dev)
    if counts is None:
        counts = torch.empty((max(P, 1),), dtype=torch.int32, device=dev)
    cand = torch.empty((max(P, 1),), dtype=torch.int64, device=dev) if want_cand else None
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_match_guided_device(ctx.h, pairs.ctypes.data if P else None, P, C.c_void_p(F_dev.data_ptr()), C.byref(opt),
                                              C.c_void_p(out.data_ptr()), out.shape[1], C.c_void_p(counts.data_ptr()),
                                              C.c_void_p(cand.data_ptr()) if want_cand else None))
    return out[:P], counts[:P], cand[:P] if want_cand else None


def match_pair(ctx, q, xy1, t, xy2, F, opt=None):
    """Dense result: out[i] = train row matched to query row i, or -1."""
    q, t = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)
    if q.ndim != 2 or t.ndim != 2 or q.shape[1] != t.shape[1]:
        raise ValueError("guided: rows are float32 [K][D] with one D")
    xy1, xy2 = np.ascontiguousarray(xy1, np.int32).reshape(-1, 2), np.ascontiguousarray(xy2, np.int32).reshape(-1, 2)
    if len(xy1) != len(q) or len(xy2) != len(t):
        raise ValueError("guided: one coordinate pair per row")
    F = _F(F, 1)
    opt = opt or options()
    K1, K2 = len(q), len(t)
    out = np.full(K1, -1, np.int32)
    cnt = C.c_int32(0)
    ctx.check(ctx.lib.rcn_match_pair_guided(ctx.h, q.ctypes.data if K1 else None, K1, xy1.ctypes.data if K1 else None,
                                            t.ctypes.data if K2 else None, K2, xy2.ctypes.data if K2 else None, q.shape[1],
                                            F.ctypes.data, C.byref(opt), out.ctypes.data if K1 else None, C.byref(cnt)))
    assert cnt.value == int((out >= 0).sum())
    return out


def knn2(ctx, pairs, F, stride, max_error_px=3.0):
    """Returns (idx int32 [P][stride][4], d2 float64 [P][stride][2]) on the host."""
    import torch
    pairs, P = _pairs(pairs)
    F = _F(F, P)
    dev = torch.device("cuda", ctx.device)
    F_dev = torch.from_numpy(F).to(dev) if P else torch.zeros((1, 9), dtype=torch.float64, device=dev)
    idx = torch.empty((max(P, 1), max(1, int(stride)), 4), dtype=torch.int32, device=dev)
    d2 = torch.empty((max(P, 1), max(1, int(stride)), 2), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_guided_knn2_device(ctx.h, pairs.ctypes.data if P else None, P, C.c_void_p(F_dev.data_ptr()), float(np.float32(max_error_px)),
                                             C.c_void_p(idx.data_ptr()), C.c_void_p(d2.data_ptr()), idx.shape[1]))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return idx[:P].cpu().numpy(), d2[:P].cpu().numpy()


def filter_model_device(ctx, pairs, table, counts, status=None, F=None):
    """The epipolar filter of a device match table in place (CUDA tensors as rcn_match_grid_device left them), keeping the models.
    Returns (status, F) as CUDA tensors; asynchronous on the ctx stream."""
    import torch
    pairs, P = _pairs(pairs)
    dev = torch.device("cuda", ctx.device)
    if status is None:
        status = torch.empty((max(P, 1),), dtype=torch.int32, device=dev)
    if F is None:
        F = torch.empty((max(P, 1), 9), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_match_table_filter_model_device(ctx.h, pairs.ctypes.data if P else None, P, C.c_void_p(table.data_ptr()), table.shape[1],
                                                          C.c_void_p(counts.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(F.data_ptr())))
    return status[:P], F[:P]


def grid_guided(ctx, pairs, out_stride, ratio=0.7, opt=None):
    """Returns (out [P][out_stride], counts [P], status [P]) on the host."""
    pairs, P = _pairs(pairs)
    opt = opt or options()
    out = np.full((max(P, 1), max(1, int(out_stride))), -1, np.int32)
    counts = np.zeros(max(P, 1), np.int32)
    status = np.zeros(max(P, 1), np.int32)
    ctx.check(ctx.lib.rcn_match_grid_guided(ctx.h, pairs.ctypes.data if P else None, P, float(np.float32(ratio)), C.byref(opt),
                                            out.ctypes.data, out.shape[1], counts.ctypes.data, status.ctypes.data))
    return out[:P], counts[:P], status[:P]


def smoke(ctx):
    """A rectified pair with a repeated structure: every query row has an exact copy in its own image row (in band) and a second copy
    two image rows away (out of band).  Unguided, the two copies tie and the ratio test refuses every row; guided, every row is matched
    to the copy in its band.  Returns (rows, matches)."""
    rng = np.random.default_rng(8)
    K, D = 96, 64
    q = rng.standard_normal((K, D)).astype(np.float32)
    t = np.concatenate([q, q])
    xy1 = np.c_[rng.integers(0, 500, K), 10 * np.arange(K)].astype(np.int32)
    xy2 = np.concatenate([np.c_[rng.integers(0, 500, K), 10 * np.arange(K) + 20], np.c_[rng.integers(0, 500, K), 10 * np.arange(K) + 1]]).astype(np.int32)
    F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float64)
    out = match_pair(ctx, q, xy1, t, xy2, F)
    assert np.array_equal(out, K + np.arange(K)), "guided matcher: the in-band copy of every row was not matched"
    wide = match_pair(ctx, q, xy1, t, xy2, F, options(max_error_px=1e4))
    assert (wide == -1).all(), "guided matcher: with both copies in band the ratio test must refuse every row"
    return K, int((out >= 0).sum())
