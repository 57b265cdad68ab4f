"""Host mirror of FeatureClassic::detect (FeatureDetector.cpp:13-35 = cv::SIFT::create()->detectAndCompute) over librcn.so
(no CPU fallback).

    layout               rcn_sift_layout: the shape of the packed Gaussian pyramid (pure host code)
    pyramid              images -> packed fp32 pyramids [n][floats per image]
    candidates           pyramids -> the scale-space extrema alone (for inspection)
    detect               pyramids -> keypoints (extrema, refinement, orientation, duplicates, canonical order, cap)
    describe             pyramids + keypoints -> 128 integer-valued floats per keypoint
    detect_and_compute   the three in one call, the pyramid in the ctx's workspace; rows straight into a caller's buffer

Images are grey, uint8 or float32 on the 0..255 scale, torch tensors [n][H][W] on the GPU with any strides.
"""
import ctypes as C

from . import _lib

INPUT_F32, INPUT_U8 = 0, 1


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def options(n_octave_layers=None, contrast_threshold=None, edge_threshold=None, sigma=None):
    o = _lib.SiftOptions()
    _lib.load().rcn_sift_default_options(C.byref(o))
    if n_octave_layers is not None:
        o.n_octave_layers = int(n_octave_layers)
    if contrast_threshold is not None:
        o.contrast_threshold = float(contrast_threshold)
    if edge_threshold is not None:
        o.edge_threshold = float(edge_threshold)
    if sigma is not None:
        o.sigma = float(sigma)
    return o


def layout(H, W, opt=None):
    """rcn_sift_layout as a dict (needs no device)."""
    L = _lib.SiftLayout()
    rc = _lib.load().rcn_sift_layout(int(H), int(W), C.byref(opt) if opt is not None else None, C.byref(L))
    if rc != _lib.RCN_OK:
        raise _lib.RcnError(rc, "rcn_sift_layout(H=%d, W=%d)" % (H, W))
    no, nl = L.n_octaves, L.n_layers
    return dict(n_octaves=no, n_layers=nl, base_sigma=L.base_sigma, base_taps=L.base_taps, oct_h=list(L.oct_h[:no]), oct_w=list(L.oct_w[:no]),
                layer_sigma=list(L.layer_sigma[:nl]), layer_taps=list(L.layer_taps[:nl]),
                layer_offset=[list(L.layer_offset[o][:nl]) for o in range(no)], floats_per_image=L.floats_per_image)


def set_chunk_images(ctx, images):
    ctx.check(ctx.lib.rcn_sift_set_chunk_images(ctx.h, int(images)))


def _images(images):
    import torch
    if not images.is_cuda or images.dim() != 3 or images.dtype not in (torch.uint8, torch.float32):
        raise ValueError("sift: images must be a uint8 or float32 CUDA tensor of shape [n][H][W]")
    return INPUT_U8 if images.dtype == torch.uint8 else INPUT_F32


def _opt(opt):
    return C.byref(opt) if opt is not None else None


def _outputs(n, K, device):
    import torch
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=device)      # noqa: E731
    i = lambda *s: torch.empty(s, dtype=torch.int32, device=device)        # noqa: E731
    return dict(xy=f(n, K, 2), xy_int=i(n, K, 2), size=f(n, K), angle=f(n, K), response=f(n, K), octave=i(n, K), counts=i(n))


def _kp_ptrs(out):
    return [_ptr(out[k]) for k in ("xy", "xy_int", "size", "angle", "response", "octave", "counts")]


def pyramid(ctx, images, opt=None):
    """rcn_sift_pyramid_device: float32 CUDA tensor [n][floats per image]."""
    import torch
    dt = _images(images)
    n, H, W = images.shape
    fpi = layout(H, W, opt)["floats_per_image"]
    pyr = torch.empty((n, fpi), dtype=torch.float32, device=images.device)
    torch.cuda.synchronize()
    si, sy, sx = images.stride()
    ctx.check(ctx.lib.rcn_sift_pyramid_device(ctx.h, _ptr(images), dt, si, sy, sx, n, H, W, _opt(opt), _ptr(pyr)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return pyr


def candidates(ctx, pyr, H, W, capacity, opt=None):
    """rcn_sift_candidates_device: (records int64 [n][capacity] as CUDA tensor, counts[n]); a record is
    (octave << 56) | (layer << 52) | (row << 26) | column."""
    import torch
    n = pyr.shape[0]
    rec = torch.zeros((n, capacity), dtype=torch.int64, device=pyr.device)
    counts = torch.empty((n,), dtype=torch.int32, device=pyr.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_sift_candidates_device(ctx.h, _ptr(pyr), n, H, W, _opt(opt), int(capacity), _ptr(rec), _ptr(counts)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return rec, counts


def detect(ctx, pyr, H, W, K, opt=None):
    """rcn_sift_detect_device on packed pyramids [n][floats per image].  Returns a dict of CUDA tensors: xy[n][K][2] float32,
    xy_int (the truncation: Feature<int>::featCoord), size, angle, response, octave [n][K], counts[n] (uncapped).  Rows past
    min(counts[i], K) are (-1, -1) / 0."""
    import torch
    if pyr.dtype != torch.float32 or not pyr.is_cuda or pyr.dim() != 2 or not pyr.is_contiguous():
        raise ValueError("sift.detect: pyr must be a contiguous float32 CUDA tensor [n][floats per image]")
    n = pyr.shape[0]
    if n and pyr.shape[1] != layout(H, W, opt)["floats_per_image"]:
        raise ValueError("sift.detect: pyr does not have the layout of H x W images")
    out = _outputs(n, max(int(K), 1), pyr.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_sift_detect_device(ctx.h, _ptr(pyr), n, H, W, _opt(opt), int(K), *_kp_ptrs(out)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return out


def describe(ctx, pyr, H, W, kp, opt=None, out=None):
    """rcn_sift_describe_device for the keypoints `detect` returned.  out: device address of an [n][K][128] float32 block (the
    slot of pairgrid.Shard.reserve) or None for a new tensor, which is returned."""
    import torch
    n, K = kp["size"].shape
    rows = None
    if out is None:
        rows = torch.empty((n, K, 128), dtype=torch.float32, device=pyr.device)
        out = rows.data_ptr()
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_sift_describe_device(ctx.h, _ptr(pyr), n, H, W, _opt(opt), K, _ptr(kp["xy"]), _ptr(kp["size"]), _ptr(kp["angle"]),
                                               _ptr(kp["octave"]), _ptr(kp["counts"]), C.c_void_p(out)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return rows


def detect_and_compute(ctx, images, K, opt=None, out=None):
    """rcn_sift_detect_and_compute_device.  Returns the dict of `detect` plus rows [n][K][128] (None when `out`, a device address,
    received them)."""
    import torch
    dt = _images(images)
    n, H, W = images.shape
    kp = _outputs(n, max(int(K), 1), images.device)
    rows = None
    if out is None:
        rows = torch.empty((n, max(int(K), 1), 128), dtype=torch.float32, device=images.device)
        out = rows.data_ptr()
    torch.cuda.synchronize()
    si, sy, sx = images.stride()
    ctx.check(ctx.lib.rcn_sift_detect_and_compute_device(ctx.h, _ptr(images), dt, si, sy, sx, n, H, W, _opt(opt), int(K), *_kp_ptrs(kp),
                                                         C.c_void_p(out)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    kp["rows"] = rows
    return kp


def smoke(ctx):
    """Two synthetic 64 x 96 images through detect_and_compute; checks the structure of the result on the host (canonical order, no
    duplicates, truncated coordinates, padding, integer rows of SIFT's norm).  Returns the keypoints per image."""
    import numpy as np
    import torch
    from .synth import blob_image
    H, W, K = 64, 96, 256
    rng = np.random.default_rng(5)
    ims = []
    for s in range(2):
        blobs = [(rng.uniform(10, W - 10), rng.uniform(10, H - 10), rng.uniform(1.5, 4), rng.uniform(1.5, 4), rng.uniform(0, 3.1), rng.uniform(40, 110) * rng.choice([-1, 1]))
                 for _ in range(14)]
        ims.append(np.rint(blob_image(H, W, blobs, texture=3.0, seed=s)).astype(np.uint8))
    r = detect_and_compute(ctx, torch.from_numpy(np.stack(ims)).cuda(), K)
    g = {k: v.cpu().numpy() for k, v in r.items()}
    for i in range(2):
        m = int(g["counts"][i])
        assert 0 < m <= K, "SIFT: no keypoints on the smoke image"
        keys = list(zip(g["xy"][i, :m, 0], g["xy"][i, :m, 1], g["size"][i, :m], g["angle"][i, :m], g["response"][i, :m], g["octave"][i, :m]))
        assert keys == sorted(keys) and len(set(keys)) == m, "SIFT: keypoints out of canonical order"
        assert np.array_equal(g["xy_int"][i, :m], np.trunc(g["xy"][i, :m]).astype(np.int32))
        assert (g["xy"][i, m:] == -1).all() and (g["size"][i, m:] == 0).all() and (g["rows"][i, m:] == 0).all()
        rows = g["rows"][i, :m]
        assert np.array_equal(rows, np.rint(rows)) and rows.min() >= 0 and rows.max() <= 255
        assert (np.abs(np.linalg.norm(rows.astype(np.float64), axis=1) - 512.0) < 12.0).all(), "SIFT: descriptor rows off the norm of 512"
    return g["counts"].tolist()
