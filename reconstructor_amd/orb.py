"""Host mirror of FeatureClassic's second detector (the cv::ORB::create() of FeatureDetector.cpp:9, :19) over librcn.so
(no CPU fallback).

    layout               rcn_orb_layout: level sizes, offsets, bytes per image and quotas (pure host code)
    default_pattern      the built-in 256 tests, int8 [1024]
    pyramid              images -> packed byte pyramids [n][bytes per image]
    fast                 pyramids -> the FAST-9/16 score map of every level, in the pyramid's layout (for inspection)
    detect               pyramids -> keypoints (FAST, 3 x 3 maximum, the two cuts per level, canonical order, cap)
    describe             pyramids + keypoints -> 32 floats in 0..255 per keypoint, and the same bytes packed
    detect_and_compute   the three in one call, the pyramid in the ctx's workspace; rows straight into a caller's buffer

Images are grey, uint8 or float32 on the 0..255 scale, torch tensors [n][H][W] on the GPU with any strides.
"""
import ctypes as C

from . import _lib

INPUT_F32, INPUT_U8 = 0, 1


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def options(nfeatures=None, scale_factor=None, nlevels=None, edge_threshold=None, fast_threshold=None, pattern=None):
    """rcn_orb_options with cv::ORB::create()'s defaults.  pattern: 1024 signed bytes (numpy int8), kept alive by the result."""
    o = _lib.OrbOptions()
    _lib.load().rcn_orb_default_options(C.byref(o))
    for name, v in (("nfeatures", nfeatures), ("nlevels", nlevels), ("edge_threshold", edge_threshold), ("fast_threshold", fast_threshold)):
        if v is not None:
            setattr(o, name, int(v))
    if scale_factor is not None:
        o.scale_factor = float(scale_factor)
    if pattern is not None:
        import numpy as np
        p = np.ascontiguousarray(pattern)
        if p.dtype != np.int8 or p.size != 1024:
            raise ValueError("orb.options: a pattern is 1024 signed bytes")
        o._pattern = p
        o.pattern = p.ctypes.data
    return o


def _opt(opt):
    return C.byref(opt) if opt is not None else None


def layout(H, W, opt=None):
    """rcn_orb_layout as a dict (needs no device)."""
    L = _lib.OrbLayout()
    rc = _lib.load().rcn_orb_layout(int(H), int(W), _opt(opt), C.byref(L))
    if rc != _lib.RCN_OK:
        raise _lib.RcnError(rc, "rcn_orb_layout(H=%d, W=%d)" % (H, W))
    n = L.n_levels
    return dict(n_levels=n, level_h=list(L.level_h[:n]), level_w=list(L.level_w[:n]), quota=list(L.quota[:n]), active=list(L.active[:n]),
                scale=list(L.scale[:n]), level_offset=list(L.level_offset[:n]), bytes_per_image=L.bytes_per_image)


def default_pattern():
    import numpy as np
    return np.ctypeslib.as_array(_lib.load().rcn_orb_default_pattern(), shape=(1024,)).copy()


def set_chunk_images(ctx, images):
    ctx.check(ctx.lib.rcn_orb_set_chunk_images(ctx.h, int(images)))


def _images(images):
    import torch
    if not images.is_cuda or images.dim() != 3 or images.dtype not in (torch.uint8, torch.float32):
        raise ValueError("orb: images must be a uint8 or float32 CUDA tensor of shape [n][H][W]")
    return INPUT_U8 if images.dtype == torch.uint8 else INPUT_F32


def _pyr(pyr, H, W, opt):
    import torch
    if pyr.dtype != torch.uint8 or not pyr.is_cuda or pyr.dim() != 2 or not pyr.is_contiguous():
        raise ValueError("orb: pyr must be a contiguous uint8 CUDA tensor [n][bytes per image]")
    if pyr.shape[0] and pyr.shape[1] != layout(H, W, opt)["bytes_per_image"]:
        raise ValueError("orb: pyr does not have the layout of H x W images")
    return pyr.shape[0]


def _outputs(n, K, device):
    import torch
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=device)      # noqa: E731
    i = lambda *s: torch.empty(s, dtype=torch.int32, device=device)        # noqa: E731
    return dict(xy=f(n, K, 2), xy_int=i(n, K, 2), size=f(n, K), angle=f(n, K), response=f(n, K), octave=i(n, K), counts=i(n))


def _kp_ptrs(out):
    return [_ptr(out[k]) for k in ("xy", "xy_int", "size", "angle", "response", "octave", "counts")]


def pyramid(ctx, images, opt=None):
    """rcn_orb_pyramid_device: uint8 CUDA tensor [n][bytes per image]."""
    import torch
    dt = _images(images)
    n, H, W = images.shape
    pyr = torch.zeros((n, layout(H, W, opt)["bytes_per_image"]), dtype=torch.uint8, device=images.device)
    torch.cuda.synchronize()
    si, sy, sx = images.stride()
    ctx.check(ctx.lib.rcn_orb_pyramid_device(ctx.h, _ptr(images), dt, si, sy, sx, n, H, W, _opt(opt), _ptr(pyr)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return pyr


def fast(ctx, pyr, H, W, opt=None):
    """rcn_orb_fast_device: the score maps, uint8 CUDA tensor [n][bytes per image]."""
    import torch
    n = _pyr(pyr, H, W, opt)
    out = torch.empty_like(pyr)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_orb_fast_device(ctx.h, _ptr(pyr), n, H, W, _opt(opt), _ptr(out)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return out


def detect(ctx, pyr, H, W, K, opt=None):
    """rcn_orb_detect_device.  Returns a dict of CUDA tensors: xy[n][K][2] float32, xy_int (the truncation:
    Feature<int>::featCoord), size, angle, response, octave [n][K], counts[n] (uncapped; -1: overflow).  Rows past
    min(counts[i], K) are (-1, -1) / 0."""
    import torch
    n = _pyr(pyr, H, W, opt)
    out = _outputs(n, max(int(K), 1), pyr.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_orb_detect_device(ctx.h, _ptr(pyr), n, H, W, _opt(opt), int(K), *_kp_ptrs(out)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return out


def describe(ctx, pyr, H, W, kp, opt=None, out=None, packed=True):
    """rcn_orb_describe_device for the keypoints `detect` returned.  out: device address of an [n][K][32] float32 block (the
    slot of pairgrid.Shard.reserve) or None for a new tensor.  Returns (rows or None, packed bytes [n][K][32] or None)."""
    import torch
    n = _pyr(pyr, H, W, opt)
    K = kp["size"].shape[1]
    rows = None
    if out is None:
        rows = torch.empty((n, K, 32), dtype=torch.float32, device=pyr.device)
        out = rows.data_ptr()
    by = torch.empty((n, K, 32), dtype=torch.uint8, device=pyr.device) if packed else None
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_orb_describe_device(ctx.h, _ptr(pyr), n, H, W, _opt(opt), K, _ptr(kp["xy"]), _ptr(kp["octave"]), _ptr(kp["counts"]),
                                              C.c_void_p(out), _ptr(by)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return rows, by


def detect_and_compute(ctx, images, K, opt=None, out=None, packed=True):
    """rcn_orb_detect_and_compute_device.  Returns the dict of `detect` plus rows [n][K][32] (None when `out`, a device
    address, received them) and packed [n][K][32] uint8 (None unless asked for)."""
    import torch
    dt = _images(images)
    n, H, W = images.shape
    Kb = max(int(K), 1)
    kp = _outputs(n, Kb, images.device)
    rows = None
    if out is None:
        rows = torch.empty((n, Kb, 32), dtype=torch.float32, device=images.device)
        out = rows.data_ptr()
    by = torch.empty((n, Kb, 32), dtype=torch.uint8, device=images.device) if packed else None
    torch.cuda.synchronize()
    si, sy, sx = images.stride()
    ctx.check(ctx.lib.rcn_orb_detect_and_compute_device(ctx.h, _ptr(images), dt, si, sy, sx, n, H, W, _opt(opt), int(K), *_kp_ptrs(kp),
                                                        C.c_void_p(out), _ptr(by)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    kp["rows"] = rows
    kp["packed"] = by
    return kp


def smoke(ctx):
    """A synthetic 128 x 128 image of rectangles and its quarter turn through detect_and_compute; checks on the host: canonical
    order, truncated coordinates, padding, integer rows in 0..255 equal to the packed bytes, and that the level-0 keypoints of
    the turned image carry the rows of their originals (the direction turns with the patch: exact).  Returns the keypoints per
    image and the number of level-0 rows compared."""
    import numpy as np
    import torch
    H, W, K = 128, 128, 1024
    rng = np.random.default_rng(11)
    img = np.full((H, W), 120, np.int32)
    for _ in range(60):
        x, y, a, b = int(rng.integers(0, W - 8)), int(rng.integers(0, H - 8)), int(rng.integers(6, 40)), int(rng.integers(6, 40))
        img[y:y + b, x:x + a] = int(rng.integers(20, 236))
    img = (img + rng.integers(-4, 5, (H, W))).astype(np.uint8)       # without noise the corners of a rectangle tie and the strict maximum drops them
    ims = np.stack([img, np.rot90(img).copy()])
    r = detect_and_compute(ctx, torch.from_numpy(ims).cuda(), K)
    g = {k: v.cpu().numpy() for k, v in r.items()}
    lv0 = []
    for i in range(2):
        m = int(g["counts"][i])
        assert 0 < m <= K, "ORB: no keypoints on the smoke image"
        oc, xy = g["octave"][i, :m], g["xy"][i, :m]
        sc = np.array(layout(H, W)["scale"], np.float32)[oc]
        keys = list(zip(oc.tolist(), np.rint(xy[:, 1] / sc).tolist(), np.rint(xy[:, 0] / sc).tolist()))
        assert keys == sorted(keys) and len(set(keys)) == m, "ORB: keypoints out of canonical order"
        assert np.array_equal(g["xy_int"][i, :m], np.trunc(xy).astype(np.int32))
        assert (g["xy"][i, m:] == -1).all() and (g["size"][i, m:] == 0).all() and (g["rows"][i, m:] == 0).all()
        rows = g["rows"][i, :m]
        assert np.array_equal(rows, np.rint(rows)) and rows.min() >= 0 and rows.max() <= 255
        assert np.array_equal(rows.astype(np.uint8), g["packed"][i, :m]), "ORB: float rows differ from the packed bytes"
        lv0.append({(int(x), int(y)): rows[k] for k, (o, y, x) in enumerate(keys) if o == 0})
    # np.rot90 turns counter-clockwise: pixel (x, y) of the image is pixel (y, W - 1 - x) of the turned one
    same = 0
    for (x, y), row in lv0[0].items():
        t = lv0[1].get((y, W - 1 - x))
        assert t is not None and np.array_equal(t, row), "ORB: a quarter turn changed a level-0 row"
        same += 1
    assert same == len(lv0[1]) and same > 0
    return g["counts"].tolist(), same
