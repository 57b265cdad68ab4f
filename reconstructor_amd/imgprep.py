"""Host mirror of what detectFeatures does to a decoded photograph before a detector sees it, and of what becomes of the colours
(SequentialReconstructor.cpp:55-110, :429-433; Utils::readImg / reshapeImg / saveCloud) over librcn.so (no CPU fallback;
DESIGN.md section 26).

    reshape_size      Utils::reshapeImg's target size and factor (pure host code)
    resize_tables     one axis of cv::resize's INTER_LINEAR tables (pure host code)
    plan              the tile rcn_img_prepare_device works in for a horizontal resize (pure host code)
    prepare           decoded images [n][H][W][3] or [n][H][W] uint8 -> (rgb, gray, factor): swap, resize, grey in one kernel
    feat_colors       the colour under every keypoint
    landmark_colors   a landmark's colour = its first feature's
    cloud_vertices    Utils::saveCloud's vertices as 16-byte records
    write_ply         those records as a PLY file (host code)
    save_cloud        a BA session (or arrays) -> coloured .ply

Images are torch uint8 tensors on the GPU; the last dimension (pixels, interleaved channels) must be dense, rows and images may
be any distance apart.  gray feeds sift.detect_and_compute and superpoint_net unchanged.
"""
import ctypes as C

import numpy as np

from . import _lib

ORDERS = {"rgb": 0, "bgr": 1}
VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def options(order=None, gray_bits=None):
    o = _lib.ImgOptions()
    _lib.load().rcn_img_default_options(C.byref(o))
    if order is not None:
        if order not in ORDERS:
            raise ValueError("imgprep: order must be 'rgb' or 'bgr'")
        o.order = ORDERS[order]
    if gray_bits is not None:
        o.gray_bits = int(gray_bits)
    return o


def reshape_size(rows, cols, max_size=512):
    """rcn_img_reshape_size: (rows', cols', factor)."""
    r, c, f = C.c_int32(), C.c_int32(), C.c_double()
    rc = _lib.load().rcn_img_reshape_size(int(rows), int(cols), int(max_size), C.byref(r), C.byref(c), C.byref(f))
    if rc != _lib.RCN_OK:
        raise _lib.RcnError(rc, "rcn_img_reshape_size(rows=%d, cols=%d, max_size=%d)" % (rows, cols, max_size))
    return r.value, c.value, f.value


def resize_tables(src, dst, horizontal=True):
    """rcn_img_resize_tables: (index int32 [dst], weights int16 [dst][2], xmax)."""
    idx, w, xmax = np.zeros(max(int(dst), 0), np.int32), np.zeros((max(int(dst), 0), 2), np.int16), C.c_int32()
    rc = _lib.load().rcn_img_resize_tables(int(src), int(dst), int(bool(horizontal)), idx.ctypes.data, w.ctypes.data, C.byref(xmax))
    if rc != _lib.RCN_OK:
        raise _lib.RcnError(rc, "rcn_img_resize_tables(src=%d, dst=%d)" % (src, dst))
    return idx, w, xmax.value


def plan(src_cols, cols, channels=3):
    """rcn_img_prepare_plan: dict(tile_cols, tile_rows, lds_bytes); tile_rows == 0: the one-row tile that stages nothing."""
    tc, tr, lds = C.c_int32(), C.c_int32(), C.c_int32()
    rc = _lib.load().rcn_img_prepare_plan(int(src_cols), int(cols), int(channels), C.byref(tc), C.byref(tr), C.byref(lds))
    if rc != _lib.RCN_OK:
        raise _lib.RcnError(rc, "rcn_img_prepare_plan(src_cols=%d, cols=%d, channels=%d)" % (src_cols, cols, channels))
    return dict(tile_cols=tc.value, tile_rows=tr.value, lds_bytes=lds.value)


def _source(images):
    import torch
    if not images.is_cuda or images.dtype != torch.uint8 or images.dim() not in (3, 4):
        raise ValueError("imgprep: images must be a uint8 CUDA tensor [n][H][W][3] or [n][H][W]")
    ch = images.shape[3] if images.dim() == 4 else 1
    st = images.stride()
    if (images.dim() == 4 and (st[3] != 1 or st[2] != ch)) or (images.dim() == 3 and st[2] != 1):
        raise ValueError("imgprep: the pixels of a row must be dense and interleaved")
    return ch, st[0], st[1]


def prepare_to(ctx, images, rows, cols, order="bgr", gray_bits=14, want_rgb=True, want_gray=True):
    """rcn_img_prepare_device to an explicit size: (rgb [n][rows][cols][3] or None, gray [n][rows][cols] or None)."""
    import torch
    ch, si, sr = _source(images)
    n, H, W = images.shape[:3]
    rgb = torch.empty((n, rows, cols, 3), dtype=torch.uint8, device=images.device) if want_rgb and ch == 3 else None
    gray = torch.empty((n, rows, cols), dtype=torch.uint8, device=images.device) if want_gray else None
    opt = options(order, gray_bits)
    if n == 0:
        return rgb, gray
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_img_prepare_device(ctx.h, _ptr(images), si, sr, ch, n, H, W, int(rows), int(cols), C.byref(opt), _ptr(rgb), _ptr(gray)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return rgb, gray


def prepare(ctx, images, max_size=512, order="bgr", gray_bits=14):
    """detectFeatures' chain for n decoded images of one size: (rgb, gray, factor) at reshape_size(H, W, max_size).  A
    single-channel batch [n][H][W] gives (None, the resized planes, factor)."""
    rows, cols, factor = reshape_size(images.shape[1], images.shape[2], max_size)
    rgb, gray = prepare_to(ctx, images, rows, cols, order, gray_bits)
    return rgb, gray, factor


def feat_colors(ctx, rgb, xy_int, counts):
    """rcn_feat_colors_device: uint8 [n][K][4] = (r, g, b, 0) of rgb[i][y][x] at xy_int[i][k] = (x, y)."""
    import torch
    n, rows, cols = rgb.shape[:3]
    K = xy_int.shape[1]
    rgb, xy_int, counts = rgb.contiguous(), xy_int.contiguous(), counts.contiguous()
    out = torch.empty((n, K, 4), dtype=torch.uint8, device=rgb.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_feat_colors_device(ctx.h, _ptr(rgb), n, rows, cols, _ptr(xy_int), _ptr(counts), K, _ptr(out)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return out


def landmark_colors(ctx, feat_rgba, first_img, first_feat):
    """rcn_landmark_colors_device: uint8 [L][4], the colour of every landmark's first feature."""
    import torch
    n, K = feat_rgba.shape[:2]
    dev = feat_rgba.device
    fi = torch.as_tensor(np.ascontiguousarray(first_img, np.int32)).to(dev)
    ff = torch.as_tensor(np.ascontiguousarray(first_feat, np.int32)).to(dev)
    L = fi.numel()
    out = torch.empty((L, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_landmark_colors_device(ctx.h, _ptr(feat_rgba.contiguous()), n, K, L, _ptr(fi), _ptr(ff), _ptr(out)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return out


def _cloud(ctx, xyz_ptr, L, lm_rgba, inliers, poses34, device):
    import torch
    P = torch.as_tensor(np.ascontiguousarray(poses34, np.float64).reshape(-1, 12)).to(device)
    Cn = P.shape[0]
    if lm_rgba is None:
        col = torch.zeros((L, 4), dtype=torch.uint8, device=device)
    else:
        col = torch.as_tensor(lm_rgba).to(device).contiguous()
        if col.dtype != torch.uint8 or tuple(col.shape) != (L, 4):
            raise ValueError("imgprep: landmark colours must be uint8 [L][4]")
    inl = None if inliers is None else torch.as_tensor(np.ascontiguousarray(inliers).astype(np.uint8)).to(device)
    if inl is not None and inl.numel() != L:
        raise ValueError("imgprep: one inlier flag per landmark")
    total = (2 if inl is not None else 1) * L + Cn
    out = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=device)
    nv = C.c_int64()
    one = torch.zeros(1, dtype=torch.uint8, device=device)          # a flag array of length 0 still means "with flags"
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_cloud_vertices_device(ctx.h, xyz_ptr, _ptr(col), None if inl is None else C.c_void_p((inl if L else one).data_ptr()), L,
                                                _ptr(P), Cn, C.c_void_p(out.data_ptr()), C.byref(nv)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    assert nv.value == total
    return out[:total].cpu().numpy().reshape(-1).view(VERTEX_DTYPE)


def cloud_vertices(ctx, xyz, lm_rgba, inliers, poses34):
    """rcn_cloud_vertices_device on arrays: records of VERTEX_DTYPE on the host.  xyz [L][3] float64 (numpy or CUDA tensor),
    lm_rgba uint8 [L][4] or None (black), inliers [L] or None, poses34 [C][12] rows of [R | t] in the order they are written."""
    import torch
    x = xyz if isinstance(xyz, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(xyz, np.float64).reshape(-1, 3))
    x = x.cuda().contiguous()
    if x.dtype != torch.float64:
        raise ValueError("imgprep: xyz must be float64")
    return _cloud(ctx, _ptr(x), x.shape[0], lm_rgba, inliers, poses34, x.device)


def write_ply(path, vertices, binary=False):
    """rcn_cloud_write_ply (host code)."""
    v = np.ascontiguousarray(vertices, VERTEX_DTYPE)
    rc = _lib.load().rcn_cloud_write_ply(str(path).encode(), v.ctypes.data if len(v) else None, len(v), int(bool(binary)))
    if rc != _lib.RCN_OK:
        raise _lib.RcnError(rc, "rcn_cloud_write_ply(%s)" % path)


def save_cloud(source, path, inliers=None, binary=False, lm_rgba=None, poses34=None):
    """Utils::saveCloud.  source: a ba.BaSession (its points are read where they live, in HBM; poses34 defaults to the session's
    cameras as the pipeline holds them) or a tuple (ctx, xyz, poses34).  Returns the records written."""
    import torch
    if isinstance(source, tuple):
        ctx, xyz, poses34 = source
        v = cloud_vertices(ctx, xyz, lm_rgba, inliers, poses34)
    else:
        from .ba import poses34_from_angle_axis
        ctx = source.ctx
        L = source.counts()[1]
        if poses34 is None:
            poses34 = poses34_from_angle_axis(source.cameras()[0])
        ptr = ctx.lib.rcn_ba_session_points_device(source.h) if L else None
        v = _cloud(ctx, C.c_void_p(ptr) if L else None, L, lm_rgba, inliers, poses34, torch.device("cuda", ctx.device))
    write_ply(path, v, binary)
    return v


def smoke(ctx):
    """One 37 x 50 BGR image with a padded row stride through prepare at max_size 24, and a three-vertex cloud; checks on the
    host what does not need the contract's arithmetic: a constant image stays constant, the swap, the grey of the resized
    colours, the shape.  Returns the prepared shape."""
    import torch
    buf = torch.zeros((1, 37, 50 * 3 + 5), dtype=torch.uint8, device="cuda")
    img = buf[:, :, :150].view(1, 37, 50, 3)
    img[..., 0], img[..., 1], img[..., 2] = 200, 100, 50            # blue, green, red
    rgb, gray, factor = prepare(ctx, img, max_size=24)
    assert tuple(rgb.shape) == (1, 16, 24, 3) and tuple(gray.shape) == (1, 16, 24) and abs(factor - 24 / 50) < 1e-15
    assert (rgb.cpu().numpy() == np.array([50, 100, 200], np.uint8)).all(), "image preparation: a constant image did not stay constant"
    assert (gray.cpu().numpy() == (4899 * 50 + 9617 * 100 + 1868 * 200 + 8192) >> 14).all(), "image preparation: grey value"
    v = cloud_vertices(ctx, np.array([[1.0, 2.0, 3.0]]), np.array([[9, 8, 7, 0]], np.uint8), [0], np.array([[1, 0, 0, -1, 0, 1, 0, -2, 0, 0, 1, -3.0]]))
    assert [tuple(r) for r in v.tolist()] == [(1, 2, 3, 253, 0, 0, 255), (1, 2, 3, 9, 8, 7, 255), (1, 2, 3, 0, 250, 0, 255)], "cloud vertices"
    return tuple(rgb.shape[1:3])
