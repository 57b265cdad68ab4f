"""Plane-sweep depth maps, the cross-view check and the dense cloud over librcn.so (no CPU fallback).

    options           rcn_mvs_options
    layout            rcn_mvs_layout: the sweep's tile, LDS and array sizes (pure host code)
    inv_depths        the uniform-in-inverse-depth plane list over [near, far] (pure host code)
    homographies      H[s][k] of one reference view (pure host code, no contraction)
    session_views     a BA session -> every camera's S most covisible cameras and its depth range, one call on the device
    undistort         the resample that removes k1, k2
    sweep             views -> plane int16, depth float32, cost float32
    consistency       -> mask uint8, counts int32
    fuse              -> 16-byte vertices (imgprep.VERTEX_DTYPE), (written, total)
    dense_cloud       the chain, optionally to a PLY file

Images are torch uint8 tensors on the GPU, dense in their last dimension; cameras are numpy arrays: poses34 [n][12] rows of [R | t],
intrinsics [n][6] = fx fy cx cy k1 k2; views int32 [V][1 + S] = (reference image, its sources, -1: none).
"""
import ctypes as C

import numpy as np

from . import _lib
from .imgprep import VERTEX_DTYPE, write_ply

MAX_PLANES, MAX_SOURCES = 1024, 16


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def options(radius=None, min_sources=None, min_consistent=None, stride=None, max_cost=None, rel_tol=None):
    o = _lib.MvsOptions()
    _lib.load().rcn_mvs_default_options(C.byref(o))
    for name, v in (("radius", radius), ("min_sources", min_sources), ("min_consistent", min_consistent), ("stride", stride)):
        if v is not None:
            setattr(o, name, int(v))
    for name, v in (("max_cost", max_cost), ("rel_tol", rel_tol)):
        if v is not None:
            setattr(o, name, float(v))
    return o


def layout(rows, cols, V, D, S, radius=3):
    z = _lib.MvsSizes()
    rc = _lib.load().rcn_mvs_layout(int(rows), int(cols), int(V), int(D), int(S), int(radius), C.byref(z))
    if rc != _lib.RCN_OK:
        raise _lib.RcnError(rc, "rcn_mvs_layout(rows=%d, cols=%d, V=%d, D=%d, S=%d, radius=%d)" % (rows, cols, V, D, S, radius))
    return {k: getattr(z, k) for k, _ in z._fields_}


def inv_depths(near, far, D):
    out = np.zeros(max(int(D), 0))
    rc = _lib.load().rcn_mvs_inv_depths(float(near), float(far), int(D), out.ctypes.data if len(out) else None)
    if rc != _lib.RCN_OK:
        raise _lib.RcnError(rc, "rcn_mvs_inv_depths(near=%r, far=%r, D=%d)" % (near, far, D))
    return out


def homographies(poses34, intrinsics, ref, srcs, inv):
    """float64 [S][D][9] (rcn_mvs_homographies)."""
    P = np.ascontiguousarray(poses34, np.float64).reshape(-1, 12)
    K = np.ascontiguousarray(intrinsics, np.float64).reshape(-1, 6)
    srcs, inv = np.ascontiguousarray(srcs, np.int32).reshape(-1), np.ascontiguousarray(inv, np.float64).reshape(-1)
    if int(ref) >= len(P) or (len(srcs) and srcs.max() >= len(P)):
        raise ValueError("mvs: a camera index outside the cameras")
    out = np.zeros((len(srcs), len(inv), 9))
    rc = _lib.load().rcn_mvs_homographies(P.ctypes.data, K.ctypes.data, int(ref), srcs.ctypes.data if len(srcs) else None, len(srcs),
                                          inv.ctypes.data if len(inv) else None, len(inv), out.ctypes.data if out.size else None)
    if rc != _lib.RCN_OK:
        raise _lib.RcnError(rc, "rcn_mvs_homographies(ref=%d, srcs=%s, D=%d)" % (ref, srcs.tolist(), len(inv)))
    return out


def view_homographies(poses34, intrinsics, views, inv):
    """float64 [V][S][D][9] for views [V][1 + S] and plane lists inv [V][D]."""
    views = np.asarray(views, np.int32)
    return np.stack([homographies(poses34, intrinsics, v[0], v[1:], inv[i]) for i, v in enumerate(views)]) if len(views) else np.zeros((0, views.shape[1] - 1, 0, 9))


def session_views(session, S, poses34=None, want_counts=False):
    """(sources int32 [n_cams][S], depth range float64 [n_cams][2][, shared-landmark counts int32 [n_cams][n_cams]])
    (rcn_ba_session_mvs_views).  poses34 defaults to the session's cameras as the pipeline holds them."""
    from .ba import poses34_from_angle_axis
    nc = session.counts()[0]
    if poses34 is None:
        poses34 = poses34_from_angle_axis(session.cameras()[0])
    P = np.ascontiguousarray(poses34, np.float64).reshape(-1, 12)
    if len(P) != nc:
        raise ValueError("mvs: one pose per session camera")
    src, rng = np.full((nc, max(int(S), 1)), -1, np.int32), np.zeros((nc, 2))
    cov = np.zeros((nc, nc), np.int32) if want_counts else None
    session.ctx.check(session.ctx.lib.rcn_ba_session_mvs_views(session.h, P.ctypes.data if nc else None, int(S), src.ctypes.data if nc else None,
                                                               rng.ctypes.data if nc else None, cov.ctypes.data if want_counts and nc else None))
    return (src, rng, cov) if want_counts else (src, rng)


def _images(images, what):
    import torch
    if not isinstance(images, torch.Tensor) or not images.is_cuda or images.dtype != torch.uint8 or images.dim() not in (3, 4):
        raise ValueError("mvs: %s must be a uint8 CUDA tensor [n][rows][cols] or [n][rows][cols][3]" % what)
    ch = images.shape[3] if images.dim() == 4 else 1
    st = images.stride()
    if (images.dim() == 4 and (st[3] != 1 or st[2] != ch)) or (images.dim() == 3 and st[2] != 1):
        raise ValueError("mvs: the pixels of a row must be dense")
    return ch, st[0], st[1]


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def undistort(ctx, images, intrinsics):
    """rcn_img_undistort_device: a dense tensor of the images' shape."""
    import torch
    ch, si, sr = _images(images, "images")
    n, rows, cols = images.shape[:3]
    K = _dev(np.asarray(intrinsics, np.float64).reshape(-1, 6), np.float64)
    if K.shape[0] != n:
        raise ValueError("mvs: one intrinsics row per image")
    out = torch.empty(tuple(images.shape), dtype=torch.uint8, device=images.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_img_undistort_device(ctx.h, _ptr(images), si, sr, ch, n, rows, cols, _ptr(K), _ptr(out)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return out


def _views(views):
    v = np.ascontiguousarray(views, np.int32)
    if v.ndim != 2 or v.shape[1] < 2:
        raise ValueError("mvs: views must be int32 [V][1 + S]")
    return v, v.shape[0], v.shape[1] - 1


def sweep(ctx, gray, views, H, inv, opt=None):
    """rcn_mvs_sweep_device: (plane int16, depth float32, cost float32), CUDA tensors [V][rows][cols].  H float64 [V][S][D][9] and inv
    float64 [V][D] are numpy arrays or CUDA tensors."""
    import torch
    ch, si, sr = _images(gray, "gray")
    if ch != 1:
        raise ValueError("mvs: the sweep reads one channel")
    n, rows, cols = gray.shape
    v, V, S = _views(views)
    Hd = H if isinstance(H, torch.Tensor) else _dev(H, np.float64)
    invd = inv if isinstance(inv, torch.Tensor) else _dev(np.asarray(inv, np.float64).reshape(V, -1), np.float64)
    D = invd.shape[1] if V else 1
    if V and (tuple(Hd.shape) != (V, S, D, 9) or Hd.dtype != torch.float64 or invd.dtype != torch.float64):
        raise ValueError("mvs: H must be float64 [V][S][D][9] and inv float64 [V][D]")
    plane = torch.empty((V, rows, cols), dtype=torch.int16, device=gray.device)
    depth = torch.empty((V, rows, cols), dtype=torch.float32, device=gray.device)
    cost = torch.empty((V, rows, cols), dtype=torch.float32, device=gray.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_mvs_sweep_device(ctx.h, _ptr(gray), si, sr, n, rows, cols, v.ctypes.data if V else None, V, S, _ptr(Hd.contiguous()), _ptr(invd.contiguous()),
                                           D, C.byref(opt) if opt is not None else None, _ptr(plane), _ptr(depth), _ptr(cost)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return plane, depth, cost


def consistency(ctx, views, poses34, intrinsics, plane, depth, opt=None):
    """rcn_mvs_consistency_device: (mask uint8 [V][rows][cols], counts int32 [V]), CUDA tensors."""
    import torch
    v, V, S = _views(views)
    P, K = _dev(np.asarray(poses34, np.float64).reshape(-1, 12), np.float64), _dev(np.asarray(intrinsics, np.float64).reshape(-1, 6), np.float64)
    if tuple(plane.shape) != tuple(depth.shape) or plane.shape[0] != V or P.shape[0] != K.shape[0]:
        raise ValueError("mvs: plane and depth must be [V][rows][cols], one pose per intrinsics row")
    rows, cols = plane.shape[1:]
    mask = torch.empty((V, rows, cols), dtype=torch.uint8, device=plane.device)
    counts = torch.empty((max(V, 1),), dtype=torch.int32, device=plane.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_mvs_consistency_device(ctx.h, v.ctypes.data if V else None, V, S, _ptr(P), _ptr(K), P.shape[0], rows, cols, _ptr(plane.contiguous()),
                                                 _ptr(depth.contiguous()), C.byref(opt) if opt is not None else None, _ptr(mask), _ptr(counts)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return mask, counts[:V]


def fuse(ctx, views, poses34, intrinsics, rgb, depth, mask, opt=None, capacity=None):
    """rcn_mvs_fuse_device: (vertices on the host as VERTEX_DTYPE records, (written, total)).  rgb [n][rows][cols][3] dense or None
    (black); capacity None: room for every sampled pixel."""
    import torch
    v, V, S = _views(views)
    P, K = _dev(np.asarray(poses34, np.float64).reshape(-1, 12), np.float64), _dev(np.asarray(intrinsics, np.float64).reshape(-1, 6), np.float64)
    rows, cols = depth.shape[1:]
    if rgb is not None and (tuple(rgb.shape) != (P.shape[0], rows, cols, 3) or not rgb.is_contiguous()):
        raise ValueError("mvs: rgb must be dense [n][rows][cols][3]")
    stride = opt.stride if opt is not None else 1
    if capacity is None:
        capacity = V * ((rows + stride - 1) // max(stride, 1)) * ((cols + stride - 1) // max(stride, 1))
    out = torch.empty((max(int(capacity), 1), 16), dtype=torch.uint8, device=depth.device)
    cnt = torch.zeros(2, dtype=torch.int64, device=depth.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_mvs_fuse_device(ctx.h, v.ctypes.data if V else None, V, S, _ptr(P), _ptr(K), P.shape[0], _ptr(rgb), rows, cols, _ptr(depth.contiguous()),
                                          _ptr(mask.contiguous()), C.byref(opt) if opt is not None else None, int(capacity), C.c_void_p(out.data_ptr()), _ptr(cnt)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    written, total = (int(x) for x in cnt.cpu())
    return out[:written].cpu().numpy().reshape(-1).view(VERTEX_DTYPE), (written, total)


def dense_cloud(source, gray, rgb=None, views=None, inv=None, S=4, D=128, widen=1.25, opt=None, capacity=None, path=None, binary=True):
    """views -> undistort -> sweep -> consistency -> fuse (-> PLY).  source: a ba.BaSession (its cameras; views and plane lists
    default to session_views with every range widened by `widen` on both sides and D planes) or a tuple (ctx, poses34, intrinsics)
    with explicit views [V][1 + S] and inv [V][D].  gray [n][rows][cols], rgb [n][rows][cols][3] or None: the prepared planes of
    imgprep.prepare, image i seen by camera i.  Returns dict(views, inv, plane, depth, cost, mask, counts, vertices, written, total)."""
    if isinstance(source, tuple):
        ctx, poses34, intrinsics = source
        if views is None or inv is None:
            raise ValueError("mvs: explicit cameras need explicit views and plane lists")
    else:
        from .ba import poses34_from_angle_axis
        ctx = source.ctx
        pose6, intrinsics = source.cameras()
        poses34 = poses34_from_angle_axis(pose6)
        if views is None or inv is None:
            src, rng = session_views(source, S, poses34)
            keep = [c for c in range(len(src)) if src[c, 0] >= 0 and rng[c, 0] > 0]
            views = np.concatenate([np.array(keep, np.int32)[:, None], src[keep]], 1) if keep else np.zeros((0, 1 + S), np.int32)
            inv = np.stack([inv_depths(rng[c, 0] / widen, rng[c, 1] * widen, D) for c in keep]) if keep else np.zeros((0, D))
    views, inv = np.ascontiguousarray(views, np.int32), np.ascontiguousarray(inv, np.float64)
    g = undistort(ctx, gray, intrinsics)
    c = None if rgb is None else undistort(ctx, rgb, intrinsics)
    H = view_homographies(poses34, intrinsics, views, inv)
    plane, depth, cost = sweep(ctx, g, views, H, inv, opt)
    mask, counts = consistency(ctx, views, poses34, intrinsics, plane, depth, opt)
    vert, (written, total) = fuse(ctx, views, poses34, intrinsics, c, depth, mask, opt, capacity)
    if path is not None:
        write_ply(path, vert, binary)
    return dict(views=views, inv=inv, plane=plane, depth=depth, cost=cost, mask=mask, counts=counts, vertices=vert, written=written, total=total)


def smoke(ctx):
    """A ray-cast wall 5 away seen by four 48 x 40 cameras, every camera a reference: the chain end to end; every vertex must lie near
    the wall (no contract on the host here: the tests hold the device to it bit for bit).  Returns (views, vertices, worst |z - 5|)."""
    import torch
    from . import synth_mvs
    sc = synth_mvs.wall_scene(4, 40, 48, 60.0, d=5.0, baseline=0.3)
    views = np.array([[i] + [j for j in range(4) if j != i] for i in range(4)], np.int32)
    inv = np.tile(inv_depths(3.0, 8.0, 24), (4, 1))
    out = dense_cloud((ctx, sc["poses34"], sc["intrinsics"]), torch.as_tensor(sc["gray"]).cuda(), torch.as_tensor(sc["rgb"]).cuda(), views, inv,
                      opt=options(radius=2, stride=2))
    v = out["vertices"]
    assert out["written"] == out["total"] == len(v) and len(v) > 200, "plane sweep: too few consistent pixels (%d)" % len(v)
    worst = float(np.abs(v["z"] - 5.0).max())
    assert worst < 0.25, "plane sweep: a vertex %.3f off the wall" % worst
    assert (v["alpha"] == 255).all() and (v["green"] == 255 - v["red"]).all(), "plane sweep: vertex colours"
    return len(views), len(v), worst
