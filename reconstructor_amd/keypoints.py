"""Host mirror of the keypoint half of FeatureSuperPoint::detect over librcn.so (no CPU fallback).

    processKeypoints       FeatureSuperPoint.cpp:145-179   extractHeatMap, threshold scan, nmsFast, removeBorderKeypoints
    processDescriptors     FeatureSuperPoint.cpp:183-211   for a batch of images (rcn_desc_sample_batch_device)

Everything stays in HBM: `detect` takes the network's [n][65][H/8][W/8] logits as a torch tensor on
the GPU (any strides: a channel-last tensor is read in place), `nms` a dense heat map, `sample_batch` writes the unit-norm
descriptor rows of the keypoints straight into a caller's buffer -- the slot of pairgrid.Shard.reserve, for one.
"""
import ctypes as C

from . import _lib

HEAT_REFERENCE = 0      # extractHeatMap as the reference writes it (RCN_KP_HEAT_REFERENCE)
HEAT_SOFTMAX = 1        # softmax over the 65 channels of a cell (RCN_KP_HEAT_SOFTMAX)
LDS_STATUS_BYTES = 131072   # RCN_KP_LDS_STATUS_BYTES: images of more than 4 * this many pixels keep the NMS status in HBM


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _outputs(n, K, H, W, want_heat, device):
    import torch
    return dict(xy=torch.empty((n, K, 2), dtype=torch.int32, device=device), conf=torch.empty((n, K), dtype=torch.float32, device=device),
                counts=torch.empty((n,), dtype=torch.int32, device=device), rounds=torch.empty((n,), dtype=torch.int32, device=device),
                heat=torch.empty((n, H, W), dtype=torch.float32, device=device) if want_heat else None)


def detect(ctx, logits, H, W, K, mode=HEAT_REFERENCE, conf_thresh=0.015, nms_radius=4, border=4, want_heat=False):
    """rcn_kp_detect_device.  logits: float32 CUDA tensor of shape [n][65][H/8][W/8], any strides.  Returns a dict of CUDA
    tensors: xy[n][K][2] int32 (x, y) in raster order, conf[n][K], counts[n] (uncapped survivors), rounds[n], heat[n][H][W] or
    None.  Rows past min(counts[i], K) are (-1, -1) / 0."""
    import torch
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 4 or logits.shape[1] != 65 or \
            tuple(logits.shape[2:]) != (H // 8, W // 8):
        raise ValueError("detect: logits must be a float32 CUDA tensor of shape [n][65][H/8][W/8]")
    n = logits.shape[0]
    out = _outputs(n, max(K, 1), H, W, want_heat, logits.device)
    torch.cuda.synchronize()
    si, sc, sy, sx = logits.stride()
    ctx.check(ctx.lib.rcn_kp_detect_device(ctx.h, _ptr(logits), si, sc, sy, sx, n, H, W, int(mode), float(conf_thresh), int(nms_radius),
                                           int(border), int(K), _ptr(out["xy"]), _ptr(out["conf"]), _ptr(out["counts"]), _ptr(out["heat"]),
                                           _ptr(out["rounds"])))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return out


def nms(ctx, heat, K, conf_thresh=0.015, nms_radius=4, border=4):
    """rcn_kp_nms_device: the exact stages on heat maps the caller has, a contiguous float32 CUDA tensor [n][H][W].  Returns
    the dict of `detect` without the heat map."""
    import torch
    if heat.dtype != torch.float32 or not heat.is_cuda or heat.dim() != 3 or not heat.is_contiguous():
        raise ValueError("nms: heat must be a contiguous float32 CUDA tensor of shape [n][H][W]")
    n, H, W = heat.shape
    out = _outputs(n, max(K, 1), H, W, False, heat.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_kp_nms_device(ctx.h, _ptr(heat), n, H, W, float(conf_thresh), int(nms_radius), int(border), int(K),
                                        _ptr(out["xy"]), _ptr(out["conf"]), _ptr(out["counts"]), _ptr(out["rounds"])))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return out


def sample_batch(ctx, desc_maps, xy, counts, D=256, out=None, channel_last=False):
    """rcn_desc_sample_batch_device.  desc_maps: float32 CUDA tensor [n][C][Hc][Wc] (any strides), or [n][Hc][Wc][C] with
    channel_last; xy[n][K][2] / counts[n] as `detect` returns them.  out: device address of an [n][K][D] float32 block (the
    slot of pairgrid.Shard.reserve) or None for a new tensor, which is returned.  Rows past min(counts[i], K) are zeros."""
    import torch
    m = desc_maps.permute(0, 3, 1, 2) if channel_last else desc_maps
    if m.dtype != torch.float32 or not m.is_cuda or m.dim() != 4 or m.shape[1] < D:
        raise ValueError("sample_batch: desc_maps must be a float32 CUDA tensor with at least D channels")
    n, K = xy.shape[0], xy.shape[1]
    if xy.dtype != torch.int32 or counts.dtype != torch.int32 or not xy.is_contiguous() or m.shape[0] != n or counts.shape[0] != n:
        raise ValueError("sample_batch: xy[n][K][2] and counts[n] must be contiguous int32 CUDA tensors")
    rows = None
    if out is None:
        rows = torch.empty((n, K, D), dtype=torch.float32, device=m.device)
        out = rows.data_ptr()
    torch.cuda.synchronize()
    si, sc, sy, sx = m.stride()
    ctx.check(ctx.lib.rcn_desc_sample_batch_device(ctx.h, _ptr(m), si, sc, sy, sx, m.shape[2], m.shape[3], _ptr(xy), _ptr(counts), n, K, D,
                                                   C.c_void_p(out)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return rows


def smoke(ctx):
    """Two synthetic 64 x 96 images through detect -> sample_batch; checks the structure of the result (raster order, spacing,
    border, padding, unit rows) on the host.  Returns (keypoints per image, rounds per image)."""
    import numpy as np
    import torch
    n, H, W, K = 2, 64, 96, 128
    rng = np.random.default_rng(11)
    logits = torch.from_numpy((1.2 * rng.standard_normal((n, 65, H // 8, W // 8))).astype(np.float32)).cuda()
    dmap = torch.from_numpy(rng.standard_normal((n, 256, H // 8, W // 8)).astype(np.float32)).cuda()
    r = detect(ctx, logits, H, W, K, want_heat=True)
    rows = sample_batch(ctx, dmap, r["xy"], r["counts"]).cpu().numpy()
    xy, conf, counts, heat = r["xy"].cpu().numpy(), r["conf"].cpu().numpy(), r["counts"].cpu().numpy(), r["heat"].cpu().numpy()
    for i in range(n):
        m = int(counts[i])
        assert 0 < m <= K, "keypoint stage: no keypoints on the smoke image"
        x, y = xy[i, :m, 0].astype(np.int64), xy[i, :m, 1].astype(np.int64)
        assert (np.diff(y * W + x) > 0).all() and x.min() >= 4 and x.max() < W - 4 and y.min() >= 4 and y.max() < H - 4
        assert np.array_equal(conf[i, :m], heat[i, y, x]) and (conf[i, :m] >= 0.015).all()
        d = np.maximum(np.abs(x[:, None] - x[None]), np.abs(y[:, None] - y[None]))
        assert (d[~np.eye(m, dtype=bool)] > 4).all(), "keypoint stage: two keypoints inside one NMS window"
        assert (xy[i, m:] == -1).all() and (conf[i, m:] == 0).all() and (rows[i, m:] == 0).all()
        assert np.allclose(np.linalg.norm(rows[i, :m].astype(np.float64), axis=1), 1.0, atol=1e-6)
    return counts.tolist(), r["rounds"].cpu().numpy().tolist()
