"""Host mirror of SuperPoint's convolutional network over librcn.so (no CPU fallback).

    FeatureSuperPoint::detect   FeatureSuperPoint.cpp:228-263   superNet.forward, then the keypoint and descriptor stages
    prepImg                     FeatureSuperPoint.cpp:278-285   byte image -> float, v / 255.0 in double

The library ships no weights.  `pack_state_dict` takes a state dict under the published parameter names (numpy arrays or
torch tensors), checks every shape and packs the layers in the order rcn_sp_net_create documents; `Net` hands the block to
the library; `forward` returns the channel-last logits and descriptor maps, `detect` runs the keypoint stage and the
descriptor sampling behind them in the same call (reconstructor_amd.keypoints describes their outputs).  Everything stays
in HBM.  `random_weights` is the seeded generator the tests, the smoke run and tools/superpoint_net_timing.py share: a
network in which every ReLU layer is alive.
"""
import ctypes as C

import numpy as np

from .keypoints import HEAT_REFERENCE, _outputs, _ptr

N_PARAMS = 1300865                     # RCN_SP_N_PARAMS
NORMALIZE_DESC = 1                     # RCN_SP_NORMALIZE_DESC
INPUT_F32, INPUT_U8 = 0, 1             # RCN_SP_INPUT_*
D = 256

# (name, Cout, Cin, kernel size) in the packing order of rcn_sp_net_create.  The names are those of the authors' released
# model (conv1a.weight ... convDb.bias), written down from memory: they cannot be checked here against a checkpoint.
_LAYERS = [("conv1a", 64, 1, 3), ("conv1b", 64, 64, 3), ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3), ("conv3a", 128, 64, 3),
           ("conv3b", 128, 128, 3), ("conv4a", 128, 128, 3), ("conv4b", 128, 128, 3), ("convPa", 256, 128, 3), ("convPb", 65, 256, 1),
           ("convDa", 256, 128, 3), ("convDb", 256, 256, 1)]
RELU_LAYERS = [n for n, _, _, k in _LAYERS if k == 3]      # every 3 x 3 convolution is followed by a ReLU


def layer_table():
    return list(_LAYERS)


def param_count():
    return sum(co * ci * k * k + co for _, co, ci, k in _LAYERS)


def _np(v):
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)


def pack_state_dict(sd):
    """params float32 [N_PARAMS]: per layer W [Cout][Cin][k][k] row-major, then b [Cout].  Missing keys, extra keys and wrong
    shapes are rejected."""
    want = {n + s for n, _, _, _ in _LAYERS for s in (".weight", ".bias")}
    missing, extra = sorted(want - set(sd)), sorted(set(sd) - want)
    if missing or extra:
        raise KeyError("pack_state_dict: missing %s, unexpected %s" % (missing, extra))
    parts = []
    for name, co, ci, k in _LAYERS:
        W, b = _np(sd[name + ".weight"]), _np(sd[name + ".bias"])
        if W.shape != (co, ci, k, k) or b.shape != (co,):
            raise ValueError("%s: weight %s / bias %s, expected %s / (%d,)" % (name, W.shape, b.shape, (co, ci, k, k), co))
        parts += [W.astype(np.float32).ravel(), b.astype(np.float32)]
    params = np.concatenate(parts)
    assert params.size == N_PARAMS
    return params


GAINS = {"convPb": 2.5}          # per-layer factors on the He standard deviation (default 1): a one-cell image is all border and loses signal layer by layer


def random_weights(seed, gains=None):
    """A seeded state dict (fp32 numpy arrays, published names and shapes): weights N(0, g^2 * 2 / fan_in), biases
    0.05 N(0, 1).  With images U(0, 1) every ReLU layer keeps between 20 % and 80 % of its outputs positive and the logits
    have a standard deviation above 0.1 (tests/test_superpoint_net_ref.py asserts it on the test cases)."""
    g = dict(GAINS, **(gains or {}))
    rng = np.random.default_rng(seed)
    sd = {}
    for name, co, ci, k in _LAYERS:
        sd[name + ".weight"] = (rng.standard_normal((co, ci, k, k)) * g.get(name, 1.0) * np.sqrt(2.0 / (ci * k * k))).astype(np.float32)
        sd[name + ".bias"] = (0.05 * rng.standard_normal(co)).astype(np.float32)
    return sd


def prep_u8(img):
    """prepImg's rule on the host: (float)((double)v / 255.0)."""
    return (np.asarray(img, np.uint8).astype(np.float64) / 255.0).astype(np.float32)


def set_chunk_images(ctx, images):
    """rcn_sp_net_set_chunk_images: images per chunk of the forward (<= 0: as many as fit the default workspace cap)."""
    ctx.check(ctx.lib.rcn_sp_net_set_chunk_images(ctx.h, int(images)))


class Net:
    """One rcn_sp_net: the packed layers of `pack_state_dict` in HBM.  Close it before its ctx."""

    def __init__(self, ctx, params):
        params = np.ascontiguousarray(params, np.float32)
        h = C.c_void_p()
        ctx.check(ctx.lib.rcn_sp_net_create(ctx.h, params.ctypes.data, int(params.size), C.byref(h)))
        self.ctx, self.h = ctx, h

    @classmethod
    def from_state_dict(cls, ctx, sd):
        return cls(ctx, pack_state_dict(sd))

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.rcn_sp_net_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _images(images):
    """(pointer, dtype, stride_img, stride_y, stride_x, n, H, W) of a float32 or uint8 CUDA tensor [n][H][W], any strides."""
    import torch
    if images.dim() != 3 or not images.is_cuda or images.dtype not in (torch.float32, torch.uint8):
        raise ValueError("images must be a float32 or uint8 CUDA tensor of shape [n][H][W]")
    n, H, W = images.shape
    return (_ptr(images), INPUT_U8 if images.dtype == torch.uint8 else INPUT_F32, *images.stride(), n, H, W)


def forward(ctx, net, images, normalize=True, out=None):
    """rcn_sp_net_forward_device.  images: [n][H][W] float32 in [0, 1] or uint8, any strides.  Returns (logits [n][Hc][Wc][65],
    desc [n][Hc][Wc][256]), channel-last; `out` gives the two tensors to write into."""
    import torch
    args = _images(images)
    n, H, W = args[-3:]
    lg, ds = out if out is not None else (torch.empty((n, H // 8, W // 8, 65), dtype=torch.float32, device=images.device),
                                          torch.empty((n, H // 8, W // 8, D), dtype=torch.float32, device=images.device))
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_sp_net_forward_device(ctx.h, net.h, *args, NORMALIZE_DESC if normalize else 0, _ptr(lg), _ptr(ds)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return lg, ds


def detect(ctx, net, images, K, normalize=True, mode=HEAT_REFERENCE, conf_thresh=0.015, nms_radius=4, border=4, want_heat=False):
    """rcn_sp_net_detect_device: the forward, rcn_kp_detect_device and rcn_desc_sample_batch_device in one call.  Returns the
    dict of keypoints.detect plus rows [n][K][256]: unit descriptor rows, zeros past min(counts[i], K)."""
    import torch
    args = _images(images)
    n, H, W = args[-3:]
    o = _outputs(n, max(K, 1), H, W, want_heat, images.device)
    o["rows"] = torch.empty((n, max(K, 1), D), dtype=torch.float32, device=images.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_sp_net_detect_device(ctx.h, net.h, *args, NORMALIZE_DESC if normalize else 0, int(mode), float(conf_thresh), int(nms_radius),
                                               int(border), int(K), D, _ptr(o["xy"]), _ptr(o["conf"]), _ptr(o["counts"]), _ptr(o["rows"]),
                                               _ptr(o["heat"]), _ptr(o["rounds"])))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return o


def smoke(ctx):
    """Two synthetic 64 x 96 images through `detect` with seeded weights; checks the structure of the result (raster order,
    spacing, border, padding, unit rows) on the host, as keypoints.smoke does.  Returns (keypoints per image, rounds)."""
    import torch
    n, H, W, K = 2, 64, 96, 256
    rng = np.random.default_rng(11)
    images = torch.from_numpy(rng.random((n, H, W), dtype=np.float32)).cuda()
    with Net.from_state_dict(ctx, random_weights(7)) as net:
        r = detect(ctx, net, images, K, want_heat=True)
    xy, conf, counts, heat, rows = (r[k].cpu().numpy() for k in ("xy", "conf", "counts", "heat", "rows"))
    for i in range(n):
        m = int(counts[i])
        assert 0 < m <= K, "SuperPoint network: no keypoints on the smoke image"
        x, y = xy[i, :m, 0].astype(np.int64), xy[i, :m, 1].astype(np.int64)
        assert (np.diff(y * W + x) > 0).all() and x.min() >= 4 and x.max() < W - 4 and y.min() >= 4 and y.max() < H - 4
        assert np.array_equal(conf[i, :m], heat[i, y, x]) and (conf[i, :m] >= 0.015).all()
        d = np.maximum(np.abs(x[:, None] - x[None]), np.abs(y[:, None] - y[None]))
        assert (d[~np.eye(m, dtype=bool)] > 4).all(), "SuperPoint network: two keypoints inside one NMS window"
        assert (xy[i, m:] == -1).all() and (conf[i, m:] == 0).all() and (rows[i, m:] == 0).all()
        assert np.allclose(np.linalg.norm(rows[i, :m].astype(np.float64), axis=1), 1.0, atol=1e-6)
    return counts.tolist(), r["rounds"].cpu().numpy().tolist()
