"""Float64 numpy statement of SuperPoint's forward (DeTone et al., CVPR-W 2018, and the authors' released forward), written
from the paper: the reference tests/test_superpoint_net_ref.py and tests/test_superpoint_net_gpu.py compare against
(DESIGN.md section 22).  Also the fp32 torch transcription whose deviation from it is the unit of the GPU tolerance, the
seeded weights, images and cases the tests share, and the delta weights of the exact test."""
import functools

import numpy as np

from reconstructor_amd import superpoint_net as SP

SEED_WEIGHTS = 2038
# H x W of the GPU test (the issue's table); the three smallest are in the golden file
SHAPES = [(8, 8), (16, 24), (40, 72), (8, 264), (136, 8), (64, 96)]
GOLDEN_SHAPES = [(8, 8), (16, 24), (40, 72)]
ENCODER = ["conv1a", "conv1b", "pool", "conv2a", "conv2b", "pool", "conv3a", "conv3b", "pool", "conv4a", "conv4b"]


@functools.lru_cache(maxsize=None)
def weights():
    sd = SP.random_weights(SEED_WEIGHTS)
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def image(H, W, seed=0):
    """A seeded grey image [H][W] float32 in [0, 1]: smooth blobs plus noise (neither flat nor white)."""
    rng = np.random.default_rng(1000 * H + W + 7919 * seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 0.5 + 0.25 * np.sin(0.37 * x + rng.uniform(0, 6)) * np.cos(0.23 * y + rng.uniform(0, 6)) + 0.2 * rng.standard_normal((H, W))
    img = np.clip(img, 0.0, 1.0).astype(np.float32)
    img.setflags(write=False)
    return img


def conv(x, W, b):
    """x [Cin][H][W], W [Cout][Cin][k][k], k = 1 or 3, zero padding k // 2, plus bias; float64."""
    co, ci, k, _ = W.shape
    H, Wd = x.shape[1:]
    p = k // 2
    xp = np.zeros((ci, H + 2 * p, Wd + 2 * p))
    xp[:, p:p + H, p:p + Wd] = x
    out = np.zeros((co, H, Wd))
    for ky in range(k):
        for kx in range(k):
            out += np.tensordot(W[:, :, ky, kx], xp[:, ky:ky + H, kx:kx + Wd], axes=(1, 0))
    return out + b[:, None, None]


def pool(x):
    C, H, W = x.shape
    return x.reshape(C, H // 2, 2, W // 2, 2).max(axis=(2, 4))


def forward(sd, img, normalize=True, alive=None):
    """(logits [65][Hc][Wc], desc [256][Hc][Wc]) in float64.  sd: state dict under the published names; img [H][W] in [0, 1].
    alive: a dict that receives, per ReLU layer, the fraction of outputs that are positive."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items()}

    def cr(name, x):
        y = conv(x, w[name + ".weight"], w[name + ".bias"])
        if alive is not None:
            alive[name] = float((y > 0).mean())
        return np.maximum(y, 0.0)
    x = np.asarray(img, np.float64)[None]
    for name in ENCODER:
        x = pool(x) if name == "pool" else cr(name, x)
    logits = conv(cr("convPa", x), w["convPb.weight"], w["convPb.bias"])
    desc = conv(cr("convDa", x), w["convDb.weight"], w["convDb.bias"])
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore"):
            desc = desc / np.sqrt((desc * desc).sum(axis=0, keepdims=True))
    return logits, desc


def forward_torch(sd, imgs, normalize=True, dtype=None):
    """The same forward transcribed with torch.nn.functional on whatever device the tensors of `sd` live on; imgs [n][H][W].
    Returns (logits [n][65][Hc][Wc], desc [n][256][Hc][Wc])."""
    import torch
    import torch.nn.functional as F
    t = {k: (torch.from_numpy(np.array(v)) if isinstance(v, np.ndarray) else v) for k, v in sd.items()}
    if dtype is not None:
        t = {k: v.to(dtype) for k, v in t.items()}
    x = (torch.from_numpy(np.array(imgs)) if isinstance(imgs, np.ndarray) else imgs)[:, None].to(t["conv1a.weight"].dtype).to(t["conv1a.weight"].device)
    c = lambda name, x, pad: F.conv2d(x, t[name + ".weight"], t[name + ".bias"], padding=pad)
    for name in ENCODER:
        x = F.max_pool2d(x, 2, 2) if name == "pool" else F.relu(c(name, x, 1))
    logits = c("convPb", F.relu(c("convPa", x, 1)), 0)
    desc = c("convDb", F.relu(c("convDa", x, 1)), 0)
    if normalize:
        desc = desc / torch.norm(desc, p=2, dim=1, keepdim=True)
    return logits, desc


@functools.lru_cache(maxsize=None)
def case(H, W, normalize=True, seed=0):
    """(image, logits f64 [65][Hc][Wc], desc f64 [256][Hc][Wc]) of the seeded weights; computed once, read-only."""
    lg, ds = forward(weights(), image(H, W, seed), normalize)
    lg.setflags(write=False)
    ds.setflags(write=False)
    return image(H, W, seed), lg, ds


@functools.lru_cache(maxsize=None)
def delta_weights(seed=2):
    """Every output channel of every layer has exactly one non-zero weight, 1, at a seeded (cin, ky, kx); biases 0.  (The seed
    is one at which the one-cell-high case keeps some non-zero outputs: there two taps in three read padding only.)"""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, co, ci, k in SP.layer_table():
        W = np.zeros((co, ci, k, k), np.float32)
        W[np.arange(co), rng.integers(0, ci, co), rng.integers(0, k, co), rng.integers(0, k, co)] = 1.0
        W.setflags(write=False)
        sd[name + ".weight"] = W
        sd[name + ".bias"] = np.zeros(co, np.float32)
    return sd


@functools.lru_cache(maxsize=None)
def delta_image(H, W):
    """Integers 0..255 over 256: every value and every sum of one term is exact in fp32."""
    img = (np.random.default_rng(H * 31 + W).integers(0, 256, (H, W)).astype(np.float64) / 256.0).astype(np.float32)
    img.setflags(write=False)
    return img
