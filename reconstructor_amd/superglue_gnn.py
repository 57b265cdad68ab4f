"""Host mirror of SuperGlue's attentional graph network over librcn.so (no CPU fallback).

    FeatureMatcherSuperglue::matchFeatures   FeatureMatcherSuperglue.cpp:51-101   what runs in front of the optimal-matching layer
    normalizeFeatCoords                      utils.cpp:119-149

The library ships no weights.  `fold_state_dict` takes a state dict under the published parameter names (numpy arrays or
torch tensors), folds every BatchNorm into the convolution in front of it in float64, rounds once to fp32 and packs the
plain linear layers in the order rcn_sg_net_create documents; `Net` hands the block to the library; `forward` returns the
matching descriptors, `match` runs the optimal-matching layer behind them in the same call (reconstructor_amd.superglue
describes its outputs).  Everything stays in HBM.  `random_weights` is the seeded generator the tests, the smoke run and
tools/superglue_gnn_timing.py share: weights at which attention is neither uniform nor one-hot.
"""
import ctypes as C

import numpy as np

from .superglue import _counts, _desc, _out_args, _outputs, _ptr

D = 256
ENC = (3, 32, 64, 128, 256, 256)
SELF, CROSS = 0, 1                     # RCN_SG_LAYER_*
BN_EPS = 1e-5
COORD_RANGE = 0.7                      # normalizeFeatCoords: scale = max(H, W) * range


def layer_table(L):
    """The one table of names: (convolution, BatchNorm behind it or None, Cout, Cin) in the packing order of rcn_sg_net_create.
    The names are those of the authors' released model, written down from memory: check them against a real checkpoint."""
    t = [("kenc.encoder.%d" % (3 * i), "kenc.encoder.%d" % (3 * i + 1) if i < 4 else None, ENC[i + 1], ENC[i]) for i in range(5)]
    for l in range(L):
        p = "gnn.layers.%d." % l
        t += [(p + "attn.proj.0", None, D, D), (p + "attn.proj.1", None, D, D), (p + "attn.proj.2", None, D, D),
              (p + "attn.merge", None, D, D), (p + "mlp.0", p + "mlp.1", 2 * D, 2 * D), (p + "mlp.3", None, D, 2 * D)]
    return t + [("final_proj", None, D, D)]


def param_count(L):
    return sum(co * ci + co for _, _, co, ci in layer_table(L))


def _np64(v):
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64)


def count_layers(sd):
    L = 0
    while "gnn.layers.%d.attn.merge.weight" % L in sd:
        L += 1
    return L


def fold_layers(sd, L=None):
    """[(W [Cout][Cin], b [Cout])] in float64, in packing order, BatchNorm folded: s = gamma / sqrt(var + eps), W' = s W,
    b' = s (b - mean) + beta."""
    L = count_layers(sd) if L is None else L
    out = []
    for conv, bn, co, ci in layer_table(L):
        W, b = _np64(sd[conv + ".weight"]), _np64(sd[conv + ".bias"])
        if W.shape not in ((co, ci), (co, ci, 1)) or b.shape != (co,):
            raise ValueError("%s: weight %s / bias %s, expected (%d, %d[, 1]) / (%d,)" % (conv, W.shape, b.shape, co, ci, co))
        W = W.reshape(co, ci)
        if bn is not None:
            g, beta, mean, var = (_np64(sd[bn + "." + k]) for k in ("weight", "bias", "running_mean", "running_var"))
            if not all(a.shape == (co,) for a in (g, beta, mean, var)):
                raise ValueError("%s: BatchNorm parameters must have shape (%d,)" % (bn, co))
            s = g / np.sqrt(var + BN_EPS)
            W, b = s[:, None] * W, s * (b - mean) + beta
        out.append((W, b))
    return out


def fold_state_dict(sd, layer_types=None):
    """(params float32 [param_count(L)], layer_types [L], bin_score).  layer_types default to the published alternation
    self, cross, self, ... (the state dict does not carry them)."""
    L = count_layers(sd)
    layers = fold_layers(sd, L)
    types = [SELF if l % 2 == 0 else CROSS for l in range(L)] if layer_types is None else [CROSS if t in (CROSS, "cross") else SELF for t in layer_types]
    if len(types) != L:
        raise ValueError("fold_state_dict: %d layer types for %d layers" % (len(types), L))
    params = np.concatenate([np.concatenate([W.ravel(), b]) for W, b in layers]).astype(np.float32)
    assert params.size == param_count(L)
    return params, types, float(_np64(sd["bin_score"]).reshape(-1)[0])


GAINS = dict(qk=12.0, v=0.3, merge=0.3, mlp0=1.4, mlp1=0.3, enc_first=3.0, enc=1.4, enc_last_scale=0.02, final=12.0, bin_score=1.0)


def random_weights(seed, L, gains=None):
    """A seeded state dict (fp32 numpy arrays, published names and shapes) of L layers: weights N(0, g^2 / Cin) with the
    gains of GAINS (overridden by `gains`), biases 0.05 N(0, 1) and zero on the last layer of each MLP, BatchNorm gamma and
    variance U(0.5, 1.5), beta and mean 0.1 N(0, 1).  PyTorch's default initialisation gives near-uniform attention, which
    exercises nothing; these gains give peak probabilities that sharpen over the layers."""
    g = dict(GAINS, **(gains or {}))
    rng = np.random.default_rng(seed)
    sd = {}
    for idx, (conv, bn, co, ci) in enumerate(layer_table(L)):
        tail = conv.rsplit(".", 1)[-1]
        if conv.startswith("kenc"):
            gain = g["enc_first"] if idx == 0 else g["enc"] * (g["enc_last_scale"] if idx == 4 else 1.0)
        elif conv == "final_proj":
            gain = g["final"]
        elif "attn.proj" in conv:
            gain = g["qk"] if tail in ("0", "1") else g["v"]
        elif "merge" in conv:
            gain = g["merge"]
        else:
            gain = g["mlp0"] if tail == "0" else g["mlp1"]
        last = conv == "kenc.encoder.12" or conv.endswith("mlp.3")
        sd[conv + ".weight"] = (rng.standard_normal((co, ci, 1)) * gain / np.sqrt(ci)).astype(np.float32)
        sd[conv + ".bias"] = (np.zeros(co) if last else 0.05 * rng.standard_normal(co)).astype(np.float32)
        if bn is not None:
            sd[bn + ".weight"] = rng.uniform(0.5, 1.5, co).astype(np.float32)
            sd[bn + ".bias"] = (0.1 * rng.standard_normal(co)).astype(np.float32)
            sd[bn + ".running_mean"] = (0.1 * rng.standard_normal(co)).astype(np.float32)
            sd[bn + ".running_var"] = rng.uniform(0.5, 1.5, co).astype(np.float32)
    sd["bin_score"] = np.array(g["bin_score"], np.float32)
    return sd


def planted_inputs(rng, m, n, n_planted, desc_noise=0.05, kp_noise=0.01):
    """Inputs of a synthetic pair: unit descriptor rows, keypoints U(-0.7, 0.7) (normalised already), scores U(0.05, 1); the
    first n_planted points of image 0 reappear at random rows of image 1 (descriptor noise, keypoint noise, the same score).
    Returns (kpts0 [m][2], scores0 [m], d0 [m][256], kpts1, scores1, d1, target [m], -1 = none), fp32."""
    from .superglue import planted_pair
    d0, d1, target = planted_pair(rng, m, n, n_planted, D=D, noise=desc_noise, gain=1.0)
    k0, k1 = rng.uniform(-0.7, 0.7, (m, 2)), rng.uniform(-0.7, 0.7, (n, 2))
    s0, s1 = rng.uniform(0.05, 1.0, m), rng.uniform(0.05, 1.0, n)
    rows = np.nonzero(target >= 0)[0]
    k1[target[rows]] = k0[rows] + kp_noise * rng.standard_normal((len(rows), 2))
    s1[target[rows]] = s0[rows]
    f = np.float32
    return k0.astype(f), s0.astype(f), d0, k1.astype(f), s1.astype(f), d1, target


def set_chunk_pairs(ctx, pairs):
    """rcn_sg_net_set_chunk_pairs: pairs per chunk of the forward (<= 0: as many as fit the default workspace cap)."""
    ctx.check(ctx.lib.rcn_sg_net_set_chunk_pairs(ctx.h, int(pairs)))


class Net:
    """One rcn_sg_net: the packed plain layers of `fold_state_dict` in HBM.  Close it before its ctx."""

    def __init__(self, ctx, params, layer_types, bin_score):
        params = np.ascontiguousarray(params, np.float32)
        types = np.ascontiguousarray(layer_types, np.int32)
        h = C.c_void_p()
        ctx.check(ctx.lib.rcn_sg_net_create(ctx.h, types.ctypes.data if types.size else None, int(types.size), params.ctypes.data, int(params.size),
                                            float(bin_score), C.byref(h)))
        self.ctx, self.h, self.L, self.bin_score = ctx, h, int(types.size), float(bin_score)

    @classmethod
    def from_state_dict(cls, ctx, sd, layer_types=None):
        return cls(ctx, *fold_state_dict(sd, layer_types))

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.rcn_sg_net_destroy(self.h)
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


def _inputs(kpts0, scores0, d0, kpts1, scores1, d1, shapes0, shapes1, m, n, channel_first):
    import torch
    a, b = _desc(d0, channel_first, "d0"), _desc(d1, channel_first, "d1")
    B, M, Dd = a.shape
    N = b.shape[1]
    if b.shape[0] != B or b.shape[2] != Dd:
        raise ValueError("d0 and d1 disagree on B or D")
    for t, shape, name in ((kpts0, (B, M, 2), "kpts0"), (scores0, (B, M), "scores0"), (kpts1, (B, N, 2), "kpts1"), (scores1, (B, N), "scores1")):
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError("%s must be a contiguous float32 CUDA tensor of shape %s" % (name, list(shape)))
    for t, name in ((shapes0, "shapes0"), (shapes1, "shapes1")):
        if t is not None and (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (B, 2)):
            raise ValueError("%s must be a contiguous int32 CUDA tensor of shape [B][2] holding (H, W)" % name)
    args = (_ptr(kpts0), _ptr(scores0), _ptr(a), *a.stride(), _ptr(kpts1), _ptr(scores1), _ptr(b), *b.stride(), _ptr(shapes0), _ptr(shapes1),
            _ptr(_counts(m, B, "m")), _ptr(_counts(n, B, "n")), B, M, N, Dd)
    return args, (B, M, N), a.device


def forward(ctx, net, kpts0, scores0, d0, kpts1, scores1, d1, shapes0=None, shapes1=None, m=None, n=None, channel_first=False, out=None):
    """rcn_sg_net_forward_device.  kpts [B][M][2] / [B][N][2], scores [B][M] / [B][N], descriptors as superglue.scores;
    shapes: int32 [B][2] (H, W) or None (coordinates normalised already).  Returns (mdesc0 [B][M][256], mdesc1 [B][N][256]);
    rows past a pair's counts, and empty pairs, are not written (the tensors are filled with NaN first unless `out` gives them)."""
    import torch
    args, (B, M, N), dev = _inputs(kpts0, scores0, d0, kpts1, scores1, d1, shapes0, shapes1, m, n, channel_first)
    m0, m1 = out if out is not None else (torch.full((B, M, D), float("nan"), dtype=torch.float32, device=dev),
                                          torch.full((B, N, D), float("nan"), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_sg_net_forward_device(ctx.h, net.h, *args, _ptr(m0), _ptr(m1)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return m0, m1


def match(ctx, net, kpts0, scores0, d0, kpts1, scores1, d1, shapes0=None, shapes1=None, m=None, n=None, opt=None, channel_first=False,
          table_stride=None, want_logp=False):
    """rcn_sg_net_match_device: the forward, then the optimal-matching layer with alpha = the net's bin_score.  Result as
    superglue.match."""
    import torch
    args, (B, M, N), dev = _inputs(kpts0, scores0, d0, kpts1, scores1, d1, shapes0, shapes1, m, n, channel_first)
    o = _outputs(B, M, N, table_stride, want_logp, dev)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_sg_net_match_device(ctx.h, net.h, *args, C.byref(opt) if opt is not None else None, *_out_args(o)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return o


def smoke(ctx):
    """Image 1 is a row permutation of image 0: the network is permutation equivariant, so mdesc1[perm] must equal mdesc0 up
    to the rounding of another summation order, and the optimal-matching layer must send every row to its image.  Two pairs
    of different size in one ragged batch, two layers (self, cross).  Returns (points per pair, largest relative deviation)."""
    import torch
    rng = np.random.default_rng(11)
    shapes = [(150, 150), (70, 70)]
    M = 150
    k0, s0, d0 = np.full((2, M, 2), np.nan, np.float32), np.full((2, M), np.nan, np.float32), np.full((2, M, D), np.nan, np.float32)
    k1, s1, d1 = k0.copy(), s0.copy(), d0.copy()
    perms = []
    for b, (m, _) in enumerate(shapes):
        kp, sc, de = planted_inputs(rng, m, m, 0)[:3]
        perm = rng.permutation(m)                     # row i of image 0 is row perm[i] of image 1
        k0[b, :m], s0[b, :m], d0[b, :m] = kp, sc, de
        k1[b, perm], s1[b, perm], d1[b, perm] = kp, sc, de
        perms.append(perm)
    cnt = torch.tensor([s[0] for s in shapes], dtype=torch.int32).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (k0, s0, d0, k1, s1, d1)]
    worst = 0.0
    with Net.from_state_dict(ctx, random_weights(3, 2)) as net:
        md0, md1 = (t.cpu().numpy() for t in forward(ctx, net, *dev, m=cnt, n=cnt))
        r = match(ctx, net, *dev, m=cnt, n=cnt)
    m0, status = r["matches0"].cpu().numpy(), r["status"].cpu().numpy()
    for b, (m, _) in enumerate(shapes):
        assert np.isfinite(md0[b, :m]).all() and np.isnan(md0[b, m:]).all() and np.isnan(md1[b, m:]).all(), "padding written or a non-finite descriptor"
        dev_rel = float(np.abs(md1[b, perms[b]] - md0[b, :m]).max() / np.abs(md0[b, :m]).max())
        assert dev_rel <= 1e-4, "the network is not permutation equivariant: %.3g" % dev_rel
        assert status[b] == 0 and np.array_equal(m0[b, :m], perms[b]) and (m0[b, m:] == -1).all(), "a row is not matched to its image"
        worst = max(worst, dev_rel)
    return [s[0] for s in shapes], worst
