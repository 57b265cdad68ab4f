"""CPU references of SuperGlue's attentional graph network, written from the paper (Sarlin et al., CVPR
2020, section 3.1) and the authors' published forward: the reference project's tree holds only the call into a TorchScript file
it does not ship.

    forward         float64 numpy, BatchNorm in inference form as published: THE reference
    forward_folded  float64 numpy on plain linear layers (what the library is given): checks the folding
    forward_torch   the published forward transcribed to torch (conv1d, batch_norm, view(b, 64, 4, n), einsum, softmax) in a
                    chosen dtype: fp32 measures what an fp32 forward deviates, float64 checks the head interleave
    normalize       the reference's coordinate rule (integer centre)
    cases           the planted pairs the tests and the golden file share

One pair: m keypoints in image 0, n in image 1, D = 256, 4 heads of 64 channels; arrays are point-major [K][C].
"""
import functools

import numpy as np

from reconstructor_amd import superglue_gnn as G

D, HEADS, DEPTH = 256, 4, 64


def normalize(kpts, shape, rng=G.COORD_RANGE):
    """normalizeFeatCoords: cx = W / 2, cy = H / 2 in INTEGER division, scale = max(H, W) * range, k = (float)((x - c) / scale)
    in double.  (The published network centres at size / 2 in floating point; the reference's rule holds here.)"""
    H, W = int(shape[0]), int(shape[1])
    c = np.array([W // 2, H // 2], np.float64)
    return ((np.asarray(kpts, np.float32).astype(np.float64) - c) / (max(H, W) * np.float64(rng))).astype(np.float32)


def _p(sd, name):
    w = np.asarray(sd[name + ".weight"], np.float64)
    return w.reshape(w.shape[0], -1), np.asarray(sd[name + ".bias"], np.float64)


def _conv(sd, name, x):
    W, b = _p(sd, name)
    return x @ W.T + b


def _bn(sd, name, x):
    g, beta = np.asarray(sd[name + ".weight"], np.float64), np.asarray(sd[name + ".bias"], np.float64)
    mean, var = np.asarray(sd[name + ".running_mean"], np.float64), np.asarray(sd[name + ".running_var"], np.float64)
    return (x - mean) / np.sqrt(var + G.BN_EPS) * g + beta


def attention(q, k, v, probs=None):
    """q [K][256], k, v [Ks][256]: channel c is head c % 4 at depth c / 4.  Returns o [K][256] in the same channel order."""
    K, Ks = q.shape[0], k.shape[0]
    q, k, v = q.reshape(K, DEPTH, HEADS), k.reshape(Ks, DEPTH, HEADS), v.reshape(Ks, DEPTH, HEADS)
    s = np.einsum("idh,jdh->hij", q, k) / 8.0
    s = s - s.max(axis=2, keepdims=True)
    P = np.exp(s)
    P /= P.sum(axis=2, keepdims=True)
    if probs is not None:
        probs.append(P)
    return np.einsum("hij,jdh->idh", P, v).reshape(K, D)


def _encode(sd, kpts, scores, desc):
    x = np.concatenate([np.asarray(kpts, np.float64), np.asarray(scores, np.float64)[:, None]], axis=1)
    for i in range(5):
        x = _conv(sd, "kenc.encoder.%d" % (3 * i), x)
        if i < 4:
            x = np.maximum(_bn(sd, "kenc.encoder.%d" % (3 * i + 1), x), 0.0)
    return np.asarray(desc, np.float64) + x


def forward(sd, types, kpts0, scores0, d0, kpts1, scores1, d1, shapes=None, probs=None):
    """(mdesc0 [m][256], mdesc1 [n][256]) in float64.  shapes: ((H0, W0), (H1, W1)) or None (coordinates normalised already)."""
    if shapes is not None:
        kpts0, kpts1 = normalize(kpts0, shapes[0]), normalize(kpts1, shapes[1])
    x0, x1 = _encode(sd, kpts0, scores0, d0), _encode(sd, kpts1, scores1, d1)
    for l, t in enumerate(types):
        p = "gnn.layers.%d." % l
        s0, s1 = (x1, x0) if t == G.CROSS else (x0, x1)
        deltas = []
        for x, src in ((x0, s0), (x1, s1)):
            o = attention(_conv(sd, p + "attn.proj.0", x), _conv(sd, p + "attn.proj.1", src), _conv(sd, p + "attn.proj.2", src), probs)
            msg = _conv(sd, p + "attn.merge", o)
            h = np.maximum(_bn(sd, p + "mlp.1", _conv(sd, p + "mlp.0", np.concatenate([x, msg], axis=1))), 0.0)
            deltas.append(_conv(sd, p + "mlp.3", h))
        x0, x1 = x0 + deltas[0], x1 + deltas[1]
    return _conv(sd, "final_proj", x0), _conv(sd, "final_proj", x1)


def forward_folded(layers, types, kpts0, scores0, d0, kpts1, scores1, d1):
    """The same forward on the plain linear layers [(W, b)] of superglue_gnn.fold_layers (any float dtype, computed in float64)."""
    lay = [(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in layers]
    lin = lambda i, x: x @ lay[i][0].T + lay[i][1]

    def enc(kpts, scores, desc):
        x = np.concatenate([np.asarray(kpts, np.float64), np.asarray(scores, np.float64)[:, None]], axis=1)
        for i in range(5):
            x = lin(i, x)
            if i < 4:
                x = np.maximum(x, 0.0)
        return np.asarray(desc, np.float64) + x

    x0, x1 = enc(kpts0, scores0, d0), enc(kpts1, scores1, d1)
    for l, t in enumerate(types):
        i = 5 + 6 * l
        s0, s1 = (x1, x0) if t == G.CROSS else (x0, x1)
        deltas = []
        for x, src in ((x0, s0), (x1, s1)):
            msg = lin(i + 3, attention(lin(i, x), lin(i + 1, src), lin(i + 2, src)))
            deltas.append(lin(i + 5, np.maximum(lin(i + 4, np.concatenate([x, msg], axis=1)), 0.0)))
        x0, x1 = x0 + deltas[0], x1 + deltas[1]
    j = 5 + 6 * len(types)
    return lin(j, x0), lin(j, x1)


def forward_torch(sd, types, kpts0, scores0, d0, kpts1, scores1, d1, dtype):
    """The published forward, channel-first [1][C][K], unfolded BatchNorm in eval mode, heads by view(b, 64, 4, n)."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.as_tensor(np.array(a)).to(dtype)
    conv = lambda name, x: F.conv1d(x, t(sd[name + ".weight"]).reshape(sd[name + ".weight"].shape[0], -1, 1), t(sd[name + ".bias"]))
    bn = lambda name, x: F.batch_norm(x, t(sd[name + ".running_mean"]), t(sd[name + ".running_var"]), t(sd[name + ".weight"]), t(sd[name + ".bias"]),
                                      False, 0.0, G.BN_EPS)

    def enc(kpts, scores, desc):
        x = torch.cat([t(kpts).T[None], t(scores)[None, None]], dim=1)
        for i in range(5):
            x = conv("kenc.encoder.%d" % (3 * i), x)
            if i < 4:
                x = F.relu(bn("kenc.encoder.%d" % (3 * i + 1), x))
        return t(desc).T[None] + x

    def attn(p, x, src):
        q, k, v = (conv(p + "attn.proj.%d" % i, a).view(1, DEPTH, HEADS, -1) for i, a in enumerate((x, src, src)))
        prob = torch.softmax(torch.einsum("bdhn,bdhm->bhnm", q, k) / DEPTH ** 0.5, dim=-1)
        return conv(p + "attn.merge", torch.einsum("bhnm,bdhm->bdhn", prob, v).contiguous().view(1, D, -1))

    with torch.no_grad():
        x0, x1 = enc(kpts0, scores0, d0), enc(kpts1, scores1, d1)
        for l, ty in enumerate(types):
            p = "gnn.layers.%d." % l
            s0, s1 = (x1, x0) if ty == G.CROSS else (x0, x1)
            deltas = [conv(p + "mlp.3", F.relu(bn(p + "mlp.1", conv(p + "mlp.0", torch.cat([x, attn(p, x, s)], dim=1))))) for x, s in ((x0, s0), (x1, s1))]
            x0, x1 = x0 + deltas[0], x1 + deltas[1]
        return tuple(conv("final_proj", x)[0].T.contiguous().numpy() for x in (x0, x1))


def scores(md0, md1):
    """The score matrix the optimal-matching layer takes: mdesc0 . mdesc1 / sqrt(256)."""
    return np.asarray(md0, np.float64) @ np.asarray(md1, np.float64).T / 16.0


# ---- the cases the CPU test, the GPU test and the golden file share ---------------------------------------------------------

SHAPES = [(1, 1), (1, 5), (7, 3), (33, 47), (64, 64), (65, 130), (5, 300), (300, 5), (200, 257)]
RAGGED = [(200, 257), (0, 40), (33, 47), (272, 272)]          # one batch in capacity 272
WEIGHT_SEED = 2020
TYPES2 = [G.SELF, G.CROSS]
TYPES18 = [G.SELF, G.CROSS] * 9


@functools.lru_cache(maxsize=None)
def weights(L):
    """The seeded state dict of L layers (the L-layer net is not a prefix of a longer one: each has its own draw)."""
    sd = G.random_weights(WEIGHT_SEED + L, L)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def case_seed(m, n):
    return 7000 * m + n


@functools.lru_cache(maxsize=None)
def inputs(m, n):
    """(kpts0, scores0, d0, kpts1, scores1, d1, target) of the planted pair (m, n): 60 % of the smaller side planted."""
    out = G.planted_inputs(np.random.default_rng(case_seed(m, n)), m, n, int(round(0.6 * min(m, n))))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(m, n, L=2):
    """(inputs, (mdesc0, mdesc1) in float64) of the planted pair under the seeded L-layer net (self, cross, ...)."""
    inp = inputs(m, n)
    md = forward(weights(L), [G.SELF, G.CROSS] * (L // 2), *inp[:6])
    for a in md:
        a.setflags(write=False)
    return inp, md
