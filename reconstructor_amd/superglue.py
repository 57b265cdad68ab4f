"""Host mirror of SuperGlue's optimal-matching layer over librcn.so (no CPU fallback).

    FeatureMatcherSuperglue::matchFeatures   FeatureMatcherSuperglue.cpp:51-101   what runs behind the graph network

Everything stays in HBM: `scores` takes the two sets of matching descriptors as torch tensors on the
GPU, [B][K][D] by default or the network's [B][D][K] with channel_first (any strides: both are read in place), `assign` a
score tensor [B][M][N] of any strides, `match` is the two in one call with the scores in the ctx's workspace.  The table is
the dense `out[i] = train row or -1` form of the L2 matcher: rcn_match_compact_begin takes it as it is.
"""
import ctypes as C

from . import _lib

PATH_AUTO, PATH_FUSED, PATH_BANDED = 0, 1, 2      # RCN_SG_PATH_*
LDS_BYTES = 131072                                # RCN_SG_LDS_BYTES: (m + 1)(n + 1) floats within it take the fused path
MAX_POINTS = 4096                                 # RCN_SG_MAX_POINTS


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def options(ctx, alpha=None, match_threshold=None, score_threshold=None, iterations=None, path=None):
    o = _lib.SgOptions()
    ctx.lib.rcn_sg_default_options(C.byref(o))
    for k, v in dict(alpha=alpha, match_threshold=match_threshold, score_threshold=score_threshold, iterations=iterations, path=path).items():
        if v is not None:
            setattr(o, k, v)
    return o


def set_chunk_bytes(ctx, nbytes):
    """rcn_sg_set_chunk_bytes: bytes of score matrices per chunk of pairs on the banded path (<= 0: no limit)."""
    ctx.check(ctx.lib.rcn_sg_set_chunk_bytes(ctx.h, int(nbytes)))


def _counts(t, B, name):
    import torch
    if t is not None and (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (B,)):
        raise ValueError("%s must be a contiguous int32 CUDA tensor of shape [B]" % name)
    return t


def _desc(d, channel_first, name):
    import torch
    if d.dtype != torch.float32 or not d.is_cuda or d.dim() != 3:
        raise ValueError("%s must be a float32 CUDA tensor of shape [B][K][D] ([B][D][K] with channel_first)" % name)
    return d.permute(0, 2, 1) if channel_first else d


def _outputs(B, M, N, table_stride, want_logp, device):
    import torch
    i32, f32 = torch.int32, torch.float32
    ts = M if table_stride is None else int(table_stride)
    return dict(matches0=torch.empty((B, M), dtype=i32, device=device), matches1=torch.empty((B, N), dtype=i32, device=device),
                mscores0=torch.empty((B, M), dtype=f32, device=device), mscores1=torch.empty((B, N), dtype=f32, device=device),
                table=torch.empty((B, ts), dtype=i32, device=device), counts=torch.empty((B,), dtype=i32, device=device),
                logP=torch.empty((B, M + 1, N + 1), dtype=f32, device=device) if want_logp else None,
                status=torch.empty((B,), dtype=i32, device=device))


def _out_args(o):
    return (_ptr(o["matches0"]), _ptr(o["matches1"]), _ptr(o["mscores0"]), _ptr(o["mscores1"]), _ptr(o["table"]), o["table"].shape[1],
            _ptr(o["counts"]), _ptr(o["logP"]), _ptr(o["status"]))


def scores(ctx, d0, d1, m=None, n=None, channel_first=False):
    """rcn_sg_scores_device.  d0 [B][M][D], d1 [B][N][D] float32 CUDA tensors of any strides ([B][D][M] / [B][D][N] with
    channel_first); m / n: int32 CUDA tensors [B] or None.  Returns S [B][M][N]; entries past a pair's counts are not written
    (the tensor is filled with NaN first, so that nothing downstream can use them unnoticed)."""
    import torch
    a, b = _desc(d0, channel_first, "d0"), _desc(d1, channel_first, "d1")
    B, M, D = a.shape
    N = b.shape[1]
    if b.shape[0] != B or b.shape[2] != D:
        raise ValueError("scores: d0 and d1 disagree on B or D")
    S = torch.full((B, M, N), float("nan"), dtype=torch.float32, device=a.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_sg_scores_device(ctx.h, _ptr(a), *a.stride(), _ptr(b), *b.stride(), _ptr(_counts(m, B, "m")), _ptr(_counts(n, B, "n")),
                                           B, M, N, D, _ptr(S)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return S


def assign(ctx, S, m=None, n=None, opt=None, table_stride=None, want_logp=False):
    """rcn_sg_assign_device.  S: float32 CUDA tensor [B][M][N], any strides.  Returns a dict of CUDA tensors: matches0 [B][M],
    matches1 [B][N], mscores0, mscores1, table [B][table_stride], counts [B], status [B], logP [B][M + 1][N + 1] or None."""
    import torch
    if S.dtype != torch.float32 or not S.is_cuda or S.dim() != 3:
        raise ValueError("assign: S must be a float32 CUDA tensor of shape [B][M][N]")
    B, M, N = S.shape
    o = _outputs(B, M, N, table_stride, want_logp, S.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_sg_assign_device(ctx.h, _ptr(S), *S.stride(), _ptr(_counts(m, B, "m")), _ptr(_counts(n, B, "n")), B, M, N,
                                           C.byref(opt) if opt is not None else None, *_out_args(o)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return o


def match(ctx, d0, d1, m=None, n=None, opt=None, channel_first=False, table_stride=None, want_logp=False):
    """rcn_sg_match_device: `scores` into the ctx's workspace, then `assign`; descriptors as for `scores`, result as `assign`."""
    import torch
    a, b = _desc(d0, channel_first, "d0"), _desc(d1, channel_first, "d1")
    B, M, D = a.shape
    N = b.shape[1]
    if b.shape[0] != B or b.shape[2] != D:
        raise ValueError("match: d0 and d1 disagree on B or D")
    o = _outputs(B, M, N, table_stride, want_logp, a.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_sg_match_device(ctx.h, _ptr(a), *a.stride(), _ptr(b), *b.stride(), _ptr(_counts(m, B, "m")), _ptr(_counts(n, B, "n")),
                                          B, M, N, D, C.byref(opt) if opt is not None else None, *_out_args(o)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return o


def planted_pair(rng, m, n, n_planted, D=256, noise=0.05, gain=None):
    """Descriptors of a synthetic pair: unit rows, the first n_planted rows of image 0 reappear (perturbed by noise of `noise` times their
    norm) at random rows of image 1.  `gain` scales both sets (the graph network's output is not unit norm: its scores span
    tens); default sqrt(12 sqrt(D)): a planted score near 12.  Returns (d0 [m][D], d1 [n][D], target [m], -1 = none)."""
    import numpy as np
    d0 = rng.standard_normal((m, D))
    d1 = rng.standard_normal((n, D))
    target = np.full(m, -1, np.int64)
    k = min(n_planted, m, n)
    cols = rng.permutation(n)[:k]
    d1[cols] = d0[:k] + noise * np.linalg.norm(d0[:k], axis=1, keepdims=True) * rng.standard_normal((k, D)) / np.sqrt(D)
    target[:k] = cols
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    g = np.sqrt(12.0 * np.sqrt(D)) if gain is None else gain
    return (g * d0).astype(np.float32), (g * d1).astype(np.float32), target


def smoke(ctx):
    """Two small planted pairs, one per device path, in one ragged batch with NaN padding: the planted matches come back, the
    matches are mutual, the padding is untouched.  Returns (matches per pair, planted per pair)."""
    import numpy as np
    import torch
    rng = np.random.default_rng(5)
    M, N, D = 224, 240, 256
    shapes, planted = [(60, 75), (224, 240)], [40, 150]         # (61)(76) floats fit the LDS budget: fused; the other is banded
    d0 = np.full((2, M, D), np.nan, np.float32)
    d1 = np.full((2, N, D), np.nan, np.float32)
    targets = []
    for b, ((m, n), k) in enumerate(zip(shapes, planted)):
        a, c, t = planted_pair(rng, m, n, k)
        d0[b, :m], d1[b, :n] = a, c
        targets.append(t)
    mm = torch.tensor([s[0] for s in shapes], dtype=torch.int32).cuda()
    nn = torch.tensor([s[1] for s in shapes], dtype=torch.int32).cuda()
    r = match(ctx, torch.from_numpy(d0).cuda(), torch.from_numpy(d1).cuda(), mm, nn)
    m0, m1, table, counts, status = (r[k].cpu().numpy() for k in ("matches0", "matches1", "table", "counts", "status"))
    s0 = r["mscores0"].cpu().numpy()
    found = []
    for b, (m, n) in enumerate(shapes):
        t = targets[b]
        assert status[b] == 0
        assert (m0[b, m:] == -1).all() and (m1[b, n:] == -1).all() and (s0[b, m:] == 0).all() and (table[b, m:] == -1).all(), "padding touched"
        rows = np.nonzero(m0[b, :m] >= 0)[0]
        assert (m1[b, m0[b, rows]] == rows).all(), "a match that is not mutual"
        kept = np.nonzero(table[b] >= 0)[0]
        assert counts[b] == len(kept) and (s0[b, kept] > 0.5).all() and np.array_equal(table[b, kept], m0[b, kept])
        hit = int((table[b, :m][t >= 0] == t[t >= 0]).sum())
        assert hit >= 0.9 * planted[b], "planted matches not recovered: %d of %d" % (hit, planted[b])
        assert (table[b, :m][t < 0] == -1).sum() >= 0.9 * (t < 0).sum(), "noise rows matched"
        found.append(hit)
    return found, planted
