"""Host mirror of the retrieval ImageMatcher (ImageMatcher.h:14-33; rcn_retr_* of include/rcn.h) over librcn.so (no CPU fallback;
DESIGN.md section 24): which image pairs are matched at all, from the local descriptors already in HBM.

    train_codebook   Lloyd's k-means on the call's own rows -> Codebook
    Codebook         a trained or supplied set of centroids (centroids(), close())
    assign           rows -> nearest centroid
    encode           descriptors [n][K][D] -> VLAD global descriptors [n][C * D]
    similarity       global descriptors -> fp64 [n][n]
    top_k            similarities -> neighbour slots [n][min(k, n - 1)]
    pairs            neighbour table -> the ascending symmetric pair list (a numpy array, as matcher.match_grid takes it)
    image_pairs      encode .. pairs in one call

Descriptors are float32 CUDA tensors [n][K][D] in the matcher's device layout; counts an int32 CUDA tensor [n] or None (K each).
"""
import ctypes as C

import numpy as np

from . import _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _desc(desc, counts):
    import torch
    if not desc.is_cuda or desc.dtype != torch.float32 or desc.dim() != 3 or not desc.is_contiguous():
        raise ValueError("retrieval: descriptors must be a contiguous float32 CUDA tensor [n][K][D]")
    if counts is not None and (not counts.is_cuda or counts.dtype != torch.int32 or counts.shape != (desc.shape[0],) or not counts.is_contiguous()):
        raise ValueError("retrieval: counts must be a contiguous int32 CUDA tensor [n]")
    return desc.shape


class Codebook:
    """rcn_retr_codebook: C centroids of length D in HBM, tied to its ctx."""

    def __init__(self, ctx, centroids=None, _handle=None):
        self.ctx = ctx
        self.h = _handle
        if _handle is None:
            cen = np.ascontiguousarray(centroids, np.float32)
            if cen.ndim != 2:
                raise ValueError("retrieval.Codebook: centroids must be [C][D]")
            h = C.c_void_p()
            ctx.check(ctx.lib.rcn_retr_codebook_create(ctx.h, cen.ctypes.data, cen.shape[0], cen.shape[1], C.byref(h)))
            self.h = h
        c, d = C.c_int32(), C.c_int32()
        ctx.check(ctx.lib.rcn_retr_codebook_read(self.h, None, C.byref(c), C.byref(d)))
        self.C, self.D = c.value, d.value

    def centroids(self):
        out = np.empty((self.C, self.D), np.float32)
        self.ctx.check(self.ctx.lib.rcn_retr_codebook_read(self.h, out.ctypes.data, None, None))
        return out

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.rcn_retr_codebook_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def options(n_centroids=None, iterations=None, train_row_stride=None, top_k=None):
    o = _lib.RetrOptions()
    _lib.load().rcn_retr_default_options(C.byref(o))
    for name, v in (("n_centroids", n_centroids), ("iterations", iterations), ("train_row_stride", train_row_stride), ("top_k", top_k)):
        if v is not None:
            setattr(o, name, int(v))
    return o


def train_codebook(ctx, desc, counts=None, n_centroids=64, iterations=10, train_row_stride=0):
    """rcn_retr_codebook_train_device -> Codebook"""
    import torch
    n, K, D = _desc(desc, counts)
    o = options(n_centroids, iterations, train_row_stride)
    h = C.c_void_p()
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_retr_codebook_train_device(ctx.h, _ptr(desc), _ptr(counts), n, K, D, C.byref(o), C.byref(h)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return Codebook(ctx, _handle=h)


def assign(ctx, cb, rows):
    """rows: float32 CUDA tensor [R][D] -> int32 CUDA tensor [R]"""
    import torch
    if not rows.is_cuda or rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != cb.D or not rows.is_contiguous():
        raise ValueError("retrieval.assign: rows must be a contiguous float32 CUDA tensor [R][D of the codebook]")
    out = torch.empty((rows.shape[0],), dtype=torch.int32, device=rows.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_retr_assign_device(ctx.h, cb.h, _ptr(rows), rows.shape[0], _ptr(out)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return out


def encode(ctx, cb, desc, counts=None):
    """-> float32 CUDA tensor [n][C * D]"""
    import torch
    n, K, D = _desc(desc, counts)
    G = torch.empty((n, cb.C * cb.D), dtype=torch.float32, device=desc.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_retr_encode_device(ctx.h, cb.h, _ptr(desc), _ptr(counts), n, K, D, _ptr(G)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return G


def similarity(ctx, G, D):
    """G: float32 CUDA tensor [n][L], D the codebook's D -> float64 CUDA tensor [n][n]"""
    import torch
    if not G.is_cuda or G.dtype != torch.float32 or G.dim() != 2 or not G.is_contiguous():
        raise ValueError("retrieval.similarity: G must be a contiguous float32 CUDA tensor [n][L]")
    n, L = G.shape
    sim = torch.empty((n, n), dtype=torch.float64, device=G.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_retr_similarity_device(ctx.h, _ptr(G), n, L, int(D), _ptr(sim)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return sim


def top_k(ctx, sim, k):
    """-> int32 CUDA tensor [n][min(k, n - 1)] of slots"""
    import torch
    if not sim.is_cuda or sim.dtype != torch.float64 or sim.dim() != 2 or sim.shape[0] != sim.shape[1] or not sim.is_contiguous():
        raise ValueError("retrieval.top_k: sim must be a contiguous float64 CUDA tensor [n][n]")
    n = sim.shape[0]
    nbr = torch.empty((n, max(min(int(k), n - 1), 0)), dtype=torch.int32, device=sim.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_retr_topk_device(ctx.h, _ptr(sim), n, int(k), _ptr(nbr)))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return nbr


def pairs(ctx, nbr, k, first_img_id=0, capacity=None):
    """nbr: what top_k returned for this k -> numpy int32 [P][2]; capacity: pairs the device buffer holds (None: enough)"""
    import torch
    n = nbr.shape[0]
    kk = max(min(int(k), n - 1), 0)
    if not nbr.is_cuda or nbr.dtype != torch.int32 or nbr.shape != (n, kk) or not nbr.is_contiguous():
        raise ValueError("retrieval.pairs: nbr must be a contiguous int32 CUDA tensor [n][min(k, n - 1)]")
    cap = min(n * kk, n * (n - 1) // 2) if capacity is None else int(capacity)
    buf = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=nbr.device)
    cnt = torch.zeros((1,), dtype=torch.int32, device=nbr.device)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_retr_pairs_device(ctx.h, _ptr(nbr), n, int(k), int(first_img_id), _ptr(buf), cap, _ptr(cnt)))
    return buf[:int(cnt.item())].cpu().numpy()


def image_pairs(ctx, cb, desc, counts=None, top_k=20, first_img_id=0, capacity=None):
    """rcn_retr_image_pairs -> numpy int32 [P][2], the list matcher.match_grid takes"""
    import torch
    n, K, D = _desc(desc, counts)
    kk = max(min(int(top_k), n - 1), 0)
    cap = min(n * kk, n * (n - 1) // 2) if capacity is None else int(capacity)
    out = np.zeros((max(cap, 1), 2), np.int32)
    cnt = C.c_int32(0)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_retr_image_pairs(ctx.h, cb.h, _ptr(desc), _ptr(counts), n, K, D, int(first_img_id), int(top_k), out.ctypes.data, cap, C.byref(cnt)))
    return out[:cnt.value].copy()


def ring_scene(n, K, D, step, noise, seed):
    """float32 [n][K][D]: image i sees rows (i * step + 0 .. K - 1) of a ring of n * step unit world rows, in a random order, each with
    N(0, noise^2) added and renormalised: images overlap iff their ring distance times step is below K."""
    rng = np.random.default_rng(seed)
    pool = rng.standard_normal((n * step, D))
    pool /= np.linalg.norm(pool, axis=1, keepdims=True)
    out = np.zeros((n, K, D), np.float32)
    for i in range(n):
        idx = (i * step + np.arange(K)) % (n * step)
        rows = pool[rng.permutation(idx)] + noise * rng.standard_normal((K, D))
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        out[i] = rows.astype(np.float32)
    return out


def smoke(ctx):
    """A ring scene of 16 images: the retrieved pairs are overlapping ones and hold every immediate neighbour, and the matcher run
    on the list equals its own rows of the full grid.  Returns (pairs retrieved, pairs of the full grid, matches kept, matches of the grid)."""
    import torch
    from .matcher import HipL2Matcher, all_pairs
    n, K, D, step, k = 16, 64, 32, 16, 4
    scene = ring_scene(n, K, D, step, 0.05, 7)
    dev = torch.from_numpy(scene).cuda()
    cb = train_codebook(ctx, dev, None, n_centroids=8, iterations=5)
    got = image_pairs(ctx, cb, dev, None, top_k=k)
    staged = pairs(ctx, top_k(ctx, similarity(ctx, encode(ctx, cb, dev), D), k), k)
    cb.close()
    assert np.array_equal(got, staged), "retrieval: the one call differs from the staged calls"
    ring = lambda a, b: min((a - b) % n, (b - a) % n)      # noqa: E731
    have = {tuple(p) for p in got.tolist()}
    assert all(ring(a, b) * step < K for a, b in have), "retrieval: a retrieved pair does not overlap"
    assert all((min(i, (i + 1) % n), max(i, (i + 1) % n)) in have for i in range(n)), "retrieval: an immediate neighbour is missing"
    m = HipL2Matcher(ctx=ctx)
    m.clear()
    m.upload_batch_device(0, n, dev.data_ptr(), K, D)
    grid = all_pairs(n)
    full, fc = m.match_grid(grid, K)
    part, pc = m.match_grid(got, K)
    m.clear()
    rows = [int(np.flatnonzero((grid == p).all(1))[0]) for p in got]
    assert np.array_equal(part, full[rows]) and np.array_equal(pc, fc[rows]), "retrieval: the matcher on the list differs from the full grid"
    return len(got), len(grid), int(pc.sum()), int(fc.sum())
