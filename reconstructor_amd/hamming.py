"""Host mirror of the Hamming matcher for ORB's packed rows (cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) behind the ratio test and
the uniqueness loop of FeatureMatcher.cpp:53-64) over librcn.so (no CPU fallback).

    upload                rcn_bits_upload: uint8 [K][32] from the host as one resident image
    upload_batch_device   rcn_bits_upload_batch_device: a CUDA tensor [n][K][32] and, optionally, ORB's own counts [n], left on the device
    remove / clear / count
    match_pair            rcn_match_pair_hamming: one pair straight from host rows
    match_grid            rcn_match_grid_hamming: the dense table and counts of a pair list (None: every i < j) on the host
    match_grid_device     rcn_match_grid_hamming_device: the same as CUDA tensors (asynchronous on the ctx stream)
    knn2                  rcn_hamming_knn2_device: (j0, d0, j1, d1) per query row, -1 where absent

The binary rows are a residency of their own: the float descriptors of rcn_desc_* are not touched.  Nothing here computes a distance
for a caller; smoke() alone restates the contract in numpy to check the grid it ran.
"""
import ctypes as C

import numpy as np

from . import _lib

RATIO_THRESH = np.float32(0.7)  # FeatureMatcher.h:45
N_BYTES = 32
MAX_K = 32768


def _rows(x):
    x = np.ascontiguousarray(x)
    if x.dtype != np.uint8 or x.ndim != 2:
        raise ValueError("hamming: rows are uint8 [K][n_bytes]")
    return x


def _pairs(pairs, n_pairs):
    if pairs is None:
        return None, int(n_pairs)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    return pairs, len(pairs)


def upload(ctx, img_id, rows):
    rows = _rows(rows)
    ctx.check(ctx.lib.rcn_bits_upload(ctx.h, int(img_id), rows.ctypes.data if len(rows) else None, len(rows), rows.shape[1]))


def upload_batch_device(ctx, first_id, bytes_dev, counts_dev=None):
    """bytes_dev: uint8 CUDA tensor [n][K][32] (bytes_out_dev of the ORB stage); counts_dev: int32 CUDA tensor [n] or None (K rows each).
    The rows are copied on the ctx stream; the tensors must stay alive until that stream has passed the call."""
    import torch
    if not bytes_dev.is_cuda or bytes_dev.dtype != torch.uint8 or bytes_dev.dim() != 3 or not bytes_dev.is_contiguous():
        raise ValueError("hamming: bytes_dev must be a contiguous uint8 CUDA tensor [n][K][n_bytes]")
    n, K, nb = bytes_dev.shape
    if counts_dev is not None and (not counts_dev.is_cuda or counts_dev.dtype != torch.int32 or counts_dev.numel() != n or not counts_dev.is_contiguous()):
        raise ValueError("hamming: counts_dev must be a contiguous int32 CUDA tensor [n]")
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_bits_upload_batch_device(ctx.h, int(first_id), n, C.c_void_p(bytes_dev.data_ptr()),
                                                   C.c_void_p(counts_dev.data_ptr()) if counts_dev is not None else None, K, nb))


def remove(ctx, img_id):
    ctx.check(ctx.lib.rcn_bits_remove(ctx.h, int(img_id)))


def clear(ctx):
    ctx.check(ctx.lib.rcn_bits_clear(ctx.h))


def count(ctx):
    return int(ctx.lib.rcn_bits_count(ctx.h))


def set_workspace_rows(ctx, rows=0):
    """Query-row slots of the top-2 workspace per chunk of pairs (rcn_match_set_workspace_rows; 0: the library's default)."""
    ctx.lib.rcn_match_set_workspace_rows.restype = C.c_int
    ctx.lib.rcn_match_set_workspace_rows.argtypes = [C.c_void_p, C.c_int64]
    ctx.check(ctx.lib.rcn_match_set_workspace_rows(ctx.h, int(rows)))


def match_pair(ctx, q, t, ratio=RATIO_THRESH):
    """Dense result: out[i] = train row matched to query row i, or -1."""
    q, t = _rows(q), _rows(t)
    K1, K2 = len(q), len(t)
    out = np.full(K1, -1, np.int32)
    cnt = C.c_int32(0)
    ctx.check(ctx.lib.rcn_match_pair_hamming(ctx.h, q.ctypes.data if K1 else None, K1, t.ctypes.data if K2 else None, K2,
                                             q.shape[1], float(np.float32(ratio)), out.ctypes.data if K1 else None, C.byref(cnt)))
    assert cnt.value == int((out >= 0).sum())
    return out


def match_grid(ctx, pairs, out_stride, ratio=RATIO_THRESH, n_pairs=0):
    """pairs: (P, 2) (query image id, train image id), or None with n_pairs = n (n - 1) / 2 for every i < j over the resident binary
    ids.  Returns (out [P][out_stride], counts [P]) on the host."""
    pairs, P = _pairs(pairs, n_pairs)
    out = np.full((max(P, 1), max(1, int(out_stride))), -1, np.int32)
    counts = np.zeros(max(P, 1), np.int32)
    ctx.check(ctx.lib.rcn_match_grid_hamming(ctx.h, pairs.ctypes.data if pairs is not None and P else None, P, float(np.float32(ratio)),
                                             out.ctypes.data, out.shape[1], counts.ctypes.data))
    return out[:P], counts[:P]


def match_grid_device(ctx, pairs, out_stride, ratio=RATIO_THRESH, n_pairs=0, out=None, counts=None):
    """The same, left in HBM: returns CUDA tensors (out [P][out_stride], counts [P]); asynchronous on the ctx stream."""
    import torch
    pairs, P = _pairs(pairs, n_pairs)
    dev = torch.device("cuda", ctx.device)
    if out is None:
        out = torch.empty((max(P, 1), max(1, int(out_stride))), dtype=torch.int32, device=dev)
    if counts is None:
        counts = torch.empty((max(P, 1),), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_match_grid_hamming_device(ctx.h, pairs.ctypes.data if pairs is not None and P else None, P, float(np.float32(ratio)),
                                                    C.c_void_p(out.data_ptr()), out.shape[1], C.c_void_p(counts.data_ptr())))
    return out[:P], counts[:P]


def knn2(ctx, pairs, stride, n_pairs=0):
    """int32 [P][stride][4] = (j0, d0, j1, d1) on the host."""
    import torch
    pairs, P = _pairs(pairs, n_pairs)
    knn = torch.empty((max(P, 1), max(1, int(stride)), 4), dtype=torch.int32, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_hamming_knn2_device(ctx.h, pairs.ctypes.data if pairs is not None and P else None, P, C.c_void_p(knn.data_ptr()), knn.shape[1]))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return knn[:P].cpu().numpy()


def _popcount_grid(images, pairs, ratio, stride):
    """The contract on copied bytes, for smoke(): popcount of XOR, (d, j) order, fp32 ratio test, lowest query keeps a train row."""
    pop = np.array([bin(v).count("1") for v in range(256)], np.int32)
    table = np.full((len(pairs), stride), -1, np.int32)
    for p, (a, b) in enumerate(pairs):
        q, t = images[a], images[b]
        if len(q) == 0 or len(t) < 2:
            continue
        d = pop[q[:, None, :] ^ t[None, :, :]].sum(axis=2, dtype=np.int32)
        order = np.argsort(d, axis=1, kind="stable")[:, :2]
        i = np.arange(len(q))
        d0, d1 = d[i, order[:, 0]], d[i, order[:, 1]]
        taken = set()
        for k in np.nonzero(d0.astype(np.float32) < np.float32(ratio) * d1.astype(np.float32))[0]:
            if int(order[k, 0]) not in taken:
                taken.add(int(order[k, 0]))
                table[p, k] = order[k, 0]
    return table


def smoke(ctx):
    """Three synthetic images through the ORB stage with the packed bytes kept on the device, into the binary residency with ORB's
    own counts, the all-pairs grid; checked against a numpy popcount on the copied bytes.  Returns (rows per image, matches)."""
    import torch
    from . import orb
    H, W, K = 128, 128, 384
    rng = np.random.default_rng(12)
    img = np.full((H, W), 120, np.int32)
    for _ in range(60):
        x, y, a, b = int(rng.integers(0, W - 8)), int(rng.integers(0, H - 8)), int(rng.integers(6, 40)), int(rng.integers(6, 40))
        img[y:y + b, x:x + a] = int(rng.integers(20, 236))
    ims = np.stack([(img + rng.integers(-4, 5, (H, W))).clip(0, 255).astype(np.uint8) for _ in range(3)])      # one scene, three noise draws
    r = orb.detect_and_compute(ctx, torch.from_numpy(ims).cuda(), K)
    clear(ctx)
    upload_batch_device(ctx, 0, r["packed"], r["counts"])
    out, counts = match_grid(ctx, None, K, n_pairs=3)
    by, cn = r["packed"].cpu().numpy(), r["counts"].cpu().numpy()
    rows = [min(max(int(c), 0), K) for c in cn]
    assert min(rows) >= 2, "Hamming smoke: ORB found no keypoints"
    want = _popcount_grid({i: by[i, :rows[i]] for i in range(3)}, [(0, 1), (0, 2), (1, 2)], RATIO_THRESH, K)
    assert np.array_equal(out, want) and np.array_equal(counts, (want >= 0).sum(axis=1)), "Hamming grid differs from the popcount on the copied bytes"
    assert counts.sum() > 0
    clear(ctx)
    return rows, int(counts.sum())
