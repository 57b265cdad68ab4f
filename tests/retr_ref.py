"""The retrieval ImageMatcher restated in numpy: the contract of reconstructor_amd/csrc/retrieval.hip.

The reference has nothing here (FakeImgMatcher, ImageMatcher.cpp:6-23, pairs every image with every other), so this file is the
definition.  All arithmetic is fp64 on fp32 inputs widened to double; numpy rounds every product before it adds, and every sum
below is written as a loop so that its order is the stated one (ascending k, row, image, d, c).  Vectors run across rows or
images only, which fixes no order.

    assign          nearest centroid by squared distance, ties to the lowest index
    segment_sums    per centroid the sum of an image's rows assigned to it, and their number
    training_rows   rows r % s == 0, r < counts[i]
    train           init at evenly spaced training rows, then Lloyd steps; returns the centroids after every step
    encode          VLAD with signed root and L2 norm, float32 [n][C * D]
    similarity      two-level dot products, fp64 [n][n]
    top_k, pairs    neighbours by (similarity descending, index ascending); the symmetric ascending pair list
    ring_scene      n images that see consecutive windows of a ring of world points
"""
import numpy as np

F64 = np.float64


def _counts(counts, n, K):
    if counts is None:
        return np.full(n, K, np.int64)
    return np.clip(np.asarray(counts, np.int64), 0, K)


def assign(x, mu):
    """x [R][D], mu [C][D] float32 -> int32 [R]"""
    x = np.asarray(x, np.float32).astype(F64)
    mu = np.asarray(mu, np.float32).astype(F64)
    R, D = x.shape
    best = np.full(R, np.inf)
    arg = np.zeros(R, np.int32)
    for c in range(mu.shape[0]):
        acc = np.zeros(R)
        for k in range(D):
            d = x[:, k] - mu[c, k]
            acc = acc + d * d
        upd = acc < best                        # strict: the lowest index keeps a tie
        best[upd] = acc[upd]
        arg[upd] = c
    return arg


def segment_sums(x, a, C):
    """x [R][D] float32 (the rows taken, in ascending order), a [R] -> (S [C][D] fp64, n [C] int64)"""
    x = np.asarray(x, np.float32).astype(F64)
    S = np.zeros((C, x.shape[1]))
    cnt = np.zeros(C, np.int64)
    for r in range(x.shape[0]):
        S[a[r]] = S[a[r]] + x[r]
        cnt[a[r]] += 1
    return S, cnt


def auto_stride(n, K):
    s = 1
    while n * -(-K // s) > 2 ** 18:
        s += 1
    return s


def training_rows(counts, n, K, stride):
    """per image the training rows, ascending"""
    s = stride if stride else auto_stride(n, K)
    cn = _counts(counts, n, K)
    return [np.arange(0, cn[i], s) for i in range(n)]


def train(desc, counts, C, iterations, stride=0):
    """desc [n][K][D] float32.  Returns the list of centroid arrays [C][D] float32: after the initialisation, then after every
    Lloyd step (iterations + 1 entries).  ValueError when there are fewer training rows than centroids."""
    desc = np.asarray(desc, np.float32)
    n, K, D = desc.shape
    rows = training_rows(counts, n, K, stride)
    flat = [(i, int(r)) for i in range(n) for r in rows[i]]
    M = len(flat)
    if M < C:
        raise ValueError("fewer training rows than centroids")
    mu = np.stack([desc[flat[(c * M) // C]] for c in range(C)]).astype(np.float32)
    out = [mu.copy()]
    for _ in range(iterations):
        tot = np.zeros((C, D))
        num = np.zeros(C, np.int64)
        for i in range(n):                       # per image first, then over the images in ascending order
            x = desc[i][rows[i]]
            S, cnt = segment_sums(x, assign(x, mu), C)
            tot = tot + S
            num += cnt
        new = mu.copy()
        for c in range(C):
            if num[c] > 0:                       # an empty cluster keeps its centroid
                new[c] = (tot[c] / F64(num[c])).astype(np.float32)
        mu = new
        out.append(mu.copy())
    return out


def encode(desc, counts, mu):
    """-> G float32 [n][C * D]"""
    desc = np.asarray(desc, np.float32)
    mu = np.asarray(mu, np.float32)
    n, K, D = desc.shape
    C = mu.shape[0]
    cn = _counts(counts, n, K)
    G = np.zeros((n, C * D), np.float32)
    for i in range(n):
        x = desc[i, :cn[i]]
        S, cnt = segment_sums(x, assign(x, mu), C)
        V = S - cnt[:, None].astype(F64) * mu.astype(F64)         # the product rounded, then subtracted
        Vp = np.copysign(np.sqrt(np.abs(V)), V)
        b = np.zeros(C)
        for d in range(D):
            b = b + Vp[:, d] * Vp[:, d]
        tot = F64(0.0)
        for c in range(C):
            tot = tot + b[c]
        nrm = np.sqrt(tot)
        if nrm != 0.0:
            G[i] = (Vp / nrm).astype(np.float32).reshape(-1)
    return G


def similarity(G, D):
    """G float32 [n][C * D] -> fp64 [n][n]; blocks of D first, then the blocks"""
    G = np.asarray(G, np.float32).astype(F64)
    n, L = G.shape
    sim = np.zeros((n, n))
    for c in range(L // D):
        acc = np.zeros((n, n))
        for d in range(D):
            col = G[:, c * D + d]
            acc = acc + col[:, None] * col[None, :]
        sim = sim + acc
    return sim


def top_k(sim, k):
    """-> int32 [n][min(k, n - 1)]"""
    n = sim.shape[0]
    kk = max(min(k, n - 1), 0)
    out = np.zeros((n, kk), np.int32)
    for i in range(n):
        js = sorted((j for j in range(n) if j != i), key=lambda j: (-sim[i, j], j))
        out[i] = js[:kk]
    return out


def pairs(nbr, first_img_id=0):
    """-> int32 [P][2], ascending, no duplicates"""
    s = {(min(i, int(j)), max(i, int(j))) for i in range(nbr.shape[0]) for j in nbr[i]}
    return np.array(sorted(s), np.int32).reshape(-1, 2) + np.int32(first_img_id)


def image_pairs(desc, counts, mu, k, first_img_id=0):
    G = encode(desc, counts, mu)
    sim = similarity(G, np.asarray(desc).shape[2])
    return pairs(top_k(sim, k), first_img_id)


def ring_scene(n, K, D, step, noise, seed):
    """float32 [n][K][D]: a world pool of n * step unit rows; image i sees rows (i * step + 0 .. K - 1) mod pool in a random order,
    each with N(0, noise^2) added and renormalised.  Images i and j share rows iff their ring distance times step is below K."""
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


def ring_distance(i, j, n):
    d = abs(int(i) - int(j)) % n
    return min(d, n - d)
