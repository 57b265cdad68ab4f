"""The contract of guided matching in numpy, and the cases its tests share.

Band: csrc/guided_band.h operation by operation (numpy's element-wise fp64 products and sums are single operations, never fused).
Neighbours: among a query row's candidates only, the canonical squared distance (the oracle's fp64 fma chain, orc.knn2 on the candidate
rows) in ascending (d2, train row) order.  Acceptance, uniqueness and cross-check as the issue states them; see match_pair."""
import numpy as np

from oracle import orc

RECT_F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float64)        # rectified pair: the band is |y1 - y2| <= max_error_px
DBL_MAX = np.finfo(np.float64).max
EDGES = [(7, 10), (14, 20), (70, 100)]       # float32(d0) < float32(0.7) * float32(d1) is false for all three (hamming_ref.EDGES)


def thr2_of(max_error_px):
    e = np.float64(np.float32(max_error_px))
    return e * e


def _xy(xy):
    return np.ascontiguousarray(xy, np.int32).reshape(-1, 2).astype(np.float64)


def band(F, xy1, xy2, max_error_px=3.0):
    """bool [K1][K2]: train row t is a candidate of query row q."""
    F = np.asarray(F, np.float64).reshape(9)
    p1, p2 = _xy(xy1), _xy(xy2)
    x1, y1 = p1[:, 0][:, None], p1[:, 1][:, None]
    x2, y2 = p2[:, 0][None, :], p2[:, 1][None, :]
    thr2 = thr2_of(max_error_px)
    with np.errstate(all="ignore"):
        a = F[0] * x1 + F[1] * y1 + F[2]
        b = F[3] * x1 + F[4] * y1 + F[5]
        c = F[6] * x1 + F[7] * y1 + F[8]
        q2 = a * a + b * b
        d2 = x2 * a + y2 * b + c
        t2 = d2 * d2
        a_ = F[0] * x2 + F[3] * y2 + F[6]
        b_ = F[1] * x2 + F[4] * y2 + F[7]
        c_ = F[2] * x2 + F[5] * y2 + F[8]
        q1 = a_ * a_ + b_ * b_
        d1 = x1 * a_ + y1 * b_ + c_
        t1 = d1 * d1
        m = (q1 > 0) & (q2 > 0) & (q1 < DBL_MAX) & (q2 < DBL_MAX) & (t1 <= thr2 * q1) & (t2 <= thr2 * q2)
    return np.broadcast_to(m, (len(p1), len(p2))).copy()


def knn2(q, t, mask):
    """idx [K1][4] = (j0, j1, candidates, 0), -1 where absent; d2 [K1][2], +inf where absent."""
    q, t = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)
    K1 = len(q)
    idx = np.full((K1, 4), -1, np.int32)
    idx[:, 2:] = 0
    d2 = np.full((K1, 2), np.inf, np.float64)
    for i in range(K1):
        c = np.nonzero(mask[i])[0]
        idx[i, 2] = len(c)
        if len(c) == 0:
            continue
        j, d = orc.knn2(q[i:i + 1], t[c])          # ascending (d2, position): the positions ascend with the train rows
        for k in range(2):
            if j[0, k] >= 0:
                idx[i, k] = c[j[0, k]]
                d2[i, k] = d[0, k]
    return idx, d2


def raw(idx, d2, ratio=0.7, max_distance=0.0):
    """One-way acceptance: train row or -1 per query row."""
    with np.errstate(all="ignore"):
        dist0 = np.sqrt(d2[:, 0].astype(np.float32))
        dist1 = np.sqrt(d2[:, 1].astype(np.float32))            # +inf for a lone candidate
        ok = (idx[:, 0] >= 0) & (dist0 < np.float32(ratio) * dist1)
        if np.float32(max_distance) > 0:
            ok &= dist0 <= np.float32(max_distance)
    return np.where(ok, idx[:, 0], -1).astype(np.int32)


def match_pair(q, xy1, t, xy2, F, ratio=0.7, max_error_px=3.0, max_distance=0.0, cross_check=0, stride=None):
    """Returns (out [stride], in-band combinations)."""
    F = np.asarray(F, np.float64).reshape(9)
    m = band(F, xy1, xy2, max_error_px)
    r = raw(*knn2(q, t, m), ratio, max_distance)
    out = np.full(len(r) if stride is None else stride, -1, np.int32)
    if cross_check:
        mt = band(F.reshape(3, 3).T.reshape(9), xy2, xy1, max_error_px)        # the reversed pair under F^T, computed on its own
        rt = raw(*knn2(t, q, mt), ratio, max_distance)
        for i, j in enumerate(r):
            if j >= 0 and rt[j] == i:
                out[i] = j
    else:
        taken = set()
        for i, j in enumerate(r):                 # ascending query rows: the lowest keeps a contested train row
            if j >= 0 and int(j) not in taken:
                taken.add(int(j))
                out[i] = j
    return out, int(m.sum())


def match_grid(desc, coords, pairs, Fs, stride, **opt):
    """desc / coords: id -> rows / (K, 2); Fs [P][9].  Returns (table [P][stride], counts [P], cand [P])."""
    P = len(pairs)
    table = np.full((P, stride), -1, np.int32)
    cand = np.zeros(P, np.int64)
    for p, (a, b) in enumerate(pairs):
        table[p], cand[p] = match_pair(desc[a], coords[a], desc[b], coords[b], Fs[p], stride=stride, **opt)
    return table, (table >= 0).sum(axis=1).astype(np.int32), cand


# ---- cases ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(0, 5), (5, 0), (1, 1), (3, 2), (63, 64), (64, 65), (65, 63), (300, 515)]
DIMS = [32, 40, 128, 256]
PLANT_COUNTS = [0, 1, 2, 23, 24, 25, 49, 65]


def rows(rng, K, D):
    return rng.standard_normal((K, D)).astype(np.float32)


def two_view(rng, K1, K2, share=0.6, noise=1.0, size=1000):
    """Integer keypoints of two cameras looking at one cloud, and the pair's true F in the filter's convention (p2^T F p1)."""
    n = max(K1, K2, 1)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 9, n)]
    Kc = np.array([[700., 0, size / 2], [0, 700., size / 2], [0, 0, 1]])
    ang = 0.12
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    tr = np.array([-0.8, 0.05, 0.1])
    def proj(Xc):
        p = (Kc @ Xc.T).T
        return p[:, :2] / p[:, 2:]
    p1, p2 = proj(X), proj((R @ X.T).T + tr)
    xy1 = np.rint(p1[:K1] + rng.normal(0, noise, (K1, 2))).astype(np.int32)
    xy2 = np.rint(p2[:K2] + rng.normal(0, noise, (K2, 2))).astype(np.int32)
    stray = rng.random(K2) > share                  # train points that belong to nothing
    xy2[stray] = rng.integers(0, size, (int(stray.sum()), 2))
    tx = np.array([[0, -tr[2], tr[1]], [tr[2], 0, -tr[0]], [-tr[1], tr[0], 0]])
    Fm = np.linalg.inv(Kc).T @ tx @ R @ np.linalg.inv(Kc)
    Fm = Fm / Fm[2, 2] if abs(Fm[2, 2]) > 1e-12 else Fm / np.abs(Fm).max()
    return xy1, xy2, Fm.reshape(9), stray


def shape_case(K1, K2, D, seed):
    """Random rows over a two-view scene; the train rows that share a world point with a query row are noisy copies of it."""
    rng = np.random.default_rng(seed)
    xy1, xy2, F, stray = two_view(rng, K1, K2)
    q, t = rows(rng, K1, D), rows(rng, K2, D)
    for j in range(min(K1, K2)):
        if not stray[j]:
            t[j] = q[j] + np.float32(0.15) * rows(rng, 1, D)[0]
    return q, xy1, t, xy2, F


def planted_counts_case(D, seed=5):
    """Rectified F: query row r has exactly PLANT_COUNTS[r] train rows within 3 px of its y, in a shuffled train image."""
    rng = np.random.default_rng(seed)
    K1 = len(PLANT_COUNTS)
    xy1 = np.c_[rng.integers(0, 900, K1), 100 * np.arange(K1) + 50].astype(np.int32)
    ys = []
    for r, c in enumerate(PLANT_COUNTS):
        ys += [int(xy1[r, 1] + rng.integers(-3, 4)) for _ in range(c)]
    ys += [int(xy1[r, 1] + s * 4) for r in range(K1) for s in (-1, 1)]      # 4 px off: just outside every band
    ys = np.array(ys)[rng.permutation(len(ys))]
    xy2 = np.c_[rng.integers(0, 900, len(ys)), ys].astype(np.int32)
    return rows(rng, K1, D), xy1, rows(rng, len(xy2), D), xy2, RECT_F.copy()


def all_in_band_case(K1, K2, D, seed=6):
    """Rectified F and one image row: every train row is a candidate of every query row."""
    rng = np.random.default_rng(seed)
    xy1 = np.c_[rng.integers(0, 900, K1), np.full(K1, 77)].astype(np.int32)
    xy2 = np.c_[rng.integers(0, 900, K2), 77 + rng.integers(-3, 4, K2)].astype(np.int32)
    q, t = rows(rng, K1, D), rows(rng, K2, D)
    for j in range(0, min(K1, K2), 2):
        t[j] = q[j] + np.float32(0.1) * rows(rng, 1, D)[0]
    return q, xy1, t, xy2, RECT_F.copy()


def ragged_grid(D=128, seed=21):
    """Six images of ragged K (one empty) of one cloud seen by six cameras; pairs scrambled with repeats.
    Returns (desc id -> rows, coords id -> xy, pairs [P][2], true F per pair [P][9] scaled to max |F| = 1)."""
    rng = np.random.default_rng(seed)
    Ks = [70, 0, 33, 130, 97, 64]
    n = 140
    world = rows(rng, n, D)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(5, 9, n)]
    Kc = np.array([[600., 0, 400], [0, 600., 300], [0, 0, 1]])
    cams, desc, coords = [], {}, {}
    for i, K in enumerate(Ks):
        ang = 0.04 * i
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        tr = np.array([-0.35 * i, 0.06 * i, 0.08 * i])
        cams.append((R, tr))
        sel = rng.permutation(n)[:K]
        pr = (Kc @ ((R @ X[sel].T).T + tr).T).T
        desc[i] = world[sel] + np.float32(0.1) * rows(rng, K, D)
        coords[i] = np.rint(pr[:, :2] / pr[:, 2:] + rng.normal(0, 0.4, (K, 2))).astype(np.int32).reshape(K, 2)
    pairs = np.array([(3, 0), (0, 4), (5, 3), (1, 2), (2, 1), (4, 5), (3, 0), (0, 3), (2, 5), (4, 3)], np.int32)
    Fs = np.zeros((len(pairs), 9))
    Ki = np.linalg.inv(Kc)
    for p, (a, b) in enumerate(pairs):
        (Ra, ta), (Rb, tb) = cams[a], cams[b]
        R = Rb @ Ra.T
        tr = tb - R @ ta
        tx = np.array([[0, -tr[2], tr[1]], [tr[2], 0, -tr[0]], [-tr[1], tr[0], 0]])
        Fm = Ki.T @ tx @ R @ Ki
        Fs[p] = (Fm / np.abs(Fm).max()).reshape(9)
    return desc, coords, pairs, Fs
