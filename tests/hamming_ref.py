"""The contract of the Hamming matcher (reconstructor_amd/csrc/hamming.hip) restated in numpy: what
cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) returns behind the ratio test and the uniqueness loop of FeatureMatcher.cpp:53-64.
OpenCV is not available here, so parity with it is unpinned; this file is what the GPU must equal, bit for bit (everything is integer).

    rows_of(count, K)             clamp(count, 0, K): the rows of an image that take part
    distances(q, t)               popcount(q_i XOR t_j), int32 [K1][K2]
    knn2(q, t)                    int32 [K1][4] = (j0, d0, j1, d1), train rows ordered by (d, j) ascending, -1 where absent
    ratio_pass(d0, d1, ratio)     float32(d0) < float32(ratio) * float32(d1): one fp32 product, one fp32 comparison
    match_pair(q, t, ratio)       the set rule: the lowest passing query row keeps a contested train row -> (out [K1], count)
    match_pair_loop(q, t, ratio)  the reference's sequential loop written out, for the test that the two agree
    match_grid(images, pairs, ratio, stride)   the dense table and counts of a list of (query, train) pairs

Rows are uint8 [K][32]; images for match_grid are (bytes [K][32], count) with count as ORB reports it (it may exceed K or be -1).
"""
import numpy as np

B = 32
POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int32)


def rows_of(count, K):
    return int(min(max(int(count), 0), int(K)))


def _rows(x):
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.ndim != 2 or x.shape[1] != B:
        raise ValueError("rows are uint8 [K][32]")
    return x


def distances(q, t):
    q, t = _rows(q), _rows(t)
    d = np.zeros((len(q), len(t)), np.int32)
    for lo in range(0, len(q), 256):                  # blocks of queries: the XOR cube stays small
        d[lo:lo + 256] = POPCOUNT[q[lo:lo + 256, None, :] ^ t[None, :, :]].sum(axis=2, dtype=np.int32)
    return d


def knn2(q, t):
    d = distances(q, t)
    K1, K2 = d.shape
    out = np.full((K1, 4), -1, np.int32)
    if K1 == 0 or K2 == 0:
        return out
    order = np.argsort(d, axis=1, kind="stable")[:, :2]          # stable: a tie on the distance goes to the lower train row
    rows = np.arange(K1)
    out[:, 0] = order[:, 0]
    out[:, 1] = d[rows, order[:, 0]]
    if K2 >= 2:
        out[:, 2] = order[:, 1]
        out[:, 3] = d[rows, order[:, 1]]
    return out


def ratio_pass(d0, d1, ratio=0.7):
    return np.float32(d0) < np.float32(ratio) * np.float32(d1)


def match_pair(q, t, ratio=0.7):
    """The set rule on the knn2 table."""
    k = knn2(q, t)
    out = np.full(len(k), -1, np.int32)
    if len(k) == 0 or _rows(t).shape[0] < 2:
        return out, 0
    ok = ratio_pass(k[:, 1].astype(np.float32), k[:, 3].astype(np.float32), ratio)
    idx = np.nonzero(ok)[0]
    first = {}
    for i in idx:                                     # ascending: the first query to name a train row is the lowest
        first.setdefault(int(k[i, 0]), int(i))
    for j, i in first.items():
        out[i] = j
    return out, len(first)


def match_pair_loop(q, t, ratio=0.7):
    """FeatureMatcher.cpp:53-64 as it stands there: a list of matched train rows, searched for every passing query in turn."""
    k = knn2(q, t)
    matches = {}
    matched = []
    if _rows(t).shape[0] >= 2:                        # the reference reads knn[i][1] unconditionally: fewer than two train rows give nothing here
        for i in range(len(k)):
            if np.float32(k[i, 1]) < np.float32(ratio) * np.float32(k[i, 3]):
                j = int(k[i, 0])
                if j not in matched:
                    matches[i] = j
                    matched.append(j)
    out = np.full(len(k), -1, np.int32)
    for i, j in matches.items():
        out[i] = j
    return out, len(matches)


def match_grid(images, pairs, ratio=0.7, stride=None):
    """images: id -> (bytes [K][32], count or None for K).  Returns (table [n_pairs][stride], counts [n_pairs])."""
    live = {i: _rows(b)[:rows_of(len(b) if c is None else c, len(b))] for i, (b, c) in images.items()}
    if stride is None:
        stride = max([len(images[a][0]) for a, _ in pairs] + [1])
    table = np.full((len(pairs), stride), -1, np.int32)
    counts = np.zeros(len(pairs), np.int32)
    for p, (a, b) in enumerate(pairs):
        out, n = match_pair(live[a], live[b], ratio)
        table[p, :len(out)] = out
        counts[p] = n
    return table, counts


def random_rows(rng, K):
    return rng.integers(0, 256, (K, B), dtype=np.uint8)


def flip_bits(rng, row, n):
    """row with n distinct bits flipped."""
    out = row.copy()
    for bit in rng.choice(256, size=n, replace=False):
        out[bit // 8] ^= np.uint8(1 << (bit % 8))
    return out


def planted_pair(rng, K1, K2, share=0.5, max_flips=20):
    """Random query and train rows; a share of the train rows are query rows with 0 .. max_flips flipped bits, so that a good fraction
    passes the ratio test while the rest sits near d = 128 with plenty of distance ties."""
    q, t = random_rows(rng, K1), random_rows(rng, K2)
    if K1 and K2:
        for j in rng.choice(K2, size=int(K2 * share), replace=False):
            t[j] = flip_bits(rng, q[rng.integers(K1)], int(rng.integers(0, max_flips + 1)))
    return q, t


# ---- the cases the CPU and GPU tests and tests/golden/make_hamming_golden.py share

SHAPES = [(0, 5), (5, 0), (1, 1), (3, 1), (1, 2), (2, 2), (17, 16), (127, 129), (128, 128), (129, 257), (300, 515)]
EDGES = [(7, 10), (14, 20), (70, 100)]          # float32(d0) < float32(0.7) * float32(d1) is false for all three


def shape_cases():
    """name -> (q, t): seeded random rows of every shape, a share of the train rows planted near query rows."""
    return {"shape_%d_%d" % s: planted_pair(np.random.default_rng(100 + k), *s) for k, s in enumerate(SHAPES)}


def _with_bits(n):
    """A row whose first n bits are set: distance n to the zero row."""
    row = np.zeros(B, np.uint8)
    for bit in range(n):
        row[bit // 8] |= np.uint8(1 << (bit % 8))
    return row


def planted_cases():
    """name -> (q, t) with known answers (the tests state them)."""
    rng = np.random.default_rng(7)
    out = {}
    # duplicate train rows: best = the lower index, second = the twin, d0 == d1 and no match
    q, t = random_rows(rng, 4), random_rows(rng, 40)
    t[31] = t[9] = flip_bits(rng, q[2], 3)
    out["twins"] = (q, t)
    # d0 = 0 with d1 > 0 matches; d0 = d1 = 0 does not
    q, t = random_rows(rng, 3), random_rows(rng, 20)
    t[5] = q[1]
    t[11] = t[12] = q[2]
    out["exact"] = (q, t)
    # the fp32 edges: the zero query against rows at distance d0, d1 and all-ones rows (d = 256); (6, 10) for contrast: it passes
    for d0, d1 in EDGES + [(6, 10)]:
        t = np.full((6, B), 255, np.uint8)
        t[4], t[1] = _with_bits(d0), _with_bits(d1)
        out["edge_%d_%d" % (d0, d1)] = (np.zeros((1, B), np.uint8), t)
    # all-zero and all-ones rows: d = 256 needs the 9th bit
    q = np.stack([np.zeros(B, np.uint8), np.full(B, 255, np.uint8)])
    t = np.stack([np.full(B, 255, np.uint8), np.zeros(B, np.uint8), np.full(B, 255, np.uint8)])
    out["extremes"] = (q, t)
    out["extremes_only"] = (np.zeros((2, B), np.uint8), np.full((3, B), 255, np.uint8))
    return out


def far_rows_case():
    """K2 = 4100: query 0 has two train rows at the same distance, rows 3 and 4099 (the row bits beyond 12); query 1's close row is 4099."""
    rng = np.random.default_rng(9)
    q, t = random_rows(rng, 2), random_rows(rng, 4100)
    t[3], t[4099] = flip_bits(rng, q[0], 5), flip_bits(rng, q[0], 5)
    q[1] = flip_bits(rng, t[4099], 3)
    return q, t


def counts_case(K=40):
    """Six images of K row slots whose counts are -1, 0, 1, K - 1, K and K + 7; the slots past clamp(count, 0, K) hold copies of
    the next image's rows -- garbage that would match at distance 0 if it took part.  Returns (bytes [6][K][32], counts [6])."""
    rng = np.random.default_rng(13)
    base = random_rows(rng, K)
    by = np.stack([np.stack([flip_bits(rng, base[r], int(rng.integers(0, 40))) for r in range(K)]) for _ in range(6)])
    counts = np.array([-1, 0, 1, K - 1, K, K + 7], np.int32)
    clean = by.copy()
    for i, c in enumerate(counts):
        by[i, rows_of(c, K):] = clean[(i + 1) % 6, rows_of(c, K):]
    return by, counts


def ragged_images():
    """Six images of ragged row counts, planted against one another: id -> bytes."""
    rng = np.random.default_rng(17)
    Ks = [64, 1, 37, 130, 257, 300]
    world = random_rows(rng, 320)
    ims = {}
    for i, K in enumerate(Ks):
        pick = rng.choice(len(world), size=K, replace=False)
        ims[10 + 3 * i] = np.stack([flip_bits(rng, world[w], int(rng.integers(0, 30))) for w in pick])
    return ims
