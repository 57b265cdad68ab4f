"""Inputs that reach the fp16 coarse pass's error bound, in plain numpy: the emulation of the coarse pass with
the fp32 -> fp16 conversion as a parameter, the bound eps(q) and its accumulation-only part, a replica of k_filter's two certificates,
and four generators.  Imported by tests/test_coarse_stress_ref.py (CPU: the constructions do what they claim),
tests/test_coarse_stress_gpu.py and tools/mfma_error_stress.py (the hardware against them).

Every set is a small grid: a list of images and a pair list (query image, train image), at most 128 query and 256 train rows per
pair: images are padded to 512 rows, the train index takes 9 bits of the packed key, and the truncation quantum (512 ulp of the
accumulator) stays below 0.03 eps.

    aligned(D)     every element of a row has the same magnitude just below (down-type, m = 1 + 2^-11 - 2^-20) or just above
                   (up-type, 1 + 2^-11 + 2^-20) an fp16 rounding midpoint at the bottom of a binade, so the conversion moves every
                   element by u = 2^-11 (relative) in the same direction; a query's twin (same signs) is a train row, every product of
                   the pair errs the same way and q.t = |q| |t|: the first term of eps, a Cauchy-Schwarz worst case, is nearly met.
    accumulation_only(D)   fp16-exact operands with full 11-bit significands, a query and its two partners sharing signs: the operands
                   carry no error, what is left comes from the accumulation inside the MFMA and the rounding of the half-norm, and is
                   judged against eps_acc (the last three terms of eps).
    misranked(D)   per query three planted rows: T1 (nearest), T3 (the true second, down-type like the query) and T2 (fp16-exact),
                   whose exact accumulator lies ABOVE T3's while its coarse one lies BELOW: the coarse pass's second candidate is not
                   the second neighbour, and the ratio d0^2 / d^2(T3) sits a fraction of the bound away from 0.49 on either side.
    band(D)        queries whose (best, second) sit so close to the 0.7 line that k_filter's two certificates leave them undecided
                   with eps, though they would decide them with eps / 2."""
import numpy as np

U = 2.0 ** -11
DIMS = (32, 40, 64, 100, 128, 256)
M_DOWN = 1.0 + 2.0 ** -11 - 2.0 ** -20       # RNE to fp16 rounds it DOWN to 1 (error -u, nearly)
M_UP = 1.0 + 2.0 ** -11 + 2.0 ** -20         # ... UP to 1 + 2^-10
M_TRUNC = 1.0 + 2.0 ** -10 - 2.0 ** -20      # RNE keeps it within 2^-20; a truncating conversion loses 2u: the control of the CPU test
RATIO = np.float32(0.7)


def padded(D):
    """The kernel's DP: D padded to 32, 64, 128 or 256."""
    return max(32, 1 << int(np.ceil(np.log2(D))))


# ---- the error model (fix_scale / coarse_eps of csrc/match.hip) -------------------------------------------------------------------
def model(images, D=None):
    """The scale constants fix_scale derives from the resident rows (no BIG-row split, fp16 path): a dict."""
    D = D or images[0].shape[1]
    maxabs = max(float(np.abs(im).max()) for im in images if len(im))
    maxn2 = max(float((im.astype(np.float64) ** 2).sum(1).max()) for im in images if len(im))
    _, ex = np.frexp(maxabs)
    s = float(np.ldexp(1.0, 14 - int(ex)))
    mn, en = np.frexp(maxn2 * (1 + 1e-12))
    maxn2q = float(np.ldexp(np.ceil(mn * 32.0) / 32.0, int(en)))
    bias = 0.5625 * s * s * maxn2q + 1.0
    nmax = float(np.sqrt(maxn2q))
    return {"s": s, "bias": bias, "nmax": nmax, "DP": padded(D), "hn_max": 0.5 * s * s * nmax * nmax + bias}


def eps_acc(mdl, nq):
    """The part of eps that does not come from the operands: accumulation inside the MFMA, the fp32 half-norm, the evaluation slack."""
    s, nmax, DP, hn_max = mdl["s"], mdl["nmax"], mdl["DP"], mdl["hn_max"]
    return (DP + 8) * 2.0 ** -23 * (hn_max + s * s * nq * nmax) + 6.0e-8 * hn_max + 1e-9


def eps(mdl, nq):
    """eps(q) for query norms nq (the caller applies the (1 + 1e-12) the kernel puts on the norm), accumulator units."""
    s, nmax, DP = mdl["s"], mdl["nmax"], mdl["DP"]
    return (2 * U + U * U) * s * s * nq * nmax + 2.0 ** -14 * np.sqrt(DP) * s * (nq + nmax) + eps_acc(mdl, nq)


def qnorm(q):
    return np.sqrt((q.astype(np.float64) ** 2).sum(1)) * (1 + 1e-12)


def err_bound_d2(mdl):
    """What rcn_match_last_stats reports: 2 eps(Nmax) / s^2, a squared distance."""
    return 2.0 * float(eps(mdl, mdl["nmax"])) / (mdl["s"] ** 2)


# ---- the coarse pass -------------------------------------------------------------------------------------------------------------
def rne_f16(x):
    """fp32 -> fp16, round to nearest even: what k_prepare does."""
    return x.astype(np.float32).astype(np.float16)


def trunc_f16(x):
    """fp32 -> fp16 by dropping the low 13 significand bits (normal range): a conversion fault the instrument must see."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFFE000)
    return b.view(np.float32).astype(np.float16)


def emulate(q, t, mdl, convert=rne_f16):
    """(acc, exact): the fp32 accumulators of the coarse pass for every (query, train) pair -- inputs scaled by s and converted,
    products accumulated in fp32 on top of the fp32 half-norm (in numpy's order: the bound must hold for any) -- and the real values
    A* = s^2 (|t|^2 / 2 - q.t) + BIAS in float64."""
    s, bias = mdl["s"], mdl["bias"]
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    a = convert(s * t64)
    b = convert(-s * q64)
    hn = (0.5 * s * s * (t64 ** 2).sum(1) + bias).astype(np.float32)
    acc = (hn[None, :] + (b.astype(np.float32) @ a.astype(np.float32).T)).astype(np.float32).astype(np.float64)
    exact = 0.5 * s * s * (t64 ** 2).sum(1)[None, :] + bias - s * s * (q64 @ t64.T)
    return acc, exact


def index_mask(K2):
    """The low bits of a packed key that hold the train row: the library pads an image to a multiple of 512 rows, so 9 for every set here."""
    Kp = 512 * max(1, -(-K2 // 512))
    return np.uint32((1 << int(np.ceil(np.log2(Kp)))) - 1)


def coarse_top2(acc, K2):
    """The packed (best, second) keys the kernel keeps: the fp32 accumulator with the train row in its low bits."""
    mask = index_mask(K2)
    packed = (acc.astype(np.float32).view(np.uint32) & ~mask) | np.arange(K2, dtype=np.uint32)[None, :]
    packed.sort(axis=1)
    return packed[:, 0].copy(), packed[:, 1].copy(), mask


def ratio_pass(d2a, d2b):
    return np.sqrt(d2a.astype(np.float32)) < RATIO * np.sqrt(d2b.astype(np.float32))


def filter_decisions(q, c0, c1, mask, mdl, e):
    """k_filter's two certificates from the packed keys and a bound e per query: (certified 'no match', certified 'match = best')."""
    s, bias, nmax = mdl["s"], mdl["bias"], mdl["nmax"]
    f = lambda k: k.astype(np.uint32).view(np.float32).astype(np.float64)
    nq2 = (q.astype(np.float64) ** 2).sum(1)
    slack = 1e-9 * (nq2 + nmax * nmax)
    d2 = lambda a_: nq2 + (2.0 / (s * s)) * (a_ - bias)
    lo0, hi0 = f(c0 & ~mask), f((c0 & ~mask) + mask + np.uint32(1))
    lo1, hi1 = f(c1 & ~mask), f((c1 & ~mask) + mask + np.uint32(1))
    lb0, ub1 = np.maximum(d2(lo0 - e) - slack, 0.0), d2(hi1 + e) + slack
    ub0, lbnc = d2(hi0 + e) + slack, np.maximum(d2(lo1 - e) - slack, 0.0)
    cert_fail = ~ratio_pass(lb0, ub1)
    cert_pass = ~cert_fail & (ub0 >= 0.0) & (ub0 < lbnc) & ratio_pass(ub0, lbnc)
    return cert_fail, cert_pass


# ---- generators ------------------------------------------------------------------------------------------------------------------
def _f32(x):
    y = np.ascontiguousarray(x, np.float32)
    assert np.array_equal(y.astype(np.float64), np.asarray(x, np.float64)), "the construction needs fp32-exact values"
    return y


def _peaked_row(D, norm, rng):
    """One row whose largest element is 0.9 of its norm: max |x| sqrt(D) / Nmax = 14.4 at D = 256, fix_scale refuses int8."""
    x = rng.standard_normal(D)
    x[17] = 0.0
    x *= np.sqrt(1.0 - 0.81) / np.linalg.norm(x)
    x[17] = 0.9
    return (0.999 * norm * x).astype(np.float32)       # (just inside the set's largest norm: Nmax stays what the set made it)


def aligned(D, seed=0):
    """Two pairs (down-type, up-type) of 48 queries x 128 train rows.  Query 3i + j has norm N / 4^{(0, 1, 3)[j]}; train row 2k is
    query k's twin at norm N (the query times a power of two), 2k + 1 its mirror (aligned with -q, the largest accumulator of the
    row); the rest are rows of the same alphabet with independent signs."""
    rng = np.random.default_rng(1000 + 7 * D + seed)
    images, pairs, info = [], [], []
    for m in (M_DOWN, M_UP):
        sg = rng.choice([-1.0, 1.0], (48, D))
        shrink = np.array([1.0, 0.25, 1.0 / 64])[np.arange(48) % 3]
        q = sg * m * shrink[:, None]
        t = rng.choice([-1.0, 1.0], (128, D)) * m
        t[0:96:2] = sg * m
        t[1:96:2] = -sg * m
        pairs.append((len(images), len(images) + 1))
        images += [_f32(q), _f32(t)]
        info.append({"type": "down" if m == M_DOWN else "up", "twin": 2 * np.arange(48), "mirror": 2 * np.arange(48) + 1,
                     "full_norm": np.nonzero(shrink == 1.0)[0]})
    return {"images": images, "pairs": pairs, "info": info}


def truncation_control(D, seed=0):
    """The aligned construction at magnitude 1 + 2^-10 - 2^-20: harmless under RNE, 2u per element under a truncating conversion."""
    rng = np.random.default_rng(2000 + D + seed)
    sg = rng.choice([-1.0, 1.0], (16, D))
    t = rng.choice([-1.0, 1.0], (64, D)) * M_TRUNC
    t[:16] = sg * M_TRUNC
    return {"images": [_f32(sg * M_TRUNC), _f32(t)], "pairs": [(0, 1)], "info": [{"twin": np.arange(16)}]}


def accumulation_only(D, seed=0):
    """Two pairs of 32 queries x 64 train rows; every element
    is +-(1024 + k) / 1024 * 2^e with k odd (all 11 significand bits in use, exact in fp16 after the power-of-two scale), e in
    {0, -1}; train rows 2i and 2i + 1 carry query i's signs, so the products of the pair all have one sign and the partial sums fall
    monotonically from the half-norm.
        pair 0   row 2i is the query itself, row 2i + 1 the query with four magnitudes redrawn: the sum falls from hn (about
                 1.06 s^2 N^2) to about s^2 N^2 / 16, the largest cancellation the bias allows, and the final accumulator's ulp -- the
                 unit in which the packed key is read -- is the smallest
        pair 1   both partners have magnitudes of their own.
    What the instrument can resolve: the key drops the accumulator's low 9 bits, 512 ulp of the final value (32 - 64 ulp of the
    half-norm in pair 0), and eps_acc is about (DP + 8) ulp of the half-norm's binade times two: an accumulation error shows once it
    exceeds 0.4 eps_acc at DP = 32 and 0.04 eps_acc at DP = 256; tools/mfma_error_stress.py reports that quantum next to the excursion."""
    rng = np.random.default_rng(3000 + 11 * D + seed)
    images, pairs = [], []
    mag = lambda n: (1024 + 2 * rng.integers(0, 512, (n, D)) + 1) / 1024.0 * 2.0 ** (-rng.integers(0, 2, (n, D)).astype(np.float64))
    for p in range(2):
        sg = rng.choice([-1.0, 1.0], (32, D))
        q = sg * mag(32)
        t = np.empty((64, D))
        t[0::2] = sg * mag(32)
        t[1::2] = sg * mag(32)
        if p == 0:
            t[0::2] = q
            t[1::2] = q
            for i in range(32):
                e = rng.permutation(D)[:4]
                t[2 * i + 1, e] = sg[i, e] * mag(1)[0, e]
        pairs.append((len(images), len(images) + 1))
        images += [_f32(q), _f32(t)]
    return {"images": images, "pairs": pairs, "info": [{}, {}]}


MISRANK_C = (0.02, -0.02, 0.05, -0.05, 0.1, -0.1, 0.15, -0.15, 0.3, -0.3, 0.6, -0.6, 1.2, -1.2, 0.08, -0.08)


def misranked(D, peaked=False, seed=0):
    """Two pairs of 32 queries x 128 train rows.  Query i (all elements +-m, down-type) owns train rows 3i (T1), 3i + 1 (T2), 3i + 2 (T3):
        T1  q with f / 2 sign flips, one of them partial, so that d0^2 = 0.49 d^2(T3) + c E(q) with c from MISRANK_C
            (E = 2 eps / s^2, the bound as a squared distance)
        T3  q with f sign flips, down-type: the true second neighbour, d^2 = 4 f m^2
        T2  magnitude 1 (fp16-exact) with q's signs, f flips, one kept element scaled by 1 - k 2^-9.  With delta = k 2^-9 the exact
            accumulators differ by A*(T2) - A*(T3) = s^2 (delta^2 / 2 - 2 u f + ...) and the coarse ones by s^2 (delta^2 / 2 - u D):
            for 512 f < k^2 < 256 D the exact order is T3 < T2 and the coarse order T2 < T3.  k sweeps that band.
    f = 2 (D // 16); rows 96 .. 127 are fillers of the same alphabet.  peaked: one filler of the last image becomes a row with one
    large element (keeps a D = 256 set off the int8 path; the scale is a power of two, so nothing else changes but s)."""
    rng = np.random.default_rng(4000 + 13 * D + seed)
    f = 2 * (D // 16)
    m = M_DOWN
    N = np.sqrt(D) * m
    k_lo, k_hi = np.sqrt(512.0 * f), np.sqrt(256.0 * D)
    images, pairs, info = [], [], []
    for p in range(2):
        sg = rng.choice([-1.0, 1.0], (32, D))
        q = sg * m
        t = rng.choice([-1.0, 1.0], (128, D)) * m
        if peaked and p == 1:
            x = np.full(D, 0.5) * rng.choice([-1.0, 1.0], D)
            x[17] = 12.0                                       # max |x| sqrt(D) / Nmax = 12: above RCN_I8_PEAK_MAX
            assert (x ** 2).sum() < N * N
            t[127] = x
        images += [_f32(q), None]
        # the bound as a squared distance, for the partial element of T1: every pair of the set has the same max |x| binade and Nmax
        mdl = model([_f32(q), _f32(t)], D)
        E = 2.0 * eps(mdl, qnorm(_f32(q))) / mdl["s"] ** 2
        ks, cs = [], []
        for i in range(32):
            perm = rng.permutation(D)
            k = int(np.clip(np.rint(k_lo + (k_hi - k_lo) * (0.25 + 0.7 * ((i * 7) % 32) / 32.0)), np.ceil(k_lo), np.floor(k_hi)))
            c = MISRANK_C[(i + 16 * p) % len(MISRANK_C)] if i < 16 else MISRANK_C[(i * 5 + p) % len(MISRANK_C)]
            t1 = q[i].copy()
            t1[perm[:f // 2]] *= -1.0
            a = np.sqrt((1.96 * f * m * m + c * E[i] - 4.0 * m * m * (f // 2 - 1)) / (m * m)) - 1.0
            t1[perm[0]] = -a * q[i, perm[0]]
            t3 = q[i].copy()
            t3[perm[f:2 * f]] *= -1.0
            t2 = sg[i].copy()
            t2[perm[2 * f:3 * f]] *= -1.0
            t2[perm[3 * f]] *= 1.0 - k * 2.0 ** -9
            t[3 * i], t[3 * i + 1], t[3 * i + 2] = t1, t2, t3
            ks.append(k)
            cs.append(c)
        images[-1] = np.ascontiguousarray(t, np.float32)        # (T1's partial element is rounded to fp32; everything downstream reads the rounded row)
        pairs.append((len(images) - 2, len(images) - 1))
        info.append({"k": np.array(ks), "c": np.array(cs), "T1": 3 * np.arange(32), "T2": 3 * np.arange(32) + 1, "T3": 3 * np.arange(32) + 2})
    return {"images": images, "pairs": pairs, "info": info}


def band_status(q, t, mdl, scale):
    """Per query: decided by k_filter's certificates when the bound is scale * eps?  (On the emulated coarse pass.)"""
    acc, _ = emulate(q, t, mdl)
    c0, c1, mask = coarse_top2(acc, len(t))
    cf, cp = filter_decisions(q, c0, c1, mask, mdl, scale * eps(mdl, qnorm(q)))
    return cf | cp


def band(D, peaked=False, seed=0):
    """Two pairs of up to 64 queries x 192 train rows of unit-norm Gaussian rows.  Query i owns train rows 2i (at distance d0) and
    2i + 1 (d1^2 = 0.2, far inside every other row's distance) with d0^2 = 0.49 d1^2 + c E(q): |c| in 0.9 .. 1.26 puts the row inside
    the band that the certificates (which need |d0^2 - 0.49 d1^2| > 1.49 E, about) leave open with eps and close with eps / 2.
    Only queries that the replica of k_filter leaves undecided at 0.9 eps AND decides at 0.55 eps stay: the 10 % on either side keep
    a different accumulation order from mattering.  The train images are not touched by that selection.
    peaked: the last row of the last image is a row with one large element (see misranked)."""
    rng = np.random.default_rng(5000 + 17 * D + seed)
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    qs = [unit(rng.standard_normal((64, D))) for _ in range(2)]
    ts = [unit(rng.standard_normal((192, D))) for _ in range(2)]
    if peaked:
        ts[1][191] = _peaked_row(D, 1.0, rng)
    side = [np.where((np.arange(64) + p) % 2 == 0, 1.0, -1.0) for p in range(2)]
    cabs = [rng.uniform(0.9, 1.26, 64) for _ in range(2)]
    dirs = []
    for p in range(2):
        n = rng.standard_normal((64, 2, D))
        n -= (n @ qs[p][:, :, None]) * qs[p][:, None, :]       # orthogonal to q: |t|^2 = 1 + d^2
        dirs.append(n / np.linalg.norm(n, axis=2, keepdims=True))
    d1 = 0.2
    for _ in range(2):       # the planted rows raise Nmax: the second round prices E with the model they leave
        mdl = model([x.astype(np.float32) for x in qs + ts], D)
        for p in range(2):
            E = 2.0 * eps(mdl, qnorm(qs[p].astype(np.float32))) / mdl["s"] ** 2
            d0 = 0.49 * d1 + side[p] * cabs[p] * E
            ts[p][0:128:2] = qs[p] + np.sqrt(d0)[:, None] * dirs[p][:, 0]
            ts[p][1:128:2] = qs[p] + np.sqrt(d1) * dirs[p][:, 1]
    q32 = [x.astype(np.float32) for x in qs]
    t32 = [x.astype(np.float32) for x in ts]
    for _ in range(3):       # dropping queries may move max |x|: select under the model of what stays
        mdl = model(q32 + t32, D)
        keep = [~band_status(q, t, mdl, 0.9) & band_status(q, t, mdl, 0.55) for q, t in zip(q32, t32)]
        if all(k.all() for k in keep):
            break
        q32 = [np.ascontiguousarray(q[k]) for q, k in zip(q32, keep)]
    images = [np.ascontiguousarray(x) for qt in zip(q32, t32) for x in qt]
    return {"images": images, "pairs": [(0, 1), (2, 3)], "info": [{}, {}]}


def pipeline_decisions(q, t, mdl, scale=1.0):
    """The match table of one pair as k_filter and the re-rank's `certify` would leave it with the bound scale * eps, on the
    emulated coarse pass: -1 / train row, and -2 where neither certifies (the exact tiers decide those rows, correctly by
    construction).  A replica for the CPU test: it shows that the misranked rows turn into wrong entries under a bound that is
    too small, which is what makes their tables on the hardware a test of the bound."""
    acc, _ = emulate(q, t, mdl)
    c0, c1, mask = coarse_top2(acc, len(t))
    e = scale * eps(mdl, qnorm(q))
    cf, cp = filter_decisions(q, c0, c1, mask, mdl, e)
    ia, ib = (c0 & mask).astype(np.int64), (c1 & mask).astype(np.int64)
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    ea, eb = ((q64 - t64[ia]) ** 2).sum(1), ((q64 - t64[ib]) ** 2).sum(1)
    swap = (eb < ea) | ((eb == ea) & (ib < ia))
    ia = np.where(swap, ib, ia)
    ea, eb = np.minimum(ea, eb), np.maximum(ea, eb)
    nq2 = (q64 ** 2).sum(1)
    lo1 = (c1 & ~mask).astype(np.uint32).view(np.float32).astype(np.float64)
    lbnc = nq2 + (2.0 / mdl["s"] ** 2) * (lo1 - e - mdl["bias"]) - 1e-9 * (nq2 + mdl["nmax"] ** 2)
    lb1, lb0 = np.maximum(np.minimum(eb, lbnc), 0.0), np.maximum(np.minimum(ea, lbnc), 0.0)
    res = np.full(len(q), -2, np.int64)
    res[~ratio_pass(lb0, eb)] = -1
    match = (ea < lbnc) & ratio_pass(ea, lb1)
    res[match] = ia[match]
    res[cf] = -1
    res[cp] = (c0 & mask).astype(np.int64)[cp]
    return res
