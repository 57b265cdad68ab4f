"""numpy model of the int8 coarse pass (csrc/match.hip: fix_scale, k_prepare_i8, k_coarse_top2_i8, k_filter, certify), shared by
tests/test_int8_emulation.py (CPU) and tests/test_int8_gpu.py.  Everything the device computes in integers is computed here in
integers; the certificates are evaluated in float64 as the kernels do."""
import math

import numpy as np

IDX_BITS = 12
PAD_ACC = (1 << (32 - IDX_BITS)) - 1
RES_MAX = 8.01
M_MAX = 720.0
PEAK_MAX = 8.0
RATIO = np.float32(0.7)


def _round_up_grid(v, steps):
    m, e = math.frexp(v * (1.0 + 1e-12))
    return math.ldexp(math.ceil(m * steps) / steps, e)


def fix_scale(images, force=False):
    """The int8 branch of fix_scale for a resident set (list of float32 arrays, D <= 256).  Returns None when the device keeps fp16
    (force=True: the scale it WOULD use, to show that a refused data kind is refused for speed, not for correctness)."""
    rows = [im for im in images if im.shape[0] > 0]
    maxabs = max((float(np.abs(im).max()) for im in rows), default=0.0)
    maxn2 = max((float((im.astype(np.float64) ** 2).sum(1).max()) for im in rows), default=0.0)
    if not (0.0 < maxabs <= 3.4028234e38 and 0.0 < maxn2 <= 1.7976931348623157e308):
        return None
    n_max = math.sqrt(_round_up_grid(maxn2, 32))
    maxabs_q = _round_up_grid(maxabs, 64)
    peak = maxabs_q * 16.0 / n_max
    if peak >= PEAK_MAX and not force:
        return None
    s = min(127.0 / maxabs_q, (M_MAX - 8.5) / n_max)
    M = s * n_max + 8.5
    bias = math.ceil(0.5 * M * M + RES_MAX * M) + 2.0
    return {"s": s, "bias": bias, "n_max": n_max, "peak": peak, "M": M}


def quantise(x, s):
    """(xq int64 [K, 256], residual norm, quantised norm) of float32 rows; D < 256 is zero-padded."""
    v = np.zeros((x.shape[0], 256), np.float64)
    v[:, : x.shape[1]] = x.astype(np.float64) * s
    q = np.clip(np.rint(v), -127, 127)
    r = v - q
    return q.astype(np.int64), np.sqrt((r * r).sum(1)), np.sqrt((q * q).sum(1))


def half_norms(x, S):
    n2 = (x.astype(np.float64) ** 2).sum(1)
    return (np.rint(0.5 * S["s"] ** 2 * n2) + S["bias"]).astype(np.int64)


def accumulators(qq, tq, hn):
    """exact integer accumulator of every (query, train) pair"""
    return hn[None, :] - qq @ tq.T


def keys_top2(acc):
    """the packed (best, second) keys the kernel leaves: the two smallest of (acc << 12 | row)"""
    key = (acc.astype(np.int64) << IDX_BITS) | np.arange(acc.shape[1], dtype=np.int64)[None, :]
    part = np.partition(key, 1, axis=1)[:, :2]
    part.sort(axis=1)
    return part.astype(np.uint32)


def ratio_pass(d0, d1, ratio=RATIO):
    a = np.sqrt(np.asarray(d0, np.float64).astype(np.float32))
    b = np.sqrt(np.asarray(d1, np.float64).astype(np.float32))
    return a < np.float32(ratio) * b


def decide_pair(q, t, S, rho, tau, exact_d2):
    """The tiers for one (query image, train image): returns (result, tier) per query row.  result >= 0 match, -1 no match, -2 left to
    the exact tiers; tier 0 = decided by the coarse pair alone (k_filter), 1 = by the re-rank (certify), 2 = past the re-rank.
    exact_d2(query rows, train rows) -> canonical fp64 squared distances of row pairs."""
    K1, K2 = q.shape[0], t.shape[0]
    res = np.full(K1, -2, np.int64)
    tier = np.full(K1, 2, np.int64)
    if K1 == 0 or K2 < 2:
        return res, tier
    s2 = S["s"] ** 2
    qq, rq, nq = quantise(q, S["s"])
    tq, _, _ = quantise(t, S["s"])
    acc = accumulators(qq, tq, half_norms(t, S))
    assert acc.min() >= 1 and acc.max() < PAD_ACC, (acc.min(), acc.max())
    keys = keys_top2(acc)
    a0, a1 = (keys[:, 0] >> IDX_BITS).astype(np.float64), (keys[:, 1] >> IDX_BITS).astype(np.float64)
    i0, i1 = (keys[:, 0] & 0xFFF).astype(np.int64), (keys[:, 1] & 0xFFF).astype(np.int64)
    nq2 = (q.astype(np.float64) ** 2).sum(1)
    E = (nq * rho + rq * (tau + rho)) * (1.0 + 1e-9) + 0.5 + 1.0e-3
    slack = 1e-9 * (nq2 + S["n_max"] ** 2)
    d2 = lambda a: nq2 + (2.0 / s2) * (a - S["bias"])
    lb0 = np.maximum(d2(a0 - E) - slack, 0.0)
    ub1 = d2(a1 + E) + slack
    surv = ratio_pass(lb0, ub1)
    ub0 = d2(a0 + E) + slack
    lbnc = np.maximum(d2(a1 - E) - slack, 0.0)
    match = surv & (K2 > 2) & (ub0 >= 0.0) & (ub0 < lbnc) & ratio_pass(ub0, lbnc)
    res[~surv] = -1
    tier[~surv] = 0
    res[match] = i0[match]
    tier[match] = 0
    und = np.nonzero(surv & ~match)[0]
    if und.size and K2 > 2:
        ea = exact_d2(q[und], t[i0[und]])
        eb = exact_d2(q[und], t[i1[und]])
        ia, ib = i0[und].copy(), i1[und].copy()
        sw = (eb < ea) | ((eb == ea) & (ib < ia))
        ea, eb = np.where(sw, eb, ea), np.where(sw, ea, eb)
        ia = np.where(sw, ib, ia)
        lb = lbnc[und]
        nn = ea < lb
        lb1 = np.maximum(np.minimum(eb, lb), 0.0)
        l0 = np.maximum(np.minimum(ea, lb), 0.0)
        yes = nn & ratio_pass(ea, lb1)
        no = ~yes & ~ratio_pass(l0, eb)
        res[und[yes]] = ia[yes]
        res[und[no]] = -1
        tier[und[yes | no]] = 1
        tier[und[~(yes | no)]] = 2
    return res, tier
