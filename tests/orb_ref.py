"""The arithmetic contract of the ORB stage (csrc/orb.hip), in numpy: cv::ORB::create() with its
defaults (FeatureDetector.cpp:9, :19), written from the algorithm.  Integers throughout except two places, and there only
single correctly rounded float64 operations (no fused multiply-add): the Harris response and the patch direction.  The GPU
equals every function here bit for bit; `angle`, which no decision reads, to one fp32 ulp.

    layout      scale_l = float32(pow(float64(scale_factor), l)); level l has rint(H / scale_l) x rint(W / scale_l) pixels
                (float64 division, half to even); its keypoint quota is OpenCV's geometric split in float32
    pyramid     bytes; level l is level l - 1 through img_ref.resize_linear_u8 (cv::resize's 8-bit INTER_LINEAR).  A level
                that halves its predecessor on both axes would take resize's area branch: layout refuses it
    FAST-9/16   score = the largest t >= fast_threshold with 9 contiguous circle pixels all > p + t or all < p - t, else 0
                = max over the 16 arcs of (min over the arc of +-(c - p)) - 1; 0 within 3 pixels of the border
    NMS         score > 0 and strictly greater than its 8 neighbours, edge_threshold <= x < w - edge_threshold, y alike
    selection   per level, as sets: FAST score >= the (2 quota)-th largest; of those, Harris response >= the quota-th largest
    Harris      7 x 7 block of Sobel-like integer gradients; (double(det) - 0.04 * double(tr2)) * s4
    direction   integer moments over the circular patch of radius 15; cs = m10 / sqrt(h2), sn = m01 / sqrt(h2)
    blur        7 x 7, sigma 2, reflect-101, integer weights summing to 256 per axis, (v + 2^15) >> 16
    descriptor  256 tests steered by (cs, sn): ix = rint(x cs - y sn), iy = rint(x sn + y cs), bit = blur[p0] < blur[p1]
    output      ascending (level, y, x); beyond K the K largest by (response descending, canonical rank ascending)

Not pinned against OpenCV itself: INTER_LINEAR_EXACT's constants (INTER_LINEAR's are used), the 8-bit
GaussianBlur's constants, the learned test pattern (an input here), the order retainBest leaves (a set rule here).
"""
import math

import numpy as np

import img_ref

MAX_LEVELS = 16
MAX_SURVIVORS = 8192
PATCH = 31
HALF = 15
HARRIS_K = 0.04
_S = 1.0 / (4 * 7 * 255.0)
HARRIS_S4 = _S * _S * _S * _S
RAD2DEG = 180.0 / math.pi
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))   # (dx, dy)
DEFAULTS = dict(nfeatures=500, scale_factor=1.2, nlevels=8, edge_threshold=31, fast_threshold=20)


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise KeyError(k)
        o[k] = v
    return o


def check_pattern(pattern):
    p = np.asarray(pattern)
    if p.dtype != np.int8 or p.size != 1024:
        raise ValueError("orb_ref: a pattern is 1024 signed bytes")
    if np.abs(p.astype(np.int32)).max() > HALF:
        raise ValueError("orb_ref: pattern coordinate beyond +-15")
    return p.reshape(256, 4)


def cv_round(x):
    """cvRound of a float: half to even"""
    return int(np.rint(np.float64(x)))


def layout(H, W, opt=None):
    o = options(**(opt or {}))
    nf, nl, edge, thr, sf = int(o["nfeatures"]), int(o["nlevels"]), int(o["edge_threshold"]), int(o["fast_threshold"]), float(o["scale_factor"])
    if nf < 1 or not 1 <= nl <= MAX_LEVELS or not 22 <= edge <= 4096 or not 1 <= thr <= 254 or not 1.0 < sf <= 4.0:
        raise ValueError("orb_ref.layout: option out of range")
    if H < 1 or W < 1 or H > 65535 or W > 65535 or H * W > 2 ** 31 - 1:
        raise ValueError("orb_ref.layout: image size out of range")
    scale = [np.float32(math.pow(sf, l)) for l in range(nl)]
    hs = [int(np.rint(np.float64(H) / np.float64(s))) for s in scale]
    ws = [int(np.rint(np.float64(W) / np.float64(s))) for s in scale]
    for l in range(nl):
        if hs[l] < 1 or ws[l] < 1:
            raise ValueError("orb_ref.layout: level %d is empty" % l)
        if l and hs[l - 1] == 2 * hs[l] and ws[l - 1] == 2 * ws[l]:
            raise ValueError("orb_ref.layout: level %d halves level %d" % (l, l - 1))
    # OpenCV's split, in float as there
    f = np.float32(1.0 / sf)
    nd = np.float32(np.float32(np.float32(nf) * np.float32(np.float32(1) - f)) / np.float32(np.float32(1) - np.float32(math.pow(float(f), float(nl)))))
    quota, total = [], 0
    for l in range(nl - 1):
        q = cv_round(nd)
        quota.append(q)
        total += q
        nd = np.float32(nd * f)
    quota.append(max(nf - total, 0))
    off, offs = 0, []
    for l in range(nl):
        offs.append(off)
        off += (hs[l] * ws[l] + 15) & ~15
    return dict(n_levels=nl, level_h=hs, level_w=ws, quota=quota, active=[int(min(hs[l], ws[l]) > 2 * edge) for l in range(nl)],
                scale=scale, level_offset=offs, bytes_per_image=off, edge_threshold=edge, fast_threshold=thr, nfeatures=nf)


def to_bytes(img):
    """FeatureClassic::prepImg: a float image rounded half to even and clamped; a byte image as it is"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img
    return np.clip(np.rint(img.astype(np.float32)), 0, 255).astype(np.uint8)


def pyramid(img, L):
    lv = [to_bytes(img)]
    for l in range(1, L["n_levels"]):
        lv.append(img_ref.resize_linear_u8(lv[-1], L["level_h"][l], L["level_w"][l]))
    return lv


def pack(levels, L):
    out = np.zeros(L["bytes_per_image"], np.uint8)
    for l, a in enumerate(levels):
        out[L["level_offset"][l]:L["level_offset"][l] + a.size] = a.ravel()
    return out


def unpack(buf, L):
    return [buf[L["level_offset"][l]:L["level_offset"][l] + L["level_h"][l] * L["level_w"][l]].reshape(L["level_h"][l], L["level_w"][l])
            for l in range(L["n_levels"])]


def fast_scores(level, threshold):
    """byte score map of one level"""
    h, w = level.shape
    out = np.zeros((h, w), np.uint8)
    if h < 7 or w < 7:
        return out
    p = level.astype(np.int32)
    c = p[3:h - 3, 3:w - 3]
    d = np.stack([p[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in CIRCLE])
    ext = np.concatenate([d, d[:8]])
    bright = np.max(np.stack([ext[s:s + 9].min(axis=0) for s in range(16)]), axis=0) - 1
    dark = np.max(np.stack([(-ext[s:s + 9]).min(axis=0) for s in range(16)]), axis=0) - 1
    s = np.maximum(bright, dark)
    s[s < threshold] = 0
    out[3:h - 3, 3:w - 3] = s
    return out


def nms(scores, edge):
    """(ys, xs) of the candidates, ascending (y, x)"""
    h, w = scores.shape
    s = np.pad(scores.astype(np.int32), 1)
    c = s[1:-1, 1:-1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                keep &= c > s[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    inside = np.zeros_like(keep)
    if h > 2 * edge and w > 2 * edge:
        inside[edge:h - edge, edge:w - edge] = True
    ys, xs = np.nonzero(keep & inside)
    return ys.astype(np.int64), xs.astype(np.int64)


def harris(level, ys, xs):
    """float64 responses at the given pixels (at least 4 from the border)"""
    p = level.astype(np.int64)
    o = np.arange(-3, 4)
    Y = ys[:, None, None] + o[None, :, None]
    X = xs[:, None, None] + o[None, None, :]
    g = lambda dy, dx: p[Y + dy, X + dx]              # noqa: E731
    ix = 2 * (g(0, 1) - g(0, -1)) + (g(-1, 1) - g(-1, -1)) + (g(1, 1) - g(1, -1))
    iy = 2 * (g(1, 0) - g(-1, 0)) + (g(1, -1) - g(-1, -1)) + (g(1, 1) - g(-1, 1))
    a = (ix * ix).sum(axis=(1, 2))
    b = (iy * iy).sum(axis=(1, 2))
    c = (ix * iy).sum(axis=(1, 2))
    det = a * b - c * c
    tr2 = (a + b) * (a + b)
    return (det.astype(np.float64) - HARRIS_K * tr2.astype(np.float64)) * HARRIS_S4


def select_level(level, scores, quota, edge):
    """(ys, xs, responses) of one level, ascending (y, x); None when the survivors of the FAST cut exceed MAX_SURVIVORS"""
    ys, xs = nms(scores, edge)
    if quota < 1 or len(ys) == 0:
        return ys[:0], xs[:0], np.zeros(0)
    s = scores[ys, xs].astype(np.int32)
    if len(s) > 2 * quota:
        cut = np.sort(s)[::-1][2 * quota - 1]
        k = s >= cut
        ys, xs = ys[k], xs[k]
    if len(ys) > MAX_SURVIVORS:
        return None
    r = harris(level, ys, xs)
    if len(r) > quota:
        cut = np.sort(r)[::-1][quota - 1]
        k = r >= cut
        ys, xs, r = ys[k], xs[k], r[k]
    return ys, xs, r


def umax_table():
    """the half widths of the rows of the circular patch, built as OpenCV builds them"""
    umax = [0] * (HALF + 2)
    vmax = int(math.floor(HALF * math.sqrt(2.0) / 2 + 1))
    vmin = int(math.ceil(HALF * math.sqrt(2.0) / 2))
    for v in range(vmax + 1):
        umax[v] = int(np.rint(math.sqrt(float(HALF * HALF - v * v))))
    v0 = 0
    for v in range(HALF, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax[:HALF + 1]


UMAX = umax_table()
assert UMAX == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
_PU = np.array([u for v in range(-HALF, HALF + 1) for u in range(-UMAX[abs(v)], UMAX[abs(v)] + 1)], np.int64)
_PV = np.array([v for v in range(-HALF, HALF + 1) for u in range(-UMAX[abs(v)], UMAX[abs(v)] + 1)], np.int64)


def moments(level, ys, xs):
    p = level.astype(np.int64)[ys[:, None] + _PV[None, :], xs[:, None] + _PU[None, :]]
    return (p * _PU[None, :]).sum(axis=1), (p * _PV[None, :]).sum(axis=1)


def direction(m10, m01):
    """(cs, sn) float64, angle float32 degrees in [0, 360)"""
    m10 = np.asarray(m10, np.int64)
    m01 = np.asarray(m01, np.int64)
    h2 = m10 * m10 + m01 * m01
    z = h2 == 0
    r = np.sqrt(np.where(z, 1, h2).astype(np.float64))
    cs = np.where(z, 1.0, m10.astype(np.float64) / r)
    sn = np.where(z, 0.0, m01.astype(np.float64) / r)
    a = np.arctan2(m01.astype(np.float64), m10.astype(np.float64)) * RAD2DEG
    a = np.where(a < 0, a + 360.0, a).astype(np.float32)
    a[a >= np.float32(360)] = 0
    return cs, sn, a


def blur_weights():
    """7 integer weights summing to 256: rint(256 g / sum g) half to even off the centre, the centre takes the remainder"""
    g = [math.exp(-((i - 3) * (i - 3)) / (2.0 * 2.0 * 2.0)) for i in range(7)]
    s = sum(g)
    w = [int(np.rint(256.0 * v / s)) for v in g]
    w[3] = 256 - (sum(w) - w[3])
    return w


BLUR_W = blur_weights()


def blur(level):
    h, w = level.shape
    P = np.pad(level.astype(np.int64), 3, mode="reflect")
    r = sum(BLUR_W[i] * P[:, i:i + w] for i in range(7))
    v = sum(BLUR_W[j] * r[j:j + h] for j in range(7))
    return ((v + (1 << 15)) >> 16).astype(np.uint8)


def describe_level(blurred, ys, xs, cs, sn, pattern):
    """packed descriptors uint8 [m][32]"""
    pat = check_pattern(pattern).astype(np.float64)
    b = blurred.astype(np.int32)

    def at(px, py):
        ix = np.rint(px[None, :] * cs[:, None] - py[None, :] * sn[:, None]).astype(np.int64)
        iy = np.rint(px[None, :] * sn[:, None] + py[None, :] * cs[:, None]).astype(np.int64)
        return b[ys[:, None] + iy, xs[:, None] + ix]

    bits = at(pat[:, 0], pat[:, 1]) < at(pat[:, 2], pat[:, 3])
    return np.packbits(bits, axis=1, bitorder="little")


def default_pattern():
    """A BRIEF pattern: 512 points of an isotropic Gaussian (sigma = 31 / 5, a sum of 12 bytes of a linear congruential
    generator standing for the normal variate), clipped to +-13; a test whose two points coincide is drawn again.
    Integers only."""
    state = [20260101]

    def byte():
        state[0] = (state[0] * 1664525 + 1013904223) & 0xFFFFFFFF
        return state[0] >> 24

    def coord():
        g = sum(byte() for _ in range(12)) * 2 - 12 * 255          # twice the centred sum: standard deviation about 2 * 256
        num, den = g * PATCH, 2 * 256 * 5
        v = (abs(num) * 2 + den) // (2 * den)                       # nearest, halves away from zero
        v = v if num >= 0 else -v
        return max(-13, min(13, v))

    out = []
    while len(out) < 256:
        t = (coord(), coord(), coord(), coord())
        if (t[0], t[1]) != (t[2], t[3]):
            out.append(t)
    return np.array(out, np.int8).reshape(1024)


def detect_and_compute(img, K, opt=None, pattern=None):
    """One image: dict of xy [K][2] float32, xy_int, size, angle, response, octave, rows [K][32] float32, packed [K][32] uint8
    (padded as the GPU pads) and count (uncapped; -1 for an overflow), plus the lists behind them."""
    pattern = default_pattern() if pattern is None else pattern
    check_pattern(pattern)
    img = np.asarray(img)
    L = layout(img.shape[0], img.shape[1], opt)
    lv = pyramid(img, L)
    lev, ys, xs, rs = [], [], [], []
    overflow = False
    for l in range(L["n_levels"]):
        if not L["active"][l]:
            continue
        r = select_level(lv[l], fast_scores(lv[l], L["fast_threshold"]), L["quota"][l], L["edge_threshold"])
        if r is None:
            overflow = True
            break
        lev.append(np.full(len(r[0]), l, np.int64)); ys.append(r[0]); xs.append(r[1]); rs.append(r[2])
    cat = lambda a, dt: np.concatenate(a).astype(dt) if a else np.zeros(0, dt)        # noqa: E731
    lev, ys, xs, rs = cat(lev, np.int64), cat(ys, np.int64), cat(xs, np.int64), cat(rs, np.float64)
    K = max(int(K), 1)
    out = dict(xy=np.full((K, 2), -1, np.float32), xy_int=np.full((K, 2), -1, np.int32), size=np.zeros(K, np.float32), angle=np.zeros(K, np.float32),
               response=np.zeros(K, np.float32), octave=np.zeros(K, np.int32), rows=np.zeros((K, 32), np.float32), packed=np.zeros((K, 32), np.uint8))
    if overflow:
        out["count"] = -1
        return out
    out["count"] = len(lev)
    if len(lev) > K:
        order = np.lexsort((np.arange(len(lev)), -rs))[:K]
        keep = np.sort(order)
        lev, ys, xs, rs = lev[keep], ys[keep], xs[keep], rs[keep]
    m = len(lev)
    sc = np.array(L["scale"], np.float32)[lev]
    out["xy"][:m, 0] = xs.astype(np.float32) * sc
    out["xy"][:m, 1] = ys.astype(np.float32) * sc
    out["xy_int"][:m] = np.trunc(out["xy"][:m]).astype(np.int32)
    out["size"][:m] = np.float32(PATCH) * sc
    out["response"][:m] = rs.astype(np.float32)
    out["octave"][:m] = lev
    for l in sorted(set(lev.tolist())):
        k = np.nonzero(lev == l)[0]
        m10, m01 = moments(lv[l], ys[k], xs[k])
        cs, sn, ang = direction(m10, m01)
        out["angle"][k] = ang
        out["packed"][k] = describe_level(blur(lv[l]), ys[k], xs[k], cs, sn, pattern)
    out["rows"][:m] = out["packed"][:m].astype(np.float32)
    out.update(level=lev, y=ys, x=xs, response64=rs, layout=L, levels=lv)
    return out


def level_coords(xy, octave, L):
    """the integer level coordinates a describe call recovers from emitted fields: rint(float64(xy) / float64(scale))"""
    sc = np.array(L["scale"], np.float32)[octave].astype(np.float64)
    return np.rint(xy[:, 1].astype(np.float64) / sc).astype(np.int64), np.rint(xy[:, 0].astype(np.float64) / sc).astype(np.int64)


def corner_image(H, W, seed, n_rect=None, noise=2):
    """Test input: overlapping axis-parallel and rotated rectangles of random grey levels over mild noise (many FAST corners)."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 110.0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for _ in range(n_rect or max(8, H * W // 700)):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        a, b = rng.uniform(4, 26), rng.uniform(4, 26)
        t = rng.uniform(0, math.pi)
        u = (xx - cx) * math.cos(t) + (yy - cy) * math.sin(t)
        v = -(xx - cx) * math.sin(t) + (yy - cy) * math.cos(t)
        img[(np.abs(u) < a) & (np.abs(v) < b)] = rng.uniform(10, 245)
    img += rng.integers(-noise, noise + 1, size=(H, W))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
