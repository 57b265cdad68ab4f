"""CPU restatement of cv::SIFT::create()->detectAndCompute as reconstructor_amd/csrc/sift.hip computes it.

OpenCV is not available to the tests, so this file IS the contract: every constant below is written from knowledge of OpenCV
4.x's sift.dispatch.cpp / sift.simd.hpp; DESIGN.md section 1 lists what could not be pinned against the library itself.

    layout / weights            the pyramid's shape: octaves, per-layer sigmas, taps, fp32 weights, packed offsets
    pyramid                     float64 arithmetic on the identical fp32 weights and index rules (the accuracy reference)
    pyramid_f32                 the GPU's own fp32 sequence emulated exactly (fmaf chains in ascending tap order)
    candidates / keypoints      the stages behind the pyramid in float64 on any fp32 pyramid handed in
    describe                    calcSIFTDescriptor for given keypoints
    select                      duplicates, canonical order, cap

Every candidate and keypoint carries a MARGIN: the smallest distance of any of its decisions from flipping (the 0.5 tests and
cvRounds of the offsets, the contrast and edge tests, the cvRounds of radius and point, the orientation bins of samples of
non-negligible weight, the peak tests, per descriptor element the distance of the pre-rounding value from a half-integer).
Two float64 evaluations of the same formulas agree on every decision whose margin exceeds GUARD.
"""
import math
from fractions import Fraction

import numpy as np

BORDER, STEPS, NBINS = 5, 5, 36
ORI_SIG, ORI_RADIUS, PEAK_RATIO = 1.5, 4.5, 0.8
DESCR_WIDTH, DESCR_BINS, DESCR_SCL, DESCR_CLIP, INT_FCTR = 4, 8, 3.0, 0.2, 512.0
FLT_EPS = float(np.finfo(np.float32).eps)
GUARD = 1e-6
DEFAULTS = dict(S=3, contrast=0.04, edge=10.0, sigma=1.6)


def cv_round(x):
    return int(round(float(x)))          # round-half-to-even


def half_dist(x):
    """distance of x from the nearest half-integer: how far a cvRound is from flipping"""
    return abs((float(x) - math.floor(float(x))) - 0.5)


# ---- pyramid ---------------------------------------------------------------------------------------------------------

def taps_of(sigma):
    return cv_round(8.0 * sigma + 1.0) | 1


def weights(sigma, taps):
    w = [math.exp(-((i - taps // 2) ** 2) / (2.0 * sigma * sigma)) for i in range(taps)]
    s = 0.0
    for v in w:
        s += v
    return np.array([v / s for v in w], dtype=np.float64).astype(np.float32)


def layout(H, W, S=3, sigma=1.6):
    m = min(2 * H, 2 * W)
    n_oct = cv_round(math.log(float(m)) / math.log(2.0) - 2.0) + 1
    base_sigma = math.sqrt(max(sigma * sigma - 1.0, 0.01))
    k = math.pow(2.0, 1.0 / S)
    sig = [sigma]
    for i in range(1, S + 3):
        prev = math.pow(k, float(i - 1)) * sigma
        total = prev * k
        sig.append(math.sqrt(total * total - prev * prev))
    hs, ws, offs, off = [], [], [], 0
    h, w = 2 * H, 2 * W
    for _ in range(n_oct):
        if h < 1 or w < 1:
            break
        hs.append(h)
        ws.append(w)
        offs.append([off + i * h * w for i in range(S + 3)])
        off += (S + 3) * h * w
        h //= 2
        w //= 2
    return dict(n_octaves=len(hs), n_layers=S + 3, base_sigma=base_sigma, base_taps=taps_of(base_sigma), oct_h=hs, oct_w=ws,
                layer_sigma=sig, layer_taps=[0] + [taps_of(s) for s in sig[1:]], layer_offset=offs, floats_per_image=off)


def reflect101(i, n):
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def _up_index(n_dst, n_src):
    d = np.arange(n_dst)
    i0 = np.where(d & 1, (d - 1) // 2, d // 2 - 1)
    f = np.where(d & 1, 0.25, 0.75)
    lo, hi = i0 < 0, None
    f = np.where(lo, 0.0, f)
    i0 = np.where(lo, 0, i0)
    hi = i0 >= n_src - 1
    f = np.where(hi, 0.0, f)
    i0 = np.where(hi, n_src - 1, i0)
    return i0, np.minimum(i0 + 1, n_src - 1), f


def upsample2(img, dtype=np.float64):
    """INTER_LINEAR at scale 2, horizontal pass first; dtype float32 reproduces the GPU's roundings"""
    a = np.asarray(img).astype(np.float32).astype(dtype)
    H, W = a.shape
    x0, x1, fx = _up_index(2 * W, W)
    y0, y1, fy = _up_index(2 * H, H)
    fx, fy = fx.astype(dtype), fy.astype(dtype)
    one = dtype(1.0)
    h = a[:, x0] * (one - fx)[None, :] + a[:, x1] * fx[None, :]
    return h[y0, :] * (one - fy)[:, None] + h[y1, :] * fy[:, None]


def decimate(src, h, w):
    sh, sw = src.shape
    ys = np.minimum(np.floor(np.arange(h) * (sh / h)).astype(np.int64), sh - 1)
    xs = np.minimum(np.floor(np.arange(w) * (sw / w)).astype(np.int64), sw - 1)
    return src[np.ix_(ys, xs)]


def _fma32(w, s, acc):
    """float32 fma(w, s, acc), elementwise and exact: the product is exact in float64; the float64 sum is rounded once more to
    float32, which differs from the single rounding only when it lands on a float32 midpoint -- those elements are redone in
    rational arithmetic."""
    d = np.float64(w) * s.astype(np.float64) + acc.astype(np.float64)
    out = d.astype(np.float32)
    bits = d.view(np.uint64) & np.uint64((1 << 29) - 1)
    tie = np.flatnonzero(bits.ravel() == np.uint64(1 << 28))
    if tie.size:
        o, sf, af = out.ravel(), s.ravel(), acc.ravel()
        for i in tie:
            exact = Fraction(float(w)) * Fraction(float(sf[i])) + Fraction(float(af[i]))
            lo = np.nextafter(np.float32(d.ravel()[i]), np.float32(-np.inf))
            hi = np.nextafter(np.float32(d.ravel()[i]), np.float32(np.inf))
            best = min((lo, np.float32(d.ravel()[i]), hi), key=lambda c: (abs(Fraction(float(c)) - exact), int(np.float32(c).view(np.uint32)) & 1))
            o[i] = best
        out = o.reshape(out.shape)
    return out


def _pass(src, w, axis, f32):
    n = src.shape[axis]
    R = len(w) // 2
    idx = reflect101(np.arange(-R, n + R), n)
    ext = np.take(src, idx, axis=axis)
    sl = (lambda t: ext[:, t:t + n]) if axis == 1 else (lambda t: ext[t:t + n, :])
    if f32:
        acc = np.float32(w[0]) * sl(0)
        for t in range(1, len(w)):
            acc = _fma32(w[t], sl(t), acc)
        return acc
    acc = float(w[0]) * sl(0)
    for t in range(1, len(w)):
        acc = acc + float(w[t]) * sl(t)
    return acc


def blur(src, sigma, taps, f32=False):
    w = weights(sigma, taps)
    return _pass(_pass(src, w, 1, f32), w, 0, f32)       # rows first, then columns


def _pyramid(img, S, sigma, f32):
    H, W = np.asarray(img).shape
    L = layout(H, W, S, sigma)
    base = upsample2(img, np.float32 if f32 else np.float64)
    pyr = []
    for o in range(L["n_octaves"]):
        if o == 0:
            layers = [blur(base, L["base_sigma"], L["base_taps"], f32)]
        else:
            layers = [decimate(pyr[o - 1][S], L["oct_h"][o], L["oct_w"][o])]
        for i in range(1, S + 3):
            layers.append(blur(layers[i - 1], L["layer_sigma"][i], L["layer_taps"][i], f32))
        pyr.append(layers)
    return pyr


def pyramid(img, S=3, sigma=1.6):
    """list [octave][layer] of float64 arrays"""
    return _pyramid(img, S, sigma, False)


def pyramid_f32(img, S=3, sigma=1.6):
    """the float32 sequence of k_sift_blur, bit for bit"""
    return _pyramid(img, S, sigma, True)


def pyramid_bound(H, W, S=3, sigma=1.6):
    """Derived bound [octave][layer] on |fp32 pyramid - float64 pyramid|, both on the same fp32 weights (0..255 scale).
    One pass of T taps is a product and T - 1 fmas: computed = sum w_i v_i (1 + t_i) with |t_i| <= gamma_T = T u / (1 - T u),
    u = 2^-24, so the pass adds at most gamma_T * sum w_i |v_i| <= gamma_T * 255 (1 + 2^-20) -- the weights are positive and sum to 1
    within T / 2 ulp -- and hands on what its input carried, times that same sum.  A layer collects two passes per blur along
    its chain: the base blur, the layers before it in its octave, and through layer S of every octave before (the halving
    copies).  The 2x upsample adds two passes of a product, a product and a sum on weights that are exact: 2 gamma_3 * 255
    (nothing at all for byte input, where every product and sum is exact).  The float64 side errs by 1e-13 of that."""
    L = layout(H, W, S, sigma)
    u = 2.0 ** -24
    gam = lambda T: T * u / (1.0 - T * u)      # noqa: E731
    vmax, grow = 255.0 * (1.0 + 2.0 ** -20), 1.0 + 2.0 ** -20
    out = []
    for o in range(L["n_octaves"]):
        row = [(2.0 * gam(3) * vmax) * grow * grow + 2.0 * gam(L["base_taps"]) * vmax if o == 0 else out[o - 1][S]]
        for i in range(1, S + 3):
            row.append(row[i - 1] * grow * grow + 2.0 * gam(L["layer_taps"][i]) * vmax)
        out.append(row)
    return out


def pack(pyr):
    return np.concatenate([np.asarray(l).ravel() for layers in pyr for l in layers])


def unpack(flat, H, W, S=3, sigma=1.6):
    L = layout(H, W, S, sigma)
    return [[np.asarray(flat[L["layer_offset"][o][i]:L["layer_offset"][o][i] + L["oct_h"][o] * L["oct_w"][o]], dtype=np.float32)
             .reshape(L["oct_h"][o], L["oct_w"][o]) for i in range(S + 3)] for o in range(L["n_octaves"])]


# ---- behind the pyramid ----------------------------------------------------------------------------------------------

def _dogs(pyr32):
    return [[(np.asarray(l[i + 1], dtype=np.float32) - np.asarray(l[i], dtype=np.float32)) for i in range(len(l) - 1)] for l in pyr32]


def candidates(pyr32, S=3, contrast=0.04):
    """set of (octave, layer, r, c): fp32 comparisons only"""
    thr = np.float32(math.floor(0.5 * contrast / S * 255.0))
    out = []
    for o, dog in enumerate(_dogs(pyr32)):
        h, w = dog[0].shape
        if h <= 2 * BORDER or w <= 2 * BORDER:
            continue
        for l in range(1, S + 1):
            c = dog[l][BORDER:h - BORDER, BORDER:w - BORDER]
            mx = (np.abs(c) > thr) & (c > 0)
            mn = (np.abs(c) > thr) & (c < 0)
            for dl in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        u = dog[l + dl][BORDER + dy:h - BORDER + dy, BORDER + dx:w - BORDER + dx]
                        mx &= c >= u
                        mn &= c <= u
            ys, xs = np.nonzero(mx | mn)
            out += [(o, l, int(y) + BORDER, int(x) + BORDER) for y, x in zip(ys, xs)]
    return out


def _solve3(A, g):
    """x with A x = g by elimination with partial pivoting; a singular A gives 0"""
    M = [[float(A[i][j]) for j in range(3)] + [float(g[i])] for i in range(3)]
    for k in range(3):
        p = k
        for i in range(k + 1, 3):
            if abs(M[i][k]) > abs(M[p][k]):
                p = i
        if M[p][k] == 0.0:
            return [0.0, 0.0, 0.0]
        M[k], M[p] = M[p], M[k]
        for i in range(k + 1, 3):
            f = M[i][k] / M[k][k]
            for j in range(k, 4):
                M[i][j] -= f * M[k][j]
    X = [0.0, 0.0, 0.0]
    for k in (2, 1, 0):
        s = M[k][3]
        for j in range(k + 1, 3):
            s -= M[k][j] * X[j]
        X[k] = s / M[k][k]
    return X


def refine(dog, o, layer, r, c, S, contrast, edge, sigma):
    """adjustLocalExtrema.  Returns (keypoint dict or None, margin)."""
    h, w = dog[0].shape
    img_scale = 1.0 / 255.0
    d1, d2, dc = img_scale * 0.5, img_scale, img_scale * 0.25
    margin = math.inf
    it = 0
    while it < STEPS:
        D = lambda dl, dy, dx: float(dog[layer + dl][r + dy, c + dx])      # noqa: E731
        v0 = D(0, 0, 0)
        g = [(D(0, 0, 1) - D(0, 0, -1)) * d1, (D(0, 1, 0) - D(0, -1, 0)) * d1, (D(1, 0, 0) - D(-1, 0, 0)) * d1]
        v2 = v0 * 2.0
        dxx = (D(0, 0, 1) + D(0, 0, -1) - v2) * d2
        dyy = (D(0, 1, 0) + D(0, -1, 0) - v2) * d2
        dss = (D(1, 0, 0) + D(-1, 0, 0) - v2) * d2
        dxy = (D(0, 1, 1) - D(0, 1, -1) - D(0, -1, 1) + D(0, -1, -1)) * dc
        dxs = (D(1, 0, 1) - D(1, 0, -1) - D(-1, 0, 1) + D(-1, 0, -1)) * dc
        dys = (D(1, 1, 0) - D(1, -1, 0) - D(-1, 1, 0) + D(-1, -1, 0)) * dc
        X = _solve3([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]], g)
        xc, xr, xi = -X[0], -X[1], -X[2]
        big = 2147483647.0 / 3.0
        if not (abs(xi) <= big and abs(xr) <= big and abs(xc) <= big):
            return None, margin
        margin = min(margin, *(abs(0.5 - abs(v)) for v in (xi, xr, xc)))
        if abs(xi) < 0.5 and abs(xr) < 0.5 and abs(xc) < 0.5:
            break
        margin = min(margin, *(half_dist(v) for v in (xi, xr, xc)))
        c += cv_round(xc)
        r += cv_round(xr)
        layer += cv_round(xi)
        if layer < 1 or layer > S or c < BORDER or c >= w - BORDER or r < BORDER or r >= h - BORDER:
            return None, margin
        it += 1
    if it >= STEPS:
        return None, margin
    t = g[0] * xc + g[1] * xr + g[2] * xi
    contr = v0 * img_scale + t * 0.5
    margin = min(margin, abs(abs(contr) * S - contrast))
    if abs(contr) * S < contrast:
        return None, margin
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    lhs, rhs = tr * tr * edge, (edge + 1.0) * (edge + 1.0) * det
    denom = abs(dxx * dyy) + dxy * dxy
    margin = min(margin, abs(det) / denom if denom > 0 else 0.0)
    if det > 0:
        margin = min(margin, abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    if det <= 0.0 or lhs >= rhs:
        return None, margin
    po = float(1 << o)
    size = sigma * 2.0 ** ((layer + xi) / S) * po * 2.0
    return dict(o=o, layer=layer, r=r, c=c, x=(c + xc) * po, y=(r + xr) * po, size=size, response=abs(contr),
                octave=o + (layer << 8) + (cv_round((xi + 0.5) * 255.0) << 16), scl=size * 0.5 / po), margin


def orientation_hist(G, r, c, scl):
    """calcOrientationHist on Gaussian layer G (fp32 values, float64 arithmetic).  Returns (smoothed histogram, margin)."""
    h, w = G.shape
    radius = cv_round(ORI_RADIUS * scl)
    margin = half_dist(ORI_RADIUS * scl)
    es = -1.0 / (2.0 * (ORI_SIG * scl) * (ORI_SIG * scl))
    ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
    y, x = r + ii, c + jj
    ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    ii, jj, y, x = ii[ok], jj[ok], y[ok], x[ok]
    G = G.astype(np.float64)
    dx = G[y, x + 1] - G[y, x - 1]
    dy = G[y - 1, x] - G[y + 1, x]
    wgt = np.exp((ii * ii + jj * jj).astype(np.float64) * es)
    mag = np.sqrt(dx * dx + dy * dy)
    ori = np.arctan2(dy, dx) * (180.0 / math.pi)
    ori = np.where(ori < 0.0, ori + 360.0, ori)
    rb = ori * (NBINS / 360.0)
    b = np.rint(rb).astype(np.int64)
    b = np.where(b >= NBINS, b - NBINS, b)
    b = np.where(b < 0, b + NBINS, b)
    vote = wgt * mag
    raw = np.zeros(NBINS)
    np.add.at(raw, b, vote)
    if vote.size:
        # a sample that changes bin moves its vote: below 1e-7 of the largest bin that can turn no peak test outside the guard and
        # moves the angle by less than an fp32 ulp at 360 (flat regions, where dx == dy happens, vote next to nothing)
        heavy = vote > 1e-7 * max(float(raw.max()), 1e-300)
        if heavy.any():
            margin = min(margin, float(np.abs((rb[heavy] - np.floor(rb[heavy])) - 0.5).min()))
    n = NBINS
    hist = np.array([(raw[(k - 2) % n] + raw[(k + 2) % n]) * (1.0 / 16.0) + (raw[(k - 1) % n] + raw[(k + 1) % n]) * (4.0 / 16.0) + raw[k] * (6.0 / 16.0)
                     for k in range(n)])
    return hist, margin


def keypoints(pyr32, S=3, contrast=0.04, edge=10.0, sigma=1.6, cands=None):
    """The stages behind the candidates, before the selection.  Returns (list of keypoint dicts, number of unsure candidates that
    gave no keypoint).  A keypoint dict: x y size angle response (float32, first-octave correction applied), octave (packed, corrected),
    ident = (octave index, layer, r, c, peak bin), margin (of the whole chain of its candidate)."""
    dogs = _dogs(pyr32)
    if cands is None:
        cands = candidates(pyr32, S, contrast)
    out, unsure = [], 0
    for (o, l, r, c) in cands:
        kp, margin = refine(dogs[o], o, l, r, c, S, contrast, edge, sigma)
        if kp is None:
            unsure += margin <= GUARD
            continue
        hist, m2 = orientation_hist(np.asarray(pyr32[o][kp["layer"]]), kp["r"], kp["c"], kp["scl"])
        margin = min(margin, m2)
        omax = float(hist.max())
        found = []
        for j in range(NBINS):
            lft, rgt = hist[(j - 1) % NBINS], hist[(j + 1) % NBINS]
            conds = [(hist[j] - lft, hist[j] > lft), (hist[j] - rgt, hist[j] > rgt), (hist[j] - omax * PEAK_RATIO, hist[j] >= omax * PEAK_RATIO)]
            rel = [abs(d) / omax if omax > 0 else 0.0 for d, _ in conds]
            if all(t for _, t in conds):
                margin = min(margin, *rel)
                b = j + 0.5 * (lft - rgt) / (lft - 2.0 * hist[j] + rgt)
                b = NBINS + b if b < 0 else b - NBINS if b >= NBINS else b
                ang = np.float32(360.0 - (360.0 / NBINS) * b)
                if abs(ang - np.float32(360.0)) < FLT_EPS:
                    ang = np.float32(0.0)
                found.append((j, ang))
            else:
                margin = min(margin, max(m for m, (_, t) in zip(rel, conds) if not t))
        for j, ang in found:
            packed = kp["octave"]
            out.append(dict(x=np.float32(kp["x"] * 0.5), y=np.float32(kp["y"] * 0.5), size=np.float32(kp["size"] * 0.5), angle=ang,
                            response=np.float32(kp["response"]), octave=(packed & ~255) | ((packed - 1) & 255),
                            ident=(o, kp["layer"], kp["r"], kp["c"], j)))
        for k in out[len(out) - len(found):] if found else []:
            k["margin"] = margin
        if not found:
            unsure += margin <= GUARD
    return out, unsure


def select(kps, K=None):
    """Duplicates out, canonical order, cap.  Returns (emitted list, uncapped count)."""
    key = lambda k: (float(k["x"]), float(k["y"]), float(k["size"]), float(k["angle"]), float(k["response"]), int(k["octave"]),      # noqa: E731
                     k["ident"][2], k["ident"][3], (k["ident"][0] << 16) | (k["ident"][1] << 8) | k["ident"][4])
    srt = sorted(kps, key=key)
    uniq = [k for i, k in enumerate(srt) if i == 0 or k["ident"] != srt[i - 1]["ident"]]
    count = len(uniq)
    if K is not None and count > K:
        best = sorted(range(count), key=lambda i: (-float(uniq[i]["response"]), i))[:K]
        uniq = [uniq[i] for i in sorted(best)]
    return uniq, count


def describe(pyr32, x, y, size, angle, octave):
    """calcSIFTDescriptor for emitted keypoints (arrays of equal length).  Returns (rows uint8 [N][128], margins float64 [N][128]): the
    margin of an element is the distance of its pre-rounding value from a half-integer, capped by the keypoint's own cvRound margins."""
    d, n = DESCR_WIDTH, DESCR_BINS
    N = len(x)
    rows, margins = np.zeros((N, d * d * n), dtype=np.uint8), np.zeros((N, d * d * n))
    for q in range(N):
        packed = int(octave[q])
        o8, layer = packed & 255, (packed >> 8) & 255
        o8 = o8 if o8 < 128 else o8 - 256
        scale = 1.0 / float(1 << o8) if o8 >= 0 else float(1 << -o8)
        G = np.asarray(pyr32[o8 + 1][layer]).astype(np.float64)
        h, w = G.shape
        scl = float(size[q]) * scale * 0.5
        px, py = float(x[q]) * scale, float(y[q]) * scale
        ang = 360.0 - float(angle[q])
        if abs(ang - 360.0) < FLT_EPS:
            ang = 0.0
        ptx, pty = cv_round(px), cv_round(py)
        hw = DESCR_SCL * scl
        radius = cv_round(hw * 1.4142135623730951 * (d + 1) * 0.5)
        kmargin = min(half_dist(px), half_dist(py), half_dist(hw * 1.4142135623730951 * (d + 1) * 0.5))
        radius = min(radius, int(math.sqrt(float(w) * w + float(h) * h)))
        ct, st = math.cos(ang * (math.pi / 180.0)) / hw, math.sin(ang * (math.pi / 180.0)) / hw
        es, bpr = -1.0 / (d * d * 0.5), n / 360.0
        ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
        ii, jj = ii.ravel(), jj.ravel()
        c_rot, r_rot = jj * ct - ii * st, jj * st + ii * ct
        rbin, cbin = r_rot + d // 2 - 0.5, c_rot + d // 2 - 0.5
        r, c = pty + ii, ptx + jj
        ok = (rbin > -1.0) & (rbin < d) & (cbin > -1.0) & (cbin < d) & (r > 0) & (r < h - 1) & (c > 0) & (c < w - 1)
        rbin, cbin, r, c, c_rot, r_rot = rbin[ok], cbin[ok], r[ok], c[ok], c_rot[ok], r_rot[ok]
        dx = G[r, c + 1] - G[r, c - 1]
        dy = G[r - 1, c] - G[r + 1, c]
        ori = np.arctan2(dy, dx) * (180.0 / math.pi)
        ori = np.where(ori < 0.0, ori + 360.0, ori)
        mag = np.sqrt(dx * dx + dy * dy) * np.exp((c_rot * c_rot + r_rot * r_rot) * es)
        obin = (ori - ang) * bpr
        r0, c0, o0 = np.floor(rbin).astype(np.int64), np.floor(cbin).astype(np.int64), np.floor(obin).astype(np.int64)
        rbin, cbin, obin = rbin - r0, cbin - c0, obin - o0
        o0 = np.where(o0 < 0, o0 + n, o0)
        o0 = np.where(o0 >= n, o0 - n, o0)
        v_r1 = mag * rbin
        v_r0 = mag - v_r1
        v_rc11 = v_r1 * cbin
        v_rc10 = v_r1 - v_rc11
        v_rc01 = v_r0 * cbin
        v_rc00 = v_r0 - v_rc01
        v111 = v_rc11 * obin
        v110 = v_rc11 - v111
        v101 = v_rc10 * obin
        v100 = v_rc10 - v101
        v011 = v_rc01 * obin
        v010 = v_rc01 - v011
        v001 = v_rc00 * obin
        v000 = v_rc00 - v001
        hist = np.zeros((d + 2) * (d + 2) * (n + 2))
        idx = ((r0 + 1) * (d + 2) + c0 + 1) * (n + 2) + o0
        for off, v in ((0, v000), (1, v001), (n + 2, v010), (n + 3, v011), ((d + 2) * (n + 2), v100), ((d + 2) * (n + 2) + 1, v101),
                       ((d + 3) * (n + 2), v110), ((d + 3) * (n + 2) + 1, v111)):
            np.add.at(hist, idx + off, v)
        dst = np.zeros(d * d * n)
        for i in range(d):
            for j in range(d):
                b = ((i + 1) * (d + 2) + (j + 1)) * (n + 2)
                hist[b] += hist[b + n]
                hist[b + 1] += hist[b + n + 1]
                dst[(i * d + j) * n:(i * d + j + 1) * n] = hist[b:b + n]
        nrm2 = 0.0
        for v in dst:
            nrm2 += v * v
        thr = math.sqrt(nrm2) * DESCR_CLIP
        nrm2 = 0.0
        for v in dst:
            v = min(v, thr)
            nrm2 += v * v
        f = INT_FCTR / max(math.sqrt(nrm2), FLT_EPS)
        val = np.minimum(dst, thr) * f
        rows[q] = np.clip(np.rint(val), 0, 255).astype(np.uint8)
        margins[q] = np.minimum(np.abs((val - np.floor(val)) - 0.5), kmargin)
    return rows, margins


def detect_and_compute(pyr32, S=3, contrast=0.04, edge=10.0, sigma=1.6, K=None):
    """Everything behind the pyramid.  Returns a dict of arrays in canonical order (x y size angle response float32, octave int32,
    ident int32 [N][5], margin float64 [N], rows uint8 [N][128], row_margin float64 [N][128]) plus count (uncapped), candidates (list) and
    unsure (candidates below the guard that gave no keypoint)."""
    cands = candidates(pyr32, S, contrast)
    kps, unsure = keypoints(pyr32, S, contrast, edge, sigma, cands)
    kps, count = select(kps, K)
    f = lambda name, dt: np.array([k[name] for k in kps], dtype=dt)      # noqa: E731
    out = dict(x=f("x", np.float32), y=f("y", np.float32), size=f("size", np.float32), angle=f("angle", np.float32),
               response=f("response", np.float32), octave=f("octave", np.int32), ident=np.array([k["ident"] for k in kps], dtype=np.int32).reshape(-1, 5),
               margin=f("margin", np.float64), count=count, candidates=cands, unsure=int(unsure))
    out["rows"], out["row_margin"] = describe(pyr32, out["x"], out["y"], out["size"], out["angle"], out["octave"])
    return out
