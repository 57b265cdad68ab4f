"""The arithmetic contract of the image-preparation stage, in numpy and integer arithmetic throughout.

What detectFeatures does to a decoded photograph before a detector sees it (SequentialReconstructor.cpp:55-110): Utils::readImg
swaps BGR to RGB and calls reshapeImg (utils.cpp:61-98: cv::resize to at most imgMaxSize pixels on the longer side, the other
side cut down to a multiple of 8), cv::cvtColor(RGB2GRAY) follows; every feature then takes the colour under it (:98-106), a
landmark the colour of its first feature (:429-433), and the cloud is written by Utils::saveCloud (utils.cpp:205-275, :345-368).

cv::resize is restated for 8-bit data and its default INTER_LINEAR, after the plain C++ paths of OpenCV's resize.cpp:

    tables   scale = 1.0 / ((double)dst / src); for every d: f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s in
             float.  Horizontally s < 0 gives s = 0, f = 0 and s + 1 >= src gives s = src - 1, f = 0 (xmax: the first such d);
             vertically f stays and the two rows are clip(s) and clip(s + 1).  Weights rint((1.f - f) * 2048.f), rint(f * 2048.f),
             half to even, int16.
    rows     H[d] = S[s] * w0 + S[s + 1] * w1 in int32 (S[s] * 2048 from xmax on: the same number, w1 being 0 there)
    columns  ((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16), then (... + 2) >> 2, saturated to 0..255
    2 x 2    when src == 2 dst on BOTH axes INTER_LINEAR is replaced by the fast area path: (a + b + c + d + 2) >> 2
    copy     equal sizes

Error of the fixed-point resize against float64 bilinear interpolation at the same sample positions (the bound of
test_img_ref.py), in units of one grey level, for pixels p <= 255:

    the sample fractions     f is the float nearest to the double position: |f - f64| <= 2^-24 * max(1, |position|) < 2^-24 * src.
                             For src <= 4096 that is 2^-12, and a change of one fraction by e moves a bilinear value by at
                             most 255 e: 2 * 255 * 2^-12 < 0.125 for both axes.
    the weights              rint to a multiple of 1/2048 moves each weight by at most 2^-12; (1.f - f) adds at most 2^-25.  Two
                             weights per axis, pixels <= 255: 4 * 255 * 2^-12 < 0.25 for both axes (products of errors are
                             below 2^-20).
    H >> 4                   H is a multiple of 1/2048 grey levels; dropping 4 bits loses less than 16 / 2048 = 2^-7 per row,
                             weighted by b0 + b1 <= 2048 + 1: < 0.0079.
    (b * h) >> 16            b h is in units of 2^-18 grey levels (2^-11 for b, 2^-7 for h); >> 16 leaves units of 1/4 and drops
                             less than one of them, twice: < 0.5.
    (... + 2) >> 2           rounds to the nearest grey level: 0.5.

    total                    0.125 + 0.25 + 0.0079 + 0.5 + 0.5 < 1.39 grey levels.  RESIZE_BOUND = 1.39.

The truncations all round down and the last step rounds to nearest, so the typical error is well under one level; the bound is
the worst case of the roundings, not a fit to what the code gives.

Not pinned against OpenCV itself, which is not available where this was written.
"""
import math

import numpy as np

COEF_BITS = 11
ONE = 1 << COEF_BITS          # INTER_RESIZE_COEF_SCALE
RESIZE_BOUND = 1.39           # grey levels; derived above, for sources of at most 4096 pixels a side
GRAY_TABLES = {14: (4899, 9617, 1868), 15: (9798, 19235, 3735)}     # OpenCV 4.2 (the reference's build file), later releases
OUTLIER_RGB = (253, 0, 0)
CAMERA_RGB = (0, 250, 0)
VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])


def reshape_size(rows, cols, max_size):
    """Utils::reshapeImg's target size: (rows', cols', factor)."""
    rows, cols, max_size = int(rows), int(cols), int(max_size)
    if rows < 1 or cols < 1 or max_size < 1:
        raise ValueError("reshape_size: sizes must be positive")
    if rows > cols:
        if rows <= max_size:
            return rows, cols, 1.0
        c = max_size * (float(cols) / rows)
        c = c - math.fmod(c, 8.0)
        r2, c2, factor = max_size, int(c), float(max_size) / rows
    else:
        if cols <= max_size:
            return rows, cols, 1.0
        r = max_size * (float(rows) / cols)
        r = r - math.fmod(r, 8.0)
        r2, c2, factor = int(r), max_size, float(max_size) / cols
    if r2 < 1 or c2 < 1:
        raise ValueError("reshape_size: %d x %d at max_size %d leaves an empty image" % (rows, cols, max_size))
    return r2, c2, factor


def resize_tables(src, dst, horizontal=True):
    """One axis of INTER_LINEAR: (index int32 [dst], weights int16 [dst][2], xmax).  Horizontally index is the clamped left
    source pixel; vertically it is floor(f) itself (-1 .. src - 1), to be clipped together with its successor.  xmax is dst on
    the vertical axis."""
    src, dst = int(src), int(dst)
    scale = 1.0 / (float(dst) / src)
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int32)
    f = (f - s.astype(np.float32)).astype(np.float32)
    xmax = dst
    if horizontal:
        lo = s < 0
        s[lo] = 0
        f[lo] = 0
        hi = s + 1 >= src
        if hi.any():
            xmax = int(np.argmax(hi))
        s[hi] = src - 1
        f[hi] = 0
    w = np.empty((dst, 2), np.int16)
    w[:, 0] = np.rint((np.float32(1.0) - f).astype(np.float32) * np.float32(ONE)).astype(np.int16)
    w[:, 1] = np.rint(f * np.float32(ONE)).astype(np.int16)
    return s, w, xmax


def is_area_fast(src_rows, src_cols, rows, cols):
    return src_rows == 2 * rows and src_cols == 2 * cols


def resize_linear_u8(img, rows, cols):
    """cv::resize(img, Size(cols, rows)) with the default interpolation, for uint8 [H][W] or [H][W][C] interleaved."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError("resize_linear_u8: uint8 [H][W] or [H][W][C]")
    flat = img.ndim == 2
    S = (img[:, :, None] if flat else img).astype(np.int32)
    H, W = S.shape[:2]
    if (rows, cols) == (H, W):
        out = S
    elif is_area_fast(H, W, rows, cols):
        out = (S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2
    else:
        xs, xw, xmax = resize_tables(W, cols, True)
        ys, yw, _ = resize_tables(H, rows, False)
        x1 = np.minimum(xs + 1, W - 1)                      # never read from xmax on: its weight is 0 there
        Hh = S[:, xs] * xw[None, :, 0, None].astype(np.int32) + S[:, x1] * xw[None, :, 1, None].astype(np.int32)
        Hh[:, xmax:] = S[:, xs[xmax:]] * ONE
        r0 = np.clip(ys, 0, H - 1)
        r1 = np.clip(ys + 1, 0, H - 1)
        b0 = yw[:, 0].astype(np.int32)[:, None, None]
        b1 = yw[:, 1].astype(np.int32)[:, None, None]
        v = ((b0 * (Hh[r0] >> 4)) >> 16) + ((b1 * (Hh[r1] >> 4)) >> 16)
        out = np.clip((v + 2) >> 2, 0, 255)
    out = out.astype(np.uint8)
    return out[:, :, 0] if flat else out


def resize_bilinear_f64(img, rows, cols):
    """Float64 bilinear interpolation at the sample positions of resize_tables (the double positions, clamped as the tables
    clamp them): what the fixed-point path approximates.  Not part of the contract."""
    img = np.asarray(img)
    flat = img.ndim == 2
    S = (img[:, :, None] if flat else img).astype(np.float64)
    H, W = S.shape[:2]

    def axis(src, dst):
        p = (np.arange(dst) + 0.5) * (1.0 / (float(dst) / src)) - 0.5
        s = np.floor(p)
        return s.astype(np.int64), p - s

    xs, fx = axis(W, cols)
    ys, fy = axis(H, rows)
    fx = np.where((xs < 0) | (xs + 1 >= W), 0.0, fx)
    xs = np.clip(xs, 0, W - 1)
    x1 = np.minimum(xs + 1, W - 1)
    Hh = S[:, xs] * (1 - fx)[None, :, None] + S[:, x1] * fx[None, :, None]
    r0, r1 = np.clip(ys, 0, H - 1), np.clip(ys + 1, 0, H - 1)
    out = Hh[r0] * (1 - fy)[:, None, None] + Hh[r1] * fy[:, None, None]
    return out[:, :, 0] if flat else out


def rgb_to_gray_u8(rgb, bits=14):
    """cv::cvtColor(RGB2GRAY) on uint8 [..][3] in the order red, green, blue."""
    if bits not in GRAY_TABLES:
        raise ValueError("rgb_to_gray_u8: bits must be 14 or 15")
    r2y, g2y, b2y = GRAY_TABLES[bits]
    p = np.asarray(rgb).astype(np.int32)
    return ((r2y * p[..., 0] + g2y * p[..., 1] + b2y * p[..., 2] + (1 << (bits - 1))) >> bits).astype(np.uint8)


def prepare(src, order="bgr", max_size=512, bits=14):
    """detectFeatures' chain on one decoded image: (rgb [rows'][cols'][3], grey [rows'][cols'], factor).  A single-channel
    source is readGrayImg + reshapeImg: (None, the resized plane, factor)."""
    src = np.asarray(src)
    if order not in ("rgb", "bgr"):
        raise ValueError("prepare: order must be 'rgb' or 'bgr'")
    rows, cols, factor = reshape_size(src.shape[0], src.shape[1], max_size)
    if src.ndim == 2:
        return None, resize_linear_u8(src, rows, cols), factor
    if order == "bgr":
        src = src[:, :, ::-1]
    rgb = resize_linear_u8(np.ascontiguousarray(src), rows, cols)
    return rgb, rgb_to_gray_u8(rgb, bits), factor


def feat_colors(rgb, xy_int, count):
    """rgb[y, x] as (red, green, blue, 0) for the first min(count, K) rows of xy_int [K][2] = (x, y); zero bytes for the rest
    and for coordinates outside the image."""
    rgb = np.asarray(rgb)
    xy = np.asarray(xy_int)
    K = xy.shape[0]
    out = np.zeros((K, 4), np.uint8)
    for k in range(min(max(int(count), 0), K)):
        x, y = int(xy[k, 0]), int(xy[k, 1])
        if 0 <= x < rgb.shape[1] and 0 <= y < rgb.shape[0]:
            out[k, :3] = rgb[y, x]
    return out


def landmark_colors(feat_rgba, first_img, first_feat):
    """A landmark takes the colour of its first feature: feat_rgba [n][K][4]; an index out of range gives zero bytes."""
    feat_rgba = np.asarray(feat_rgba)
    n, K = feat_rgba.shape[:2]
    out = np.zeros((len(first_img), 4), np.uint8)
    for l, (i, k) in enumerate(zip(first_img, first_feat)):
        if 0 <= i < n and 0 <= k < K:
            out[l] = feat_rgba[i, k]
    return out


def camera_centres(poses34):
    """-R^T t in float64: each component of R^T t one ascending dot product over the three rows, products rounded before they
    are added, then negated."""
    P = np.asarray(poses34, np.float64).reshape(-1, 3, 4)
    out = np.empty((len(P), 3), np.float64)
    for j in range(3):
        acc = P[:, 0, j] * P[:, 0, 3]
        acc = acc + P[:, 1, j] * P[:, 1, 3]
        acc = acc + P[:, 2, j] * P[:, 2, 3]
        out[:, j] = -acc
    return out


def cloud_vertices(xyz, lm_rgb, inlier, poses34):
    """Utils::saveCloud's vertices as records of VERTEX_DTYPE.  With flags: the L landmarks with outliers painted (253, 0, 0),
    the same L landmarks in their own colours, one vertex per camera (0, 250, 0); without: the landmarks, then the cameras.
    lm_rgb is [L][3] or [L][4] (the fourth byte is ignored); alpha is 255."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    rgb = np.asarray(lm_rgb, np.uint8)
    rgb = rgb.reshape(len(xyz), rgb.shape[-1] if rgb.ndim > 1 else 3)[:, :3]
    L = len(xyz)
    cen = camera_centres(poses34)
    C = len(cen)
    v = np.zeros(((2 if inlier is not None else 1) * L + C,), VERTEX_DTYPE)
    v["alpha"] = 255

    def put(at, pos, col):
        sl = slice(at, at + len(pos))
        p32 = pos.astype(np.float32)
        v["x"][sl], v["y"][sl], v["z"][sl] = p32[:, 0], p32[:, 1], p32[:, 2]
        v["red"][sl], v["green"][sl], v["blue"][sl] = col[:, 0], col[:, 1], col[:, 2]

    at = 0
    if inlier is not None:
        ok = np.asarray(inlier).astype(bool)
        put(0, xyz, np.where(ok[:, None], rgb, np.asarray(OUTLIER_RGB, np.uint8)[None, :]))
        at = L
    put(at, xyz, rgb)
    put(at + L, cen, np.tile(np.asarray(CAMERA_RGB, np.uint8), (C, 1)))
    return v


def read_ply(path):
    """A PLY file of vertex records (ASCII or binary_little_endian, the seven properties of VERTEX_DTYPE in order) back as
    records: the parser the tests read rcn_cloud_write_ply's files with."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] in ("format ascii 1.0", "format binary_little_endian 1.0")
    assert lines[2].startswith("element vertex ")
    n = int(lines[2].split()[2])
    props = [l.split()[1:] for l in lines[3:] if l.startswith("property ")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"], ["uchar", "alpha"]]
    assert [l for l in lines[3:] if l and not l.startswith("property ")] == ["end_header"]
    if lines[1] == "format ascii 1.0":
        v = np.zeros(n, VERTEX_DTYPE)
        rows = raw[end:].decode("ascii").split("\n")
        assert len(rows) == n + 1 and rows[-1] == ""
        for i, row in enumerate(rows[:n]):
            t = row.split()
            assert len(t) == 7
            v[i] = (np.float32(t[0]), np.float32(t[1]), np.float32(t[2]), int(t[3]), int(t[4]), int(t[5]), int(t[6]))
        return v
    assert len(raw) - end == n * VERTEX_DTYPE.itemsize
    return np.frombuffer(raw, VERTEX_DTYPE, n, end).copy()
