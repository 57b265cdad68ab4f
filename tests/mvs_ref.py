"""The contract of the plane sweep (reconstructor_amd/csrc/mvs.hip, csrc/mvs_geom.h) in numpy: what the GPU must
equal bit for bit.

Every sum over a window is an integer sum (int64, exact in any order); every floating-point step is one numpy operation on float64
arrays -- a separately rounded IEEE double -- in the order mvs_geom.h writes it.  Cameras: poses34 rows of [R | t] (world -> camera),
intrinsics rows of six (fx fy cx cy k1 k2); the sweep, the check and the fusion read the first four (pinhole), undistort all six.

    inv_depths       the uniform-in-inverse-depth plane list over [near, far]
    homographies     H[s][k] = K_s (R_rel + t_rel e3^T inv[k]) K_r^-1, K_r^-1 in closed form
    warp / sample    the one sample per (pixel, plane, source): 1/32-pixel position, 5-bit bilinear blend, 0 .. 255 * 1024
    sweep_view       ZNCC cost over (2R + 1)^2 windows, mean over the valid sources, argmin, parabola -> plane, depth, cost
    sweep            a batch of views
    consistency      lift, project, compare with the source's own map -> mask, counts
    fuse             kept pixels of every stride-th row and column as vertices in (view, y, x) order, whole rows within a capacity
    undistort        the resample that removes k1, k2
    dense_cloud      the chain
"""
import numpy as np

SUB = 32
VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
DEFAULTS = dict(radius=3, min_sources=2, min_consistent=2, stride=1, max_cost=0.5, rel_tol=0.01)


def inv_depths(near, far, D):
    lo, hi = np.float64(1.0) / np.float64(far), np.float64(1.0) / np.float64(near)
    t = np.arange(D, dtype=np.float64) / np.float64(D - 1) if D > 1 else np.array([0.5])
    return lo + (hi - lo) * t


def homography(Pr, Kr, Ps, Ks, inv):
    """One H (9 doubles, row-major) for the plane z = 1 / inv of the reference frame."""
    Pr, Ps = np.asarray(Pr, np.float64).reshape(3, 4), np.asarray(Ps, np.float64).reshape(3, 4)
    Kr, Ks, inv = np.asarray(Kr, np.float64), np.asarray(Ks, np.float64), np.float64(inv)
    M = np.zeros((3, 3))
    for i in range(3):
        rrel = [(Ps[i, 0] * Pr[j, 0] + Ps[i, 1] * Pr[j, 1]) + Ps[i, 2] * Pr[j, 2] for j in range(3)]
        trel = Ps[i, 3] - ((rrel[0] * Pr[0, 3] + rrel[1] * Pr[1, 3]) + rrel[2] * Pr[2, 3])
        M[i] = [rrel[0], rrel[1], rrel[2] + trel * inv]
    G = np.zeros((3, 3))
    for j in range(3):
        G[0, j] = Ks[0] * M[0, j] + Ks[2] * M[2, j]
        G[1, j] = Ks[1] * M[1, j] + Ks[3] * M[2, j]
        G[2, j] = M[2, j]
    H = np.zeros((3, 3))
    for i in range(3):
        H[i, 0] = G[i, 0] / Kr[0]
        H[i, 1] = G[i, 1] / Kr[1]
        H[i, 2] = (G[i, 2] - (G[i, 0] * Kr[2]) / Kr[0]) - (G[i, 1] * Kr[3]) / Kr[1]
    return H.reshape(9)


def homographies(poses34, intrinsics, ref, srcs, inv):
    """[S][D][9]; zeros for a source < 0."""
    poses34, intrinsics = np.asarray(poses34, np.float64).reshape(-1, 12), np.asarray(intrinsics, np.float64).reshape(-1, 6)
    out = np.zeros((len(srcs), len(inv), 9))
    for s, src in enumerate(srcs):
        if src < 0:
            continue
        assert src != ref, "a reference listed as its own source"
        for k, v in enumerate(inv):
            out[s, k] = homography(poses34[ref], intrinsics[ref], poses34[src], intrinsics[src], v)
    return out


def _quantise(u, v, rows, cols):
    with np.errstate(invalid="ignore", over="ignore"):
        fu, fv = np.floor(u * np.float64(SUB) + 0.5), np.floor(v * np.float64(SUB) + 0.5)
        ok = (fu >= 0) & (fu <= SUB * (cols - 1)) & (fv >= 0) & (fv <= SUB * (rows - 1))
    return np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64), ok


def warp(H, rows, cols):
    """(qu, qv, valid) of every reference pixel behind H."""
    ys, xs = np.mgrid[0:rows, 0:cols].astype(np.float64)
    with np.errstate(all="ignore"):
        w = (H[6] * xs + H[7] * ys) + H[8]
        u = ((H[0] * xs + H[1] * ys) + H[2]) / w
        v = ((H[3] * xs + H[4] * ys) + H[5]) / w
    qu, qv, ok = _quantise(u, v, rows, cols)
    return qu, qv, ok & (w > 0)


def sample(img, qu, qv):
    """The integer blend of a [rows][cols] uint8 plane at 1/32-pixel positions: int64 in 0 .. 255 * 1024."""
    rows, cols = img.shape
    p = img.astype(np.int64)
    x0, y0, wx, wy = qu >> 5, qv >> 5, qu & 31, qv & 31
    x1, y1 = np.minimum(x0 + 1, cols - 1), np.minimum(y0 + 1, rows - 1)
    top = (SUB - wx) * p[y0, x0] + wx * p[y0, x1]
    bot = (SUB - wx) * p[y1, x0] + wx * p[y1, x1]
    return (SUB - wy) * top + wy * bot


def _box(a, R):
    """Sums over the (2R + 1)^2 window around every pixel whose window lies inside; 0 elsewhere.  int64."""
    rows, cols = a.shape
    out = np.zeros((rows, cols), np.int64)
    w = 2 * R + 1
    if rows < w or cols < w:
        return out
    c = np.zeros((rows + 1, cols + 1), np.int64)
    c[1:, 1:] = a.astype(np.int64).cumsum(0).cumsum(1)
    out[R:rows - R, R:cols - R] = c[w:, w:] - c[:-w, w:] - c[w:, :-w] + c[:-w, :-w]
    return out


def cost_volume(gray, ref, srcs, H, R, min_sources):
    """float64 [D][rows][cols]: the plane costs of one view (+inf: fewer than min_sources valid sources)."""
    a = gray[ref].astype(np.int64)
    rows, cols = a.shape
    n = (2 * R + 1) ** 2
    D = H.shape[1]
    Sa, Saa = _box(a, R), _box(a * a, R)
    Va = n * Saa - Sa * Sa
    inwin = np.zeros((rows, cols), bool)
    if rows > 2 * R and cols > 2 * R:
        inwin[R:rows - R, R:cols - R] = True
    vol = np.full((D, rows, cols), np.inf)
    for k in range(D):
        tot, cnt = np.zeros((rows, cols)), np.zeros((rows, cols), np.int64)
        for s, src in enumerate(srcs):                     # source order: the costs are added in it
            if src < 0:
                continue
            qu, qv, ok = warp(H[s, k], rows, cols)
            b = np.where(ok, sample(gray[src], qu, qv), 0)
            Sb, Sbb, Sab, nv = _box(b, R), _box(b * b, R), _box(a * b, R), _box(ok.astype(np.int64), R)
            Vb = n * Sbb - Sb * Sb
            A = n * Sab - Sa * Sb
            good = inwin & (nv == n) & (Va > 0) & (Vb > 0)
            with np.errstate(all="ignore"):
                c = 1.0 - A.astype(np.float64) / np.sqrt(Va.astype(np.float64) * Vb.astype(np.float64))
            tot = np.where(good, tot + np.where(good, c, 0.0), tot)
            cnt += good
        with np.errstate(all="ignore"):
            vol[k] = np.where((cnt >= min_sources) & (cnt > 0), tot / cnt.astype(np.float64), np.inf)
    return vol


def refine(vol, plane, inv):
    """The refined inverse depth of every pixel with plane >= 0 (float64 [rows][cols], inv[plane] where no parabola applies)."""
    D = vol.shape[0]
    inv = np.asarray(inv, np.float64)
    k = np.maximum(plane.astype(np.int64), 0)
    take = lambda kk: np.take_along_axis(vol, np.clip(kk, 0, D - 1)[None], 0)[0]
    c0, cm, cp = take(k), take(k - 1), take(k + 1)
    have = (k > 0) & np.isfinite(cm) & (k + 1 < D) & np.isfinite(cp)
    inv0, invm, invp = inv[k], inv[np.clip(k - 1, 0, D - 1)], inv[np.clip(k + 1, 0, D - 1)]
    with np.errstate(all="ignore"):
        den = (cm - 2.0 * c0) + cp
        off = (0.5 * (cm - cp)) / den
        off = np.where(off > 0.5, 0.5, np.where(off < -0.5, -0.5, off))
        use = have & (den > 0)
        r = np.where(use & (off > 0), inv0 + off * (invp - inv0), np.where(use & (off < 0), inv0 + off * (inv0 - invm), inv0))
    return r


def sweep_view(gray, ref, srcs, H, inv, radius=3, min_sources=2, max_cost=0.5, **_):
    """(plane int16, depth float32, cost float32) of one reference view; H [S][D][9], inv [D]."""
    vol = cost_volume(gray, ref, srcs, H, radius, min_sources)
    plane = vol.argmin(0)                                  # the first of equal minima: ties to the lowest plane
    best = np.take_along_axis(vol, plane[None], 0)[0]
    valid = np.isfinite(best) & ~(best > max_cost)
    plane = np.where(valid, plane, -1).astype(np.int16)
    with np.errstate(all="ignore"):
        depth = np.where(valid, 1.0 / refine(vol, plane, inv), 0.0).astype(np.float32)
    cost = np.where(valid, best, np.inf).astype(np.float32)
    return plane, depth, cost


def view_homographies(poses34, intrinsics, views, inv):
    """[V][S][D][9] for views [V][1 + S] and inv [V][D]."""
    return np.stack([homographies(poses34, intrinsics, int(v[0]), [int(s) for s in v[1:]], inv[i]) for i, v in enumerate(views)])


def sweep(gray, views, H, inv, **opt):
    outs = [sweep_view(gray, int(v[0]), [int(s) for s in v[1:]], H[i], inv[i], **opt) for i, v in enumerate(views)]
    return tuple(np.stack([o[j] for o in outs]) for j in range(3))


def lift(P, K, depth):
    """World points [rows][cols][3] of a depth map (float32 depths widened to float64)."""
    P, K = np.asarray(P, np.float64), np.asarray(K, np.float64)
    rows, cols = depth.shape
    ys, xs = np.mgrid[0:rows, 0:cols].astype(np.float64)
    z = depth.astype(np.float64)
    d0 = ((xs - K[2]) / K[0]) * z - P[3]
    d1 = ((ys - K[3]) / K[1]) * z - P[7]
    d2 = z - P[11]
    return np.stack([(P[i] * d0 + P[4 + i] * d1) + P[8 + i] * d2 for i in range(3)], -1)


def project(P, K, X):
    P, K = np.asarray(P, np.float64), np.asarray(K, np.float64)
    l = [((P[4 * i] * X[..., 0] + P[4 * i + 1] * X[..., 1]) + P[4 * i + 2] * X[..., 2]) + P[4 * i + 3] for i in range(3)]
    with np.errstate(all="ignore"):
        u = K[0] * (l[0] / l[2]) + K[2]
        v = K[1] * (l[1] / l[2]) + K[3]
    return u, v, l[2]


def consistency(views, poses34, intrinsics, plane, depth, rel_tol=0.01, min_consistent=2, **_):
    """(mask uint8 [V][rows][cols], counts int32 [V]).  A source that is no reference view of the batch agrees with nothing; an image
    swept twice answers with its first map."""
    views = np.asarray(views).reshape(len(plane), -1)
    poses34, intrinsics = np.asarray(poses34, np.float64).reshape(-1, 12), np.asarray(intrinsics, np.float64).reshape(-1, 6)
    V, rows, cols = plane.shape
    view_of = {}
    for i, v in enumerate(views):
        view_of.setdefault(int(v[0]), i)
    mask = np.zeros((V, rows, cols), np.uint8)
    for i, v in enumerate(views):
        ref = int(v[0])
        X = lift(poses34[ref], intrinsics[ref], depth[i])
        agree = np.zeros((rows, cols), np.int64)
        for src in v[1:]:
            src = int(src)
            if src < 0 or src not in view_of:
                continue
            sv = view_of[src]
            u, w, z = project(poses34[src], intrinsics[src], X)
            with np.errstate(all="ignore"):
                fu, fv = np.floor(u + 0.5), np.floor(w + 0.5)
                ok = (z > 0) & (fu >= 0) & (fu <= cols - 1) & (fv >= 0) & (fv <= rows - 1)
                iu, iv = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
                ok &= plane[sv][iv, iu] >= 0
                ok &= np.abs(z - depth[sv][iv, iu].astype(np.float64)) <= np.float64(rel_tol) * z
            agree += ok
        mask[i] = (plane[i] >= 0) & (agree >= min_consistent)
    return mask, mask.reshape(V, -1).sum(1).astype(np.int32)


def fuse(views, poses34, intrinsics, rgb, depth, mask, stride=1, capacity=None, **_):
    """(vertices VERTEX_DTYPE [written], (written, total)): the kept pixels of rows / columns 0, stride, ... in (view, y, x) order; row j
    of the sampled rows is written iff rows 0 .. j fit the capacity.  rgb [n][rows][cols][3] or None (black)."""
    views = np.asarray(views).reshape(len(mask), -1)
    poses34, intrinsics = np.asarray(poses34, np.float64).reshape(-1, 12), np.asarray(intrinsics, np.float64).reshape(-1, 6)
    out, written, total = [], 0, 0
    for i, v in enumerate(views):
        ref = int(v[0])
        X = lift(poses34[ref], intrinsics[ref], depth[i]).astype(np.float32)
        for y in range(0, mask.shape[1], stride):
            xs = np.arange(0, mask.shape[2], stride)
            xs = xs[mask[i, y, xs] != 0]
            total += len(xs)
            if capacity is not None and total > capacity:
                continue                                   # the totals ascend: every later row is refused too
            rec = np.zeros(len(xs), VERTEX_DTYPE)
            rec["x"], rec["y"], rec["z"] = X[y, xs, 0], X[y, xs, 1], X[y, xs, 2]
            if rgb is not None:
                rec["red"], rec["green"], rec["blue"] = rgb[ref, y, xs, 0], rgb[ref, y, xs, 1], rgb[ref, y, xs, 2]
            rec["alpha"] = 255
            out.append(rec)
            written = total
    return (np.concatenate(out) if out else np.zeros(0, VERTEX_DTYPE)), (written, total)


def undistort(img, K6):
    """One image [rows][cols] or [rows][cols][3] through the additive model; K6 = fx fy cx cy k1 k2."""
    K = np.asarray(K6, np.float64)
    rows, cols = img.shape[:2]
    ys, xs = np.mgrid[0:rows, 0:cols].astype(np.float64)
    with np.errstate(all="ignore"):
        xn, yn = (xs - K[2]) / K[0], (ys - K[3]) / K[1]
        rho = xn * xn + yn * yn
        d = K[4] * rho + (K[5] * rho) * rho
        u, v = K[0] * (xn + d) + K[2], K[1] * (yn + d) + K[3]
    qu, qv, ok = _quantise(u, v, rows, cols)
    planes = img.reshape(rows, cols, -1)
    out = np.stack([np.where(ok, (sample(planes[..., c], qu, qv) + 512) >> 10, 0) for c in range(planes.shape[2])], -1).astype(np.uint8)
    return out.reshape(img.shape)


def dense_cloud(poses34, intrinsics, gray, rgb, views, inv, capacity=None, **opt):
    """undistort -> sweep -> consistency -> fuse; returns dict(gray, rgb, H, plane, depth, cost, mask, counts, vertices, written, total)."""
    o = dict(DEFAULTS, **opt)
    intrinsics = np.asarray(intrinsics, np.float64).reshape(-1, 6)
    g = np.stack([undistort(gray[i], intrinsics[i]) for i in range(len(gray))])
    c = None if rgb is None else np.stack([undistort(rgb[i], intrinsics[i]) for i in range(len(rgb))])
    H = view_homographies(poses34, intrinsics, views, inv)
    plane, depth, cost = sweep(g, views, H, inv, **o)
    mask, counts = consistency(views, poses34, intrinsics, plane, depth, **o)
    vert, (written, total) = fuse(views, poses34, intrinsics, c, depth, mask, stride=o["stride"], capacity=capacity)
    return dict(gray=g, rgb=c, H=H, plane=plane, depth=depth, cost=cost, mask=mask, counts=counts, vertices=vert, written=written, total=total)


def all_views(n, S):
    """views [n][1 + S]: every image a reference, its sources the next images in a ring, padded with -1."""
    out = np.full((n, 1 + S), -1, np.int32)
    for i in range(n):
        out[i, 0] = i
        others = [(i + 1 + j) % n for j in range(n - 1)][:S]
        out[i, 1:1 + len(others)] = others
    return out


# ---- the cases the tests share ---------------------------------------------------------------------------------------------------

def wall_case(kind="fronto", n=4, rows=72, cols=96, D=32):
    """The ray-cast scene of DESIGN.md section 32: four 96 x 72 views (f = 100, baselines about 0.35, a few hundredths of a radian of
    rotation) of a plane textured with twelve sinusoids; D planes uniform in inverse depth over 1/8 .. 1/3.  'fronto': the wall lies
    exactly on plane 13 of camera 0; 'slanted': 0.25 x + 0.1 y + z = 5.  Returns (scene dict of synth_mvs.wall_scene, inv [D])."""
    from reconstructor_amd import synth_mvs
    inv = inv_depths(3.0, 8.0, D)
    normal, d = ((0.0, 0.0, 1.0), float(1.0 / inv[13])) if kind == "fronto" else ((0.25, 0.1, 1.0), 5.0)
    return synth_mvs.wall_scene(n, rows, cols, 100.0, normal, d), inv


def true_depths(sc, view):
    from reconstructor_amd import synth_mvs
    rows, cols = sc["gray"].shape[1:]
    return synth_mvs.wall_depths(sc["poses34"][view], sc["intrinsics"][view], rows, cols, sc["normal"], sc["d"])


def true_planes(sc, inv, view=0):
    """The plane nearest in inverse depth to the true surface, per pixel."""
    return np.abs(1.0 / true_depths(sc, view)[..., None] - np.asarray(inv)[None, None]).argmin(-1)


def small_case(rows, cols, n=3, D=5, seed=0, f=30.0, near=3.0, far=8.0, d=5.0):
    """A small ray-cast wall for shape tests: n views of rows x cols."""
    from reconstructor_amd import synth_mvs
    sc = synth_mvs.wall_scene(n, rows, cols, f, (0.1, -0.05, 1.0), d, seed=seed, baseline=0.3)
    return sc, inv_depths(near, far, D)


def session_views(n_cams, obs_pt, obs_cam, points, poses34, S):
    """(sources int32 [n_cams][S], range float64 [n_cams][2], shared-landmark counts int32 [n_cams][n_cams]) from a session's graph:
    a landmark counts once per distinct camera of its track; sources by count descending, ties to the lower index, -1 where fewer
    share any; the range over the positive depths ((P[8] X + P[9] Y) + P[10] Z) + P[11], (0, 0) when there is none."""
    poses34, points = np.asarray(poses34, np.float64).reshape(-1, 12), np.asarray(points, np.float64).reshape(-1, 3)
    cams_of = [set() for _ in range(len(points))]
    for p, c in zip(obs_pt, obs_cam):
        cams_of[int(p)].add(int(c))
    cov = np.zeros((n_cams, n_cams), np.int32)
    rng = np.zeros((n_cams, 2))
    lo, hi = np.full(n_cams, np.inf), np.zeros(n_cams)
    for j, cs in enumerate(cams_of):
        X = points[j]
        for a in cs:
            for b in cs:
                cov[a, b] += 1
            P = poses34[a]
            z = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11]
            if z > 0 and np.isfinite(z):
                lo[a], hi[a] = min(lo[a], z), max(hi[a], z)
    src = np.full((n_cams, S), -1, np.int32)
    for c in range(n_cams):
        order = sorted((d for d in range(n_cams) if d != c and cov[c, d] > 0), key=lambda d: (-cov[c, d], d))[:S]
        src[c, :len(order)] = order
        if hi[c] > 0:
            rng[c] = lo[c], hi[c]
    return src, rng, cov
