"""CPU restatement of batched P3P-RANSAC view registration with refit (csrc/pnp.hip), for the tests only.

The kernel's arithmetic is + - * / sqrt on separately rounded IEEE doubles in one fixed order; every function below states
that order once, and runs either on Python floats (one entry at a time) or on numpy arrays (element-wise over the entries:
the same IEEE operations, so the same bits).  No numpy reduction is used anywhere: sums are written out.

pnp_ransac(..., literal=True)    the sequential loop of the canonical algorithm: one iteration at a time, one entry at a
                                 time, Python floats.
pnp_ransac(..., literal=False)   the kernel's structure: rounds of B hypotheses (draw, solve, score with numpy over the
                                 entries, accept in iteration order, discard what lies behind the stopping point).
Both give the same mask, count, iteration count and poses, bit for bit, for every B.
"""
import math

import numpy as np

DEFAULT_OPTIONS = dict(max_projection_error=4.0, confidence=0.99, max_iterations=10000, refine_iterations=20)
P3P_BISECT = 80         # bisection steps on the resolvent cubic
P3P_CUBIC_NEWTON = 3    # guarded Newton steps on the resolvent cubic after the bisection
P3P_QUARTIC_NEWTON = 2  # guarded Newton steps on the quartic per root
CHUNK = 8               # entries per chunk of the refit's sums
LAMBDA0 = 1e-3
DBL_MIN = 2.2250738585072014e-308


def default_options():
    return dict(DEFAULT_OPTIONS)


# ---- IEEE helpers (Python raises where IEEE returns inf / nan) -------------------------------------------------------

def _div(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.divide(a, b)
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(a):
    if isinstance(a, np.ndarray):
        return np.sqrt(a)
    return math.nan if (a != a or a < 0.0) else math.sqrt(a)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _finite(x):
    return x - x == 0.0


class RNG:
    """cv::RNG (fmat.hip rng_next)."""

    def __init__(self):
        self.s = (1 << 64) - 1

    def next(self):
        self.s = ((self.s & 0xFFFFFFFF) * 4164903690 + (self.s >> 32)) & ((1 << 64) - 1)
        return self.s & 0xFFFFFFFF


def update_num_iters(p, ep, model_points, max_iters):
    """RANSACUpdateNumIters (fmat.hip update_num_iters)."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))


def draw_sample(rng, n):
    """4 distinct entry indices, each next() % n, redrawn while equal to an earlier one."""
    idx = []
    while len(idx) < 4:
        i = rng.next() % n
        if i not in idx:
            idx.append(i)
    return idx


# ---- camera ---------------------------------------------------------------------------------------------------------

def bearing(K, u, v):
    """Camera.h:79-93 unprojection of the pixel, normalised."""
    x = _div(u - K[2], K[0])
    y = _div(v - K[3], K[1])
    radius = x * x + y * y
    d = K[4] * radius + (K[5] * radius) * radius
    x = x - d
    y = y - d
    nrm = _sqrt((x * x + y * y) + 1.0)
    return [_div(x, nrm), _div(y, nrm), _div(1.0, nrm)]


def project(P, K, X0, X1, X2):
    """camgeom.h: P X, divide, additive distortion, K.  Returns (u, v, l, x, y, radius, R X) for the refit's Jacobian."""
    W = [(P[4 * i] * X0 + P[4 * i + 1] * X1) + P[4 * i + 2] * X2 for i in range(3)]
    l = [W[i] + P[4 * i + 3] for i in range(3)]
    x, y = _div(l[0], l[2]), _div(l[1], l[2])
    radius = x * x + y * y
    d = K[4] * radius + (K[5] * radius) * radius
    xd = x + d
    yd = y + d
    return K[0] * xd + K[2], K[1] * yd + K[3], l, x, y, radius, W


def reproj_sq(P, K, X0, X1, X2, ox, oy):
    """camgeom.h reproj_sq: squared L2 reprojection error in double."""
    u, v = project(P, K, X0, X1, X2)[:2]
    du = u - ox
    dv = v - oy
    return du * du + dv * dv


# ---- P3P ------------------------------------------------------------------------------------------------------------

def _frame(A0, A1, A2):
    e1 = [A1[i] - A0[i] for i in range(3)]
    n1 = _sqrt(_dot(e1, e1))
    e1 = [_div(e1[i], n1) for i in range(3)]
    d2 = [A2[i] - A0[i] for i in range(3)]
    e3 = _cross(e1, d2)
    n3 = _sqrt(_dot(e3, e3))
    e3 = [_div(e3[i], n3) for i in range(3)]
    e2 = _cross(e3, e1)
    return e1, e2, e3


def _cubic(m, c2, c1, c0):
    return ((m + c2) * m + c1) * m + c0


def _quartic(x, b3, b2, b1, b0):
    return (((x + b3) * x + b2) * x + b1) * x + b0


def p3p(f, P):
    """Grunert's quartic in v = s3 / s1, solved by Ferrari's method: the positive root of the resolvent cubic by a fixed
    number of bisection steps from the Cauchy bound plus guarded Newton steps, two quadratics, guarded Newton steps on the
    quartic; then the rigid motion between the two triangles from their orthonormal frames.  f: three unit bearings,
    P: three world points.  Returns the poses (12 floats, rows of [R | t]) with three positive depths, in solver order."""
    d12 = [P[1][i] - P[2][i] for i in range(3)]
    d02 = [P[0][i] - P[2][i] for i in range(3)]
    d01 = [P[0][i] - P[1][i] for i in range(3)]
    a2, b2, c2 = _dot(d12, d12), _dot(d02, d02), _dot(d01, d01)
    if a2 == 0.0 or b2 == 0.0 or c2 == 0.0:
        return []
    ca, cb, cg = _dot(f[1], f[2]), _dot(f[0], f[2]), _dot(f[0], f[1])
    q = _div(a2 - c2, b2)
    p = _div(a2 + c2, b2)
    rc = _div(c2, b2)
    ra = _div(a2, b2)
    A4 = (q - 1.0) * (q - 1.0) - (4.0 * rc) * (ca * ca)
    A3 = 4.0 * (((q * (1.0 - q)) * cb - ((1.0 - p) * ca) * cg) + ((2.0 * rc) * (ca * ca)) * cb)
    A2 = 2.0 * (((((q * q - 1.0) + (2.0 * (q * q)) * (cb * cb)) + (2.0 * _div(b2 - c2, b2)) * (ca * ca)) - ((4.0 * p) * (ca * cb)) * cg)
                + (2.0 * _div(b2 - a2, b2)) * (cg * cg))
    A1 = 4.0 * (((((-q) * (1.0 + q)) * cb) + ((2.0 * ra) * (cg * cg)) * cb) - ((1.0 - p) * ca) * cg)
    A0 = (1.0 + q) * (1.0 + q) - (4.0 * ra) * (cg * cg)
    s = (((A4 + A3) + A2) + A1) + A0
    if not _finite(s) or A4 == 0.0:
        return []
    b3, b2_, b1, b0 = _div(A3, A4), _div(A2, A4), _div(A1, A4), _div(A0, A4)
    sh = b3 * 0.25
    sh2 = sh * sh
    pp = b2_ - 6.0 * sh2
    qq = (b1 - (2.0 * b2_) * sh) + (8.0 * sh2) * sh
    rr = ((b0 - b1 * sh) + b2_ * sh2) - (3.0 * sh2) * sh2
    # resolvent cubic m^3 + c2 m^2 + c1 m + c0, c0 <= 0: a root in [0, 1 + max |c|]
    k2 = pp
    k1 = (pp * pp) * 0.25 - rr
    k0 = -((qq * qq) * 0.125)
    lo = 0.0
    hi = 1.0 + max(max(abs(k2), abs(k1)), abs(k0))
    if not _finite(hi):
        return []
    for _ in range(P3P_BISECT):
        mid = 0.5 * (lo + hi)
        if _cubic(mid, k2, k1, k0) > 0.0:
            hi = mid
        else:
            lo = mid
    m = hi
    gm = _cubic(m, k2, k1, k0)
    for _ in range(P3P_CUBIC_NEWTON):
        dg = (3.0 * m + 2.0 * k2) * m + k1
        mn = m - _div(gm, dg)
        gn = _cubic(mn, k2, k1, k0)
        if mn > 0.0 and abs(gn) < abs(gm):
            m, gm = mn, gn
    w = _sqrt(2.0 * m)
    hq = _div(qq, 2.0 * w)
    base = 0.5 * pp + m
    roots = []
    for sign in (1.0, -1.0):            # y^2 - w y + (base + hq), then y^2 + w y + (base - hq)
        cq = base + sign * hq
        disc = w * w - 4.0 * cq
        if disc >= 0.0:
            sd = _sqrt(disc)
            roots.append(0.5 * (sign * w + sd) - sh)
            roots.append(0.5 * (sign * w - sd) - sh)
    out = []
    fp = None
    for v in roots:
        fv = _quartic(v, b3, b2_, b1, b0)
        for _ in range(P3P_QUARTIC_NEWTON):
            dv = ((4.0 * v + 3.0 * b3) * v + 2.0 * b2_) * v + b1
            vn = v - _div(fv, dv)
            fn = _quartic(vn, b3, b2_, b1, b0)
            if abs(fn) < abs(fv):
                v, fv = vn, fn
        if not v > 0.0:
            continue
        den = 2.0 * (cg - v * ca)
        u = _div((((q - 1.0) * v) * v - ((2.0 * q) * cb) * v) + (1.0 + q), den)
        if not u > 0.0:
            continue
        s1sq = _div(b2, (1.0 + v * v) - (2.0 * v) * cb)
        if not s1sq > 0.0:
            continue
        s1 = _sqrt(s1sq)
        s2 = u * s1
        s3 = v * s1
        Y = [[s1 * f[0][i] for i in range(3)], [s2 * f[1][i] for i in range(3)], [s3 * f[2][i] for i in range(3)]]
        if fp is None:
            fp = _frame(P[0], P[1], P[2])
        fy = _frame(Y[0], Y[1], Y[2])
        pose = [0.0] * 12
        for i in range(3):
            for j in range(3):
                pose[4 * i + j] = (fy[0][i] * fp[0][j] + fy[1][i] * fp[1][j]) + fy[2][i] * fp[2][j]
        for i in range(3):
            pose[4 * i + 3] = Y[0][i] - ((pose[4 * i] * P[0][0] + pose[4 * i + 1] * P[0][1]) + pose[4 * i + 2] * P[0][2])
        ok = True
        for k in range(3):              # the three points in front of the camera under the pose itself
            z = ((pose[8] * P[k][0] + pose[9] * P[k][1]) + pose[10] * P[k][2]) + pose[11]
            if not z > 0.0:
                ok = False
        if ok:
            out.append(pose)
    return out


def sample_model(idx, landmark, X, xy, K):
    """Step 3: the sample's model, or None."""
    for a in range(4):
        for b in range(a):
            if landmark[idx[a]] == landmark[idx[b]]:
                return None
    f = [bearing(K, float(xy[idx[k]][0]), float(xy[idx[k]][1])) for k in range(3)]
    P = [[float(X[idx[k]][i]) for i in range(3)] for k in range(3)]
    best, best_e = None, math.inf
    X3 = X[idx[3]]
    for pose in p3p(f, P):
        e = reproj_sq(pose, K, float(X3[0]), float(X3[1]), float(X3[2]), float(xy[idx[3]][0]), float(xy[idx[3]][1]))
        if e < best_e:
            best, best_e = pose, e
    return best


# ---- scoring --------------------------------------------------------------------------------------------------------

def _inliers_numpy(pose, K, X, xyf, t2):
    with np.errstate(all="ignore"):
        e = reproj_sq(pose, K, X[:, 0], X[:, 1], X[:, 2], xyf[:, 0], xyf[:, 1]).astype(np.float32)
        return e <= t2          # a NaN compares false


def _inliers_literal(pose, K, X, xyf, t2):
    m = np.zeros(len(X), bool)
    for e in range(len(X)):
        err = np.float32(reproj_sq(pose, K, float(X[e, 0]), float(X[e, 1]), float(X[e, 2]), float(xyf[e, 0]), float(xyf[e, 1])))
        m[e] = bool(err <= t2)
    return m


# ---- refit ----------------------------------------------------------------------------------------------------------

def _terms(pose, K, X0, X1, X2, ox, oy):
    """The 28 per-entry terms of the normal equations: upper triangle of J'J row by row (21), J'r (6), r'r."""
    u, v, l, x, y, radius, W = project(pose, K, X0, X1, X2)
    ru = u - ox
    rv = v - oy
    iz = _div(1.0, l[2])
    g = 2.0 * (K[4] + (2.0 * K[5]) * radius)
    gx = g * x
    gy = g * y
    uxx = K[0] * (1.0 + gx)
    uxy = K[0] * gy
    vxx = K[1] * gx
    vxy = K[1] * (1.0 + gy)
    zero = W[0] * 0.0 if isinstance(W[0], np.ndarray) else 0.0
    one = zero + 1.0
    dY = [[zero, W[2], -W[1], one, zero, zero],
          [-W[2], zero, W[0], zero, one, zero],
          [W[1], -W[0], zero, zero, zero, one]]
    Ju, Jv = [], []
    for k in range(6):
        dx = (dY[0][k] - x * dY[2][k]) * iz
        dy = (dY[1][k] - y * dY[2][k]) * iz
        Ju.append(uxx * dx + uxy * dy)
        Jv.append(vxx * dx + vxy * dy)
    t = []
    for k in range(6):
        for j in range(k, 6):
            t.append(Ju[k] * Ju[j] + Jv[k] * Jv[j])
    for k in range(6):
        t.append(Ju[k] * ru + Jv[k] * rv)
    t.append(ru * ru + rv * rv)
    return t


def _cost_term(pose, K, X0, X1, X2, ox, oy):
    return [reproj_sq(pose, K, X0, X1, X2, ox, oy)]


def _chunked_sums(fn, nterms, pose, K, X, xyf, mask, literal):
    """Sums of fn's terms over the entries with mask set: chunks of CHUNK consecutive entries, each summed in entry order
    from 0.0, the chunk sums added in chunk order from 0.0."""
    n = len(X)
    nch = (n + CHUNK - 1) // CHUNK
    if literal:
        tot = [0.0] * nterms
        for c in range(nch):
            acc = [0.0] * nterms
            for e in range(c * CHUNK, min(n, (c + 1) * CHUNK)):
                if mask[e]:
                    t = fn(pose, K, float(X[e, 0]), float(X[e, 1]), float(X[e, 2]), float(xyf[e, 0]), float(xyf[e, 1]))
                    for k in range(nterms):
                        acc[k] = acc[k] + t[k]
            for k in range(nterms):
                tot[k] = tot[k] + acc[k]
        return tot
    with np.errstate(all="ignore"):
        t = fn(pose, K, X[:, 0], X[:, 1], X[:, 2], xyf[:, 0], xyf[:, 1])
        T = np.zeros((nterms, nch * CHUNK))
        for k in range(nterms):
            T[k, :n] = t[k]
        M = np.zeros(nch * CHUNK, bool)
        M[:n] = mask
        T = T.reshape(nterms, nch, CHUNK)
        M = M.reshape(nch, CHUNK)
        acc = np.zeros((nterms, nch))
        for j in range(CHUNK):
            acc = np.where(M[None, :, j], acc + T[:, :, j], acc)
        tot = [0.0] * nterms
        for c in range(nch):
            for k in range(nterms):
                tot[k] = tot[k] + float(acc[k, c])
        return tot


def _solve6(A, g, lam):
    """(A + lam diag A) d = -g by Cholesky; None when a pivot is not positive."""
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j] + lam * A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = _sqrt(s)
        for i in range(j + 1, 6):
            s = A[j][i]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = _div(s, L[j][j])
    z = [0.0] * 6
    for i in range(6):
        s = -g[i]
        for k in range(i):
            s = s - L[i][k] * z[k]
        z[i] = _div(s, L[i][i])
    d = [0.0] * 6
    for i in range(5, -1, -1):
        s = z[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * d[k]
        d[i] = _div(s, L[i][i])
    return d


def _apply(pose, d):
    """R <- Q(w) R with Q the rotation of the normalised quaternion (1, w / 2); t <- t + dt."""
    qb, qc, qd = 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]
    nrm = _sqrt(((1.0 + qb * qb) + qc * qc) + qd * qd)
    a, b, c, dd = _div(1.0, nrm), _div(qb, nrm), _div(qc, nrm), _div(qd, nrm)
    Q = [[((a * a + b * b) - c * c) - dd * dd, 2.0 * (b * c - a * dd), 2.0 * (b * dd + a * c)],
         [2.0 * (b * c + a * dd), ((a * a - b * b) + c * c) - dd * dd, 2.0 * (c * dd - a * b)],
         [2.0 * (b * dd - a * c), 2.0 * (c * dd + a * b), ((a * a - b * b) - c * c) + dd * dd]]
    out = [0.0] * 12
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (Q[i][0] * pose[j] + Q[i][1] * pose[4 + j]) + Q[i][2] * pose[8 + j]
        out[4 * i + 3] = pose[4 * i + 3] + d[3 + i]
    return out


def refit(pose0, K, X, xyf, mask, iters, literal=False):
    """Damped Gauss-Newton on the masked entries from pose0 (damping lam diag(J'J), lam from 1e-3, / 10 after an accepted
    step, x 10 after a rejected one; only cost-decreasing steps are accepted; stops once a step changes the cost by no
    more than 1e-14 of it, accepted or not); pose0 itself when a normal matrix is not positive definite."""
    pose = list(pose0)
    lam = LAMBDA0
    for _ in range(iters):
        s = _chunked_sums(_terms, 28, pose, K, X, xyf, mask, literal)
        A = [[0.0] * 6 for _ in range(6)]
        q = 0
        for k in range(6):
            for j in range(k, 6):
                A[k][j] = s[q]
                q += 1
        g = s[21:27]
        c0 = s[27]
        d = _solve6(A, g, lam)
        if d is None:
            return list(pose0)
        trial = _apply(pose, d)
        c1 = _chunked_sums(_cost_term, 1, trial, K, X, xyf, mask, literal)[0]
        if c1 < c0:
            done = (c0 - c1) <= 1e-14 * c0
            pose = trial
            lam = lam / 10.0
            if done:
                break
        else:
            if (c1 - c0) <= 1e-14 * c0:         # rejected, but equal to rounding: converged
                break
            lam = lam * 10.0
    return pose


# ---- the search -----------------------------------------------------------------------------------------------------

def pnp_ransac(landmark, xy, points, intr6, opt=None, literal=False, B=32):
    """One view.  landmark (n,) int, xy (n, 2) int pixels, points (n_points, 3), intr6 = fx fy cx cy k1 k2.
    Returns dict(count, mask, pose34, ransac_pose34, iterations)."""
    o = default_options()
    if opt:
        o.update(opt)
    landmark = np.asarray(landmark, np.int64)
    n = len(landmark)
    K = [float(v) for v in np.asarray(intr6, np.float64)]
    res = dict(count=-2, mask=np.zeros(n, np.uint8), pose34=np.zeros(12), ransac_pose34=np.zeros(12), iterations=0)
    if n < 4:
        return res
    points = np.asarray(points, np.float64).reshape(-1, 3)
    X = points[landmark]
    xyf = np.asarray(xy, np.int32).reshape(n, 2).astype(np.float64)
    thr = float(o["max_projection_error"])
    t2 = np.float32(thr * thr)
    conf = float(o["confidence"])
    inl = _inliers_literal if literal else _inliers_numpy
    rng = RNG()
    niters = int(o["max_iterations"])
    best, best_pose, best_mask = 0, None, None
    it = 0
    if literal:
        while it < niters:
            idx = draw_sample(rng, n)
            pose = sample_model(idx, landmark, X, xyf, K)
            if pose is not None:
                m = inl(pose, K, X, xyf, t2)
                good = int(m.sum())
                if good > max(best, 3):
                    best, best_pose, best_mask = good, pose, m
                    niters = update_num_iters(conf, (n - good) / n, 4, niters)
            it += 1
    else:
        stop = False
        while not stop and it < niters:
            base = it
            samples = [draw_sample(rng, n) for _ in range(B)]
            poses = [sample_model(idx, landmark, X, xyf, K) for idx in samples]
            masks = [None if p is None else inl(p, K, X, xyf, t2) for p in poses]
            for h in range(B):
                if base + h >= niters:
                    stop = True
                    break
                if poses[h] is not None:
                    good = int(masks[h].sum())
                    if good > max(best, 3):
                        best, best_pose, best_mask = good, poses[h], masks[h]
                        niters = update_num_iters(conf, (n - good) / n, 4, niters)
                it = base + h + 1
    res["iterations"] = it
    if best_pose is None:
        res["count"] = -1
        return res
    res["count"] = best
    res["mask"] = best_mask.astype(np.uint8)
    res["ransac_pose34"] = np.array(best_pose, np.float64)
    res["pose34"] = np.array(refit(best_pose, K, X, xyf, best_mask, int(o["refine_iterations"]), literal), np.float64)
    return res


def pnp_ransac_batch(off, landmark, xy, points, intr6, opt=None, **kw):
    """The batch of rcn_pnp_ransac: view v owns entries off[v] .. off[v + 1]."""
    nv = len(off) - 1
    n = int(off[-1])
    out = dict(pose34=np.zeros((nv, 12)), ransac_pose34=np.zeros((nv, 12)), mask=np.zeros(n, np.uint8),
               count=np.zeros(nv, np.int32), iterations=np.zeros(nv, np.int32))
    xy = np.asarray(xy).reshape(-1, 2)
    for v in range(nv):
        a, b = int(off[v]), int(off[v + 1])
        r = pnp_ransac(np.asarray(landmark)[a:b], xy[a:b], points, np.asarray(intr6).reshape(nv, 6)[v], opt, **kw)
        out["pose34"][v], out["ransac_pose34"][v], out["mask"][a:b] = r["pose34"], r["ransac_pose34"], r["mask"]
        out["count"][v], out["iterations"][v] = r["count"], r["iterations"]
    return out


# ---- test scenes ----------------------------------------------------------------------------------------------------

def scene_views(seed, wrong_share, n_cams=12, n_pts=1500):
    """Section 17's test scenes: synth_ba.make_scene(n_cams, n_pts, obs_per_point=8, seed), every camera a view, pixels
    truncated to integers, a share of the entries given a random other landmark.  Returns (points, views), a view being
    dict(landmark, xy, intr6, pose34_gt, wrong)."""
    from reconstructor_amd import synth_ba
    sc = synth_ba.make_scene(n_cams, n_pts, obs_per_point=min(n_cams, 8), seed=seed)
    rng = np.random.default_rng(seed + 9)
    views = []
    for v in range(n_cams):
        o = np.flatnonzero(sc["obs_cam"] == v)
        lm = sc["obs_pt"][o].astype(np.int32).copy()
        xy = np.trunc(sc["obs_uv"][o]).astype(np.int32)
        bad = rng.random(len(o)) < wrong_share
        lm[bad] = rng.integers(0, n_pts, int(bad.sum()))
        views.append(dict(landmark=lm, xy=xy, intr6=sc["intr_gt"][v].astype(np.float64).copy(),
                          pose34_gt=synth_ba.poses_to_34(sc["poses_gt"][v:v + 1]).reshape(12).astype(np.float64), wrong=bad))
    return sc["points_gt"].astype(np.float64).copy(), views


def within(pose, K, points, landmark, xy, thr=4.0):
    """Entries within the threshold under the pose (the kernel's own rule)."""
    X = np.asarray(points, np.float64).reshape(-1, 3)[np.asarray(landmark, np.int64)]
    xyf = np.asarray(xy).reshape(-1, 2).astype(np.float64)
    return _inliers_numpy([float(v) for v in pose], [float(v) for v in K], X, xyf, np.float32(thr * thr))


def edge_cases():
    """Section 17's edge cases: list of (name, landmark, xy, points, intr6)."""
    pts, views = scene_views(3, 0.0, n_cams=4, n_pts=400)
    v = views[0]
    lm, xy, K = v["landmark"], v["xy"], v["intr6"]
    cases = [("n0", lm[:0], xy[:0], pts, K), ("n3", lm[:3], xy[:3], pts, K), ("n4", lm[:4], xy[:4], pts, K)]
    # n = 4 coplanar: four points of the plane z = 0.3 seen by the view's own camera
    P = v["pose34_gt"].reshape(3, 4)
    rng = np.random.default_rng(5)
    flat = np.concatenate([rng.uniform(-0.5, 0.5, (4, 2)), np.full((4, 1), 0.3)], 1)
    l = flat @ P[:, :3].T + P[:, 3]
    fxy = np.trunc(np.stack([K[0] * l[:, 0] / l[:, 2] + K[2], K[1] * l[:, 1] / l[:, 2] + K[3]], 1)).astype(np.int32)
    cases.append(("n4_coplanar", np.arange(4, dtype=np.int32), fxy, flat, K))
    cases.append(("same_landmark", np.full(60, lm[0], np.int32), xy[:60], pts, K))
    rep = lm[:150].copy()
    rep[100:150] = lm[7]
    cases.append(("repeated50", rep, xy[:150], pts, K))
    nanp = pts.copy()
    nanp[lm[5:40:3]] = np.nan
    cases.append(("nan_points", lm[:200], xy[:200], nanp, K))
    # k1, k2 != 0: pixels re-projected with the distorted camera
    Kd = K.copy()
    Kd[4:] = rng.normal(0, 1e-3, 2)
    X = pts[lm]
    l = X @ P[:, :3].T + P[:, 3]
    x, y = l[:, 0] / l[:, 2], l[:, 1] / l[:, 2]
    r = x * x + y * y
    d = Kd[4] * r + Kd[5] * r * r
    dxy = np.trunc(np.stack([Kd[0] * (x + d) + Kd[2], Kd[1] * (y + d) + Kd[3]], 1) + rng.normal(0, 0.5, (len(lm), 2))).astype(np.int32)
    wrong = lm.copy()
    bad = rng.random(len(lm)) < 0.3
    wrong[bad] = rng.integers(0, len(pts), int(bad.sum()))
    cases.append(("distortion", wrong, dxy, pts, Kd))
    w9 = lm[:200].copy()
    bad = rng.random(200) < 0.9
    w9[bad] = rng.integers(0, len(pts), int(bad.sum()))
    cases.append(("w09", w9, xy[:200], pts, K))
    return cases
