"""CPU restatement of two-view initialisation: batched 5-point RANSAC and pose recovery (csrc/twoview.hip, DESIGN.md
section 18), for the tests only.

The kernel's arithmetic is + - * / sqrt on separately rounded IEEE doubles in one fixed order; every function below states
that order once.  The solver runs on Python floats; the scoring and the cheirality test run either on Python floats (one
entry at a time) or on numpy arrays (element-wise over the entries: the same IEEE operations, so the same bits).  No numpy
reduction is used anywhere: sums are written out.

two_view_init(..., literal=True)    the sequential loop of the canonical algorithm, one iteration and one entry at a time.
two_view_init(..., literal=False)   the kernel's structure: rounds of B samples (draw, solve, score, accept in iteration
                                    order, discard what lies behind the stopping point).
Both give the same masks, counts, iteration count, E and pose, bit for bit, for every B.  pow / log in update_num_iters is
the one place where the host and the device may round differently (section 18).
"""
import math

import numpy as np

DEFAULT_OPTIONS = dict(threshold=1.0, confidence=0.999, distance_threshold=50.0, max_iterations=1000)
ROOT_BISECT = 40        # bisection steps per isolated root
ROOT_NEWTON = 4         # guarded Newton steps per root after the bisection
POLISH_STEPS = 3        # Gauss-Newton steps on (x, y, z) against the constraints of E itself
DBL_MIN = 2.2250738585072014e-308

# monomials: degree <= 1 as (x, y, z, 1); degree <= 2 and <= 3 in the orders below (exponents of x, y, z).  The order of the
# 20 is the elimination's: ten leading monomials, then x * (z^2, z, 1), y * (z^2, z, 1), z^3, z^2, z, 1.
MONO1 = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
MONO2 = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
MONO3 = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
         (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _add(a, b):
    return tuple(p + q for p, q in zip(a, b))


M12 = [[MONO2.index(_add(a, b)) for b in MONO1] for a in MONO1]       # (4, 4) -> 0 .. 9
M23 = [[MONO3.index(_add(a, b)) for b in MONO1] for a in MONO2]       # (10, 4) -> 0 .. 19


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
    """5 distinct entry indices, each next() % n, redrawn while equal to an earlier one."""
    idx = []
    while len(idx) < 5:
        i = rng.next() % n
        if i not in idx:
            idx.append(i)
    return idx


# ---- normalisation ---------------------------------------------------------------------------------------------------

def mean_camera(K1, K2):
    """fx fy cx cy of the mean of the two camera matrices."""
    return [(K1[i] + K2[i]) * 0.5 for i in range(4)]


def normalise(K, Km, u, v):
    """Camera.h:79-93 unprojection of the pixel, scaled back by the mean camera matrix, normalised by it again."""
    x = _div(u - K[2], K[0])
    y = _div(v - K[3], K[1])
    radius = x * x + y * y
    d = K[4] * radius + (K[5] * radius) * radius
    x = x - d
    y = y - d
    pu = Km[0] * x + Km[2]
    pv = Km[1] * y + Km[3]
    return _div(pu - Km[2], Km[0]), _div(pv - Km[3], Km[1])


# ---- five-point solver -----------------------------------------------------------------------------------------------

def nullspace4(Q):
    """Four vectors spanning the null space of the 5 x 9 matrix Q (list of rows; destroyed): Gauss-Jordan with complete
    pivoting (the first largest |.| in row-major order over the remaining block), columns swapped in place, the four
    vectors then mixed by a fixed Hadamard matrix.  None when a pivot is zero or not finite."""
    perm = list(range(9))
    for k in range(5):
        pr, pc, pa = k, k, -1.0
        for r in range(k, 5):
            for c in range(k, 9):
                a = abs(Q[r][c])
                if a > pa:
                    pr, pc, pa = r, c, a
        if not (pa > 0.0) or not _finite(pa):
            return None
        if pr != k:
            Q[k], Q[pr] = Q[pr], Q[k]
        if pc != k:
            for r in range(5):
                Q[r][k], Q[r][pc] = Q[r][pc], Q[r][k]
            perm[k], perm[pc] = perm[pc], perm[k]
        p = Q[k][k]
        for c in range(k + 1, 9):
            Q[k][c] = _div(Q[k][c], p)
        for r in range(5):
            if r == k:
                continue
            f = Q[r][k]
            for c in range(k + 1, 9):
                Q[r][c] = Q[r][c] - f * Q[k][c]
    basis = []
    for b in range(4):
        v = [0.0] * 9
        v[perm[5 + b]] = 1.0
        for k in range(5):
            v[perm[k]] = -Q[k][5 + b]
        basis.append(v)
    # The raw vectors are unit vectors on the four free columns, so E's coordinates in them would be four of E's own
    # entries, and E has entries that are small by structure (the diagonal, for a small rotation): mixed by a fixed
    # Hadamard matrix, the coordinate that is set to 1 is a sum of four entries instead.
    X, Y, Z, W = basis
    return [[((X[i] + Y[i]) + Z[i]) + W[i] for i in range(9)], [((X[i] - Y[i]) + Z[i]) - W[i] for i in range(9)],
            [((X[i] + Y[i]) - Z[i]) - W[i] for i in range(9)], [((X[i] - Y[i]) - Z[i]) + W[i] for i in range(9)]]


def _mul11(a, b):
    out = [0.0] * 10
    for i in range(4):
        for j in range(4):
            out[M12[i][j]] = out[M12[i][j]] + a[i] * b[j]
    return out


def _mul21(a, b):
    out = [0.0] * 20
    for i in range(10):
        for j in range(4):
            out[M23[i][j]] = out[M23[i][j]] + a[i] * b[j]
    return out


def constraint_rows(basis):
    """The 10 x 20 matrix of the cubic constraints on E = x X + y Y + z Z + W: rows 0 .. 8 the entries of
    (E E' - trace(E E') / 2 I) E row by row, row 9 det E; columns in MONO3 order."""
    E = [[[basis[b][3 * i + j] for b in range(4)] for j in range(3)] for i in range(3)]
    EEt = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            a, b, c = _mul11(E[i][0], E[j][0]), _mul11(E[i][1], E[j][1]), _mul11(E[i][2], E[j][2])
            EEt[i][j] = [(a[m] + b[m]) + c[m] for m in range(10)]
            EEt[j][i] = EEt[i][j]
    tr = [(EEt[0][0][m] + EEt[1][1][m]) + EEt[2][2][m] for m in range(10)]
    L = [[EEt[i][j] if i != j else [EEt[i][i][m] - 0.5 * tr[m] for m in range(10)] for j in range(3)] for i in range(3)]
    rows = []
    for i in range(3):
        for j in range(3):
            a, b, c = _mul21(L[i][0], E[0][j]), _mul21(L[i][1], E[1][j]), _mul21(L[i][2], E[2][j])
            rows.append([(a[m] + b[m]) + c[m] for m in range(20)])
    m0 = [p - q for p, q in zip(_mul11(E[1][1], E[2][2]), _mul11(E[1][2], E[2][1]))]
    m1 = [p - q for p, q in zip(_mul11(E[1][0], E[2][2]), _mul11(E[1][2], E[2][0]))]
    m2 = [p - q for p, q in zip(_mul11(E[1][0], E[2][1]), _mul11(E[1][1], E[2][0]))]
    a, b, c = _mul21(m0, E[0][0]), _mul21(m1, E[0][1]), _mul21(m2, E[0][2])
    rows.append([(a[m] - b[m]) + c[m] for m in range(20)])
    return rows


def eliminate(A):
    """Gauss-Jordan on the 10 x 20 matrix over its first ten columns, partial pivoting (the first largest |.| of the column
    among the remaining rows).  False when a pivot is zero or not finite."""
    for k in range(10):
        pr, pa = k, -1.0
        for r in range(k, 10):
            a = abs(A[r][k])
            if a > pa:
                pr, pa = r, a
        if not (pa > 0.0) or not _finite(pa):
            return False
        if pr != k:
            A[k], A[pr] = A[pr], A[k]
        p = A[k][k]
        for c in range(k + 1, 20):
            A[k][c] = _div(A[k][c], p)
        for r in range(10):
            if r == k:
                continue
            f = A[r][k]
            for c in range(k + 1, 20):
                A[r][c] = A[r][c] - f * A[k][c]
    return True


def _conv(a, b):
    out = [0.0] * (len(a) + len(b) - 1)
    for i in range(len(a)):
        for j in range(len(b)):
            out[i + j] = out[i + j] + a[i] * b[j]
    return out


def _horner(c, d, x):
    """c[0] + c[1] x + ... + c[d] x^d."""
    r = c[d]
    for i in range(d - 1, -1, -1):
        r = r * x + c[i]
    return r


def z_polynomials(A):
    """Rows 4 .. 9 of the eliminated matrix (x^2 z, x^2, y^2 z, y^2, x y z, x y) give three equations
    bx(z) x + by(z) y + b1(z) = 0; returns (p1, p2, p3, c): (x, y, 1) ~ (p1, p2, p3)(z), c the degree-10 determinant.
    Coefficients in ascending powers of z."""
    B = []
    for e, f in ((4, 5), (6, 7), (8, 9)):
        re, rf = A[e][10:], A[f][10:]
        bx = [re[2], re[1] - rf[2], re[0] - rf[1], -rf[0]]
        by = [re[5], re[4] - rf[5], re[3] - rf[4], -rf[3]]
        b1 = [re[9], re[8] - rf[9], re[7] - rf[8], re[6] - rf[7], -rf[6]]
        B.append((bx, by, b1))
    p1 = [p - q for p, q in zip(_conv(B[0][1], B[1][2]), _conv(B[0][2], B[1][1]))]
    p2 = [p - q for p, q in zip(_conv(B[0][2], B[1][0]), _conv(B[0][0], B[1][2]))]
    p3 = [p - q for p, q in zip(_conv(B[0][0], B[1][1]), _conv(B[0][1], B[1][0]))]
    a, b, c = _conv(p1, B[2][0]), _conv(p2, B[2][1]), _conv(p3, B[2][2])
    return p1, p2, p3, [(a[m] + b[m]) + c[m] for m in range(11)]


def real_roots(c):
    """Real roots of the degree-10 polynomial c (ascending powers), ascending: made monic, Cauchy bound R = 1 + max |a_i|,
    then level by level through the derivative chain (degree 1 .. 10): a level's roots separate the next level's, every
    interval between consecutive separators (and -R, R) whose end values differ in sign (v > 0) holds one root, found by
    ROOT_BISECT bisection steps and ROOT_NEWTON Newton steps that must stay inside the bracket and reduce |f|."""
    s = 0.0
    for i in range(11):
        s = s + c[i]
    if not _finite(s) or c[10] == 0.0:
        return []
    D = [None] * 11
    D[10] = [_div(c[i], c[10]) for i in range(10)] + [1.0]
    R = 0.0
    for i in range(10):
        a = abs(D[10][i])
        if a > R:
            R = a
    R = 1.0 + R
    if not _finite(R):
        return []
    for d in range(10, 1, -1):
        D[d - 1] = [D[d][i + 1] * float(i + 1) for i in range(d)]
    roots = []
    for d in range(1, 11):
        pts = roots + [R]
        roots = []
        lo = -R
        flo = _horner(D[d], d, lo)
        for hi0 in pts:
            fhi0 = _horner(D[d], d, hi0)
            if (flo > 0.0) != (fhi0 > 0.0):
                a, b = lo, hi0
                for _ in range(ROOT_BISECT):
                    mid = 0.5 * (a + b)
                    if (_horner(D[d], d, mid) > 0.0) == (flo > 0.0):
                        a = mid
                    else:
                        b = mid
                x = 0.5 * (a + b)
                fx = _horner(D[d], d, x)
                for _ in range(ROOT_NEWTON):
                    xn = x - _div(fx, _horner(D[d - 1], d - 1, x)) if d > 1 else x - _div(fx, D[1][1])
                    if xn >= a and xn <= b:
                        fn = _horner(D[d], d, xn)
                        if abs(fn) < abs(fx):
                            x, fx = xn, fn
                roots.append(x)
            lo, flo = hi0, fhi0
    return roots


def _mm(A, B):
    return [(A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def _mmt(A, B):
    return [(A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1]) + A[3 * i + 2] * B[3 * j + 2] for i in range(3) for j in range(3)]


def _cofactors(e):
    return [e[4] * e[8] - e[5] * e[7], e[5] * e[6] - e[3] * e[8], e[3] * e[7] - e[4] * e[6],
            e[2] * e[7] - e[1] * e[8], e[0] * e[8] - e[2] * e[6], e[1] * e[6] - e[0] * e[7],
            e[1] * e[5] - e[2] * e[4], e[2] * e[3] - e[0] * e[5], e[0] * e[4] - e[1] * e[3]]


def _constraints(E):
    """The ten constraint values of E (nine of (E E' - trace(E E') / 2 I) E, then det E), M = E E' - trace / 2 I, and
    their squared sum."""
    M = _mmt(E, E)
    h = 0.5 * ((M[0] + M[4]) + M[8])
    M[0], M[4], M[8] = M[0] - h, M[4] - h, M[8] - h
    f = _mm(M, E)
    f.append((E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6])) + E[2] * (E[3] * E[7] - E[4] * E[6]))
    c = 0.0
    for k in range(10):
        c = c + f[k] * f[k]
    return f, M, c


def polish(basis, x, y, z):
    """POLISH_STEPS Gauss-Newton steps on (x, y, z) against the ten constraints evaluated on E itself (not on the
    eliminated system, whose conditioning depends on how close two solutions' z lie): a step is kept only if it lowers the
    squared sum of the constraints.  Returns E = x X + y Y + z Z + W."""
    def at(x, y, z):
        return [((x * basis[0][i] + y * basis[1][i]) + z * basis[2][i]) + basis[3][i] for i in range(9)]
    E = at(x, y, z)
    f, M, c = _constraints(E)
    for _ in range(POLISH_STEPS):
        cof = _cofactors(E)
        J = []
        for D in basis[:3]:
            a, b = _mmt(D, E), _mmt(E, D)
            dM = [a[i] + b[i] for i in range(9)]
            h = 0.5 * ((dM[0] + dM[4]) + dM[8])
            dM[0], dM[4], dM[8] = dM[0] - h, dM[4] - h, dM[8] - h
            a, b = _mm(dM, E), _mm(M, D)
            col = [a[i] + b[i] for i in range(9)]
            dd = 0.0
            for i in range(9):
                dd = dd + cof[i] * D[i]
            col.append(dd)
            J.append(col)
        N = [[0.0] * 3 for _ in range(3)]
        g = [0.0] * 3
        for a in range(3):
            for b in range(a, 3):
                t = 0.0
                for k in range(10):
                    t = t + J[a][k] * J[b][k]
                N[a][b] = t
            t = 0.0
            for k in range(10):
                t = t + J[a][k] * f[k]
            g[a] = t
        c00 = N[1][1] * N[2][2] - N[1][2] * N[1][2]
        c01 = N[0][2] * N[1][2] - N[0][1] * N[2][2]
        c02 = N[0][1] * N[1][2] - N[0][2] * N[1][1]
        c11 = N[0][0] * N[2][2] - N[0][2] * N[0][2]
        c12 = N[0][1] * N[0][2] - N[0][0] * N[1][2]
        c22 = N[0][0] * N[1][1] - N[0][1] * N[0][1]
        det = (N[0][0] * c00 + N[0][1] * c01) + N[0][2] * c02
        if not det > 0.0:
            break
        xn = x - _div((c00 * g[0] + c01 * g[1]) + c02 * g[2], det)
        yn = y - _div((c01 * g[0] + c11 * g[1]) + c12 * g[2], det)
        zn = z - _div((c02 * g[0] + c12 * g[1]) + c22 * g[2], det)
        En = at(xn, yn, zn)
        fn, Mn, cn = _constraints(En)
        if not cn < c:
            break
        x, y, z, E, f, M, c = xn, yn, zn, En, fn, Mn, cn
    return E


def five_point(x1, y1, x2, y2):
    """Nister's five-point method on five normalised correspondences (x2' E x1 = 0): up to ten E (9 floats, row-major, unit
    Frobenius norm) in ascending order of the root z."""
    Q = [[x2[k] * x1[k], x2[k] * y1[k], x2[k], y2[k] * x1[k], y2[k] * y1[k], y2[k], x1[k], y1[k], 1.0] for k in range(5)]
    basis = nullspace4(Q)
    if basis is None:
        return []
    A = constraint_rows(basis)
    if not eliminate(A):
        return []
    p1, p2, p3, c = z_polynomials(A)
    out = []
    for z in real_roots(c):
        w = _horner(p3, 6, z)
        x = _div(_horner(p1, 7, z), w)
        y = _div(_horner(p2, 7, z), w)
        E = polish(basis, x, y, z)
        s = 0.0
        for i in range(9):
            s = s + E[i] * E[i]
        nrm = _sqrt(s)
        if not _finite(nrm) or nrm == 0.0:
            continue
        out.append([_div(E[i], nrm) for i in range(9)])
    return out


# ---- scoring ---------------------------------------------------------------------------------------------------------

def sampson(E, x1, y1, x2, y2):
    """OpenCV's essential-matrix error: (x2' E x1)^2 / (|E x1|_xy^2 + |E' x2|_xy^2)."""
    a0 = (E[0] * x1 + E[1] * y1) + E[2]
    a1 = (E[3] * x1 + E[4] * y1) + E[5]
    a2 = (E[6] * x1 + E[7] * y1) + E[8]
    b0 = (E[0] * x2 + E[3] * y2) + E[6]
    b1 = (E[1] * x2 + E[4] * y2) + E[7]
    r = (x2 * a0 + y2 * a1) + a2
    den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1
    return _div(r * r, den)


def _inliers_numpy(E, P, t2):
    with np.errstate(all="ignore"):
        return sampson(E, P[:, 0], P[:, 1], P[:, 2], P[:, 3]).astype(np.float32) <= t2      # a NaN compares false


def _inliers_literal(E, P, t2):
    m = np.zeros(len(P), bool)
    for e in range(len(P)):
        err = np.float32(sampson(E, float(P[e, 0]), float(P[e, 1]), float(P[e, 2]), float(P[e, 3])))
        m[e] = bool(err <= t2)
    return m


# ---- pose recovery ---------------------------------------------------------------------------------------------------

def decompose(E):
    """E = [t]x R without an SVD.  t: the largest (first among equals) of the cross products of E's columns (c0 x c1,
    c0 x c2, c1 x c2), normalised; with En = E / sqrt(|E|_F^2 / 2): R1 = cof(En) - [t]x En, R2 = cof(En) + [t]x En.
    Returns (R1, R2, t) as flat lists, or None when E has no two independent columns."""
    col = [[E[j], E[3 + j], E[6 + j]] for j in range(3)]
    best, bn = None, 0.0
    for a, b in ((0, 1), (0, 2), (1, 2)):
        p, q = col[a], col[b]
        c = [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
        n2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        if n2 > bn:
            best, bn = c, n2
    if best is None or not _finite(bn):
        return None
    nt = _sqrt(bn)
    t = [_div(best[i], nt) for i in range(3)]
    s = 0.0
    for i in range(9):
        s = s + E[i] * E[i]
    sc = _sqrt(0.5 * s)
    e = [_div(E[i], sc) for i in range(9)]
    cof = [e[4] * e[8] - e[5] * e[7], e[5] * e[6] - e[3] * e[8], e[3] * e[7] - e[4] * e[6],
           e[2] * e[7] - e[1] * e[8], e[0] * e[8] - e[2] * e[6], e[1] * e[6] - e[0] * e[7],
           e[1] * e[5] - e[2] * e[4], e[2] * e[3] - e[0] * e[5], e[0] * e[4] - e[1] * e[3]]
    tx = [0.0] * 9
    for j in range(3):          # [t]x En, column by column
        tx[j] = t[1] * e[6 + j] - t[2] * e[3 + j]
        tx[3 + j] = t[2] * e[j] - t[0] * e[6 + j]
        tx[6 + j] = t[0] * e[3 + j] - t[1] * e[j]
    R1 = [cof[i] - tx[i] for i in range(9)]
    R2 = [cof[i] + tx[i] for i in range(9)]
    return R1, R2, t


def depths(R, t, x1, y1, x2, y2):
    """The two depths z1, z2 that bring z1 R (x1, y1, 1) + t closest to z2 (x2, y2, 1): 2 x 2 normal equations."""
    a0 = (R[0] * x1 + R[1] * y1) + R[2]
    a1 = (R[3] * x1 + R[4] * y1) + R[5]
    a2 = (R[6] * x1 + R[7] * y1) + R[8]
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    bb = (x2 * x2 + y2 * y2) + 1.0
    ab = (a0 * x2 + a1 * y2) + a2
    at = (a0 * t[0] + a1 * t[1]) + a2 * t[2]
    bt = (x2 * t[0] + y2 * t[1]) + t[2]
    det = aa * bb - ab * ab
    z1 = _div(ab * bt - at * bb, det)
    z2 = _div(aa * bt - ab * at, det)
    return z1, z2


def candidates(E):
    d = decompose(E)
    if d is None:
        return None
    R1, R2, t = d
    nt = [-t[0], -t[1], -t[2]]
    return [(R1, t), (R2, t), (R1, nt), (R2, nt)]        # OpenCV's order


def _good(R, t, P, dist, literal):
    if literal:
        g = np.zeros(len(P), bool)
        for e in range(len(P)):
            z1, z2 = depths(R, t, float(P[e, 0]), float(P[e, 1]), float(P[e, 2]), float(P[e, 3]))
            g[e] = z1 > 0.0 and z1 < dist and z2 > 0.0 and z2 < dist
        return g
    with np.errstate(all="ignore"):
        z1, z2 = depths(R, t, P[:, 0], P[:, 1], P[:, 2], P[:, 3])
        return (z1 > 0.0) & (z1 < dist) & (z2 > 0.0) & (z2 < dist)


def recover_pose(E, P, mask, dist, literal=False):
    """cv::recoverPose on the RANSAC mask: (pose34, cheirality mask, its count, index of the winning candidate)."""
    n = len(P)
    cand = candidates(E)
    if cand is None:
        return np.zeros(12), np.zeros(n, np.uint8), 0, -1
    good = [_good(R, t, P, dist, literal) & mask.astype(bool) for R, t in cand]
    g = [int(m.sum()) for m in good]
    if g[0] >= g[1] and g[0] >= g[2] and g[0] >= g[3]:
        w = 0
    elif g[1] >= g[0] and g[1] >= g[2] and g[1] >= g[3]:
        w = 1
    elif g[2] >= g[0] and g[2] >= g[1] and g[2] >= g[3]:
        w = 2
    else:
        w = 3
    R, t = cand[w]
    pose = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]
    return np.array(pose, np.float64), good[w].astype(np.uint8), g[w], w


# ---- the search ------------------------------------------------------------------------------------------------------

def normalised_entries(xy1, xy2, K1, K2):
    """(n, 4) float64: x1 y1 x2 y2 of every entry, and the mean camera."""
    Km = mean_camera(K1, K2)
    a = np.asarray(xy1, np.int32).reshape(-1, 2).astype(np.float64)
    b = np.asarray(xy2, np.int32).reshape(-1, 2).astype(np.float64)
    with np.errstate(all="ignore"):
        x1, y1 = normalise(K1, Km, a[:, 0], a[:, 1])
        x2, y2 = normalise(K2, Km, b[:, 0], b[:, 1])
    return np.stack([x1, y1, x2, y2], 1) if len(a) else np.zeros((0, 4)), Km


def solve_sample(idx, P):
    return five_point([float(P[i, 0]) for i in idx], [float(P[i, 1]) for i in idx],
                      [float(P[i, 2]) for i in idx], [float(P[i, 3]) for i in idx])


def two_view_init(xy1, xy2, intr6_1, intr6_2, opt=None, literal=False, B=32):
    """One pair.  xy1, xy2 (n, 2) int pixels in ascending query-feature order, intr6 = fx fy cx cy k1 k2 per image.
    Returns dict(count, mask, E, pose34, cheir_mask, cheir_count, iterations, candidate)."""
    o = default_options()
    if opt:
        o.update(opt)
    K1 = [float(v) for v in np.asarray(intr6_1, np.float64)]
    K2 = [float(v) for v in np.asarray(intr6_2, np.float64)]
    P, Km = normalised_entries(xy1, xy2, K1, K2)
    n = len(P)
    res = dict(count=-2, mask=np.zeros(n, np.uint8), E=np.zeros(9), pose34=np.zeros(12), cheir_mask=np.zeros(n, np.uint8),
               cheir_count=0, iterations=0, candidate=-1)
    if n < 5:
        return res
    thr = _div(float(o["threshold"]), (Km[0] + Km[1]) * 0.5)
    t2 = np.float32(thr * thr)
    conf = float(o["confidence"])
    inl = _inliers_literal if literal else _inliers_numpy
    rng = RNG()
    niters = int(o["max_iterations"])
    best, best_E, best_mask = 0, None, None
    it = 0
    if literal:
        while it < niters:
            for E in solve_sample(draw_sample(rng, n), P):
                m = inl(E, P, t2)
                good = int(m.sum())
                if good > max(best, 4):
                    best, best_E, best_mask = good, E, m
                    niters = update_num_iters(conf, (n - good) / n, 5, niters)
            it += 1
    else:
        stop = False
        while not stop and it < niters:
            base = it
            samples = [draw_sample(rng, n) for _ in range(B)]
            models = [solve_sample(idx, P) for idx in samples]
            masks = [[inl(E, P, t2) for E in ms] for ms in models]
            for h in range(B):
                if base + h >= niters:
                    stop = True
                    break
                for E, m in zip(models[h], masks[h]):
                    good = int(m.sum())
                    if good > max(best, 4):
                        best, best_E, best_mask = good, E, m
                        niters = update_num_iters(conf, (n - good) / n, 5, niters)
                it = base + h + 1
    res["iterations"] = it
    if best_E is None:
        res["count"] = -1
        return res
    res["count"] = best
    res["mask"] = best_mask.astype(np.uint8)
    res["E"] = np.array(best_E, np.float64)
    res["pose34"], res["cheir_mask"], res["cheir_count"], res["candidate"] = \
        recover_pose(best_E, P, res["mask"], float(o["distance_threshold"]), literal)
    return res


def two_view_init_batch(off, xy1, xy2, intr6_1, intr6_2, opt=None, **kw):
    """The batch of rcn_twoview_init: pair p owns entries off[p] .. off[p + 1]."""
    npairs = len(off) - 1
    n = int(off[-1])
    out = dict(E=np.zeros((npairs, 9)), pose34=np.zeros((npairs, 12)), mask=np.zeros(n, np.uint8), cheir_mask=np.zeros(n, np.uint8),
               count=np.zeros((npairs, 2), np.int32), iterations=np.zeros(npairs, np.int32))
    xy1 = np.asarray(xy1).reshape(-1, 2)
    xy2 = np.asarray(xy2).reshape(-1, 2)
    K1 = np.asarray(intr6_1, np.float64).reshape(npairs, 6)
    K2 = np.asarray(intr6_2, np.float64).reshape(npairs, 6)
    for p in range(npairs):
        a, b = int(off[p]), int(off[p + 1])
        r = two_view_init(xy1[a:b], xy2[a:b], K1[p], K2[p], opt, **kw)
        out["E"][p], out["pose34"][p], out["mask"][a:b], out["cheir_mask"][a:b] = r["E"], r["pose34"], r["mask"], r["cheir_mask"]
        out["count"][p] = (r["count"], r["cheir_count"])
        out["iterations"][p] = r["iterations"]
    return out


def choose_initial_pair(pairs, offsets):
    """The canonical initial pair: most matches, the lexicographically first (i, j) among equals.  Returns (i, j, index)."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    size = np.diff(np.asarray(offsets, np.int64))
    best = None
    for k in range(len(pairs)):
        key = (-int(size[k]), int(pairs[k, 0]), int(pairs[k, 1]))
        if best is None or key < best[0]:
            best = (key, k)
    if best is None:
        raise ValueError("no pairs")
    k = best[1]
    return int(pairs[k, 0]), int(pairs[k, 1]), k


# ---- test scenes -----------------------------------------------------------------------------------------------------

def rot(w):
    """Rodrigues."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def essential(R, t):
    t = np.asarray(t, np.float64)
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R


def scene_pair(seed, outlier_share, n=300, baseline=1.0, planar=False, noise=0.0, distortion=False):
    """Section 18's test scenes: a random relative pose (second camera [R | t], |t| = baseline), n points 3 .. 8 in front of
    the first camera seen by both, pixels truncated to integers, a share of the entries given a random pixel in the
    second image.  Returns dict(xy1, xy2, K1, K2, R, t, wrong)."""
    rng = np.random.default_rng(seed)
    K1 = np.array([900.0 + rng.uniform(-50, 50), 900.0 + rng.uniform(-50, 50), 640.0, 480.0, 0.0, 0.0])
    K2 = np.array([900.0 + rng.uniform(-50, 50), 900.0 + rng.uniform(-50, 50), 650.0, 470.0, 0.0, 0.0])
    if distortion:
        K1[4:] = rng.normal(0, 1e-3, 2)
        K2[4:] = rng.normal(0, 1e-3, 2)
    R = rot(rng.normal(0, 0.15, 3))
    t = rng.normal(0, 1, 3)
    t = baseline * t / np.linalg.norm(t) if baseline > 0 else np.zeros(3)
    X = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2, 2, n), rng.uniform(3, 8, n)], 1)
    if planar:
        X[:, 2] = 5.0 + 0.2 * X[:, 0] - 0.1 * X[:, 1]
    Y = X @ R.T + t

    def proj(K, Z):
        x, y = Z[:, 0] / Z[:, 2], Z[:, 1] / Z[:, 2]
        r = x * x + y * y
        d = K[4] * r + K[5] * r * r
        return np.stack([K[0] * (x + d) + K[2], K[1] * (y + d) + K[3]], 1)

    p1 = proj(K1, X) + rng.normal(0, 1, (n, 2)) * noise
    p2 = proj(K2, Y) + rng.normal(0, 1, (n, 2)) * noise
    wrong = rng.random(n) < outlier_share
    p2[wrong] = np.stack([rng.uniform(0, 1280, int(wrong.sum())), rng.uniform(0, 960, int(wrong.sum()))], 1)
    return dict(xy1=np.trunc(p1).astype(np.int32), xy2=np.trunc(p2).astype(np.int32), K1=K1, K2=K2, R=R, t=t, wrong=wrong)


def edge_cases():
    """Section 18's edge cases: list of (name, xy1, xy2, K1, K2)."""
    s = scene_pair(11, 0.2, n=200)
    K1, K2 = s["K1"], s["K2"]
    cases = [("n0", s["xy1"][:0], s["xy2"][:0], K1, K2), ("n4", s["xy1"][:4], s["xy2"][:4], K1, K2),
             ("n5", s["xy1"][:5], s["xy2"][:5], K1, K2), ("n6", s["xy1"][:6], s["xy2"][:6], K1, K2)]
    cases.append(("identical", np.repeat(s["xy1"][:1], 40, 0), np.repeat(s["xy2"][:1], 40, 0), K1, K2))
    r = scene_pair(12, 0.1, n=150, baseline=0.0)
    cases.append(("pure_rotation", r["xy1"], r["xy2"], r["K1"], r["K2"]))
    p = scene_pair(13, 0.1, n=150, planar=True)
    cases.append(("planar", p["xy1"], p["xy2"], p["K1"], p["K2"]))
    Kn = K1.copy()
    Kn[0] = 0.0                         # (u - cx) / 0: inf and nan coordinates in the first image
    cases.append(("nan_coordinates", s["xy1"][:60], s["xy2"][:60], Kn, K2))
    rng = np.random.default_rng(14)
    cases.append(("random12", rng.integers(0, 1000, (12, 2)).astype(np.int32), rng.integers(0, 1000, (12, 2)).astype(np.int32), K1, K2))
    d = scene_pair(15, 0.3, n=250, distortion=True)
    cases.append(("distortion", d["xy1"], d["xy2"], d["K1"], d["K2"]))
    return cases
