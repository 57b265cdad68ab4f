"""One Levenberg-Marquardt step of the bundle adjustment (csrc/ba.hip) restated in numpy, generic over the dtype: the judge of
tests/test_ba_step_gpu.py (which feeds every stage the GPU's own captured inputs to that stage, tools/ba_step_check) and of
tests/test_ba_step_ref.py (which checks the judge itself on the CPU).  numpy only; np.longdouble is the x87 extended format here.

The residual is BundleAdjuster.h's functor over ceres::AngleAxisRotatePoint, first-order branch at theta^2 <= DBL_EPSILON included;
the Jacobian is its COMPLEX STEP, Im f(x + i h) / h with h = 1e-30 -- no subtraction, so no cancellation, and a derivation that shares
nothing with the kernel's analytic one.  It follows the branch the real part takes, so below sqrt(DBL_EPSILON) it is the derivative of
the first-order expression, as Ceres' jets give it.

Every stage is one function; `real` is np.longdouble (the reference) or np.float64 (the baseline whose own error sets the
function-type tolerances).  A sum-type stage returns (value, A, m): A the same expression on absolute values, m the number of
rounded operations on the longest path to an entry, so that |gpu - value| <= gamma(m) A holds for ANY summation order and for FMA
contraction (Higham, Accuracy and Stability of Numerical Algorithms, 3.1: a sum of L products carries at most L roundings on a path --
one for the product, L - 1 for the additions, fewer under FMA).  The counts, per stage:

  Uraw, gcraw    2 k_c          the camera's 2 k_c products (two rows per observation)
  Vraw, gpraw    2 k_j
  W              4              jc sa, . jp, +, . sp
  Y              3              three products, two additions
  gps            1
  S off-diagonal 3 P            P the entries of the block's pair list, three products each
  S diagonal     3 (k_c + P) + 3 (+ 2 on the diagonal itself)     ... + Uraw sc sc (two products, one addition) + dgc / radius
  rhs            3 k_c + 2      ... + gcraw sc
  tobs           dim_c
  stp            k_j + 3        g_p - sum t_o, then a row of Vinv
  dlc, dlp       2              alpha step scale
  model change   2 n_obs + 18   per row 13 products of pre-multiplied pairs, m (r + m / 2), the sum over both rows of all observations
  |dx|^2, |x|^2, g . delta      12 n_cams + 3 n_points + 2: one product per coordinate, squares of differences one rounding more
  cost           2 n_obs + 1    from the residuals the GPU wrote (current point)
"""
import os

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
EPS = float(np.finfo(np.float64).eps)      # DBL_EPSILON
BETA = 1.0e200                             # RCN_RHS_BETA (csrc/chol.h)
SENTINEL = 0xFFFFFFFFFFFFFFFF              # "not there yet" of the one-launch backward substitution
H = 1e-30
JROW, WROW, CROT, BLOCK = 28, 30, 28, 128


def cplx(real):
    return np.clongdouble if real is LD else np.complex128


def gamma(m):
    mu = np.asarray(m, dtype=LD) * LD(U)
    return mu / (1 - mu)


# ---------------------------------------------------------------------------------------------------------------------
# residual and Jacobian
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def rotate(w, X):
    """ceres::AngleAxisRotatePoint, rows of w and X; the branch is taken on the real part"""
    th2 = (w * w).sum(-1)
    big = np.real(th2) > EPS
    safe = np.where(big, th2, 1)
    th = np.sqrt(safe)
    c, s = np.cos(th), np.sin(th)
    n = w / th[..., None]
    tmp = (n * X).sum(-1) * (1 - c)
    p_big = X * c[..., None] + _cross(n, X) * s[..., None] + n * tmp[..., None]
    p_small = X + _cross(w, X)
    return np.where(big[..., None], p_big, p_small)


def residual(pose, intr, X, uv):
    """BundleAdjuster.h:27-58 for rows of (pose 6, intrinsics 6, point 3, observed pixel 2) of any one dtype, complex included"""
    p = rotate(pose[..., :3], X) + pose[..., 3:]
    x, y = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    rr = x * x + y * y
    dist = intr[..., 4] * rr + intr[..., 5] * rr * rr
    return np.stack([intr[..., 0] * (x + dist) + intr[..., 2] - uv[..., 0], intr[..., 1] * (y + dist) + intr[..., 3] - uv[..., 1]], -1)


def depth(pose, X):
    return np.real(rotate(pose[..., :3], X)[..., 2] + pose[..., 5])


def residual_jacobian(pose, intr, X, uv, real=LD):
    """(r [N, 2], J [N, 2, 15] over pose 6 | intrinsics 6 | point 3) in `real`; J by the complex step"""
    ct = cplx(real)
    par = np.concatenate([np.asarray(pose, real), np.asarray(intr, real), np.asarray(X, real)], -1)
    uvr = np.asarray(uv, real)
    r = residual(par[..., :6], par[..., 6:12], par[..., 12:], uvr)
    J = np.empty(r.shape + (15,), real)
    uvc = uvr.astype(ct)
    for k in range(15):
        z = par.astype(ct)
        z[..., k] += ct(1j) * ct(H)
        J[..., k] = np.imag(residual(z[..., :6], z[..., 6:12], z[..., 12:], uvc)) / real(H)
    return r, J


# ---------------------------------------------------------------------------------------------------------------------
# structure
def structure(nc, mode, fix0, fix1):
    """tangent columns from the options (BundleAdjuster.cpp:99-129): cols [nc, 10], cam_dim [nc], cam_off [nc + 1]"""
    cols = np.zeros((nc, 10), np.int32)
    dim = np.zeros(nc, np.int32)
    for c in range(nc):
        k = []
        if not (c == 0 and fix0):
            k += list(range(3 if (c == 1 and fix1) else 6))
        if mode == 1:
            k += [6, 7, 10, 11]
        cols[c, :len(k)] = k
        dim[c] = len(k)
    off = np.concatenate([[0], np.cumsum(dim)]).astype(np.int32)
    return cols, dim, off


def padded(n):
    return max(BLOCK, (n + BLOCK - 1) // BLOCK * BLOCK)


def cam_split(nc, max_cam_obs):
    """workgroups a camera is split over (the per-camera kernels): restated to say what a scene is FOR; the test asserts the captured value"""
    return 1 if nc >= 128 else max(1, min(min(16, 512 // max(nc, 1)), (max_cam_obs + 767) // 768))


def obs_rows(poses, intr, pts, uv, ocam, opt, cols, dim, real=LD):
    """the observation rows as k_ba_eval<true> writes them: [N, 28] = tangent camera Jacobian 2 x 10 | point Jacobian 2 x 3 | residual"""
    r, J = residual_jacobian(np.asarray(poses)[ocam], np.asarray(intr)[ocam], np.asarray(pts)[opt], uv, real)
    N = len(ocam)
    rows = np.zeros((N, JROW), real)
    on = np.arange(10)[None, :] < dim[ocam][:, None]
    for i in range(2):
        rows[:, 10 * i:10 * i + 10] = np.where(on, np.take_along_axis(J[:, i, :], cols[ocam].astype(np.int64), 1), 0)
        rows[:, 20 + 3 * i:23 + 3 * i] = J[:, i, 12:]
    rows[:, 26:] = r
    return rows


def cam_rot_table(poses, real=LD):
    """k_ba_cam_rot's table per camera: R 9, right Jacobian Jr 9, cos, sin, axis 3, small-angle flag, w 3, 0.  R = I + sin K + (1 - cos) K^2
    on the unit axis, Jr = I - a K(w) + b K(w)^2 with a = (1 - cos) / th^2 and b = (th - sin) / th^3, both by their Taylor series below
    th = 0.1 (16 terms: exact to the last bit in either dtype, where the closed forms cancel); first-order branch: R = I + K(w), Jr = I"""
    w = np.asarray(poses, real)[:, :3]
    nc = len(w)
    out = np.zeros((nc, CROT), real)
    for c in range(nc):
        v = w[c]
        th2 = (v * v).sum()
        K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], real)
        I = np.eye(3, dtype=real)
        if th2 > EPS:
            th = np.sqrt(th2)
            cs, sn = np.cos(th), np.sin(th)
            n = v / th
            Kn = K / th
            hs = np.sin(th / 2)
            R = I + sn * Kn + 2 * hs * hs * (Kn @ Kn)
            if th < 0.1:
                a = b = real(0)
                ta, tb = real(1) / 2, real(1) / 6
                for k in range(16):
                    a, b = a + ta, b + tb
                    ta = -ta * th2 / ((2 * k + 3) * (2 * k + 4))
                    tb = -tb * th2 / ((2 * k + 4) * (2 * k + 5))
            else:
                a, b = 2 * hs * hs / th2, (th - sn) / (th2 * th)
            Jr = I - a * K + b * (K @ K)
            out[c, :9], out[c, 9:18] = R.reshape(-1), Jr.reshape(-1)
            out[c, 18], out[c, 19], out[c, 20:23], out[c, 23] = cs, sn, n, 0
        else:
            out[c, :9], out[c, 9:18] = (I + K).reshape(-1), I.reshape(-1)
            out[c, 18], out[c, 19], out[c, 23] = 1, 0, 1
        out[c, 24:27] = v
    return out


# ---------------------------------------------------------------------------------------------------------------------
# normal blocks
def normal_blocks(rows, ocam, opt, nc, npts, real=LD):
    """per camera Uraw = sum Jc'Jc [10, 10], gcraw = sum Jc'r [10]; per landmark Vraw [3, 3], gpraw [3].  Returns a dict of
    (value, A, m) per name"""
    rows = np.asarray(rows, real)
    out = {}
    kc = np.bincount(ocam, minlength=nc)
    kj = np.bincount(opt, minlength=npts)
    for tag, idx, cnt, a0, w in (("cam", ocam, kc, 0, 10), ("pt", opt, kj, 20, 3)):
        vals = []
        for src in (rows, np.abs(rows)):
            ja, jb, r = src[:, a0:a0 + w], src[:, a0 + w:a0 + 2 * w], src[:, 26:]
            blk = ja[:, :, None] * ja[:, None, :] + jb[:, :, None] * jb[:, None, :]
            g = ja * r[:, :1] + jb * r[:, 1:]
            B = np.zeros((len(cnt), w, w), real)
            G = np.zeros((len(cnt), w), real)
            np.add.at(B, idx, blk)
            np.add.at(G, idx, g)
            vals.append((B, G))
        m = 2 * cnt
        names = ("Uraw", "gcraw") if tag == "cam" else ("Vraw", "gpraw")
        out[names[0]] = (vals[0][0], vals[1][0], m[:, None, None])
        out[names[1]] = (vals[0][1], vals[1][1], m[:, None])
    return out


def reduced_diag(Uraw, dim, off):
    """diagonal of the camera blocks in reduced order [n]"""
    U_ = np.asarray(Uraw).reshape(-1, 10, 10)
    return np.concatenate([np.diagonal(U_[c])[:dim[c]] for c in range(len(dim))]) if off[-1] else np.zeros(0, U_.dtype)


def jacobi_scale(diag, jacobi, real=LD):
    d = np.asarray(diag, real)
    return 1 / (1 + np.sqrt(d)) if jacobi else np.ones_like(d)


def lm_diagonal(diag, scale, lo, hi, real=LD):
    d, s = np.asarray(diag, real), np.asarray(scale, real)
    return np.minimum(np.maximum(d * s * s, real(lo)), real(hi))


def point_solve(Vraw, sp, dgp, gpraw, inv_radius, real=LD):
    """V = scaled Vraw + dgp / radius, its inverse by the adjugate [np, 3, 3]; gps = gpraw sp as (value, A, m)"""
    V = np.asarray(Vraw, real).reshape(-1, 3, 3)
    s = np.asarray(sp, real).reshape(-1, 3)
    V = V * s[:, :, None] * s[:, None, :]
    i3 = np.arange(3)
    V[:, i3, i3] += np.asarray(dgp, real).reshape(-1, 3) * real(inv_radius)
    a, b, c, e, f, g = V[:, 0, 0], V[:, 0, 1], V[:, 0, 2], V[:, 1, 1], V[:, 1, 2], V[:, 2, 2]
    A, B, C = e * g - f * f, c * f - b * g, b * f - c * e
    det = a * A + b * B + c * C
    Vi = np.stack([A, B, C, B, a * g - c * c, b * c - a * f, C, b * c - a * f, a * e - b * b], -1) / det[:, None]
    gp = np.asarray(gpraw, real).reshape(-1, 3)
    return Vi.reshape(-1, 3, 3), det, (gp * s, np.abs(gp * s), 1)


def w_plane(rows, sc, sp, ocam, opt, dim, off, real=LD):
    """scaled W_o = Jc'Jp as the plane holds it, [N, 3, 10] (camera coordinate fastest, zero beyond the camera's dimension): (value, A, 4)"""
    out = []
    scf = np.asarray(sc, real)
    k = np.arange(10)
    on = k[None, :] < dim[ocam][:, None]
    sa = np.where(on, scf[np.minimum(off[ocam][:, None] + k[None, :], max(len(scf) - 1, 0))] if len(scf) else 0, 0)
    spj = np.asarray(sp, real).reshape(-1, 3)[opt]
    for src in (np.asarray(rows, real), np.abs(np.asarray(rows, real))):
        j0, j1 = src[:, 0:10] * sa, src[:, 10:20] * sa
        W = (j0[:, None, :] * src[:, 20:23, None] + j1[:, None, :] * src[:, 23:26, None]) * spj[:, :, None]
        out.append(W)
    return out[0], out[1], 4


def y_plane(W, Vinv, opt, real=LD):
    """Y_o = W_o Vinv: Y[o, m, a] = sum_k W[o, k, a] Vinv[j, k, m]: (value, A, 3)"""
    W = np.asarray(W, real).reshape(-1, 3, 10)
    Vi = np.asarray(Vinv, real).reshape(-1, 3, 3)[opt]
    Y = np.einsum("oka,okm->oma", W, Vi)
    A = np.einsum("oka,okm->oma", np.abs(W), np.abs(Vi))
    return Y, A, 3


# ---------------------------------------------------------------------------------------------------------------------
# pair lists
def pair_lists(ocam, pt_off, dim, nc):
    """(pk_off [nc nc + 1], pk_list uint64): per key c nc + c2 with c2 <= c the ascending (o << 32 | o2) over the ordered pairs o != o2
    of one landmark whose two cameras both have a free parameter"""
    ocam = np.asarray(ocam, np.int64)
    k = np.diff(pt_off)
    keys, vals = [], []
    for kk in np.unique(k):
        if kk < 2:
            continue
        first = np.asarray(pt_off[:-1])[k == kk].astype(np.int64)
        o = first[:, None, None] + np.arange(kk)[None, :, None] + np.zeros((1, 1, kk), np.int64)
        o2 = first[:, None, None] + np.arange(kk)[None, None, :] + np.zeros((1, kk, 1), np.int64)
        c, c2 = ocam[o], ocam[o2]
        m = (o != o2) & (c2 <= c) & (dim[c] > 0) & (dim[c2] > 0)
        keys.append((c * nc + c2)[m])
        vals.append(((o << 32) | o2)[m])
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    vals = np.concatenate(vals) if vals else np.zeros(0, np.int64)
    order = np.lexsort((vals, keys))
    keys, vals = keys[order], vals[order]
    off = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=nc * nc))]).astype(np.int32)
    return off, vals.astype(np.uint64), keys


# ---------------------------------------------------------------------------------------------------------------------
# reduced system
def reduced_system(W, Y, gps, Uraw, gcraw, sc, dgc, inv_radius, ocam, opt, dim, off, pk_keys, pk_list, nc, real=LD, chunk=20000):
    """S = Us + D / radius - sum Y W' (lower block triangle, dense [n, n]) and rhs = gcs - sum Y gps, by plain sums over each block's
    pairs: ((S, A_S, m_S), (rhs, A_rhs, m_rhs)).  Blocks above the diagonal stay zero."""
    n = int(off[-1])
    W = np.asarray(W, real).reshape(-1, 3, 10)
    Y = np.asarray(Y, real).reshape(-1, 3, 10)
    nkeys = nc * nc
    N = len(ocam)
    # the pairs: the listed ones and every observation of a free camera with itself
    free = dim[ocam] > 0
    self_o = np.flatnonzero(free).astype(np.int64)
    o1 = np.concatenate([(np.asarray(pk_list, np.uint64) >> np.uint64(32)).astype(np.int64), self_o])
    o2 = np.concatenate([(np.asarray(pk_list, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64), self_o])
    key = np.concatenate([np.asarray(pk_keys, np.int64), ocam[self_o].astype(np.int64) * nc + ocam[self_o]])
    cnt = np.bincount(key, minlength=nkeys)
    B = np.zeros((nkeys, 10, 10), real)
    BA = np.zeros((nkeys, 10, 10), real)
    for s in range(0, len(key), chunk):
        e = slice(s, s + chunk)
        np.add.at(B, key[e], np.einsum("pma,pmb->pab", Y[o1[e]], W[o2[e]]))
        np.add.at(BA, key[e], np.einsum("pma,pmb->pab", np.abs(Y[o1[e]]), np.abs(W[o2[e]])))
    S = np.zeros((n, n), real)
    A = np.zeros((n, n), real)
    M = np.zeros((n, n), np.int64)
    scf, dg = np.asarray(sc, real), np.asarray(dgc, real)
    Ur = np.asarray(Uraw, real).reshape(-1, 10, 10)
    for c in range(nc):
        dc, oc = int(dim[c]), int(off[c])
        if dc == 0:
            continue
        for c2 in range(c + 1):
            d2, o2c = int(dim[c2]), int(off[c2])
            if d2 == 0:
                continue
            k = c * nc + c2
            S[oc:oc + dc, o2c:o2c + d2] = -B[k, :dc, :d2]
            A[oc:oc + dc, o2c:o2c + d2] = BA[k, :dc, :d2]
            M[oc:oc + dc, o2c:o2c + d2] = 3 * cnt[k]
        s = scf[oc:oc + dc]
        S[oc:oc + dc, oc:oc + dc] += Ur[c, :dc, :dc] * s[:, None] * s[None, :]
        A[oc:oc + dc, oc:oc + dc] += np.abs(Ur[c, :dc, :dc]) * s[:, None] * s[None, :]
        M[oc:oc + dc, oc:oc + dc] += 3
        i = np.arange(oc, oc + dc)
        S[i, i] += dg[oc:oc + dc] * real(inv_radius)
        A[i, i] += dg[oc:oc + dc] * real(inv_radius)
        M[i, i] += 2
    g = np.asarray(gps, real).reshape(-1, 3)[opt]
    t = np.einsum("oma,om->oa", Y, g)
    ta = np.einsum("oma,om->oa", np.abs(Y), np.abs(g))
    R = np.zeros((nc, 10), real)
    RA = np.zeros((nc, 10), real)
    np.add.at(R, ocam, t)
    np.add.at(RA, ocam, ta)
    kc = np.bincount(ocam, minlength=nc)
    gc = np.asarray(gcraw, real).reshape(-1, 10)
    rhs = np.zeros(n, real)
    ra = np.zeros(n, real)
    rm = np.zeros(n, np.int64)
    for c in range(nc):
        dc, oc = int(dim[c]), int(off[c])
        rhs[oc:oc + dc] = gc[c, :dc] * scf[oc:oc + dc] - R[c, :dc]
        ra[oc:oc + dc] = np.abs(gc[c, :dc]) * scf[oc:oc + dc] + RA[c, :dc]
        rm[oc:oc + dc] = 3 * kc[c] + 2
    return (S, A, M), (rhs, ra, rm)


# ---------------------------------------------------------------------------------------------------------------------
# back-substitution, model, Plus
def backsub(W, y, gps, Vinv, ocam, opt, pt_off, dim, off, tobs_in=None, real=LD):
    """t_o = W_o' y_c [N, 3] as (value, A, dim_c per row); the scaled point step -Vinv (g_p - sum_o t_o) [np, 3] as (value, A, k_j + 3) --
    from `tobs_in` (the GPU's own per-observation terms) when given"""
    W = np.asarray(W, real).reshape(-1, 3, 10)
    y = np.asarray(y, real)
    k = np.arange(10)
    on = k[None, :] < dim[ocam][:, None]
    yo = np.where(on, y[np.minimum(off[ocam][:, None] + k[None, :], max(len(y) - 1, 0))] if len(y) else 0, 0)
    t = np.einsum("oma,oa->om", W, yo)
    ta = np.einsum("oma,oa->om", np.abs(W), np.abs(yo))
    tin = t if tobs_in is None else np.asarray(tobs_in, real).reshape(-1, 3)
    npts = len(pt_off) - 1
    g = np.asarray(gps, real).reshape(-1, 3)
    tt = g.copy()
    tta = np.abs(g)
    np.subtract.at(tt, opt, tin)
    np.add.at(tta, opt, np.abs(tin))
    Vi = np.asarray(Vinv, real).reshape(-1, 3, 3)
    stp = -np.einsum("jab,jb->ja", Vi, tt)
    stpa = np.einsum("jab,jb->ja", np.abs(Vi), tta)
    return (t, ta, np.maximum(dim[ocam], 0)[:, None]), (stp, stpa, (np.diff(pt_off)[:npts] + 3)[:, None])


def model_change(rows, sc, stc, sp, stp, ocam, opt, dim, off, real=LD):
    """-sum_o m (r + m / 2), m = Js step: (value, A, 2 N + 18)"""
    rows = np.asarray(rows, real)
    k = np.arange(10)
    on = k[None, :] < dim[ocam][:, None]
    v = np.asarray(sc, real) * np.asarray(stc, real)
    vc = np.where(on, v[np.minimum(off[ocam][:, None] + k[None, :], max(len(v) - 1, 0))] if len(v) else 0, 0)
    vp = (np.asarray(sp, real) * np.asarray(stp, real)).reshape(-1, 3)[opt]
    tot, tota = real(0), real(0)
    for i in range(2):
        m = (rows[:, 10 * i:10 * i + 10] * vc).sum(1) + (rows[:, 20 + 3 * i:23 + 3 * i] * vp).sum(1)
        ma = (np.abs(rows[:, 10 * i:10 * i + 10]) * np.abs(vc)).sum(1) + (np.abs(rows[:, 20 + 3 * i:23 + 3 * i]) * np.abs(vp)).sum(1)
        r = rows[:, 26 + i]
        tot = tot + (m * (r + m / 2)).sum()
        tota = tota + (ma * (np.abs(r) + ma / 2)).sum()
    return -tot, tota, 2 * len(rows) + 18


def plus(poses, intr, pts, dlc, dlp, cols, dim, off, mode, ub, gcraw, gpraw, cam_used, pt_used, fix0, real=LD):
    """candidate = clamp(x + delta) (Plus, with the focal clamp of mode 1) and the three sums of k_ba_plus:
    dict(poses2, intr2, pts2, dx2, x2, gd) -- the sums as (value, A, m)"""
    P = np.asarray(poses, real).copy()
    I = np.asarray(intr, real).copy()
    X = np.asarray(pts, real).reshape(-1, 3)
    P0, I0 = P.copy(), I.copy()
    dl = np.asarray(dlc, real)
    gd = gda = real(0)
    gc = np.asarray(gcraw, real).reshape(-1, 10)
    for c in range(len(dim)):
        for k in range(int(dim[c])):
            col, d = int(cols[c, k]), dl[off[c] + k]
            gd, gda = gd + gc[c, k] * d, gda + abs(gc[c, k] * d)
            if col < 6:
                P[c, col] += d
            else:
                I[c, col - 6] += d
                if mode == 1 and col - 6 < 2 and I[c, col - 6] > real(ub):
                    I[c, col - 6] = real(ub)
    dp = np.asarray(dlp, real).reshape(-1, 3)
    gp = np.asarray(gpraw, real).reshape(-1, 3)
    gd, gda = gd + (gp * dp).sum(), gda + np.abs(gp * dp).sum()
    dx2 = ((P - P0) ** 2).sum() + ((I - I0) ** 2).sum() + (dp * dp).sum()
    pose_in = cam_used & (dim > 0) & (cols[:, 0] < 6)
    intr_in = cam_used & (mode == 1)
    x2 = (P0[pose_in] ** 2).sum() + (I0[intr_in] ** 2).sum() + (X[pt_used] ** 2).sum()
    m = 12 * len(dim) + 3 * len(X) + 2
    return dict(poses2=P, intr2=I, pts2=X + dp, dx2=(dx2, dx2, m), x2=(x2, x2, m), gd=(gd, gda, m))


def projected_gradient_max(gcraw, gpraw, intr, cols, dim, mode, ub):
    """max |x - clamp(x - g)| over the free coordinates in float64: the same IEEE operations as the kernel's, so the same bits"""
    m = 0.0
    gc = np.asarray(gcraw, np.float64).reshape(-1, 10)
    for c in range(len(dim)):
        for k in range(int(dim[c])):
            g, col = gc[c, k], int(cols[c, k])
            if mode == 1 and col in (6, 7):
                x = np.float64(intr[c][col - 6])
                g = x - min(x - g, np.float64(ub))
            m = max(m, abs(g))
    gp = np.asarray(gpraw, np.float64)
    return max(m, float(np.abs(gp).max()) if gp.size else 0.0)


def directional_derivative(poses, intr, pts, uv, ocam, opt, cols, dim, off, dlc, dlp, real=LD):
    """sum_o r_o' (Jc_o dlc + Jp_o dlp) at a trial point: (value, A, 2 N + 16)"""
    return gradient_along(obs_rows(poses, intr, pts, uv, ocam, opt, cols, dim, real), dlc, dlp, ocam, opt, dim, off, real)


def gradient_along(rows, dlc, dlp, ocam, opt, dim, off, real=LD):
    """sum_o r_o' (Jc_o dlc + Jp_o dlp) from observation rows"""
    rows = np.asarray(rows, real)
    k = np.arange(10)
    on = k[None, :] < dim[ocam][:, None]
    v = np.asarray(dlc, real)
    vc = np.where(on, v[np.minimum(off[ocam][:, None] + k[None, :], max(len(v) - 1, 0))] if len(v) else 0, 0)
    vp = np.asarray(dlp, real).reshape(-1, 3)[opt]
    tot = tota = real(0)
    for i in range(2):
        m = (rows[:, 10 * i:10 * i + 10] * vc).sum(1) + (rows[:, 20 + 3 * i:23 + 3 * i] * vp).sum(1)
        ma = (np.abs(rows[:, 10 * i:10 * i + 10]) * np.abs(vc)).sum(1) + (np.abs(rows[:, 20 + 3 * i:23 + 3 * i]) * np.abs(vp)).sum(1)
        tot, tota = tot + (rows[:, 26 + i] * m).sum(), tota + (np.abs(rows[:, 26 + i]) * ma).sum()
    return tot, tota, 2 * len(rows) + 16


def cost_of(r, real=LD):
    r = np.asarray(r, real)
    c = (r * r).sum() / 2
    return c, c, r.size + 1


# ---------------------------------------------------------------------------------------------------------------------
# one whole step from the problem's inputs (the end-to-end check, and the CPU tests of the judge)
def full_step(sc, opts, radius, real=LD):
    """delta of the first LM iteration from the scene's inputs, every stage chained in `real`.  opts: dict(mode, fix0, fix1, jacobi, ub,
    lo, hi).  Returns a dict of every intermediate."""
    nc, npts = len(sc["poses"]), len(sc["points"])
    ocam, opt = np.asarray(sc["obs_cam"], np.int64), np.asarray(sc["obs_pt"], np.int64)
    pt_off = np.concatenate([[0], np.cumsum(np.bincount(opt, minlength=npts))]).astype(np.int64)
    cols, dim, off = structure(nc, opts["mode"], opts["fix0"], opts["fix1"])
    intr = np.array(sc["intrinsics"], np.float64)
    if opts["mode"] == 1:
        intr[:, :2] = np.minimum(intr[:, :2], opts["ub"])
    rows = obs_rows(sc["poses"], intr, sc["points"], sc["obs_uv"], ocam, opt, cols, dim, real)
    nb = normal_blocks(rows, ocam, opt, nc, npts, real)
    Uraw, gcraw, Vraw, gpraw = (nb[k][0] for k in ("Uraw", "gcraw", "Vraw", "gpraw"))
    du, dv = reduced_diag(Uraw, dim, off), np.diagonal(Vraw, axis1=1, axis2=2).reshape(-1)
    scl, spl = jacobi_scale(du, opts["jacobi"], real), jacobi_scale(dv, opts["jacobi"], real)
    dgc, dgp = lm_diagonal(du, scl, opts["lo"], opts["hi"], real), lm_diagonal(dv, spl, opts["lo"], opts["hi"], real)
    ir = real(1) / real(radius)
    Vinv, det, (gps, _, _) = point_solve(Vraw, spl, dgp, gpraw, ir, real)
    W, _, _ = w_plane(rows, scl, spl, ocam, opt, dim, off, real)
    Y, _, _ = y_plane(W, Vinv, opt, real)
    pk_off, pk_list, pk_keys = pair_lists(ocam, pt_off, dim, nc)
    (S, _, _), (rhs, _, _) = reduced_system(W, Y, gps, Uraw, gcraw, scl, dgc, ir, ocam, opt, dim, off, pk_keys, pk_list, nc, real)
    Sf = np.tril(S) + np.tril(S, -1).T
    y = solve_spd(Sf, rhs, real)
    (tobs, _, _), (stp, _, _) = backsub(W, y, gps, Vinv, ocam, opt, pt_off, dim, off, None, real)
    stc = -y
    return dict(rows=rows, Uraw=Uraw, gcraw=gcraw, Vraw=Vraw, gpraw=gpraw, sc=scl, sp=spl, dgc=dgc, dgp=dgp, Vinv=Vinv, gps=gps, W=W, Y=Y,
                S=Sf, rhs=rhs, y=y, stc=stc, stp=stp.reshape(-1), dlc=stc * scl, dlp=stp.reshape(-1) * spl, cols=cols, dim=dim, off=off,
                pt_off=pt_off, intr=intr, pk_off=pk_off, pk_list=pk_list, cost=cost_of(rows[:, 26:], real)[0])


def solve_spd(S, b, real=LD, steps=4):
    """S x = b: LAPACK in float64, refined in `real` (tests/chol_ref.py's scheme) when real is long double"""
    S64, b64 = np.asarray(S, np.float64), np.asarray(b, np.float64)
    if S64.shape[0] == 0:
        return np.zeros(0, real)
    L = np.linalg.cholesky(S64)

    def sol(r):
        return np.linalg.solve(L.T, np.linalg.solve(L, r))
    x = sol(b64).astype(real)
    if real is LD:
        Sl, bl = np.asarray(S, LD), np.asarray(b, LD)
        for _ in range(steps):
            r = bl - (Sl * x[None, :]).sum(axis=1)
            x = x + sol(r.astype(np.float64)).astype(LD)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the tool's files
def write_scene(d, name, sc):
    nc, npts, no = len(sc["poses"]), len(sc["points"]), len(sc["obs_cam"])
    with open(os.path.join(d, name + ".dims"), "w") as f:
        f.write("%d %d %d\n" % (nc, npts, no))
    for ext, key, dt in ((".poses", "poses", "<f8"), (".intr", "intrinsics", "<f8"), (".pts", "points", "<f8"), (".uv", "obs_uv", "<f8"),
                         (".ocam", "obs_cam", "<i4"), (".opt", "obs_pt", "<i4")):
        np.ascontiguousarray(sc[key], dtype=dt).tofile(os.path.join(d, name + ext))


def write_cases(d, cases):
    """cases: dicts(name, scene, iteration, mode, fix0, fix1, jacobi, ub, radius[, lm]); lm: (min_lm_diagonal, max_lm_diagonal), absent or
    None for the defaults -- the line then has no such columns"""
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("# name scene iteration intrinsics_mode fix_cam0_pose fix_cam1_translation jacobi_scaling focal_upper_bound initial_radius [min_lm_diagonal max_lm_diagonal]\n")
        for c in cases:
            lm = c.get("lm")
            f.write("%s %s %d %d %d %d %d %.17g %.17g%s\n" % (c["name"], c["scene"], c["iteration"], c["mode"], c["fix0"], c["fix1"], c["jacobi"], c["ub"], c["radius"],
                                                          "" if lm is None else " %.17g %.17g" % tuple(lm)))


_TYPES = dict(flag="<i4", flag_b="<i4", cam_off="<i4", cam_dim="<i4", cols="<i4", pk_off="<i4", tickets="<u4", tickets_b="<u4", pk_list="<u8")
ARRAYS = ("J crot Uraw gcraw Vraw gpraw sc sp dgc dgp Vinv gps WY S rhs flag cam_off cam_dim cols pk_off tickets pk_list "
          "x tobs stc stp dlc dlp poses2 intr2 pts2 crot2 scal flag_b tickets_b trials log").split()


def read_capture(d, name):
    cap = {}
    with open(os.path.join(d, name + ".meta")) as f:
        for line in f:
            k, v = line.split()
            cap[k] = float(v) if k == "radius" else int(v)
    for a in ARRAYS:
        cap[a] = np.fromfile(os.path.join(d, name + "." + a), dtype=_TYPES.get(a, "<f8"))
    return cap
