"""Shared intrinsics of the bundle adjuster (cameras tied in groups): the judge (test helper, CPU only).  Shares no code with the library.

  (a) judge       scipy.optimize.least_squares on synth_ba.project residuals over the free poses, the observed points and ONE intrinsics
                  vector (fx, fy, k1, k2) per group or per camera of its own -- another minimiser (trust-region reflective or dogleg on a
                  finite-difference Jacobian) than the library's Levenberg-Marquardt on analytic derivatives.
  (b) tied_step   one LM step in long double (and the same in float64 beside it): the observation rows of tests/ba_ref.py, the columns
                  tied (J' = J P), then Ceres' arithmetic with one parameter block per group: scale 1 / (1 + sqrt(diag J'^T J')), damping
                  clamp(scale^2 diag, lo, hi) / radius, normal equations, the step expanded to the per-camera parameters.

normalise() restates the rules of include/rcn.h: a group of one camera is a camera of its own; a group with a constant member is held
(its free members keep their pose columns only); live groups are numbered in ascending order of their smallest member.
tests/test_ba_tied_ref.py checks the judge itself; tests/golden/make_ba_tied_golden.py records its results for the GPU suite."""
import functools
import os

import numpy as np

from reconstructor_amd import synth_ba

import ba_graphs
import ba_ref as B

LD = B.LD
OWN, HELD = -1, -2
ICOL = (0, 1, 4, 5)          # fx, fy, k1, k2 inside a camera's six intrinsics
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_tied_judge.npz")


def normalise(nc, groups, constant=None, mode=1):
    """-> (grp [nc]: OWN, HELD or the live group's number; members: list of arrays, one per live group)"""
    grp = np.full(nc, OWN, np.int64)
    constant = np.zeros(nc, bool) if constant is None else np.asarray(constant, bool)
    members = []
    if groups is None or mode != 1:
        return grp, members
    groups = np.asarray(groups)
    assert groups.shape == (nc,) and (groups >= -1).all()
    firsts = []
    for gid in np.unique(groups[groups >= 0]):
        m = np.flatnonzero(groups == gid)
        if len(m) < 2:
            continue
        if constant[m].any():
            grp[m[~constant[m]]] = HELD
        else:
            firsts.append((m[0], m))
    for k, (_, m) in enumerate(sorted(firsts, key=lambda t: t[0])):
        grp[m] = k
        members.append(m)
    return grp, members


def structure(nc, groups, constant=None, mode=1, fix=(1, 1)):
    """Per-camera tangent columns (ba_ref.structure with constant and held cameras) and the map onto the tied columns:
    dict(cols, dim, off, map, n, n_tied, n_own, grp, members)"""
    constant = np.zeros(nc, bool) if constant is None else np.asarray(constant, bool)
    grp, members = normalise(nc, groups, constant, mode)
    cols, dim = np.zeros((nc, 10), np.int32), np.zeros(nc, np.int32)
    cmap, a = [], 0
    for c in range(nc):
        k = []
        if not constant[c] and not (c == 0 and fix[0]):
            k += list(range(3 if (c == 1 and fix[1]) else 6))
            cmap += list(range(a, a + len(k)))
            a += len(k)
        if not constant[c] and mode == 1 and grp[c] != HELD:
            k += [6, 7, 10, 11]
            if grp[c] == OWN:
                cmap += list(range(a, a + 4))
                a += 4
            else:
                cmap += [-1 - 4 * grp[c] - j for j in range(4)]
        cols[c, :len(k)], dim[c] = k, len(k)
    cmap = np.array(cmap, np.int64)
    neg = cmap < 0
    cmap[neg] = a + (-1 - cmap[neg])
    off = np.concatenate([[0], np.cumsum(dim)]).astype(np.int32)
    return dict(cols=cols, dim=dim, off=off, map=cmap, n=int(off[-1]), n_tied=a + 4 * len(members), n_own=a, grp=grp, members=members)


# ---------------------------------------------------------------------------------------------------------------- (a)
def rho_scaled(r, loss):
    """r [N, 2] -> the residuals whose squares sum to the robust cost: r sqrt(rho(s) / s)"""
    if loss is None:
        return r
    kind, a = loss
    assert kind == "cauchy"
    b = a * a
    s = (r * r).sum(1)
    w = np.where(s > 0, b * np.log1p(s / b) / np.where(s > 0, s, 1), 1.0)
    return r * np.sqrt(w)[:, None]


def judge(sc, groups, constant=None, fix=(1, 1), mode=1, method="trf", loss=None, ub=np.inf):
    """Minimise the (robust) reprojection error over the free poses, the observed points and one (fx, fy, k1, k2) per group / own camera.
    Returns (poses, intrinsics, points, rms in pixels of the plain residuals)."""
    from scipy.optimize import least_squares
    nc = len(sc["poses"])
    constant = np.zeros(nc, bool) if constant is None else np.asarray(constant, bool)
    grp, members = normalise(nc, groups, constant, mode)
    pose_idx = []
    for c in range(nc):
        if constant[c] or (c == 0 and fix[0]):
            continue
        pose_idx += [(c, k) for k in range(3 if (c == 1 and fix[1]) else 6)]
    pc, pk = (np.array([t[i] for t in pose_idx], np.int64) for i in (0, 1))
    units = [np.array([c]) for c in range(nc) if mode == 1 and not constant[c] and grp[c] == OWN] + list(members)
    seen = np.zeros(len(sc["points"]), bool)
    seen[sc["obs_pt"]] = True
    fp = np.flatnonzero(seen)
    P0, X0 = np.array(sc["poses"], np.float64), np.array(sc["points"], np.float64)
    I0 = np.array(sc["intrinsics"], np.float64)
    if mode == 1:
        for u in units:
            I0[u, :2] = np.minimum(I0[u, :2], ub)
    cam, pt, uv0 = sc["obs_cam"], sc["obs_pt"], sc["obs_uv"]
    n_p, n_i = len(pc), 4 * len(units)

    def unpack(x):
        P, I, X = P0.copy(), I0.copy(), X0.copy()
        P[pc, pk] = x[:n_p]
        for j, u in enumerate(units):
            I[np.ix_(u, ICOL)] = x[n_p + 4 * j:n_p + 4 * j + 4]
        X[fp] = x[n_p + n_i:].reshape(-1, 3)
        return P, I, X

    def fun(x):
        P, I, X = unpack(x)
        uv, _ = synth_ba.project(P[cam], I[cam], X[pt])
        return rho_scaled(uv - uv0, loss).reshape(-1)

    x0 = np.concatenate([P0[pc, pk], np.concatenate([I0[u[0], ICOL] for u in units]) if units else np.zeros(0), X0[fp].reshape(-1)])
    hi = np.full(len(x0), np.inf)
    for j in range(len(units)):
        hi[n_p + 4 * j:n_p + 4 * j + 2] = ub
    r = least_squares(fun, x0, jac="3-point", method=method, x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=400,
                      bounds=(np.full(len(x0), -np.inf), hi))
    P, I, X = unpack(r.x)
    uv, _ = synth_ba.project(P[cam], I[cam], X[pt])
    return P, I, X, float(np.sqrt(((uv - uv0) ** 2).sum() / max(len(pt), 1)))


# ---------------------------------------------------------------------------------------------------------------- (b)
def tied_step(sc, groups, constant=None, fix=(1, 1), mode=1, jacobi=1, ub=1000.0, lo=1e-6, hi=1e32, radius=1e4, loss=None, real=LD):
    """The first LM step, x_out - x_in per parameter, with one block per group.  Returns dict(dP [nc, 6], dI [nc, 6], dX [np, 3], n_tied)."""
    nc, npts = len(sc["poses"]), len(sc["points"])
    st = structure(nc, groups, constant, mode, fix)
    cols, dim, off, cmap, n, nt = st["cols"], st["dim"], st["off"], st["map"], st["n"], st["n_tied"]
    ocam, opt = np.asarray(sc["obs_cam"], np.int64), np.asarray(sc["obs_pt"], np.int64)
    intr = np.array(sc["intrinsics"], np.float64)
    if mode == 1:
        free_intr = np.array([10 in cols[c, :dim[c]] for c in range(nc)])      # the cameras whose intrinsics move: projected onto the box at entry
        intr[free_intr, :2] = np.minimum(intr[free_intr, :2], ub)
    rows = B.obs_rows(sc["poses"], intr, sc["points"], sc["obs_uv"], ocam, opt, cols, dim, real)
    if loss is not None:      # Ceres' corrector with rho'' <= 0: the row times sqrt(rho'(s))
        assert loss[0] == "cauchy"
        sq = (rows[:, 26:] ** 2).sum(1)
        rows = rows * np.sqrt(1 / (1 + sq / real(loss[1] * loss[1])))[:, None]
    m = nt + 3 * npts
    # H' = J'^T J' and g' = J'^T r with J' = J P, accumulated observation by observation (the tied column of every entry of a row)
    k10 = np.arange(10)
    on = k10[None, :] < dim[ocam][:, None]
    ccol = np.where(on, cmap[np.minimum(off[ocam][:, None] + k10[None, :], max(n - 1, 0))] if n else 0, 0)      # [N, 10]
    pcol = nt + 3 * opt[:, None] + np.arange(3)[None, :]                                                           # [N, 3]
    idx = np.concatenate([ccol, pcol], 1)                                                                          # [N, 13]
    H, g = np.zeros((m, m), real), np.zeros(m, real)
    for i in range(2):
        Ji = np.concatenate([np.where(on, rows[:, 10 * i:10 * i + 10], 0), rows[:, 20 + 3 * i:23 + 3 * i]], 1)      # [N, 13]
        # a tied column may appear once per row only (one camera per observation), so J' row entries are just relabelled
        np.add.at(H, (idx[:, :, None], idx[:, None, :]), Ji[:, :, None] * Ji[:, None, :])
        np.add.at(g, idx, Ji * rows[:, 26 + i][:, None])
    used = np.zeros(m, bool)
    used[:nt] = True
    used[nt:] = np.repeat(np.bincount(opt, minlength=npts) > 0, 3)
    d = np.diagonal(H).copy()
    s = 1 / (1 + np.sqrt(d)) if jacobi else np.ones(m, real)
    D = np.minimum(np.maximum(d * s * s, real(lo)), real(hi))
    A = H * s[:, None] * s[None, :]
    A[np.arange(m), np.arange(m)] += D / real(radius)
    u = np.flatnonzero(used)
    y = np.zeros(m, real)
    y[u] = B.solve_spd(A[np.ix_(u, u)], (g * s)[u], real)
    delta = -y * s
    dP, dI = np.zeros((nc, 6), real), np.zeros((nc, 6), real)
    for c in range(nc):
        for k in range(dim[c]):
            col, v = cols[c, k], delta[cmap[off[c] + k]]
            if col < 6:
                dP[c, col] = v
            else:
                dI[c, col - 6] = v
    if mode == 1:      # Plus clamps the candidate's focal lengths
        new = np.asarray(intr, real) + dI
        new[:, :2] = np.where(dI[:, :2] != 0, np.minimum(new[:, :2], real(ub)), new[:, :2])
        dI = new - np.asarray(intr, real)
    return dict(dP=dP, dI=dI, dX=delta[nt:].reshape(-1, 3), n_tied=nt, intr0=intr)


# ---------------------------------------------------------------------------------------------------------------- the GPU suite's cases
def perturbed(sc, seed, groups, f=4.0):
    """The scenes of ba_graphs start off the minimum in poses and points and AT the true intrinsics: move the focal lengths too, the
    members of a group alike."""
    rng = np.random.default_rng(seed)
    out = ba_graphs.copy_scene(sc)
    I = np.array(sc["intrinsics"], np.float64)
    I[:, :2] += f * rng.standard_normal((len(I), 2))
    g = np.asarray(groups)
    for gid in np.unique(g[g >= 0]):
        m = np.flatnonzero(g == gid)
        I[m] = I[m[0]]
    out["intrinsics"] = I
    return out


def _grp(nc, *sets):
    g = np.full(nc, -1, np.int32)
    for k, s in enumerate(sets):
        g[list(s)] = k
    return g


# name -> dict(nc, npts, seed, groups, constant, fix, loss, ub, intr): the shapes of the issue, each the smallest that can hit its target
CASES = {
    "one_group_12": dict(nc=12, npts=160, seed=21, groups=_grp(12, range(12))),                                   # n' = 67: one block
    "mixed_12": dict(nc=12, npts=160, seed=22, groups=_grp(12, range(0, 12, 2), (1, 3))),                         # cameras 0 and 1 tied to others; own and shared columns
    "one_group_20": dict(nc=20, npts=220, seed=23, groups=_grp(20, range(20))),                                   # n = 191: two blocks, n' = 115: one
    "exactly_128": dict(nc=22, npts=240, seed=24, groups=_grp(22, range(2, 12), range(12, 22)), constant=(0, 1), fix=(0, 0)),      # npad = n': no right-hand-side row
    "n_138": dict(nc=23, npts=250, seed=25, groups=_grp(23, range(2, 12), range(12, 22)), constant=(0, 1), fix=(0, 0)),
    "two_groups_66": dict(nc=66, npts=330, seed=26, groups=_grp(66, range(0, 66, 2), range(1, 66, 2))),           # n' = 395: four blocks
    "held_12": dict(nc=12, npts=160, seed=27, groups=_grp(12, range(12)), constant=(4,)),                         # a constant member: intrinsics held
    "distorted_12": dict(nc=12, npts=160, seed=28, groups=_grp(12, range(1, 12))),                                # (every scene of ba_graphs has k1 = -0.08, k2 = 0.02, fy = 1.07 fx; here camera 0 keeps its own)
    "cauchy_12": dict(nc=12, npts=160, seed=29, groups=_grp(12, range(12)), loss=("cauchy", 2.0)),
    "bound_12": dict(nc=12, npts=160, seed=30, groups=_grp(12, range(12)), ub=700.0, start_f=720.0),              # starts above the bound: projected once per tied fx, fy
}


@functools.lru_cache(maxsize=None)
def _case_scene(name):
    c = CASES[name]
    nc = c["nc"]
    sc = ba_graphs.graph_scene(nc, c["npts"], c["seed"], lengths=[2, 3, 4, nc])
    sc = perturbed(sc, c["seed"], c["groups"])
    if "start_f" in c:
        sc["intrinsics"][:, :2] = c["start_f"]
    for v in sc.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc


def case(name):
    """(scene, keyword arguments of judge / tied_step: groups, constant, fix, and loss / ub where set)"""
    c = CASES[name]
    const = np.zeros(c["nc"], bool)
    const[list(c.get("constant", ()))] = True
    return dict(_case_scene(name)), dict(groups=c["groups"], constant=const, fix=c.get("fix", (1, 1)))


def judged(name, method="trf"):
    c = CASES[name]
    sc, kw = case(name)
    return judge(sc, method=method, loss=c.get("loss"), ub=c.get("ub", 1000.0), **kw)


def stepped(name, real=LD):
    c = CASES[name]
    sc, kw = case(name)
    return tied_step(sc, ub=c.get("ub", 1000.0), loss=c.get("loss"), real=real, **kw)


@functools.lru_cache(maxsize=None)
def recorded(name):
    """dict of the judge's record for a case (tests/golden/ba_tied_judge.npz): P, I, X, rms, spread (rms, poses, intrinsics, points: trf
    against dogbox), and the first step: dP, dI, dX (long double rounded to float64), eP, eI, eX = |float64 run - long double run|"""
    with np.load(GOLDEN) as z:
        return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + ".")}
