"""The robust losses of the bundle adjustment (csrc/ba_loss.h) restated in numpy on top of tests/ba_ref.py, generic
over the dtype like it: the judge of tests/test_ba_loss_step_gpu.py, tests/test_ba_loss_gpu.py and tests/test_ba_loss_session_gpu.py,
itself checked on the CPU by tests/test_ba_loss_ref.py.  `real` is np.longdouble (the reference) or np.float64 (the baseline whose own
error sets the function-type tolerances).

  rho, drho, weight          the three losses and the trivial one; a loss is (kind, scale) with kind 0 .. 3 or None
  corrected_rows             ba_ref.obs_rows times sqrt(rho'(s)) per observation: what k_ba_eval<true, true> writes
  robust_cost                1/2 sum rho(s) as (value, A, m) from residuals
  directional_derivative     sum_o rho'(s_o) r_o . (J_o d) as (value, A, m)
  report                     rcn_ba_loss_report and the weights
  lm_solve                   a whole Levenberg-Marquardt solve at intrinsics_mode 0 composed of ba_ref's stages, step for step what
                             rcn_int_ba_solve does: the Jacobi scale fixed at the start, the gradient test at every new point, invalid,
                             rejected and accepted steps, the radius update, the three tolerances.  No line search: mode 0 has no bounds.
b is the device's: the float64 product scale * scale, carried into `real`."""
import numpy as np

import ba_ref as B

LD = B.LD
DBL_MIN = float(np.finfo(np.float64).tiny)
TRIVIAL, HUBER, SOFT_L1, CAUCHY = 0, 1, 2, 3
NAMES = {TRIVIAL: "trivial", HUBER: "huber", SOFT_L1: "soft_l1", CAUCHY: "cauchy"}


def _ab(loss, real):
    kind, a = (TRIVIAL, 1.0) if loss is None else loss
    a = np.float64(a)
    return int(kind), real(a), real(a * a)


def rho(loss, s, real=LD):
    kind, a, b = _ab(loss, real)
    s = np.asarray(s, real)
    with np.errstate(all="ignore"):
        if kind == HUBER:
            return np.where(s <= b, s, 2 * a * np.sqrt(s) - b)
        if kind == SOFT_L1:
            return 2 * s / (np.sqrt(1 + s / b) + 1)          # = 2 b (sqrt(1 + s/b) - 1) without its cancellation
        if kind == CAUCHY:
            return b * np.log1p(s / b)
    return s.copy()


def drho(loss, s, real=LD):
    kind, a, b = _ab(loss, real)
    s = np.asarray(s, real)
    with np.errstate(all="ignore"):
        if kind == HUBER:
            return np.where(s <= b, real(1), np.maximum(real(DBL_MIN), a / np.sqrt(np.where(s <= b, 1, s))))
        if kind == SOFT_L1:
            return np.maximum(real(DBL_MIN), 1 / np.sqrt(1 + s / b))
        if kind == CAUCHY:
            return np.maximum(real(DBL_MIN), 1 / (1 + s / b))
    return np.ones_like(s)


def weight(loss, s, real=LD):
    return np.sqrt(drho(loss, s, real))


def sq(r, real=LD):
    r = np.asarray(r, real)
    return r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]


def corrected_rows(poses, intr, pts, uv, ocam, opt, cols, dim, loss, real=LD):
    """(corrected rows [N, 28], plain rows, s [N]): Jacobian and residual of every observation times sqrt(rho'(s))"""
    rows = B.obs_rows(poses, intr, pts, uv, ocam, opt, cols, dim, real)
    s = sq(rows[:, 26:], real)
    return rows * weight(loss, s, real)[:, None], rows, s


def robust_cost(r, loss, real=LD):
    """1/2 sum_o rho(s_o) from residuals [N, 2]: (value, A, m) -- rho >= 0, so A is the value; per term two products, an addition and
    rho's own operations (at most 6), then the sum and the halving"""
    v = rho(loss, sq(r, real), real).sum() / 2
    return v, v, len(np.asarray(r).reshape(-1, 2)) + 10


def directional_derivative(poses, intr, pts, uv, ocam, opt, cols, dim, off, dlc, dlp, loss, real=LD):
    """sum_o rho'(s_o) r_o' (Jc_o dlc + Jp_o dlp) at a trial point: (value, A, 2 N + 20)"""
    rows = B.obs_rows(poses, intr, pts, uv, ocam, opt, cols, dim, real)
    k = np.arange(10)
    on = k[None, :] < dim[ocam][:, None]
    v = np.asarray(dlc, real)
    vc = np.where(on, v[np.minimum(off[ocam][:, None] + k[None, :], max(len(v) - 1, 0))] if len(v) else 0, 0)
    vp = np.asarray(dlp, real).reshape(-1, 3)[opt]
    acc = np.zeros(len(rows), real)
    acca = np.zeros(len(rows), real)
    for i in range(2):
        m = (rows[:, 10 * i:10 * i + 10] * vc).sum(1) + (rows[:, 20 + 3 * i:23 + 3 * i] * vp).sum(1)
        ma = (np.abs(rows[:, 10 * i:10 * i + 10]) * np.abs(vc)).sum(1) + (np.abs(rows[:, 20 + 3 * i:23 + 3 * i]) * np.abs(vp)).sum(1)
        acc, acca = acc + rows[:, 26 + i] * m, acca + np.abs(rows[:, 26 + i]) * ma
    d = drho(loss, sq(rows[:, 26:], real), real)
    return (d * acc).sum(), (d * acca).sum(), 2 * len(rows) + 20


def report(poses, intr, pts, uv, ocam, opt, loss, real=LD):
    """dict(n_obs, n_beyond_scale, plain_rms_px, max_residual_px, weights, s): rcn_ba_loss_report at a point.  Without a loss nothing
    lies beyond the scale."""
    r = B.residual(np.asarray(poses, real)[ocam], np.asarray(intr, real)[ocam], np.asarray(pts, real)[opt], np.asarray(uv, real))
    s = sq(r, real)
    _, _, b = _ab(loss, real)
    trivial = loss is None or loss[0] == TRIVIAL
    n = len(s)
    return dict(n_obs=n, n_beyond_scale=0 if trivial else int((s > b).sum()), plain_rms_px=np.sqrt(s.sum() / max(n, 1)),
                max_residual_px=np.sqrt(s.max()) if n else real(0), weights=drho(loss, s, real), s=s, r=r)


def weight_floors(loss, r, uv):
    """The |ref| of the function-type rule for rho'(s) and for sqrt(rho'(s)), per observation.  The residual is a prediction minus an
    exact observation, so ITS floor is the prediction's size p = |r + uv| (tests/test_ba_step_gpu.py); rho' and the row weight are functions
    of that residual, and a relative change u of the prediction moves them by u |d/dr| p.  So the floors are the values' own sizes plus
    that first-order term: |rho'| + |rho''| 2 (|r0| p0 + |r1| p1), and the same through the square root.  |rho''| in closed form:
    Huber a / (2 s^1.5) beyond b, soft-L1 (1 + s/b)^-1.5 / (2 b), Cauchy (1 + s/b)^-2 / b."""
    r, uv = np.asarray(r, LD), np.asarray(uv, LD)
    s = sq(r)
    p = np.abs(r + uv)
    kind, a, b = _ab(loss, LD)
    with np.errstate(all="ignore"):
        d2 = {TRIVIAL: 0 * s, HUBER: np.where(s <= b, 0, a / (2 * np.where(s <= b, 1, s) ** LD(1.5))), SOFT_L1: (1 + s / b) ** LD(-1.5) / (2 * b),
              CAUCHY: (1 + s / b) ** LD(-2) / b}[kind]
    spread = d2 * 2 * (np.abs(r[:, 0]) * p[:, 0] + np.abs(r[:, 1]) * p[:, 1])
    d = drho(loss, s)
    return d + spread, np.sqrt(d) + spread / (2 * np.sqrt(d))


def row_floors(loss, plain_rows, uv):
    """The floors of the corrected rows [N, 28] for the function-type rule: a corrected entry is w x, so a relative change u of the
    prediction moves it by u (|x|-floor w + |x| |dw|): the plain entry's own floor (|J|, and the prediction for the residual) times w, plus
    the plain entry times the weight's first-order term (weight_floors)."""
    rows = np.asarray(plain_rows, LD)
    r = rows[:, 26:]
    w = weight(loss, sq(r))
    _, fw = weight_floors(loss, r, uv)
    own = np.abs(rows).copy()
    own[:, 26:] = np.abs(r + np.asarray(uv, LD))
    return own * w[:, None] + np.abs(rows) * (fw - w)[:, None]


# ---------------------------------------------------------------------------------------------------------------------
def default_opts(nc, **over):
    """rcn_ba_default_options with intrinsics_mode 0 whatever the camera count"""
    o = dict(max_iterations=150 if nc < 10 else 50, fix0=1, fix1=1, jacobi=1, radius=1e4, max_radius=1e16, min_radius=1e-32,
             min_relative_decrease=1e-3, lo=1e-6, hi=1e32, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
             max_consecutive_invalid_steps=5)
    o.update(over)
    return o


FUNCTION, GRADIENT, PARAMETER, RADIUS, NO_CONVERGENCE, FAILURE = 1, 2, 3, 4, 5, 6


def lm_solve(scene, opts, loss, real=LD):
    """The solve of rcn_int_ba_solve at intrinsics_mode 0 in `real`.  Returns (poses, intrinsics, points, summary dict: iterations,
    termination, successful_steps, unsuccessful_steps, invalid_steps, cost_trace, initial_cost, final_cost, final_rms_px)."""
    nc, npts = len(scene["poses"]), len(scene["points"])
    ocam, opt = np.asarray(scene["obs_cam"], np.int64), np.asarray(scene["obs_pt"], np.int64)
    uv = np.asarray(scene["obs_uv"], np.float64)
    N = len(ocam)
    pt_off = np.concatenate([[0], np.cumsum(np.bincount(opt, minlength=npts))]).astype(np.int64)
    cols, dim, off = B.structure(nc, 0, opts["fix0"], opts["fix1"])
    n = int(off[-1])
    used_c, used_p = np.bincount(ocam, minlength=nc) > 0, np.diff(pt_off) > 0
    pk_off, pk_list, pk_keys = B.pair_lists(ocam, pt_off, dim, nc)
    P, I, X = np.array(scene["poses"], real), np.array(scene["intrinsics"], real), np.array(scene["points"], real).reshape(-1, 3)

    def linearise(P, I, X):
        rows, _, s = corrected_rows(P, I, X, uv, ocam, opt, cols, dim, loss, real)
        nb = B.normal_blocks(rows, ocam, opt, nc, npts, real)
        return rows, rho(loss, s, real).sum() / 2, {k: nb[k][0] for k in ("Uraw", "gcraw", "Vraw", "gpraw")}

    def cost_at(P, I, X):
        r = B.residual(P[ocam], I[ocam], X[opt], uv.astype(real))
        return rho(loss, sq(r, real), real).sum() / 2

    rows, cost, nb = linearise(P, I, X)
    du, dv = B.reduced_diag(nb["Uraw"], dim, off), np.diagonal(nb["Vraw"], axis1=1, axis2=2).reshape(-1)
    scl, spl = B.jacobi_scale(du, opts["jacobi"], real), B.jacobi_scale(dv, opts["jacobi"], real)      # fixed at the start
    out = dict(initial_cost=cost, successful_steps=0, unsuccessful_steps=0, invalid_steps=0)
    trace = {0: cost}
    radius, decrease = float(opts["radius"]), 2.0
    need_gradient, invalid_run, it, termination = True, 0, 0, 0
    dgc = dgp = None
    while True:
        if need_gradient:
            # mode 0: no bounds, the projected gradient is the gradient (J'r of the unscaled rows, free coordinates only)
            g = [np.abs(np.asarray(nb["gcraw"], real).reshape(-1, 10)[c, :dim[c]]).max() for c in range(nc) if dim[c]]
            gmax = max(g + [np.abs(nb["gpraw"]).max() if npts else 0])
            du, dv = B.reduced_diag(nb["Uraw"], dim, off), np.diagonal(nb["Vraw"], axis1=1, axis2=2).reshape(-1)
            dgc, dgp = B.lm_diagonal(du, scl, opts["lo"], opts["hi"], real), B.lm_diagonal(dv, spl, opts["lo"], opts["hi"], real)
            need_gradient = False
            if gmax <= opts["gradient_tolerance"]:
                termination = GRADIENT
                break
        if it >= opts["max_iterations"] or radius <= opts["min_radius"]:
            termination = NO_CONVERGENCE if it >= opts["max_iterations"] else RADIUS
            break
        it += 1
        ir = real(1) / real(radius)
        ok = True
        try:
            Vinv, det, (gps, _, _) = B.point_solve(nb["Vraw"], spl, dgp, nb["gpraw"], ir, real)
            W, _, _ = B.w_plane(rows, scl, spl, ocam, opt, dim, off, real)
            Y, _, _ = B.y_plane(W, Vinv, opt, real)
            (S, _, _), (rhs, _, _) = B.reduced_system(W, Y, gps, nb["Uraw"], nb["gcraw"], scl, dgc, ir, ocam, opt, dim, off, pk_keys, pk_list, nc, real)
            y = B.solve_spd(np.tril(S) + np.tril(S, -1).T, rhs, real)
            (_, _, _), (stp, _, _) = B.backsub(W, y, gps, Vinv, ocam, opt, pt_off, dim, off, None, real)
            stc, stp = -y, stp.reshape(-1)
            model = B.model_change(rows, scl, stc, spl, stp, ocam, opt, dim, off, real)[0]
            pl = B.plus(P, I, X, stc * scl, stp * spl, cols, dim, off, 0, 0.0, nb["gcraw"], nb["gpraw"], used_c, used_p, opts["fix0"], real)
            finite = all(np.isfinite(np.asarray(pl[k], np.float64)).all() for k in ("poses2", "intr2", "pts2"))
            ok = bool(finite and np.isfinite(np.float64(model)))
        except np.linalg.LinAlgError:
            ok = False
        if not ok or not model > 0:
            out["invalid_steps"] += 1
            invalid_run += 1
            if invalid_run >= opts["max_consecutive_invalid_steps"]:
                termination = FAILURE
                break
            radius /= decrease
            decrease *= 2.0
            trace[it] = cost
            continue
        invalid_run = 0
        cand = cost_at(pl["poses2"], pl["intr2"], pl["pts2"])
        if not np.isfinite(np.float64(cand)):
            cand = real(np.finfo(np.float64).max)
        if np.sqrt(pl["dx2"][0]) <= opts["parameter_tolerance"] * (np.sqrt(pl["x2"][0]) + opts["parameter_tolerance"]):
            termination, trace[it] = PARAMETER, cost
            break
        change = cost - cand
        if abs(change) <= opts["function_tolerance"] * cost:
            termination, trace[it] = FUNCTION, cost
            break
        q = float(change / model)
        if q > opts["min_relative_decrease"]:
            P, I, X = pl["poses2"], pl["intr2"], pl["pts2"]
            rows, cost, nb = linearise(P, I, X)
            need_gradient = True
            out["successful_steps"] += 1
            t = 2.0 * q - 1.0
            radius = min(opts["max_radius"], radius / max(1.0 / 3.0, 1.0 - t * t * t))
            decrease = 2.0
        else:
            out["unsuccessful_steps"] += 1
            radius /= decrease
            decrease *= 2.0
        trace[it] = cost
    out.update(iterations=it, termination=termination, final_cost=cost, final_rms_px=np.sqrt(2 * cost / max(N, 1)),
               initial_rms_px=np.sqrt(2 * out["initial_cost"] / max(N, 1)),
               cost_trace=np.array([trace[k] for k in range(min(160, it + 1))], real))
    return P, I, X, out


# ---------------------------------------------------------------------------------------------------------------------
# scenes and the tool's files
def plant_outliers(sc, count, seed, lo=20.0, hi=120.0):
    """a copy of the scene with `count` observations displaced by lo .. hi px per axis, either sign; the observations stay integers.
    Returns (scene, indices of the displaced observations)."""
    rng = np.random.default_rng(seed + 7919)
    out = dict(sc)
    uv = np.array(sc["obs_uv"], np.float64)
    idx = rng.choice(len(uv), size=count, replace=False)
    uv[idx] += np.rint(rng.uniform(lo, hi, (count, 2))) * rng.choice([-1.0, 1.0], (count, 2))
    out["obs_uv"] = uv
    return out, np.sort(idx)


def write_cases(d, cases):
    """ba_ref.write_cases with the tool's further optional columns: c["loss"] = (kind, scale) puts the diagonals (c.get("lm") or the
    defaults) and the loss behind the line"""
    import os
    with open(os.path.join(d, "cases.txt"), "w") as f:
        for c in cases:
            lm, loss = c.get("lm"), c.get("loss")
            tail = ""
            if lm is not None or loss is not None:
                tail += " %.17g %.17g" % tuple(lm if lm is not None else (1e-6, 1e32))
            if loss is not None:
                tail += " %d %.17g" % (int(loss[0]), float(loss[1]))
            f.write("%s %s %d %d %d %d %d %.17g %.17g%s\n" % (c["name"], c["scene"], c["iteration"], c["mode"], c["fix0"], c["fix1"], c["jacobi"], c["ub"], c["radius"], tail))


def read_capture(d, name):
    """ba_ref.read_capture plus what a case with a loss adds: cap["weights"] and cap["loss_report"]"""
    import os
    cap, rep = {}, {}
    with open(os.path.join(d, name + ".meta")) as f:
        for line in f:
            k, v = line.split()
            if k.startswith("loss_"):
                rep[k[5:]] = float(v) if k.endswith("_px") else int(v)
            else:
                cap[k] = float(v) if k == "radius" else int(v)
    for a in B.ARRAYS:
        cap[a] = np.fromfile(os.path.join(d, name + "." + a), dtype=B._TYPES.get(a, "<f8"))
    if rep:
        cap["loss_report"] = rep
        cap["weights"] = np.fromfile(os.path.join(d, name + ".weights"), dtype="<f8")
    return cap
