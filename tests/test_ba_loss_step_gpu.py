"""ONE Levenberg-Marquardt step of the bundle adjustment under a robust loss, on the GPU, through tools/ba_step_check (which takes the
loss in two further optional columns of cases.txt): what the two kernels that know the loss produce -- the corrected observation rows
and the robust cost (k_ba_eval<JAC, true>), the line search's value and directional derivative (k_ba_dirgrad<true>), the report's
weights (k_ba_loss_report) -- against tests/ba_loss_ref.py in long double, and the stages behind the rows from the GPU's OWN rows
with the unchanged functions of tests/ba_ref.py (they do not know that a loss exists).

Scenes: tests/ba_graphs.py's graph scenes cut to 63, 64, 65, 127, 128, 129 and 257 observations -- the wave and workgroup tails of both
evaluation kernels (128 and 256 threads) -- at 6 cameras in mode 0 (camera dimensions 0, 3, 6) and 12 cameras in mode 1 (4, 7, 10), every
eighth observation displaced by 20 to 120 px per axis, scale 4 px: every wave of eight rows or more holds observations on both sides of
the scale, and the two one-row tails (the cuts at 65 and 129) lie on different sides (asserted).

The two rules of tests/test_ba_step_gpu.py, nothing fitted:
  function-type  err_gpu <= 16 max(err_f64, u |ref|) per row for the corrected J and r and per observation for the weights; |ref| is the
                 floor of ba_loss_ref.row_floors / weight_floors (the residual is a prediction minus an exact observation).
  sum-type       the robust cost within gamma_m times the sum plus, per observation, the allowance of its term: rho' <= 1 and
                 rho'' <= 0 make rho / 2 Lipschitz in s / 2, so a residual within e of the reference's moves it by at most |r| e + e^2 / 2 --
                 the allowance the plain candidate cost gets there."""
import os
import subprocess
import time

import numpy as np
import pytest

import ba_graphs
import ba_loss_ref as R
import ba_ref as B
import test_ba_step_gpu as T
from reconstructor_amd import synth_ba

pytestmark = pytest.mark.gpu
LD, U = B.LD, B.U
COUNTS = (63, 64, 65, 127, 128, 129, 257)
SCALE = 4.0
LOSSES = [(R.HUBER, SCALE), (R.SOFT_L1, SCALE), (R.CAUCHY, SCALE)]


def case(name, scene, loss, **kw):
    c = T.case(name, scene, **kw)
    c["loss"] = loss
    return c


def run_tool(tmp_path, scenes, cases, timeout=170):
    assert os.path.exists(T.EXE), "tools/ba_step_check missing: run __graft_entry__.build()"
    d = str(tmp_path)
    for name, sc in scenes.items():
        assert (np.diff(sc["obs_pt"]) >= 0).all()
        B.write_scene(d, name, sc)
    R.write_cases(d, cases)
    t0 = time.time()
    r = subprocess.run([T.EXE, d], capture_output=True, text=True, timeout=timeout)
    print("%d cases in %.2f s" % (len(cases), time.time() - t0))
    assert r.returncode == 0, "ba_step_check exit code %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-2000:]
    return {c["name"]: R.read_capture(d, c["name"]) for c in cases}


def term_allowance(r, r64, uv):
    e = 16 * np.maximum(np.abs(r64 - r), LD(U) * np.abs(r + uv))
    return (np.abs(r) * e).sum() + (e * e).sum() / 2


def judge(sc, c, cap, point=None, both_sides=True):
    """the captured iteration of a case with a loss; `point`: where it linearises (the start when None)"""
    rep = T.Report(c["name"])
    loss = c["loss"]
    nc, npts, N = len(sc["poses"]), len(sc["points"]), len(sc["obs_cam"])
    ocam, opt = np.asarray(sc["obs_cam"], np.int64), np.asarray(sc["obs_pt"], np.int64)
    uv = np.asarray(sc["obs_uv"], np.float64)
    pt_off = np.concatenate([[0], np.cumsum(np.bincount(opt, minlength=npts))]).astype(np.int64)
    poses, intr, pts = T.start_point(sc, c) if point is None else point
    assert cap["got_a"] == 1 and cap["got_b"] == 1, (c["name"], cap["got_a"], cap["got_b"], cap["iterations"])
    cols, dim, off = B.structure(nc, c["mode"], c["fix0"], c["fix1"])
    # ---- the corrected rows, the robust cost, the weights
    rows = cap["J"].reshape(N, B.JROW)
    ref, plain, s = R.corrected_rows(poses, intr, pts, uv, ocam, opt, cols, dim, loss, LD)
    f64, plain64, _ = R.corrected_rows(poses, intr, pts, uv, ocam, opt, cols, dim, loss, np.float64)
    b = LD(np.float64(loss[1]) ** 2)
    assert (np.abs(s - b) > LD(1e-9) * b).all()
    if both_sides:
        for w0 in range(0, N, 64):
            if N - w0 >= 8:       # (a tail of one row has one side; planted() puts the two one-row tails on different sides)
                assert (s[w0:w0 + 64] > b).any() and (s[w0:w0 + 64] <= b).any(), "wave %d has one side of the scale only" % (w0 // 64)
        assert N <= 64 or s[64] <= b
        assert N <= 128 or s[128] > b
    fl = R.row_floors(loss, plain, uv)
    rep.add("J", T.fn_ratio(rows[:, :26], ref[:, :26], f64[:, :26], axis=1, floor=fl[:, :26]))
    rep.add("r", T.fn_ratio(rows[:, 26:], ref[:, 26:], f64[:, 26:], axis=1, floor=fl[:, 26:]))
    rc = R.robust_cost(plain[:, 26:], loss)
    rep.add("cost", float(abs(LD(cap["scal"][0]) - rc[0]) / (B.gamma(rc[2]) * rc[1] + term_allowance(plain[:, 26:], plain64[:, 26:], uv))))
    if c["iteration"] == 1 or point is not None:
        fd, _ = R.weight_floors(loss, plain[:, 26:], uv)
        rep.add("weights", T.fn_ratio(cap["weights"], R.drho(loss, s), R.drho(loss, R.sq(plain64[:, 26:], np.float64), np.float64), floor=fd))
        lr = cap["loss_report"]
        rep.exact("report counts", lr["n_obs"] == N and lr["n_beyond_scale"] == int((s > b).sum()))
    # ---- the stages behind the rows, from the GPU's rows, by functions that know no loss
    nb = B.normal_blocks(rows, ocam, opt, nc, npts)
    for k in ("Uraw", "gcraw", "Vraw", "gpraw"):
        rep.add(k, T.sum_ratio(cap[k], nb[k]))
    Wg, Yg = cap["WY"][:B.WROW * N].reshape(N, 3, 10), cap["WY"][B.WROW * N:].reshape(N, 3, 10)
    rep.add("W", T.sum_ratio(Wg, B.w_plane(rows, cap["sc"], cap["sp"], ocam, opt, dim, off)))
    rep.add("Y", T.sum_ratio(Yg, B.y_plane(Wg, cap["Vinv"], opt)))
    rep.add("model", T.sum_ratio(cap["scal"][2], B.model_change(rows, cap["sc"], cap["stc"], cap["sp"], cap["stp"], ocam, opt, dim, off)))
    used_c, used_p = np.bincount(ocam, minlength=nc) > 0, np.diff(pt_off) > 0
    d1c, d1p = cap["stc"].astype(LD) * cap["sc"], cap["stp"].astype(LD) * cap["sp"]
    tail = (cols, dim, off, c["mode"], c["ub"], cap["gcraw"], cap["gpraw"], used_c, used_p, c["fix0"], LD)
    g1 = B.plus(poses, intr, pts, d1c, d1p, *tail)["gd"]
    rep.add("g.delta", T.sum_ratio(cap["scal"][8], (g1[0], g1[1], g1[2] + 2)))
    rep.exact("gradient max", cap["scal"][12] == B.projected_gradient_max(cap["gcraw"], cap["gpraw"], intr, cols, dim, c["mode"], c["ub"]))
    # ---- the candidate's robust cost at the GPU's candidate
    P2, I2, X2 = cap["poses2"].reshape(nc, 6), cap["intr2"].reshape(nc, 6), cap["pts2"].reshape(npts, 3)
    r2 = B.residual(P2.astype(LD)[ocam], I2.astype(LD)[ocam], X2.astype(LD)[opt], uv.astype(LD))
    r264 = B.residual(P2[ocam], I2[ocam], X2[opt], uv)
    cc = R.robust_cost(r2, loss)
    rep.add("candidate cost", float(abs(LD(cap["scal"][1]) - cc[0]) / (B.gamma(cc[2]) * cc[1] + term_allowance(r2, r264, uv))))
    # ---- the line search's trials: robust value, rho' r . (J d)
    tri = cap["trials"].reshape(-1, 4)
    for t, (al, cost_t, dg, dmax) in enumerate(tri):
        if np.isnan(dg):
            continue
        la = LD(al)
        tp = B.plus(poses, intr, pts, la * d1c, la * d1p, *tail)
        tP, tI, tX = (np.asarray(tp[k], np.float64) for k in ("poses2", "intr2", "pts2"))      # the kernel differentiates at ITS candidate
        rr = B.residual(tP.astype(LD)[ocam], tI.astype(LD)[ocam], tX.astype(LD)[opt], uv.astype(LD))
        rr64 = B.residual(tP[ocam], tI[ocam], tX[opt], uv)
        ct = R.robust_cost(rr, loss)
        rep.add("trial %d cost" % t, float(abs(LD(cost_t) - ct[0]) / (B.gamma(ct[2]) * ct[1] + term_allowance(rr, rr64, uv))))
        v, A, m = R.directional_derivative(tP, tI, tX, uv, ocam, opt, cols, dim, off, la * d1c, la * d1p, loss)
        v64, _, _ = R.directional_derivative(tP, tI, tX, uv, ocam, opt, cols, dim, off, np.asarray(la * d1c, np.float64), np.asarray(la * d1p, np.float64), loss, np.float64)
        rep.add("trial %d derivative" % t, float(abs(LD(dg) * la - v) / (B.gamma(m) * A + 16 * max(abs(LD(v64) - v), LD(U) * A))))
    rep.done()
    return P2, I2, X2


def planted(nc, seed):
    sc = ba_graphs.graph_scene(nc, 120, seed, (2, 3, 4, 5), repeat=0.1)
    assert len(sc["obs_cam"]) >= max(COUNTS)
    rng = np.random.default_rng(seed)
    sc = ba_graphs.copy_scene(sc)
    idx = np.concatenate([np.arange(3, len(sc["obs_cam"]), 8), [128]])
    sc["obs_uv"][idx] += np.rint(rng.uniform(20, 120, (len(idx), 2))) * rng.choice([-1.0, 1.0], (len(idx), 2))
    # observations 64 and 128 are the one-row wave tails of the cuts at 65 and 129: 128 is displaced, 64 is moved onto the start's own
    # prediction (rounded to the pixel: |r| <= 0.71 px, inside the scale)
    o = 64
    r = B.residual(sc["poses"][sc["obs_cam"][o]], sc["intrinsics"][sc["obs_cam"][o]], sc["points"][sc["obs_pt"][o]], sc["obs_uv"][o])
    sc["obs_uv"][o] = np.rint(sc["obs_uv"][o] + r)
    return sc


@pytest.mark.parametrize("nc,mode,seed", [(6, 0, 301), (12, 1, 302)])
def test_rows_cost_and_weights_at_the_wave_and_workgroup_tails(tmp_path, nc, mode, seed):
    full = planted(nc, seed)
    assert set(B.structure(nc, mode, 1, 1)[1]) == ({0, 3, 6} if mode == 0 else {4, 7, 10})
    scenes, cases = {}, []
    for i, no in enumerate(COUNTS):
        keep = np.zeros(len(full["obs_cam"]), bool)
        keep[:no] = True
        scenes["n%d" % no] = ba_graphs.select(full, keep)
        # every count under one loss in turn, the largest under all three
        for loss in (LOSSES if no == COUNTS[-1] else [LOSSES[i % 3]]):
            cases.append(case("n%d_%s" % (no, R.NAMES[loss[0]]), "n%d" % no, loss, mode=mode, jacobi=i % 2))
    for sc in scenes.values():
        assert len(set(sc["obs_cam"])) == nc, "a camera kind is missing from the cut"
    caps = run_tool(tmp_path, scenes, cases)
    for c in cases:
        judge(scenes[c["scene"]], c, caps[c["name"]])


def test_line_search_trials_under_a_loss(tmp_path):
    """tests/test_ba_step_gpu.py's far-off start with bounds, 8 % of its observations displaced, under Huber: the first run logs every
    iteration's scalars, the second captures the first iteration that backtracks: every trial's robust cost and directional derivative"""
    base = synth_ba.make_scene(12, 200, obs_per_point=6, seed=1, perturb=(0.4, 2.0, 1.5))
    sc, _ = R.plant_outliers(base, 96, 1)
    loss = (R.HUBER, SCALE)
    cap0 = run_tool(tmp_path, {"far": sc}, [case("log", "far", loss, iteration=12, mode=1)])["log"]
    log = cap0["log"].reshape(-1, 15)
    assert (log[:, 14] > 0).any(), "no iteration backtracks"
    k = int(np.flatnonzero(log[:, 14] > 0)[0]) + 1
    j = T.last_accepted(log, k)
    print("first backtracking iteration: %d (%d backtracks), behind the accepted iteration %d" % (k, log[k - 1, 14], j))
    cases = ([case("at%d" % j, "s", loss, iteration=j, mode=1)] if j else []) + [case("at%d" % k, "s", loss, iteration=k, mode=1)]
    sub = tmp_path / "second"
    sub.mkdir()
    caps = run_tool(sub, {"s": sc}, cases)
    point = None
    if j:
        cj = caps["at%d" % j]
        assert cj["got_b"] == 1
        point = (cj["poses2"].reshape(12, 6), cj["intr2"].reshape(12, 6), cj["pts2"].reshape(-1, 3))
    cap = caps["at%d" % k]
    tri = cap["trials"].reshape(-1, 4)
    assert len(tri) >= log[k - 1, 14] + 1 and not np.isnan(tri[0, 2])
    judge(sc, cases[-1], cap, point=point, both_sides=False)
