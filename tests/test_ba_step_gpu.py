"""ONE Levenberg-Marquardt step of the bundle adjustment (csrc/ba.hip) as a unit on the GPU: tools/ba_step_check (built by
__graft_entry__.build(); a driver only) runs the product's own rcn_int_ba_solve with the internal probe set and writes every array
the chosen iteration produced; tests/ba_ref.py restates each stage in long double FROM THE GPU'S OWN INPUTS TO THAT STAGE, so an error
is charged to the kernel that made it.  One tool run per test instance (two where a first run has to find the iteration).

Tolerances (none taken from the GPU, none fitted):
  integers       cols, cam_off, cam_dim, pk_off, pk_list, the padding rows' 0 / 1 / RCN_RHS_BETA, the sentinel pattern, flag and ticket
                 words: exactly.
  sum-type       |gpu - ref| <= gamma_m A componentwise, A the expression on absolute values, gamma_m = m u / (1 - m u), m the rounded
                 operations on the longest path (counted per stage in ba_ref.py's docstring): holds for any summation order and for
                 FMA contraction.
  function-type  err_gpu <= 16 max(err_f64, u |ref|), err_f64 the error of ba_ref's float64 run against its long-double run; per row
                 for J, per block for Vinv and the rotation tables.  The residual is a prediction minus an exact observation, so its
                 |ref| is the prediction's.
  solution       backward error against the CAPTURED system <= n u (chol_ref.bwd): the hand-off (row n, beta, sentinel, y out of the
                 factor), not a second test of the factorisation.
  delta          end to end from the problem's inputs: |d_gpu - d_ref| <= 16 max(|d_f64 - d_ref|, u |d_ref|), cameras and landmarks apart.
Every check prints its figure (largest observed part of its bound) before it asserts; pytest -s shows them.

The damped inverses (k_ba_point_solve, k_ba_gradmax's fused launch) are carried in double-double on the device: in plain FP64 a block's nine
entries share ONE amplified rounding (1 / det of a badly conditioned V), whose ratio to the float64 run's is heavy-tailed, and 3 to 5 blocks in a
thousand missed the per-block rule -- on the device and in a float64 restatement on the CPU alike."""
import os
import subprocess
import time

import numpy as np
import pytest

import ba_graphs
import ba_ref as B
import chol_ref
from oracle import orc_ba
from reconstructor_amd import synth_ba

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "ba_step_check")
LD, U = B.LD, B.U
LO, HI = 1e-6, 1e32          # min / max_lm_diagonal of rcn_ba_default_options


def case(name, scene, iteration=1, mode=0, fix0=1, fix1=1, jacobi=1, ub=1000.0, radius=1e4):
    return dict(name=name, scene=scene, iteration=iteration, mode=mode, fix0=fix0, fix1=fix1, jacobi=jacobi, ub=ub, radius=radius)


def run_tool(tmp_path, scenes, cases, timeout=170):
    assert os.path.exists(EXE), "tools/ba_step_check missing: run __graft_entry__.build()"
    d = str(tmp_path)
    for name, sc in scenes.items():
        assert len(sc["obs_cam"]) <= 13000 and (np.diff(sc["obs_pt"]) >= 0).all()
        B.write_scene(d, name, sc)
    B.write_cases(d, cases)
    t0 = time.time()
    r = subprocess.run([EXE, d], capture_output=True, text=True, timeout=timeout)
    print("%d cases in %.2f s" % (len(cases), time.time() - t0))
    print(r.stdout[-6000:])
    assert r.returncode == 0, "ba_step_check exit code %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-2000:]
    return {c["name"]: B.read_capture(d, c["name"]) for c in cases}


# ---------------------------------------------------------------------------------------------------------------------
# the bounds
class Report:
    def __init__(self, label):
        self.label, self.lines, self.bad = label, [], []

    def add(self, stage, ratio, limit=1.0):
        ratio = float(ratio)
        self.lines.append("%s %.3g" % (stage, ratio))
        if not ratio <= limit:
            self.bad.append("%s: %s is %.3g of its bound" % (self.label, stage, ratio))

    def exact(self, stage, ok):
        if not ok:
            self.bad.append("%s: %s differs" % (self.label, stage))

    def done(self):
        print("%-22s %s" % (self.label, "  ".join(self.lines)))
        assert not self.bad, "\n".join(self.bad)


def sum_ratio(gpu, ref):
    """largest |gpu - value| / (gamma_m A) over the entries; an entry whose bound is zero must be met exactly"""
    v, A, m = ref
    e = np.abs(np.asarray(gpu, LD).reshape(np.shape(v)) - v)
    bound = B.gamma(m) * A * np.ones(np.shape(v), LD)
    if np.ndim(e) == 0:
        e, bound = np.reshape(e, 1), np.reshape(bound, 1)
    if not np.isfinite(np.asarray(gpu, np.float64)).all():
        return np.inf
    z = bound == 0
    if (e[z] != 0).any():
        return np.inf
    return float((e[~z] / bound[~z]).max()) if (~z).any() else 0.0


def fn_ratio(gpu, ref, f64, axis=None, floor=None, over=None):
    """largest err_gpu / (16 max(err_f64, u |ref|)), errors and |ref| as maxima over `axis` (None: entry by entry)"""
    gpu, f64 = np.asarray(gpu, LD).reshape(ref.shape), np.asarray(f64, LD).reshape(ref.shape)
    if not np.isfinite(gpu.astype(np.float64)).all():
        return np.inf
    eg, ef, sc = np.abs(gpu - ref), np.abs(f64 - ref), np.abs(ref) if floor is None else np.asarray(floor, LD)
    if axis is not None:
        eg, ef, sc = eg.max(axis), ef.max(axis), sc.max(axis)
    bound = 16 * np.maximum(ef, LD(U) * sc)
    z = bound == 0
    if over is not None:
        over.append(int((eg[~z] > bound[~z]).sum() + (eg[z] != 0).sum()))
    if (eg[z] != 0).any():
        return np.inf
    return float((eg[~z] / bound[~z]).max()) if (~z).any() else 0.0


def start_point(sc, c):
    """the point the first iteration linearises at: the scene's, focal lengths projected onto the box in mode 1"""
    intr = np.array(sc["intrinsics"], np.float64)
    if c["mode"] == 1:
        intr[:, :2] = np.minimum(intr[:, :2], c["ub"])
    return np.array(sc["poses"], np.float64), intr, np.array(sc["points"], np.float64)


def judge(sc, c, cap, point=None, e2e=False, expect=None):
    """every stage of the captured iteration against ba_ref; `point`: (poses, intrinsics, points) the iteration linearises at (the
    start when None).  expect: what the capture must say was launched.  Returns the capture's candidate for a later iteration."""
    rep = Report(c["name"])
    nc, npts, N = len(sc["poses"]), len(sc["points"]), len(sc["obs_cam"])
    ocam, opt = np.asarray(sc["obs_cam"], np.int64), np.asarray(sc["obs_pt"], np.int64)
    uv = np.asarray(sc["obs_uv"], np.float64)
    pt_off = np.concatenate([[0], np.cumsum(np.bincount(opt, minlength=npts))]).astype(np.int64)
    kc = np.bincount(ocam, minlength=nc)
    poses, intr, pts = start_point(sc, c) if point is None else point
    assert cap["got_a"] == 1 and cap["got_b"] == 1, (c["name"], cap["got_a"], cap["got_b"], cap["iterations"])
    # ---- structure
    cols, dim, off = B.structure(nc, c["mode"], c["fix0"], c["fix1"])
    n, npad = int(off[-1]), B.padded(int(off[-1]))
    rep.exact("cols / cam_off / cam_dim", np.array_equal(cap["cols"].reshape(nc, 10), cols) and np.array_equal(cap["cam_dim"], dim) and np.array_equal(cap["cam_off"], off))
    rep.exact("n / npad", (cap["n"], cap["npad"]) == (n, npad))
    rep.exact("csplit", cap["csplit"] == B.cam_split(nc, int(kc.max())))
    rep.exact("diagonal kernel", cap["diag_smb"] == (4 if nc >= 128 else 12) and (nc < 128 or cap["csplit"] == 1))
    rep.exact("finish", cap["fin"] == (-1 if n == npad else 1) and cap["rhs_row"] == (n != npad))
    for k, v in (expect or {}).items():
        rep.exact("%s = %r (captured %r)" % (k, v, cap[k]), cap[k] == v)
    rep.exact("flag words", cap["flag"][0] == 0 and cap["flag"][1] == 0 and not cap["flag"][8:12].any() and not cap["flag_b"][8:12].any() and cap["flag_b"][0] == 0)
    rep.exact("ticket words", not cap["tickets"].any() and not cap["tickets_b"].any())
    # ---- residual and Jacobian at the GPU's point
    rows = cap["J"].reshape(N, B.JROW)
    ref = B.obs_rows(poses, intr, pts, uv, ocam, opt, cols, dim, LD)
    f64 = B.obs_rows(poses, intr, pts, uv, ocam, opt, cols, dim, np.float64)
    rep.add("J", fn_ratio(rows[:, :26], ref[:, :26], f64[:, :26], axis=1))
    rep.add("r", fn_ratio(rows[:, 26:], ref[:, 26:], f64[:, 26:], axis=1, floor=np.abs(ref[:, 26:] + uv)))
    rep.add("cost", sum_ratio(cap["scal"][0], B.cost_of(rows[:, 26:])))
    tr, t64 = B.cam_rot_table(poses, LD), B.cam_rot_table(poses, np.float64)
    tab = cap["crot"].reshape(nc, B.CROT)
    rep.add("crot", max(fn_ratio(tab[:, a:b], tr[:, a:b], t64[:, a:b], axis=1) for a, b in ((0, 9), (9, 18), (18, 23))))
    rep.exact("crot flag / w", np.array_equal(tab[:, 23:], tr[:, 23:].astype(np.float64)))
    # ---- normal blocks from the GPU's rows
    nb = B.normal_blocks(rows, ocam, opt, nc, npts)
    for k in ("Uraw", "gcraw", "Vraw", "gpraw"):
        rep.add(k, sum_ratio(cap[k], nb[k]))
    # ---- scales and the clamped diagonal from the GPU's blocks
    du, dv = B.reduced_diag(cap["Uraw"], dim, off), cap["Vraw"].reshape(-1, 9)[:, ::4].reshape(-1)
    if c["iteration"] == 1:          # (the Jacobi scale is fixed at the start: later iterations only use it)
        rep.add("sc", fn_ratio(cap["sc"], B.jacobi_scale(du, c["jacobi"]), B.jacobi_scale(du, c["jacobi"], np.float64)))
        rep.add("sp", fn_ratio(cap["sp"], B.jacobi_scale(dv, c["jacobi"]), B.jacobi_scale(dv, c["jacobi"], np.float64)))
    if not expect or not expect.get("reuse_diag"):
        rep.add("dgc", fn_ratio(cap["dgc"], B.lm_diagonal(du, cap["sc"], LO, HI), B.lm_diagonal(du, cap["sc"], LO, HI, np.float64)))
        rep.add("dgp", fn_ratio(cap["dgp"], B.lm_diagonal(dv, cap["sp"], LO, HI), B.lm_diagonal(dv, cap["sp"], LO, HI, np.float64)))
    ir = 1.0 / cap["radius"]
    Vi, det, gps = B.point_solve(cap["Vraw"], cap["sp"], cap["dgp"], cap["gpraw"], ir)
    Vi64, _, _ = B.point_solve(cap["Vraw"], cap["sp"], cap["dgp"], cap["gpraw"], ir, np.float64)
    assert (det > 0).all()
    over = []
    rv = fn_ratio(cap["Vinv"].reshape(-1, 9), Vi.reshape(-1, 9), Vi64.reshape(-1, 9), axis=1, over=over)
    rep.add("Vinv (%d of %d blocks over)" % (over[0], npts), rv)
    rep.add("gps", sum_ratio(cap["gps"], gps))
    # ---- W / Y planes
    Wg, Yg = cap["WY"][:B.WROW * N].reshape(N, 3, 10), cap["WY"][B.WROW * N:].reshape(N, 3, 10)
    rep.add("W", sum_ratio(Wg, B.w_plane(rows, cap["sc"], cap["sp"], ocam, opt, dim, off)))
    rep.add("Y", sum_ratio(Yg, B.y_plane(Wg, cap["Vinv"], opt)))
    # ---- pair lists
    pk_off, pk_list, pk_keys = B.pair_lists(ocam, pt_off, dim, nc)
    rep.exact("pk_off", np.array_equal(cap["pk_off"], pk_off))
    rep.exact("pk_list", np.array_equal(cap["pk_list"], pk_list))
    # ---- the reduced system from the GPU's planes and blocks, and the rows behind it
    (S, SA, SM), rhs = B.reduced_system(Wg, Yg, cap["gps"], cap["Uraw"], cap["gcraw"], cap["sc"], cap["dgc"], ir, ocam, opt, dim, off, pk_keys, pk_list, nc)
    Sg = cap["S"].reshape(npad, npad)
    low = np.tril(np.ones((n, n), bool))
    rep.add("S", sum_ratio(Sg[:n, :n][low], (S[low], SA[low], SM[low])))
    rhs_g = Sg[n, :n] if cap["fin"] >= 0 else cap["rhs"][:n]
    rep.add("rhs", sum_ratio(rhs_g, rhs))
    if n < npad:
        pad = np.zeros((npad - n, npad))
        pad[np.arange(npad - n), np.arange(n, npad)] = 1.0
        pad[0, n] = B.BETA
        pad[0, :n] = rhs_g
        rep.exact("padding rows", np.array_equal(Sg[n:], pad))
        rep.exact("sentinel", (cap["rhs"][:n].view(np.uint64) == np.uint64(B.SENTINEL)).all() and not cap["rhs"][n:].any())
    # ---- the solution against the captured system
    x = cap["x"][:n]
    Sf = np.tril(Sg[:n, :n]) + np.tril(Sg[:n, :n], -1).T
    if n:
        rep.add("solution (bwd / n u)", chol_ref.bwd(Sf, rhs_g, x) / (n * U) if np.isfinite(x).all() else np.inf)
    # ---- back-substitution
    tob, stp = B.backsub(Wg, x, cap["gps"], cap["Vinv"], ocam, opt, pt_off, dim, off, tobs_in=cap["tobs"])
    rep.add("tobs", sum_ratio(cap["tobs"], tob))
    rep.exact("stc", np.array_equal(cap["stc"], -x))
    rep.add("stp", sum_ratio(cap["stp"], stp))
    # ---- model change, Plus and its sums, costs
    rep.add("model", sum_ratio(cap["scal"][2], B.model_change(rows, cap["sc"], cap["stc"], cap["sp"], cap["stp"], ocam, opt, dim, off)))
    tri = cap["trials"].reshape(-1, 4)
    found = len(tri) and np.isnan(tri[-1, 2]) and tri[-1, 1] <= cap["scal"][0] + 1e-4 * cap["scal"][8] * tri[-1, 0]
    alpha = 1.0 if (len(tri) == 0 or not found) else float(tri[-1, 0])
    a = LD(alpha)
    rep.add("dlc", sum_ratio(cap["dlc"], (a * cap["stc"].astype(LD) * cap["sc"], np.abs(a * cap["stc"].astype(LD) * cap["sc"]), 2)))
    rep.add("dlp", sum_ratio(cap["dlp"], (a * cap["stp"].astype(LD) * cap["sp"], np.abs(a * cap["stp"].astype(LD) * cap["sp"]), 2)))
    used_c, used_p = kc > 0, np.diff(pt_off) > 0
    # (the candidate from k_ba_plus's own inputs -- alpha, the scaled step, the scales: x + alpha step scale may be one contracted operation, so
    #  the stored delta is not an input of the sum -- per parameter block: a pose, a camera's intrinsics, a landmark)
    tail = (cols, dim, off, c["mode"], c["ub"], cap["gcraw"], cap["gpraw"], used_c, used_p, c["fix0"])
    pl = B.plus(poses, intr, pts, a * cap["stc"].astype(LD) * cap["sc"], a * cap["stp"].astype(LD) * cap["sp"], *tail, LD)
    pl64 = B.plus(poses, intr, pts, alpha * cap["stc"] * cap["sc"], alpha * cap["stp"] * cap["sp"], *tail, np.float64)
    P2, I2, X2 = cap["poses2"].reshape(nc, 6), cap["intr2"].reshape(nc, 6), cap["pts2"].reshape(npts, 3)
    rep.add("candidate", max(fn_ratio(P2, pl["poses2"], pl64["poses2"], axis=1), fn_ratio(I2, pl["intr2"], pl64["intr2"], axis=1), fn_ratio(X2, pl["pts2"], pl64["pts2"], axis=1)))
    if c["mode"] == 1:
        rep.exact("focal clamp", (I2[:, :2] <= c["ub"]).all())
    # (|dx|^2 is summed from the candidate the kernel has just rounded: judged on that candidate)
    dx2 = ((P2.astype(LD) - poses) ** 2).sum() + ((I2.astype(LD) - intr) ** 2).sum() + (cap["dlp"].astype(LD) ** 2).sum()
    rep.add("|dx|^2", sum_ratio(cap["scal"][3], (dx2, dx2, pl["dx2"][2] + 1)))
    rep.add("|x|^2", sum_ratio(cap["scal"][4], pl["x2"]))
    d1c, d1p = cap["stc"].astype(LD) * cap["sc"], cap["stp"].astype(LD) * cap["sp"]
    g1 = B.plus(poses, intr, pts, d1c, d1p, cols, dim, off, c["mode"], c["ub"], cap["gcraw"], cap["gpraw"], used_c, used_p, c["fix0"], LD)["gd"]
    rep.add("g.delta", sum_ratio(cap["scal"][8], (g1[0], g1[1], g1[2] + 2)))
    rep.exact("non-finite count", cap["scal"][9] == 0.0 and cap["scal"][13] == 0.0)
    t2, t264 = B.cam_rot_table(P2, LD), B.cam_rot_table(P2, np.float64)
    tab2 = cap["crot2"].reshape(nc, B.CROT)
    rep.add("crot2", max(fn_ratio(tab2[:, a_:b_], t2[:, a_:b_], t264[:, a_:b_], axis=1) for a_, b_ in ((0, 9), (9, 18), (18, 23))))
    # candidate cost: from the GPU's candidate; the residuals are the kernel's own (function-type), so their allowance is carried into the sum
    rc = B.residual(P2.astype(LD)[ocam], I2.astype(LD)[ocam], X2.astype(LD)[opt], uv.astype(LD))
    rc64 = B.residual(P2[ocam], I2[ocam], X2[opt], uv)
    e_o = 16 * np.maximum(np.abs(rc64 - rc), LD(U) * np.abs(rc + uv))
    cc = B.cost_of(rc)
    bound = B.gamma(cc[2]) * cc[1] + (np.abs(rc) * e_o).sum() + (e_o * e_o).sum() / 2
    rep.add("candidate cost", float(abs(LD(cap["scal"][1]) - cc[0]) / bound))
    # projected gradient maximum: the kernel's own IEEE operations, so its bits
    rep.exact("gradient max (%.17g)" % cap["scal"][12], cap["scal"][12] == B.projected_gradient_max(cap["gcraw"], cap["gpraw"], intr, cols, dim, c["mode"], c["ub"]))
    # ---- line-search trials of the iteration
    for t, (al, cost_t, dg, dmax) in enumerate(tri):
        if np.isnan(dg):
            continue
        la = LD(al)
        tp = B.plus(poses, intr, pts, la * d1c, la * d1p, cols, dim, off, c["mode"], c["ub"], cap["gcraw"], cap["gpraw"], used_c, used_p, c["fix0"], LD)
        # the kernel differentiates at ITS candidate, which is the reference's rounded to float64
        tP, tI, tX = (np.asarray(tp[k], np.float64) for k in ("poses2", "intr2", "pts2"))
        v, A, m = B.directional_derivative(tP, tI, tX, uv, ocam, opt, cols, dim, off, la * d1c, la * d1p)
        rr = B.residual(tP.astype(LD)[ocam], tI.astype(LD)[ocam], tX.astype(LD)[opt], uv.astype(LD))
        rr64 = B.residual(tP[ocam], tI[ocam], tX[opt], uv)
        e_t = 16 * np.maximum(np.abs(rr64 - rr), LD(U) * np.abs(rr + uv))
        ct = B.cost_of(rr)
        rep.add("trial %d cost" % t, float(abs(LD(cost_t) - ct[0]) / (B.gamma(ct[2]) * ct[1] + (np.abs(rr) * e_t).sum() + (e_t * e_t).sum() / 2)))
        rep.add("trial %d |delta|inf" % t, sum_ratio(dmax, (max(np.abs(d1c).max() if n else 0, np.abs(d1p).max()), max(np.abs(d1c).max() if n else 0, np.abs(d1p).max()), 4)))
        # (directional derivative: r'(J d) / alpha with r and J the kernel's own function-type values: judged like the Jacobian, against
        #  the float64 run of the same expression)
        v64, _, _ = B.directional_derivative(tP, tI, tX, uv, ocam, opt, cols, dim, off, np.asarray(la * d1c, np.float64), np.asarray(la * d1p, np.float64), np.float64)
        rep.add("trial %d derivative" % t, float(abs(LD(dg) * la - v) / (B.gamma(m) * A + 16 * max(abs(LD(v64) - v), LD(U) * A))))
    # ---- delta end to end from the problem's inputs
    if e2e:
        o = dict(mode=c["mode"], fix0=c["fix0"], fix1=c["fix1"], jacobi=c["jacobi"], ub=c["ub"], lo=LO, hi=HI)
        fl, f6 = B.full_step(sc, o, c["radius"], LD), B.full_step(sc, o, c["radius"], np.float64)
        for tag, g_, k in (("cameras", d1c, "dlc"), ("landmarks", d1p, "dlp")):
            nrm = lambda v_: np.sqrt((np.asarray(v_, LD) ** 2).sum())
            eg, ef = nrm(np.asarray(g_, np.float64).astype(LD) - fl[k]), nrm(f6[k].astype(LD) - fl[k])
            rep.add("delta " + tag, float(eg / (16 * max(ef, LD(U) * nrm(fl[k])))) if nrm(fl[k]) > 0 else float(eg != 0))
    rep.done()
    return P2, I2, X2


# ---------------------------------------------------------------------------------------------------------------------
# scenes
def tracks_scene(nc, tracks, seed, k1k2=(ba_graphs.K1, ba_graphs.K2)):
    """make_scene's ring of cameras and ball of points (every camera sees every point: depth >= 7) under an explicit list of tracks,
    graph_scene's intrinsics (fy = 1.07 fx, the principal point moved, k1 and k2 of order 1e-1 / 1e-2)"""
    base = synth_ba.make_scene(nc, len(tracks), obs_per_point=1, seed=seed)
    rng = np.random.default_rng(seed + 15485863)
    intr = base["intr_gt"].copy()
    intr[:, 1] *= 1.07
    intr[:, 2] += 3.5
    intr[:, 3] -= 2.25
    intr[:, 4], intr[:, 5] = k1k2
    sc = {"poses_gt": base["poses_gt"], "points_gt": base["points_gt"], "poses": base["poses"], "points": base["points"], "intrinsics": intr}
    sc = ba_graphs._finish(sc, base["poses_gt"], intr, base["points_gt"], [np.asarray(t, np.int64) for t in tracks], rng)
    assert (B.depth(sc["poses"][sc["obs_cam"]], sc["points"][sc["obs_pt"]]) >= 0.5).all()
    assert (np.abs(sc["intrinsics"][:, 4]) >= 1e-2).all() and (np.abs(sc["intrinsics"][:, 5]) >= 1e-3).all()
    return sc


def shared_pairs_scene(shares, seed, first=1):
    """cameras first, first + 1 | first + 2, first + 3 | ...: the i-th couple shares exactly shares[i] landmarks that nobody else sees"""
    tracks = []
    for i, s in enumerate(shares):
        tracks += [(first + 2 * i + 1, first + 2 * i)] * s      # (the larger camera first: unsorted inside the track)
    return tracks_scene(first + 2 * len(shares), tracks, seed), tracks


def seg(sc, c, mode, fix0=1, fix1=1):
    nc = len(sc["poses"])
    _, dim, _ = B.structure(nc, mode, fix0, fix1)
    off, _, _ = B.pair_lists(sc["obs_cam"], sc["pt_off"], dim, nc)
    return np.diff(off).reshape(nc, nc)


def sumsq(sc):
    k = np.diff(sc["pt_off"])
    return int((k * k).sum())


# ---------------------------------------------------------------------------------------------------------------------
def test_camera_model_and_small_observation_counts(tmp_path):
    """zero, sub-sqrt(eps), sub-1e-2 and ordinary angles under non-zero distortion; camera dimensions 0, 3, 6 (mode 0) and 4, 7, 10 (mode
    1); a camera without observations; Jacobi scaling off and on; 1 ... 257 observations (the edges of the 64-row and 128-row blocks)"""
    r8, r11 = ba_graphs.scene("rig8"), ba_graphs.scene("rig11")
    for name, sc in (("rig8", r8), ("rig11", r11)):
        ba_graphs.conditions(name, sc)
        assert (B.depth(sc["poses"][sc["obs_cam"]], sc["points"][sc["obs_pt"]]) >= 0.5).all() and (sc["intrinsics"][:, 4:] != 0).all()
    r8 = ba_graphs.select(r8, r8["obs_cam"] != 5)
    r11 = ba_graphs.select(r11, r11["obs_cam"] != 7)
    assert np.bincount(r8["obs_cam"], minlength=8)[5] == 0 and np.bincount(r11["obs_cam"], minlength=11)[7] == 0
    scenes = {"rig8": r8, "rig11": r11}
    cases = [case("rig8_m0_j1", "rig8"), case("rig8_m0_j0", "rig8", jacobi=0), case("rig11_m1_j1", "rig11", mode=1), case("rig11_m1_j0", "rig11", mode=1, jacobi=0)]
    for i, no in enumerate((1, 63, 64, 65, 127, 128, 129, 255, 257)):
        keep = np.zeros(len(r11["obs_cam"]), bool)
        keep[:no] = True
        scenes["rig11_%d" % no] = ba_graphs.select(r11, keep)
        cases.append(case("rig11_no%d" % no, "rig11_%d" % no, mode=i % 2, jacobi=(i // 2) % 2))
    assert {0, 3, 6} == set(B.structure(8, 0, 1, 1)[1]) and {4, 7, 10} == set(B.structure(11, 1, 1, 1)[1])
    caps = run_tool(tmp_path, scenes, cases)
    for c in cases:
        judge(scenes[c["scene"]], c, caps[c["name"]], e2e=c["scene"] in ("rig8", "rig11"), expect=dict(csplit=1, offdiag_kernel=1))


SHARES = (0, 1, 5, 6, 21, 22, 32, 33, 63, 64, 65, 127, 128, 129)


def test_off_diagonal_lists_on_the_one_wave_kernel(tmp_path):
    """camera couples that share exactly 0 ... 129 landmarks: every edge of the 64-pair chunk and of the 4-step gather trip of
    k_ba_schur_mfma<4>, and the insertion sort's last length (32) beside the LDS sort's first (33)"""
    sc, _ = shared_pairs_scene(SHARES, 201)
    nc = len(sc["poses"])
    s = seg(sc, None, 0)
    assert [int(s[2 + 2 * i, 1 + 2 * i]) for i in range(len(SHARES))] == list(SHARES) and s.sum() == sum(SHARES)
    assert sumsq(sc) // (nc * (nc - 1) // 2) <= 128
    cases = [case("pairs_m0", "pairs"), case("pairs_m1", "pairs", mode=1)]
    caps = run_tool(tmp_path, {"pairs": sc}, cases)
    for c in cases:
        judge(sc, c, caps[c["name"]], e2e=True, expect=dict(offdiag_kernel=1, pair_path=1))      # (other camera dimensions: the lists are built again)


def test_long_lists_on_the_workgroup_kernel(tmp_path):
    """four free cameras with lists of 511, 512, 513 and 1000 entries: k_ba_schur_mfma_wg's eight waves over eight chunks exactly, one
    pair short and one pair over, and a second trip"""
    tracks = [(2, 1)] * 511 + [(3, 2)] * 512 + [(4, 3)] * 513 + [(4, 1)] * 1000
    sc = tracks_scene(5, tracks, 202)
    s = seg(sc, None, 0)
    assert (s[2, 1], s[3, 2], s[4, 3], s[4, 1]) == (511, 512, 513, 1000) and sumsq(sc) // 10 > 128
    assert np.bincount(sc["obs_cam"], minlength=5)[0] == 0
    cases = [case("wg_m0", "wg"), case("wg_m1_free", "wg", mode=1, fix1=0)]
    caps = run_tool(tmp_path, {"wg": sc}, cases)
    for c in cases:
        judge(sc, c, caps[c["name"]], e2e=True, expect=dict(offdiag_kernel=2))


@pytest.mark.parametrize("L", [4096, 4097])
def test_long_segments_of_the_pair_sort(tmp_path, L):
    """three cameras that all see L landmarks: three lists of L entries -- the LDS bitonic sort's last length and the global one's first --
    beside couples with 64 and 65 (a full network of 64 and the first padded one of 128)"""
    tracks = [(3, 1, 2)] * L + [(5, 4)] * 64 + [(7, 6)] * 65
    sc = tracks_scene(8, tracks, 203)
    s = seg(sc, None, 0)
    assert (s[2, 1], s[3, 1], s[3, 2], s[5, 4], s[7, 6]) == (L, L, L, 64, 65) and sumsq(sc) > 16384
    c = case("sort_%d" % L, "sort")
    caps = run_tool(tmp_path, {"sort": sc}, [c])
    judge(sc, c, caps[c["name"]], expect=dict(pair_path=2, offdiag_kernel=2))


def _builder_tracks(nc, extra, seed):
    rng = np.random.default_rng(seed)
    tracks = [tuple(rng.permutation(nc)[:4]) for _ in range(1000)]
    for _ in range(42 + extra):          # a landmark that sees one camera twice: diagonal lists
        a, b = rng.permutation(nc)[:2]
        tracks.append((a, b, a))
    return tracks


def test_list_builders_at_their_limits(tmp_path):
    """k_pair_small at nc = 32 (1024 keys) with sum k^2 just under 16384; count / scan / fill just over it, and at nc = 33 (1089 keys: two
    scan chunks); repeated (landmark, camera) observations, so the diagonal lists are not empty"""
    scenes = {"small": tracks_scene(32, _builder_tracks(32, 0, 204), 204), "over": tracks_scene(32, _builder_tracks(32, 1, 204), 204),
              "keys": tracks_scene(33, _builder_tracks(33, 0, 205), 205)}
    assert sumsq(scenes["small"]) == 16378 and sumsq(scenes["over"]) == 16387 and 33 * 33 > 1024
    for sc in scenes.values():
        assert seg(sc, None, 1).diagonal().sum() > 0 and ba_graphs.repeated_second(sc).any()
    cases = [case("small32", "small", mode=1), case("over32", "over", mode=1), case("keys33", "keys", mode=1)]
    caps = run_tool(tmp_path, scenes, cases)
    for c, path in zip(cases, (1, 2, 2)):
        judge(scenes[c["scene"]], c, caps[c["name"]], e2e=c["name"] == "small32", expect=dict(pair_path=path, offdiag_kernel=1))


def _counted_scene(counts, fillers, seed):
    """cameras 1 .. len(counts) with exactly counts[i] observations, every landmark also seen by one of `fillers` further cameras in turn"""
    tracks = []
    f0 = 1 + len(counts)
    for i, k in enumerate(counts):
        tracks += [(1 + i, f0 + (len(tracks) + t) % fillers) for t in range(k)]
    sc = tracks_scene(f0 + fillers, tracks, seed)
    assert list(np.bincount(sc["obs_cam"], minlength=f0 + fillers)[1:f0]) == list(counts)
    return sc


@pytest.mark.parametrize("which", [1, 2, 3])
def test_per_camera_kernels_at_their_trip_and_split_edges(tmp_path, which):
    """cameras with 1 ... 1537 observations: the 32-observation chunks and 256-observation trips of k_ba_cam_raw, the 1024-observation trip
    of the Schur diagonal kernel, and the splits over 1, 2 and 3 workgroups (a split of 2 begins at 769 observations)"""
    counts, fillers = {1: ((1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 768), 4), 2: ((769, 1023, 1024, 1025), 6), 3: ((1537, 1, 300), 4)}[which]
    sc = _counted_scene(counts, fillers, 205 + which)
    kmax = int(np.bincount(sc["obs_cam"]).max())
    assert kmax == max(counts) and B.cam_split(len(sc["poses"]), kmax) == which
    c = case("split%d" % which, "counted", mode=1)
    caps = run_tool(tmp_path, {"counted": sc}, [c])
    judge(sc, c, caps[c["name"]], expect=dict(csplit=which))


@pytest.mark.parametrize("nc", [128, 130])
def test_many_cameras_take_the_shallow_diagonal_kernel(tmp_path, nc):
    """nc >= 128: k_ba_schur_diag_mfma<4>, no split whatever the observation counts"""
    sc = ba_graphs.graph_scene(nc, 300, 206, (2, 3, 4, 5), repeat=0.1)
    assert (B.depth(sc["poses"][sc["obs_cam"]], sc["points"][sc["obs_pt"]]) >= 0.5).all()
    c = case("many%d" % nc, "many", mode=1)
    caps = run_tool(tmp_path, {"many": sc}, [c])
    judge(sc, c, caps[c["name"]], expect=dict(diag_smb=4, csplit=1, pair_path=2, offdiag_kernel=1))


def test_reduced_dimension_at_the_block_edges(tmp_path):
    """n = 384 = npad (65 cameras, mode 0, camera 1 free): no right-hand-side row, the unfused finish, the forward substitution as a
    launch of its own; n = 255 (44 cameras): the beta row is the last row of its block; n = 387 and 381: the rows next to the edge"""
    s65, s44 = ba_graphs.graph_scene(65, 300, 207, (2, 3, 4), repeat=0.1), ba_graphs.graph_scene(44, 200, 208, (2, 3, 4), repeat=0.1)
    cases = [case("n384", "s65", fix1=0), case("n381", "s65"), case("n387", "s65", fix0=0), case("n255", "s44")]
    dims = [int(B.structure(len(s["poses"]), 0, c["fix0"], c["fix1"])[2][-1]) for s, c in zip((s65, s65, s65, s44), cases)]
    assert dims == [384, 381, 387, 255] and B.padded(384) == 384 and 255 % 128 == 127
    caps = run_tool(tmp_path, {"s65": s65, "s44": s44}, cases)
    for c in cases:
        judge(s65 if c["scene"] == "s65" else s44, c, caps[c["name"]], e2e=True, expect=dict(fin=-1 if c["name"] == "n384" else 1, fused_finish=int(c["name"] != "n384")))


def test_focal_bounds_projection_and_clamp(tmp_path):
    """mode 1 with focal lengths that start above the bound (the projection at the start) and just below it with the step crossing (the
    clamp in Plus, |dx|^2 of the clamped step, the projected gradient)"""
    sc = ba_graphs.copy_scene(ba_graphs.scene("rig11"))
    ub = 600.0
    sc["intrinsics"][::2, 0] = ub + 14.4
    sc["intrinsics"][1::2, 0] = ub - 0.5
    sc["intrinsics"][:, 1] = ub - 0.25
    c = case("bounds", "b", mode=1, ub=ub)
    caps = run_tool(tmp_path, {"b": sc}, [c])
    cap = caps["bounds"]
    assert cap["bound_projections"] == 6
    P2, I2, X2 = judge(sc, c, cap)
    assert (I2[:, :2] == ub).sum() >= 6, "no focal length was clamped by the step: the case does not do what it is here for"


def last_accepted(log, k):
    """the last iteration before k whose step was accepted (0: none), from the logged scalars: rho = (cost - candidate cost) / model change
    -- valid for iterations without backtracks, whose logged candidate cost is the full step's"""
    j_acc = 0
    for j in range(1, k):
        cost, cand, model = log[j - 1, 0], log[j - 1, 1], log[j - 1, 2]
        assert log[j - 1, 14] == 0
        if log[j - 1, 13] == 0 and log[j - 1, 9] == 0 and model > 0 and (cost - cand) / model > 1e-3:
            j_acc = j
    return j_acc


def capture_iteration(tmp_path, sc, k, log, **opts):
    """second run: iteration k, and the last accepted one before it, whose candidate is the point iteration k linearises at"""
    j = last_accepted(log, k)
    cases = ([case("at%d" % j, "s", iteration=j, **opts)] if j else []) + [case("at%d" % k, "s", iteration=k, **opts)]
    sub = tmp_path / "second"
    sub.mkdir()
    caps = run_tool(sub, {"s": sc}, cases)
    point = None
    if j:
        cj = caps["at%d" % j]
        assert cj["got_b"] == 1
        nc, npts = len(sc["poses"]), len(sc["points"])
        point = (cj["poses2"].reshape(nc, 6), cj["intr2"].reshape(nc, 6), cj["pts2"].reshape(npts, 3))
    return cases[-1], caps["at%d" % k], point


def test_line_search_trials_of_the_first_backtracking_iteration(tmp_path):
    """a far-off start with bounds (tests/test_ba_gpu.py's line-search scene): the first run logs the scalars of every iteration, the
    second captures the first iteration that backtracks; every trial's cost, directional derivative and |delta|_inf against the reference
    at that alpha, the next alpha against rcn_ls::next_step"""
    sc = synth_ba.make_scene(12, 200, obs_per_point=6, seed=1, perturb=(0.4, 2.0, 1.5))
    assert (B.depth(sc["poses"][sc["obs_cam"]], sc["points"][sc["obs_pt"]]) >= 0.5).all()
    cap0 = run_tool(tmp_path, {"far": sc}, [case("log", "far", iteration=12, mode=1)])["log"]
    log = cap0["log"].reshape(-1, 15)
    assert (log[:, 14] > 0).any(), "no iteration backtracks"
    k = int(np.flatnonzero(log[:, 14] > 0)[0]) + 1
    print("first backtracking iteration: %d (%d backtracks)" % (k, log[k - 1, 14]))
    c, cap, point = capture_iteration(tmp_path, sc, k, log, mode=1)
    tri = cap["trials"].reshape(-1, 4)
    assert len(tri) >= log[k - 1, 14] + 1 and not np.isnan(tri[0, 2])
    judge(sc, c, cap, point=point)
    start = (0.0, cap["scal"][0], cap["scal"][8], 1.0, 1.0)
    prev = (0.0, 0.0, 0.0, 0.0, 0.0)
    for t in range(len(tri) - 1):
        a, v, g, _ = tri[t]
        if np.isnan(g):
            break
        cur = (a, v, g, 1.0, 1.0)
        nxt = orc_ba.ls_next_step(start, prev, cur, 1e-3 * a, 0.6 * a)
        assert nxt == tri[t + 1, 0], (t, nxt, tri[t + 1, 0])
        prev = cur


def test_a_later_iteration_behind_a_rejected_step(tmp_path):
    """the iteration behind a rejected step keeps its diagonal (reuse_diag) and only damps the landmark blocks again at the smaller radius"""
    # (a far-off start of make_scene -- k1 = k2 = 0 -- whose fourth step the CPU oracle rejects; no other scene of this module leaves a step rejected)
    sc = synth_ba.make_scene(8, 150, obs_per_point=5, seed=1, perturb=(0.5, 2.5, 1.5))
    assert (B.depth(sc["poses"][sc["obs_cam"]], sc["points"][sc["obs_pt"]]) >= 0.5).all()
    cap0 = run_tool(tmp_path, {"far": sc}, [case("log", "far", iteration=12)])["log"]
    log = cap0["log"].reshape(-1, 15)
    rho = (log[:, 0] - log[:, 1]) / log[:, 2]
    rejected = np.flatnonzero((log[:, 2] > 0) & (rho <= 1e-3) & (log[:, 13] == 0))
    assert len(rejected) and rejected[0] + 2 <= len(log), "no step is rejected"
    k = int(rejected[0]) + 2
    print("first rejected iteration: %d; capturing %d" % (k - 1, k))
    c, cap, point = capture_iteration(tmp_path, sc, k, log)
    assert cap["radius"] < (1e4 if k == 2 else np.inf)
    judge(sc, c, cap, point=point)


def test_a_later_iteration_behind_an_accepted_step(tmp_path):
    """iteration 2 behind an accepted step: the diagonal and the damped inverses come from k_ba_gradmax's fused launch, the rotation table
    from k_ba_plus; the point it linearises at is the first iteration's candidate"""
    sc = ba_graphs.scene("few_cams")
    cases = [case("it1", "few", iteration=1), case("it2", "few", iteration=2)]
    caps = run_tool(tmp_path, {"few": sc}, cases)
    point = judge(sc, cases[0], caps["it1"], e2e=True)
    log = caps["it2"]["log"].reshape(-1, 15)
    rho = (log[0, 0] - log[0, 1]) / log[0, 2]
    assert rho > 1e-3 and caps["it2"]["radius"] > 1e4, "the first step was not accepted"
    assert caps["it2"]["scal"][0] == log[0, 1] or abs(caps["it2"]["scal"][0] - log[0, 1]) <= 1e-9 * log[0, 1]
    judge(sc, cases[1], caps["it2"], point=point)
