"""The judge of the one-step tests (tests/ba_ref.py) checked on the CPU: its long-double Jacobian against mpmath at 50 digits and, at
float64, against the oracle's; its Schur path against a dense solve of the full normal equations; its model change against the
linearised cost; its float64 first step against the oracle's first accepted step.  Every test prints its figures before it asserts."""
import mpmath as mp
import numpy as np
import pytest

import ba_graphs
import ba_ref as B
from oracle import orc_ba
from reconstructor_amd import synth_ba

LD = B.LD
EPS_LD = float(np.finfo(LD).eps)


def _mp_residual(par, uv):
    w, t, K, X = par[0:3], par[3:6], par[6:12], par[12:15]
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    if th2 > mp.mpf(B.EPS):
        th = mp.sqrt(th2)
        c, s = mp.cos(th), mp.sin(th)
        n = [v / th for v in w]
        nx = cr(n, X)
        tmp = (n[0] * X[0] + n[1] * X[1] + n[2] * X[2]) * (1 - c)
        p = [X[i] * c + nx[i] * s + n[i] * tmp for i in range(3)]
    else:
        wx = cr(w, X)
        p = [X[i] + wx[i] for i in range(3)]
    p = [p[i] + t[i] for i in range(3)]
    x, y = p[0] / p[2], p[1] / p[2]
    rr = x * x + y * y
    d = K[4] * rr + K[5] * rr * rr
    return [K[0] * (x + d) + K[2] - uv[0], K[1] * (y + d) + K[3] - uv[1]]


def _observations():
    """about twenty observations: rotation magnitudes 0, below sqrt(eps) (first-order branch), between it and 1e-2, ordinary; k1, k2 != 0"""
    rng = np.random.default_rng(5)
    mags = [0.0, 1e-9, 1.2e-8, 1.6e-8, 1e-5, 5e-3, 9.9e-3, 1.01e-2, 5e-2, 0.7, 2.5]
    rows = []
    for i, m in enumerate(mags + mags[1:10]):
        ax = rng.standard_normal(3)
        w = ax / np.linalg.norm(ax) * m
        t = 0.3 * rng.standard_normal(3)
        X = synth_ba.rodrigues(w).T @ (np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1, 1), rng.uniform(4, 8)]) - t)      # in front of the camera
        K =np.array([614.4, 650.0, 259.5, 165.75, -0.08 * (1 + 0.1 * i), 0.02 + 0.005 * i])
        uv = np.trunc(synth_ba.project(np.concatenate([w, t]), K, X)[0] + rng.standard_normal(2))
        rows.append((np.concatenate([w, t]), K, X, uv))
    return [np.array([r[k] for r in rows]) for k in range(4)]


def test_long_double_jacobian_against_mpmath():
    assert EPS_LD < 2e-19, "np.longdouble is not the x87 extended format"
    pose, K, X, uv = _observations()
    th2 = (pose[:, :3] ** 2).sum(1)
    assert (th2 == 0).any() and ((th2 > 0) & (th2 <= B.EPS)).any() and ((th2 > B.EPS) & (th2 < 1e-4)).any() and (th2 > 1e-4).any()
    assert (B.depth(pose, X) >= 0.5).all()
    r, J = B.residual_jacobian(pose, K, X, uv, LD)
    r64, J64 = B.residual_jacobian(pose, K, X, uv, np.float64)
    mp.mp.dps = 50
    worst = worst64 = ratio = 0.0
    for o in range(len(pose)):
        par = [mp.mpf(float(v)) for v in np.concatenate([pose[o], K[o], X[o]])]
        u = [mp.mpf(float(v)) for v in uv[o]]
        rm = _mp_residual(par, u)
        Jm = np.empty((2, 15), object)
        for k in range(15):
            for i in range(2):
                Jm[i, k] = mp.diff(lambda v, i=i, k=k: _mp_residual(par[:k] + [v] + par[k + 1:], u)[i], par[k], h=mp.mpf(10) ** -20)
        for i in range(2):
            scale = max(abs(float(v)) for v in Jm[i])
            e = max(abs(float(mp.mpf(_ld_str(J[o, i, k])) - Jm[i, k])) for k in range(15))
            e64 = max(abs(float(mp.mpf(float(J64[o, i, k])) - Jm[i, k])) for k in range(15))
            worst, worst64 = max(worst, e / scale), max(worst64, e64 / scale)
            ratio = max(ratio, e / max(e64, B.U * scale))
            # per row: a few dozen long-double roundings, or -- where the formula itself amplifies, (1 - cos) / theta just above the
            # first-order branch -- far below what the float64 run of the same formula loses, which is what the GPU tests allow for
            assert e <= max(256 * EPS_LD * scale, e64 / 64), (o, i, e, e64, scale)
            # (the residual is a difference of pixel coordinates: its error is the prediction's)
            er = abs(float(mp.mpf(_ld_str(r[o, i])) - rm[i])) / (float(np.abs(uv[o]).max()) + 1.0)
            assert er <= 64 * EPS_LD, (o, i, er)
    print("Jacobian rows against mpmath: long double %.2e, float64 %.2e of the row's largest entry (eps_ld = %.1e)" % (worst, worst64, EPS_LD))
    print("largest long-double error as a part of max(float64 error, u |row|): %.2e" % ratio)
    assert ratio <= 1.0 / 64


def _ld_str(v):
    return np.format_float_scientific(v, precision=25, unique=False)


def test_float64_jacobian_against_the_oracle():
    pose, K, X, uv = _observations()
    r, J = B.residual_jacobian(pose, K, X, uv, LD)
    r64, J64 = B.residual_jacobian(pose, K, X, uv, np.float64)
    worst = 0.0
    for o in range(len(pose)):
        ro, Jo = orc_ba.residual_jacobian(pose[o], K[o], X[o], uv[o])
        for i in range(2):
            scale = float(np.abs(J[o, i]).max())
            e_orc = float(np.abs(Jo[i].astype(LD) - J[o, i]).max())
            e_64 = float(np.abs(J64[o, i].astype(LD) - J[o, i]).max())
            worst = max(worst, e_orc / max(e_64, B.U * scale))
            assert e_orc <= 16 * max(e_64, B.U * scale), (o, i, e_orc, e_64)
        er_orc, er_64 = float(np.abs(ro.astype(LD) - r[o]).max()), float(np.abs(r64[o].astype(LD) - r[o]).max())
        assert er_orc <= 16 * max(er_64, B.U * (float(np.abs(uv[o]).max()) + 1.0)), (o, er_orc, er_64)
    print("oracle Jacobian rows: at most %.2f of max(own float64 error, u |row|)" % worst)


OPTS0 = dict(mode=0, fix0=1, fix1=1, jacobi=1, ub=1000.0, lo=1e-6, hi=1e32)


def _small_scenes():
    a = ba_graphs.graph_scene(6, 40, 301, (1, 2, 3, 6), repeat=0.2)
    b = ba_graphs.rig_scene(5, 30, 302, k=3)
    return [("graph6 mode 0", a, OPTS0), ("graph6 mode 1 unscaled", a, dict(OPTS0, mode=1, jacobi=0, fix1=0)), ("rig5 mode 1", b, dict(OPTS0, mode=1))]


def _dense_step(st, sc, radius):
    """(Js'Js + D / r) ds = -Js'r assembled densely over [cameras | landmarks] in long double"""
    n, npts = int(st["off"][-1]), len(sc["points"])
    N = len(sc["obs_cam"])
    Js = np.zeros((2 * N, n + 3 * npts), LD)
    rows = st["rows"]
    for o in range(N):
        c, j = int(sc["obs_cam"][o]), int(sc["obs_pt"][o])
        dc, oc = int(st["dim"][c]), int(st["off"][c])
        for i in range(2):
            Js[2 * o + i, oc:oc + dc] = rows[o, 10 * i:10 * i + dc] * st["sc"][oc:oc + dc]
            Js[2 * o + i, n + 3 * j:n + 3 * j + 3] = rows[o, 20 + 3 * i:23 + 3 * i] * st["sp"][3 * j:3 * j + 3]
    r = rows[:, 26:].reshape(-1)
    D = np.concatenate([st["dgc"], st["dgp"]])
    A = Js.T @ Js + np.diag(D / LD(radius))
    return Js, r, B.solve_spd(A, -(Js.T @ r), LD)


@pytest.mark.parametrize("which", range(3))
def test_schur_path_against_the_dense_normal_equations(which):
    label, sc, opts = _small_scenes()[which]
    assert len(sc["poses"]) <= 6 and len(sc["points"]) <= 40
    radius = 1e4
    st = B.full_step(sc, opts, radius, LD)
    Js, r, ds = _dense_step(st, sc, radius)
    n = int(st["off"][-1])
    got = np.concatenate([st["stc"], st["stp"]])
    e = float(np.linalg.norm((got - ds).astype(np.float64)) / np.linalg.norm(ds.astype(np.float64)))
    kappa = np.linalg.cond(st["S"].astype(np.float64))
    print("%s: n %d, Schur step against the dense step %.2e (kappa(S) %.1e)" % (label, n, e, kappa))
    # both in long double: what is left is kappa eps_ld of either solve
    assert e <= 64 * kappa * EPS_LD + 1e-15, e
    # the model change against cost - |r + Js ds|^2 / 2
    mc, _, _ = B.model_change(st["rows"], st["sc"], st["stc"], st["sp"], st["stp"], np.asarray(sc["obs_cam"], np.int64), np.asarray(sc["obs_pt"], np.int64),
                              st["dim"], st["off"], LD)
    lin = r + Js @ got
    want = (r * r).sum() / 2 - (lin * lin).sum() / 2
    rel = float(abs(mc - want) / abs(want))
    print("%s: model change %.6e against the linearised cost: %.2e" % (label, float(mc), rel))
    assert mc > 0 and rel <= 1e-12, rel


def test_float64_first_step_against_the_oracle():
    sc = ba_graphs.scene("few_cams")
    o = orc_ba.default_options(len(sc["poses"]))
    _, _, _, s = orc_ba.solve(sc, o, threads=2)
    assert o.intrinsics_mode == 0 and s["successful_steps"] >= 1 and s["cost_trace"][1] < s["cost_trace"][0]
    opts = dict(mode=0, fix0=o.fix_cam0_pose, fix1=o.fix_cam1_translation, jacobi=o.jacobi_scaling, ub=o.focal_upper_bound, lo=o.min_lm_diagonal, hi=o.max_lm_diagonal)
    st = B.full_step(sc, opts, o.initial_trust_region_radius, np.float64)
    nc = len(sc["poses"])
    used_c, used_p = np.bincount(sc["obs_cam"], minlength=nc) > 0, np.diff(st["pt_off"]) > 0
    cand = B.plus(sc["poses"], st["intr"], sc["points"], st["dlc"], st["dlp"], st["cols"], st["dim"], st["off"], 0, opts["ub"], st["gcraw"], st["gpraw"],
                  used_c, used_p, 1, np.float64)
    r = B.residual(cand["poses2"][sc["obs_cam"]], cand["intr2"][sc["obs_cam"]], cand["pts2"][sc["obs_pt"]], np.asarray(sc["obs_uv"], np.float64))
    c1 = float((r * r).sum() / 2)
    print("cost %.9e -> %.9e, the oracle's trace %.9e -> %.9e" % (float(st["cost"]), c1, s["cost_trace"][0], s["cost_trace"][1]))
    assert abs(float(st["cost"]) - s["cost_trace"][0]) <= 1e-12 * s["cost_trace"][0]
    assert abs(c1 - s["cost_trace"][1]) <= 1e-7 * s["cost_trace"][1]      # (the whole-solve tests' rtol for a cost trace)


def test_pair_lists_have_the_lengths_the_graph_helper_counts():
    for name in ("long_small", "few_cams"):
        sc = ba_graphs.scene(name)
        nc = len(sc["poses"])
        _, dim, _ = B.structure(nc, 1 if nc >= 10 else 0, 1, 1)      # (the defaults at that many cameras: camera 0 is free from ten on)
        off, lst, keys = B.pair_lists(sc["obs_cam"], sc["pt_off"], dim, nc)
        assert np.array_equal(np.diff(off).reshape(nc, nc), ba_graphs.segment_lengths(sc)) and len(lst) == off[-1]
        for k in np.unique(keys):
            seg = lst[off[k]:off[k + 1]]
            assert (np.diff(seg.astype(np.int64)) > 0).all()
