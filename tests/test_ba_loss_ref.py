"""The judge of the robust-loss tests checked on the CPU (no GPU here): tests/ba_loss_ref.py's lm_solve -- a whole mode-0
Levenberg-Marquardt solve composed of tests/ba_ref.py's stages -- against the CPU oracle at the trivial loss, and its float64 run against
its long-double run under every loss on scenes with planted outliers.  The criteria are those of
tests/test_ba_gpu.py::test_small_scenes_match_oracle: the same iterations and termination, cost_trace at rtol 1e-7, poses at atol 1e-6,
points at atol 1e-5."""
import numpy as np
import pytest

import ba_loss_ref as R
import ba_ref as B
from oracle import orc_ba
from reconstructor_amd import synth_ba

LD = B.LD


def agree(a, b):
    (P1, I1, X1, s1), (P0, I0, X0, s0) = a, b
    assert s1["iterations"] == s0["iterations"] and s1["termination"] == s0["termination"], (s1["iterations"], s0["iterations"], s1["termination"], s0["termination"])
    t1, t0 = np.asarray(s1["cost_trace"], np.float64), np.asarray(s0["cost_trace"], np.float64)
    assert len(t1) == len(t0) and np.allclose(t1, t0, rtol=1e-7, atol=0)
    assert np.allclose(np.asarray(P1, np.float64), np.asarray(P0, np.float64), atol=1e-6, rtol=0)
    assert np.allclose(np.asarray(X1, np.float64), np.asarray(X0, np.float64), atol=1e-5, rtol=0)
    assert np.array_equal(np.asarray(I1, np.float64), np.asarray(I0, np.float64))      # mode 0: the intrinsics do not move
    return float(np.abs(t1 / t0 - 1).max()), float(np.abs(np.asarray(P1, np.float64) - np.asarray(P0, np.float64)).max())


@pytest.mark.parametrize("nc,npts,k", [(6, 60, 4), (8, 120, 5), (4, 40, 3)])
def test_lm_solve_without_a_loss_is_the_oracle(nc, npts, k):
    sc = synth_ba.make_scene(nc, npts, obs_per_point=k, seed=5)
    o = orc_ba.default_options(nc)
    assert o.intrinsics_mode == 0
    ref = orc_ba.solve(sc, o, threads=2)
    for loss in (None, (R.TRIVIAL, 3.0)):
        for real in (np.float64, LD):
            got = R.lm_solve(sc, R.default_opts(nc), loss, real)
            print(nc, npts, k, loss, real.__name__, got[3]["iterations"], got[3]["termination"], agree(got, ref))
            for key in ("successful_steps", "unsuccessful_steps", "invalid_steps"):
                assert got[3][key] == ref[3][key]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("kind", [R.HUBER, R.SOFT_L1, R.CAUCHY])
def test_float64_and_long_double_agree_under_a_loss(kind, seed):
    """make_scene(6, 60, 4) with 20 of its 240 observations displaced by 20 to 120 px per axis, a = 2"""
    sc, idx = R.plant_outliers(synth_ba.make_scene(6, 60, obs_per_point=4, seed=seed), 20, seed)
    assert len(sc["obs_cam"]) == 240
    a = R.lm_solve(sc, R.default_opts(6), (kind, 2.0), np.float64)
    b = R.lm_solve(sc, R.default_opts(6), (kind, 2.0), LD)
    print(R.NAMES[kind], seed, a[3]["iterations"], a[3]["termination"], agree(a, b))
    assert a[3]["iterations"] >= 2 and a[3]["successful_steps"] >= 1
    # the loss did something: the robust cost is below the plain one at the same point, and the typical outlier carries a small weight
    rep = R.report(b[0], b[1], b[2], sc["obs_uv"], sc["obs_cam"], sc["obs_pt"], (kind, 2.0))
    # (a displaced observation whose landmark follows it keeps weight 1: the typical one is judged, 20 px at a = 2 is rho' <= 0.1)
    assert rep["n_beyond_scale"] >= 15 and np.median(np.float64(rep["weights"][idx])) < 0.2
    assert b[3]["final_cost"] < rep["s"].sum() / 2


def test_the_losses_in_both_dtypes():
    """rho' is the derivative of rho (centred difference in long double), rho(0) = 0, rho'(0) = 1, Huber is the identity up to b;
    float64 against long double to a few u"""
    s = np.array([0.0, 1e-6, 0.3, 3.999, 4.0, 4.001, 9.0, 1e4, 1e9])
    for kind in (R.TRIVIAL, R.HUBER, R.SOFT_L1, R.CAUCHY):
        loss = (kind, 2.0)
        r, d = R.rho(loss, s), R.drho(loss, s)
        r64, d64 = R.rho(loss, s, np.float64), R.drho(loss, s, np.float64)
        assert r64.dtype == np.float64 and r.dtype == LD
        assert np.all(np.abs(r64 - r) <= 4 * B.U * np.abs(r)) and np.all(np.abs(d64 - d) <= 4 * B.U * d)
        assert r[0] == 0 and d[0] == 1
        if kind == R.HUBER:
            assert np.array_equal(r64[:5], s[:5]) and (d64[:5] == 1).all() and (d64[5:] < 1).all()
        h = LD(2.0) ** -20 * s[np.array([2, 3, 6, 7, 8])].astype(LD)
        x = s[np.array([2, 3, 6, 7, 8])].astype(LD)
        fd = (R.rho(loss, x + h) - R.rho(loss, x - h)) / (2 * h)
        assert np.all(np.abs(fd - R.drho(loss, x)) <= LD(2.0) ** -36 * R.drho(loss, x))
    assert not np.isfinite(np.float64(R.rho((R.CAUCHY, 2.0), np.array([np.nan, np.inf]), np.float64))).any()


def test_corrected_rows_cost_and_derivative_are_consistent():
    """the gradient of the robust cost along a direction, three ways: from the corrected rows (J_c' r_c), from directional_derivative
    (rho' r . J d), and by a centred difference of robust_cost in long double"""
    sc, _ = R.plant_outliers(synth_ba.make_scene(6, 60, obs_per_point=4, seed=4), 20, 4)
    nc = 6
    cols, dim, off = B.structure(nc, 0, 1, 1)
    ocam, opt, uv = sc["obs_cam"].astype(np.int64), sc["obs_pt"].astype(np.int64), sc["obs_uv"]
    rng = np.random.default_rng(3)
    dlc, dlp = rng.normal(size=int(off[-1])) * 1e-3, rng.normal(size=3 * 60) * 1e-3
    for kind in (R.HUBER, R.SOFT_L1, R.CAUCHY):
        loss = (kind, 2.0)
        rows, plain, s = R.corrected_rows(sc["poses"], sc["intrinsics"], sc["points"], uv, ocam, opt, cols, dim, loss)
        assert np.allclose(np.float64(rows), np.float64(plain * np.sqrt(R.drho(loss, s))[:, None]), rtol=1e-15, atol=0)
        g_rows = B.gradient_along(rows, dlc, dlp, ocam, opt, dim, off)[0]
        g_dir = R.directional_derivative(sc["poses"], sc["intrinsics"], sc["points"], uv, ocam, opt, cols, dim, off, dlc, dlp, loss)[0]
        assert abs(g_rows - g_dir) <= 1e-15 * abs(g_dir)

        def cost(t):
            used = np.ones(nc, bool), np.ones(60, bool)
            pl = B.plus(sc["poses"], sc["intrinsics"], sc["points"], LD(t) * dlc, LD(t) * dlp, cols, dim, off, 0, 0.0, np.zeros((nc, 10)), np.zeros(180), *used, 1)
            return R.robust_cost(B.residual(pl["poses2"][ocam], pl["intr2"][ocam], pl["pts2"][opt], uv.astype(LD)), loss)[0]
        t = LD(1e-4)
        fd = (cost(t) - cost(-t)) / (2 * t)
        print(R.NAMES[kind], float(g_dir), float(fd))
        assert abs(fd - g_dir) <= 1e-5 * abs(g_dir)
        assert R.robust_cost(plain[:, 26:], loss)[0] == R.rho(loss, s).sum() / 2
