"""GPU suite: the robust losses of the bundle adjustment through the C ABI (rcn_ba_solve_robust, csrc/ba.hip).

  bits        loss NULL, the trivial kind, and Huber at scale 1e150 (the robust kernels with every weight exactly 1) all give
              rcn_ba_solve's bits -- poses, intrinsics, points, cost_trace, counters -- on a mode-0 and a mode-1 scene; two robust solves
              give the same bits.
  solves      whole solves under each loss against tests/ba_loss_ref.py's lm_solve in long double, by the criteria of
              tests/test_ba_gpu.py::test_small_scenes_match_oracle (iterations, termination, cost_trace at rtol 1e-7, poses at 1e-6,
              points at 1e-5, the final robust RMS within 1e-5 px).  The judge alone is far inside them (tests/test_ba_loss_ref.py).
  outliers    make_scene(6, 60, 4) with 20 of its 240 observations -- 8 % -- displaced by 20 px or more per axis against 0.5 px of noise:
              Cauchy must end closer to the ground truth's camera centres than the plain solve.  The ordering is no matter of margin: the
              plain cost gives one such observation the pull of 1600 inliers.
  report      n_obs and n_beyond_scale exactly (no reference s within 1e-9 b of b); plain_rms_px by the sum-type rule, each term with its
              function-type allowance; max_residual_px and the weights function-type (ba_loss_ref.weight_floors).
  errors      unknown kinds, scale 0, negative, inf and NaN: RCN_ERR_ARG with a message; a valid call works afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest

import ba_loss_ref as R
import ba_ref as B
import test_ba_step_gpu as T
from reconstructor_amd import _lib, synth_ba

pytestmark = pytest.mark.gpu
LD, U = B.LD, B.U
LOSSES = [(R.HUBER, 2.0), (R.SOFT_L1, 2.0), (R.CAUCHY, 2.0)]


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("out"):
        seed = int(name[3:])
        return R.plant_outliers(synth_ba.make_scene(6, 60, obs_per_point=4, seed=seed), 20, seed)[0]
    if name == "twelve":      # 12 cameras: rcn_ba_default_options would pick intrinsics_mode 1
        return R.plant_outliers(synth_ba.make_scene(12, 100, obs_per_point=5, seed=11), 40, 11)[0]
    if name == "bounds":      # mode 1 as the defaults give it, fx and fy of some cameras above the bound at the start
        sc = dict(R.plant_outliers(synth_ba.make_scene(12, 150, obs_per_point=5, seed=12, focal_factor=1.9), 60, 12)[0])
        return sc
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, loss):
    sc = scene(name)
    return R.lm_solve(sc, R.default_opts(len(sc["poses"])), loss, LD)


def options(ctx, sc, mode=None):
    from reconstructor_amd import ba
    o = ba.default_options(ctx, len(sc["poses"]))
    if mode is not None:
        o.intrinsics_mode = mode
    return o


def same_solution(a, b):
    (P1, I1, X1, s1), (P0, I0, X0, s0) = a, b
    assert P1.tobytes() == P0.tobytes() and I1.tobytes() == I0.tobytes() and X1.tobytes() == X0.tobytes()
    assert s1["cost_trace"].tobytes() == s0["cost_trace"].tobytes()
    for k in ("initial_cost", "final_cost", "iterations", "successful_steps", "unsuccessful_steps", "invalid_steps", "termination",
              "line_search_backtracks", "bound_projections", "reduced_dim"):
        assert s1[k] == s0[k], k


@pytest.mark.parametrize("name,mode", [("out1", 0), ("bounds", 1)])
def test_no_loss_trivial_and_an_idle_huber_give_the_plain_bits(gpu_ctx, name, mode):
    from reconstructor_amd import ba
    sc = scene(name)
    o = options(gpu_ctx, sc)
    assert o.intrinsics_mode == mode
    plain = ba.solve_scene(gpu_ctx, sc, o)
    print(name, "iterations", plain[3]["iterations"], "backtracks", plain[3]["line_search_backtracks"], "termination", plain[3]["termination"])
    assert plain[3]["successful_steps"] >= 2
    same_solution(ba.solve_scene(gpu_ctx, sc, o, report=True), plain)                  # loss == NULL through rcn_ba_solve_robust
    same_solution(ba.solve_scene(gpu_ctx, sc, o, loss=(R.TRIVIAL, 2.0)), plain)
    same_solution(ba.solve_scene(gpu_ctx, sc, o, loss=(R.TRIVIAL, -1.0)), plain)       # (the trivial kind's scale means nothing)
    idle = ba.solve_scene(gpu_ctx, sc, o, loss=(R.HUBER, 1e150), report=True)          # the robust kernels, every weight exactly 1
    same_solution(idle, plain)
    assert (idle[3]["loss_weights"] == 1.0).all() and idle[3]["loss_report"]["n_beyond_scale"] == 0


@pytest.mark.parametrize("name,mode", [("out2", 0), ("bounds", 1)])
@pytest.mark.parametrize("loss", LOSSES, ids=lambda l: R.NAMES[l[0]])
def test_two_robust_solves_give_the_same_bits(gpu_ctx, name, mode, loss):
    from reconstructor_amd import ba
    sc = scene(name)
    a = ba.solve_scene(gpu_ctx, sc, options(gpu_ctx, sc), loss=loss, report=True)
    b = ba.solve_scene(gpu_ctx, sc, options(gpu_ctx, sc), loss=loss, report=True)
    print(name, R.NAMES[loss[0]], "iterations", a[3]["iterations"], "backtracks", a[3]["line_search_backtracks"], "rms", a[3]["final_rms_px"])
    same_solution(a, b)
    assert a[3]["loss_weights"].tobytes() == b[3]["loss_weights"].tobytes() and a[3]["loss_report"] == b[3]["loss_report"]
    assert a[3]["final_cost"] < a[3]["initial_cost"]


@pytest.mark.parametrize("name", ["out1", "out2", "out3", "twelve"])
@pytest.mark.parametrize("loss", LOSSES, ids=lambda l: R.NAMES[l[0]])
def test_whole_solves_match_the_long_double_loop(gpu_ctx, name, loss):
    from reconstructor_amd import ba
    sc = scene(name)
    P0, I0, X0, s0 = reference(name, loss)
    P1, I1, X1, s1 = ba.solve_scene(gpu_ctx, sc, options(gpu_ctx, sc, mode=0), loss=loss)
    t0 = np.asarray(s0["cost_trace"], np.float64)
    n = min(len(t0), len(s1["cost_trace"]))
    print(name, R.NAMES[loss[0]], "reference", s0["iterations"], s0["termination"], float(s0["final_rms_px"]), "gpu", s1["iterations"], s1["termination"], s1["final_rms_px"],
          "trace %.3g poses %.3g points %.3g" % (np.abs(s1["cost_trace"][:n] / t0[:n] - 1).max(), np.abs(P1 - np.float64(P0)).max(), np.abs(X1 - np.float64(X0)).max()))
    assert abs(s1["initial_cost"] - float(s0["initial_cost"])) <= 1e-9 * float(s0["initial_cost"])
    assert abs(s1["final_rms_px"] - float(s0["final_rms_px"])) <= 1e-5
    assert s1["iterations"] == s0["iterations"] and s1["termination"] == s0["termination"]
    assert np.allclose(s1["cost_trace"][:n], t0[:n], rtol=1e-7)
    assert np.allclose(P1, np.float64(P0), atol=1e-6) and np.allclose(X1, np.float64(X0), atol=1e-5) and np.allclose(I1, np.float64(I0), rtol=1e-6, atol=1e-6)
    assert s1["final_rms_px"] == np.sqrt(2.0 * s1["final_cost"] / len(sc["obs_cam"]))        # the robust cost's, as the header says


def centres(P):
    P = np.asarray(P, np.float64)
    return np.stack([-synth_ba.rodrigues(p[:3]).T @ p[3:] for p in P])


@pytest.mark.parametrize("name", ["out1", "out2", "out3"])
def test_cauchy_ends_closer_to_the_ground_truth_than_no_loss(gpu_ctx, name):
    from reconstructor_amd import ba
    sc = scene(name)
    gt = centres(sc["poses_gt"])
    plain = ba.solve_scene(gpu_ctx, sc)
    cauchy = ba.solve_scene(gpu_ctx, sc, loss=("cauchy", 2.0))
    e0, e1 = np.linalg.norm(centres(plain[0]) - gt, axis=1).mean(), np.linalg.norm(centres(cauchy[0]) - gt, axis=1).mean()
    print(name, "mean centre error: no loss %.4f, Cauchy %.4f" % (e0, e1))
    assert e1 < e0


@pytest.mark.parametrize("name,mode", [("out3", 0), ("bounds", 1)])
@pytest.mark.parametrize("loss", LOSSES, ids=lambda l: R.NAMES[l[0]])
def test_the_report_at_the_final_point(gpu_ctx, name, mode, loss):
    from reconstructor_amd import ba
    sc = scene(name)
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, options(gpu_ctx, sc), loss=loss, report=True)
    ocam, opt, uv = sc["obs_cam"].astype(np.int64), sc["obs_pt"].astype(np.int64), sc["obs_uv"]
    ref, f64 = R.report(P, I, X, uv, ocam, opt, loss), R.report(P, I, X, uv, ocam, opt, loss, np.float64)
    b = LD(np.float64(loss[1]) * np.float64(loss[1]))
    assert (np.abs(ref["s"] - b) > LD(1e-9) * b).all()
    rep, w = s["loss_report"], s["loss_weights"]
    assert rep["n_obs"] == ref["n_obs"] == len(ocam) and rep["n_beyond_scale"] == ref["n_beyond_scale"]
    assert 0 < rep["n_beyond_scale"] < len(ocam)
    # sum s: the summation's bound (two products and an addition per term, the sum) plus each term's function-type allowance
    r, r64 = ref["r"], f64["r"]
    e = 16 * np.maximum(np.abs(r64 - r), LD(U) * np.abs(r + uv))
    S = ref["s"].sum()
    bound = B.gamma(len(ocam) + 3) * S + (2 * np.abs(r) * e + e * e).sum()
    rel = bound / S
    ratio_rms = float(abs(LD(rep["plain_rms_px"]) / ref["plain_rms_px"] - 1) / (rel / 2 * (1 + rel) + 3 * LD(U)))
    fl_d, _ = R.weight_floors(loss, r, uv)
    ratio_w = T.fn_ratio(w, ref["weights"], f64["weights"], floor=fl_d)
    k = int(np.argmax(ref["s"]))
    smax_floor = 2 * (np.abs(r[k]) * np.abs(r[k] + uv[k])).sum() / (2 * ref["max_residual_px"]) + ref["max_residual_px"]
    ratio_max = T.fn_ratio(np.array([rep["max_residual_px"]]), np.array([ref["max_residual_px"]]), np.array([f64["max_residual_px"]]), floor=np.array([smax_floor]))
    print(name, R.NAMES[loss[0]], "beyond", rep["n_beyond_scale"], "rms %.6f (%.3g of its bound) max %.4f (%.3g) weights %.3g" % (rep["plain_rms_px"], ratio_rms, rep["max_residual_px"], ratio_max, ratio_w))
    assert ratio_rms <= 1 and ratio_max <= 1 and ratio_w <= 1
    assert (w >= R.DBL_MIN).all() and (w <= 1).all()


def test_argument_errors(gpu_ctx):
    from reconstructor_amd import ba
    sc = scene("out1")
    L = gpu_ctx.lib
    poses, intr, pts = (np.array(sc[k], np.float64, order="C") for k in ("poses", "intrinsics", "points"))
    uv, cam, pt = np.ascontiguousarray(sc["obs_uv"], np.float64), np.ascontiguousarray(sc["obs_cam"], np.int32), np.ascontiguousarray(sc["obs_pt"], np.int32)
    pb = _lib.BaProblem(len(poses), len(pts), len(cam), 0, poses.ctypes.data, intr.ctypes.data, pts.ctypes.data, uv.ctypes.data, cam.ctypes.data, pt.ctypes.data)
    o = ba.default_options(gpu_ctx, len(poses))
    for kind, scale in ((4, 2.0), (-1, 2.0), (1, 0.0), (2, -1.0), (3, float("inf")), (1, float("nan")), (0, float("nan")), (0, float("inf"))):
        s = _lib.BaSummary()
        before = poses.copy()
        rc = L.rcn_ba_solve_robust(gpu_ctx.h, C.byref(pb), C.byref(o), C.byref(_lib.BaLoss(kind, 0, scale)), C.byref(s), None, None)
        msg = L.rcn_last_error(gpu_ctx.h).decode()
        print(kind, scale, rc, msg)
        assert rc == -1 and ("kind" in msg or "scale" in msg) and np.array_equal(before, poses)
        with pytest.raises(_lib.RcnError):
            ba.solve_scene(gpu_ctx, sc, loss=(kind, scale))
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, loss=("huber", 2.0))
    assert s["termination"] in (1, 2, 3) and s["final_cost"] < s["initial_cost"]
