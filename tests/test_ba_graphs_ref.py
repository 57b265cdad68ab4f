"""CPU tier of the graph-shape suite for bundle adjustment (tests/ba_graphs.py): the oracle, which the GPU suite
(tests/test_ba_graphs_gpu.py) compares against, is itself checked on these scenes -- against an independent minimiser, for
the cases doing what they are in the suite for, and for how much the ORDER of the observations inside a track moves it (the
floor under every GPU tolerance: nothing but the order of summation changes).  No GPU."""
import numpy as np
import pytest

import ba_graphs
from oracle import orc_ba
from reconstructor_amd import synth_ba


@pytest.mark.parametrize("name", list(ba_graphs.SCENES))
def test_every_scene_reaches_what_it_is_here_for(name):
    sc = ba_graphs.scene(name)
    ba_graphs.conditions(name, sc)
    P, I, X, s = orc_ba.solve(sc, threads=4)
    print(name, "observations", len(sc["obs_pt"]), "sum k^2", int((ba_graphs.track_lengths(sc) ** 2).sum()), "iterations", s["iterations"],
          "termination", s["termination"], "backtracks", s["line_search_backtracks"], "rms", s["initial_rms_px"], "->", s["final_rms_px"])
    assert s["termination"] == 1 and s["invalid_steps"] == 0 and s["unsuccessful_steps"] == 0
    assert s["final_rms_px"] < 0.8 < s["initial_rms_px"]
    nc = len(sc["poses"])
    assert s["reduced_dim"] == (6 * (nc - 1) - 3 if nc < 10 else 6 * (nc - 1) - 3 + 4 * nc)


def _few_cams(lengths):
    return ba_graphs.graph_scene(6, 120, 103, lengths, repeat=0.15)


FEW = {"ragged": (0, 1, 2, 3, 6), "two_and_more": (2, 2, 3, 6)}


def _scipy_minimum(sc, P, X):
    """scipy.optimize.least_squares from (P, X) over the oracle's gauge below 10 cameras -- camera 0 fixed, camera 1 rotation
    only, intrinsics constant -- with synth_ba.project as the residual; landmarks nobody observes are left out (they have no
    residual).  Returns the cost, 0.5 sum r^2."""
    from scipy.optimize import least_squares
    nc = len(P)
    seen = np.flatnonzero(np.bincount(sc["obs_pt"], minlength=len(X)) > 0)
    slot = np.full(len(X), -1)
    slot[seen] = np.arange(len(seen))
    mask = np.zeros((nc, 6), bool)
    mask[1:, :3] = True
    mask[2:, 3:] = True
    ncam = int(mask.sum())

    def fun(x):
        cam = np.array(P, copy=True)
        cam[mask] = x[:ncam]
        pts = x[ncam:].reshape(-1, 3)
        uv, _ = synth_ba.project(cam[sc["obs_cam"]], sc["intrinsics"][sc["obs_cam"]], pts[slot[sc["obs_pt"]]])
        return (uv - sc["obs_uv"]).ravel()

    r = least_squares(fun, np.concatenate([P[mask], X[seen].ravel()]), method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return float(r.cost)


@pytest.mark.parametrize("case", list(FEW))
def test_oracle_minimum_is_scipys_minimum(case):
    """Repeats, ragged tracks, unsorted tracks and distortion on six cameras: the oracle at its default options ends within the
    suite's 5e-6 of the minimum scipy finds (test_scene_traces_match_golden_and_scipy_minimum's figure), and run to a function
    tolerance of 1e-14 it ends AT it -- scipy, started there, gains less than 1e-9 relative (measured: 1e-15 and 4e-14; the default run 1e-7)."""
    sc = _few_cams(FEW[case])
    assert len(sc["poses"]) == 6 and ba_graphs.repeated_second(sc).any()
    P0, I0, X0, s0 = orc_ba.solve(sc, threads=2)
    o = orc_ba.default_options(6)
    o.function_tolerance = 1e-14
    o.max_iterations = 200
    P1, I1, X1, s1 = orc_ba.solve(sc, o, threads=2)
    assert s1["termination"] in (1, 2, 3, 4) and s1["iterations"] < 200
    cmin = _scipy_minimum(sc, P1, X1)
    tight, default = s1["final_cost"], s0["final_cost"]
    print(case, "scipy", cmin, "tight - scipy", (tight - cmin) / cmin, "default - scipy", (default - cmin) / cmin, "iterations", s0["iterations"], s1["iterations"])
    assert cmin <= tight * (1 + 1e-9)
    assert tight - cmin <= 1e-9 * cmin
    assert default - cmin <= 5e-6 * cmin


@pytest.mark.parametrize("case", list(FEW))
def test_a_repeated_observation_counts(case):
    """A camera seen twice by one landmark is two residuals: without the second of every such pair the solve ends elsewhere."""
    sc = _few_cams(FEW[case])
    rep = ba_graphs.repeated_second(sc)
    P0, I0, X0, s0 = orc_ba.solve(sc, threads=2)
    P1, I1, X1, s1 = orc_ba.solve(ba_graphs.select(sc, ~rep), threads=2)
    print(case, "repeats", int(rep.sum()), "rms", s0["final_rms_px"], "without", s1["final_rms_px"])
    assert rep.sum() >= 5 and abs(s1["final_rms_px"] - s0["final_rms_px"]) > 1e-4


def test_the_distortion_counts_and_unobserved_landmarks_stay():
    sc = _few_cams(FEW["ragged"])
    P0, I0, X0, s0 = orc_ba.solve(sc, threads=2)
    flat = ba_graphs.copy_scene(sc)
    flat["intrinsics"][:, 4:] = 0.0
    P1, I1, X1, s1 = orc_ba.solve(flat, threads=2)
    print("rms", s0["final_rms_px"], "with k1 = k2 = 0", s1["final_rms_px"])
    assert s0["final_rms_px"] < 0.7 and s1["final_rms_px"] > 1.0
    assert np.array_equal(I0, sc["intrinsics"])                       # below 10 cameras the intrinsics are constant
    k = ba_graphs.track_lengths(sc)
    assert (k == 0).sum() >= 10 and X0[k == 0].tobytes() == sc["points"][k == 0].tobytes()
    assert not np.array_equal(X0[k == 1], sc["points"][k == 1])


ORDER_BOUND = 1e-9


@pytest.mark.parametrize("name", list(ba_graphs.SCENES))
def test_order_inside_a_track_moves_the_oracle_by_rounding_only(name):
    """Three random orders inside the tracks, and the order sorted by camera: the same iterations, and cost trace and final RMS
    within 1e-9 relative (measured: below 1e-12) -- so the 1e-7 / 1e-5 px of the GPU suite leave a real error nowhere to hide."""
    sc = ba_graphs.scene(name)
    P0, I0, X0, s0 = orc_ba.solve(sc, threads=4)
    worst_trace = worst_rms = 0.0
    for how, seed in (("shuffle", 1), ("shuffle", 2), ("shuffle", 3), ("sort", 0)):
        sp = ba_graphs.reorder_tracks(sc, how, seed)
        assert np.array_equal(sp["pt_off"], sc["pt_off"]) and np.array_equal(np.sort(sp["obs_cam"]), np.sort(sc["obs_cam"]))
        P1, I1, X1, s1 = orc_ba.solve(sp, threads=4)
        assert (s1["iterations"], s1["termination"], s1["successful_steps"]) == (s0["iterations"], s0["termination"], s0["successful_steps"])
        worst_trace = max(worst_trace, float(np.abs(s1["cost_trace"] / s0["cost_trace"] - 1).max()))
        worst_rms = max(worst_rms, abs(s1["final_rms_px"] / s0["final_rms_px"] - 1))
    print(name, "order sensitivity of the oracle: cost trace %.2e  final rms %.2e (relative)" % (worst_trace, worst_rms))
    assert worst_trace < ORDER_BOUND and worst_rms < ORDER_BOUND
