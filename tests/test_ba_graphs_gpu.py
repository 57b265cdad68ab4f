"""GPU suite: bundle adjustment on the graph shapes synth_ba.make_scene never produces (tests/ba_graphs.py) -- tracks of 0, 1
and up to 41 observations in any order, a camera seen twice by one landmark, non-zero distortion with fx != fy, free cameras
whose rotation vector is zero, tiny or small -- against the CPU oracle at the tolerances of tests/test_ba_gpu.py (BASELINE.json
north_star: final RMS within 1e-5 px), against itself under a reordering of the tracks, through a session, and against the
diagnostic build's other list builder and other Schur build.  tests/test_ba_graphs_ref.py checks the oracle on the same scenes."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ba_graphs
from oracle import orc_ba
from reconstructor_amd import synth_ba

pytestmark = pytest.mark.gpu
RMS_TOL_PX = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_solves = {}


def _gpu(ctx, name):
    """The shipping library's solve of a named scene, once per session."""
    from reconstructor_amd import ba
    if name not in _solves:
        _solves[name] = ba.solve_scene(ctx, ba_graphs.scene(name))
    return _solves[name]


def _reproject(sc, P, I, X, obs):
    uv, _ = synth_ba.project(P[sc["obs_cam"][obs]], I[sc["obs_cam"][obs]], X[sc["obs_pt"][obs]])
    return uv


@pytest.mark.parametrize("name", list(ba_graphs.SCENES))
def test_graph_shapes_match_oracle(gpu_ctx, name):
    from reconstructor_amd import ba
    sc = ba_graphs.scene(name)
    ba_graphs.conditions(name, sc)
    P0, I0, X0, s0 = orc_ba.solve(sc, threads=4)
    P1, I1, X1, s1 = _gpu(gpu_ctx, name)
    nc = len(sc["poses"])
    k = ba_graphs.track_lengths(sc)
    n = min(len(s0["cost_trace"]), len(s1["cost_trace"]), 12)
    # a camera with one observation: its block has rank 2, the LM diagonal holds the rest -- compared by what it projects
    obs_per_cam = np.bincount(sc["obs_cam"], minlength=nc)
    held = obs_per_cam == 1
    assert held.any() == (name == "one_obs_camera")
    one = np.flatnonzero((k == 1)[sc["obs_pt"]] | held[sc["obs_cam"]])
    reproj = np.abs(_reproject(sc, P1, I1, X1, one) - _reproject(sc, P0, I0, X0, one)).max() if len(one) else 0.0
    # (a landmark whose only second observation is the held camera's keeps its other observations: it is compared in X too)
    dev_trace = np.abs(s1["cost_trace"][:n] / s0["cost_trace"][:n] - 1).max()
    print("%s: oracle %d iterations rms %.9f, gpu %d iterations rms %.9f | deviations: initial cost %.1e, cost trace %.1e, rms %.1e px, "
          "poses %.1e, intrinsics %.1e, points (k >= 2) %.1e, (k == 1: %.1e), reprojection of k == 1 %.1e px"
          % (name, s0["iterations"], s0["final_rms_px"], s1["iterations"], s1["final_rms_px"], abs(s1["initial_cost"] / s0["initial_cost"] - 1),
             dev_trace, abs(s1["final_rms_px"] - s0["final_rms_px"]), np.abs(P1 - P0)[~held].max(), np.abs(I1 - I0)[~held].max(),
             np.abs(X1 - X0)[k >= 2].max(), np.abs(X1 - X0)[k == 1].max(initial=0.0), reproj))
    assert abs(s1["initial_cost"] - s0["initial_cost"]) <= 1e-9 * s0["initial_cost"]
    for key in ("iterations", "termination", "successful_steps", "unsuccessful_steps", "invalid_steps", "line_search_backtracks", "reduced_dim"):
        assert s1[key] == s0[key], key
    assert np.allclose(s1["cost_trace"][:n], s0["cost_trace"][:n], rtol=1e-6 if s0["line_search_backtracks"] else 1e-7, atol=0)
    assert abs(s1["final_rms_px"] - s0["final_rms_px"]) <= RMS_TOL_PX
    assert np.allclose(P1[~held], P0[~held], rtol=0, atol=1e-6)
    assert np.allclose(I1[~held], I0[~held], rtol=1e-6, atol=1e-6)
    assert np.allclose(X1[k >= 2], X0[k >= 2], rtol=0, atol=1e-5)
    assert X1[k == 0].tobytes() == sc["points"][k == 0].tobytes()
    assert reproj <= 1e-5
    # again: the same bits (the second solve finds the pair lists of the first)
    P2, I2, X2, s2 = ba.solve_scene(gpu_ctx, sc)
    assert P2.tobytes() == P1.tobytes() and I2.tobytes() == I1.tobytes() and X2.tobytes() == X1.tobytes()
    assert np.array_equal(s2["cost_trace"], s1["cost_trace"])


@pytest.mark.parametrize("how", ["shuffle", "sort"])
def test_order_inside_a_track_changes_rounding_only(gpu_ctx, how):
    """No oracle needed: the observations of every track in another order (pt_off unchanged) are the same problem, summed in
    another order.  The bound is the one the CPU tier asserts for the oracle itself."""
    from reconstructor_amd import ba
    sc = ba_graphs.scene("long_general")
    P1, I1, X1, s1 = _gpu(gpu_ctx, "long_general")
    sp = ba_graphs.reorder_tracks(sc, how, seed=5)
    assert not np.array_equal(sp["obs_cam"], sc["obs_cam"]) and np.array_equal(sp["obs_pt"], sc["obs_pt"])
    P2, I2, X2, s2 = ba.solve_scene(gpu_ctx, sp)
    dev = np.abs(s2["cost_trace"] / s1["cost_trace"] - 1).max() if len(s2["cost_trace"]) == len(s1["cost_trace"]) else np.inf
    print("long_general, tracks in another order (%s): cost trace moves by %.1e relative, poses by %.1e" % (how, dev, np.abs(P2 - P1).max()))
    for key in ("iterations", "termination", "successful_steps", "unsuccessful_steps", "invalid_steps", "reduced_dim"):
        assert s2[key] == s1[key], key
    assert dev <= 1e-9


@pytest.mark.parametrize("name", ["few_cams", "long_small"])
def test_session_keeps_repeats_and_insertion_order(gpu_ctx, name):
    """The observations reach a session in two calls that each carry a random part of the list: tracks are split across the
    calls, a landmark's camera may come twice in one call or once in each.  The session's own flattening, solved by
    rcn_ba_solve, and the session's solve give the same bits."""
    from reconstructor_amd import ba
    sc = ba_graphs.scene(name)
    nc, no = len(sc["poses"]), len(sc["obs_pt"])
    first = np.random.default_rng(17).random(no) < 0.5
    xy = sc["obs_uv"].astype(np.int32)
    ses = ba.BaSession(gpu_ctx)
    try:
        for c in range(nc):
            ses.add_camera(sc["poses"][c], sc["intrinsics"][c])
        ses.add_points(sc["points"])
        for part in (first, ~first):
            ses.add_observations(sc["obs_pt"][part], sc["obs_cam"][part], xy[part])
        pt, cam, xy2 = ses.graph()
        assert ses.counts() == (nc, len(sc["points"]), no) and (np.diff(pt) >= 0).all()
        # per track: the first call's observations in their order, then the second call's
        order = np.lexsort((np.arange(no), ~first, sc["obs_pt"]))
        assert np.array_equal(pt, sc["obs_pt"][order]) and np.array_equal(cam, sc["obs_cam"][order]) and np.array_equal(xy2, xy[order])
        assert not np.array_equal(cam, sc["obs_cam"])
        poses, intr = ses.cameras()
        flat = {"poses": poses, "intrinsics": intr, "points": ses.points(), "obs_uv": xy2.astype(np.float64), "obs_cam": cam, "obs_pt": pt}
        assert ba_graphs.repeated_second(flat).sum() == ba_graphs.repeated_second(sc).sum() > 0
        P1, I1, X1, s1 = ba.solve_scene(gpu_ctx, flat)
        s2 = ses.solve()
        P2, I2 = ses.cameras()
        X2 = ses.points()
        assert P2.tobytes() == P1.tobytes() and I2.tobytes() == I1.tobytes() and X2.tobytes() == X1.tobytes()
        assert s2["iterations"] == s1["iterations"] and np.array_equal(s2["cost_trace"], s1["cost_trace"])
        P0, I0, X0, s0 = orc_ba.solve(flat, threads=4)
        assert s2["iterations"] == s0["iterations"] and abs(s2["final_rms_px"] - s0["final_rms_px"]) <= RMS_TOL_PX
    finally:
        ses.close()


ALT_SCENES = ("long_small", "few_cams", "edge_256", "sees_all")


def _digest(P, I, X, s):
    return hashlib.sha256(P.tobytes() + I.tobytes() + X.tobytes() + repr((int(s["iterations"]), int(s["termination"]), float(s["final_cost"]))).encode()).hexdigest()


_ALT = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import ba_graphs
from reconstructor_amd import _lib, ba
assert b"DIAGNOSTIC" in _lib.load().rcn_version()
ctx = _lib.Context(0)
out = {}
for name in %r:
    P, I, X, s = ba.solve_scene(ctx, ba_graphs.scene(name))
    out.update({name + "/P": P, name + "/I": I, name + "/X": X, name + "/it": s["iterations"], name + "/term": s["termination"],
                name + "/cost": s["final_cost"], name + "/rms": s["final_rms_px"]})
np.savez(sys.argv[1], **out)
"""


def _alternative(env, tmp_path):
    diag = os.path.join(ROOT, "tools", "librcn_diag.so")
    assert os.path.exists(diag), "tools/librcn_diag.so missing: run __graft_entry__.build()"
    out = str(tmp_path / "alt.npz")
    r = subprocess.run([sys.executable, "-c", _ALT % (ROOT, os.path.join(ROOT, "tests"), ALT_SCENES), out],
                       env=dict(os.environ, RCN_LIB=diag, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    return {name: (z[name + "/P"], z[name + "/I"], z[name + "/X"],
                   {"iterations": int(z[name + "/it"]), "termination": int(z[name + "/term"]), "final_cost": float(z[name + "/cost"]),
                    "final_rms_px": float(z[name + "/rms"])}) for name in ALT_SCENES}


def test_the_six_launch_list_builder_gives_the_one_workgroup_builders_bits(gpu_ctx, tmp_path):
    """long_small and few_cams take the one-workgroup list builder (k_pair_small) in the shipping library -- landmarks of up to
    26 x 26 pairs shared out over a few threads each; with RCN_PAIR_SMALL=0 the diagnostic build counts, scans and fills in six
    launches, a workgroup per landmark walking k * k > 256 pairs in several trips.  The lists are sorted behind either: the
    same bits.  (edge_256 and sees_all take the six launches in both; they pin the diagnostic build to the shipping one.)"""
    for name in ("long_small", "few_cams"):
        sc = ba_graphs.scene(name)
        assert len(sc["poses"]) ** 2 <= 1024 and (ba_graphs.track_lengths(sc) ** 2).sum() <= 16384
    alt = _alternative({"RCN_PAIR_SMALL": "0"}, tmp_path)
    for name in ALT_SCENES:
        assert _digest(*alt[name]) == _digest(*_gpu(gpu_ctx, name)), name


def test_the_atomic_schur_build_lands_where_the_gather_lists_do(gpu_ctx, tmp_path):
    """RCN_BA_SCHUR_ATOMICS=1: a workgroup per landmark (its size taken from kmax * kmax) adds every pair's block with float
    atomics, the repeated camera's diagonal terms among them -- no lists at all.  Same iterations, and the optimum to the
    figures of test_alternative_device_paths_agree."""
    alt = _alternative({"RCN_BA_SCHUR_ATOMICS": "1"}, tmp_path)
    for name in ALT_SCENES:
        P0, I0, X0, s0 = _gpu(gpu_ctx, name)
        P, I, X, s = alt[name]
        k = ba_graphs.track_lengths(ba_graphs.scene(name))
        print("%s, atomic Schur build: rms differs by %.1e px, poses by %.1e, points by %.1e (k == 1: %.1e)"
              % (name, abs(s["final_rms_px"] - s0["final_rms_px"]), np.abs(P - P0).max(), np.abs(X - X0).max(), np.abs(X - X0)[k == 1].max(initial=0.0)))
        assert s["iterations"] == s0["iterations"] and s["termination"] == s0["termination"]
        assert abs(s["final_rms_px"] - s0["final_rms_px"]) < 1e-9
        assert np.allclose(P, P0, rtol=0, atol=1e-8)
        assert np.allclose(X, X0, rtol=0, atol=1e-7)
